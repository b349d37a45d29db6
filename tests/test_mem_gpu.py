"""GPU tests of the grow-only buffers behind a handle (csrc/bp_mem.h: Buf, grow_all; -m gpu): grow, then reuse.

Each test makes a small call (A), a large call (B) and the small call again on ONE handle; every result must equal, bit for bit,
the same call on a fresh handle that made only that call.  A holder that frees early, or a pointer that survives a regrow, shows
as other bits (or as a fault: then the cause is in the code, not in a second run).

Geometry: the smallest the signal layer accepts, fea_dim D = 33 (hop 32, n_fft 64), context 3, the net [3*33, 64, 33] with
bunchsize 32 and max_chunk_frames 1200 (ld_L = 64).  A buffer that holds `a` bytes after A has the capacity a + a/4 + 4096
(csrc/bp_mem.h), so B must ask for more than that; out_chunk holds n + n/4 + 64 frames.  T = (len - 1) // hop + 2 frames per
sentence, padded = (frames + n_sent) * hop samples.

  enhance_waves   A = 1 sentence of 5 hop = 160 samples: 6 frames, 224 padded samples, 8 staged rows
                  B = 3 sentences of 200 hop = 6400 samples: 603 frames, 19392 padded samples, 609 staged rows
      input block (device and pinned)   2560 B -> capacity  7296;  B asks  79104
      spectrum    frames * 33 * 8       1584 B -> capacity  6076;  B asks 159192
      synthesis   frames * 64 * 4       1536 B -> capacity  6016;  B asks 154368
      samples (device and pinned)        896 B -> capacity  5216;  B asks  77568
      out_chunk / host_out                 6 frames -> capacity 71; B asks    603
  mixtures        A = the plan of one clean sentence of 160 samples (6 frames, 7 segments)
                  B = the plan of three clean sentences of 389 hop = 12448 samples (390 frames each: 1170 frames, 1173 segments,
                      1176 rows of the 1200).  Three sentences of 200 hop fall short for the input block: it holds six tables of
                      n_mix entries (256 B each for n_mix <= 63) and 4 bytes per frame, 1792 B -> capacity 6336 after A, and B
                      asks 1536 + al256(4 * frames) = 6400 only from 1153 frames on.
      input block (device, pinned 0 and 1)   1792 B -> capacity  6336;  B asks   6400
      x, s, v, enhanced samples segs*32*4     896 B -> capacity  5216;  B asks 150144
      noisy LPS   frames * 33 * 4             792 B -> capacity  5086;  B asks 154440
      spectrum / synthesis frames            1584, 1536 B as above;      B asks 308880, 299520
      the two LPS blocks 2 al256(frames*132) 2048 B -> capacity  6656;  B asks 309248
      work block: 12 bytes per sample resampled to 10 kHz and more (200 against 46680 samples)
      out_chunk / host_out                      6 frames -> capacity 71; B asks 1170
      (the gains, 4 bytes per mixture, and the score tables scale with n_mix alone and do not grow here)
  windows         8 against 400 samples of 10 and 402 frames: frames 1320 B -> capacity 5746, B asks 53064 (targets the same);
                  tables 96 B -> capacity 4216, B asks 4800.  The staging sets alternate, so A, B, A allocates set 1, set 0 and
                  reuses set 1; B, B, A behind them reuses set 0, regrows set 1 from small to large and reuses set 0.
  forward         8 against 200 frames: out_chunk capacity 74 frames after A."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D, HOP, CTX, TOFF, B, CAP, FS = 33, 32, 3, 1, 32, 1200, 8000
LS = [CTX * D, 64, D]


def _handle(pkg):
    W, b = pkg.glorot_net(LS, seed=5, beta=0.5)
    return pkg.BP_GPU(1, 3, LS, B, 0.05, 0.5, 0.0, W, b, max_chunk_frames=CAP)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(x, y):
    """bit-equal: arrays, scalars, None, and lists / dicts of them"""
    if isinstance(x, dict):
        return isinstance(y, dict) and x.keys() == y.keys() and all(_same(x[k], y[k]) for k in x)
    if isinstance(x, (list, tuple)):
        return isinstance(y, (list, tuple)) and len(x) == len(y) and all(_same(a, b) for a, b in zip(x, y))
    if x is None or y is None:
        return x is None and y is None
    return np.shape(x) == np.shape(y) and np.array_equal(_bits(x), _bits(y))


def _fresh(pkg, call):
    g = _handle(pkg)
    try:
        return call(g)
    finally:
        g.close()


def _grow_then_reuse(pkg, calls, sequence):
    """calls: {name: f(handle)}; every call of the sequence on one handle equals the same call alone on a fresh handle"""
    ref = {k: _fresh(pkg, f) for k, f in calls.items()}
    assert not _same(ref["A"], ref["B"])
    g = _handle(pkg)
    try:
        for i, k in enumerate(sequence):
            assert _same(calls[k](g), ref[k]), (i, k, sequence)
    finally:
        g.close()


def _sentences(rng, lens):
    return [np.round(rng.normal(0, 3000, n)).astype(np.float32) for n in lens]


def test_enhance_waves_grow_then_reuse(pkg):
    rng = np.random.default_rng(31)
    mean, istd = rng.normal(10.0, 2.0, D).astype(np.float32), rng.uniform(0.2, 0.5, D).astype(np.float32)
    xa, xb = _sentences(rng, [5 * HOP]), _sentences(rng, [200 * HOP] * 3)
    calls = {"A": lambda g: g.enhance_waves(xa, mean, istd, CTX, TOFF, return_net=True),
             "B": lambda g: g.enhance_waves(xb, mean, istd, CTX, TOFF, return_net=True)}
    _grow_then_reuse(pkg, calls, "ABA")


def test_mix_and_eval_grow_then_reuse(pkg):
    rng = np.random.default_rng(32)
    mean, istd = rng.normal(10.0, 2.0, D).astype(np.float32), rng.uniform(0.2, 0.5, D).astype(np.float32)
    clean = _sentences(rng, [5 * HOP] + [389 * HOP] * 3)
    noise = [np.round(rng.normal(0, 800, 9000)).astype(np.float32)]
    plans = {}
    for k, mixes in (("A", [(0, 0, 17, 5.0)]), ("B", [(1, 0, 11, 0.0), (2, 0, 3000, 5.0), (3, 0, 8999, 10.0)])):
        plans[k] = np.zeros(len(mixes), pkg.MIXTURE_DTYPE)
        for i, m in enumerate(mixes):
            plans[k][i] = m

    def call(g, k):
        if getattr(g, "mix_fea_dim", None) is None:              # (once per handle; a fresh handle makes it and the one call)
            g.set_mix_corpus(clean, noise, mean, istd, CTX, TOFF, "lps")
        return g.mix_features(plans[k]), g.eval_mix(plans[k], FS, return_pcm=True)

    calls = {"A": lambda g: call(g, "A"), "B": lambda g: call(g, "B")}
    _grow_then_reuse(pkg, calls, "ABA")


def test_cv_windows_grow_then_reuse(pkg):
    rng = np.random.default_rng(33)

    def chunk(n):
        fea = rng.normal(size=(n + CTX - 1, D)).astype(np.float32)
        tg = rng.normal(size=(n + CTX - 1, LS[-1])).astype(np.float32)
        return fea, tg, CTX, np.arange(n, dtype=np.int32), np.arange(n, dtype=np.int32) + TOFF

    ca, cb = chunk(8), chunk(400)
    calls = {"A": lambda g: g.CrossValid_windows(*ca), "B": lambda g: g.CrossValid_windows(*cb)}
    _grow_then_reuse(pkg, calls, "ABABBA")                       # (A, B, A; then a set that regrows, see above)


def test_forward_grow_then_reuse(pkg):
    rng = np.random.default_rng(34)
    xa, xb = rng.normal(size=(8, LS[0])).astype(np.float32), rng.normal(size=(200, LS[0])).astype(np.float32)
    calls = {"A": lambda g: g.forward(xa), "B": lambda g: g.forward(xb)}
    _grow_then_reuse(pkg, calls, "ABA")
