"""GPU tests of the sample-rate converter (bp_resample_waves and the rate= key of the tools; -m gpu): the device's output equals,
bit for bit, the float64 restatement in tests/resample_np.py fed the library's own taps.

The kernel (bp_wave_resample) gives every output sample to one lane of a workgroup of 256 consecutive samples of a
sentence.  Its paths, and the cases below that reach them:
  LDS span         the workgroup's input span staged in LDS: every case but `1/1024`
  global fallback  the span does not fit LDS (255 q + 2 Lh > 16000 p): `1/1024` with zeros = 32, where one output reads 65 537 taps
  last partial block  a sentence whose n_out is no multiple of 256: the sentences of 1, 2 and 7 samples of every case, and the long
                   sentence of every case (its n_out is chosen off the multiple; at 1024/1 every n_out is a multiple of 256 and
                   the 164 workgroups of the long sentence are all full), which also crosses several workgroups
"""
import subprocess

import numpy as np
import pytest

import resample_np as RS
import wave_np as WN

pytestmark = pytest.mark.gpu

# name -> (rate_in, rate_out, (zeros, beta, rolloff)); rate_out / rate_in is the p/q of the name
CASES = {
    "1/2": (16000, 8000, RS.DEFAULTS), "2/1": (8000, 16000, RS.DEFAULTS), "3/2": (2, 3, RS.DEFAULTS), "2/3": (3, 2, RS.DEFAULTS),
    "160/441": (44100, 16000, RS.DEFAULTS), "800/999": (19980, 16000, RS.DEFAULTS),
    "1/1024": (1024, 1, (32, 8.6, 0.9)), "1024/1": (1, 1024, (1, 8.6, 0.9)), "3/2 other parameters": (2, 3, (5, 3.0, 1.0)),
}
_memo = {}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _case(pkg, name):
    """The sentences of a case, the device's output for them in one call and the restatement's; made once."""
    if name in _memo:
        return _memo[name]
    rate_in, rate_out, prm = CASES[name]
    p, q = pkg.resample_ratio(rate_in, rate_out)
    assert "%d/%d" % (p, q) == name.split()[0]
    rng = np.random.default_rng(sum(map(ord, name)))
    # the long sentence: about 2.7 workgroups of output (1/1024: 1.2, 1024/1: one sample more than 160), n p / q not whole where q > 1
    long_n = {"1/1024": 300 * 1024 + 5, "1024/1": 41}.get(name, (700 * q) // p + 1)
    if q > 1 and (long_n * p) % q == 0:
        long_n += 1
    # 1 sample; 2 samples; shorter than one tap span (2 Lh / p samples; at 1024/1 that is the sentence of 1); n p / q whole; the long one
    lens = [long_n, 1, 2 * q, 2, 7]
    h = pkg.resample_taps(p, q, prm)
    assert 7 < 2 * prm[0] * max(p, q) / p or name == "1024/1"
    assert RS.length(long_n, p, q) > 256 and (RS.length(long_n, p, q) % 256 != 0 or p % 256 == 0)
    xs = [np.round(rng.standard_normal(n) * 3000).astype(np.float32) for n in lens]
    got = pkg.resample_waves(0, rate_in, rate_out, xs, prm)
    ref = [RS.resample(x, p, q, h) for x in xs]
    _memo[name] = (rate_in, rate_out, prm, p, q, xs, got, ref)
    return _memo[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_bits_equal_restatement(pkg, name):
    rate_in, rate_out, prm, p, q, xs, got, ref = _case(pkg, name)
    assert len(got) == len(xs)
    for s, (x, g, r) in enumerate(zip(xs, got, ref)):
        assert g.size == RS.length(x.size, p, q) == pkg.resample_len(x.size, p, q), (name, s)
        assert np.array_equal(_bits(g), _bits(r)), (name, s, x.size, int((_bits(g) != _bits(r)).sum()), float(np.abs(g - r).max()))
    assert float(max(np.abs(g).max() for g in got)) > 100.0          # (the output is a signal, not zeros)


@pytest.mark.parametrize("name", sorted(CASES))
def test_alone_as_in_company_and_twice(pkg, name):
    rate_in, rate_out, prm, p, q, xs, got, ref = _case(pkg, name)
    for s, x in enumerate(xs):
        alone = pkg.resample_waves(0, rate_in, rate_out, [x], prm)
        assert len(alone) == 1 and np.array_equal(_bits(alone[0]), _bits(got[s])), (name, s)
    again = pkg.resample_waves(0, rate_in, rate_out, xs, prm)
    assert all(np.array_equal(_bits(a), _bits(g)) for a, g in zip(again, got)), name
    back = pkg.resample_waves(0, rate_in, rate_out, xs[::-1], prm)[::-1]
    assert all(np.array_equal(_bits(a), _bits(g)) for a, g in zip(back, got)), name


def test_equal_rates_return_the_input(pkg):
    rng = np.random.default_rng(3)
    xs = [rng.standard_normal(n).astype(np.float32) for n in (1, 300, 17)]
    ys = pkg.resample_waves(0, 44100, 44100, xs, (3, 1.0, 0.5))
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(xs, ys))


# ---- the tools end to end, by bits
def _write_pcm16(path, x, rate):
    import wave
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(rate)
        w.writeframes(np.asarray(x, np.int16).tobytes())


def _read_pcm16(path):
    import wave
    with wave.open(str(path), "rb") as w:
        assert w.getnchannels() == 1 and w.getsampwidth() == 2
        return np.frombuffer(w.readframes(w.getnframes()), np.int16), w.getframerate()


def _read_pfile(path, dim):
    raw = open(path, "rb").read()
    hdr = raw[:32768].split(b"\0")[0].decode()
    ns = int(hdr.split("-num_sentences")[1].split()[0]); nf = int(hdr.split("-num_frames")[1].split()[0])
    rec = np.frombuffer(raw, ">u4", nf * (2 + dim), 32768).reshape(nf, 2 + dim)
    table = np.frombuffer(raw, ">i4", ns + 1, 32768 + nf * (2 + dim) * 4)
    return rec[:, 2:].astype("<u4").view("<f4"), table


def _ints(rng, n, s):
    return np.clip(np.round(rng.normal(0, s, n)), -32768, 32767).astype(np.float32)


def _exe(pkg, tool):
    return str(pkg.LIB_PATH).replace("libbp_hip.so", tool)


def _list(d, tag, xs, rates):
    for i, (x, r) in enumerate(zip(xs, rates)):
        _write_pcm16(d / ("%s%d.wav" % (tag, i)), x, r)
    (d / (tag + ".list")).write_text("".join("%s\n" % (d / ("%s%d.wav" % (tag, i))) for i in range(len(xs))))
    return str(d / (tag + ".list"))


def test_bpfeat_rate(pkg, tmp_path):
    D = 65
    rng = np.random.default_rng(21)
    xs = [_ints(rng, n, 3000) for n in (3001, 700, 1200, 1)]
    rates = [16000, 8000, 16000, 16000]
    lst = _list(tmp_path, "x", xs, rates)
    r = subprocess.run([_exe(pkg, "bpfeat"), "wav_list=" + lst, "out_file=%s" % (tmp_path / "x.pfile"), "fea_dim=%d" % D, "rate=8000"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 1, r.stdout + r.stderr
    assert r.stdout.count("converted from") == 1 and "3 recordings converted from 16000 Hz to 8000 Hz" in r.stdout, r.stdout
    conv = pkg.resample_waves(0, 16000, 8000, [xs[0], xs[2], xs[3]])
    at8 = [conv[0], xs[1], conv[1], conv[2]]
    ref = pkg.wave_lps(0, D, at8)
    fea, table = _read_pfile(tmp_path / "x.pfile", D)
    assert list(np.diff(table)) == [a.shape[0] for a in ref]
    assert np.array_equal(_bits(fea), _bits(np.concatenate(ref)))


def test_bpenhance_rate(pkg, tmp_path):
    import pfile_util as PU
    D, ctx, toff, B, cap = 65, 3, 1, 32, 2000
    rng = np.random.default_rng(22)
    x = _ints(rng, 5001, 3000)
    _write_pcm16(tmp_path / "in.wav", x, 16000)
    mean, istd = np.full(D, 9.0, np.float32), np.full(D, 0.25, np.float32)
    # a net near the identity (the centre frame's LPS, 0.5 lower, through slightly perturbed weights): audible output, every layer at work
    ls, W, b = WN.identity_net(D, ctx, toff, False, mean, istd)
    W[1] = (W[1] + rng.normal(0, 0.002, W[1].shape)).astype(np.float32)
    b[2] = (b[2] - 0.5).astype(np.float32)
    PU.write_wts(str(tmp_path / "net.wts"), ls, W, b)
    PU.write_norm(str(tmp_path / "x.norm"), mean, istd)
    r = subprocess.run([_exe(pkg, "bpenhance"), "norm_file=%s" % (tmp_path / "x.norm"), "initwts_file=%s" % (tmp_path / "net.wts"),
                        "layersizes=%s" % ",".join(map(str, ls)), "fea_dim=%d" % D, "fea_context=%d" % ctx, "targ_offset=%d" % toff,
                        "in_wav=%s" % (tmp_path / "in.wav"), "out_wav=%s" % (tmp_path / "out.wav"), "traincache=%d" % cap, "bunchsize=%d" % B,
                        "rate=8000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1, r.stdout + r.stderr
    assert "from 16000 Hz to 8000 Hz" in r.stdout and "from 8000 Hz to 16000 Hz" in r.stdout, r.stdout
    # the Python chain: resample -> enhance_waves -> resample back -> trim -> PCM16
    x8 = pkg.resample_waves(0, 16000, 8000, [x])
    g = pkg.BP_GPU(1, 3, ls, B, 0.0, 0.0, 0.0, W, b, max_chunk_frames=cap)
    try:
        e8 = g.enhance_waves(x8, mean, istd, ctx, toff)
    finally:
        g.close()
    e16 = pkg.resample_waves(0, 8000, 16000, e8)[0]
    assert e16.size >= x.size
    want = np.clip(np.rint(e16[:x.size]), -32768, 32767).astype(np.int16)
    y, rate = _read_pcm16(tmp_path / "out.wav")
    assert rate == 16000 and y.size == x.size
    assert np.array_equal(y, want), int((y != want).sum())
    assert int(np.abs(want.astype(np.int32)).max()) > 1000          # (a signal came out)


def _cut(frames, ctx, cap):
    calls, first, rows = [], 0, 0
    for m, T in enumerate(frames):
        if rows + T + ctx - 1 > cap:
            calls.append((first, m)); first, rows = m, 0
        rows += T + ctx - 1
    return calls + [(first, len(frames))]


def test_bpmix_rate(pkg, tmp_path):
    import pfile_util as PU
    D, ctx, toff, B, cap, seed = 65, 3, 1, 32, 200, 77
    rng = np.random.default_rng(23)
    clean = [_ints(rng, n, 3000) for n in (1500, 400, 2200, 900)]
    noise16 = [_ints(rng, 9001, 1500)]
    lists = ["clean_list=" + _list(tmp_path, "clean", clean, [8000] * 4), "noise_list=" + _list(tmp_path, "noise", noise16, [16000]),
             "cv_clean_list=%s" % (tmp_path / "clean.list")]
    ls = [ctx * D, 64, D]
    W, b = pkg.glorot_net(ls, seed=5, beta=0.5)
    PU.write_wts(str(tmp_path / "init.wts"), ls, W, b)
    mean, istd = np.full(D, 9.0, np.float32), np.full(D, 0.25, np.float32)
    PU.write_norm(str(tmp_path / "mix.norm"), mean, istd)
    r = subprocess.run([_exe(pkg, "bpmix")] + lists + [
        "fea_dim=%d" % D, "snr_list=0,10", "init_randem_seed=%d" % seed, "traincache=%d" % cap, "norm_file=%s" % (tmp_path / "mix.norm"),
        "fea_context=%d" % ctx, "targ_offset=%d" % toff, "numlayers=3", "layersizes=%s" % ",".join(map(str, ls)), "bunchsize=%d" % B,
        "lrate=0.01", "momentum=0.5", "weightcost=0.0001", "initwts_file=%s" % (tmp_path / "init.wts"), "rate=8000",
        "outwts_file=%s" % (tmp_path / "out.wts"), "log_file=%s" % (tmp_path / "out.log")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "all finish!" in r.stdout, r.stdout + r.stderr
    assert r.stdout.count("converted from") == 1 and "bpmix: noise_list: 1 recording converted from 16000 Hz to 8000 Hz" in r.stdout, r.stdout
    # the same epoch through the Python API on the noise resampled in Python: the same plan, the same seed
    noise8 = pkg.resample_waves(0, 16000, 8000, noise16)
    plan = pkg.mix_plan(seed, len(clean), 1, [x.size for x in noise8], [0.0, 10.0])
    g = pkg.BP_GPU(1, 3, ls, B, 0.01, 0.5, 1e-4, W, b, max_chunk_frames=cap)
    try:
        g.set_mix_corpus(clean, noise8, mean, istd, ctx, toff, "lps", 5.0)
        calls = _cut(g.mix_frames(plan), ctx, cap)
        for k, (a, e) in enumerate(calls):
            g.train_mix(plan[a:e], pkg.mix_shuffle(seed, k, int(g.mix_frames(plan[a:e]).sum())))
        Wp, bp = g.get_weights()
    finally:
        g.close()
    PU.write_wts(str(tmp_path / "py.wts"), ls, Wp, bp)
    assert (tmp_path / "py.wts").read_bytes() == (tmp_path / "out.wts").read_bytes()
    assert (tmp_path / "py.wts").read_bytes() != (tmp_path / "init.wts").read_bytes()
