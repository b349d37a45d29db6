"""GPU tests of the signal layer at every frame size it accepts (-m gpu): fea_dim 33, 65, 129, 257, 513 and 1025, against the
float64 restatement in tests/wave_np.py.  tests/geometry_cases.py holds the sizes, the sentences and the table that says which
test holds which entry point at which size; the cases whose body an older file already had were added to that file's
parametrize list instead (analysis, streams, mixtures, log-MMSE).

Bars, the same at every size (tests/test_wave_f32_host.py derives that from the restatement alone): resynthesis 1e-5 of the
sentence's largest sample, the all-zero frames 1e-5 of their own segment's largest sample, the net outputs util.TOL; the scores
the four bars of tests/test_eval_gpu.py; eval_mix bit for bit.

The sentences of a size (geometry_cases.sentences): 1, hop - 1, hop, hop + 1, n_fft - 1, 5 hop + 7 and 12 hop + 3 samples, 33 frames
in all: two bunches of 16 and a partial one.  Samples [3 hop, 7 hop) of the last are zero, so its frames 4, 5 and 6 are all-zero:
in LPS mode the noisy bin there has no phase and synth_frame takes its unit-phase branch; in mask mode the output is exactly 0.

Measured (profiles/geometry_parity_numbers.json): resynthesis 1.6e-7 .. 3.6e-7, the all-zero frames 2.5e-7 .. 7.3e-7, identity
6.2e-7 .. 9.7e-7; net outputs 3.8e-7 .. 6.6e-7 except at fea_dim 65, where they are 5.7e-6 (LPS net) and 9.4e-6 (mask net): one
bin of that size's sentences carries 2.6e-4 of its frame's largest magnitude, its LPS feature is correspondingly rough in fp32,
and the float32 restatement of tests/test_wave_f32_host.py fed through the same net differs from float64 by 5.7e-6 as well."""
import numpy as np
import pytest

import eval_np as EN
import geometry_cases as GC
import test_eval_gpu as TE
import wave_np as WN
from util import TOL, relerr

pytestmark = pytest.mark.gpu

BAR = GC.WAVE_BAR
CTX, TOFF = GC.CTX, GC.TOFF
_CASES = {}


def _case(D):
    """The sentences of a size, their restated spectra and norm statistics: computed once, shared, read-only."""
    if D not in _CASES:
        xs = GC.sentences(D)
        Y = [WN.analysis(x, D) for x in xs]
        m, i = WN.norm_stats(xs, D)
        c = dict(xs=xs, Y=Y, m=m.astype(np.float32), i=i.astype(np.float32))
        for a in xs + Y + [c["m"], c["i"]]:
            a.setflags(write=False)
        _CASES[D] = c
    return _CASES[D]


def _wave_err(y, ref):
    return float(np.abs(np.asarray(y, np.float64) - ref).max() / np.abs(ref).max())


# ---- 1. resynthesis, both targets
@pytest.mark.parametrize("D", GC.FEA_DIMS)
@pytest.mark.parametrize("target", ["lps", "mask"])
def test_resynthesis_matches_restatement(pkg, target, D, parity_record):
    c = _case(D)
    xs, m, i = c["xs"], c["m"], c["i"]
    mask = target == "mask"
    ls = GC.net_sizes(D, target)
    W, b = pkg.glorot_net(ls, seed=5, beta=0.5)
    hkw = dict(output_activation=1, output_linear_cols=D) if mask else {}
    code, out_col = (pkg.WAVE_MASK, D) if mask else (pkg.WAVE_LPS, 0)
    g = pkg.BP_GPU(1, len(ls), ls, GC.BUNCH, 0.0, 0.0, 0.0, W, b, max_chunk_frames=256, **hkw)
    try:
        got, net = g.enhance_waves(xs, m, i, CTX, TOFF, target=code, out_col=out_col, return_net=True)
    finally:
        g.close()
    assert [y.size for y in got] == [x.size for x in xs]
    assert sum(o.shape[0] for o in net) % GC.BUNCH != 0 and sum(o.shape[0] for o in net) > 2 * GC.BUNCH
    e_net = e_wave = 0.0
    for x, Y, y, o in zip(xs, c["Y"], got, net):
        assert o.shape == (Y.shape[0], ls[-1]) and np.isfinite(y).all()
        z = (WN.lps(Y) - m.astype(np.float64)) * i.astype(np.float64)
        want = WN.forward(W, b, WN.stack(z, CTX, TOFF, True), out_act=int(mask), out_lin=D)
        for lo in range(0, ls[-1], D):                          # (each block against its own largest value)
            e_net = max(e_net, relerr(o[:, lo:lo + D], want[:, lo:lo + D]))
        if mask:
            assert 0.0 < o[:, D:].min() and o[:, D:].max() < 1.0
        ref = WN.resynth(Y, o[:, out_col:out_col + D], code, x.size)
        e_wave = max(e_wave, _wave_err(y, ref))
    # the all-zero frames of the last sentence (y, ref and Y are its)
    zf = GC.zero_frames(Y)
    assert len(zf) >= 2, zf
    lo, hi = GC.zero_segment(D, zf)
    assert hi - lo >= D - 1
    rec = dict(fea_dim=D, out_net_relerr=e_net, wave_err=e_wave, zero_frames=len(zf))
    if mask:
        assert not y[lo:hi].any() and not ref[lo:hi].any(), "mask x 0: exact zeros"
    else:
        assert np.abs(ref[lo:hi]).max() > 0 and y[lo:hi].any(), "unit phase where the noisy bin is zero: the segment is not silent"
        rec["zero_frames_err"] = float(np.abs(y[lo:hi] - ref[lo:hi]).max() / np.abs(ref[lo:hi]).max())
    print("fea_dim %d %s: %s" % (D, target, rec))
    parity_record(**rec)
    assert e_net <= TOL, e_net
    assert e_wave <= BAR, e_wave
    if not mask:
        assert rec["zero_frames_err"] <= BAR, rec["zero_frames_err"]


# ---- 2. identity round trip
@pytest.mark.parametrize("D", GC.FEA_DIMS)
def test_identity_round_trip(pkg, D, parity_record):
    c = _case(D)
    xs, m, i = c["xs"], c["m"], c["i"]
    ls, W, b = WN.identity_net(D, 1, 0, False, m, i)
    g = pkg.BP_GPU(1, len(ls), ls, GC.BUNCH, 0.0, 0.0, 0.0, W, b, max_chunk_frames=256)
    try:
        got = g.enhance_waves(xs, m, i, 1, 0)
    finally:
        g.close()
    assert [y.size for y in got] == [x.size for x in xs]
    err = max(_wave_err(y, x.astype(np.float64)) for y, x in zip(got, xs))
    print("fea_dim %d identity: %.3g" % (D, err))
    parity_record(fea_dim=D, max_rel_wave_err=err)
    assert err <= BAR, err


# ---- 3. scores (the LSD part depends on the frame size; 129 and 257 run in tests/test_eval_gpu.py)
@pytest.mark.parametrize("D", [33, 65, 513, 1025])
def test_scores_match_restatement(pkg, D, parity_record):
    TE.score_case(pkg, 16000, D, parity_record)


# ---- 4. eval_mix is its parts (129 runs in tests/test_eval_gpu.py)
FS = 8000


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("D", [33, 65, 257, 513, 1025])
def test_eval_mix_is_its_parts(pkg, D, parity_record):
    rng = np.random.default_rng(300 + D)
    clean = [np.round(EN.speech_like(rng, n, FS, gaps=k)).astype(np.float32) for n, k in ((9000, 1), (6000, 0), (12000, 1))]
    noise = [np.round(rng.normal(0, 2000, 7000)).astype(np.float32), np.zeros(500, np.float32)]
    mean, istd = rng.normal(10.0, 2.0, D).astype(np.float32), rng.uniform(0.2, 0.5, D).astype(np.float32)
    mixes = [(0, 0, 11, 0.0), (1, 1, 3, 5.0), (2, 0, 6999, 10.0)]           # (1, silent noise): g = 0, x == s
    plan = np.zeros(len(mixes), pkg.MIXTURE_DTYPE)
    for k, mx in enumerate(mixes):
        plan[k] = mx
    ls = [(CTX + 1) * D, 64, D]
    W, b = pkg.glorot_net(ls, seed=5, beta=0.5)
    g = pkg.BP_GPU(1, 3, ls, 32, 0.05, 0.5, 0.0, W, b, max_chunk_frames=3000)
    try:
        g.set_mix_corpus(clean, noise, mean, istd, CTX, TOFF, "lps")
        ev = g.eval_mix(plan, FS, pkg.WAVE_LPS, 0, return_pcm=True)
        lens = [clean[k].size for k in plan["clean"]]
        mix = np.split(g.mix_features(plan)["pcm"], np.cumsum(lens)[:-1])
        enh = g.enhance_waves(mix, mean, istd, CTX, TOFF, pkg.WAVE_LPS, 0)
    finally:
        g.close()
    refs = [clean[k] for k in plan["clean"]]
    differ = sum(int((_bits(a) != _bits(e)).sum()) for a, e in zip(ev["pcm"], enh))
    assert [a.size for a in ev["pcm"]] == lens and differ == 0, differ
    assert np.array_equal(_bits(ev["noisy"]), _bits(pkg.score_waves(0, D, FS, refs, mix)))
    assert np.array_equal(_bits(ev["enhanced"]), _bits(pkg.score_waves(0, D, FS, refs, enh)))
    assert ev["noisy"][1, 0] == 35.0 and np.isfinite(ev["enhanced"][:, :2]).all(), (ev["noisy"], ev["enhanced"])
    assert any(e.any() for e in enh)
    parity_record(fea_dim=D, samples_differing=differ, noisy=ev["noisy"].tolist(), enhanced=ev["enhanced"].tolist())
