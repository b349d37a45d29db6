"""CPU tests of the MFCC auxiliary target (include/bp_c_api.h): the two host tables against the restatement in
tests/mel_np.py, their properties, the range rules, the mutants of the definition, and bpmix's aux_* keys up to the point where it
would use the device.

Mutant factors on the GPU tests' own inputs (test_mutants_miss_the_gpu_bars; the bars are those of tests/test_mel_gpu.py: 2 fp32 ulp
on logmel, bit equality on the coefficients, counted here as 1 ulp), smallest over the six geometries (one per frame size): edges
shifted one bin 2.6e5 x the logmel bar, log10 for ln 3.8e6 x, j for j + 0.5 5.6e9 ulp, lifter dropped 1.5e7 ulp, c0 present 1.5e9 ulp (the ulp is
that of the true value, and some true coefficients lie near zero).  A mutant is left out where it is the definition itself: the
lifter at L = 0, c0 at first_coef = 0."""
import os
import struct
import subprocess

import numpy as np
import pytest

import mel_np as MN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BPMIX = os.path.join(ROOT, "dnn-for-speech-enhancement_amd", "bpmix")
IDS = [MN.geo_id(g) for g in MN.GEOMETRIES]


def _mel(pkg, g, **kw):
    return pkg.mel_params(g["sample_rate"], n_mel=g["n_mel"], n_ceps=g["n_ceps"], first_coef=g["first_coef"], lifter=g["lifter"], **kw)


def _ulps(a, ref64):
    return MN.ulp_distance(a, ref64)


@pytest.mark.parametrize("g", MN.GEOMETRIES, ids=IDS)
def test_tables_match_the_restatement(pkg, g):
    mp = _mel(pkg, g)
    w, first, nb = pkg.mel_filters(g["fea_dim"], mp)
    t = pkg.mel_dct(mp)
    w64, t64 = MN.filters64(g), MN.dct64(g)
    assert w.shape == w64.shape and t.shape == t64.shape
    # within 1 fp32 ulp: libm's log10 / pow / cos may differ from numpy's in the last double bit
    nz = w64 > 0
    assert _ulps(w[nz], w64[nz]) <= 1.0 and not w[~nz].any()
    assert np.abs(t.astype(np.float64) - t64).max() <= np.spacing(np.float32(np.abs(t64).max()))
    assert _ulps(t[np.abs(t64) > 1e-3], t64[np.abs(t64) > 1e-3]) <= 1.0
    _, f2, n2 = MN.filters(g)
    assert np.array_equal(first, f2) and np.array_equal(nb, n2)
    for j in range(g["n_mel"]):                                   # first_bin / n_bins delimit the bins with w > 0
        k = np.nonzero(w[j] > 0)[0]
        assert k[0] == first[j] and k.size == nb[j] and k[-1] == first[j] + nb[j] - 1


@pytest.mark.parametrize("g", MN.GEOMETRIES, ids=IDS)
def test_filter_rows_are_triangles_that_sum_to_one_inside(pkg, g):
    w, first, nb = pkg.mel_filters(g["fea_dim"], _mel(pkg, g))
    assert (w >= 0).all() and (w <= 1).all()
    e, f = MN.edges(g), MN.bin_hz(g)
    inside = (f >= e[1]) & (f <= e[g["n_mel"]])
    assert inside.sum() > g["n_mel"] // 2
    assert np.abs(w[:, inside].astype(np.float64).sum(axis=0) - 1.0).max() <= 1e-6
    assert (np.diff(first) >= 0).all() and nb.min() >= 1
    assert ((w > 0).sum(axis=0) <= 2).all() and int(nb.sum()) <= 2 * g["fea_dim"]     # a bin lies under at most two triangles


@pytest.mark.parametrize("g", MN.GEOMETRIES, ids=IDS)
def test_unliftered_dct_rows_are_the_orthonormal_dct(pkg, g):
    sf = pytest.importorskip("scipy.fft")
    mp = _mel(pkg, dict(g, lifter=0.0))
    t = pkg.mel_dct(mp).astype(np.float64)
    x = np.random.default_rng(5).normal(size=(16, g["n_mel"]))
    ref = sf.dct(x, type=2, norm="ortho", axis=1)
    for r in range(g["n_ceps"]):
        i = g["first_coef"] + r
        if i >= 1:                                                # (row 0 of the orthonormal DCT carries another factor 1 / sqrt 2)
            assert np.abs(x @ t[r] - ref[:, i]).max() <= 1e-6 * np.abs(ref).max()
    if g["first_coef"] == 0:
        assert np.abs(x @ t[0] - np.sqrt(2.0) * ref[:, 0]).max() <= 1e-6 * np.abs(ref).max()


def test_lifter_is_htk_s(pkg):
    g = MN.GEOMETRIES[1]
    lifted, plain = pkg.mel_dct(_mel(pkg, g)).astype(np.float64), pkg.mel_dct(_mel(pkg, dict(g, lifter=0.0))).astype(np.float64)
    i = np.arange(g["n_ceps"])
    want = 1.0 + 11.0 * np.sin(np.pi * i / 22.0)
    big = np.abs(plain) > 1e-2
    assert np.abs((lifted / np.where(big, plain, 1.0))[big] - np.broadcast_to(want[:, None], plain.shape)[big]).max() <= 1e-5


def test_defaults(pkg):
    mp = pkg.mel_params(16000)
    assert (mp.sample_rate, mp.n_mel, mp.n_ceps, mp.first_coef, mp.f_lo, mp.f_hi, mp.lifter) == (16000, 26, 13, 0, 0.0, 8000.0, 22.0)
    assert not mp.mean and not mp.scale
    with pytest.raises(pkg.BPError, match="unknown field"):
        pkg.mel_params(8000, n_filters=3)
    with pytest.raises(pkg.BPError, match="n_ceps = 13 values"):
        pkg.mel_params(8000, mean=np.zeros(12))
    with pytest.raises(pkg.BPError, match="sample_rate must be > 0"):
        pkg.mel_params(0)


def test_the_four_geometries_hold_no_empty_filter_and_26_filters_do_not_fit_33_bins(pkg):
    assert sorted(g["fea_dim"] for g in MN.GEOMETRIES) == [33, 65, 129, 257, 513, 1025]        # (six by now: one per frame size)
    for g in MN.GEOMETRIES:
        _, _, nb = MN.filters(g)
        assert nb.min() >= 1
    with pytest.raises(ValueError, match="filter 0 "):
        MN.filters(dict(fea_dim=33, sample_rate=8000, n_mel=26))
    with pytest.raises(pkg.BPError, match=r"mel filter 0 holds no bin.*status -1"):
        pkg.mel_filters(33, pkg.mel_params(8000))


def test_every_range_violation_is_refused(pkg):
    g = MN.GEOMETRIES[0]
    bad = [dict(sample_rate=0), dict(sample_rate=-8000), dict(n_mel=1), dict(n_mel=129), dict(n_ceps=0), dict(n_ceps=8), dict(first_coef=-1),
           dict(first_coef=2), dict(f_lo=-1.0), dict(f_lo=float("nan")), dict(f_hi=float("nan")), dict(f_hi=4000.5), dict(f_lo=2000.0, f_hi=2000.0),
           dict(f_lo=3000.0, f_hi=1000.0), dict(lifter=-1.0), dict(lifter=float("inf")), dict(lifter=float("nan"))]
    for kw in bad:
        mp = _mel(pkg, g)
        for k, v in kw.items():
            setattr(mp, k, v)
        with pytest.raises(pkg.BPError, match="status -1"):
            pkg.mel_filters(g["fea_dim"], mp)
        with pytest.raises(pkg.BPError, match="status -1"):
            pkg.mel_dct(mp)
    mp = _mel(pkg, dict(g, n_ceps=7))                             # first_coef = 1: 7 of 8 is the most
    assert pkg.mel_dct(mp).shape == (7, 8)
    for D in (32, 17, 100, 2049):
        with pytest.raises(pkg.BPError, match="power of two.*status -1"):
            pkg.mel_filters(D, _mel(pkg, g))
    for bad_val in (np.inf, np.nan):
        mp = _mel(pkg, g, scale=np.ones(g["n_ceps"]))
        mp._keep_scale[1] = bad_val
        with pytest.raises(pkg.BPError, match="entry 1 is not finite"):
            pkg.mel_dct(mp)
    lib = pkg.load_library()
    assert lib.bp_mel_filters(33, None, None, None, None) == -1 and lib.bp_mel_dct(None, None) == -1 and lib.bp_mel_defaults(8000, None) == -1


def test_a_band_inside_the_spectrum(pkg):
    g = dict(fea_dim=129, sample_rate=8000, n_mel=20, n_ceps=12, first_coef=1, lifter=22.0, f_lo=64.0, f_hi=3800.0)
    mp = _mel(pkg, g, f_lo=64.0, f_hi=3800.0)
    w, first, nb = pkg.mel_filters(129, mp)
    _, f2, n2 = MN.filters(g)
    assert np.array_equal(first, f2) and np.array_equal(nb, n2) and _ulps(w[w > 0], MN.filters64(g)[w > 0]) <= 1.0
    f = MN.bin_hz(g)
    assert not w[:, f <= 64.0].any() and not w[:, f >= 3800.0].any()


# ---- the mutants, from the restatement alone, on the GPU tests' own inputs
def _chain(g, x, mutant):
    """The definition with its fp32 steps on float64 power (the stand-in for the device's): logmel fp32 and the coefficients."""
    import wave_np
    P = (np.abs(wave_np.analysis(x, g["fea_dim"])) ** 2).astype(np.float32)
    w, first, nb = MN.filters(g, mutant)
    lm = MN.log_floor(MN.mel_energy(P, w, first, nb), mutant).astype(np.float32)
    return lm, MN.cepstrum(lm, MN.dct(g, mutant))


@pytest.mark.parametrize("g", MN.GEOMETRIES, ids=IDS)
def test_mutants_miss_the_gpu_bars(g):
    sents = MN.make_sentences(g, 1000 + g["fea_dim"])[3:5]          # two of the random sentences of test_mel_gpu.py
    factors = {}
    for m in MN.MUTANTS:
        if m == "no_lifter" and not g["lifter"] > 0:
            continue
        if m == "c0_present" and g["first_coef"] == 0:
            continue
        worst = 0.0
        for x in sents:
            lm, cc = _chain(g, x, None)
            lm_m, cc_m = _chain(g, x, m)
            if m in ("edges_shifted", "log10"):
                worst = max(worst, MN.ulp_distance(lm_m, lm.astype(np.float64)) / 2.0)     # in units of the 2-ulp logmel bar
            else:
                assert np.array_equal(lm, lm_m)
                worst = max(worst, MN.ulp_distance(cc_m, cc.astype(np.float64)))           # bit equality: counted as 1 ulp
        factors[m] = worst
        assert worst >= 1e4, (m, worst)
    print("mutant factors at %s: %s" % (MN.geo_id(g), ", ".join("%s %.3g" % kv for kv in factors.items())))


# ---- bpmix: the aux_* keys, up to the point where the device would be used
def _wav(path, n, rate=8000):
    pcm = [((i * 37 + n) % 2001) - 1000 for i in range(n)]
    data = struct.pack("<%dh" % n, *pcm)
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, 1, rate, 2 * rate, 2, 16))
        f.write(b"data" + struct.pack("<I", len(data)) + data)


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    if not os.path.exists(BPMIX):
        import __graft_entry__
        __graft_entry__.build()
    d = tmp_path_factory.mktemp("melcli")
    j = lambda n: str(d / n)
    _wav(j("a.wav"), 900); _wav(j("b.wav"), 1300); _wav(j("n.wav"), 4000); _wav(j("c16.wav"), 700, rate=16000)
    open(j("clean.list"), "w").write("%s\n%s\n" % (j("a.wav"), j("b.wav")))
    open(j("noise.list"), "w").write(j("n.wav") + "\n")
    open(j("mixed.list"), "w").write("%s\n%s\n" % (j("a.wav"), j("c16.wav")))
    open(j("norm33"), "w").write("<mean>\n" + "0.5\n" * 33 + "<inverse std>\n" + "2\n" * 33)
    open(j("norm3"), "w").write("<mean>\n" + "0.5\n" * 3 + "<inverse std>\n" + "2\n" * 3)
    return d


def _run(cli, args):
    r = subprocess.run([BPMIX] + [a.replace("<TMP>", str(cli)) for a in args], capture_output=True, text=True, timeout=120)
    return r.returncode, r.stdout


MIX = ["fea_dim=33", "clean_list=<TMP>/clean.list", "noise_list=<TMP>/noise.list"]
TRAIN = MIX + ["fea_context=3", "bunchsize=32", "traincache=2000", "cv_clean_list=<TMP>/clean.list", "outwts_file=<TMP>/mix.wts",
               "log_file=<TMP>/mix.log", "norm_file=<TMP>/norm33", "aux_target=mfcc", "aux_mel=8", "aux_ceps=5", "aux_first=1"]
CLI_CASES = [
    ("aux_target_name", ["aux_target=mel"], "aux_target: mel is not mfcc\n"),
    ("aux_mel_low", ["aux_mel=1"], "bpmix: bad value for aux_mel: 1\n"),
    ("aux_mel_high", ["aux_mel=129"], "bpmix: bad value for aux_mel: 129\n"),
    ("aux_ceps_zero", ["aux_ceps=0"], "bpmix: bad value for aux_ceps: 0\n"),
    ("aux_first_two", ["aux_first=2"], "bpmix: bad value for aux_first: 2\n"),
    ("aux_lifter_neg", ["aux_lifter=-1"], "bpmix: bad value for aux_lifter: -1\n"),
    ("aux_weight_text", ["aux_weight=heavy"], "bpmix: bad value for aux_weight: heavy\n"),
    ("aux_rate_zero", ["aux_rate=0"], "bpmix: bad value for aux_rate: 0\n"),
    ("aux_keys_alone", MIX + ["aux_mel=8"], "bpmix: the aux_* keys need aux_target=mfcc\n"),
    ("default_filters_do_not_fit", MIX + ["aux_target=mfcc"],
     "bpmix: aux_target: bp_mel_filters: mel filter 0 holds no bin (fea_dim 33, 8000 Hz, 26 filters): fewer filters or a larger fea_dim\n"),
    ("too_many_coefficients", MIX + ["aux_target=mfcc", "aux_mel=8", "aux_ceps=8", "aux_first=1"],
     "bpmix: aux_target: bp_mel_filters: n_ceps outside [1, n_mel - first_coef]\n"),
    ("mixed_rates", ["fea_dim=33", "clean_list=<TMP>/mixed.list", "noise_list=<TMP>/noise.list", "aux_target=mfcc", "aux_mel=8"],
     "bpmix: aux_target needs clean sentences of one sample rate (sentence 1 has 16000 Hz, sentence 0 8000 Hz)\n"),
    ("mask_first_target", TRAIN + ["target=irm", "layersizes=99,64,38"],
     "bpmix: aux_target=mfcc needs a target that begins with lps (lps, lps+irm or lps+ibm)\n"),
    ("last_layer_without_the_coefficients", TRAIN + ["target=lps+ibm", "layersizes=99,64,66"],
     "bpmix: layersizes[last] must be 71 for this target with aux_target=mfcc (aux_ceps columns behind the LPS)\n"),
    ("last_layer_lps", TRAIN + ["target=lps", "layersizes=99,64,33"],
     "bpmix: layersizes[last] must be 38 for this target with aux_target=mfcc (aux_ceps columns behind the LPS)\n"),
    ("aux_norm_file_short", TRAIN + ["target=lps", "layersizes=99,64,38", "aux_norm_file=<TMP>/norm3"], "normalization file too short\n"),
    ("aux_norm_file_missing", TRAIN + ["target=lps", "layersizes=99,64,38", "aux_norm_file=<TMP>/none"],
     "can not open normalization file: <TMP>/none\n"),
]


@pytest.mark.parametrize("name,args,text", CLI_CASES, ids=[c[0] for c in CLI_CASES])
def test_bpmix_aux_keys_before_the_device(cli, name, args, text):
    rc, out = _run(cli, args)
    assert rc == 0 and out == text.replace("<TMP>", str(cli)), out
