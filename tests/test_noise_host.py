"""Host tests of the MMSE-SPP noise tracker of the log-MMSE baseline: what the float64 restatement in
tests/noise_np.py does on its fixtures -- the ramped ceiling is exercised, a step in the noise level is followed where the
VAD-gated estimate freezes, and every listed mutant of the definition misses the project's bar -- and the parts of the library
and the tools that answer before the device is used: parameter checks, defaults, and the lm_noise= key."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import classic_np as CN
import noise_np as NN
from util import TOL, relerr

FEA_DIMS = [33, 65, 129, 257]


def _sentence(D, kind):
    _, kinds, xs = NN.fixture(D)
    i = kinds.index(kind)
    return i, xs[i]


# ---- 1. the restatement on its fixtures
def test_fixtures_extend_the_classic_ones():
    for (D, kinds, xs), (Dc, kc, xc) in zip(NN.fixtures(), sorted(CN.fixtures(), key=lambda f: f[0])):
        assert D == Dc and kinds[:len(kc)] == list(kc) and kinds[len(kc):] == ["sustained", "step"]
        assert all(np.array_equal(a, b) for a, b in zip(xs, xc))
        assert CN.n_frames(xs[-2].size, D) == NN.SUSTAINED_FRAMES and CN.n_frames(xs[-1].size, D) == NN.STEP_FRAMES
    assert [D for D, _ in NN.wide_fixtures()] == [513, 1025]


@pytest.mark.parametrize("D", FEA_DIMS)
def test_sustained_tones_reach_the_ramp_and_the_full_ceiling(D):
    i, _ = _sentence(D, "sustained")
    r = NN.reference(D, i)
    print("fea_dim %d: %d frame-bins inside the ramp, %d at the full ceiling" % (D, r["ramp"], r["full"]))
    assert r["ramp"] > 0 and r["full"] > 0


@pytest.mark.parametrize("D", FEA_DIMS)
def test_the_tracker_follows_a_step_and_the_vad_gated_estimate_does_not(D):
    i, _ = _sentence(D, "step")
    spp = NN.step_level_db(NN.reference(D, i)["noise"], D)
    vad = NN.step_level_db(NN.reference(D, i, NN.MODE_VAD)["noise"], D)
    print("fea_dim %d: tracker %.2f dB, VAD-gated %.2f dB of the true noise power" % (D, spp, vad))
    assert spp >= -2.5 and vad <= -5.0


def test_the_busy_parameters_make_the_carried_pbar_matter_in_every_bin():
    """The stream tests compare with the offline call bit for bit; that says something about the pbar a stream carries between
    pushes only where pbar reaches the ramp.  At the defaults that is a few tone bins of the 62-frame sentence and none at all of
    the wide sentences (a dozen frames); under noise_np.BUSY it is every bin, at every size."""
    cases = [(D, NN.fixture(D)[2][0]) for D in FEA_DIMS] + [(D, x) for D, xs in CN.wide_fixtures() for x in (xs[2], xs[0])]
    assert sorted({D for D, _ in cases}) == [33, 65, 129, 257, 513, 1025]
    for D, x in cases:
        ramp, full, share = NN.ceiling_share(x, D, NN.BUSY)
        print("fea_dim %d, %d samples: %d frame-bins inside the ramp, %d at the ceiling, %.3f of the bins moved" % (D, x.size, ramp, full, share))
        assert ramp > 0 and full > 0 and share == 1.0, (D, x.size)
        if D > 257:
            assert NN.ceiling_share(x, D, None)[:2] == (0, 0)         # the defaults never get there in a dozen frames


def test_vad_mode_is_the_classic_restatement():
    D = 129
    i, x = _sentence(D, "tones")
    a, b = NN.reference(D, i, NN.MODE_VAD), CN.reference(D, i)
    assert np.array_equal(a["G"], b["G"]) and np.array_equal(a["vad"], b["vad"]) and np.array_equal(a["pcm"], b["pcm"])
    Y = CN.analysis(x, D)
    P = Y.real ** 2 + Y.imag ** 2
    assert np.array_equal(a["noise"][0], np.maximum(P[:6].mean(axis=0), CN.LAMBDA_FLOOR))


def test_a_silent_sentence_stays_at_the_floor():
    r = NN.reference(129, _sentence(129, "zero")[0])
    assert not r["G"].any() and not r["pcm"].any() and np.all(r["noise"] == CN.LAMBDA_FLOOR)


# ---- 2. the mutants: each misses the bar on some fixture, shown from the restatement alone
MUTANT_FIXTURES = [(33, "sustained"), (65, "sustained"), (33, "step")]


@pytest.mark.parametrize("mutant", NN.MUTANTS)
def test_every_mutant_misses_the_bar(mutant):
    worst = 0.0
    for D, kind in MUTANT_FIXTURES:
        i, x = _sentence(D, kind)
        r = NN.reference(D, i)
        if mutant == "pbar_carried":                             # the sentence before it in the call leaves its pbar behind
            q = NN.enhance(x, D, pbar0=NN.reference(D, i - 1)["pbar"])
        else:
            q = NN.enhance(x, D, mutant=mutant)
        worst = max(worst, relerr(q["G"] * q["absY"], r["G"] * r["absY"]), relerr(q["noise"], r["noise"]))
    print("%s: %.3g" % (mutant, worst))
    assert worst > TOL


# ---- 3. the library before the device
def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def test_noise_defaults_and_symbols(pkg):
    lib = pkg.load_library()
    for s in ("bp_noise_defaults", "bp_logmmse_waves_nt", "bp_eval_mix_logmmse_nt", "bp_lmstream_open_nt"):
        assert hasattr(lib, s) and s in pkg.ABI_SYMBOLS
    assert lib.bp_abi_version() == 5
    nz = pkg.BPNoiseParams()
    assert lib.bp_noise_defaults(C.byref(nz)) == 0 and lib.bp_noise_defaults(None) == -1
    assert (nz.mode, nz.xi_h1_db, nz.q, nz.a_pow, nz.a_spp, nz.p_lo, nz.p_cap) == (1, 15.0, 0.5, 0.8, 0.9, 0.98, 0.99)
    assert (pkg.NOISE_VAD, pkg.NOISE_SPP) == (0, 1)
    d = pkg.noise_params({"mode": "vad", "q": 0.4})
    assert (d.mode, d.q, d.a_pow) == (0, 0.4, 0.8) and pkg.noise_params("spp").mode == 1 and pkg.noise_params(d) is d
    for bad in ({"beta": 1.0}, {"mode": "imcra"}):
        with pytest.raises(pkg.BPError):
            pkg.noise_params(bad)


BAD = [("mode", {"mode": 2}), ("mode", {"mode": -1}), ("xi_h1_db", {"xi_h1_db": -0.5}), ("xi_h1_db", {"xi_h1_db": 40.5}),
       ("xi_h1_db", {"xi_h1_db": float("nan")}), ("q", {"q": 0.0}), ("q", {"q": 1.0}), ("a_pow", {"a_pow": -0.1}), ("a_pow", {"a_pow": 1.0}),
       ("a_spp", {"a_spp": -0.1}), ("a_spp", {"a_spp": 1.0}), ("p_lo", {"p_lo": 0.0}), ("p_lo", {"p_lo": 0.99}),
       ("p_cap", {"p_cap": 1.0}), ("p_cap", {"p_cap": 0.5}), ("p_cap", {"p_cap": float("nan")})]


@pytest.mark.parametrize("field,bad", BAD)
def test_noise_parameters_out_of_range_are_argument_errors(pkg, field, bad):
    """BP_ERR_ARG with the field's name, from both handle-less calls, before the device is used (there is none here)."""
    lib = pkg.load_library()
    nz = pkg.noise_params(bad)
    x, lens = np.ones(300, np.float32), (C.c_int * 1)(300)
    out = np.empty(300, np.float32)
    assert lib.bp_logmmse_waves_nt(0, 129, None, C.byref(nz), 1, lens, _fp(x), _fp(out), None, None, None) == -1
    msg = lib.bp_last_error().decode()
    assert msg.startswith("bp_logmmse_waves_nt: ") and field in msg, msg
    s = C.c_void_p()
    assert lib.bp_lmstream_open_nt(0, 129, None, C.byref(nz), 1, 1000, C.byref(s)) == -1 and not s.value
    msg = lib.bp_last_error().decode()
    assert msg.startswith("bp_lmstream_open_nt: ") and field in msg, msg
    m, sc = np.zeros(1, pkg.MIXTURE_DTYPE), np.zeros(5, np.float32)
    assert lib.bp_eval_mix_logmmse_nt(None, None, C.byref(nz), 1, m.ctypes.data_as(C.c_void_p), 8000, 3, _fp(sc), _fp(sc), None) == -1


def test_the_other_arguments_are_checked_as_in_the_calls_without_noise(pkg):
    lib = pkg.load_library()
    x, lens, out = np.ones(300, np.float32), (C.c_int * 1)(300), np.empty(300, np.float32)
    lm = pkg.logmmse_params({"alpha": 1.5})
    s = C.c_void_p()
    for D, p in ((100, None), (129, C.byref(lm))):
        assert lib.bp_logmmse_waves_nt(0, D, p, None, 1, lens, _fp(x), _fp(out), None, None, None) == -1
        assert lib.bp_last_error().decode().startswith("bp_logmmse_waves_nt: ")
        assert lib.bp_lmstream_open_nt(0, D, p, None, 1, 1000, C.byref(s)) == -1
        assert lib.bp_last_error().decode().startswith("bp_lmstream_open_nt: ")
    assert lib.bp_logmmse_waves_nt(0, 129, None, None, 1, lens, _fp(x), None, None, None, None) == -1
    assert lib.bp_lmstream_open_nt(0, 129, None, None, 0, 1000, C.byref(s)) == -1
    assert lib.bp_lmstream_open_nt(0, 129, None, None, 1, 1000, None) == -1
    # the calls without noise parameters keep their names in their messages
    assert lib.bp_lmstream_open(0, 129, None, 0, 1000, C.byref(s)) == -1 and lib.bp_last_error().decode().startswith("bp_lmstream_open: ")


# ---- 4. the lm_noise= key
def _tool(pkg, name, *keys):
    exe = str(pkg.LIB_PATH).replace("libbp_hip.so", name)
    r = subprocess.run([exe] + list(keys), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr                # message + exit(0): the reference convention
    return r.stdout.strip()


def test_lm_noise_key_of_bpenhance(pkg, tmp_path):
    io = ["in_wav=%s" % (tmp_path / "in.wav"), "out_wav=%s" % (tmp_path / "out.wav"), "fea_dim=129"]
    for v in ("", "SPP", "1", "imcra"):
        assert _tool(pkg, "bpenhance", "method=logmmse", "lm_noise=%s" % v, *io) == "lm_noise: %s is not vad or spp" % v
    for v in ("vad", "spp"):
        assert _tool(pkg, "bpenhance", "lm_noise=%s" % v, *io) == "bpenhance: lm_noise needs method=logmmse"
        # a good value gets as far as the input file, which is not there
        assert "in.wav" in _tool(pkg, "bpenhance", "method=logmmse", "lm_noise=%s" % v, "lm_stream_block=160", *io)
    assert not (tmp_path / "out.wav").exists()


def test_lm_noise_key_of_bpeval(pkg, tmp_path):
    keys = ["clean_list=%s" % (tmp_path / "c.list"), "noise_list=%s" % (tmp_path / "n.list"), "fea_dim=129"]
    assert _tool(pkg, "bpeval", "baseline=logmmse", "lm_noise=imcra", *keys) == "bpeval: bad value for lm_noise: imcra"
    assert _tool(pkg, "bpeval", "lm_noise=spp", *keys) == "bpeval: lm_noise needs baseline=logmmse"
    assert _tool(pkg, "bpeval", "lm_noise=vad", *keys) == "bpeval: lm_noise needs baseline=logmmse"
    assert "pairs_list takes only" in _tool(pkg, "bpeval", "pairs_list=%s" % (tmp_path / "p.list"), "fea_dim=129", "lm_noise=spp")
    assert "lm_noise" not in _tool(pkg, "bpeval", "baseline=logmmse", "lm_noise=spp", *keys)     # accepted: the next complaint is another
