"""GPU tests of the simulated room impulse responses (bp_rir_image, and bpmix / bpeval with rir_rooms=; -m gpu) against the
float64 restatement in tests/rir_np.py.

The bar is derived, not measured: per tap |got - ref| <= ulp32(ref) + 1e-9 max|ref| (rir_np.bar).  One fp32 ulp covers a
rounding flip of the final fl32; the absolute term covers the double-precision error of the sum, the device's factored window
included (a few double ulps per term, at most a few thousand terms per tap: below 1e-12).  tests/test_rir_host.py shows from the
restatement alone that every image reaching fixtures a .. e has a >= 1e-4, so a dropped or doubled image misses this bar by
more than two orders of magnitude.  A call has one sample rate and one window, so the fixtures travel in one call per setting,
each with company; measured worst error / bar per fixture: profiles/r12_parity_numbers.json, DESIGN.md 20."""
import subprocess

import numpy as np
import pytest

import rir_np as RN

pytestmark = pytest.mark.gpu

FX = RN.fixtures()
NAMES = list(RN.FIXTURE_ORDER)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _rooms(names):
    return np.array([FX[k][0] for k in names], RN.ROOM_DTYPE)


def _groups():
    """the fixtures by (fs, Tw), each group with two companions of other lengths so that no fixture is alone in its call"""
    out = {}
    for k in NAMES:
        out.setdefault((FX[k][1], FX[k][3]), []).append(k)
    return out


@pytest.fixture(scope="module")
def refs():
    return {k: RN.response64(*FX[k]) for k in NAMES}


@pytest.fixture(scope="module")
def together(pkg):
    """every fixture from the call of its group: {name: taps}, and the calls' arguments"""
    got, calls = {}, {}
    for (fs, Tw), names in _groups().items():
        rooms = np.concatenate([_rooms(names), _rooms(["b", "a"])])
        lens = [FX[k][2] for k in names] + [77, 513]
        hs = pkg.rir_image(0, fs, rooms, lens, Tw)
        assert [h.size for h in hs] == lens and all(h.dtype == np.float32 for h in hs)
        got.update(zip(names, hs))
        calls[(fs, Tw)] = (rooms, lens, hs)
    return got, calls


@pytest.mark.parametrize("k", NAMES)
def test_matches_restatement(pkg, refs, together, k, parity_record):
    r, fs, n, Tw = FX[k]
    (alone,) = pkg.rir_image(0, fs, [r], [n], Tw)
    ref = refs[k]
    bar = RN.bar(ref)
    worst = {}
    for tag, h in (("alone", alone), ("together", together[0][k])):
        err = np.abs(h.astype(np.float64) - ref)
        worst[tag] = float((err / bar).max()) if ref.any() else float(err.max())
        print("fixture %s %s: worst error / bar %.4g (max |ref| %.6g)" % (k, tag, worst[tag], np.abs(ref).max()))
    parity_record(**{"err_over_bar_" + t: v for t, v in worst.items()}, max_ref=float(np.abs(ref).max()))
    for tag, h in (("alone", alone), ("together", together[0][k])):
        assert np.all(np.abs(h.astype(np.float64) - ref) <= bar), (k, tag, worst[tag])
    if k == "f":
        assert not _bits(alone).any(), "nothing arrives: +0.0 everywhere"
    else:
        assert int(np.argmax(np.abs(alone))) == int(np.argmax(np.abs(ref)))
    if k in "acg":
        assert int(np.argmax(np.abs(alone))) == round(RN.d0(r) * fs / RN.C), "the direct path is the largest tap"


def test_same_bits_again_alone_and_reversed(pkg, together):
    got, calls = together
    for (fs, Tw), (rooms, lens, hs) in calls.items():
        again = pkg.rir_image(0, fs, rooms, lens, Tw)
        back = pkg.rir_image(0, fs, rooms[::-1], lens[::-1], Tw)[::-1]
        for i, h in enumerate(hs):
            assert np.array_equal(_bits(h), _bits(again[i])), ("a second call", fs, Tw, i)
            assert np.array_equal(_bits(h), _bits(back[i])), ("the rooms reversed", fs, Tw, i)
            (alone,) = pkg.rir_image(0, fs, rooms[i:i + 1], lens[i:i + 1], Tw)
            assert np.array_equal(_bits(h), _bits(alone)), ("alone", fs, Tw, i)


def test_one_more_tap_keeps_the_first_300(pkg, together):
    r, fs, n, Tw = FX["a"]
    assert n == 300 and pkg.rir_orders(r, fs, 300, Tw) == pkg.rir_orders(r, fs, 301, Tw), "the same box: only then the windows agree"
    (h301,) = pkg.rir_image(0, fs, [r], [301], Tw)
    assert np.array_equal(_bits(h301[:300]), _bits(together[0]["a"]))


def test_default_window_and_python_errors(pkg):
    r = FX["a"][0]
    (h,) = pkg.rir_image(0, 8000, [r], [200])
    (h64,) = pkg.rir_image(0, 8000, [r], [200], 64)
    assert np.array_equal(_bits(h), _bits(h64)), "window_taps defaults to 2 round(0.004 fs)"
    with pytest.raises(pkg.BPError, match="2 rooms but 1 lengths"):
        pkg.rir_image(0, 8000, [r, r], [200])
    with pytest.raises(pkg.BPError, match="status -1"):
        pkg.rir_image(0, 8000, [r], [0])


# ---- bpmix / bpeval with rir_rooms=
def _write_pcm16(path, x, rate=8000):
    import wave
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(rate)
        w.writeframes(np.asarray(x, np.int16).tobytes())


def _write_list(d, tag, xs):
    for i, x in enumerate(xs):
        _write_pcm16(d / ("%s%d.wav" % (tag, i)), x)
    (d / (tag + ".list")).write_text("".join("%s\n" % (d / ("%s%d.wav" % (tag, i))) for i in range(len(xs))))
    return str(d / (tag + ".list"))


def _cut(frames, ctx, cap):
    """the calls of bpmix: consecutive mixtures while frames + n_mix (ctx-1) <= traincache"""
    calls, first, rows = [], 0, 0
    for m, T in enumerate(frames):
        if rows + T + ctx - 1 > cap:
            calls.append((first, m)); first, rows = m, 0
        rows += T + ctx - 1
    return calls + [(first, len(frames))]


RANGE_ARGS = ["rir_room_lo=3,2.5,2.2", "rir_room_hi=5,4,3", "rir_t60=0.15,0.3", "rir_margin=0.4", "rir_dist=0.4,2", "rir_ms=30"]
RANGE_KW = dict(L_lo=(3, 2.5, 2.2), L_hi=(5, 4, 3), t60=(0.15, 0.3), margin=0.4, dist=(0.4, 2))


def test_bpmix_rir_rooms_matches_python_api(pkg, tmp_path):
    import pfile_util as PU
    exe = str(pkg.LIB_PATH).replace("libbp_hip.so", "bpmix")
    D, ctx, toff, B, cap, seed, early_ms, fs = 65, 3, 1, 32, 120, 345, 2.0, 8000
    rng = np.random.default_rng(72)
    ints = lambda n, s: np.clip(np.round(rng.normal(0, s, n)), -32768, 32767).astype(np.float32)
    clean = [ints(n, 3000) for n in (1500, 400, 2300, 90)]
    noise = [ints(n, 1500) for n in (5000, 700)]
    cv_clean = [ints(n, 3000) for n in (1800, 600)]
    cl, nl, cvl = (_write_list(tmp_path, t, x) for t, x in (("clean", clean), ("noise", noise), ("cv", cv_clean)))
    (tmp_path / "mix.norm").write_text("<mean>\n" + "0\n" * D + "<inverse std>\n" + "1\n" * D)
    ls = [ctx * D, 64, D]
    W, b = pkg.glorot_net(ls, seed=9, beta=0.5)
    PU.write_wts(str(tmp_path / "init.wts"), ls, W, b)
    args = ["clean_list=" + cl, "noise_list=" + nl, "cv_clean_list=" + cvl, "rir_rooms=4", "cv_rir_rooms=2", "reverb_target=early",
            "early_ms=%g" % early_ms, "rir_rooms_out=%s" % (tmp_path / "rooms.txt"),
            "fea_dim=%d" % D, "snr_list=0,10", "mix_per_clean=2", "init_randem_seed=%d" % seed, "traincache=%d" % cap,
            "norm_file=%s" % (tmp_path / "mix.norm"), "fea_context=%d" % ctx, "targ_offset=%d" % toff, "numlayers=3",
            "layersizes=%s" % ",".join(map(str, ls)), "bunchsize=%d" % B, "lrate=0.01", "momentum=0.5", "weightcost=0.0001",
            "initwts_file=%s" % (tmp_path / "init.wts"), "outwts_file=%s" % (tmp_path / "out.wts"), "log_file=%s" % (tmp_path / "out.log")]
    r = subprocess.run([exe] + args + RANGE_ARGS, capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "all finish!" in r.stdout, r.stdout + r.stderr
    rooms = pkg.rir_rooms(seed, 4, **RANGE_KW)
    listed = np.array([[float(v) for v in ln.split()] for ln in (tmp_path / "rooms.txt").read_text().splitlines()])
    assert listed.shape == (4, 15)
    assert np.array_equal(listed, np.concatenate([rooms["L"], rooms["src"], rooms["mic"], rooms["beta"]], axis=1)), "rir_rooms_out lists the rooms"
    rirs = pkg.rir_image(0, fs, rooms, [240] * 4)                # 30 ms at 8 kHz, the default window
    assert all(np.abs(h).max() > 0.5 for h in rirs)
    plan = pkg.mix_plan(seed, len(clean), 2, [x.size for x in noise], [0.0, 10.0])
    plan["clean"] += len(clean)
    g = pkg.BP_GPU(1, 3, ls, B, 0.01, 0.5, 1e-4, W, b, max_chunk_frames=cap)
    try:
        g.set_mix_corpus(clean, noise, np.zeros(D, np.float32), np.ones(D, np.float32), ctx, toff, "lps")
        g.set_mix_reverb(rirs, np.arange(len(clean)), pkg.mix_reverb_pairs(seed, len(clean), 4), "early", int(early_ms * fs / 1000 + 0.5))
        calls = _cut(g.mix_frames(plan), ctx, cap)
        assert len(calls) > 1
        for k, (a, e) in enumerate(calls):
            g.train_mix(plan[a:e], pkg.mix_shuffle(seed, k, int(g.mix_frames(plan[a:e]).sum())))
        Wp, bp = g.get_weights()
        PU.write_wts(str(tmp_path / "py.wts"), ls, Wp, bp)
    finally:
        g.close()
    assert (tmp_path / "py.wts").read_bytes() == (tmp_path / "out.wts").read_bytes()
    assert "Reverberation: 4 simulated impulse responses, target early, 16 early taps." in (tmp_path / "out.log").read_text()


def test_bpeval_rir_rooms_matches_eval_mix(pkg, tmp_path):
    import pfile_util as PU
    exe = str(pkg.LIB_PATH).replace("libbp_hip.so", "bpeval")
    D, ctx, toff, seed, fs = 65, 3, 1, 91, 8000
    rng = np.random.default_rng(73)
    ints = lambda n, s: np.clip(np.round(rng.normal(0, s, n)), -32768, 32767).astype(np.float32)
    clean = [ints(n, 3000) for n in (3000, 2100, 4000)]
    noise = [ints(n, 1500) for n in (5000, 900)]
    cl, nl = (_write_list(tmp_path, t, x) for t, x in (("clean", clean), ("noise", noise)))
    (tmp_path / "x.norm").write_text("<mean>\n" + "0\n" * D + "<inverse std>\n" + "1\n" * D)
    ls = [ctx * D, 64, D]
    W, b = pkg.glorot_net(ls, seed=5, beta=0.5)
    PU.write_wts(str(tmp_path / "net.wts"), ls, W, b)
    r = subprocess.run([exe, "clean_list=" + cl, "noise_list=" + nl, "norm_file=%s" % (tmp_path / "x.norm"),
                        "initwts_file=%s" % (tmp_path / "net.wts"), "fea_dim=%d" % D, "fea_context=%d" % ctx, "targ_offset=%d" % toff,
                        "layersizes=%s" % ",".join(map(str, ls)), "snr_list=0,10", "mix_per_clean=1", "init_randem_seed=%d" % seed,
                        "traincache=2000", "bunchsize=32", "scores_out=%s" % (tmp_path / "s.txt"), "rir_rooms=2", "rir_window=48",
                        "rir_rooms_out=%s" % (tmp_path / "rooms.txt")] + RANGE_ARGS, capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and r.stdout.strip().splitlines()[-1].startswith("all:"), r.stdout + r.stderr
    rooms = pkg.rir_rooms(seed, 2, **RANGE_KW)
    listed = np.array([[float(v) for v in ln.split()] for ln in (tmp_path / "rooms.txt").read_text().splitlines()])
    assert np.array_equal(listed, np.concatenate([rooms["L"], rooms["src"], rooms["mic"], rooms["beta"]], axis=1))
    rirs = pkg.rir_image(0, fs, rooms, [240] * 2, 48)
    plan = pkg.mix_plan(seed, len(clean), 1, [x.size for x in noise], [0.0, 10.0])
    plan["clean"] += len(clean)
    rows = [ln.split() for ln in (tmp_path / "s.txt").read_text().splitlines()]
    assert [int(x[0]) for x in rows] == [int(c) for c in plan["clean"]], "scores_out lists the derived entries"
    got = np.array([[float(v) for v in x[4:]] for x in rows], np.float32)
    g = pkg.BP_GPU(1, 3, ls, 32, 0.0, 0.0, 0.0, W, b, max_chunk_frames=2000)
    try:
        g.set_mix_corpus(clean, noise, np.zeros(D, np.float32), np.ones(D, np.float32), ctx, toff, "lps")
        g.set_mix_reverb(rirs, np.arange(len(clean)), pkg.mix_reverb_pairs(seed, len(clean), 2), "reverberant", 400)
        assert int((g.mix_frames(plan) + ctx - 1).sum()) <= 2000  # (one call, as bpeval cuts it)
        ev = g.eval_mix(plan, fs)
    finally:
        g.close()
    want = np.stack([ev["noisy"][:, 0], ev["enhanced"][:, 0], ev["noisy"][:, 1], ev["enhanced"][:, 1], ev["noisy"][:, 2], ev["enhanced"][:, 2]], axis=1)
    assert np.array_equal(_bits(got), _bits(want))
