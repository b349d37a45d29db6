"""GPU tests of the reverberant corpus entries (bp_reverb_waves, bp_set_mix_reverb and the mixing calls on derived entries; -m gpu)
against the float64 restatement in tests/reverb_np.py.  The restatement performs the device's operations in the device's order,
so r and e are compared with np.array_equal on the uint32 view; everything downstream of them is compared as
tests/test_mix_gpu.py compares the dry path (bit-identical where that file is, its bars where it has bars)."""
import os
import subprocess

import numpy as np
import pytest

import mix_np as MX
import reverb_np as RV
import wave_np as WN

pytestmark = pytest.mark.gpu

EARLY_TAPS = [0, 1, 40, 100000]                                  # (the last: >= Lh of every response)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _response(rng, Lh, pos, scale=3000.0):
    h = rng.normal(0.0, scale, Lh).astype(np.float32)
    h[pos] = np.float32(4.0) * np.abs(h).max() + np.float32(1.0)
    return h


# ---- 1. bp_reverb_waves against the restatement
@pytest.fixture(scope="module")
def grid():
    """every sentence with every response; the references for all of EARLY_TAPS, computed once"""
    rng = np.random.default_rng(2026)
    lens = [1, 7, 255, 256, 257, 5000, RV.BLOCK + 1, 300]
    sents = [rng.normal(0.0, 3000.0, n).astype(np.float32) for n in lens]
    sents[-1][:] = 0.0                                           # all zeros: exact zeros out
    rirs, delays = [], []
    for Lh in (1, 2, 63, 64, 65, 1500, RV.TAP_TILE + 1):
        for pos in sorted({0, Lh // 2, Lh - 1}):                 # the delay at 0, in the middle, at the last tap
            rirs.append(_response(rng, Lh, pos)); delays.append(pos)
    jobs = [(si, hi) for si in range(len(sents)) for hi in range(len(rirs))]
    ref = [RV.reverb(sents[si], rirs[hi], EARLY_TAPS) for si, hi in jobs]
    assert any(sents[si].size < rirs[hi].size for si, hi in jobs)
    return dict(sents=sents, rirs=rirs, delays=delays, jobs=jobs, ref=ref)


def _run(pkg, grid, jobs, early_taps, early=True):
    return pkg.reverb_waves(0, [grid["sents"][si] for si, _ in jobs], [hi for _, hi in jobs], grid["rirs"], early_taps, early)


@pytest.mark.parametrize("k", range(len(EARLY_TAPS)))
def test_waves_match_restatement(pkg, grid, k):
    for h, d in zip(grid["rirs"], grid["delays"]):
        assert pkg.rir_delay(h) == d
    rev, ear = _run(pkg, grid, grid["jobs"], EARLY_TAPS[k])
    for (si, hi), r, e, (rr, re) in zip(grid["jobs"], rev, ear, grid["ref"]):
        assert np.array_equal(_bits(r), _bits(rr)), ("r", si, hi)
        assert np.array_equal(_bits(e), _bits(re[k])), ("e", si, hi, EARLY_TAPS[k])
        if k == len(EARLY_TAPS) - 1:
            assert np.array_equal(_bits(e), _bits(r))
        if not grid["sents"][si].any():
            assert not _bits(r).any() and not _bits(e).any(), "a silent sentence gives +0.0 everywhere"


def test_waves_exact_data(pkg):
    """half-integer samples, integer taps in [-2, 2]: every sum is exact, so np.convolve itself is the reference"""
    rng = np.random.default_rng(5)
    s, h = RV.exact_case(rng, RV.BLOCK + 700, 2 * RV.TAP_TILE + 3)
    d = RV.delay(h)
    (r,), (e,) = pkg.reverb_waves(0, [s], [0], [h], 40)
    full = np.convolve(s.astype(np.float64), h.astype(np.float64))
    part = np.convolve(s.astype(np.float64), h.astype(np.float64)[:d + 41])
    assert np.array_equal(r.astype(np.float64), full[d:d + s.size])
    assert np.array_equal(e.astype(np.float64), np.concatenate([part, np.zeros(s.size)])[d:d + s.size])
    rr, re = RV.reverb(s, h, 40)
    assert np.array_equal(_bits(r), _bits(rr)) and np.array_equal(_bits(e), _bits(re))


def test_waves_same_bits_again_and_in_smaller_calls(pkg, grid):
    jobs = grid["jobs"]
    rev, ear = _run(pkg, grid, jobs, 40)
    rev2, ear2 = _run(pkg, grid, jobs, 40)
    for a, b in zip(rev + ear, rev2 + ear2):
        assert np.array_equal(_bits(a), _bits(b))
    sub = list(range(3, len(jobs), 7))
    rev3, ear3 = _run(pkg, grid, [jobs[i] for i in sub], 40)
    for i, r, e in zip(sub, rev3, ear3):
        assert np.array_equal(_bits(r), _bits(rev[i])) and np.array_equal(_bits(e), _bits(ear[i]))
    one = jobs.index((5, len(grid["rirs"]) - 4))                  # the 5000-sample sentence alone, without the early output
    (r,), none = _run(pkg, grid, [jobs[one]], 40, early=False)
    assert none is None and np.array_equal(_bits(r), _bits(rev[one]))
    import ctypes as C                                           # out_rev == NULL: the early output alone
    ip, fp = C.POINTER(C.c_int), C.POINTER(C.c_float)
    s, h = grid["sents"][5], grid["rirs"][jobs[one][1]]
    e = np.empty(s.size, np.float32)
    rc = pkg.load_library().bp_reverb_waves(0, 1, np.array([s.size], np.int32).ctypes.data_as(ip), s.ctypes.data_as(fp),
                                            np.zeros(1, np.int32).ctypes.data_as(ip), 1, np.array([h.size], np.int32).ctypes.data_as(ip),
                                            h.ctypes.data_as(fp), 40, None, e.ctypes.data_as(fp))
    assert rc == 0 and np.array_equal(_bits(e), _bits(ear[one]))


# ---- 2 .. 6: derived entries through the mixing path
def _norm(D, rng):
    return rng.normal(10.0, 2.0, D).astype(np.float32), rng.uniform(0.2, 0.5, D).astype(np.float32)


def _plan(pkg, mixes):
    p = np.zeros(len(mixes), pkg.MIXTURE_DTYPE)
    for i, m in enumerate(mixes):
        p[i] = m
    return p


def _small(rng):
    """3 clean sentences, an all-zero and a real noise recording, 2 responses, 4 pairs"""
    clean = [x + np.float32(0.0) for x in WN.make_sentences(rng, [700, RV.BLOCK + 52, 45])]
    noise = [np.zeros(500, np.float32), WN.make_sentences(rng, [3000], scale=1500.0)[0]]
    rirs = [_response(rng, 40, 5, 0.2), _response(rng, 300, 0, 0.05)]
    return clean, noise, rirs, [0, 1, 2, 1], [0, 1, 1, 0]


def _net(pkg, ls, B=32, cap=4000, **kw):
    W, b = pkg.glorot_net(ls, seed=5, beta=0.5)
    return pkg.BP_GPU(1, len(ls), ls, B, 0.01, 0.5, 1e-4, W, b, max_chunk_frames=cap, **kw)


@pytest.mark.parametrize("target", ["early", "reverberant"])
def test_derived_entries_mix_like_their_signals(pkg, target, parity_record):
    D, ctx, toff, early = 33, 3, 1, 10
    rng = np.random.default_rng(12)
    clean, noise, rirs, pc, pr = _small(rng)
    mean, istd = _norm(D, rng)
    sig = [RV.reverb(clean[c], rirs[h], early) for c, h in zip(pc, pr)]
    g = _net(pkg, [ctx * D, 32, D])
    try:
        g.set_mix_corpus(clean, noise, mean, istd, ctx, toff, MX.LPS)
        g.set_mix_reverb(rirs, pc, pr, target, early)
        assert g.mix_reverb_entries == len(pc)
        n0 = len(clean)
        quiet = _plan(pkg, [(n0 + k, 0, 7 * k, 5.0) for k in range(len(pc))])
        loud = [(n0 + k, 1, 2999 - k, -5.0 + 5 * k) for k in range(len(pc))]
        fq, fl = g.mix_features(quiet), g.mix_features(_plan(pkg, loud))
    finally:
        g.close()
    cuts = np.cumsum([clean[c].size for c in pc])[:-1]
    frames = [(clean[c].size - 1) // (D - 1) + 2 for c in pc]
    worst = 0.0
    for k, (x, t) in enumerate(zip(np.split(fq["pcm"], cuts), np.split(fq["targ"], np.cumsum(frames)[:-1]))):
        r, e = sig[k]
        assert np.array_equal(_bits(x), _bits(r)), "g = 0 on silent noise: x is the mixing signal r"
        mag = np.abs(WN.analysis(e if target == "early" else r, D))   # the target rows: the analysis of the target signal
        for f in range(mag.shape[0]):
            if mag[f].max() > 0:
                worst = max(worst, float(np.abs(np.exp(t[f].astype(np.float64) / 2) - mag[f]).max() / mag[f].max()))
            else:
                assert np.all(t[f] == np.float32(WN.LN_FLOOR))
    assert worst <= 1e-5, worst                                  # (the bar of test_mix_gpu.py for clean LPS)
    # the gain of the definition, computed for r
    ref = [MX.mixture([s[0] for s in sig], noise, (c - n0, n, o, snr)) for c, n, o, snr in loud]
    for x, (xr, _, _, _) in zip(np.split(fl["pcm"], cuts), ref):
        assert np.abs(x - xr).max() <= 1e-6 * np.abs(xr).max()
    parity_record(lps=worst)


def test_dry_entries_keep_their_bits(pkg):
    D, ctx, toff = 33, 3, 1
    rng = np.random.default_rng(13)
    clean, noise, rirs, pc, pr = _small(rng)
    mean, istd = _norm(D, rng)
    ls = [(ctx + 1) * D, 32, 2 * D]
    a, b = _net(pkg, ls), _net(pkg, ls)
    plan = _plan(pkg, [(0, 1, 11, 0.0), (1, 0, 3, 5.0), (2, 1, 2999, -5.0), (1, 1, 100, 10.0)])
    try:
        for g in (a, b):
            g.set_mix_corpus(clean, noise, mean, istd, ctx, toff, MX.LPS_IRM)
        a.set_mix_reverb(rirs, pc, pr, "early", 10)
        fa, fb = a.mix_features(plan), b.mix_features(plan)
        for k in ("fea", "lps", "targ", "nat", "pcm"):
            assert np.array_equal(_bits(fa[k]), _bits(fb[k])), k
        assert np.float32(a.CrossValid_mix(plan)).view(np.uint32) == np.float32(b.CrossValid_mix(plan)).view(np.uint32)
    finally:
        a.close()
        b.close()


def test_identity_response_is_the_dry_sentence(pkg):
    D, ctx, toff, fs = 129, 3, 1, 8000
    rng = np.random.default_rng(14)
    clean = WN.make_sentences(rng, [9000, 4100])
    noise = WN.make_sentences(rng, [7000], scale=1500.0)
    mean, istd = _norm(D, rng)
    g = _net(pkg, [ctx * D, 64, D])
    dry = _plan(pkg, [(0, 0, 11, 0.0), (1, 0, 6999, 10.0)])
    wet = dry.copy()
    wet["clean"] += len(clean)
    try:
        g.set_mix_corpus(clean, noise, mean, istd, ctx, toff, MX.LPS)
        g.set_mix_reverb([np.ones(1, np.float32)], [0, 1], [0, 0], "early", 0)
        fd, fw = g.mix_features(dry), g.mix_features(wet)
        ed, ew = g.eval_mix(dry, fs, return_pcm=True), g.eval_mix(wet, fs, return_pcm=True)
    finally:
        g.close()
    for k in ("fea", "lps", "targ", "pcm"):
        assert np.array_equal(_bits(fd[k]), _bits(fw[k])), k
    for k in ("noisy", "enhanced"):
        assert np.array_equal(_bits(ed[k]), _bits(ew[k])), k
    for x, y in zip(ed["pcm"], ew["pcm"]):
        assert np.array_equal(_bits(x), _bits(y))


def _bits_equal(a, b):
    (wa, ba), (da, dba) = a.get_weights(), a.get_deltas()
    (wb, bb), (db, dbb) = b.get_weights(), b.get_deltas()
    for l in range(1, a.numlayers):
        for u, v in ((wa[l], wb[l]), (ba[l], bb[l]), (da[l], db[l]), (dba[l], dbb[l])):
            if not np.array_equal(u.view(np.uint32), v.view(np.uint32)):
                return False
    return True


@pytest.mark.parametrize("compute_dtype", [0, 1])
def test_training_on_derived_entries_equals_window_path(pkg, compute_dtype):
    """bp_train_mix on derived entries = bp_train_chunk_windows fed with bp_mix_features' outputs (the equivalence of
    test_mix_gpu.py), fp32 and bf16"""
    D, ctx, toff = 33, 3, 1
    rng = np.random.default_rng(15)
    clean, noise, rirs, pc, pr = _small(rng)
    noise[0] = WN.make_sentences(rng, [50], scale=800.0)[0]
    mean, istd = _norm(D, rng)
    ls = [(ctx + 1) * D, 64, 48, 2 * D]
    kw = dict(dropoutflag=1, visible_omit=0.1, hid_omit=0.2, seed=99, compute_dtype=compute_dtype)
    a, b = _net(pkg, ls, **kw), _net(pkg, ls, **kw)
    n0 = len(clean)
    plan = _plan(pkg, [(n0 + 0, 1, 5, 0.0), (1, 0, 49, 5.0), (n0 + 1, 0, 0, -5.0), (n0 + 3, 1, 2999, 10.0), (n0 + 2, 1, 77, 0.0)])
    try:
        for g in (a, b):
            g.set_mix_corpus(clean, noise, mean, istd, ctx, toff, MX.LPS_IBM, 3.0)
            g.set_mix_reverb(rirs, pc, pr, "early", 10)
        for ci, p in enumerate((plan[:3], plan[2:])):
            frames = a.mix_frames(p)
            order = pkg.mix_shuffle(345, ci, int(frames.sum()))
            a.train_mix(p, order)
            f = b.mix_features(p)
            rows = MX.staged_rows(f["fea"], frames, ctx, toff)
            tg = np.zeros((rows.shape[0], f["targ"].shape[1]), np.float32)
            tg[:f["targ"].shape[0]] = f["targ"]
            ws, tf, nr = MX.window_tables(frames, ctx, order)
            b.train_windows(rows, tg, ctx, ws, tf, nat=f["nat"], nat_row=nr)
        assert _bits_equal(a, b)
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("target", ["early", "reverberant"])
def test_eval_mix_scores_against_the_target_signal(pkg, target):
    D, ctx, toff, fs, early = 129, 3, 1, 8000, 80
    rng = np.random.default_rng(16)
    clean = WN.make_sentences(rng, [9000, 4100])
    noise = WN.make_sentences(rng, [7000], scale=1500.0)
    rirs = [_response(rng, 900, 12, 0.05)]
    mean, istd = _norm(D, rng)
    g = _net(pkg, [ctx * D, 64, D])
    plan = _plan(pkg, [(2, 0, 11, 5.0), (3, 0, 6999, 0.0)])
    try:
        g.set_mix_corpus(clean, noise, mean, istd, ctx, toff, MX.LPS)
        g.set_mix_reverb(rirs, [0, 1], [0, 0], target, early)
        x = np.split(g.mix_features(plan)["pcm"], [clean[0].size])
        ev = g.eval_mix(plan, fs, return_pcm=True)
        lm = g.eval_mix_logmmse(plan, fs)
    finally:
        g.close()
    sig = [RV.reverb(c, rirs[0], early) for c in clean]
    refs = [s[1] if target == "early" else s[0] for s in sig]
    assert np.array_equal(_bits(ev["noisy"]), _bits(pkg.score_waves(0, D, fs, refs, x)))
    assert np.array_equal(_bits(ev["enhanced"]), _bits(pkg.score_waves(0, D, fs, refs, ev["pcm"])))
    assert np.array_equal(_bits(lm["noisy"]), _bits(ev["noisy"]))
    if target == "early":                                        # (scored against r the figures differ: the reference matters)
        other = pkg.score_waves(0, D, fs, [s[0] for s in sig], x)
        assert not np.array_equal(_bits(other[:, 0]), _bits(ev["noisy"][:, 0]))


# ---- 6. lifetimes and errors
def test_lifetimes_and_errors(pkg):
    D, ctx, toff = 33, 3, 1
    rng = np.random.default_rng(17)
    clean, noise, rirs, pc, pr = _small(rng)
    mean, istd = _norm(D, rng)
    ls = [ctx * D, 32, D]
    a, b = _net(pkg, ls), _net(pkg, ls)
    n0 = len(clean)
    try:
        with pytest.raises(pkg.BPError, match="status -3"):      # no corpus yet
            a.set_mix_reverb(rirs, pc, pr)
        for g in (a, b):
            g.set_mix_corpus(clean, noise, mean, istd, ctx, toff, MX.LPS)
            g.set_mix_reverb(rirs, pc, pr, "early", 10)
        last = _plan(pkg, [(n0 + 3, 1, 0, 0.0)])
        want = b.mix_features(last)
        bad = [dict(rirs=[]), dict(pair_clean=[], pair_rir=[]), dict(rirs=[rirs[0], np.zeros(0, np.float32)]),
               dict(rirs=[np.ones(RV.MAX_TAPS + 1, np.float32)], pair_rir=[0, 0, 0, 0]), dict(rirs=[rirs[0], np.array([1, np.nan], np.float32)]),
               dict(pair_clean=[0, 1, 3, 1]), dict(pair_clean=[0, -1, 2, 1]), dict(pair_rir=[0, 2, 1, 0]), dict(pair_rir=[0, -1, 1, 0]),
               dict(target=2), dict(target=-1), dict(early_taps=-1)]
        for kw in bad:
            args = dict(rirs=rirs, pair_clean=pc, pair_rir=pr, target="early", early_taps=10)
            args.update(kw)
            with pytest.raises(pkg.BPError, match="status -1"):
                a.set_mix_reverb(**args)
        got = a.mix_features(last)                               # the previous entries are still usable, with their bits
        for k in ("fea", "lps", "targ", "pcm"):
            assert np.array_equal(_bits(got[k]), _bits(want[k])), k
        a.set_mix_reverb(rirs, pc[:2], pr[:2], "reverberant")    # a second call replaces the entries
        assert a.mix_reverb_entries == 2
        a.mix_features(_plan(pkg, [(n0 + 1, 1, 0, 0.0)]))
        for c in (n0 + 2, n0 + 3):
            with pytest.raises(pkg.BPError, match="status -1"):
                a.train_mix(_plan(pkg, [(c, 1, 0, 0.0)]))
        a.set_mix_corpus(clean, noise, mean, istd, ctx, toff, MX.LPS)   # a new corpus drops them
        assert a.mix_reverb_entries == 0
        for call in (a.train_mix, a.CrossValid_mix):
            with pytest.raises(pkg.BPError, match="status -1"):
                call(_plan(pkg, [(n0, 1, 0, 0.0)]))
        a.dp_attach(1, 0, "reverb-%d" % os.getpid())
        with pytest.raises(pkg.BPError, match="status -3"):
            a.set_mix_reverb(rirs, pc, pr)
    finally:
        a.close()
        b.close()


# ---- 7. bpmix rir_list=
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


def test_bpmix_rir_list_matches_python_api(pkg, tmp_path):
    import pfile_util as PU
    exe = str(pkg.LIB_PATH).replace("libbp_hip.so", "bpmix")
    D, ctx, toff, B, cap, seed, early_ms = 65, 3, 1, 32, 120, 345, 2.0
    snrs = [0.0, 10.0]
    rng = np.random.default_rng(71)
    ints = lambda n, s: np.clip(np.round(rng.normal(0, s, n)), -32768, 32767).astype(np.float32)
    clean = [ints(n, 3000) for n in (1500, 400, 2300, 90)]
    noise = [ints(n, 1500) for n in (5000, 700)]
    cv_clean = [ints(n, 3000) for n in (1800, 600)]
    rirs = []
    for Lh, pos in ((30, 3), (200, 0), (64, 10)):                # int16 taps: the direct path at 20000, a decaying tail
        h = np.round(rng.normal(0, 1, Lh) * 3000 * np.exp(-np.arange(Lh) / (Lh / 4))).astype(np.float32)
        h[pos] = 20000
        rirs.append(h)
    cl, nl, cvl, rl = (_write_list(tmp_path, t, x) for t, x in (("clean", clean), ("noise", noise), ("cv", cv_clean), ("rir", rirs)))
    (tmp_path / "mix.norm").write_text("<mean>\n" + "0\n" * D + "<inverse std>\n" + "1\n" * D)
    ls = [ctx * D, 64, D]
    W, b = pkg.glorot_net(ls, seed=9, beta=0.5)
    PU.write_wts(str(tmp_path / "init.wts"), ls, W, b)
    args = ["clean_list=" + cl, "noise_list=" + nl, "cv_clean_list=" + cvl, "rir_list=" + rl, "reverb_target=early", "early_ms=%g" % early_ms,
            "fea_dim=%d" % D, "snr_list=0,10", "mix_per_clean=2", "init_randem_seed=%d" % seed, "traincache=%d" % cap,
            "norm_file=%s" % (tmp_path / "mix.norm"), "fea_context=%d" % ctx, "targ_offset=%d" % toff, "numlayers=3",
            "layersizes=%s" % ",".join(map(str, ls)), "bunchsize=%d" % B, "lrate=0.01", "momentum=0.5", "weightcost=0.0001",
            "initwts_file=%s" % (tmp_path / "init.wts"), "outwts_file=%s" % (tmp_path / "out.wts"), "log_file=%s" % (tmp_path / "out.log"),
            "mix_plan_out=%s" % (tmp_path / "plan.txt")]
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "all finish!" in r.stdout, r.stdout + r.stderr
    plan = pkg.mix_plan(seed, len(clean), 2, [x.size for x in noise], snrs)
    plan["clean"] += len(clean)                                  # the plan addresses the derived entries
    rows = [ln.split() for ln in (tmp_path / "plan.txt").read_text().splitlines()]
    assert [(int(c), int(n), int(o), np.float32(s)) for c, n, o, s in rows] == [(int(c), int(n), int(o), s) for c, n, o, s in plan.tolist()]
    assert min(int(c) for c, _, _, _ in rows) >= len(clean)
    g = pkg.BP_GPU(1, 3, ls, B, 0.01, 0.5, 1e-4, W, b, max_chunk_frames=cap)
    try:
        g.set_mix_corpus(clean, noise, np.zeros(D, np.float32), np.ones(D, np.float32), ctx, toff, "lps")
        g.set_mix_reverb(rirs, np.arange(len(clean)), pkg.mix_reverb_pairs(seed, len(clean), len(rirs)), "early", int(early_ms * 8000 / 1000 + 0.5))
        calls = _cut(g.mix_frames(plan), ctx, cap)
        assert len(calls) > 1
        for k, (a, e) in enumerate(calls):
            g.train_mix(plan[a:e], pkg.mix_shuffle(seed, k, int(g.mix_frames(plan[a:e]).sum())))
        Wp, bp = g.get_weights()
        PU.write_wts(str(tmp_path / "py.wts"), ls, Wp, bp)
    finally:
        g.close()
    assert (tmp_path / "py.wts").read_bytes() == (tmp_path / "out.wts").read_bytes()
    assert "Reverberation: 3 impulse responses, target early, 16 early taps." in (tmp_path / "out.log").read_text()
