"""GPU tests of the post-processing of the LPS estimate (bp_set_post, bp_post_rows, bp_gv_mix; -m gpu) against
the restatement in tests/post_np.py.  The value and the sums are held to the bit (np.array_equal); resynthesis from the
post-processed rows to 1e-5 of the largest magnitude, the bar tests/test_wave_gpu.py holds resynthesis to.

Shapes: every frame size of the signal layer (tests/geometry_cases.py).  At fea_dim 33 and 129 sentences of 1, 31, 500 and 3000
samples and a corpus of three clean sentences (31, 500, 3000 samples); at the other four sizes nothing longer than 12 hop + 7
samples (14 frames): sentences of 1, hop + 1, 5 hop + 3 and 12 hop + 7 samples, clean sentences of 2, 5 and 14 frames.  Two
noises; nets 3 D -> 64 -> 2 D with a logistic mask block.  What changes with the size: the bins per thread of the synthesis
kernels (one up to 257, two at 513, four at 1025) and the large LDS layout of the stream synthesis from 257 on, and the
ceil(D / 64) column blocks of the two sum kernels (1, 2 -- the second with one live thread -- 3, 5, 9, 17)."""
import subprocess

import numpy as np
import pytest

import post_np as PN
import wave_np as WN

pytestmark = pytest.mark.gpu

DIMS = [33, 65, 129, 257, 513, 1025]
LONG = (33, 129)                                                         # the sizes that keep the long sentences
FS = 8000
GATE = dict(mask_lo=0.3, mask_hi=0.7, mask_weight=0.8)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return all(u.shape == v.shape and np.array_equal(_bits(u), _bits(v)) for u, v in zip(a, b)) and len(a) == len(b)


def _net(pkg, D, seed=3):
    ls = [3 * D, 64, 2 * D]
    W, b = pkg.glorot_net(ls, seed=seed, beta=0.5)
    return ls, W, b


def _handle(pkg, D, bf16=False, cap=1024, B=32, lrate=0.0, **kw):
    ls, W, b = _net(pkg, D)
    return pkg.BP_GPU(1, 3, ls, B, lrate, 0.5, 0.0, W, b, max_chunk_frames=cap, compute_dtype=int(bf16), output_activation=1,
                      output_linear_cols=D, **kw)


def _norm(D):
    rng = np.random.default_rng(D)
    return rng.normal(10.0, 2.0, D).astype(np.float32), rng.uniform(0.2, 0.5, D).astype(np.float32)


def _gv(D):
    rng = np.random.default_rng(2 * D)
    return rng.normal(0.5, 0.3, D).astype(np.float32), rng.uniform(1.1, 1.9, D).astype(np.float32)


def _lens(D):
    hop = D - 1
    return [1, 31, 500, 3000] if D in LONG else [1, hop + 1, 5 * hop + 3, 12 * hop + 7]


def _clean_lens(D):
    hop = D - 1
    return [31, 500, 3000] if D in LONG else [hop - 1, 3 * hop + 5, 12 * hop + 7]


def _corpus(D):
    rng = np.random.default_rng(7 + D)
    clean = WN.make_sentences(rng, _clean_lens(D))
    noise = [np.round(rng.normal(0, 1500, 5000)).astype(np.float32), np.round(rng.normal(0, 300, 777)).astype(np.float32)]
    return clean, noise


# Frame counts of a bp_gv_mix call (64 parts): below 64, where some parts are empty; a multiple of 64; one frame more; about 700.
# The clean entries have 2, 17 and 95 frames at fea_dim 33 and 2, 5 and 25 at 129; 2, 5 and 14 at the other sizes, where the
# largest call has 187 frames: three frames per part, part 62 with one frame and part 63 empty.
SHORT = {7: [1, 0], 64: [2, 2, 2, 2, 0, 0, 0, 0], 65: [2, 2, 2, 2, 1, 0, 0], 187: [2] * 13 + [1]}
PLANS = {33: {19: [1, 0], 128: [2, 1] + [0] * 8, 129: [2, 1, 1], 699: [2] * 7 + [1, 1]},
         129: {7: [1, 0], 64: [2, 2, 1, 1, 0, 0], 65: [2, 2, 1, 1, 1], 700: [2] * 28},
         65: SHORT, 257: SHORT, 513: SHORT, 1025: SHORT}


def _plan(pkg, D, frames):
    """The plan of the corpus with exactly `frames` frames."""
    idx = PLANS[D][frames]
    assert sum((_clean_lens(D)[c] - 1) // (D - 1) + 2 for c in idx) == frames
    p = np.zeros(len(idx), pkg.MIXTURE_DTYPE)
    for i, c in enumerate(idx):
        p[i] = (c, i % 2, (37 * i) % 700, float(5 * (i % 3)))
    return p


def _mixtures(g, plan):
    """The mixed sentences of the plan and the noisy LPS rows of the device."""
    f = g.mix_features(plan)
    lens = [g.mix_clean_len[c] for c in plan["clean"]]
    return np.split(f["pcm"], np.cumsum(lens)[:-1]), f["lps"]


# ---- 1. bp_post_rows against the restatement, to the bit
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("what", ["gv", "gate", "both", "step"])
def test_post_rows_equal_the_restatement(pkg, D, what, parity_record):
    rng = np.random.default_rng(D + len(what))
    n = 70
    est = rng.normal(9.0, 3.0, (n, D)).astype(np.float32)
    y = (est + rng.normal(1.5, 2.0, (n, D))).astype(np.float32)
    y[3] = np.float32(WN.LN_FLOOR)                                       # a frame at the LPS floor
    m = rng.uniform(-0.1, 1.1, (n, D)).astype(np.float32)                # below lo, above hi and in between
    m[5, ::3] = np.nan
    m[6, :4] = [0.3, 0.7, 0.5, np.float32(0.7) - np.float32(6e-8)]       # the thresholds themselves
    c, s = _gv(D)
    kw = {}
    if what in ("gv", "both"):
        kw.update(gv_center=c, gv_scale=s)
    if what in ("gate", "both"):
        kw.update(mask=m, **GATE)
    if what == "step":
        kw.update(mask=m, mask_lo=0.5, mask_hi=0.5, mask_weight=1.0)
    got = pkg.post_rows(0, est, y, **kw)
    want = PN.post(est, y, kw.get("mask"), kw.get("gv_center"), kw.get("gv_scale"), kw.get("mask_lo", 0.5), kw.get("mask_hi", 0.5),
                   kw.get("mask_weight", 1.0))
    diff = int((_bits(got) != _bits(want)).sum())
    parity_record(words_differing=diff, values=int(got.size), nan_masks=int(np.isnan(m).sum()))
    assert diff == 0
    assert not np.array_equal(_bits(got), _bits(est))
    if "mask" in kw:
        assert np.array_equal(_bits(got[5, ::3]), _bits(PN.post(est, center=kw.get("gv_center"), scale=kw.get("gv_scale"))[5, ::3]))
    if what == "step":                                                   # the hard rule: the noisy LPS where the mask reaches 0.5
        on = m >= 0.5
        assert np.allclose(got[on], y[on], rtol=0, atol=4e-6) and np.array_equal(_bits(got[~on]), _bits(est[~on]))


def test_post_rows_argument_checks(pkg):
    D = 33
    est, y = np.zeros((4, D), np.float32), np.ones((4, D), np.float32)
    c, s = _gv(D)
    bad = [dict(gv_center=c, gv_scale=-s), dict(gv_center=c * np.float32(np.nan), gv_scale=s), dict(mask=est, mask_lo=0.8, mask_hi=0.2),
           dict(mask=est, mask_weight=1.5), dict(mask=est, mask_weight=-0.1), dict(mask=est, mask_lo=np.inf, mask_hi=np.inf),
           dict(gv_center=c[:-1], gv_scale=s[:-1])]
    for kw in bad:
        with pytest.raises(pkg.BPError):
            pkg.post_rows(0, est, y, **kw)
    with pytest.raises(pkg.BPError, match="status -1"):
        pkg.post_rows(0, np.zeros((4, 34), np.float32), np.zeros((4, 34), np.float32))
    with pytest.raises(pkg.BPError, match="status -1"):
        pkg.post_rows(99, est, y)


# ---- 2. / 3. bp_gv_mix against the restated sums, to the bit
def _frame_counts(D):
    return sorted(PLANS[D])


@pytest.fixture(scope="module")
def raw_case(pkg):
    """Per fea_dim: a handle with the corpus, and per frame count the plan, the net columns, the noisy and the clean LPS."""
    out = {}
    for D in DIMS:
        g = _handle(pkg, D)
        mean, istd = _norm(D)
        clean, noise = _corpus(D)
        g.set_mix_corpus(clean, noise, mean, istd, 3, 1, "lps+ibm")
        ref_lps = pkg.wave_lps(0, D, clean)
        cases = {}
        for n in _frame_counts(D):
            plan = _plan(pkg, D, n)
            mix, lps = _mixtures(g, plan)
            _, net = g.enhance_waves(mix, mean, istd, 3, 1, return_net=True)
            cases[n] = dict(plan=plan, net=np.concatenate(net), lps=lps, ref=np.concatenate([ref_lps[c] for c in plan["clean"]]))
            assert cases[n]["net"].shape[0] == n
        out[D] = dict(g=g, mean=mean, istd=istd, cases=cases)
    yield out
    for v in out.values():
        v["g"].close()


def _sums_equal(got, want):
    return sum(int((got[k].view(np.uint64) != want[k].view(np.uint64)).sum()) for k in ("est_sum", "est_sq", "ref_sum", "ref_sq"))


@pytest.mark.parametrize("D", DIMS)
def test_gv_mix_raw_equals_the_restated_sums(pkg, raw_case, D, parity_record):
    rc = raw_case[D]
    g, rec = rc["g"], {}
    for n, c in rc["cases"].items():
        got = g.gv_mix(c["plan"], out_col=0, stage="raw")
        want = PN.gv_sums(c["net"][:, :D], c["ref"])
        assert got["frames"] == n == want["frames"]
        rec[n] = _sums_equal(got, want)
        again = g.gv_mix(c["plan"], out_col=0, stage="post")             # post-processing is off: identical to raw
        assert _sums_equal(again, got) == 0
    parity_record(fea_dim=D, words_differing_by_frames=rec)
    assert all(v == 0 for v in rec.values()), rec
    # the mask block as the estimate: another column offset
    c = rc["cases"][_frame_counts(D)[2]]
    assert _sums_equal(g.gv_mix(c["plan"], out_col=D), PN.gv_sums(c["net"][:, D:], c["ref"])) == 0


# (the bf16 x dynamic cross at fea_dim 33 and 129; the other four sizes in fp32 with the static row)
@pytest.mark.parametrize("D,nat,bf16", [(D, nat, bf16) for D in LONG for nat in ("static", "dynamic") for bf16 in (False, True)] +
                         [(D, "static", False) for D in DIMS if D not in LONG])
def test_gv_mix_post_equals_the_restated_sums(pkg, D, bf16, nat, parity_record):
    """The fused value, pinned to the bit: the sums of post_np over the net's columns and the device's noisy LPS.  Nets with the
    noise-aware block (context 2: 3 D inputs), in both of its modes."""
    g = _handle(pkg, D, bf16=bf16)
    mean, istd = _norm(D)
    clean, noise = _corpus(D)
    c, s = _gv(D)
    try:
        g.set_nat(nat)
        g.set_mix_corpus(clean, noise, mean, istd, 2, 0, "lps+ibm")
        plan = _plan(pkg, D, _frame_counts(D)[2])
        mix, lps = _mixtures(g, plan)
        _, net = g.enhance_waves(mix, mean, istd, 2, 0, return_net=True)
        net = np.concatenate(net)
        clean_lps = pkg.wave_lps(0, D, clean)
        ref = np.concatenate([clean_lps[k] for k in plan["clean"]])
        rec = {}
        for name, kw in (("gv", dict(gv_center=c, gv_scale=s)), ("gate", dict(mask_col=D, **GATE)),
                         ("both", dict(gv_center=c, gv_scale=s, mask_col=D, **GATE)),
                         ("step", dict(mask_col=D, mask_lo=0.5, mask_hi=0.5, mask_weight=1.0, fea_dim=D))):
            if "fea_dim" not in kw and "gv_center" not in kw:
                kw["fea_dim"] = D
            g.set_post(**kw)
            rows = PN.post(net[:, :D], lps, net[:, D:] if kw.get("mask_col", -1) >= 0 else None, kw.get("gv_center"), kw.get("gv_scale"),
                           kw.get("mask_lo", 0.5), kw.get("mask_hi", 0.5), kw.get("mask_weight", 1.0))
            rec[name] = _sums_equal(g.gv_mix(plan, stage="post"), PN.gv_sums(rows, ref))
            assert _sums_equal(g.gv_mix(plan, stage="raw"), PN.gv_sums(net[:, :D], ref)) == 0
            assert not np.array_equal(_bits(rows), _bits(net[:, :D]))
        parity_record(fea_dim=D, bf16=bf16, nat=nat, words_differing=rec)
        assert all(v == 0 for v in rec.values()), rec
    finally:
        g.close()


# ---- 4. resynthesis from the post-processed rows
@pytest.mark.parametrize("D", DIMS)
def test_resynthesis_from_the_post_processed_rows(pkg, D, parity_record):
    rng = np.random.default_rng(40 + D)
    xs = WN.make_sentences(rng, _lens(D))
    mean, istd = _norm(D)
    c, s = _gv(D)
    g = _handle(pkg, D)
    try:
        off, net = g.enhance_waves(xs, mean, istd, 3, 1, return_net=True)
        g.set_post(gv_center=c, gv_scale=s, mask_col=D, **GATE)
        on, net_on = g.enhance_waves(xs, mean, istd, 3, 1, return_net=True)
    finally:
        g.close()
    assert _same(net, net_on)                                            # out_net remains the net's own outputs
    lps = pkg.wave_lps(0, D, xs)
    err = 0.0
    for x, y, o, l, o0 in zip(xs, on, net, lps, off):
        rows = PN.post(o[:, :D], l, o[:, D:], c, s, GATE["mask_lo"], GATE["mask_hi"], GATE["mask_weight"])
        ref = WN.resynth(WN.analysis(x, D), rows, 0, x.size)
        err = max(err, float(np.abs(y - ref).max() / np.abs(ref).max()))
        assert not np.array_equal(_bits(y), _bits(o0))
    parity_record(fea_dim=D, wave_err=err)
    assert err <= 1e-5, err


def test_the_hard_rule_with_a_mask_of_one_returns_the_noisy_input(pkg, parity_record):
    """The identity multi-objective net of test_multi_objective_columns (LPS columns 6 dB down, mask = 1): with lo = hi = 0.5 and
    weight 1 every bin takes the noisy LPS, and the output is the input."""
    D = 129
    rng = np.random.default_rng(5)
    xs = WN.make_sentences(rng, [1500, 400])
    m, i = WN.norm_stats(xs, D)
    m, i = m.astype(np.float32), i.astype(np.float32)
    ls, W, b = WN.identity_net(D, 3, 1, False, m, i)
    ls[-1] = 2 * D
    W[2] = np.concatenate([W[2], np.zeros_like(W[2])], axis=1)
    b[2] = np.concatenate([b[2] + np.float32(2 * np.log(0.5)), np.full(D, 40.0, np.float32)]).astype(np.float32)
    g = pkg.BP_GPU(1, 3, ls, 64, 0.0, 0.0, 0.0, W, b, max_chunk_frames=2000, output_activation=1, output_linear_cols=D)
    try:
        half = g.enhance_waves(xs, m, i, 3, 1)
        g.set_post(mask_col=D, mask_lo=0.5, mask_hi=0.5, mask_weight=1.0, fea_dim=D)
        full = g.enhance_waves(xs, m, i, 3, 1)
    finally:
        g.close()
    e_half = max(float(np.abs(2 * h - x).max() / np.abs(x).max()) for h, x in zip(half, xs))
    e_full = max(float(np.abs(f - x).max() / np.abs(x).max()) for f, x in zip(full, xs))
    parity_record(half_err=e_half, noisy_err=e_full)
    assert e_half <= 1e-5 and e_full <= 1e-5, (e_half, e_full)


# ---- 5. bit for bit across the paths
def _stream_run(s, xs, rng, hop):
    """The sentences dealt to the stream's channels and pushed in ragged blocks; the finished sentences in their order."""
    nc = s.n_chan
    queue = [list(range(c, len(xs), nc)) for c in range(nc)]
    pos, outs, cur = [0] * nc, {}, [q.pop(0) if q else None for q in queue]
    acc = [[] for _ in range(nc)]
    while any(k is not None for k in cur):
        blocks, end = [], []
        for c in range(nc):
            k = cur[c]
            if k is None:
                blocks.append(None); end.append(False)
                continue
            n = int(rng.integers(0, 3 * hop + 2))
            blk = xs[k][pos[c]:pos[c] + n]
            pos[c] += blk.size
            blocks.append(blk); end.append(pos[c] >= xs[k].size)
        got = s.push(blocks, end)
        for c in range(nc):
            if cur[c] is None:
                continue
            acc[c].append(got[c])
            if end[c]:
                outs[cur[c]] = np.concatenate(acc[c])
                acc[c], pos[c] = [], 0
                cur[c] = queue[c].pop(0) if queue[c] else None
    return [outs[k] for k in range(len(xs))]


@pytest.mark.parametrize("D", DIMS)
def test_paths_agree_bit_for_bit(pkg, D, parity_record):
    mean, istd = _norm(D)
    clean, noise = _corpus(D)
    c, s = _gv(D)
    post = dict(gv_center=c, gv_scale=s, mask_col=D, **GATE)
    plan = _plan(pkg, D, _frame_counts(D)[2])
    xs = WN.make_sentences(np.random.default_rng(50 + D), _lens(D))
    hop = D - 1
    g, fresh = _handle(pkg, D), _handle(pkg, D)
    try:
        for h in (g, fresh):
            h.set_mix_corpus(clean, noise, mean, istd, 3, 1, "lps+ibm")
        before = g.stream_open(mean, istd, 3, 1, n_chan=2, max_push_samples=8 * hop)       # opened before set_post
        assert before.post is False
        off_single = [g.enhance_waves([x], mean, istd, 3, 1)[0] for x in xs]
        g.set_post(**post)
        assert g.post is True
        # eval_mix is its parts
        ev = g.eval_mix(plan, FS, return_pcm=True)
        mix, _ = _mixtures(g, plan)
        enh = g.enhance_waves(mix, mean, istd, 3, 1)
        refs = [clean[k] for k in plan["clean"]]
        assert _same(ev["pcm"], enh)
        assert np.array_equal(_bits(ev["enhanced"]), _bits(pkg.score_waves(0, D, FS, refs, enh)))
        assert np.array_equal(_bits(ev["noisy"]), _bits(pkg.score_waves(0, D, FS, refs, mix)))
        ext = g.eval_mix(plan, FS, return_pcm=True, extended=True)
        assert _same(ext["pcm"], enh)
        assert not _same(enh, fresh.enhance_waves(mix, mean, istd, 3, 1))
        # a default stream and a packed stream, ragged pushes on two channels
        on_single = [g.enhance_waves([x], mean, istd, 3, 1)[0] for x in xs]
        st = g.stream_open(mean, istd, 3, 1, n_chan=2, max_push_samples=8 * hop)
        assert st.post is True and not st.packed
        assert _same(_stream_run(st, xs, np.random.default_rng(1), hop), on_single)
        g.set_forward(pkg.FORWARD_ROWINV)
        on_rowinv = [g.enhance_waves([x], mean, istd, 3, 1)[0] for x in xs]
        pk = g.stream_open(mean, istd, 3, 1, n_chan=2, max_push_samples=8 * hop)
        assert pk.post is True and pk.packed
        g.set_forward(pkg.FORWARD_DEFAULT)
        assert _same(_stream_run(pk, xs, np.random.default_rng(2), hop), on_rowinv)
        # the stream opened before set_post keeps the bits of the run with post-processing off; an open one keeps them on
        assert _same(_stream_run(before, xs, np.random.default_rng(3), hop), off_single)
        g.set_post(None)
        assert g.post is False
        assert _same(_stream_run(st, xs, np.random.default_rng(4), hop), on_single)
        for t in (before, st, pk):
            t.close()
        # after set_post(None): the bits of a fresh handle, call by call
        assert _same(g.enhance_waves(xs, mean, istd, 3, 1), fresh.enhance_waves(xs, mean, istd, 3, 1))
        a, b = g.eval_mix(plan, FS, return_pcm=True), fresh.eval_mix(plan, FS, return_pcm=True)
        assert _same(a["pcm"], b["pcm"]) and np.array_equal(_bits(a["enhanced"]), _bits(b["enhanced"]))
        assert _sums_equal(g.gv_mix(plan, stage="post"), fresh.gv_mix(plan)) == 0
        fs = fresh.stream_open(mean, istd, 3, 1, n_chan=2, max_push_samples=8 * hop)
        gs = g.stream_open(mean, istd, 3, 1, n_chan=2, max_push_samples=8 * hop)
        assert gs.post is False
        assert _same(_stream_run(gs, xs, np.random.default_rng(6), hop), _stream_run(fs, xs, np.random.default_rng(6), hop))
        parity_record(fea_dim=D, enhanced=ev["enhanced"].tolist())
    finally:
        g.close()
        fresh.close()


# ---- 6. training is unaffected
def test_training_is_unaffected(pkg):
    D = 33
    mean, istd = _norm(D)
    clean, noise = _corpus(D)
    c, s = _gv(D)
    plan = _plan(pkg, D, 129)
    got = []
    for with_post in (False, True):
        g = _handle(pkg, D, lrate=0.05, dropoutflag=1, visible_omit=0.1, hid_omit=0.2, seed=9)
        try:
            g.set_mix_corpus(clean, noise, mean, istd, 3, 1, "lps+ibm")
            if with_post:
                g.set_post(gv_center=c, gv_scale=s, mask_col=D, **GATE)
                g.gv_mix(plan, stage="post")
            g.train_mix(plan)
            cv = g.CrossValid_mix(plan)
            if with_post:
                g.eval_mix(plan, FS)
            g.train_mix(plan)
            got.append((g.get_weights(), g.get_deltas(), cv))
        finally:
            g.close()
    (w0, d0, cv0), (w1, d1, cv1) = got
    assert cv0 == cv1
    for a, b in zip(w0 + d0, w1 + d1):
        for x, y in zip(a, b):
            assert (x is None and y is None) or np.array_equal(_bits(x), _bits(y))


# ---- 7. every argument check; the handle is unchanged afterwards
def test_argument_checks_leave_the_handle_unchanged(pkg):
    D = 33
    mean, istd = _norm(D)
    clean, noise = _corpus(D)
    c, s = _gv(D)
    plan = _plan(pkg, D, 19)
    xs = WN.make_sentences(np.random.default_rng(8), [400])
    g, ref = _handle(pkg, D, lrate=0.05), _handle(pkg, D, lrate=0.05)
    try:
        with pytest.raises(pkg.BPError, match="status -3"):               # no corpus
            g.gv_mix(plan)
        for h in (g, ref):
            h.set_mix_corpus(clean, noise, mean, istd, 3, 1, "lps+ibm")
        good = dict(gv_center=c, gv_scale=s, mask_col=D, **GATE)
        g.set_post(**good)
        want = g.enhance_waves(xs, mean, istd, 3, 1)
        nan_c, zero_s, inf_s = c.copy(), s.copy(), s.copy()
        nan_c[4], zero_s[0], inf_s[D - 1] = np.nan, 0.0, np.inf
        bad = [dict(good, gv_center=nan_c), dict(good, gv_scale=zero_s), dict(good, gv_scale=inf_s), dict(good, gv_scale=-s),
               dict(good, mask_col=D + 1), dict(good, mask_col=-2), dict(good, mask_lo=0.8, mask_hi=0.2), dict(good, mask_weight=1.01),
               dict(good, mask_weight=-0.01), dict(good, mask_lo=np.nan), dict(good, mask_hi=np.inf), dict(good, mask_weight=np.nan),
               dict(good, gv_center=np.zeros(34, np.float32), gv_scale=np.ones(34, np.float32)),       # 2 (fea_dim - 1) no power of two
               dict(good, gv_center=np.zeros(65, np.float32), gv_scale=np.ones(65, np.float32))]       # mask_col + 65 > 2 D
        for kw in bad:
            with pytest.raises(pkg.BPError, match="status -1"):
                g.set_post(**kw)
            assert g.post is True
        with pytest.raises(pkg.BPError):
            g.set_post(gv_center=c)
        assert _same(g.enhance_waves(xs, mean, istd, 3, 1), want)        # the parameters of the last good call still hold
        # calls that resynthesise: another fea_dim, or the mask target
        with pytest.raises(pkg.BPError, match="status -1"):
            g.enhance_waves(xs, mean, istd, 3, 1, target=pkg.WAVE_MASK, out_col=D)
        with pytest.raises(pkg.BPError, match="status -1"):
            g.eval_mix(plan, FS, target=pkg.WAVE_MASK, out_col=D)
        with pytest.raises(pkg.BPError, match="status -1"):
            g.eval_mix(plan, FS, target=pkg.WAVE_MASK, out_col=D, extended=True)
        with pytest.raises(pkg.BPError, match="status -1"):
            g.stream_open(mean, istd, 3, 1, target=pkg.WAVE_MASK, out_col=D)
        g.set_post(mask_col=0, fea_dim=65, **GATE)                        # set for another fea_dim than the calls'
        with pytest.raises(pkg.BPError, match="fea_dim 65"):
            g.enhance_waves(xs, mean, istd, 3, 1)
        with pytest.raises(pkg.BPError, match="fea_dim 65"):
            g.eval_mix(plan, FS)
        with pytest.raises(pkg.BPError, match="fea_dim 65"):
            g.stream_open(mean, istd, 3, 1)
        with pytest.raises(pkg.BPError, match="fea_dim 65"):
            g.gv_mix(plan, stage="post")
        assert g.gv_mix(plan, stage="raw")["frames"] == 19
        g.set_post(**good)
        for kw in (dict(out_col=D + 1), dict(out_col=-1), dict(stage="raw", out_col=2 * D)):
            with pytest.raises(pkg.BPError, match="status -1"):
                g.gv_mix(plan, **kw)
        with pytest.raises(pkg.BPError):
            g.gv_mix(plan, stage="both")
        assert g.eval_mix_logmmse(plan, FS)["enhanced"].shape == (plan.size, 3)          # the log-MMSE calls do not read it
        g.set_post(None)
        for h in (g, ref):
            h.train_mix(plan)
        for x, y in zip(g.get_weights()[0], ref.get_weights()[0]):
            assert (x is None and y is None) or np.array_equal(_bits(x), _bits(y))
        assert _same(g.enhance_waves(xs, mean, istd, 3, 1), ref.enhance_waves(xs, mean, istd, 3, 1))
    finally:
        g.close()
        ref.close()


# ---- 8. the command-line tools: bpeval gv_out= -> bpenhance post_gv=, byte for byte what the Python calls give
def _write_pcm16(path, x, rate=FS):
    import wave
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(rate)
        w.writeframes(np.asarray(x, np.int16).tobytes())


def _pcm16_bytes(path):
    import wave
    with wave.open(str(path), "rb") as w:
        assert w.getnchannels() == 1 and w.getsampwidth() == 2 and w.getframerate() == FS
        return w.readframes(w.getnframes())


def _as_pcm16(y):
    """write_wav's conversion (csrc/host/wav_io.cpp): NaN 0, round to nearest even, clip"""
    y = np.where(np.isnan(y), np.float32(0), np.rint(y))
    return np.clip(y, -32768, 32767).astype(np.int16).tobytes()


@pytest.mark.parametrize("mode", ["indep", "dep"])
def test_tools_equal_the_python_calls(pkg, tmp_path, mode, parity_record):
    import pfile_util as PU
    D, cache = 33, 150
    exe = {k: str(pkg.LIB_PATH).replace("libbp_hip.so", k) for k in ("bpeval", "bpenhance")}
    clean, noise = _corpus(D)
    noise = [np.clip(x, -32768, 32767) for x in noise]
    mean, istd = _norm(D)
    for tag, xs in (("clean", clean), ("noise", noise)):
        for i, x in enumerate(xs):
            _write_pcm16(tmp_path / ("%s%d.wav" % (tag, i)), x)
        (tmp_path / (tag + ".list")).write_text("".join("%s\n" % (tmp_path / ("%s%d.wav" % (tag, i))) for i in range(len(xs))))
    (tmp_path / "x.norm").write_text("<mean>\n" + "".join("%.9g\n" % v for v in mean) + "<inverse std>\n" + "".join("%.9g\n" % v for v in istd))
    ls, W, b = _net(pkg, D)
    PU.write_wts(str(tmp_path / "net.wts"), ls, W, b)
    seed, snrs, per = 5, [-5.0, 0.0, 5.0], 2
    net_keys = ["norm_file=%s" % (tmp_path / "x.norm"), "initwts_file=%s" % (tmp_path / "net.wts"), "fea_dim=%d" % D, "fea_context=3",
                "targ_offset=1", "layersizes=%s" % ",".join(map(str, ls)), "bunchsize=32", "output_act=sigmoid", "output_linear_dims=%d" % D]
    r = subprocess.run([exe["bpeval"], "clean_list=%s" % (tmp_path / "clean.list"), "noise_list=%s" % (tmp_path / "noise.list"),
                        "snr_list=-5,0,5", "mix_per_clean=%d" % per, "init_randem_seed=%d" % seed, "traincache=%d" % cache,
                        "gv_out=%s" % (tmp_path / "gv.norm"), "gv_mode=%s" % mode] + net_keys, capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and r.stdout.startswith("bpeval: GV factor") and r.stdout.count("\n") == 1, r.stdout + r.stderr
    gv_line = r.stdout
    v = (tmp_path / "gv.norm").read_text().split("\n")
    got_c, got_s = np.array(v[1:1 + D], np.float32), np.array(v[2 + D:2 + 2 * D], np.float32)
    xs = [np.clip(x, -32768, 32767) for x in WN.make_sentences(np.random.default_rng(60), [3000, 31, 1, 500])]
    for i, x in enumerate(xs):
        _write_pcm16(tmp_path / ("in%d.wav" % i), x)
    post_keys = ["post_gv=%s" % (tmp_path / "gv.norm"), "post_mask_col=%d" % D, "post_mask_lo=0.3", "post_mask_hi=0.7", "post_mask_weight=0.8"]
    runs = {"off": [], "on": post_keys, "stream": post_keys + ["stream_block=77", "stream_chan=2"]}
    for tag, extra in runs.items():
        (tmp_path / (tag + ".list")).write_text("".join("%s %s\n" % (tmp_path / ("in%d.wav" % i), tmp_path / ("%s%d.wav" % (tag, i)))
                                                        for i in range(len(xs))))
        # (traincache 100: the 3000-sample file fills a call of its own, the other three share the next)
        r = subprocess.run([exe["bpenhance"], "wav_list=%s" % (tmp_path / (tag + ".list")), "traincache=100"] + net_keys + extra,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 1, r.stdout + r.stderr
    g = _handle(pkg, D, cap=cache)
    try:
        g.set_mix_corpus(clean, noise, mean, istd, 3, 1, "lps+irm")
        plan = pkg.mix_plan(seed, len(clean), per, [x.size for x in noise], snrs)
        T = g.mix_frames(plan) + 2                                       # the tools' cut: calls of at most traincache rows
        st, first, rows, calls = None, 0, 0, 0
        for i in range(len(plan) + 1):
            if i == len(plan) or rows + T[i] > cache:
                one = g.gv_mix(plan[first:i])
                st = one if st is None else {k: st[k] + one[k] for k in one}
                first, rows, calls = i, 0, calls + 1
            if i < len(plan):
                rows += T[i]
        assert calls > 1
        c, s = pkg.gv_factors(st, mode)
        assert np.array_equal(_bits(got_c), _bits(c)) and np.array_equal(_bits(got_s), _bits(s))
        assert ("of %d frames of %d mixtures" % (st["frames"], plan.size)) in gv_line, gv_line
        off = [g.enhance_waves(q, mean, istd, 3, 1) for q in ([xs[0]], xs[1:])]
        g.set_post(gv_center=c, gv_scale=s, mask_col=D, **GATE)
        on = [g.enhance_waves(q, mean, istd, 3, 1) for q in ([xs[0]], xs[1:])]
        single = [g.enhance_waves([x], mean, istd, 3, 1)[0] for x in xs]
    finally:
        g.close()
    off, on = off[0] + off[1], on[0] + on[1]
    differing = 0
    for i in range(len(xs)):
        assert _pcm16_bytes(tmp_path / ("off%d.wav" % i)) == _as_pcm16(off[i])
        assert _pcm16_bytes(tmp_path / ("on%d.wav" % i)) == _as_pcm16(on[i])
        assert _pcm16_bytes(tmp_path / ("stream%d.wav" % i)) == _as_pcm16(single[i])
        differing += _as_pcm16(on[i]) != _as_pcm16(off[i])
    assert differing >= 3
    parity_record(gv_mode=mode, scale_min=float(s.min()), scale_max=float(s.max()), frames=st["frames"])
