"""GPU tests of the row-invariant inference forward (bp_set_forward: BP_FORWARD_ROWINV, bp_infer.hip; -m gpu) and of the streams
that pack their channels on it.

The contract under test: in ROWINV a frame's output row is a function of the bits of its stacked input row, the weights and the
forward's settings alone -- not of its row in the chunk, the number of rows, the handle's bunch, the other rows or the entry point.
Every such comparison is np.array_equal on the uint32 view.  Against the CPU oracle's CV forward the bar is the 1e-4 of
tests/test_gpu_parity.py (max|a - ref| / max|ref|), and on data whose arithmetic is exact (tests/infer_np.py, the recipe of
tests/exact_data.py) np.array_equal: the test that sees a dropped or doubled k-slice.

Which case reaches which kernel and branch of the dispatch (restated in tests/infer_np.py; tests/test_infer_host.py holds the list
against the built library):
  net S  264-96-33 (the net of tests/test_stream_gpu.py): bp_infer_layer<false> -- no k-slices (K = 320, 128), a half-empty last
         column tile (N = 64), row tiles that end inside (bunch 7, 100 = 3 x 32 + 4 rows)
  net W  1548-2048-2048-129: bp_infer_layer<true> -- 8 k-slices on every layer, partial sums without k-rows (K = 1600), several row
         tiles per launch (bunch 64 and 256), whole and half column tiles (N = 2048, 192)
  net M  1000-4096-570-129: bp_infer_layer<true> with 4, 8 and 2 k-slices in ONE net -- the read-back of fewer than 8 slices,
         layers that lay their slices out at different strides in the shared slab (the widest layer has the fewest slices), ticket
         words per layer, and uneven partial sums (K = 576: 36 units over 8 partial sums of 5, the last holds one unit)
  S66    net S with the 66-wide output: the logistic output columns."""
import numpy as np
import pytest

import exact_data as ED
import infer_np as IN
import test_eval_gpu as TE
import test_stream_gpu as TS
import wave_np as WN

pytestmark = pytest.mark.gpu

FD = TS.FD
BAR = 1e-4
NETS = {"S": dict(ls=IN.NET_S, D=33, ctx=7, B=32, B2=7, seed=21), "W": dict(ls=IN.NET_W, D=129, ctx=11, B=64, B2=256, seed=3),
        "M": dict(ls=IN.NET_M, D=125, ctx=7, B=64, B2=256, seed=5)}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _relerr(a, ref):
    return float(np.abs(np.asarray(a, np.float64) - ref).max() / np.abs(ref).max())


def _handle(pkg, ls, W, b, B, cap=1024, mode=None, **kw):
    return pkg.BP_GPU(1, len(ls), ls, B, kw.pop("lrate", 0.0), kw.pop("momentum", 0.0), 0.0, W, b, max_chunk_frames=cap,
                      forward_mode=pkg.FORWARD_ROWINV if mode is None else mode, **kw)


def _forward_windows(pkg, g, fea, ctx, ws, nat, nr):
    """bp_forward_windows: sample i = fea[ws[i] : ws[i] + ctx] stacked, then nat[nr[i]]."""
    import ctypes as C
    zt = np.zeros((fea.shape[0], g.layersizes[-1]), np.float32)
    c, keep = g._windows(fea, zt, ctx, ws, np.zeros(ws.size, np.int32), nat, nr)
    out = np.empty((ws.size, g.layersizes[-1]), np.float32)
    g._check(g._lib.bp_forward_windows(g._h, C.byref(c), out.ctypes.data_as(C.POINTER(C.c_float))))
    return out


# ---- 1. invariance
@pytest.mark.parametrize("net", ["S", "W", "M"])
def test_invariance(pkg, net, parity_record):
    cf = NETS[net]
    ls, D, ctx = cf["ls"], cf["D"], cf["ctx"]
    W, b = pkg.glorot_net(ls, seed=cf["seed"], beta=0.5)
    rng = np.random.default_rng(31)
    n = 100
    fea = rng.standard_normal((n + ctx + 4, D)).astype(np.float32)
    nat = rng.standard_normal((3, D)).astype(np.float32)
    ws = rng.integers(0, fea.shape[0] - ctx + 1, n).astype(np.int32)
    nr = rng.integers(0, 3, n).astype(np.int32)
    X = np.concatenate([fea[ws[:, None] + np.arange(ctx)].reshape(n, ctx * D), nat[nr]], axis=1)
    assert X.shape == (n, ls[0])
    g = _handle(pkg, ls, W, b, cf["B"])
    g2 = _handle(pkg, ls, W, b, cf["B2"], cap=512)
    try:
        ref = g.forward(X)
        assert np.isfinite(ref).all() and np.unique(ref).size > n
        assert _same(g.forward(X), ref), "a second run of the same call"
        perm = rng.permutation(n)
        assert _same(g.forward(X[perm]), ref[perm]), "permuted rows"
        alone = np.concatenate([g.forward(X[k:k + 1]) for k in range(n)])
        assert _same(alone, ref), "each row alone: %d rows differ" % int((_bits(alone) != _bits(ref)).any(axis=1).sum())
        for k in (1, 31, 32, 33, 64, 65):
            assert _same(g.forward(X[n - k:]), ref[n - k:]), "a call of %d rows" % k
        assert _same(g2.forward(X), ref), "a handle of bunch size %d" % cf["B2"]
        assert _same(_forward_windows(pkg, g, fea, ctx, ws, nat, nr), ref), "bp_forward_windows on the same stacked rows"
        assert _same(_forward_windows(pkg, g2, fea, ctx, ws, nat, nr), ref)
        assert _same(g.forward(X), ref), "the first comparison once more"
        # what the mode is for: the default forward's bits do depend on the row (not asserted: a property of the other kernels)
        g.set_forward(pkg.FORWARD_DEFAULT)
        d_all = g.forward(X)
        d_alone = np.concatenate([g.forward(X[k:k + 1]) for k in range(0, n, 5)])
        parity_record(rowinv_vs_default_max_rel=_relerr(ref, d_all.astype(np.float64)),
                      default_rows_that_move_when_alone=int((_bits(d_alone) != _bits(d_all[::5])).any(axis=1).sum()), of_rows=int(d_alone.shape[0]))
    finally:
        g.close()
        g2.close()


# ---- 2. parity with the CPU oracle
PARITY = {
    "S relu": dict(net="S", act=0),
    "S sigmoid dropout": dict(net="S", act=1, drop=True),
    "S66 relu dropout logistic": dict(net="S66", act=0, drop=True, out=(1, 0)),
    "S66 sigmoid logistic upper half": dict(net="S66", act=1, out=(1, FD)),
    "W relu dropout": dict(net="W", act=0, drop=True),
    "W sigmoid": dict(net="W", act=1),
    "M relu dropout": dict(net="M", act=0, drop=True),
    "M sigmoid": dict(net="M", act=1),
}


@pytest.mark.parametrize("name", list(PARITY))
def test_parity(pkg, oracle_mod, name, parity_record):
    cf = PARITY[name]
    ls = IN.NET_S66 if cf["net"] == "S66" else NETS[cf["net"]]["ls"]
    B = 64 if cf["net"] in ("W", "M") else 32
    W, b = pkg.glorot_net(ls, seed=9, beta=0.5)
    x = np.random.default_rng(5).standard_normal((65, ls[0])).astype(np.float32)
    kw = dict(dropoutflag=1, visible_omit=0.1, hid_omit=0.2) if cf.get("drop") else {}
    o = oracle_mod.Oracle(ls, B, 1.0, 0.5, 0.0, W, b, activation=cf["act"], **kw)
    ref = o.forward(x).astype(np.float64)
    out = cf.get("out")
    if out:
        z = ref[:, out[1]:].astype(np.float32)
        ref[:, out[1]:] = np.float32(1.0) / (np.float32(1.0) + np.exp(-z))
    g = _handle(pkg, ls, W, b, B, activation=cf["act"], **kw)
    try:
        if out:
            g.set_output(out[0], out[1], 0)
        got = g.forward(x)
    finally:
        g.close()
    err = _relerr(got, ref)
    print("%s: max|a - ref| / max|ref| = %.3g" % (name, err))
    parity_record(case=name, err=err, bar=BAR)
    assert err < BAR, (name, err)


@pytest.mark.parametrize("net", ["S", "W", "M"])
def test_exact(pkg, oracle_mod, net, parity_record):
    """Integer weights, half-integer inputs and biases, no dropout, ReLU: every partial sum in every order is an fp32 number
    (tests/test_infer_host.py checks the conditions), so the device equals the oracle bit for bit -- unless a k-slice, a unit or a
    partial sum is dropped or added twice."""
    ls, B = NETS[net]["ls"], NETS[net]["B"]
    W, b = IN.exact_net(ls, 1)
    x = IN.exact_inputs(ls, 65, 1)
    ref = oracle_mod.Oracle(ls, B, 1.0, 0.5, 0.0, W, b, activation=0).forward(x)
    assert np.array_equal(ref.astype(np.float64), IN.exact_forward(ls, W, b, x)[0])
    g = _handle(pkg, ls, W, b, B)
    try:
        got = g.forward(x)
        alone = np.concatenate([g.forward(x[k:k + 1]) for k in (0, 31, 32, 64)])
    finally:
        g.close()
    parity_record(unequal=ED.count_unequal(got, ref), of=int(ref.size))
    assert ED.unequal("forward", got, ref) is None, ED.unequal("forward", got, ref)
    assert np.array_equal(alone, ref[[0, 31, 32, 64]])


# ---- 3. the offline signal path
@pytest.mark.parametrize("target", ["lps", "mask"])
def test_enhance_waves_together_equals_alone(pkg, target):
    ctx, toff, hop = 7, 3, FD - 1
    mask = target == "mask"
    ls, W, b = TS._net(pkg, FD, ctx, True, out_mult=2 if mask else 1)
    hkw = dict(output_activation=1, output_linear_cols=FD) if mask else {}
    kw = dict(target=pkg.WAVE_MASK, out_col=FD) if mask else {}
    g = _handle(pkg, ls, W, b, 32, cap=2048, **hkw)
    m, i = TS._stats(FD)
    xs = WN.make_sentences(np.random.default_rng(8), [1, 5 * hop, 6 * hop - 1, hop + 1, 12 * hop + 7, 3 * hop])
    try:
        pcm, net = g.enhance_waves(xs, m, i, ctx, toff, return_net=True, **kw)
        for k, x in enumerate(xs):
            p1, n1 = g.enhance_waves([x], m, i, ctx, toff, return_net=True, **kw)
            assert _same(pcm[k], p1[0]), "out_pcm of sentence %d" % k
            assert _same(net[k], n1[0]), "out_net of sentence %d" % k
    finally:
        g.close()


def test_eval_mix_is_its_parts_in_rowinv(pkg):
    rng = np.random.default_rng(11)
    clean, noise = TE._corpus(rng)
    mean, istd = TE._norm(rng)
    plan = TE._plan(pkg)
    g = TE._handle(pkg, True, False)
    try:
        g.set_forward(pkg.FORWARD_ROWINV)
        g.set_mix_corpus(clean, noise, mean, istd, TE.CTX, TE.TOFF, "lps+irm")
        ev = g.eval_mix(plan, TE.FS, pkg.WAVE_MASK, TE.D, return_pcm=True)
        lens = [clean[c].size for c in plan["clean"]]
        mix = np.split(g.mix_features(plan)["pcm"], np.cumsum(lens)[:-1])
        enh = g.enhance_waves(mix, mean, istd, TE.CTX, TE.TOFF, pkg.WAVE_MASK, TE.D)
        alone = [g.enhance_waves([x], mean, istd, TE.CTX, TE.TOFF, pkg.WAVE_MASK, TE.D)[0] for x in mix]
        refs = [clean[c] for c in plan["clean"]]
        for a, b_, c in zip(ev["pcm"], enh, alone):
            assert _same(a, b_) and _same(a, c)
        assert _same(ev["noisy"], pkg.score_waves(0, TE.D, TE.FS, refs, mix))
        assert _same(ev["enhanced"], pkg.score_waves(0, TE.D, TE.FS, refs, enh))
    finally:
        g.close()


# ---- 4. streams
@pytest.fixture(scope="module")
def stream_case(pkg):
    """Net S in ROWINV; the yardstick twice: every sentence in a call of its own, and all of them in one call."""
    ctx, toff = 7, 3
    ls, W, b = TS._net(pkg, FD, ctx, True)
    g = _handle(pkg, ls, W, b, 32, cap=2048)
    m, i = TS._stats(FD)
    xs = WN.make_sentences(np.random.default_rng(1), TS.LENGTHS)
    ref = TS._offline(g, xs, m, i, ctx, toff)
    ref_all = g.enhance_waves(xs, m, i, ctx, toff)
    for r in ref + ref_all:
        r.setflags(write=False)
    yield dict(g=g, m=m, i=i, ctx=ctx, toff=toff, xs=xs, ref=ref, ref_all=ref_all)
    g.close()


@pytest.mark.parametrize("schedule", ["hop", "ragged", "single"])
@pytest.mark.parametrize("n_chan", [1, 3, 8])
def test_packed_stream_same_bits(pkg, stream_case, n_chan, schedule, parity_record):
    c1 = stream_case
    keep = [k for k, x in enumerate(c1["xs"]) if schedule != "single" or x.size <= 192]
    xs = [c1["xs"][k] for k in keep]
    chans = TS._deal(xs, n_chan)
    s = c1["g"].stream_open(c1["m"], c1["i"], c1["ctx"], c1["toff"], n_chan=n_chan, max_push_samples=8192)
    try:
        assert s.packed
        feed = TS._Feed(pkg, s, FD, c1["ctx"], c1["toff"], True)            # (checks n_out against stream_counts after every push)
        feed.play(TS._plans(chans, schedule, FD - 1, np.random.default_rng(17)))
        TS._check(feed, chans, TS._deal([c1["ref"][k] for k in keep], n_chan))
        TS._check(feed, chans, TS._deal([c1["ref_all"][k] for k in keep], n_chan))
    finally:
        s.close()
    parity_record(pushes=feed.pushes, sentences=len(xs))


def test_packed_lockstep_channels_on_a_small_chunk(pkg, parity_record):
    ctx, toff = 7, 3
    ls, W, b = TS._net(pkg, FD, ctx, True)
    g = _handle(pkg, ls, W, b, 32, cap=64)
    m, i = TS._stats(FD)
    xs = WN.make_sentences(np.random.default_rng(14), [400, 400, 400, 400])
    try:
        ref = TS._offline(g, xs, m, i, ctx, toff)
        s = g.stream_open(m, i, ctx, toff, n_chan=4, max_push_samples=4 * (FD - 1))
        feed = TS._Feed(pkg, s, FD, ctx, toff, True)
        feed.play(TS._plans([[x] for x in xs], "hop", FD - 1, None))
        TS._check(feed, [[x] for x in xs], [[r] for r in ref])
        s.close()
    finally:
        g.close()
    parity_record(pushes=feed.pushes)


def test_streams_of_both_modes_on_one_handle(pkg):
    """A stream keeps the mode of its bp_stream_open: bp_set_forward between the pushes changes neither."""
    ctx, toff = 7, 3
    ls, W, b = TS._net(pkg, FD, ctx, True)
    g = _handle(pkg, ls, W, b, 32, cap=2048, mode=pkg.FORWARD_DEFAULT)
    m, i = TS._stats(FD)
    rng = np.random.default_rng(6)
    xs = WN.make_sentences(rng, [333, 1200, 700])
    try:
        ref_d = TS._offline(g, xs, m, i, ctx, toff)
        a = g.stream_open(m, i, ctx, toff, n_chan=3, max_push_samples=4096)
        g.set_forward(pkg.FORWARD_ROWINV)
        ref_r = TS._offline(g, xs, m, i, ctx, toff)
        b_ = g.stream_open(m, i, ctx, toff, n_chan=3, max_push_samples=4096)
        assert not a.packed and b_.packed
        fa, fb = TS._Feed(pkg, a, FD, ctx, toff, True), TS._Feed(pkg, b_, FD, ctx, toff, True)
        plans = TS._plans([[x] for x in xs], "hop", FD - 1, None)
        for k in range(max(len(p) for p in plans)):
            items = [p[k] if k < len(p) else None for p in plans]
            g.set_forward(pkg.FORWARD_ROWINV if k % 2 else pkg.FORWARD_DEFAULT)
            fa.push(items)
            if k % 3 == 0:
                g.set_forward(pkg.FORWARD_DEFAULT if k % 2 else pkg.FORWARD_ROWINV)
            fb.push(items)
        assert not a.packed and b_.packed
        TS._check(fa, [[x] for x in xs], [[r] for r in ref_d])
        TS._check(fb, [[x] for x in xs], [[r] for r in ref_r])
    finally:
        g.close()


def test_wide_net_eight_lockstep_channels(pkg, parity_record):
    """Net W (every layer k-split): 8 feeds in lockstep, one hop per push -- the start of a sentence and 20 pushes behind it."""
    D, ctx, toff = 129, 11, 5
    hop = D - 1
    ls = IN.NET_W
    W, b = pkg.glorot_net(ls, seed=3, beta=0.5)
    g = _handle(pkg, ls, W, b, 64, cap=1024)
    m, i = TS._stats(D)
    xs = WN.make_sentences(np.random.default_rng(2), [(6 + toff + 20) * hop + 5 * k for k in range(8)])
    try:
        ref = g.enhance_waves(xs, m, i, ctx, toff)
        s = g.stream_open(m, i, ctx, toff, n_chan=8, max_push_samples=8 * hop)
        feed = TS._Feed(pkg, s, D, ctx, toff, True)
        feed.play(TS._plans([[x] for x in xs], "hop", hop, None))
        TS._check(feed, [[x] for x in xs], [[r] for r in ref])
        s.close()
    finally:
        g.close()
    parity_record(pushes=feed.pushes)


# ---- 5. nothing else moves
def test_training_and_cv_do_not_depend_on_the_mode(pkg):
    ls, B = [264, 96, 33], 32
    W, b = pkg.glorot_net(ls, seed=4, beta=0.5)
    rng = np.random.default_rng(15)
    x = rng.standard_normal((3 * B, ls[0])).astype(np.float32)
    t = rng.standard_normal((3 * B, ls[-1])).astype(np.float32)
    xf = rng.standard_normal((40, ls[0])).astype(np.float32)
    kw = dict(dropoutflag=1, visible_omit=0.1, hid_omit=0.2, seed=77, lrate=0.05, momentum=0.5)
    g0 = _handle(pkg, ls, W, b, B, mode=pkg.FORWARD_DEFAULT, **kw)
    g1 = _handle(pkg, ls, W, b, B, **kw)
    try:
        res = []
        for g in (g0, g1):
            g.forward(xf)
            g.train(3 * B, x, t)
            g.forward(xf)
            cv = g.CrossValid(3 * B, x, t)
            res.append((g.get_weights(), g.get_deltas(), cv))
        (w0, d0, cv0), (w1, d1, cv1) = res
        assert np.float32(cv0).view(np.uint32) == np.float32(cv1).view(np.uint32), (cv0, cv1)
        for A, Bv in ((w0, w1), (d0, d1)):
            for u, v in zip(A[0][1:] + A[1][1:], Bv[0][1:] + Bv[1][1:]):
                assert _same(u, v)
        g1.set_forward(pkg.FORWARD_DEFAULT)
        assert _same(g1.forward(xf), g0.forward(xf))
    finally:
        g0.close()
        g1.close()


# ---- 6. errors leave the handle as it was
def test_errors_and_the_handle_goes_on(pkg):
    ctx, toff = 7, 3
    ls, W, b = TS._net(pkg, FD, ctx, True)
    m, i = TS._stats(FD)
    x = np.random.default_rng(1).standard_normal((5, ls[0])).astype(np.float32)
    g = _handle(pkg, ls, W, b, 32, mode=pkg.FORWARD_DEFAULT)
    gb = _handle(pkg, ls, W, b, 32, mode=pkg.FORWARD_DEFAULT, compute_dtype=1)
    try:
        d = g.forward(x)
        for bad in (2, -1, 7):
            with pytest.raises(pkg.BPError, match="status -1"):
                g.set_forward(bad)
            assert g.forward_mode == pkg.FORWARD_DEFAULT and _same(g.forward(x), d)
        g.set_forward(pkg.FORWARD_ROWINV)
        r = g.forward(x)
        with pytest.raises(pkg.BPError, match="status -1"):
            g.set_forward(3)
        assert g.forward_mode == pkg.FORWARD_ROWINV and _same(g.forward(x), r)
        assert pkg.load_library().bp_set_forward(None, 1) == -1
        fb = gb.forward(x)
        with pytest.raises(pkg.BPError, match="fp32.*status -1"):
            gb.set_forward(pkg.FORWARD_ROWINV)
        assert _same(gb.forward(x), fb)
        gb.set_forward(pkg.FORWARD_DEFAULT)
        with pytest.raises(pkg.BPError, match="status -1"):
            _handle(pkg, ls, W, b, 32, compute_dtype=1)
        s1 = g.stream_open(m, i, ctx, toff)
        g.set_forward(pkg.FORWARD_DEFAULT)
        s0 = g.stream_open(m, i, ctx, toff)
        g.set_forward(pkg.FORWARD_ROWINV)
        assert s1.packed and not s0.packed
        with pytest.raises(AttributeError):
            s1.packed = False
        # the property is the library's answer, not the Python mirror of the mode: set the mode behind the mirror's back
        lib = pkg.load_library()
        assert lib.bp_set_forward(g._h, pkg.FORWARD_DEFAULT) == 0 and g.forward_mode == pkg.FORWARD_ROWINV
        s2 = g.stream_open(m, i, ctx, toff)
        assert not s2.packed and lib.bp_stream_packed(s2._s) == 0 and lib.bp_stream_packed(s1._s) == 1 and lib.bp_stream_packed(None) == 0
    finally:
        g.close()
        gb.close()


# ---- 7. bpenhance forward=rowinv
def test_bpenhance_rowinv_same_bytes(pkg, tmp_path):
    import subprocess
    import wave
    import pfile_util as PU
    exe = str(pkg.LIB_PATH).replace("libbp_hip.so", "bpenhance")
    ctx, toff = 7, 3
    ls, W, b = TS._net(pkg, FD, ctx, True)
    m, i = TS._stats(FD)
    PU.write_wts(str(tmp_path / "net.wts"), ls, W, b)
    PU.write_norm(str(tmp_path / "x.norm"), m, i)
    xs = WN.make_sentences(np.random.default_rng(10), [1234, 1000, 900])
    for k, x in enumerate(xs):
        with wave.open(str(tmp_path / ("in%d.wav" % k)), "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(8000)
            w.writeframes(np.asarray(x, np.int16).tobytes())
    g = _handle(pkg, ls, W, b, 32, cap=2048)
    try:
        xr = [np.asarray(x, np.int16).astype(np.float32) for x in xs]
        want = [np.clip(np.rint(y), -32768, 32767).astype(np.int16).tobytes() for y in g.enhance_waves(xr, m, i, ctx, toff)]
    finally:
        g.close()
    # (traincache 2048: the offline run holds the three files in ONE call; the stream deals them to two channels)
    for tag, extra in (("off", []), ("on", ["stream_block=100", "stream_chan=2"])):
        (tmp_path / (tag + ".list")).write_text("".join("%s %s\n" % (tmp_path / ("in%d.wav" % k), tmp_path / ("%s%d.wav" % (tag, k)))
                                                        for k in range(len(xs))))
        r = subprocess.run([exe, "norm_file=%s" % (tmp_path / "x.norm"), "initwts_file=%s" % (tmp_path / "net.wts"),
                            "layersizes=%s" % ",".join(map(str, ls)), "fea_dim=%d" % FD, "fea_context=%d" % ctx, "targ_offset=%d" % toff,
                            "wav_list=%s" % (tmp_path / (tag + ".list")), "traincache=2048", "bunchsize=32", "forward=rowinv"] + extra,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 1, r.stdout + r.stderr
        got = [open(tmp_path / ("%s%d.wav" % (tag, k)), "rb").read()[44:] for k in range(len(xs))]
        assert got == want, tag
