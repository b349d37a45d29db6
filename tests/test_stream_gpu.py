"""GPU tests of the streaming sessions (bp_stream_open / _push / _close; -m gpu).  The yardstick is exact: a sentence pushed in
blocks of ANY sizes returns the same bits as ONE enhance_waves call on the finished sentence on the SAME handle: a frame's net
output does not depend on which rows share its bunch, only on its own row in it (which the stream reproduces), and analysis,
synthesis and overlap-add are per frame.  The reference is therefore one call per sentence (_offline): the same sentence behind
others in one call sits at other rows and may differ in the last bit.  Every comparison is np.array_equal on the uint32 view.
After every push the samples returned per channel equal stream_counts."""
import os

import numpy as np
import pytest

import stream_np as SN
import wave_np as WN

pytestmark = pytest.mark.gpu

FD = 33                                                   # n_fft 64, hop 32
LENGTHS = [1, 31, 32, 33, 160, 191, 192, 1000]            # T < 6 (the NAT clamp), hop multiples and one sample either side


def _net(pkg, fea_dim, ctx, nat, hidden=96, out_mult=1, seed=21):
    ls = [(ctx + (1 if nat else 0)) * fea_dim, hidden, out_mult * fea_dim]
    W, b = pkg.glorot_net(ls, seed=seed, beta=0.5)
    return ls, W, b


def _handle(pkg, ls, W, b, B=32, cap=2048, lrate=0.0, **kw):
    return pkg.BP_GPU(1, len(ls), ls, B, lrate, 0.0, 0.0, W, b, max_chunk_frames=cap, **kw)


def _stats(fea_dim, seed=5):
    xs = WN.make_sentences(np.random.default_rng(seed), [40 * (fea_dim - 1)])
    m, i = WN.norm_stats(xs, fea_dim)
    return m.astype(np.float32), i.astype(np.float32)


def _offline(g, xs, m, i, ctx, toff, **kw):
    """One enhance_waves call per finished sentence."""
    return [g.enhance_waves([x], m, i, ctx, toff, **kw)[0] for x in xs]


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _blocks(x, sizes, end_alone):
    """A sentence as a list of (block, end) pushes: blocks of the given sizes, the end flag on the last block or in a push of its own."""
    out, p = [], 0
    for k in sizes:
        out.append((x[p:p + k], False))
        p += k
    assert p == x.size
    if end_alone:
        out.append((x[:0], True))
    else:
        out[-1] = (out[-1][0], True)
    return out


class _Feed(object):
    """Drives one stream: every channel plays its list of (block, end) pushes; checks n_out against stream_counts after every
    push and collects the output per channel and sentence."""

    def __init__(self, pkg, stream, fea_dim, ctx, toff, nat):
        self.pkg, self.s, self.cfg = pkg, stream, (fea_dim, ctx, toff, nat)
        self.received = [0] * stream.n_chan
        self.out = [[[]] for _ in range(stream.n_chan)]
        self.pushes = 0

    def push(self, items, **kw):
        """items: per channel (block, end) or None."""
        items = [(np.zeros(0, np.float32), False) if it is None else it for it in items]
        got = self.s.push([b for b, _ in items], [e for _, e in items], **kw)
        self.pushes += 1
        for c, ((b, e), y) in enumerate(zip(items, got)):
            before = SN.counts(*self.cfg, self.received[c], False)[2]
            self.received[c] += b.size
            ended = bool(e) and self.received[c] > 0
            after = self.pkg.stream_counts(*self.cfg, self.received[c], ended)
            assert after == SN.counts(*self.cfg, self.received[c], ended)
            assert y.size == after[2] - before, (c, self.received[c], ended, y.size, after, before)
            self.out[c][-1].append(y)
            if ended:
                self.received[c] = 0
                self.out[c].append([])
        return got

    def play(self, plans):
        """plans: per channel a list of (block, end); channels advance in lockstep, one item per push."""
        for k in range(max(len(p) for p in plans)):
            self.push([p[k] if k < len(p) else None for p in plans])

    def sentences(self, c):
        return [np.concatenate(s) if s else np.zeros(0, np.float32) for s in self.out[c][:-1]]


def _deal(xs, n_chan):
    return [xs[c::n_chan] for c in range(n_chan)]


def _plans(chans, schedule, hop, rng):
    plans = []
    for sents in chans:
        p = []
        for x in sents:
            if schedule == "one":
                p += _blocks(x, [x.size], False)
            elif schedule == "hop":
                p += _blocks(x, [hop] * (x.size // hop) + ([x.size % hop] if x.size % hop else []), False)
            elif schedule == "single":
                p += _blocks(x, [1] * x.size, False)
            else:
                p += _blocks(x, SN.ragged_schedule(rng, x.size, hop), True)
        plans.append(p)
    return plans


def _check(feed, chans, ref_chans):
    for c, (sents, refs) in enumerate(zip(chans, ref_chans)):
        got = feed.sentences(c)
        assert len(got) == len(sents), (c, len(got), len(sents))
        for k, (y, r) in enumerate(zip(got, refs)):
            assert _same_bits(y, r), "channel %d sentence %d (%d samples): %d samples differ" % (
                c, k, r.size, int((y.view(np.uint32) != r.view(np.uint32)).sum()) if y.size == r.size else -1)


# ---- 1. any chunking gives the same bits
@pytest.fixture(scope="module")
def case1(pkg):
    ctx, toff = 7, 3
    ls, W, b = _net(pkg, FD, ctx, True)
    g = _handle(pkg, ls, W, b)
    m, i = _stats(FD)
    xs = WN.make_sentences(np.random.default_rng(1), LENGTHS)
    ref = _offline(g, xs, m, i, ctx, toff)
    yield dict(g=g, m=m, i=i, ctx=ctx, toff=toff, xs=xs, ref=ref)
    g.close()


@pytest.mark.parametrize("schedule", ["one", "hop", "single", "ragged"])
def test_any_chunking_same_bits(pkg, case1, schedule, parity_record):
    c1 = case1
    keep = [k for k, x in enumerate(c1["xs"]) if schedule != "single" or x.size <= 192]
    xs, ref = [c1["xs"][k] for k in keep], [c1["ref"][k] for k in keep]
    chans, ref_chans = _deal(xs, 3), _deal(ref, 3)
    s = c1["g"].stream_open(c1["m"], c1["i"], c1["ctx"], c1["toff"], n_chan=3, max_push_samples=4096)
    try:
        feed = _Feed(pkg, s, FD, c1["ctx"], c1["toff"], True)
        feed.play(_plans(chans, schedule, FD - 1, np.random.default_rng(17)))
        _check(feed, chans, ref_chans)
    finally:
        s.close()
    parity_record(pushes=feed.pushes, sentences=len(xs))


# ---- 2. other configurations
CONFIGS = {
    "no_nat":   dict(ctx=7, toff=3, nat=False),
    "ctx1":     dict(ctx=1, toff=0, nat=True),
    "toff0":    dict(ctx=7, toff=0, nat=True),
    "toff6":    dict(ctx=7, toff=6, nat=True),
    "mask_col": dict(ctx=7, toff=3, nat=True, out_mult=2, target="mask", hkw=dict(output_activation=1, output_linear_cols=FD)),
    "fea129":   dict(ctx=7, toff=3, nat=True, fea_dim=129, hidden=128),
    "bf16":     dict(ctx=7, toff=3, nat=True, hkw=dict(compute_dtype=1)),
}
# The other frame sizes (tests/geometry_cases.py): two workgroups per noise-aware row at 257, three at 513, five at 1025, and the
# large LDS layout of bp_stream_synthesis.  `mask`: the mask block of a [LPS | mask] output layer, read at the odd column offset D
# of a padded row.  `packed`: the stream is opened after set_forward(FORWARD_ROWINV).
for _D in (65, 257, 513, 1025):
    CONFIGS["fea%d" % _D] = dict(ctx=7, toff=3, nat=True, fea_dim=_D, hidden=128)
for _D in (257, 1025):
    CONFIGS["fea%d_mask" % _D] = dict(ctx=7, toff=3, nat=True, fea_dim=_D, hidden=128, out_mult=2, target="mask", mask=True)
for _D in (65, 129, 257, 513, 1025):
    CONFIGS["fea%d_packed" % _D] = dict(ctx=7, toff=3, nat=True, fea_dim=_D, hidden=128, packed=True)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_other_configurations(pkg, name, parity_record):
    cf = CONFIGS[name]
    D, ctx, toff, nat = cf.get("fea_dim", FD), cf["ctx"], cf["toff"], cf["nat"]
    hop = D - 1
    ls, W, b = _net(pkg, D, ctx, nat, hidden=cf.get("hidden", 96), out_mult=cf.get("out_mult", 1))
    hkw = dict(output_activation=1, output_linear_cols=D) if cf.get("mask") else cf.get("hkw", {})
    g = _handle(pkg, ls, W, b, **hkw)
    m, i = _stats(D)
    target = pkg.WAVE_MASK if cf.get("target") == "mask" else pkg.WAVE_LPS
    out_col = D if cf.get("out_mult", 1) == 2 else 0
    rng = np.random.default_rng(len(name))
    xs = WN.make_sentences(rng, [1, 5 * hop, 6 * hop - 1, hop + 1, 12 * hop + 7, 3 * hop])
    try:
        if cf.get("packed"):
            g.set_forward(pkg.FORWARD_ROWINV)
        ref = _offline(g, xs, m, i, ctx, toff, target=target, out_col=out_col)
        assert all(r.size == x.size and np.isfinite(r).all() for r, x in zip(ref, xs)) and any(r.any() for r in ref)
        chans, ref_chans = _deal(xs, 2), _deal(ref, 2)
        s = g.stream_open(m, i, ctx, toff, target=target, out_col=out_col, n_chan=2, max_push_samples=32 * hop)
        assert bool(s.packed) == bool(cf.get("packed"))
        feed = _Feed(pkg, s, D, ctx, toff, nat)
        feed.play(_plans(chans, "ragged", hop, rng))
        _check(feed, chans, ref_chans)
        s.close()
    finally:
        g.close()
    parity_record(pushes=feed.pushes, fea_dim=D, sentences=len(xs), samples_differing=0)


# ---- 3. channel reuse and independence
def test_channel_reuse_and_idle_channel(pkg, case1, parity_record):
    c1 = case1
    g, hop = c1["g"], FD - 1
    rng = np.random.default_rng(3)
    xs = WN.make_sentences(rng, [900, 200, 33, 260, 700])
    ref = _offline(g, xs, c1["m"], c1["i"], c1["ctx"], c1["toff"])
    chans = [[xs[0]], [xs[1], xs[2], xs[3]], [xs[4]]]              # channel 1 runs three sentences while 0 and 2 are mid-sentence
    ref_chans = [[ref[0]], [ref[1], ref[2], ref[3]], [ref[4]]]
    plans = [_blocks(xs[0], [50] * 18, False),
             _blocks(xs[1], [40] * 5, False) + _blocks(xs[2], [33], True) + _blocks(xs[3], [65] * 4, False),
             # channel 2: a start, then nothing for many pushes, then the rest
             [(xs[4][:100], False)] + [(xs[4][:0], False)] * 9 + _blocks(xs[4][100:], [300, 300], True)]
    s = g.stream_open(c1["m"], c1["i"], c1["ctx"], c1["toff"], n_chan=3, max_push_samples=1024)
    try:
        feed = _Feed(pkg, s, FD, c1["ctx"], c1["toff"], True)
        feed.play(plans)
        _check(feed, chans, ref_chans)
    finally:
        s.close()
    parity_record(pushes=feed.pushes)


def test_lockstep_channels_on_a_small_chunk(pkg, parity_record):
    """Four feeds in lockstep need the same rows of a bunch, so each starts a bunch of its own: the chunk of a push has more
    samples (fillers included) than max_chunk_frames = 64, which bounds the staged rows only."""
    ctx, toff = 7, 3
    ls, W, b = _net(pkg, FD, ctx, True)
    g = _handle(pkg, ls, W, b, cap=64)
    m, i = _stats(FD)
    xs = WN.make_sentences(np.random.default_rng(14), [400, 400, 400, 400])
    try:
        ref = _offline(g, xs, m, i, ctx, toff)
        s = g.stream_open(m, i, ctx, toff, n_chan=4, max_push_samples=4 * (FD - 1))
        feed = _Feed(pkg, s, FD, ctx, toff, True)
        feed.play(_plans([[x] for x in xs], "hop", FD - 1, None))
        _check(feed, [[x] for x in xs], [[r] for r in ref])
        s.close()
    finally:
        g.close()
    parity_record(pushes=feed.pushes)


# ---- 4. interleaving with other calls on the handle
def _train_chunk(g, rng, ctx, n, width_out):
    fea = rng.standard_normal((n + ctx - 1, FD)).astype(np.float32)
    tg = rng.standard_normal((n + ctx - 1, width_out)).astype(np.float32)
    ws = np.arange(n, dtype=np.int32)
    nat = rng.standard_normal((2, FD)).astype(np.float32)
    g.train_windows(fea, tg, ctx, ws, ws + 1, nat=nat, nat_row=(ws % 2).astype(np.int32))


def test_interleaved_calls_do_not_disturb_the_stream(pkg, case1, parity_record):
    c1 = case1
    g, ctx, toff = c1["g"], c1["ctx"], c1["toff"]             # (lrate 0: the training chunk leaves the weights as they are)
    rng = np.random.default_rng(4)
    xs = WN.make_sentences(rng, [777, 400])
    other = WN.make_sentences(rng, [500, 90])
    ref = _offline(g, xs, c1["m"], c1["i"], ctx, toff)
    ref_other = g.enhance_waves(other, c1["m"], c1["i"], ctx, toff)
    plans = [_blocks(x, SN.ragged_schedule(rng, x.size, FD - 1, zero_share=0.0), False) for x in xs]
    s = g.stream_open(c1["m"], c1["i"], ctx, toff, n_chan=2, max_push_samples=2048)
    try:
        feed = _Feed(pkg, s, FD, ctx, toff, True)
        for k in range(max(len(p) for p in plans)):
            feed.push([p[k] if k < len(p) else None for p in plans])
            if k % 3 == 0:
                again = g.enhance_waves(other, c1["m"], c1["i"], ctx, toff)
                assert all(_same_bits(u, v) for u, v in zip(again, ref_other))
            if k % 3 == 1:
                _train_chunk(g, rng, ctx, 3 * 32, FD)
        _check(feed, [[xs[0]], [xs[1]]], [[ref[0]], [ref[1]]])
    finally:
        s.close()
    parity_record(pushes=feed.pushes)


def _train_pair(pkg, live_stream):
    ctx, B = 3, 32
    ls = [ctx * FD, 64, FD]
    W, b = pkg.glorot_net(ls, seed=11, beta=0.5)
    g = pkg.BP_GPU(1, 3, ls, B, 0.05, 0.5, 0.0, W, b, dropoutflag=1, visible_omit=0.1, hid_omit=0.2, seed=77, max_chunk_frames=512)
    rng = np.random.default_rng(12)
    x = WN.make_sentences(np.random.default_rng(13), [600])[0]
    try:
        s = g.stream_open(np.zeros(FD, np.float32), np.ones(FD, np.float32), ctx, 1, n_chan=1, max_push_samples=256) if live_stream else None
        for ci in range(3):
            if s is not None:
                s.push([x[200 * ci:200 * (ci + 1)]], [ci == 2])
            n = 6 * B
            fea = rng.standard_normal((n + ctx - 1, FD)).astype(np.float32)
            tg = rng.standard_normal((n + ctx - 1, FD)).astype(np.float32)
            ws = np.arange(n, dtype=np.int32)
            g.train_windows(fea, tg, ctx, ws, ws + 1)
            g.train(n, rng.standard_normal((n, ctx * FD)).astype(np.float32), rng.standard_normal((n, FD)).astype(np.float32))
        return g.get_weights(), g.get_deltas()                 # (the handle closes with the stream still open)
    finally:
        g.close()


def test_training_unaffected_by_a_live_stream(pkg):
    (w0, b0), (dw0, db0) = _train_pair(pkg, False)
    (w1, b1), (dw1, db1) = _train_pair(pkg, True)
    for l in (1, 2):
        for u, v in ((w0[l], w1[l]), (b0[l], b1[l]), (dw0[l], dw1[l]), (db0[l], db1[l])):
            assert np.array_equal(u.view(np.uint32), v.view(np.uint32)), l


# ---- 5. two runs of the same schedule agree bit for bit (two streams open on one handle, pushed alternately)
def test_two_streams_same_schedule_same_bits(pkg, case1):
    c1 = case1
    rng = np.random.default_rng(6)
    xs = WN.make_sentences(rng, [333, 1200])
    plans = [_blocks(x, SN.ragged_schedule(rng, x.size, FD - 1), True) for x in xs]
    a = c1["g"].stream_open(c1["m"], c1["i"], c1["ctx"], c1["toff"], n_chan=2, max_push_samples=2048)
    b = c1["g"].stream_open(c1["m"], c1["i"], c1["ctx"], c1["toff"], n_chan=2, max_push_samples=2048)
    try:
        for k in range(max(len(p) for p in plans)):
            items = [p[k] if k < len(p) else (xs[0][:0], False) for p in plans]
            ya = a.push([u for u, _ in items], [e for _, e in items])
            yb = b.push([u for u, _ in items], [e for _, e in items])
            assert all(_same_bits(u, v) for u, v in zip(ya, yb)), k
    finally:
        a.close()
        b.close()


# ---- 6. errors leave the stream as it was
def test_errors_and_the_stream_goes_on(pkg, parity_record):
    ctx, toff = 7, 3
    ls, W, b = _net(pkg, FD, ctx, True)
    g = _handle(pkg, ls, W, b, cap=64)
    m, i = _stats(FD)
    x = WN.make_sentences(np.random.default_rng(9), [3000])[0]
    try:
        ok = dict(context=ctx, targ_offset=toff, target=pkg.WAVE_LPS, out_col=0, n_chan=1, max_push_samples=4000)
        for kw in (dict(out_col=1), dict(targ_offset=ctx), dict(targ_offset=-1), dict(context=ctx + 2), dict(context=0), dict(target=2),
                   dict(n_chan=0), dict(max_push_samples=0)):
            a = dict(ok)
            a.update(kw)
            with pytest.raises(pkg.BPError, match="status -1"):
                g.stream_open(m, i, a["context"], a["targ_offset"], target=a["target"], out_col=a["out_col"], n_chan=a["n_chan"],
                              max_push_samples=a["max_push_samples"])
        with pytest.raises(pkg.BPError, match="status -1"):            # fea_dim 34: no power-of-two FFT
            g.stream_open(np.zeros(34, np.float32), np.ones(34, np.float32), ctx, toff)
        ref = g.enhance_waves([x[:1500]], m, i, ctx, toff)[0]         # 48 frames + 6 edge rows fit the chunk of 64
        ref2 = g.enhance_waves([x[1500:]], m, i, ctx, toff)[0]
        s = g.stream_open(m, i, ctx, toff, n_chan=1, max_push_samples=4000)
        feed = _Feed(pkg, s, FD, ctx, toff, True)
        feed.push([(x[:300], False)])
        with pytest.raises(pkg.BPError, match="status -1"):            # over max_push_samples
            s.push([np.zeros(4001, np.float32)])
        with pytest.raises(pkg.BPError, match="status -1"):            # row capacity: 2700 more samples are 84 frames + 6 rows, the chunk holds 64
            s.push([x[300:]])
        with pytest.raises(pkg.BPError, match="status -1"):            # out_cap: 600 more samples make 19 frames and 608 samples final
            s.push([x[300:900]], out_cap=100)
        feed.push([(x[300:900], False)])
        g.dp_attach(1, 0, "stream-%d" % os.getpid())
        with pytest.raises(pkg.BPError, match="status -3"):            # not on an attached handle: neither a push ...
            s.push([x[900:1000]])
        with pytest.raises(pkg.BPError, match="status -3"):            # ... nor a new stream
            g.stream_open(m, i, ctx, toff)
        g.dp_detach()
        feed.push([(x[900:1500], True)])
        feed.push([(x[1500:2500], False)])                             # the next sentence on the same channel
        with pytest.raises(pkg.BPError, match="status -1"):
            s.push([x[2500:]], [True], out_cap=499)                    # the end returns everything outstanding: more than 499
        feed.push([(x[2500:], True)])
        _check(feed, [[x[:1500], x[1500:]]], [[ref, ref2]])
        s.close()
    finally:
        g.close()
    parity_record(pushes=feed.pushes)


# ---- 7. bpenhance: the streaming mode writes the same files
def test_bpenhance_stream_mode_same_bytes(pkg, tmp_path):
    import subprocess
    import wave
    import pfile_util as PU
    exe = str(pkg.LIB_PATH).replace("libbp_hip.so", "bpenhance")
    ctx, toff = 7, 3
    ls, W, b = _net(pkg, FD, ctx, True)
    m, i = _stats(FD)
    PU.write_wts(str(tmp_path / "net.wts"), ls, W, b)
    PU.write_norm(str(tmp_path / "x.norm"), m, i)
    # (traincache 64: 46, 39 and 36 rows -- no two files share a call, so that the offline run is one call per sentence)
    xs = WN.make_sentences(np.random.default_rng(10), [1234, 1000, 900])
    for k, x in enumerate(xs):
        with wave.open(str(tmp_path / ("in%d.wav" % k)), "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(8000)
            w.writeframes(np.asarray(x, np.int16).tobytes())
    outs = {}
    for tag, extra in (("off", []), ("on", ["stream_block=100", "stream_chan=2"])):
        (tmp_path / (tag + ".list")).write_text("".join("%s %s\n" % (tmp_path / ("in%d.wav" % k), tmp_path / ("%s%d.wav" % (tag, k)))
                                                        for k in range(len(xs))))
        r = subprocess.run([exe, "norm_file=%s" % (tmp_path / "x.norm"), "initwts_file=%s" % (tmp_path / "net.wts"),
                            "layersizes=%s" % ",".join(map(str, ls)), "fea_dim=%d" % FD, "fea_context=%d" % ctx, "targ_offset=%d" % toff,
                            "wav_list=%s" % (tmp_path / (tag + ".list")), "traincache=64", "bunchsize=32"] + extra,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 1, r.stdout + r.stderr
        outs[tag] = [open(tmp_path / ("%s%d.wav" % (tag, k)), "rb").read() for k in range(len(xs))]
    assert all(len(v) > 44 for v in outs["off"])
    assert outs["on"] == outs["off"]
