"""GPU tests of the log-MMSE streams (bp_lmstream_open / _push / _close; -m gpu).  The yardstick is exact: a sentence pushed in
blocks of ANY sizes, on any channel, in any company, returns the same bits as ONE logmmse_waves call on the finished sentence
alone.  Every comparison is np.array_equal on the uint32 view; no tolerance appears anywhere.  The offline call itself is held
to the float64 restatement by tests/test_classic_gpu.py.  After every push the samples returned per channel equal the counts
of tests/lmstream_np.py."""
import subprocess

import numpy as np
import pytest

import classic_np as CN
import lmstream_np as LN
import stream_np as SN
import wave_np as WN

pytestmark = pytest.mark.gpu

FD = 33                                                   # n_fft 64, hop 32
INIT = CN.DEFAULTS["init_frames"]
# T below, at and above init_frames = 6 (160 samples: T = 6), hop multiples with one sample on either side
LENGTHS = [1, 31, 32, 33, 160, 161, 191, 192, 193, 1000]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(a, b):
    return np.shape(a) == np.shape(b) and np.array_equal(_bits(a), _bits(b))


def _offline(pkg, fea_dim, xs, params=None):
    """One logmmse_waves call per finished sentence."""
    return [pkg.logmmse_waves(0, fea_dim, [x], params)[0] for x in xs]


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
    """Drives one stream: every channel plays its list of (block, end) pushes; checks the returned lengths against the counts
    after every push and collects the output per channel and sentence."""

    def __init__(self, pkg, stream, fea_dim, init=INIT):
        self.pkg, self.s, self.cfg = pkg, stream, (fea_dim, init)
        self.received = [0] * stream.n_chan
        self.out = [[[]] for _ in range(stream.n_chan)]
        self.pushes = self.idle = self.end_beside_wait = 0

    def push(self, items, **kw):
        """items: per channel (block, end) or None."""
        idle = sum(it is None or (it[0].size == 0 and not it[1]) for it in items)
        items = [(np.zeros(0, np.float32), False) if it is None else it for it in items]
        got = self.s.push([b for b, _ in items], [e for _, e in items], **kw)
        self.pushes += 1
        self.idle += 0 < idle < len(items)
        ends = waits = 0
        for c, ((b, e), y) in enumerate(zip(items, got)):
            before = LN.counts(*self.cfg, self.received[c], False)[2]
            self.received[c] += b.size
            ended = bool(e) and self.received[c] > 0
            after = self.pkg.logmmse_stream_counts(*self.cfg, self.received[c], ended)
            assert after == LN.counts(*self.cfg, self.received[c], ended)
            assert y.size == after[2] - before, (c, self.received[c], ended, y.size, after, before)
            self.out[c][-1].append(y)
            ends += ended
            waits += (not ended) and self.received[c] > 0 and after[1] == 0
            if ended:
                self.received[c] = 0
                self.out[c].append([])
        self.end_beside_wait += ends > 0 and waits > 0
        return got

    def play(self, plans):
        """plans: per channel a list of (block, end); channels advance in lockstep, one item per push."""
        for k in range(max(len(p) for p in plans)):
            self.push([p[k] if k < len(p) else None for p in plans])

    def sentences(self, c):
        return [np.concatenate(s) if s else np.zeros(0, np.float32) for s in self.out[c][:-1]]


def _plan(sents, schedule, hop, rng):
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
    return p


def _check(feed, chans, ref_chans):
    for c, (sents, refs) in enumerate(zip(chans, ref_chans)):
        got = feed.sentences(c)
        assert len(got) == len(sents), (c, len(got), len(sents))
        for k, (y, r) in enumerate(zip(got, refs)):
            assert _same_bits(y, r), "channel %d sentence %d (%d samples): %d samples differ" % (
                c, k, r.size, int((_bits(y) != _bits(r)).sum()) if y.size == r.size else -1)


def _run(pkg, fea_dim, chans, ref_chans, plans, params=None, max_push=None):
    init = INIT if params is None else params["init_frames"]
    with pkg.logmmse_stream_open(0, fea_dim, params, n_chan=len(chans), max_push_samples=max_push or 16000) as s:
        feed = _Feed(pkg, s, fea_dim, init)
        feed.play(plans)
        _check(feed, chans, ref_chans)
    return feed


# ---- 1. any chunking gives the same bits
@pytest.fixture(scope="module")
def case33(pkg):
    """Gated tones in noise behind a noise-only lead of 240 samples: the short ones are noise, the long one has both."""
    xs = [CN.gated_tones(40 + k, n, FD, 10.0) for k, n in enumerate(LENGTHS)]
    ref = _offline(pkg, FD, xs)
    _, vad = pkg.logmmse_waves(0, FD, [xs[-1]], return_vad=True)
    noise = vad[0] < CN.DEFAULTS["eta"]
    assert noise.any() and not noise.all()                       # both outcomes of the VAD on the long sentence
    assert any(not np.array_equal(r, x) for r, x in zip(ref, xs))
    return dict(xs=xs, ref=ref)


@pytest.mark.parametrize("schedule", ["one", "hop", "single", "ragged17", "ragged18", "ragged19"])
def test_any_chunking_same_bits(pkg, case33, schedule, parity_record):
    """One channel, the sentences one after the other: lambda, A_prev, the half frame and the frame index all restart."""
    keep = [k for k, x in enumerate(case33["xs"]) if schedule != "single" or x.size <= 32 or x.size == 1000]
    xs, ref = [case33["xs"][k] for k in keep], [case33["ref"][k] for k in keep]
    rng = np.random.default_rng(int(schedule[6:])) if schedule.startswith("ragged") else None
    feed = _run(pkg, FD, [xs], [ref], [_plan(xs, schedule[:6], FD - 1, rng)], max_push=1024)
    parity_record(pushes=feed.pushes, sentences=len(xs))


# ---- 2. channels are independent
def test_channels_independent(pkg, case33, parity_record):
    xs, ref = case33["xs"], case33["ref"]
    chans, ref_chans = [xs[c::3] for c in range(3)], [ref[c::3] for c in range(3)]
    plans = [_plan(sents, "ragged", FD - 1, np.random.default_rng(70 + c)) for c, sents in enumerate(chans)]
    feed = _run(pkg, FD, chans, ref_chans, plans, max_push=4096)
    # some pushes gave some channels nothing, and in some a channel ended while another waited for its noise start
    assert feed.idle > 0 and feed.end_beside_wait > 0, (feed.idle, feed.end_beside_wait)
    parity_record(pushes=feed.pushes, idle=feed.idle, end_beside_wait=feed.end_beside_wait)


def test_many_channels(pkg, case33, parity_record):
    """64 channels, hop-sized blocks: more workgroups than one wave of jobs and a job table that is not tiny.  Channel c plays
    the 160 .. 193-sample sentences starting from sentence c mod 5, so that the channels are in different phases."""
    ks = [k for k, n in enumerate(LENGTHS) if 160 <= n <= 193]
    chans = [[case33["xs"][ks[(c + i) % len(ks)]] for i in range(len(ks))] for c in range(64)]
    ref_chans = [[case33["ref"][ks[(c + i) % len(ks)]] for i in range(len(ks))] for c in range(64)]
    feed = _run(pkg, FD, chans, ref_chans, [_plan(sents, "hop", FD - 1, None) for sents in chans], max_push=64 * (FD - 1))
    parity_record(pushes=feed.pushes)


# ---- 3. the fixture calls of the offline tests (fea_dim 65, 129 and 257: at most 1, 1 and 2 bins per thread)
def _fixture_call(fea_dim):
    return [f for f in CN.fixtures() if f[0] == fea_dim][0]


def _two_channel_ragged(pkg, fea_dim, xs, ref, params, seed):
    chans, ref_chans = [xs[c::2] for c in range(2)], [ref[c::2] for c in range(2)]
    plans = [_plan(sents, "ragged", fea_dim - 1, np.random.default_rng(seed + c)) for c, sents in enumerate(chans)]
    return _run(pkg, fea_dim, chans, ref_chans, plans, params)


@pytest.mark.parametrize("fea_dim", [65, 129, 257])
def test_fixture_sentences(pkg, fea_dim, parity_record):
    D, kinds, xs = _fixture_call(fea_dim)
    assert {"one", "short", "zero", "gap"} <= set(kinds)
    ref = _offline(pkg, D, xs)
    feed = _two_channel_ragged(pkg, D, xs, ref, None, 31)
    z = kinds.index("zero")
    got = feed.sentences(z % 2)[z // 2]
    assert got.size == xs[z].size and not got.any()              # the all-zero sentence returns zeros
    parity_record(fea_dim=D, pushes=feed.pushes, sentences=len(xs), samples_differing=0)


def test_non_default_parameters(pkg):
    D, kinds, xs = _fixture_call(129)
    ref, alt = _offline(pkg, D, xs), _offline(pkg, D, xs, CN.ALT)
    _two_channel_ragged(pkg, D, xs, alt, dict(CN.ALT), 33)
    assert not _same_bits(ref[0], alt[0]) and not _same_bits(ref[kinds.index("gap")], alt[kinds.index("gap")])


# ---- 4. wide spectra (fea_dim 513 and 1025: 3 and 5 bins per thread, the largest LDS layout)
@pytest.mark.parametrize("fea_dim", [513, 1025])
def test_wide_spectra(pkg, fea_dim, parity_record):
    x = [xs for D, xs in CN.wide_fixtures() if D == fea_dim][0][2]
    ref = _offline(pkg, fea_dim, [x])
    for schedule in ("hop", "one"):
        feed = _run(pkg, fea_dim, [[x]], [ref], [_plan([x], schedule, fea_dim - 1, None)])
    parity_record(fea_dim=fea_dim, pushes=feed.pushes, samples_differing=0)


# ---- 5. determinism and isolation
def test_same_plan_twice_same_bits(pkg, case33):
    xs = case33["xs"]
    outs = []
    for _ in range(2):
        with pkg.logmmse_stream_open(0, FD, n_chan=2, max_push_samples=4096) as s:
            feed = _Feed(pkg, s, FD)
            feed.play([_plan(xs[c::2], "ragged", FD - 1, np.random.default_rng(5 + c)) for c in range(2)])
            outs.append([feed.sentences(c) for c in range(2)])
    for c in range(2):
        assert len(outs[0][c]) == len(xs[c::2])
        assert all(_same_bits(a, b) for a, b in zip(outs[0][c], outs[1][c]))


def test_streams_and_other_calls_do_not_disturb_each_other(pkg, case33):
    """Two streams pushed alternately; between the pushes an offline call and a net handle's enhance_waves."""
    xs, ref = case33["xs"], case33["ref"]
    ctx, toff = 3, 1
    ls = [ctx * FD, 48, FD]
    W, b = pkg.glorot_net(ls, seed=3, beta=0.5)
    g = pkg.BP_GPU(1, len(ls), ls, 32, 0.0, 0.0, 0.0, W, b, max_chunk_frames=512)
    m, i = WN.norm_stats(WN.make_sentences(np.random.default_rng(5), [40 * (FD - 1)]), FD)
    m, i = m.astype(np.float32), i.astype(np.float32)
    try:
        net0 = g.enhance_waves([xs[-1]], m, i, ctx, toff)[0]
        sa, sb = xs[4:7], xs[7:]
        with pkg.logmmse_stream_open(0, FD, max_push_samples=2048) as a, pkg.logmmse_stream_open(0, FD, max_push_samples=2048) as bb:
            fa, fb = _Feed(pkg, a, FD), _Feed(pkg, bb, FD)
            pa = _plan(sa, "ragged", FD - 1, np.random.default_rng(1))
            pb = _plan(sb, "hop", FD - 1, None)
            for k in range(max(len(pa), len(pb))):
                if k < len(pa):
                    fa.push([pa[k]])
                if k < len(pb):
                    fb.push([pb[k]])
                if k % 7 == 3:
                    assert _same_bits(pkg.logmmse_waves(0, FD, [xs[5]])[0], ref[5])
                if k % 11 == 5:
                    assert _same_bits(g.enhance_waves([xs[-1]], m, i, ctx, toff)[0], net0)
            _check(fa, [sa], [ref[4:7]])
            _check(fb, [sb], [ref[7:]])
    finally:
        g.close()


# ---- 6. errors leave the stream as it was
def test_errors_leave_the_stream_as_it_was(pkg, case33):
    x, ref = case33["xs"][-1], case33["ref"][-1]
    hop = FD - 1
    with pkg.logmmse_stream_open(0, FD, n_chan=2, max_push_samples=512) as s:
        feed = _Feed(pkg, s, FD)
        assert [y.size for y in feed.push([None, (x[:0], True)])] == [0, 0]      # end on a channel that received nothing
        feed.push([(x[:300], False), None])
        lib, sp = pkg.load_library(), s._s
        import ctypes as C
        n_out, out = (C.c_int * 2)(), (C.c_float * 4096)()

        def raw(n_in, cap):
            pcm = (C.c_float * 1024)(*([1.0] * 1024))
            return lib.bp_lmstream_push(sp, (C.c_int * 2)(*n_in), pcm, None, n_out, out, cap)
        assert raw([-1, 0], 4096) == -1                          # a negative n_in
        assert raw([300, 213], 4096) == -1                       # sum(n_in) > max_push_samples
        with pytest.raises(pkg.BPError, match="status -1"):
            s.push([x[300:301], x[:513]])
        # 300 received: 9 frames, 256 samples out; 200 more: 15 frames, 448 out -- 192 are due
        with pytest.raises(pkg.BPError, match="192 samples are due.*status -1"):
            s.push([x[300:500], None], out_cap=191)
        assert [y.size for y in feed.push([None, (x[:0], True)])] == [0, 0]
        feed.push([(x[300:500], False), None], out_cap=192)
        feed.push([(x[500:], True), None])
        assert _same_bits(feed.sentences(0)[0], ref)
        feed.push([None, (x[:500], False)])                      # both channels go on working
        feed.push([(x[:hop], False), (x[500:980], False)])
        feed.push([None, (x[980:], True)])
        assert _same_bits(feed.sentences(1)[0], ref)
    with pytest.raises(pkg.BPError, match="status -1"):
        pkg.logmmse_stream_open(99, FD)


# ---- 7. the command-line tool
def _write_pcm16(path, x, rate):
    import wave
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(rate)
        w.writeframes(np.asarray(x, np.int16).tobytes())


def test_bpenhance_lm_stream(pkg, tmp_path):
    exe = str(pkg.LIB_PATH).replace("libbp_hip.so", "bpenhance")
    _, kinds, xs = _fixture_call(129)
    for tag in ("off", "live"):
        (tmp_path / tag).mkdir()
    for i, x in enumerate(xs):
        _write_pcm16(tmp_path / ("in%d.wav" % i), x, 8000)
    for tag in ("off", "live"):
        (tmp_path / (tag + ".list")).write_text("".join("%s %s\n" % (tmp_path / ("in%d.wav" % i), tmp_path / tag / ("out%d.wav" % i))
                                                        for i in range(len(xs))))

    def run(*keys):
        return subprocess.run([exe, "method=logmmse", "fea_dim=129"] + list(keys), capture_output=True, text=True, timeout=120)
    r0 = run("wav_list=%s" % (tmp_path / "off.list"))
    r1 = run("wav_list=%s" % (tmp_path / "live.list"), "lm_stream_block=160", "lm_stream_chan=3")
    assert r0.returncode == 1 and r1.returncode == 1 and "streamed" in r1.stdout, r0.stdout + r1.stdout + r1.stderr
    for i in range(len(xs)):
        a, b = (tmp_path / "off" / ("out%d.wav" % i)).read_bytes(), (tmp_path / "live" / ("out%d.wav" % i)).read_bytes()
        assert len(a) >= 2 * xs[i].size and a == b, kinds[i]
    io = ["in_wav=%s" % (tmp_path / "in0.wav"), "out_wav=%s" % (tmp_path / "no.wav")]
    for keys in (["lm_stream_chan=2"], ["lm_stream_block=0"], ["lm_stream_block=2.5"], ["lm_stream_block=160", "lm_stream_chan=0"]):
        r = run(*(io + keys))
        assert r.returncode == 0 and r.stdout.strip() and not (tmp_path / "no.wav").exists(), (keys, r.stdout)
    r = subprocess.run([exe, "fea_dim=129", "lm_stream_block=160"] + io, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "method=logmmse" in r.stdout and not (tmp_path / "no.wav").exists()
