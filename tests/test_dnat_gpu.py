"""GPU tests of the dynamic noise-aware input (bp_set_nat, the nat= key; -m gpu) against the float64
restatement in tests/dnat_np.py, against the log-MMSE baseline's tracker, and against the calls it is made of.

Bars: the staged rows, and the de-normalised block read back through the selector net, within the project's bar
max|a - ref| / max|ref| < 1e-4 (tests/util.py) of the restatement on the call's own PCM, and of log(out_noise) of the baseline;
the mode holds no decision, so no fixture needs a margin.  Everything else -- company, entry points, streams, training, residue,
the tools -- bit for bit.  Shapes (dnat_np's case table): fea_dim 33 and 129, 257 once for the partial last 64-thread workgroup;
sentences of 2 (the shortest there is), 3, 6, 7 and 40 frames in one batch; context 3 / targ_offset 1 and context 1.  The rows,
the streams and the training also at the other sizes of the frame-size table (dnat_np.GEOMETRY; tests/geometry_cases.py)."""
import subprocess

import numpy as np
import pytest

import dnat_np as DN
import noise_np as NN
import stream_np as SN
import wave_np as WN
from util import TOL, relerr

pytestmark = pytest.mark.gpu
FS = 8000


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(xs, ys):
    return len(xs) == len(ys) and all(np.shape(a) == np.shape(b) and np.array_equal(_bits(a), _bits(b)) for a, b in zip(xs, ys))


def _plan(pkg, n_clean, noise, seed=3):
    return pkg.mix_plan(seed, n_clean, 1, [x.size for x in noise], [0.0, 5.0])


def _noise(D, seed=2):
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 800.0, 50 * (D - 1))
    x[x.size // 2:] *= 2.0                                       # a level that moves
    return [np.round(x).astype(np.float32), WN.make_sentences(rng, [37], scale=1500.0)[0]]


def _selector(pkg, D, ctx, mode="dynamic", **kw):
    mean, istd = DN.norm(D)
    ls, W, b = DN.selector_net(D, ctx, mean, istd)
    return pkg.BP_GPU(1, 3, ls, 32, 0.0, 0.0, 0.0, W, b, max_chunk_frames=400, nat_mode=mode, **kw), mean, istd


def _glorot(pkg, D, ctx, mode="dynamic", nat=True, cap=400, lrate=0.01, **kw):
    ls = [(ctx + (1 if nat else 0)) * D, 64, 48, D]
    W, b = pkg.glorot_net(ls, seed=5, beta=0.5)
    return pkg.BP_GPU(1, len(ls), ls, 32, lrate, 0.5, 1e-4, W, b, max_chunk_frames=cap, nat_mode=mode, **kw)


def _split(pcm, lens):
    return np.split(pcm, np.cumsum(lens)[:-1])


# ---- 1. the restatement and the baseline's tracker
@pytest.mark.parametrize("D,ctx,toff", [(33, 3, 1), (33, 1, 0), (129, 3, 1), (257, 1, 0), (65, 3, 1), (513, 3, 1), (1025, 3, 1)])
def test_rows_match_restatement_and_the_baseline(pkg, D, ctx, toff, parity_record):
    clean, noise = DN.sentences(D, D), _noise(D)
    g, mean, istd = _selector(pkg, D, ctx)
    try:
        assert g.nat_mode == "dynamic"
        g.set_mix_corpus(clean, noise, mean, istd, ctx, toff)
        plan = _plan(pkg, len(clean), noise)
        # at the tracker's defaults, and under noise_np.BUSY, where pbar reaches the ramp in every bin within these short sentences
        # (tests/test_noise_host.py): at the defaults the ceiling of the definition never acts on them
        for tag, params in (("", None), ("busy_", NN.BUSY)):
            g.set_nat("dynamic", params)
            f = g.mix_features(plan)
            lens = [clean[c].size for c in plan["clean"]]
            T = [int(t) for t in g.mix_frames(plan)]
            assert sorted(T) == list(DN.T_CLASSES) and f["nat"].shape == (sum(T), D) and np.isfinite(f["nat"]).all()
            mix = _split(f["pcm"], lens)
            ref, _ = DN.batch(mix, D, mean, istd, params)
            e_rows = relerr(f["nat"], ref)
            # through the net: bp_enhance_waves on the same samples returns the de-normalised block as its output
            _, net = g.enhance_waves(mix, mean, istd, ctx, toff, return_net=True)
            net = np.concatenate(net)
            e_net = relerr(net, DN.denormalise(ref, mean, istd))
            # the baseline's out_noise on the same PCM and parameters
            _, noise_rows = pkg.logmmse_waves(0, D, mix, noise=params or "spp", return_noise=True)
            lam32 = np.concatenate(noise_rows)
            e_base = relerr(DN.denormalise(f["nat"], mean, istd), np.log(lam32.astype(np.float64)))
            # the two analyses share Y's bits and the tracker: the rows are the fp32 expression of the baseline's fl32 lambdas, up to
            # the last bits of logf against numpy's log (the lambdas themselves are not visible through the logarithm)
            host = (np.log(lam32).astype(np.float32) - mean) * istd
            e_bits = relerr(f["nat"], host)
            print(D, ctx, tag, dict(rows=e_rows, net=e_net, baseline=e_base, fp32_expression=e_bits))
            parity_record(fea_dim=D, context=ctx, **{tag + "rows": e_rows, tag + "net": e_net, tag + "baseline": e_base,
                                                     tag + "fp32_expression": e_bits})
            assert e_rows < TOL and e_net < TOL and e_base < TOL
            # (4 ulp of a float in [16, 32) -- logf against log, the subtraction -- times inv_std <= 0.5, over max|row| >= 1)
            assert np.abs(host).max() >= 1.0 and istd.max() <= 0.5 and e_bits < 4 * 2.0 ** -19 * 0.5
            if params is not None:
                assert relerr(ref, DN.batch(mix, D, mean, istd)[0]) > 10 * TOL          # (the parameters are read)
        # static mode on the same handle: one row per mixture again
        g.set_nat("static")
        assert g.mix_features(plan)["nat"].shape == (len(plan), D)
    finally:
        g.close()


# ---- 2. equal bits between entry points
@pytest.mark.parametrize("D", [33, 129])
def test_a_sentence_alone_and_in_the_batch_and_twice(pkg, D):
    ctx, toff = 3, 1
    xs = DN.sentences(7, D)
    g, mean, istd = _selector(pkg, D, ctx)                      # (one non-zero weight per sum: the forward is exact in any row)
    try:
        w, net = g.enhance_waves(xs, mean, istd, ctx, toff, return_net=True)
        w2, net2 = g.enhance_waves(xs, mean, istd, ctx, toff, return_net=True)
        assert _same(w, w2) and _same(net, net2)
        for i, x in enumerate(xs):
            w1, n1 = g.enhance_waves([x], mean, istd, ctx, toff, return_net=True)
            assert _same(w1, [w[i]]) and _same(n1, [net[i]]), (D, i)
        g.set_nat("static")
        assert not _same(g.enhance_waves(xs, mean, istd, ctx, toff), w)
    finally:
        g.close()


def _differing(got, want):
    return sum(int((_bits(a) != _bits(b)).sum()) if a.shape == b.shape else max(a.size, b.size) for a, b in zip(got, want))


def _play(stream, feeds, hop, rng, end_early=None):
    """feeds: per channel a list of sentences, played one after the other in ragged blocks; returns per channel the output."""
    nc = len(feeds)
    plans = []
    for xs in feeds:
        p = []
        for x in xs:
            sizes = SN.ragged_schedule(rng, x.size, hop)
            at = 0
            for k, b in enumerate(sizes):
                p.append((x[at:at + b], k == len(sizes) - 1))
                at += b
        plans.append(p)
    out = [[] for _ in range(nc)]
    for step in range(max(len(p) for p in plans)):
        blocks = [p[step][0] if step < len(p) else None for p in plans]
        end = [bool(step < len(p) and p[step][1]) for p in plans]
        for c, y in enumerate(stream.push(blocks, end)):
            out[c].append(y)
    return [np.concatenate(o) for o in out]


# (every size of the frame-size table unpacked -- bp_stream_dnat with 1, 2, 3, 5, 9 and 17 workgroups per job -- and the packed form
# at the smallest and the largest)
@pytest.mark.parametrize("D,ctx,toff,packed", [(33, 3, 1, False), (33, 3, 1, True), (129, 1, 0, False), (129, 1, 0, True), (65, 3, 1, False),
                                               (257, 3, 1, False), (513, 3, 1, False), (1025, 3, 1, False), (1025, 3, 1, True)])
def test_streams_return_the_bits_of_enhance_waves(pkg, D, ctx, toff, packed, parity_record):
    hop = D - 1
    xs = DN.sentences(9, D)                                      # (2 and 3 frames: the sentence ends before the sixth frame)
    mean, istd = DN.norm(D)
    kw = dict(forward_mode=pkg.FORWARD_ROWINV) if packed else {}
    g = _glorot(pkg, D, ctx, lrate=0.0, **kw)
    try:
        # the default forward's bits depend on the row of the bunch: a stream runs frame t as row t mod bunchsize, as one sentence alone
        ref = [g.enhance_waves([x], mean, istd, ctx, toff)[0] for x in xs]
        rng = np.random.default_rng(D + ctx)
        s = g.stream_open(mean, istd, ctx, toff, n_chan=2, max_push_samples=2 * 9 * hop)
        try:
            assert s.nat_mode == "dynamic" and s.packed == packed
            g.set_nat("static")                                  # the stream keeps its mode
            feeds = [[xs[4], xs[0], xs[2]], [xs[1], xs[3]]]
            got = _play(s, feeds, hop, rng)
            assert s.nat_mode == "dynamic" and g.nat_mode == "static"
        finally:
            s.close()
        want = [np.concatenate([ref[4], ref[0], ref[2]]), np.concatenate([ref[1], ref[3]])]
        differing = _differing(got, want)
        assert _same(got, want)
        # ... and one opened before bp_set_nat keeps the static row
        stat = [g.enhance_waves([x], mean, istd, ctx, toff)[0] for x in xs]
        assert not _same(stat, ref)
        s = g.stream_open(mean, istd, ctx, toff, n_chan=2, max_push_samples=2 * 9 * hop)
        try:
            g.set_nat("dynamic")
            assert s.nat_mode == "static"
            got = _play(s, feeds, hop, np.random.default_rng(1))
        finally:
            s.close()
        assert _same(got, [np.concatenate([stat[4], stat[0], stat[2]]), np.concatenate([stat[1], stat[3]])])
        # under noise_np.BUSY the pbar a channel carries between pushes moves every bin of these short sentences
        # (tests/test_noise_host.py); at the defaults it never reaches the ramp, and a stream that lost it would return the same bits
        g.set_nat("dynamic", NN.BUSY)
        busy = [g.enhance_waves([x], mean, istd, ctx, toff)[0] for x in xs]
        assert not _same(busy, ref)
        s = g.stream_open(mean, istd, ctx, toff, n_chan=2, max_push_samples=2 * 9 * hop)
        try:
            got = _play(s, feeds, hop, np.random.default_rng(2))
        finally:
            s.close()
        want = [np.concatenate([busy[4], busy[0], busy[2]]), np.concatenate([busy[1], busy[3]])]
        differing += _differing(got, want)
        parity_record(fea_dim=D, packed=packed, samples_differing=differing)
        assert differing == 0
    finally:
        g.close()


@pytest.mark.parametrize("D", [33, 129])
def test_eval_mix_and_cv_mix_are_their_parts(pkg, D):
    ctx, toff = 3, 1
    clean, noise = DN.sentences(D + 1, D), _noise(D)
    mean, istd = DN.norm(D)
    g, b = _glorot(pkg, D, ctx), _glorot(pkg, D, ctx)
    try:
        for h in (g, b):
            h.set_mix_corpus(clean, noise, mean, istd, ctx, toff)
        plan = _plan(pkg, len(clean), noise)
        lens = [clean[c].size for c in plan["clean"]]
        ev = g.eval_mix(plan, FS, return_pcm=True)
        f = g.mix_features(plan)
        enh = g.enhance_waves(_split(f["pcm"], lens), mean, istd, ctx, toff)
        assert _same(ev["pcm"], enh)
        # bp_cv_mix against bp_cv_chunk on rows stacked on the host: window(t) ++ nat[t]
        T = g.mix_frames(plan)
        x = np.concatenate([np.concatenate([WN.stack(z, ctx, toff, False), n], axis=1)
                            for z, n in zip(_split(f["fea"], T), _split(f["nat"], T))]).astype(np.float32)
        ea = g.CrossValid_mix(plan)
        eb = b.CrossValid(x.shape[0], x, f["targ"])
        assert np.float32(ea).view(np.uint32) == np.float32(eb).view(np.uint32), (ea, eb)
    finally:
        g.close()
        b.close()


# ---- 3. training: a window meets its own frame's row after the shuffle
@pytest.mark.parametrize("D", DN.ALL_DIMS)
def test_training_equals_host_stacked_rows(pkg, D, parity_record):
    ctx, toff = 3, 1
    clean, noise = DN.sentences(21, D), _noise(D)
    mean, istd = DN.norm(D)
    a, b = _glorot(pkg, D, ctx), _glorot(pkg, D, ctx)
    try:
        for h in (a, b):
            h.set_mix_corpus(clean, noise, mean, istd, ctx, toff)
        plan = _plan(pkg, len(clean), noise)
        T = a.mix_frames(plan)
        n = int(T.sum())
        order = pkg.mix_shuffle(345, 0, n)
        assert not np.array_equal(order, np.arange(n))
        a.train_mix(plan, order)
        f = b.mix_features(plan)
        x = np.concatenate([np.concatenate([WN.stack(z, ctx, toff, False), r], axis=1)
                            for z, r in zip(_split(f["fea"], T), _split(f["nat"], T))]).astype(np.float32)
        b.train(n, np.ascontiguousarray(x[order]), np.ascontiguousarray(f["targ"][order]))
        (wa, ba), (wb, bb) = a.get_weights(), b.get_weights()
        w0, _ = pkg.glorot_net(a.layersizes, seed=5, beta=0.5)
        parity_record(fea_dim=D, rows=n, words_differing=sum(int((_bits(wa[l]) != _bits(wb[l])).sum()) + int((_bits(ba[l]) != _bits(bb[l])).sum())
                                                             for l in range(1, a.numlayers)))
        for l in range(1, a.numlayers):
            assert not np.array_equal(wa[l].reshape(-1), np.asarray(w0[l], np.float32).reshape(-1))      # (it trained)
            assert np.array_equal(wa[l], wb[l]) and np.array_equal(ba[l], bb[l]), l
    finally:
        a.close()
        b.close()


# ---- 4. no residue
def test_modes_and_sizes_leave_no_residue(pkg):
    D, ctx, toff = 33, 3, 1
    mean, istd = DN.norm(D)
    xs = DN.sentences(31, D)
    small = [xs[1], xs[3]]
    fresh = {}
    for mode in DN.MODES:
        h = _glorot(pkg, D, ctx, mode)
        try:
            fresh[mode] = (h.enhance_waves(xs, mean, istd, ctx, toff), h.enhance_waves(small, mean, istd, ctx, toff))
        finally:
            h.close()
    fs = _glorot(pkg, D, ctx)
    try:
        fresh_small = fs.enhance_waves(small, mean, istd, ctx, toff)   # (a fresh handle's FIRST call)
    finally:
        fs.close()
    g = _glorot(pkg, D, ctx)
    try:
        for mode in ("dynamic", "static", "dynamic", "static"):
            g.set_nat(mode)
            assert _same(g.enhance_waves(xs, mean, istd, ctx, toff), fresh[mode][0]), mode
        # a small call, a large one that regrows the noise-aware rows of both staging sets, the small one again
        g.set_nat("dynamic")
        assert _same(g.enhance_waves(small, mean, istd, ctx, toff), fresh_small)
        big = xs + xs + xs
        g.enhance_waves(big, mean, istd, ctx, toff)
        g.enhance_waves(big, mean, istd, ctx, toff)
        assert _same(g.enhance_waves(small, mean, istd, ctx, toff), fresh_small)
        assert _same(g.enhance_waves(small, mean, istd, ctx, toff), fresh["dynamic"][1])
    finally:
        g.close()


# ---- 5. errors leave the handle as it was
def test_errors_leave_the_handle_unchanged(pkg):
    D, ctx, toff = 33, 3, 1
    mean, istd = DN.norm(D)
    xs = DN.sentences(41, D)
    clean, noise = xs, _noise(D)
    for nat in (True, False):
        ref = _glorot(pkg, D, ctx, "static", nat=nat)
        try:
            want = ref.enhance_waves(xs, mean, istd, ctx, toff)
        finally:
            ref.close()
        g = _glorot(pkg, D, ctx, "static", nat=nat)
        try:
            bad = [("vad", "BP_NOISE_SPP"), ({"mode": 0}, "BP_NOISE_SPP"), ({"q": 1.5}, "q"), ({"xi_h1_db": 41.0}, "xi_h1_db"),
                   ({"a_pow": 1.0}, "a_pow"), ({"a_spp": -0.1}, "a_spp"), ({"p_lo": 0.995}, "p_lo"), ({"mode": 2}, "mode")]
            for noise_arg, word in bad:
                with pytest.raises(pkg.BPError, match="status -1") as e:
                    g.set_nat("dynamic", noise_arg)
                assert "bp_set_nat" in str(e.value) and word in str(e.value), (noise_arg, str(e.value))
                assert g.nat_mode == "static"
            with pytest.raises(pkg.BPError):
                g.set_nat("sometimes")
            with pytest.raises(pkg.BPError, match="status -1"):
                g.set_nat("static", {"q": 0.0})                   # the range rules hold in either mode
            assert g._lib.bp_set_nat(g._h, 2, None) == -1 and b"mode" in g._lib.bp_last_error()
            assert _same(g.enhance_waves(xs, mean, istd, ctx, toff), want)
            if not nat:
                # dynamic on a net without the block: the setter cannot know, the staging calls say so
                g.set_nat("dynamic")
                g.set_mix_corpus(clean, noise, mean, istd, ctx, toff)
                plan = _plan(pkg, len(clean), noise)
                calls = [lambda: g.enhance_waves(xs, mean, istd, ctx, toff), lambda: g.mix_features(plan), lambda: g.train_mix(plan),
                         lambda: g.CrossValid_mix(plan), lambda: g.eval_mix(plan, FS),
                         lambda: g.stream_open(mean, istd, ctx, toff)]
                for call in calls:
                    with pytest.raises(pkg.BPError, match="status -1") as e:
                        call()
                    assert "BP_NAT_DYNAMIC" in str(e.value) and "noise-aware block" in str(e.value)
                g.eval_mix_logmmse(plan, FS)                      # (no net input: the mode is not read)
                g.set_nat("static")
                assert _same(g.enhance_waves(xs, mean, istd, ctx, toff), want)
        finally:
            g.close()


# ---- 6. the tools
def _write_pcm16(path, x, rate=FS):
    import wave
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(rate)
        w.writeframes(np.asarray(x, np.int16).tobytes())


def _read_pcm16(path):
    import wave
    with wave.open(str(path), "rb") as w:
        return np.frombuffer(w.readframes(w.getnframes()), np.int16)


def _to_pcm16(y):
    """write_wav's rounding: to nearest, ties to even, clipped; not-a-number as 0."""
    y = np.asarray(y, np.float32)
    return np.clip(np.rint(np.where(np.isnan(y), np.float32(0.0), y)), -32768, 32767).astype(np.int16)


def _files(pkg, tmp_path, D, ctx, xs, noise, mean, istd):
    import pfile_util as PU
    ls = [(ctx + 1) * D, 64, 48, D]
    W, b = pkg.glorot_net(ls, seed=5, beta=0.5)
    PU.write_wts(str(tmp_path / "net.wts"), ls, W, b)
    (tmp_path / "x.norm").write_text("<mean>\n" + "".join("%.9g\n" % v for v in mean) + "<inverse std>\n" +
                                     "".join("%.9g\n" % v for v in istd))
    for tag, ys in (("clean", xs), ("noise", noise)):
        for i, x in enumerate(ys):
            _write_pcm16(tmp_path / ("%s%d.wav" % (tag, i)), x)
        (tmp_path / (tag + ".list")).write_text("".join("%s\n" % (tmp_path / ("%s%d.wav" % (tag, i))) for i in range(len(ys))))
    (tmp_path / "enh.list").write_text("".join("%s %s\n" % (tmp_path / ("clean%d.wav" % i), tmp_path / ("enh%d.wav" % i))
                                               for i in range(len(xs))))
    return ls


def test_bpenhance_and_bpeval_follow_the_key(pkg, tmp_path):
    D, ctx, toff = 33, 3, 1
    mean, istd = DN.norm(D)
    xs, noise = DN.sentences(51, D), _noise(D)
    ls = _files(pkg, tmp_path, D, ctx, xs, noise, mean, istd)
    exe = {k: str(pkg.LIB_PATH).replace("libbp_hip.so", k) for k in ("bpenhance", "bpeval")}
    net = ["norm_file=%s" % (tmp_path / "x.norm"), "initwts_file=%s" % (tmp_path / "net.wts"), "layersizes=%s" % ",".join(map(str, ls)),
           "fea_dim=%d" % D, "fea_context=%d" % ctx, "targ_offset=%d" % toff, "traincache=400", "bunchsize=32", "wave_target=mask"]
    g = _glorot(pkg, D, ctx, lrate=0.0)
    M = pkg.WAVE_MASK                                            # (the net's outputs as a mask: samples of the input's size)
    try:
        # offline: all sentences fit one call
        want = g.enhance_waves(xs, mean, istd, ctx, toff, M)
        r = subprocess.run([exe["bpenhance"]] + net + ["wav_list=%s" % (tmp_path / "enh.list"), "nat=dynamic"], capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 1, r.stdout + r.stderr
        for i, y in enumerate(want):
            assert np.array_equal(_read_pcm16(tmp_path / ("enh%d.wav" % i)), _to_pcm16(y)), i
        g.set_nat("static")
        static = g.enhance_waves(xs, mean, istd, ctx, toff, M)
        g.set_nat("dynamic")
        assert not _same(static, want)
        # a stream: one channel, frame t in row t mod bunchsize, as every sentence alone
        alone = [g.enhance_waves([x], mean, istd, ctx, toff, M)[0] for x in xs]
        r = subprocess.run([exe["bpenhance"]] + net + ["wav_list=%s" % (tmp_path / "enh.list"), "nat=dynamic", "stream_block=50"],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 1, r.stdout + r.stderr
        for i, y in enumerate(alone):
            assert np.array_equal(_read_pcm16(tmp_path / ("enh%d.wav" % i)), _to_pcm16(y)), i
        # bpeval: the score lines of eval_mix in the same mode
        r = subprocess.run([exe["bpeval"], "clean_list=%s" % (tmp_path / "clean.list"), "noise_list=%s" % (tmp_path / "noise.list")] + net +
                           ["snr_list=0,5", "init_randem_seed=3", "scores_out=%s" % (tmp_path / "s.txt"), "nat=dynamic"],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 1, r.stdout + r.stderr
        g.set_mix_corpus(xs, noise, mean, istd, ctx, toff)
        plan = pkg.mix_plan(3, len(xs), 1, [x.size for x in noise], [0.0, 5.0])
        ev = g.eval_mix(plan, FS, M)
        rows = [ln.split() for ln in open(tmp_path / "s.txt").read().splitlines()]
        got = np.array([[float(v) for v in row[4:]] for row in rows], np.float32)
        wanted = np.stack([ev["noisy"][:, 0], ev["enhanced"][:, 0], ev["noisy"][:, 1], ev["enhanced"][:, 1], ev["noisy"][:, 2],
                           ev["enhanced"][:, 2]], axis=1)
        assert np.array_equal(_bits(got), _bits(wanted))
        g.set_nat("static")
        assert not np.array_equal(_bits(g.eval_mix(plan, FS, M)["enhanced"]), _bits(ev["enhanced"]))
    finally:
        g.close()
    # errors: the classic baseline has no net input, and a net without the block has no place for the rows
    r = subprocess.run([exe["bpenhance"], "method=logmmse", "fea_dim=%d" % D, "wav_list=%s" % (tmp_path / "enh.list"), "nat=dynamic"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "method=logmmse takes no nat" in r.stdout, r.stdout
    r = subprocess.run([exe["bpenhance"]] + net + ["wav_list=%s" % (tmp_path / "enh.list"), "nat=sometimes"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "nat: sometimes is not static or dynamic" in r.stdout, r.stdout
    import pfile_util as PU
    ls0 = [ctx * D, 64, 48, D]
    W, b = pkg.glorot_net(ls0, seed=5, beta=0.5)
    PU.write_wts(str(tmp_path / "plain.wts"), ls0, W, b)
    plain = [a for a in net if not a.startswith(("initwts_file=", "layersizes="))] + \
        ["initwts_file=%s" % (tmp_path / "plain.wts"), "layersizes=%s" % ",".join(map(str, ls0))]
    for tool, extra in (("bpenhance", ["wav_list=%s" % (tmp_path / "enh.list")]),
                        ("bpeval", ["clean_list=%s" % (tmp_path / "clean.list"), "noise_list=%s" % (tmp_path / "noise.list")])):
        r = subprocess.run([exe[tool]] + plain + extra + ["nat=dynamic"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "nat=dynamic needs a net with the noise-aware block" in r.stdout, r.stdout
