"""GPU tests of the MMSE-SPP noise tracker of the log-MMSE baseline (bp_logmmse_waves_nt, bp_eval_mix_logmmse_nt,
bp_lmstream_open_nt, the lm_noise= key; -m gpu) against the float64 restatement in tests/noise_np.py and against the calls they
are made of.

Bars: G |Y_ref|, out_pcm, out_vad and out_noise within the project's bar max|a - ref| / max|ref| < 1e-4 per sentence
(tests/util.py); tracker mode holds no decision, so no fixture needs a margin.  Everything else -- VAD mode against the calls
without noise parameters, company, streams, the evaluation, the tools -- bit for bit.  The streams run at every frame size
(tests/geometry_cases.py), at the defaults and under noise_np.BUSY: only there does the pbar a channel carries between pushes
move every bin, so only there does "the offline bits" say something about that state."""
import subprocess

import numpy as np
import pytest

import classic_np as CN
import noise_np as NN
from util import TOL, relerr

pytestmark = pytest.mark.gpu
FS = 8000


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(xs, ys):
    return len(xs) == len(ys) and all(np.shape(a) == np.shape(b) and np.array_equal(_bits(a), _bits(b)) for a, b in zip(xs, ys))


_CALLS = {}


def _spp(pkg, D):
    """(pcm, gain, vad, noise) of one tracker call on all fixture sentences of fea_dim D, made once and shared."""
    if D not in _CALLS:
        _CALLS[D] = pkg.logmmse_waves(0, D, NN.fixture(D)[2], noise="spp", return_gain=True, return_vad=True, return_noise=True)
    return _CALLS[D]


def _errors(got, i, r):
    pcm, gain, vad, noise = (o[i] for o in got)
    assert gain.shape == r["G"].shape and noise.shape == r["noise"].shape and vad.shape == r["vad"].shape and pcm.shape == r["pcm"].shape
    assert all(np.isfinite(a).all() for a in (pcm, gain, vad, noise))
    return dict(gain_absY=relerr(gain.astype(np.float64) * r["absY"], r["G"] * r["absY"]), pcm=relerr(pcm, r["pcm"]),
                vad=relerr(vad, r["vad"]), noise=relerr(noise, r["noise"]))


# ---- 1. the restatement
@pytest.mark.parametrize("D", [33, 65, 129, 257])
def test_tracker_matches_restatement(pkg, D, parity_record):
    _, kinds, xs = NN.fixture(D)
    got = _spp(pkg, D)
    worst = {}
    for i, (kind, x) in enumerate(zip(kinds, xs)):
        r = NN.reference(D, i)
        e = _errors(got, i, r)
        print(D, kind, x.size, e)
        parity_record(**{"%d:%s:%d" % (i, kind, x.size): e})
        for k, v in e.items():
            worst[k] = max(worst.get(k, 0.0), v)
        if kind == "zero":                                       # fully silent: bit for bit
            assert not got[0][i].any() and not got[1][i].any()
            assert np.array_equal(_bits(got[3][i]), _bits(r["noise"].astype(np.float32)))
            assert np.all(got[3][i] == np.float32(CN.LAMBDA_FLOOR))
        assert max(e.values()) < TOL, (D, kind, x.size, e)
    parity_record(fea_dim=D, worst=worst)


def test_tracker_wide_spectrum_paths(pkg, parity_record):
    for D, xs in NN.wide_fixtures():
        got = pkg.logmmse_waves(0, D, xs, noise="spp", return_gain=True, return_vad=True, return_noise=True)
        e = _errors(got, 0, NN.reference(D, 0))
        print(D, e)
        parity_record(**{"fea_dim_%d" % D: e})
        assert max(e.values()) < TOL, (D, e)


# ---- 2. tracking on the device
@pytest.mark.parametrize("D", [33, 65, 129, 257])
def test_device_tracker_follows_a_step(pkg, D, parity_record):
    _, kinds, xs = NN.fixture(D)
    i = kinds.index("step")
    spp = NN.step_level_db(_spp(pkg, D)[3][i], D)
    vad = NN.step_level_db(pkg.logmmse_waves(0, D, [xs[i]], noise="vad", return_noise=True)[1][0], D)
    print("fea_dim %d: tracker %.2f dB, VAD-gated %.2f dB of the true noise power" % (D, spp, vad))
    parity_record(fea_dim=D, tracker_db=spp, vad_db=vad)
    assert spp >= -2.5 and vad <= -5.0


# ---- 3. VAD mode is the old code
def test_vad_mode_returns_the_bits_of_the_calls_without_noise(pkg):
    D = 129
    _, kinds, xs = NN.fixture(D)
    old = pkg.logmmse_waves(0, D, xs, return_gain=True, return_vad=True)
    new = pkg.logmmse_waves(0, D, xs, noise="vad", return_gain=True, return_vad=True, return_noise=True)
    for a, b in zip(old, new[:3]):
        assert _same(a, b)
    assert _same(pkg.logmmse_waves(0, D, xs, noise={"mode": 0, "q": 0.3, "a_pow": 0.5}), old[0])   # the rest is not read
    assert _same(pkg.logmmse_waves(0, D, xs, CN.ALT, noise="vad"), pkg.logmmse_waves(0, D, xs, CN.ALT))
    assert not _same(_spp(pkg, D)[0], old[0])
    for i, x in enumerate(xs):                                    # row 0: the noise start, rounded once
        Y = CN.analysis(x, D)
        P = Y.real ** 2 + Y.imag ** 2
        start = np.maximum(P[:min(6, P.shape[0])].mean(axis=0), CN.LAMBDA_FLOOR)
        assert relerr(new[3][i][0], start) < TOL, kinds[i]
    # to the bit: silence gives the floor, and a frame the VAD does not call noise hands its lambda on unchanged
    z = kinds.index("zero")
    assert np.all(new[3][z] == np.float32(CN.LAMBDA_FLOOR))
    t = kinds.index("tones")
    keep = np.flatnonzero(new[2][t][:-1] >= CN.DEFAULTS["eta"])
    move = np.flatnonzero(new[2][t][:-1] < CN.DEFAULTS["eta"])
    assert keep.size and move.size
    assert np.array_equal(_bits(new[3][t][keep + 1]), _bits(new[3][t][keep]))
    assert all((new[3][t][k + 1] != new[3][t][k]).any() for k in move)


# ---- 4. company
@pytest.mark.parametrize("D", [33, 257])
def test_a_sentence_alone_and_in_the_batch_and_twice(pkg, D):
    _, kinds, xs = NN.fixture(D)
    got = _spp(pkg, D)
    again = pkg.logmmse_waves(0, D, xs, noise="spp", return_gain=True, return_vad=True, return_noise=True)
    for a, b in zip(got, again):
        assert _same(a, b)
    assert _same(pkg.logmmse_waves(0, D, xs, noise="spp"), got[0])  # without the optional outputs
    assert _same(pkg.logmmse_waves(0, D, xs, noise=pkg.noise_params(None)), got[0])
    for i in range(len(xs)):
        one = pkg.logmmse_waves(0, D, [xs[i]], noise="spp", return_gain=True, return_vad=True, return_noise=True)
        for a, b in zip(one, got):
            assert _same(a, [b[i]]), (D, kinds[i])


# ---- 5. streams
def _schedule(n, hop, whole):
    """Block sizes of irregular kinds: 1, 7, hop - 1, 160 in turn, or the whole sentence."""
    if whole:
        return [n]
    out, k, cyc = [], 0, (1, 7, hop - 1, 160)
    while sum(out) < n:
        out.append(min(cyc[k % 4], n - sum(out)))
        k += 1
    return out


def _play(pkg, s, chans, hop):
    """chans: per channel a list of sentences.  Every channel pushes its blocks in lockstep, the end flag on a sentence's last
    block; returns per channel the list of finished sentences."""
    plans = []
    for c, sents in enumerate(chans):
        p = []
        for k, x in enumerate(sents):
            sizes = _schedule(x.size, hop, (c + k) % 4 == 3)
            pos = np.concatenate([[0], np.cumsum(sizes)])
            p += [(x[pos[j]:pos[j + 1]], j == len(sizes) - 1) for j in range(len(sizes))]
        plans.append(p)
    out = [[[]] for _ in chans]
    empty = np.zeros(0, np.float32)
    for k in range(max(len(p) for p in plans)):
        items = [p[k] if k < len(p) else (empty, False) for p in plans]
        got = s.push([b for b, _ in items], [e for _, e in items])
        for c, ((_, e), y) in enumerate(zip(items, got)):
            out[c][-1].append(y)
            if e:
                out[c].append([])
    return [[np.concatenate(s) for s in o[:-1]] for o in out]


def _wide_plan(x, hop, schedule):
    """The sentence in hop-sized blocks or as one block, the end flag on the last."""
    sizes = [x.size] if schedule == "one" else [hop] * (x.size // hop) + ([x.size % hop] if x.size % hop else [])
    pos = np.concatenate([[0], np.cumsum(sizes)])
    return [(x[pos[j]:pos[j + 1]], j == len(sizes) - 1) for j in range(len(sizes))]


def _wide_streams(pkg, D, noise):
    """fea_dim 513 and 1025 (3 and 5 bins per thread): the third sentence of classic_np's wide call and, on a second channel, the
    first one, so that the per-channel state is read at a stride of D with several bins per thread; the schedules "hop" and "one"
    as tests/test_lmstream_gpu.py::test_wide_spectra plays them.  Returns the samples that differ from the offline call."""
    xs = [w for w in CN.wide_fixtures() if w[0] == D][0][1]
    sents = [xs[2], xs[0]]
    ref = [pkg.logmmse_waves(0, D, [x], noise=noise)[0] for x in sents]
    assert not np.array_equal(_bits(ref[0]), _bits(pkg.logmmse_waves(0, D, [sents[0]], noise="vad")[0]))
    differing = 0
    empty = np.zeros(0, np.float32)
    for schedule in ("hop", "one"):
        plans = [_wide_plan(x, D - 1, schedule) for x in sents]
        out = [[] for _ in sents]
        with pkg.logmmse_stream_open(0, D, n_chan=2, max_push_samples=sum(x.size for x in sents), noise=noise) as s:
            for k in range(max(len(p) for p in plans)):
                items = [p[k] if k < len(p) else (empty, False) for p in plans]
                for c, y in enumerate(s.push([b for b, _ in items], [e for _, e in items])):
                    out[c].append(y)
        for c, r in enumerate(ref):
            y = np.concatenate(out[c])
            assert y.shape == r.shape, (D, schedule, c)
            differing += int((_bits(y) != _bits(r)).sum())
    return differing


@pytest.mark.parametrize("D", [33, 65, 129, 257, 513, 1025])
def test_tracker_streams_return_the_offline_bits(pkg, D, parity_record):
    if D > 257:
        # at the defaults, and under noise_np.BUSY: the carried pbar then moves every bin (tests/test_noise_host.py), and the offline
        # call the stream is compared with is itself held to the restatement under these parameters
        x = [w for w in CN.wide_fixtures() if w[0] == D][0][1][2]
        e = _errors(pkg.logmmse_waves(0, D, [x], noise=NN.BUSY, return_gain=True, return_vad=True, return_noise=True), 0,
                    NN.enhance(x, D, noise=NN.BUSY))
        differing = {"defaults": _wide_streams(pkg, D, "spp"), "busy": _wide_streams(pkg, D, NN.BUSY)}
        print(D, e, differing)
        parity_record(fea_dim=D, sentences=2, samples_differing=sum(differing.values()), by_parameters=differing, offline_busy=e)
        assert max(e.values()) < TOL, (D, e)
        assert differing == {"defaults": 0, "busy": 0}
        return
    _, kinds, xs = NN.fixture(D)
    ref = _spp(pkg, D)[0]
    sus, ton = kinds.index("sustained"), kinds.index("tones")
    # channel 0: sustained and then tones -- pbar must start again at the end flag; the others share the rest
    order = [[sus, ton, kinds.index("one")], [i for i in range(len(xs)) if i not in (sus, ton)][0::2],
             [i for i in range(len(xs)) if i not in (sus, ton)][1::2] + [sus]]
    chans = [[xs[i] for i in o] for o in order]
    with pkg.logmmse_stream_open(0, D, n_chan=3, max_push_samples=3 * 16000, noise="spp") as s:
        got = _play(pkg, s, chans, D - 1)
    for c, o in enumerate(order):
        assert len(got[c]) == len(o)
        for y, i in zip(got[c], o):
            assert np.shape(y) == np.shape(ref[i]) and np.array_equal(_bits(y), _bits(ref[i])), (D, c, kinds[i])
    # under noise_np.BUSY the carried pbar moves every bin (tests/test_noise_host.py), not only those of a sustained tone
    ref_busy = pkg.logmmse_waves(0, D, xs, noise=NN.BUSY)
    with pkg.logmmse_stream_open(0, D, n_chan=3, max_push_samples=3 * 16000, noise=NN.BUSY) as s:
        busy = _play(pkg, s, chans, D - 1)
    differing = sum(int((_bits(y) != _bits(ref_busy[i])).sum()) if y.shape == ref_busy[i].shape else max(y.size, ref_busy[i].size)
                    for c, o in enumerate(order) for y, i in zip(busy[c], o))
    parity_record(fea_dim=D, sentences=sum(len(o) for o in order), samples_differing=differing)
    assert differing == 0 and not _same(ref_busy, ref)
    # a VAD-mode stream opened with noise parameters against one opened without, on the same pushes
    with pkg.logmmse_stream_open(0, D, n_chan=3, max_push_samples=3 * 16000, noise="vad") as a:
        new = _play(pkg, a, chans, D - 1)
    with pkg.logmmse_stream_open(0, D, n_chan=3, max_push_samples=3 * 16000) as b:
        old = _play(pkg, b, chans, D - 1)
    for c in range(3):
        assert _same(new[c], old[c])
    assert not _same(new[0], got[0])


# ---- 6. the evaluation
ED, CTX, TOFF = 129, 3, 1


def _corpus(rng):
    clean = [CN.gated_tones(s, n, ED, 40.0, sigma=30.0) for s, n in ((21, 9000), (22, 6000), (23, 12000))]
    noise = [np.round(rng.normal(0, 800, 7000)).astype(np.float32), np.zeros(500, np.float32)]
    return clean, noise


def test_eval_mix_logmmse_nt_is_its_parts(pkg, parity_record):
    rng = np.random.default_rng(11)
    clean, noise = _corpus(rng)
    mean, istd = rng.normal(10.0, 2.0, ED).astype(np.float32), rng.uniform(0.2, 0.5, ED).astype(np.float32)
    plan = np.zeros(4, pkg.MIXTURE_DTYPE)
    for i, m in enumerate([(0, 0, 11, 0.0), (1, 1, 3, 5.0), (2, 0, 6999, 10.0), (1, 0, 100, -5.0)]):
        plan[i] = m
    ls = [CTX * ED, 64, ED]
    W, b = pkg.glorot_net(ls, seed=5, beta=0.5)
    g = pkg.BP_GPU(1, 3, ls, 32, 0.05, 0.5, 0.0, W, b, max_chunk_frames=1200)
    try:
        g.set_mix_corpus(clean, noise, mean, istd, CTX, TOFF, "lps")
        w0, d0 = g.get_weights(), g.get_deltas()
        lens = [clean[c].size for c in plan["clean"]]
        mix = np.split(g.mix_features(plan)["pcm"], np.cumsum(lens)[:-1])
        refs = [clean[c] for c in plan["clean"]]
        enh = pkg.logmmse_waves(0, ED, mix, noise="spp")
        for ext in (False, True):
            ev = g.eval_mix_logmmse(plan, FS, return_pcm=True, extended=ext, noise="spp")
            assert ev["enhanced"].shape == (4, 5 if ext else 3)
            assert _same(ev["pcm"], enh)
            assert np.array_equal(_bits(ev["noisy"]), _bits(pkg.score_waves(0, ED, FS, refs, mix, extended=ext)))
            assert np.array_equal(_bits(ev["enhanced"]), _bits(pkg.score_waves(0, ED, FS, refs, enh, extended=ext)))
            old = g.eval_mix_logmmse(plan, FS, return_pcm=True, extended=ext)
            vad = g.eval_mix_logmmse(plan, FS, return_pcm=True, extended=ext, noise="vad")
            assert _same(vad["pcm"], old["pcm"]) and not _same(vad["pcm"], enh)
            assert np.array_equal(_bits(vad["enhanced"]), _bits(old["enhanced"])) and np.array_equal(_bits(vad["noisy"]), _bits(old["noisy"]))
        alt = g.eval_mix_logmmse(plan, FS, CN.ALT, return_pcm=True, noise={"a_pow": 0.7})
        assert _same(alt["pcm"], pkg.logmmse_waves(0, ED, mix, CN.ALT, noise={"a_pow": 0.7}))
        for bad in ({"mode": 3}, {"q": 0.0}, {"p_lo": 0.995}):
            with pytest.raises(pkg.BPError, match="status -1"):
                g.eval_mix_logmmse(plan, FS, noise=bad)
        w1, d1 = g.get_weights(), g.get_deltas()
        for a, c in zip(w0 + d0, w1 + d1):
            for x, y in zip(a, c):
                assert (x is None and y is None) or np.array_equal(_bits(x), _bits(y))
        parity_record(noisy=ev["noisy"].tolist(), logmmse_spp=ev["enhanced"].tolist(), logmmse_vad=old["enhanced"].tolist())
    finally:
        g.close()


# ---- 7. the tools
def _write_pcm16(path, x, rate):
    import wave
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(rate)
        w.writeframes(np.asarray(x, np.int16).tobytes())


def _read_pcm16(path):
    import wave
    with wave.open(str(path), "rb") as w:
        return np.frombuffer(w.readframes(w.getnframes()), np.int16), w.getframerate()


def test_bpenhance_lm_noise_spp(pkg, tmp_path):
    exe = str(pkg.LIB_PATH).replace("libbp_hip.so", "bpenhance")
    D = 129
    _, kinds, xs = NN.fixture(D)
    want = [np.clip(np.rint(y), -32768, 32767).astype(np.int16) for y in _spp(pkg, D)[0]]
    for i, x in enumerate(xs):
        _write_pcm16(tmp_path / ("in%d.wav" % i), x, FS)
    for tag, keys in (("off", []), ("live", ["lm_stream_block=160", "lm_stream_chan=2"]), ("vad", ["lm_noise=vad"])):
        (tmp_path / tag).mkdir()
        (tmp_path / (tag + ".list")).write_text("".join("%s %s\n" % (tmp_path / ("in%d.wav" % i), tmp_path / tag / ("out%d.wav" % i))
                                                        for i in range(len(xs))))
        noise = [] if tag == "vad" else ["lm_noise=spp"]
        r = subprocess.run([exe, "method=logmmse", "fea_dim=%d" % D, "wav_list=%s" % (tmp_path / (tag + ".list"))] + noise + keys,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "logmmse" in r.stdout and ("streamed" in r.stdout) == (tag == "live"), r.stdout + r.stderr
    old = pkg.logmmse_waves(0, D, xs)
    for i in range(len(xs)):
        for tag in ("off", "live"):
            y, rate = _read_pcm16(tmp_path / tag / ("out%d.wav" % i))
            assert rate == FS and np.array_equal(y, want[i]), (tag, kinds[i])
        y, _ = _read_pcm16(tmp_path / "vad" / ("out%d.wav" % i))
        assert np.array_equal(y, np.clip(np.rint(old[i]), -32768, 32767).astype(np.int16)), kinds[i]
    assert any(not np.array_equal(w, np.clip(np.rint(o), -32768, 32767).astype(np.int16)) for w, o in zip(want, old))


def test_bpeval_lm_noise_spp(pkg, tmp_path):
    import pfile_util as PU
    exe = str(pkg.LIB_PATH).replace("libbp_hip.so", "bpeval")
    rng = np.random.default_rng(21)
    clean, noise = _corpus(rng)
    mean, istd = rng.normal(10.0, 2.0, ED).astype(np.float32), rng.uniform(0.2, 0.5, ED).astype(np.float32)
    for tag, xs in (("clean", clean), ("noise", noise)):
        for i, x in enumerate(xs):
            _write_pcm16(tmp_path / ("%s%d.wav" % (tag, i)), x, FS)
        (tmp_path / (tag + ".list")).write_text("".join("%s\n" % (tmp_path / ("%s%d.wav" % (tag, i))) for i in range(len(xs))))
    (tmp_path / "x.norm").write_text("<mean>\n" + "".join("%.9g\n" % v for v in mean) + "<inverse std>\n" +
                                     "".join("%.9g\n" % v for v in istd))
    ls = [CTX * ED, 64, ED]
    W, b = pkg.glorot_net(ls, seed=5, beta=0.5)
    PU.write_wts(str(tmp_path / "net.wts"), ls, W, b)
    seed, snrs, per, cache = 77, [0.0, 10.0], 2, 400
    keys = ["clean_list=%s" % (tmp_path / "clean.list"), "noise_list=%s" % (tmp_path / "noise.list"), "norm_file=%s" % (tmp_path / "x.norm"),
            "initwts_file=%s" % (tmp_path / "net.wts"), "fea_dim=%d" % ED, "fea_context=%d" % CTX, "targ_offset=%d" % TOFF,
            "layersizes=%s" % ",".join(map(str, ls)), "snr_list=0,10", "mix_per_clean=%d" % per, "init_randem_seed=%d" % seed,
            "traincache=%d" % cache, "bunchsize=32", "baseline=logmmse"]
    runs = {}
    for tag, extra in (("none", []), ("vad", ["lm_noise=vad"]), ("spp", ["lm_noise=spp"]), ("spp5", ["lm_noise=spp", "scores=extended"])):
        r = subprocess.run([exe] + keys + extra + ["scores_out=%s" % (tmp_path / (tag + ".txt"))], capture_output=True, text=True, timeout=300)
        assert r.returncode == 1, r.stdout + r.stderr
        runs[tag] = (r.stdout, [ln.split() for ln in open(tmp_path / (tag + ".txt")).read().splitlines()])
    assert runs["vad"] == runs["none"]                            # the default, byte for byte
    assert [r[:10] for r in runs["spp"][1]] == [r[:10] for r in runs["none"][1]] and runs["spp"][1] != runs["none"][1]
    plan = pkg.mix_plan(seed, len(clean), per, [x.size for x in noise], snrs)
    g = pkg.BP_GPU(1, 3, ls, 32, 0.0, 0.0, 0.0, W, b, max_chunk_frames=cache)
    try:
        g.set_mix_corpus(clean, noise, mean, istd, CTX, TOFF, "lps")
        T = g.mix_frames(plan) + CTX - 1                          # bpeval's cut: calls of at most traincache rows
        want, want5, first, rows_ = [], [], 0, 0
        for i in range(len(plan) + 1):
            if i == len(plan) or rows_ + T[i] > cache:
                want.append(g.eval_mix_logmmse(plan[first:i], FS, noise="spp")["enhanced"])
                want5.append(g.eval_mix_logmmse(plan[first:i], FS, noise="spp", extended=True)["enhanced"])
                first, rows_ = i, 0
            if i < len(plan):
                rows_ += T[i]
        want, want5 = np.concatenate(want), np.concatenate(want5)
    finally:
        g.close()
    assert [r[10:] for r in runs["spp"][1]] == [["%.9g" % v for v in w] for w in want]
    assert [r[-5:] for r in runs["spp5"][1]] == [["%.9g" % v for v in w] for w in want5]
