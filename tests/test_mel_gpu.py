"""GPU tests of the MFCC auxiliary target (bp_wave_mfcc, bp_set_mix_aux; include/bp_c_api.h; -m gpu) against
the restatement in tests/mel_np.py.

Bars.  sqrt(power): 1e-5 of the frame's largest magnitude (the analysis bar of test_wave_gpu.py).  logmel: LOGMEL_ULP fp32 ulp
from ln of the e restated from the device's own power and the library's w (the restatement is exact, only logf remains; measured
worst distance at the first four geometries: 1.82, 2.08, 2.13 and 2.14 ulp; the bar is twice the worst rounded up to a whole ulp;
above 8 ulp would be a defect; the geometries at fea_dim 65 and 513, added under the same bar, measure 1.78 and 2.10 ulp).
mfcc: np.array_equal with the restated DCT of the device's own logmel.  Everything else bit for bit."""
import math
import os
import subprocess

import numpy as np
import pytest

import mel_np as MN
import wave_np as WN

pytestmark = pytest.mark.gpu

LOGMEL_ULP = 5.0
D, CTX, TOFF, NC = 33, 3, 1, 5                                   # the mixing tests' net: [(CTX + 1) D -> 64 -> D + NC + D]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _mel(pkg, g, **kw):
    return pkg.mel_params(g["sample_rate"], n_mel=g["n_mel"], n_ceps=g["n_ceps"], first_coef=g["first_coef"], lifter=g["lifter"], **kw)


# ---- 1. bp_wave_mfcc at the six geometries, one per frame size
@pytest.mark.parametrize("g", MN.GEOMETRIES, ids=MN.geo_id)
def test_wave_mfcc_matches_restatement(pkg, g, parity_record):
    Dg = g["fea_dim"]
    sents = MN.make_sentences(g, 1000 + Dg)
    rng = np.random.default_rng(Dg)
    mean = rng.normal(0.0, 3.0, g["n_ceps"]).astype(np.float32)
    scale = rng.uniform(0.05, 0.5, g["n_ceps"]).astype(np.float32)
    mp = _mel(pkg, g, mean=mean, scale=scale)
    w, first, nb = pkg.mel_filters(Dg, mp)
    t = pkg.mel_dct(mp)
    out = pkg.wave_mfcc(0, Dg, sents, mp, return_logmel=True, return_power=True)
    worst_a = worst_b = worst_e = 0.0
    for s, x in enumerate(sents):
        P, lm, cc = out["power"][s], out["logmel"][s], out["mfcc"][s]
        T = WN.n_frames(x.size, Dg)
        assert P.shape == (T, Dg) and lm.shape == (T, g["n_mel"]) and cc.shape == (T, g["n_ceps"])
        # (a) the analysis
        mag = np.abs(WN.analysis(x, Dg))
        top = mag.max(axis=1, keepdims=True)
        ea = float((np.abs(np.sqrt(P.astype(np.float64)) - mag) / np.maximum(top, 1e-30)).max()) if top.max() > 0 else float(np.abs(P).max())
        worst_a = max(worst_a, ea)
        # (b) logmel from the device's own power: only logf remains
        e = MN.mel_energy(P, w, first, nb)
        ref = MN.log_floor(e)
        floor = ~(e > np.float32(1e-10))
        assert np.array_equal(_bits(lm[floor]), _bits(np.full(int(floor.sum()), MN.LN_FLOOR32)))
        if (~floor).any():
            worst_b = max(worst_b, MN.ulp_distance(lm[~floor], ref[~floor]))
        # (c) the cepstrum of the device's own logmel
        assert np.array_equal(_bits(cc), _bits(MN.cepstrum(lm, t, mean, scale))), "sentence %d" % s
        # (e) information: e against the pure float64 chain
        e64 = MN.mfcc64(x, g)[0]
        if e64.max() > 0:
            worst_e = max(worst_e, float((np.abs(e.astype(np.float64) - e64) / e64.max(axis=1, keepdims=True)).max()))
    silent = out["logmel"][-1]
    assert np.array_equal(_bits(silent), _bits(np.full(silent.shape, MN.LN_FLOOR32))), "the silent sentence is the floor in every filter"
    print("geometry %s: sqrt(power) %.3g of the frame's top, logmel %.3f ulp, e vs float64 chain %.3g" % (MN.geo_id(g), worst_a, worst_b, worst_e))
    parity_record(sqrt_power_rel=worst_a, logmel_ulp=worst_b, e_vs_f64_rel=worst_e, bar_logmel_ulp=LOGMEL_ULP)
    assert worst_a <= 1e-5, worst_a
    assert worst_b <= 8.0, "a defect, not a tolerance: %.3f ulp" % worst_b
    assert worst_b <= LOGMEL_ULP, worst_b
    # (d) alone against among the others, the call twice, outputs on or off: bit for bit
    again = pkg.wave_mfcc(0, Dg, sents, mp, return_logmel=True, return_power=True)
    only = pkg.wave_mfcc(0, Dg, sents, mp)
    lm_only = pkg.wave_mfcc(0, Dg, sents, mp, return_logmel=True)
    for s in range(len(sents)):
        for k in ("power", "logmel", "mfcc"):
            assert np.array_equal(_bits(out[k][s]), _bits(again[k][s])), (k, s)
        assert np.array_equal(_bits(out["mfcc"][s]), _bits(only[s]))
        assert np.array_equal(_bits(out["logmel"][s]), _bits(lm_only["logmel"][s])) and np.array_equal(_bits(out["mfcc"][s]), _bits(lm_only["mfcc"][s]))
    for s in (0, 3, len(sents) - 1):
        alone = pkg.wave_mfcc(0, Dg, [sents[s]], mp, return_logmel=True, return_power=True)
        for k in ("power", "logmel", "mfcc"):
            assert np.array_equal(_bits(out[k][s]), _bits(alone[k][0])), (k, s)


# ---- 2 .. 5: mixing
def _corpus(rng, fea=D):
    clean = [x + np.float32(0.0) for x in WN.make_sentences(rng, [1, 700, 2 * (fea - 1), 1500])]
    noise = WN.make_sentences(rng, [37, 3000], scale=2000.0)
    return clean, noise


def _rir(rng):
    h = (rng.normal(size=200) * np.exp(-np.arange(200) / 40.0)).astype(np.float32)
    h[7] = 3.0                                                   # the direct path
    return h


def _plan(pkg):
    mixes = [(0, 1, 2999, 0.0), (1, 0, 5, -10.0), (4, 1, 100, 5.0), (2, 1, 100, 0.0), (3, 1, 2999, 20.0), (3, 0, 36, -5.0)]
    p = np.zeros(len(mixes), pkg.MIXTURE_DTYPE)
    for i, m in enumerate(mixes):
        p[i] = m
    return p


def _norm(rng, fea=D):
    return rng.normal(10.0, 2.0, fea).astype(np.float32), rng.uniform(0.2, 0.5, fea).astype(np.float32)


def _aux_geo(fea=D):
    return dict(fea_dim=fea, sample_rate=8000, n_mel=8, n_ceps=NC, first_coef=1, lifter=0.0)


def _aux(pkg, rng=None, fea=D):
    kw = {}
    if rng is not None:
        kw = dict(mean=rng.normal(0.0, 3.0, NC).astype(np.float32), scale=rng.uniform(0.05, 0.5, NC).astype(np.float32))
    return _mel(pkg, _aux_geo(fea), **kw)


def _sl(target, aux, fea=D):
    return fea * (2 if target in ("lps+irm", "lps+ibm") else 1) + (NC if aux else 0)


def _handle(pkg, target, aux, compute_dtype=0, train=False, B=32, fea=D):
    ls = [(CTX + 1) * fea, 64, _sl(target, aux, fea)]
    W, b = pkg.glorot_net(ls, seed=5, beta=0.5)
    kw = dict(max_chunk_frames=2000, compute_dtype=compute_dtype)
    if train:
        kw.update(dropoutflag=1, visible_omit=0.1, hid_omit=0.2, seed=99)
    g = pkg.BP_GPU(1, 3, ls, B, 0.01, 0.5, 1e-4, W, b, **kw)
    if target != "lps":
        g.set_output(1, fea + (NC if aux else 0), 0)
    return g


def _set(pkg, g, rng_seed, target, mel, reverb=True, fea=D):
    rng = np.random.default_rng(rng_seed)
    clean, noise = _corpus(rng, fea)
    mean, istd = _norm(rng, fea)
    h = _rir(rng)
    g.set_mix_aux(mel)
    g.set_mix_corpus(clean, noise, mean, istd, CTX, TOFF, target, 3.0)
    if reverb:
        g.set_mix_reverb([h], [1], [0], "early", 20)            # entry 4: sentence 1 in the room, the early part as target
    return clean, noise, mean, istd, h


def _target_signals(pkg, clean, h, plan):
    early = pkg.reverb_waves(0, [clean[1]], [0], [h], 20, early=True)[1][0]
    return [early if c == 4 else clean[c] for c in plan["clean"]]


# (the three targets at fea_dim 33, and once at 257: two bins per thread and the MFCC columns behind a 257-wide LPS block)
@pytest.mark.parametrize("target,fea", [("lps", D), ("lps+irm", D), ("lps+ibm", D), ("lps+irm", 257)], ids=["lps", "lps+irm", "lps+ibm", "lps+irm-257"])
def test_mfcc_columns_are_wave_mfcc_of_the_target_signal(pkg, target, fea, parity_record):
    plan = _plan(pkg)
    mel = _aux(pkg, np.random.default_rng(8), fea)
    g, ref = _handle(pkg, target, True, fea=fea), _handle(pkg, target, False, fea=fea)
    try:
        clean, noise, mean, istd, h = _set(pkg, g, 21, target, mel, fea=fea)
        _set(pkg, ref, 21, target, None, fea=fea)
        assert g.mix_aux_dims == (8, NC) and ref.mix_aux_dims is None
        got, base = g.mix_features(plan), ref.mix_features(plan)
        want = np.concatenate(pkg.wave_mfcc(0, fea, _target_signals(pkg, clean, h, plan), mel))
        assert got["targ"].shape == (want.shape[0], _sl(target, True, fea))
        parity_record(fea_dim=fea, words_differing=int((_bits(got["targ"][:, fea:fea + NC]) != _bits(want)).sum()))
        assert np.array_equal(_bits(got["targ"][:, fea:fea + NC]), _bits(want))
        assert np.array_equal(_bits(got["targ"][:, :fea]), _bits(base["targ"][:, :fea]))
        if target != "lps":
            assert np.array_equal(_bits(got["targ"][:, fea + NC:]), _bits(base["targ"][:, fea:]))
        for k in ("fea", "lps", "nat", "pcm"):
            assert np.array_equal(_bits(got[k]), _bits(base[k])), k
    finally:
        g.close()
        ref.close()


def _weights_equal(a, b):
    (wa, ba), (da, dba) = a.get_weights(), a.get_deltas()
    (wb, bb), (db, dbb) = b.get_weights(), b.get_deltas()
    return all(np.array_equal(_bits(u), _bits(v)) for l in range(1, a.numlayers)
               for u, v in ((wa[l], wb[l]), (ba[l], bb[l]), (da[l], db[l]), (dba[l], dbb[l])))


def _host_chunk(g, plan, order=None):
    import mix_np as MX
    f = g.mix_features(plan)
    frames = g.mix_frames(plan)
    rows = MX.staged_rows(f["fea"], frames, CTX, TOFF)
    tg = np.zeros((rows.shape[0], f["targ"].shape[1]), np.float32)
    tg[:f["targ"].shape[0]] = f["targ"]
    ws, tf, nr = MX.window_tables(frames, CTX, order)
    return rows, tg, ws, tf, f["nat"], nr, f["targ"]


@pytest.mark.parametrize("compute_dtype", [0, 1])
def test_training_with_aux_equals_the_window_path(pkg, compute_dtype):
    plan = _plan(pkg)
    mel = _aux(pkg, np.random.default_rng(9))
    a, b = (_handle(pkg, "lps+ibm", True, compute_dtype, train=True) for _ in range(2))
    try:
        for g in (a, b):
            _set(pkg, g, 22, "lps+ibm", mel)
        for ci, (p, shuffled) in enumerate([(plan[:4], True), (plan[3:], False)]):
            T = int(a.mix_frames(p).sum())
            order = pkg.mix_shuffle(345, ci, T) if shuffled else None
            a.train_mix(p, order)
            rows, tg, ws, tf, nat, nr, _ = _host_chunk(b, p, order)
            b.train_windows(rows, tg, CTX, ws, tf, nat=nat, nat_row=nr)
        assert _weights_equal(a, b)
        # CV: the fp32 sum over all columns, samples in order, columns in order (bp_cv_chunk_windows' sum on the same data)
        ea = a.CrossValid_mix(plan)
        rows, tg, ws, tf, nat, nr, targ = _host_chunk(b, plan)
        eb = b.CrossValid_windows(rows, tg, CTX, ws, tf, nat=nat, nat_row=nr)
        assert np.float32(ea).view(np.uint32) == np.float32(eb).view(np.uint32), (ea, eb)
        if compute_dtype == 0:
            _, net = b.enhance_waves(np.split(b.mix_features(plan)["pcm"], np.cumsum([b.mix_clean_len[c] for c in plan["clean"]])[:-1]),
                                     *_norm_of(22), CTX, TOFF, pkg.WAVE_MASK, D + NC, return_net=True)
            d = (np.concatenate(net).astype(np.float64) - targ.astype(np.float64)) ** 2
            assert targ.shape[1] == 2 * D + NC and abs(ea - d.sum()) <= 1e-4 * d.sum(), (ea, d.sum())
    finally:
        a.close()
        b.close()


def _norm_of(seed):
    rng = np.random.default_rng(seed)
    _corpus(rng)
    return _norm(rng)


@pytest.mark.parametrize("target,out_col", [(1, D + NC), (0, 0)])
def test_eval_mix_from_a_three_part_net_is_its_parts(pkg, target, out_col):
    plan = _plan(pkg)
    g = _handle(pkg, "lps+irm", True)
    try:
        clean, noise, mean, istd, h = _set(pkg, g, 23, "lps+irm", _aux(pkg))
        ev = g.eval_mix(plan, 8000, target, out_col, return_pcm=True)
        lens = [g.mix_clean_len[c] for c in plan["clean"]]
        mix = np.split(g.mix_features(plan)["pcm"], np.cumsum(lens)[:-1])
        enh = g.enhance_waves(mix, mean, istd, CTX, TOFF, target, out_col)
        refs = _target_signals(pkg, clean, h, plan)
        for x, y in zip(ev["pcm"], enh):
            assert np.array_equal(_bits(x), _bits(y))
        assert np.array_equal(_bits(ev["noisy"]), _bits(pkg.score_waves(0, D, 8000, refs, mix)))
        assert np.array_equal(_bits(ev["enhanced"]), _bits(pkg.score_waves(0, D, 8000, refs, enh)))
        with pytest.raises(pkg.BPError, match="status -1"):
            g.eval_mix(plan, 8000, target, D + NC + 1)
    finally:
        g.close()


def _free_device_bytes():
    """hipMemGetInfo's free figure, from the runtime the library itself is linked to."""
    import ctypes
    path = [ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln][0]      # (loaded with libbp_hip.so)
    hip = ctypes.CDLL(path)
    free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return int(free.value)


def test_aux_takes_effect_at_the_next_corpus_and_costs_no_memory_after_the_first_call(pkg):
    plan = _plan(pkg)
    mel5 = _aux(pkg, np.random.default_rng(10))
    other = _mel(pkg, dict(_aux_geo(), n_mel=10, lifter=22.0))
    g, fresh = _handle(pkg, "lps+irm", True), _handle(pkg, "lps+irm", False)
    try:
        _set(pkg, g, 24, "lps+irm", mel5)
        t0 = g.mix_features(plan)["targ"]
        g.set_mix_aux(other)                                     # the corpus that is set keeps its tables
        assert np.array_equal(_bits(g.mix_features(plan)["targ"]), _bits(t0)) and g.mix_aux_dims == (8, NC)
        g.set_mix_aux(None)
        assert np.array_equal(_bits(g.mix_features(plan)["targ"]), _bits(t0))
        free = []
        for i in range(20):
            g.set_mix_aux(other if i % 2 else mel5)
            free.append(_free_device_bytes())
        assert len(set(free)) == 1, free
        assert np.array_equal(_bits(g.mix_features(plan)["targ"]), _bits(t0))
        # off, then a corpus: a fresh handle's targets (the net must then be the two-part one)
        g.set_mix_aux(None)
        with pytest.raises(pkg.BPError, match="status -1"):
            _set(pkg, g, 24, "lps+irm", None)                    # layersizes[last] is 2 D + NC
        assert np.array_equal(_bits(g.mix_features(plan)["targ"]), _bits(t0))
    finally:
        g.close()
    g = _handle(pkg, "lps+irm", False)
    try:
        g.set_mix_aux(mel5)
        g.set_mix_aux(None)
        _set(pkg, g, 24, "lps+irm", None)
        _set(pkg, fresh, 24, "lps+irm", None)
        a, b = g.mix_features(plan), fresh.mix_features(plan)
        for k in ("fea", "lps", "targ", "nat", "pcm"):
            assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    finally:
        g.close()
        fresh.close()


def test_errors_leave_the_handle_unchanged(pkg):
    plan = _plan(pkg)
    mel = _aux(pkg, np.random.default_rng(11))
    a, b = (_handle(pkg, "lps+ibm", True, train=True) for _ in range(2))
    try:
        for g in (a, b):
            clean, noise, mean, istd, h = _set(pkg, g, 25, "lps+ibm", mel)
        bad = [dict(n_mel=1), dict(n_mel=129), dict(n_ceps=0), dict(n_ceps=8), dict(first_coef=2), dict(f_lo=-1.0), dict(f_hi=4000.5),
               dict(f_lo=3000.0, f_hi=3000.0), dict(lifter=-1.0), dict(lifter=float("nan")), dict(sample_rate=0)]
        for kw in bad:
            m = _aux(pkg)
            for k, v in kw.items():
                setattr(m, k, v)
            with pytest.raises(pkg.BPError, match="status -1"):
                a.set_mix_aux(m)
        m = _aux(pkg, np.random.default_rng(1))
        m._keep_scale[2] = np.inf
        with pytest.raises(pkg.BPError, match="status -1"):
            a.set_mix_aux(m)
        with pytest.raises(pkg.BPError, match="begin with LPS"):
            a.set_mix_corpus(clean, noise, mean, istd, CTX, TOFF, "irm", 3.0)
        a.set_mix_aux(_mel(pkg, dict(_aux_geo(), n_ceps=6)))       # layersizes[last] is 2 D + 5
        with pytest.raises(pkg.BPError, match="parts\\*fea_dim \\+ n_ceps = 72"):
            a.set_mix_corpus(clean, noise, mean, istd, CTX, TOFF, "lps+ibm", 3.0)
        a.set_mix_aux(_mel(pkg, dict(_aux_geo(), n_mel=26, n_ceps=NC)))   # 26 filters do not fit 33 bins at 8 kHz
        with pytest.raises(pkg.BPError, match="mel filter 0 holds no bin"):
            a.set_mix_corpus(clean, noise, mean, istd, CTX, TOFF, "lps+ibm", 3.0)
        assert a.mix_aux_dims == (8, NC)
        T = int(a.mix_frames(plan).sum())
        order = pkg.mix_shuffle(3, 0, T)
        fa, fb = a.mix_features(plan), b.mix_features(plan)
        assert np.array_equal(_bits(fa["targ"]), _bits(fb["targ"]))
        a.train_mix(plan, order)
        b.train_mix(plan, order)
        assert _weights_equal(a, b)
        a.dp_attach(1, 0, "mel-%d" % os.getpid())
        with pytest.raises(pkg.BPError, match="status -3"):
            a.set_mix_aux(mel)
        with pytest.raises(pkg.BPError, match="status -3"):
            a.set_mix_aux(None)
        a.dp_detach()
        a.train_mix(plan, order)
        b.train_mix(plan, order)
        assert _weights_equal(a, b)
    finally:
        a.close()
        b.close()


# ---- 6. the bpmix command-line tool
def _write_list(d, tag, xs):
    import wave
    for i, x in enumerate(xs):
        with wave.open(str(d / ("%s%d.wav" % (tag, i))), "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(8000)
            w.writeframes(np.asarray(x, np.int16).tobytes())
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


def test_bpmix_epoch_with_aux_matches_python_api(pkg, tmp_path, parity_record):
    import pfile_util as PU
    exe = str(pkg.LIB_PATH).replace("libbp_hip.so", "bpmix")
    B, cap, seed, per, lc, weight = 32, 150, 345, 2, 5.0, 0.25
    snrs = [0.0, 10.0]
    rng = np.random.default_rng(62)
    ints = lambda n, s: np.clip(np.round(rng.normal(0, s, n)), -32768, 32767).astype(np.float32)
    clean = [ints(n, 3000) for n in (900, 300, 1500, 90)]
    noise = [ints(n, 1500) for n in (3000, 500)]
    cv_clean = [ints(n, 3000) for n in (800, 400)]
    lists = dict(clean_list=_write_list(tmp_path, "clean", clean), noise_list=_write_list(tmp_path, "noise", noise),
                 cv_clean_list=_write_list(tmp_path, "cv", cv_clean))
    aux = ["aux_target=mfcc", "aux_mel=8", "aux_ceps=%d" % NC, "aux_first=1", "aux_lifter=0"]
    # aux_norm_out: the statistics of the clean sentences' coefficients
    r = subprocess.run([exe, "clean_list=" + lists["clean_list"], "fea_dim=%d" % D, "aux_norm_out=%s" % (tmp_path / "mfcc.norm")] + aux,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 1, r.stdout + r.stderr
    v = (tmp_path / "mfcc.norm").read_text().split("\n")
    m_cli, i_cli = np.array(v[1:1 + NC], np.float64), np.array(v[2 + NC:2 + 2 * NC], np.float64)
    g0 = _aux_geo()
    w, first, nb = MN.filters(g0)
    cc = []
    for x, P in zip(clean, pkg.wave_mfcc(0, D, clean, _aux(pkg), return_power=True)["power"]):
        cc.append(MN.cepstrum(MN.log_floor(MN.mel_energy(P, w, first, nb)).astype(np.float32), MN.dct(g0)))
    cc = np.concatenate(cc).astype(np.float64)
    e_norm = max(float(np.abs(m_cli - cc.mean(0)).max() / np.abs(cc.mean(0)).max()), float(np.abs(i_cli - 1.0 / cc.std(0)).max() / np.abs(1.0 / cc.std(0)).max()))
    assert e_norm <= 1e-6, e_norm
    # one epoch with the three-part target
    ls = [(CTX + 1) * D, 64, 2 * D + NC]
    W, b = pkg.glorot_net(ls, seed=9, beta=0.5)
    PU.write_wts(str(tmp_path / "init.wts"), ls, W, b)
    PU.write_norm(str(tmp_path / "mix.norm"), np.full(D, 9.0, np.float32), np.full(D, 0.25, np.float32))
    train = ["clean_list=" + lists["clean_list"], "noise_list=" + lists["noise_list"], "fea_dim=%d" % D, "snr_list=0,10", "mix_per_clean=%d" % per,
             "init_randem_seed=%d" % seed, "traincache=%d" % cap, "norm_file=%s" % (tmp_path / "mix.norm"), "cv_clean_list=" + lists["cv_clean_list"],
             "fea_context=%d" % CTX, "targ_offset=%d" % TOFF, "numlayers=3", "layersizes=%s" % ",".join(map(str, ls)), "bunchsize=%d" % B,
             "lrate=0.01", "momentum=0.5", "weightcost=0.0001", "dropoutflag=1", "visible_omit=0.1", "hid_omit=0.2", "target=lps+ibm", "lc_db=5",
             "output_act=sigmoid", "output_linear_dims=%d" % (D + NC), "initwts_file=%s" % (tmp_path / "init.wts"),
             "aux_norm_file=%s" % (tmp_path / "mfcc.norm"), "aux_weight=%g" % weight] + aux
    r = subprocess.run([exe] + train + ["outwts_file=%s" % (tmp_path / "out.wts"), "log_file=%s" % (tmp_path / "out.log")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "all finish!" in r.stdout, r.stdout + r.stderr
    log = (tmp_path / "out.log").read_text()
    assert "Auxiliary target: mfcc, 8 filters up to 4000 Hz, 5 coefficients from c1, lifter 0, weight 0.25: target columns [33, 38).\n" in log
    assert "Auxiliary target: the net's linear prefix is output_linear_dims=38 (LPS and MFCC columns), given 38.\n" in log
    cv_line = [ln for ln in log.splitlines() if ln.startswith("CV over. squared error: ")]
    assert len(cv_line) == 1, log
    # the same epoch through the Python API
    mean, istd = np.full(D, 9.0, np.float32), np.full(D, 0.25, np.float32)
    mel = _mel(pkg, g0, mean=m_cli.astype(np.float32), scale=(i_cli.astype(np.float32).astype(np.float64) * math.sqrt(weight)).astype(np.float32))
    plan = pkg.mix_plan(seed, len(clean), per, [x.size for x in noise], snrs)
    kw = dict(dropoutflag=1, visible_omit=0.1, hid_omit=0.2, max_chunk_frames=cap, output_activation=1, output_linear_cols=D + NC)
    g = pkg.BP_GPU(1, 3, ls, B, 0.01, 0.5, 1e-4, W, b, **kw)
    try:
        g.set_mix_aux(mel)
        g.set_mix_corpus(clean, noise, mean, istd, CTX, TOFF, "lps+ibm", lc)
        calls = _cut(g.mix_frames(plan), CTX, cap)
        assert len(calls) > 1
        for k, (a, e) in enumerate(calls):
            g.train_mix(plan[a:e], pkg.mix_shuffle(seed, k, int(g.mix_frames(plan[a:e]).sum())))
        Wp, bp = g.get_weights()
        PU.write_wts(str(tmp_path / "py.wts"), ls, Wp, bp)
        g.set_mix_corpus(cv_clean, noise, mean, istd, CTX, TOFF, "lps+ibm", lc)
        cv = pkg.mix_plan(20261016, len(cv_clean), 1, [x.size for x in noise], snrs)
        err, frames = np.float32(0.0), 0
        for a, e in _cut(g.mix_frames(cv), CTX, cap):
            err = np.float32(err + np.float32(g.CrossValid_mix(cv[a:e])))
            frames += int(g.mix_frames(cv[a:e]).sum())
    finally:
        g.close()
    assert (tmp_path / "py.wts").read_bytes() == (tmp_path / "out.wts").read_bytes()
    assert cv_line[0] == "CV over. squared error: %f" % (np.float32(err) / np.float32(frames))
    parity_record(aux_norm_relerr=e_norm, calls=len(calls))
