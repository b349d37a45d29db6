"""What tests/test_sequence_gpu.py, tests/test_size_gpu.py and tests/test_xsize_gpu.py share: one call of a model step on a handle
(execute), the chunk a call leaves resident (load), the comparison as words, the procedure of a walk (run_walk) and the one body of
the four GPU tests (walk_test).  Every comparison is between two runs of the same library and is bit for bit; there is no tolerance
in this file.

Per walk three long-lived handles take part, all made from the same weights and seed:
  S   the subject: the whole walk, no read beyond the walk's own (pass 1)
  R   the replay: the training kinds and the checkpoints of the walk alone; W, b, dW, db of S equal R's as uint32 at every
      checkpoint and at the end.  (A train_resident of S that trains on the chunk a QUERY left with targets -- mix_features, the
      gradient upload -- makes R load that chunk first.)
  S2  a second subject on the same walk (pass 2) that reads its weights before each query: a fresh handle F is made from them
      with the model's switches and the corpus, makes only that call, and every array it returns equals what S returned in pass 1;
      so does what S2 itself returns.  For the gradient query F is first brought to S's position of the dropout stream by bunches
      at lrate = momentum = weightcost = 0 (they leave the weights as they were, which is checked).  For grads_resident, the gradient
      of whatever is resident, F is also given the chunk of the call that made it resident on S (load).
Every expected error is a host-side check: its status and a non-empty message are checked on S and S2, and the checkpoints behind it
still equal R, which never made the call.
R repeats set_nat, makes train_resident(0, B) where S made profile_step(0, 1), and leaves out set_post and time_kernel like any
query; a chunk is loaded in the noise-aware mode it was made in.

A step is anything with the fields pos, kind, status, before, after of sequence_model.Step; the data of a call say how large it is
(the rows of x, the sentences, the blocks), so one `execute` serves every size."""
import re
import time

import numpy as np
import pytest

import mix_np as MX
import sequence_model as SM

SEED = 77


def plan(pkg, rows):
    p = np.zeros(len(rows), pkg.MIXTURE_DTYPE)
    for i, r in enumerate(rows):
        p[i] = r
    return p


def apply_post(pkg, g, cfg, setting):
    """set_post with setting number `setting` of sequence_model.post_settings (0: off)."""
    gv, gate = SM.post_settings(cfg)[setting]
    if not gv and gate is None:
        g.set_post()
        return
    center, scale = SM.gv_arrays(cfg) if gv else (None, None)
    lo, hi, weight = gate or (0.5, 0.5, 1.0)
    g.set_post(center, scale, mask_col=SM.mask_col(cfg) if gate else -1, mask_lo=lo, mask_hi=hi, mask_weight=weight, fea_dim=SM.FEA_DIM)


def make(pkg, cfg, W, b, st, cor, cap=SM.CAP):
    """A handle in model state st (preset, output setting, forward mode, noise-aware mode, post-processing) with the corpus (on
    configuration D: the MFCC columns set before it, the reverberated entries behind it)."""
    lr, m, wc, flag = SM.PRESETS[st["preset"]]
    oa, ol, lo = cfg.outs[st["out"]]
    g = pkg.BP_GPU(1, len(cfg.ls), cfg.ls, cfg.B, lr, m, wc, W, b, dropoutflag=flag, visible_omit=SM.VISIBLE_OMIT, hid_omit=SM.HID_OMIT,
                   activation=cfg.act, seed=SEED, max_chunk_frames=cap, compute_dtype=cfg.dtype, output_activation=oa,
                   output_linear_cols=ol, output_loss=lo, forward_mode=st["fwd"])
    if cor.get("aux"):
        a = dict(cor["aux"])
        g.set_mix_aux(pkg.mel_params(a.pop("sample_rate"), **a))
    g.set_mix_corpus(cor["clean"], cor["noise"], cor["mean"], cor["inv_std"], SM.CONTEXT, SM.TARG_OFFSET, cfg.corpus_target)
    if cor.get("rirs"):
        g.set_mix_reverb(cor["rirs"], cor["pair_clean"], cor["pair_rir"], cor["reverb_target"], cor["early_taps"])
    if st.get("nat"):
        g.set_nat(SM.NAT_MODES[st["nat"]])
    if st.get("post"):
        apply_post(pkg, g, cfg, st["post"])
    return g


def win(d):
    return (d["fea"], d["targ_frames"], SM.CONTEXT, d["win_start"], d["targ_frame"]), dict(nat=d["nat"], nat_row=d["nat_row"])


def state(g):
    (w, b), (dw, db) = g.get_weights(), g.get_deltas()
    return [a for l in range(1, g.numlayers) for a in (w[l], b[l], dw[l], db[l])]


def wave_target(pkg, cfg, masked):
    """(target, out_col): the LPS columns, or on the nets that have them the mask columns."""
    return (pkg.WAVE_MASK, SM.mask_col(cfg)) if masked and SM.mask_col(cfg) is not None else (pkg.WAVE_LPS, 0)


_EXTENDED = {3: False, 5: True, 7: "full"}                     # score columns -> the binding's extended=


def execute(pkg, g, cfg, cor, step, d):
    """Make the call of one model step on g; the arrays it returns."""
    k, B = step.kind, cfg.B
    if k == "train":
        g.train(d["x"].shape[0], d["x"], d["t"])
    elif k == "train_windows":
        a, kw = win(d)
        g.train_windows(*a, **kw)
    elif k == "upload_train":
        # the second bunch alone, then every whole bunch from the start (a chunk of fewer than two bunches: the second call only;
        # of less than one: its rows, which hold no bunch)
        n = d["x"].shape[0]
        g.upload_chunk(d["x"], d["t"])
        if n >= 2 * B:
            g.train_resident(B, B)
        g.train_resident(0, n // B * B if n >= B else n)
    elif k == "train_resident":
        g.train_resident(0, B)
    elif k == "train_mix":
        g.train_mix(plan(pkg, d["plan"]), d["order"])
    elif k == "preset":                                        # assigned like `TrainObj->lrate = ...`; the next call that runs the net pushes them
        g.lrate, g.momentum, g.weightcost, g.dropoutflag = SM.PRESETS[step.after["preset"]]
    elif k == "set_output":
        g.set_output(*cfg.outs[step.after["out"]])
    elif k == "set_forward":
        g.set_forward(step.before["fwd"] ^ 1)
    elif k == "set_nat":
        g.set_nat(SM.NAT_MODES[step.after["nat"]])
    elif k == "set_post":
        apply_post(pkg, g, cfg, step.after["post"])
    elif k == "time_kernel":                                   # (its one result is a time)
        g.time_kernel(d["which"], d["iters"])
    elif k == "profile_step":                                  # (likewise; what it trains shows at the checkpoints)
        g.profile_step(0, 1)
    elif k == "gv_mix":
        r = g.gv_mix(plan(pkg, d["plan"]), out_col=0, stage=d["stage"])
        return [r["est_sum"], r["est_sq"], r["ref_sum"], r["ref_sq"], np.int64(r["frames"])]
    elif k == "eval_mix_logmmse":
        r = g.eval_mix_logmmse(plan(pkg, d["plan"]), SM.SAMPLE_RATE, return_pcm=True, extended=_EXTENDED[d["width"]], noise=d["noise"])
        return [r["noisy"], r["enhanced"]] + list(r["pcm"])
    elif k == "forward":
        return [g.forward(d["x"])]
    elif k == "cv":
        return [np.float32(g.CrossValid(d["x"].shape[0], d["x"], d["t"]))]
    elif k == "cv_windows":
        a, kw = win(d)
        return [np.float32(g.CrossValid_windows(*a, **kw))]
    elif k == "cv_mix":
        return [np.float32(g.CrossValid_mix(plan(pkg, d["plan"])))]
    elif k == "mix_features":
        f = g.mix_features(plan(pkg, d["plan"]))
        return [f[n] for n in ("fea", "lps", "targ", "nat", "pcm")]
    elif k == "enhance":
        t, c = wave_target(pkg, cfg, False)
        waves, nets = g.enhance_waves(d["sentences"], cor["mean"], cor["inv_std"], SM.CONTEXT, SM.TARG_OFFSET, target=t, out_col=c,
                                      return_net=True)
        return list(waves) + list(nets)
    elif k == "eval_mix":
        t, c = wave_target(pkg, cfg, d.get("masked", True))
        r = g.eval_mix(plan(pkg, d["plan"]), SM.SAMPLE_RATE, target=t, out_col=c, return_pcm=True, extended=_EXTENDED[d.get("width", 3)])
        return [r["noisy"], r["enhanced"]] + list(r["pcm"])
    elif k == "grads":
        g.upload_chunk(d["x"], d["t"])
        g.grads_resident(d.get("first", 3))                    # an unaligned first frame; the bunch ends with the chunk
        gw, gb = g.read_grads()
        return gw[1:] + gb[1:]
    elif k == "grads_resident":
        g.grads_resident(0)
        gw, gb = g.read_grads()
        return gw[1:] + gb[1:]
    elif k == "stream":
        # blocks: one array per push (one channel), or one list of arrays per push (one per channel) with "ends", the end flags
        # of every push
        t, c = wave_target(pkg, cfg, False)
        n = len(d["blocks"])
        one = not isinstance(d["blocks"][0], (list, tuple))
        pushes = [[blk] for blk in d["blocks"]] if one else d["blocks"]
        ends = d.get("ends", [[i == n - 1] for i in range(n)])
        s = g.stream_open(cor["mean"], cor["inv_std"], SM.CONTEXT, SM.TARG_OFFSET, target=t, out_col=c, n_chan=len(pushes[0]),
                          max_push_samples=d.get("max_push", 256))
        try:
            outs = [s.push(blks, end=e) for blks, e in zip(pushes, ends)]
            return [o[0] for o in outs] if one else [a for o in outs for a in o]
        finally:
            s.close()
    elif k == "checkpoint":
        return state(g)
    else:
        raise AssertionError(k)
    return []


def load(pkg, g, kind, d, nat=None):
    """Make the chunk that a call of `kind` with data d leaves resident WITH targets, without its training or its reads.  nat: the
    noise-aware mode the chunk was made in, where it is not the one g is in now (the chunk keeps the rows it was made with)."""
    if nat is not None and SM.NAT_MODES[nat] != g.nat_mode:
        now = g.nat_mode
        g.set_nat(SM.NAT_MODES[nat])
        try:
            load(pkg, g, kind, d)
        finally:
            g.set_nat(now)
        return
    if kind == "mix_features":
        g.mix_features(plan(pkg, d["plan"]))
    elif kind in ("train", "upload_train", "grads"):
        g.upload_chunk(d["x"], d["t"])
    elif kind == "train_windows":
        a, kw = win(d)
        g.upload_chunk_windows(*a, **kw)
    elif kind == "train_mix":
        # the shuffled chunk that bp_train_mix makes on the device, fed from the host as tests/test_mix_gpu.py feeds it (the same bits:
        # test_training_equals_window_path)
        p = plan(pkg, d["plan"])
        f, frames = g.mix_features(p), g.mix_frames(p)
        rows = MX.staged_rows(f["fea"], frames, SM.CONTEXT, SM.TARG_OFFSET)
        tg = np.zeros((rows.shape[0], f["targ"].shape[1]), np.float32)
        tg[:f["targ"].shape[0]] = f["targ"]
        ws, tf, nr = MX.window_tables(frames, SM.CONTEXT, d["order"])
        if g.nat_mode == "dynamic":                            # one nat row per frame: nat_row is the global frame index
            nr = tf
        g.upload_chunk_windows(rows, tg, SM.CONTEXT, ws, tf, nat=f["nat"], nat_row=nr)
    else:
        raise AssertionError(kind)


def words(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.float64:                                  # (the double sums of gv_mix: by their bits)
        return a.view(np.uint64)
    return a.view(np.uint32) if a.dtype == np.float32 else a.astype(np.int64)


def differing(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    n = 0
    for u, v in zip(got, want):
        if u is None or v is None:
            assert u is None and v is None, what
            continue
        u, v = words(u).reshape(-1), words(v).reshape(-1)
        assert u.shape == v.shape, (what, u.shape, v.shape)
        n += int(np.count_nonzero(u != v))
    return n


def expect_error(pkg, g, cfg, cor, step, d, names=None):
    """The call raises with the model's status and a message (one that contains `names`, where given)."""
    with pytest.raises(pkg.BPError) as e:
        execute(pkg, g, cfg, cor, step, d)
    m = re.match(r"^(.*) \(status (-?\d+)\)$", str(e.value), re.S)
    assert m, str(e.value)
    assert int(m.group(2)) == step.status, (step.pos, step.kind, SM.STATUS_NAMES[step.status], str(e.value))
    assert m.group(1).strip(), "empty bp_last_error"
    if names:
        assert names in m.group(1), (step.pos, step.kind, names, m.group(1))


def advance(g, cfg, n_bunches, W, b, cap=SM.CAP):
    """Bring g's dropout stream to position n_bunches without moving its weights."""
    saved = (g.lrate, g.momentum, g.weightcost)
    g.lrate, g.momentum, g.weightcost = 0.0, 0.0, 0.0
    per = cap // cfg.B
    g.fill_chunk_synthetic(per * cfg.B)
    left = n_bunches
    while left > 0:
        k = min(per, left)
        g.train_resident(0, k * cfg.B)
        left -= k
    g.lrate, g.momentum, g.weightcost = saved
    w, bb = g.get_weights()
    assert differing(w[1:] + bb[1:], W[1:] + b[1:], "advance") == 0


def run_walk(pkg, cfg, steps, data, cor, cap=SM.CAP, error_names=None, idle=None):
    """The procedure above over steps and their data.  (count, diff, bad): what ran, the differing words per comparison, and
    (comparison, what, words) of everything that differs.
    error_names: step -> the text its expected error must contain (None: any message).
    idle: step -> True for a successful training call that the model says trains NOTHING.  The replay leaves such a call out, so a
    weight, a momentum word or a position of the dropout stream that it moved shows at the next checkpoint; and on the second pass
    W, b, dW, db are read on both sides of it and must be the same words."""
    by_pos = {s.pos: d for s, d in zip(steps, data)}
    W0, b0 = pkg.glorot_net(cfg.ls, seed=5 + cfg.index, beta=0.5)
    fresh = SM.fresh_state()
    S, R, S2 = (make(pkg, cfg, W0, b0, fresh, cor, cap) for _ in range(3))
    diff = {"state_vs_replay": 0, "query_vs_fresh": 0, "second_pass": 0, "idle_training": 0}
    bad = []

    def compare(key, got, want, what):
        n = differing(got, want, what)
        diff[key] += n
        if n:
            bad.append((key, what, n))
    names = error_names or (lambda s: None)
    is_idle = idle or (lambda s: False)
    count = {"calls": len(steps), "queries_compared": 0, "expected_errors": 0, "checkpoints": 0, "replay_loads": 0, "idle_trainings": 0}
    try:
        # ---- pass 1: the subject
        outs = {}
        for i, (s, d) in enumerate(zip(steps, data)):
            if s.status != SM.BP_OK:
                expect_error(pkg, S, cfg, cor, s, d, names(s))
                count["expected_errors"] += 1
            else:
                outs[i] = execute(pkg, S, cfg, cor, s, d)
        # ---- the replay: training kinds and checkpoints
        r_maker = None
        for i, (s, d) in enumerate(zip(steps, data)):
            if s.status != SM.BP_OK:
                continue
            if s.kind == "checkpoint":
                compare("state_vs_replay", outs[i], execute(pkg, R, cfg, cor, s, d), ("checkpoint", s.pos))
                count["checkpoints"] += 1
                continue
            if not SM.KINDS[s.kind].training or is_idle(s):
                continue
            as_kind = SM.REPLAY_AS.get(s.kind, s.kind)         # (profile_step: the plain loop in its place)
            if as_kind == "train_resident" and s.before["maker"] != r_maker:
                mk, mp = s.before["maker_kind"], s.before["maker"]
                assert mk in SM.LOADABLE, mk
                load(pkg, R, mk, by_pos[mp], s.before["maker_nat"])
                r_maker = mp
                count["replay_loads"] += 1
            execute(pkg, R, cfg, cor, s._replace(kind=as_kind), d)
            if s.after["maker"] == s.pos and s.after["maker_kind"] == s.kind:
                r_maker = s.pos
        end_S = state(S)
        compare("state_vs_replay", end_S, state(R), "end of the walk")
        assert all(np.isfinite(a).all() for a in end_S), "the walk left the net non-finite"
        # ---- pass 2: a fresh handle per query
        cache = None
        for i, (s, d) in enumerate(zip(steps, data)):
            if s.status != SM.BP_OK:
                expect_error(pkg, S2, cfg, cor, s, d, names(s))
                continue
            k = SM.KINDS[s.kind]
            if not k.training and s.kind not in SM.NO_FRESH:
                if cache is None:
                    cache = S2.get_weights()
                F = make(pkg, cfg, cache[0], cache[1], s.before, cor, cap)
                try:
                    if s.kind in ("grads", "grads_resident"):
                        advance(F, cfg, s.before["bunches"], cache[0], cache[1], cap)
                    if s.kind == "grads_resident":
                        mk, mp = s.before["maker_kind"], s.before["maker"]
                        load(pkg, F, mk, by_pos[mp], s.before["maker_nat"])
                    compare("query_vs_fresh", execute(pkg, F, cfg, cor, s, d), outs[i], (s.pos, s.kind, "after", steps[i - 1].kind if i else None))
                finally:
                    F.close()
                count["queries_compared"] += 1
            before = state(S2) if is_idle(s) else None
            o2 = execute(pkg, S2, cfg, cor, s, d)
            if before is not None:
                compare("idle_training", state(S2), before, (s.pos, s.kind, "trains nothing"))
                count["idle_trainings"] += 1
            if not k.training:
                compare("second_pass", o2, outs[i], (s.pos, s.kind))
            else:
                cache = None
        compare("second_pass", state(S2), end_S, "end of the second pass")
    finally:
        for g in (S, R, S2):
            g.close()
    return count, diff, bad


def walk_test(pkg, parity_record, fam, cid, wid):
    """The body of a GPU test: walk `wid` of family `fam` on configuration `cid`, modelled, made, run and recorded.  A call of
    CAP + 1 rows must name the capacity; the calls that train nothing and the refusals must be the model's.  Where calls have no
    size nothing can be idle, and the record of such a family holds neither counter."""
    t0 = time.perf_counter()
    cfg = SM.BY_ID[cid]
    walk, calls = SM.walk_calls(fam, cfg, wid)
    steps = SM.run_model(fam, cfg, calls)
    data = [SM.call_data(fam, cfg, walk, s.pos, s.kind, s.size) for s in steps]
    count, diff, bad = run_walk(pkg, cfg, steps, data, SM.corpus(fam, cfg), cap=fam.cap,
                                error_names=lambda s: "capacity" if s.size == "OVER" else None, idle=lambda s: SM.idle(fam, cfg, s))
    assert count["idle_trainings"] == sum(1 for s in steps if SM.idle(fam, cfg, s))
    assert count["expected_errors"] == sum(1 for s in steps if s.status != SM.BP_OK) >= sum(1 for s in steps if s.size == "OVER")
    if not fam.sizes:
        assert count.pop("idle_trainings") == 0 and diff.pop("idle_training") == 0
    record = dict(count, config=cid, walk=wid, words_differing=sum(diff.values()), **diff)
    if fam.timed:
        record["seconds"] = round(time.perf_counter() - t0, 2)
    parity_record(**record)
    print(cid, wid, record)
    assert not bad and sum(diff.values()) == 0, (cid, wid, diff, bad[:20])

