"""Which ordered pairs of calls on one handle have run against a fresh replay -- checked without a GPU.

tests/sequence_model.py holds a model of the handle, one table of call kinds and the walks; tests/test_sequence_gpu.py runs them.
Here: the closed walk of every configuration takes every ordered pair (kind, next kind) exactly once (remove a call and the check
names the pairs that went missing); every kind occurs as a success and, where the model has a precondition, as an expected error;
the model predicts the status codes that include/bp_c_api.h states, from quotations of the header; the GPU tests it names exist, carry
the gpu mark and no skip or xfail; configuration B reaches the split output layer; and the committed figures of a GPU run
(profiles/sequence_parity_numbers.json) hold zero differing words for every walk."""
import collections
import importlib
import json
import os
import re

import numpy as np
import pytest

import dispatch_np as D
import sequence_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LK = SM.table(SM.WALK.kinds)                                   # the 19 kinds of the family WALK: sequence_model.KINDS restricted to them
NUMBERS = os.path.join(ROOT, "profiles", "sequence_parity_numbers.json")
# (the comment text of the header on one line: the ` * ` that starts a comment line goes, a `*` inside a name stays)
HEADER = re.sub(r"\s+", " ", re.sub(r"\n \*(?=\s)", " ", open(os.path.join(ROOT, "include", "bp_c_api.h")).read()))


# ------------------------------------------------------------------ 1. the pairs
def missing_and_repeated(cfg, pieces):
    ks = SM.kinds_of(SM.WALK, cfg)
    seen = collections.Counter((a, b) for p in pieces for (_, a), (_, b) in zip(p, p[1:]))
    return sorted((a, b) for a in ks for b in ks if seen[(a, b)] == 0), sorted(k for k, n in seen.items() if n > 1)


@pytest.mark.parametrize("cfg", SM.WALK.configs, ids=[c.id for c in SM.WALK.configs])
def test_the_closed_walk_takes_every_ordered_pair_once(cfg):
    ks = SM.kinds_of(SM.WALK, cfg)
    assert len(ks) == (19 if len(cfg.outs) > 1 else 18) and len(set(ks)) == len(ks)
    pieces = SM.pieces(SM.WALK, cfg, "closed")
    assert sum(len(p) - 1 for p in pieces) == len(ks) ** 2
    assert missing_and_repeated(cfg, pieces) == ([], [])
    assert sorted(SM.pair_table(SM.WALK, cfg, "closed")) == sorted((a, b) for a in ks for b in ks)
    for i in range(len(pieces) - 1):                            # a piece starts with the call the one before it ended with
        assert pieces[i][-1] == pieces[i + 1][0]
    assert pieces[0][0][1] == pieces[-1][-1][1]                # closed
    # the ids the GPU test is parametrised with are the walks of the model
    for wid in SM.walk_ids(SM.WALK, cfg):
        walk, calls = SM.walk_calls(SM.WALK, cfg, wid)
        assert calls == (pieces[int(wid[6:] or 0)] if walk == 0 else SM.random_walk(SM.WALK, cfg, walk - 1))
        assert [p for p, _ in calls] == list(range(calls[0][0], calls[0][0] + len(calls)))


@pytest.mark.parametrize("cfg", SM.WALK.configs, ids=[c.id for c in SM.WALK.configs])
def test_a_removed_call_is_noticed_and_named(cfg):
    pieces = SM.pieces(SM.WALK, cfg, "closed")
    for at in (1, len(pieces[0]) // 2, len(pieces[0]) - 2):
        cut = [list(p) for p in pieces]
        gone = cut[0].pop(at)
        missing, _ = missing_and_repeated(cfg, cut)
        before, after = pieces[0][at - 1][1], pieces[0][at + 1][1]
        # (between two calls of its own kind only the loop goes missing: the neighbours close up to a pair that was there)
        assert missing and set(missing) <= {(before, gone[1]), (gone[1], after)}, (at, gone, missing)
        assert len(missing) == 2 or gone[1] in (before, after)


@pytest.mark.parametrize("n_pieces", [2, 3, 7])
def test_cut_into_pieces_the_walk_still_takes_every_pair_once(n_pieces):
    """N_PIECES is 1 today; the cutting is the issue's provision for a walk that outgrows ten seconds and has to keep working."""
    for cfg in SM.WALK.configs:
        ps = SM.pieces(SM.WALK, cfg, "closed", n_pieces)
        assert len(ps) == n_pieces and missing_and_repeated(cfg, ps) == ([], [])
        for i in range(n_pieces - 1):
            assert ps[i][-1] == ps[i + 1][0]
        table = SM.pair_table(SM.WALK, cfg, "closed", n_pieces)
        assert len(table) == len(SM.kinds_of(SM.WALK, cfg)) ** 2 and all(len(v) == 1 for v in table.values())
        assert set(v[0] for v in table.values()) == set("closed%d" % i for i in range(n_pieces))


def test_random_walks_are_seeded_and_differ():
    for cfg in SM.WALK.configs:
        walks = [SM.random_walk(SM.WALK, cfg, s) for s in range(SM.WALK.n_random)]
        assert all(len(w) == SM.RANDOM_LEN == 60 for w in walks) and SM.WALK.n_random == 4
        assert len(set(tuple(w) for w in walks)) == SM.WALK.n_random and walks[0] == SM.random_walk(SM.WALK, cfg, 0)


# ------------------------------------------------------------------ 2. successes and expected errors
def _steps(cfg):
    return [s for wid in SM.walk_ids(SM.WALK, cfg) if wid.startswith("closed") for s in SM.run_model(SM.WALK, cfg, SM.walk_calls(SM.WALK, cfg, wid)[1])]


def test_every_kind_succeeds_and_every_precondition_fails_somewhere():
    seen = collections.defaultdict(set)
    for cfg in SM.WALK.configs:
        per = collections.defaultdict(set)
        for s in _steps(cfg):
            per[s.kind].add(s.status)
            seen[s.kind].add(s.status)
            if s.status != SM.BP_OK:                            # a failed call leaves the model state as it was
                assert s.before == s.after and s.status in LK[s.kind].fail.values()
        # every configuration trains on a resident chunk and takes its gradient, and meets both refusals of each
        for kind in ("train_resident", "grads_resident"):
            assert per[kind] == {SM.BP_OK, SM.BP_ERR_ARG, SM.BP_ERR_STATE}, (cfg.id, kind, per[kind])
        assert per["set_forward"] == ({SM.BP_ERR_ARG} if cfg.dtype == 1 else {SM.BP_OK}), cfg.id
    for name, k in LK.items():
        assert SM.BP_OK in seen[name], name
        assert (k.pre is SM._pre_none) == (not k.fail), name
        assert seen[name] == {SM.BP_OK} | set(k.fail.values()), (name, seen[name])
        assert set(k.fail.values()) <= {SM.BP_ERR_ARG, SM.BP_ERR_STATE}
    assert [n for n, k in LK.items() if k.fail] == ["train_resident", "grads_resident", "set_forward"]


def test_the_replay_trains_on_chunks_that_queries_left():
    """train_resident behind mix_features and behind the gradient upload is legal: the replay loads those chunks (LOADABLE)."""
    for cfg in SM.WALK.configs:
        for kind in ("train_resident", "grads_resident"):
            makers = collections.Counter(s.before["maker_kind"] for s in _steps(cfg) if s.kind == kind and s.status == SM.BP_OK)
            assert set(SM.LOADABLE) <= set(makers), (cfg.id, kind, makers)
            assert all(LK[m].training or m in SM.LOADABLE for m in makers), makers
            # stacked and window chunks, made by training calls and by queries
            assert set(makers) == {"train", "train_windows", "upload_train", "train_mix", "mix_features", "grads"} or kind == "train_resident", (cfg.id, makers)
        refused = set(s.before["maker_kind"] for s in _steps(cfg) if s.kind == "grads_resident" and s.status == SM.BP_ERR_STATE)
        assert {"forward", "cv"} & refused and {"cv_windows", "cv_mix", "enhance", "eval_mix"} & refused, (cfg.id, refused)   # stacked and window
    assert sorted(SM.LOADABLE) == sorted(n for n, k in LK.items() if not k.training and _after(n)["has_targ"])


def _after(kind, cfg=SM.WALK.configs[0]):
    st = SM.fresh_state()
    LK[kind].apply(cfg, st, 0)
    return st


# ------------------------------------------------------------------ 3. the model against the header
# (kind, the model state it is called in, status, the sentence of include/bp_c_api.h that says so)
_LEGAL = "bp_mix_features (it makes the targets on the device) leave a chunk that can be trained on."
HEADER_STATUS = [
    ("train_resident", dict(rows=1000, has_targ=True), SM.BP_OK, _LEGAL),
    ("grads_resident", dict(rows=1000, has_targ=True), SM.BP_OK, _LEGAL),
    ("grads_resident", dict(rows=0, has_targ=True), SM.BP_ERR_ARG,
     "A frame range outside the resident chunk returns BP_ERR_ARG (checked first)."),
    ("grads_resident", dict(rows=1000, has_targ=False), SM.BP_ERR_STATE,
     "A chunk whose targets were not supplied by the call that made it resident returns BP_ERR_STATE from a training or gradient call"),
    ("grads_resident", dict(rows=8, has_targ=False), SM.BP_ERR_ARG,
     "A frame range outside the resident chunk returns BP_ERR_ARG (checked first)."),
    ("train_resident", dict(rows=0, has_targ=True), SM.BP_ERR_ARG,
     "A frame range outside the resident chunk returns BP_ERR_ARG (checked first)."),
    ("train_resident", dict(rows=1000, has_targ=False), SM.BP_ERR_STATE,
     "A chunk whose targets were not supplied by the call that made it resident returns BP_ERR_STATE from a training or gradient call"),
    ("train_resident", dict(rows=8, has_targ=False), SM.BP_ERR_ARG,
     "A frame range outside the resident chunk returns BP_ERR_ARG (checked first)."),
    ("set_forward", dict(), SM.BP_ERR_ARG, "ROWINV on a bf16 handle returns BP_ERR_ARG"),
]
# kind -> (window chunk?, targets?, the sentence that says what the call leaves resident)
HEADER_RESIDENT = {
    "forward": (False, False, "after bp_forward[_windows], bp_cv_chunk[_windows], bp_enhance_waves, bp_cv_mix, bp_eval_mix[_logmmse] and a stream's push there are no targets on the device"),
    "cv": (False, False, "bp_forward and bp_cv_chunk (stacked)"),
    "cv_windows": (True, False, "bp_forward_windows, bp_cv_chunk_windows, bp_enhance_waves, the mixing calls and a stream's push (window)"),
    "cv_mix": (True, False, "Each of the three calls leaves the chunk as the handle's resident window chunk."),
    "mix_features": (True, True, "bp_mix_features (it makes the targets on the device) leave a chunk that can be trained on"),
    "enhance": (True, False, "The call becomes the handle's resident window chunk (as after bp_forward_windows); training afterwards is unaffected."),
    "eval_mix": (True, False, "leaves the chunk as the resident window chunk; weights and momentum state are untouched."),
    "stream": (True, False, "A push leaves its rows as the handle's resident window chunk"),
    "grads": (False, True, "bp_upload_chunk[_windows], bp_fill_chunk_synthetic, bp_train_*, bp_train_mix and bp_mix_features"),
}


def test_the_status_codes_are_the_headers():
    for name, value in (("BP_OK", SM.BP_OK), ("BP_ERR_ARG", SM.BP_ERR_ARG), ("BP_ERR_STATE", SM.BP_ERR_STATE)):
        assert re.search(r"\b%s = %d\b" % (name, value), HEADER), name
        assert SM.STATUS_NAMES[value] == name
    bf16 = [c for c in SM.WALK.configs if c.dtype == 1][0]
    for kind, state, status, quote in HEADER_STATUS:
        assert quote in HEADER, quote
        assert status == SM.BP_OK or SM.STATUS_NAMES[status] in quote
        for cfg in SM.WALK.configs:
            if kind == "set_forward" and cfg is not bf16:
                assert LK[kind].pre(cfg, SM.fresh_state(), 0) is None
                continue
            why = LK[kind].pre(cfg, dict(SM.fresh_state(), **state), 0)
            assert (SM.BP_OK if why is None else LK[kind].fail[why]) == status, (kind, state, cfg.id)
    for name, k in LK.items():                            # every status the table can return is held to a sentence
        assert set(k.fail.values()) <= set(st for kind, _, st, _ in HEADER_STATUS if kind == name), name
    assert "The handle is unchanged after either error." in HEADER and "the handle is unchanged after an error" in HEADER


def test_what_a_query_leaves_resident_is_what_the_header_says():
    queries = [n for n, k in LK.items() if not k.training and n not in ("set_forward", "checkpoint", "grads_resident")]
    assert sorted(queries) == sorted(HEADER_RESIDENT)
    for kind, (windows, has_targ, quote) in HEADER_RESIDENT.items():
        assert quote in HEADER, quote
        for cfg in SM.WALK.configs:
            st = _after(kind, cfg)
            assert (st["windows"], st["has_targ"], st["maker_kind"]) == (windows, has_targ, kind), kind
            assert 0 < st["rows"] <= SM.CAP
    for cfg in SM.WALK.configs:                                      # the sizes: every training chunk has two bunches and a part
        for kind in ("train", "train_windows", "upload_train", "train_mix"):
            rows = _after(kind, cfg)["rows"]
            assert rows // cfg.B == 2 and rows % cfg.B, (cfg.id, kind, rows)
        assert SM.query_rows(cfg) == cfg.B + 3
        assert SM.mix_rows(SM.train_clean(cfg)) + len(SM.train_clean(cfg)) * (SM.CONTEXT - 1) <= SM.CAP
        assert SM.frames_of(SM.STREAM_LEN) < cfg.B <= SM.mix_rows(SM.QUERY_CLEAN)
    assert sum(SM.STREAM_BLOCKS) == SM.STREAM_LEN and len(SM.STREAM_BLOCKS) == 3
    # the stream's first two blocks leave no frame due (the noise-aware row needs six frames): only the last push adopts a chunk
    assert sum(SM.STREAM_BLOCKS[:2]) // SM.HOP < 6


def test_the_bunch_counter_is_the_number_of_full_bunches():
    for cfg in SM.WALK.configs:
        for s in _steps(cfg):
            d = s.after["bunches"] - s.before["bunches"]
            want = {"train": 2, "train_windows": 2, "upload_train": 3, "train_resident": 1, "train_mix": 2}.get(s.kind, 0)
            assert d == (want if s.status == SM.BP_OK else 0), (s.kind, d)


# ------------------------------------------------------------------ 4. the configurations and the GPU tests
def test_configuration_b_reaches_the_split_output_layer():
    def families(cfg):
        out = 1 if cfg.outs[0][0] else 0
        return set(D.family(k) for k in D.kernels(cfg.ls, cfg.B, cfg.dtype, out, "step"))
    a, b, c = (families(SM.BY_ID[i]) for i in "ABC")
    assert "bp_out_split_stage" in b and "bp_out_split_stage" not in a | c
    assert "bp_gemm_bf16" in c and "bp_gemm_bf16" not in a | b
    for cfg in SM.WALK.configs:
        assert cfg.ls[0] == (SM.CONTEXT + 1) * SM.FEA_DIM and cfg.ls[-1] in (SM.FEA_DIM, 2 * SM.FEA_DIM)


def test_every_named_gpu_test_exists_and_is_not_skipped():
    named = SM.gpu_tests(SM.WALK) + ["tests/test_sequence_gpu.py::test_calls_that_need_targets_refuse_a_stacked_chunk_without_them",
                            "tests/test_dp_life_gpu.py::test_detached_handle_holds_the_gathered_momentum_state",
                            "tests/test_dp_life_gpu.py::test_detach_gathers_without_a_collective_read_before_it",
                            "tests/test_dp_life_gpu.py::test_life_equals_one_attachment_and_one_rank"]
    assert len(SM.gpu_tests(SM.WALK)) == len(SM.WALK.configs) * (SM.n_pieces(SM.WALK)["closed"] + SM.WALK.n_random)
    for t in named:
        path, test = t.split("::")
        assert os.path.exists(os.path.join(ROOT, path)), t
        mod = importlib.import_module(path[len("tests/"):-len(".py")])
        fn = getattr(mod, test.split("[")[0], None)
        assert callable(fn), t
        marks = getattr(mod, "pytestmark", [])
        marks = (marks if isinstance(marks, list) else [marks]) + list(getattr(fn, "pytestmark", []))
        assert any(m.name == "gpu" for m in marks), t
        assert not any(m.name in ("skip", "skipif", "xfail") for m in marks), t
        if "[" in test:
            ids = [i for m in marks if m.name == "parametrize" for i in m.kwargs["ids"]]
            assert test[test.index("[") + 1:-1] in ids, t
    src = open(os.path.join(ROOT, "tests", "test_sequence_gpu.py")).read() + open(os.path.join(ROOT, "tests", "test_dp_life_gpu.py")).read()
    assert "pytest.skip" not in src and "xfail" not in src and "importorskip" not in src


# ------------------------------------------------------------------ 5. the figures of a GPU run
def test_committed_numbers_hold_zero_differing_words_for_every_walk():
    """profiles/sequence_parity_numbers.json: `python tests/sequence_model.py numbers sequence <parity JSON> <out>` behind a -m gpu run."""
    num = json.load(open(NUMBERS))["tests"]
    for cfg in SM.WALK.configs:
        for wid in SM.walk_ids(SM.WALK, cfg):
            e = num.get(SM.test_id(SM.WALK, cfg, wid))
            assert e is not None, "no measured figure for %s" % SM.test_id(SM.WALK, cfg, wid)
            steps = SM.run_model(SM.WALK, cfg, SM.walk_calls(SM.WALK, cfg, wid)[1])
            assert e["words_differing"] == 0 and e["state_vs_replay"] == 0 and e["query_vs_fresh"] == 0 and e["second_pass"] == 0
            assert e["calls"] == len(steps)
            assert e["expected_errors"] == sum(1 for s in steps if s.status != SM.BP_OK)
            assert e["checkpoints"] == sum(1 for s in steps if s.kind == "checkpoint")
            assert e["queries_compared"] == sum(1 for s in steps if s.status == SM.BP_OK and not LK[s.kind].training
                                                and s.kind not in ("checkpoint", "set_forward"))
            assert e["queries_compared"] > 0 and e["replay_loads"] >= 0
    life = num["tests/test_dp_life_gpu.py::test_detached_handle_holds_the_gathered_momentum_state"]
    assert set(life["d2_vs_d1_words_differing"].values()) == {0} and life["d1_nonzero_words"] > 0
    blind = num["tests/test_dp_life_gpu.py::test_detach_gathers_without_a_collective_read_before_it"]
    assert set(blind["detached_vs_collective_read_words_differing"].values()) == {0}
    end = num["tests/test_dp_life_gpu.py::test_life_equals_one_attachment_and_one_rank"]
    assert end["life_vs_one_attachment_words_differing"] == 0 and end["life_rank0_vs_rank1_words_differing"] == 0
    assert max(end["life_vs_one_rank_global_bunch"].values()) < end["strict_bar"] == 1e-5


# ------------------------------------------------------------------ 6. the whole table (the family EXTENDED)
XIDS = [c.id for c in SM.CONFIGS]
RAW_HEADER = open(os.path.join(ROOT, "include", "bp_c_api.h")).read()


def _x_missing_and_repeated(cfg, pieces):
    ks = SM.kinds_of(SM.EXTENDED, cfg)
    seen = collections.Counter((a, b) for p in pieces for (_, a), (_, b) in zip(p, p[1:]))
    return sorted((a, b) for a in ks for b in ks if seen[(a, b)] == 0), sorted(k for k, n in seen.items() if n > 1)


def _x_all_steps(cfg):
    """[(walk id, steps)] of every walk of EXTENDED, each from a fresh handle."""
    return [(wid, SM.run_model(SM.EXTENDED, cfg, calls)) for wid, _, calls in SM.all_walks(SM.EXTENDED, cfg)]


def _why(cfg, s):
    return SM.KINDS[s.kind].pre(cfg, s.before, s.pos)


def test_the_extended_table_is_a_superset_and_the_old_one_is_as_it_was():
    assert list(SM.KINDS)[:len(LK)] == list(LK) and len(LK) == 19
    assert SM.NEW_KINDS == ["set_nat", "set_post", "gv_mix", "eval_mix_logmmse", "time_kernel", "profile_step"]
    for name, k in LK.items():
        x = SM.KINDS[name]
        assert (x.training, x.apply) == (k.training, k.apply) and (x.fail == k.fail or name == "eval_mix")
    assert [n for n in SM.NEW_KINDS if SM.KINDS[n].training] == ["set_nat", "profile_step"]
    assert SM.CONFIGS[:3] == SM.WALK.configs and [c.id for c in SM.CONFIGS] == ["A", "B", "C", "D"]
    assert not set(SM.gpu_tests(SM.EXTENDED)) & set(SM.gpu_tests(SM.WALK)) and len(SM.gpu_tests(SM.EXTENDED)) == 4 * (SM.n_pieces(SM.EXTENDED)["xclosed"] + 1 + SM.EXTENDED.n_random)
    # on the old kinds and configurations a call of an extended walk is made of what call_data makes (eval_mix: plus its choices)
    for cfg in SM.WALK.configs:
        for kind in LK:
            a, b = SM.call_data(SM.EXTENDED, cfg, 10, 4, kind), SM.call_data(SM.WALK, cfg, 10, 4, kind)
            assert sorted(set(a) - set(b)) == (["masked", "width"] if kind == "eval_mix" else []), kind
            for key in b:
                assert repr(a[key]) == repr(b[key]) and np.asarray(a[key], dtype=object).shape == np.asarray(b[key], dtype=object).shape, (kind, key)


@pytest.mark.parametrize("cid", XIDS)
def test_the_extended_closed_walk_takes_every_ordered_pair_once(cid):
    cfg = SM.BY_ID[cid]
    ks = SM.kinds_of(SM.EXTENDED, cfg)
    assert len(ks) == (25 if len(cfg.outs) > 1 else 24) and len(set(ks)) == len(ks) and set(SM.kinds_of(SM.WALK, cfg)) < set(ks)
    pieces = SM.pieces(SM.EXTENDED, cfg, "xclosed")
    assert sum(len(p) - 1 for p in pieces) == len(ks) ** 2 and _x_missing_and_repeated(cfg, pieces) == ([], [])
    assert sorted(SM.pair_table(SM.EXTENDED, cfg, "xclosed")) == sorted((a, b) for a in ks for b in ks)
    for n_pieces in (1, 2, 3, 7):                               # cut, a piece starts with the call the one before it ended with
        ps = SM.pieces(SM.EXTENDED, cfg, "xclosed", n_pieces)
        assert len(ps) == n_pieces and _x_missing_and_repeated(cfg, ps) == ([], [])
        assert all(ps[i][-1] == ps[i + 1][0] for i in range(n_pieces - 1)) and ps[0][0][1] == ps[-1][-1][1]
        assert all(len(v) == 1 for v in SM.pair_table(SM.EXTENDED, cfg, "xclosed", n_pieces).values())
    ids = SM.walk_ids(SM.EXTENDED, cfg)
    assert ids == ["xclosed", "xmeasure"] + ["xrandom%d" % s for s in range(4)] and SM.n_pieces(SM.EXTENDED)["xclosed"] == 1
    walks = {}
    for wid in ids:
        walk, calls = SM.walk_calls(SM.EXTENDED, cfg, wid)
        walks[wid] = walk
        assert [p for p, _ in calls] == list(range(calls[0][0], calls[0][0] + len(calls))) and all(k in ks for _, k in calls)
    # the data of a walk follows its number: none of the legacy walks' (0 .. 4), no two the same
    assert len(set(walks.values())) == len(ids) and min(walks.values()) > SM.WALK.n_random
    rnd = [SM.random_walk(SM.EXTENDED, cfg, s) for s in range(SM.EXTENDED.n_random)]
    assert all(len(w) == SM.RANDOM_LEN for w in rnd) and len(set(map(tuple, rnd))) == SM.EXTENDED.n_random
    assert all(SM.random_walk(SM.EXTENDED, cfg, s) != SM.random_walk(SM.WALK, cfg, s) for s in range(SM.EXTENDED.n_random))
    for at in (1, len(pieces[0]) // 2, len(pieces[0]) - 2):     # a removed call is noticed and named
        cut = [list(p) for p in pieces]
        gone = cut[0].pop(at)
        missing, _ = _x_missing_and_repeated(cfg, cut)
        before, after = pieces[0][at - 1][1], pieces[0][at + 1][1]
        assert missing and set(missing) <= {(before, gone[1]), (gone[1], after)}, (at, gone, missing)
        assert len(missing) == 2 or gone[1] in (before, after)


@pytest.mark.parametrize("cid", XIDS)
def test_every_extended_kind_succeeds_and_every_precondition_fails_somewhere(cid):
    cfg = SM.BY_ID[cid]
    closed = [s for wid, ss in _x_all_steps(cfg) if wid.startswith("xclosed") for s in ss]
    status, reasons = collections.defaultdict(set), collections.defaultdict(set)
    for s in closed:
        status[s.kind].add(s.status)
        if s.status != SM.BP_OK:                                # a failed call leaves the model state as it was
            assert s.before == s.after and SM.KINDS[s.kind].fail[_why(cfg, s)] == s.status
            reasons[s.kind].add(_why(cfg, s))
    bf16, masked = cfg.dtype == 1, SM.mask_col(cfg) is not None
    for kind in SM.kinds_of(SM.EXTENDED, cfg):
        want = set(SM.KINDS[kind].fail)
        if kind in ("set_forward", "time_kernel", "profile_step") and bf16:
            want = {"bf16"}                                     # (checked first: nothing behind it is reached)
        elif kind in ("set_forward", "time_kernel", "profile_step"):
            want -= {"bf16"}
        if kind == "eval_mix" and not masked:
            want = set()
        assert reasons[kind] == want, (cid, kind, reasons[kind], want)
        assert (SM.BP_OK in status[kind]) == (not (bf16 and "bf16" in SM.KINDS[kind].fail)), (cid, kind)
    assert [n for n, k in SM.KINDS.items() if k.fail] == ["train_resident", "eval_mix", "grads_resident", "set_forward", "time_kernel", "profile_step"]
    # the bunch counter: profile_step(0, 1) is one bunch, the other new kinds none
    for s in closed:
        d = s.after["bunches"] - s.before["bunches"]
        want = {"train": 2, "train_windows": 2, "upload_train": 3, "train_resident": 1, "train_mix": 2, "profile_step": 1}.get(s.kind, 0)
        assert d == (want if s.status == SM.BP_OK else 0), (s.kind, d)


# (kind, configuration ids, model state, position or None for any, reason or None, the sentence of the header)
_TK = "Refusals of bp_time_kernel, in this order:"
_PS = "Refusals of bp_profile_step, in this order:"
X_HEADER_STATUS = [
    ("time_kernel", "C", dict(rows=1000), "bf16", "BP_ERR_STATE on a bf16 handle (the first of the state checks)"),
    ("time_kernel", "C", dict(rows=0), "bf16", "BP_ERR_STATE on a bf16 handle (the first of the state checks)"),
    ("time_kernel", "ABD", dict(rows=0), "no stacked chunk", "BP_ERR_STATE when no stacked chunk of at least bunchsize rows is resident"),
    ("time_kernel", "ABD", dict(rows=1000, windows=True), "no stacked chunk", "BP_ERR_STATE when no stacked chunk of at least bunchsize rows is resident"),
    ("time_kernel", "ABD", dict(rows=1000, has_targ=False), None, "It runs on the first bunchsize rows of a resident STACKED chunk, with or without targets"),
    ("profile_step", "C", dict(rows=0), "bf16", "BP_ERR_STATE on a bf16 or data-parallel handle (checked first)"),
    ("profile_step", "ABD", dict(rows=8, has_targ=False), "range", "then the two of bp_train_resident: a frame range outside the resident chunk (BP_ERR_ARG)"),
    ("profile_step", "ABD", dict(rows=1000, has_targ=False), "no targets", "a chunk without targets (BP_ERR_STATE)"),
    ("profile_step", "ABD", dict(rows=1000, has_targ=True), None, "Trains like bp_train_resident does: the same bits in the weights and the momentum state"),
]


def test_the_extended_model_is_the_headers():
    assert _TK in HEADER and _PS in HEADER
    for kind, cids, state, why, quote in X_HEADER_STATUS:
        assert quote in HEADER, quote
        for cid in cids:
            cfg = SM.BY_ID[cid]
            got = SM.KINDS[kind].pre(cfg, dict(SM.fresh_state(), **state), 0)
            assert got == why, (kind, cid, state, got)
            if why is not None:
                assert SM.STATUS_NAMES[SM.KINDS[kind].fail[why]] in quote
    for name in ("time_kernel", "profile_step"):                # every reason of the two is held to a sentence
        assert set(SM.KINDS[name].fail) == set(w for k, _, _, w, _ in X_HEADER_STATUS if k == name and w)
    # the order of the sentences in the header is the order of the checks in the model
    tk = HEADER[HEADER.index(_TK):]
    assert tk.index("on a bf16 handle") < tk.index("when no stacked chunk") < tk.index("The handle is unchanged after each.")
    # bp_time_kernel: what it leaves and what it may overwrite; no training, no query, left out of the replay
    assert ("bp_time_kernel leaves the weights, the momentum state, the resident chunk and the position of the dropout stream unchanged"
            in HEADER and "it may overwrite the activations and the back-propagated errors of the last bunch" in HEADER)
    tk_kind = SM.KINDS["time_kernel"]
    st = dict(SM.fresh_state(), rows=1000, has_targ=True)
    before = dict(st)
    tk_kind.apply(SM.BY_ID["D"], st, 0)
    assert st == before and not tk_kind.training and "time_kernel" in SM.NO_FRESH
    assert SM.time_ids(SM.BY_ID["D"]) == [0, 1, 2, 3, 4, 5] and all(SM.time_ids(SM.BY_ID[c]) == [3, 4, 5] for c in "ABC")
    assert "ids 0..2 on a net without a hidden -> hidden layer" in HEADER
    # bp_profile_step is one bunch of bp_train_resident: the replay makes that call in its place
    assert SM.REPLAY_AS == {"profile_step": "train_resident"} and SM.KINDS["profile_step"].apply is LK["train_resident"].apply
    # the switches: who reads them
    assert "bp_enhance_waves, bp_train_mix, bp_cv_mix, bp_mix_features, bp_eval_mix and bp_eval_mix_ext" in HEADER      # bp_set_nat
    assert SM.KINDS["set_nat"].training and set(SM.READS_NAT) == {"train_mix", "cv_mix", "mix_features", "enhance", "eval_mix", "gv_mix", "stream"}
    assert "The log-MMSE calls, training and CV are unaffected." in HEADER and not SM.KINDS["set_post"].training
    assert "on the corpus and the handle state of bp_eval_mix (fp32 and bf16 handles, both noise-aware modes" in HEADER      # bp_gv_mix reads nat
    # bp_eval_mix on the mask target under post-processing
    quote = "they return BP_ERR_ARG, with nothing touched, when the call's fea_dim differs from the one that was set, and when the target is BP_WAVE_MASK"
    assert quote in HEADER and SM.KINDS["eval_mix"].fail == {"mask target under post-processing": SM.BP_ERR_ARG}
    for cfg in SM.CONFIGS:
        pos_masked = [p for p in range(64) if SM.choice(cfg, p, "eval_mix")["masked"]][0]
        pos_lps = [p for p in range(64) if not SM.choice(cfg, p, "eval_mix")["masked"]][0]
        for post in range(len(SM.post_settings(cfg))):
            st = dict(SM.fresh_state(), post=post)
            refused = post > 0 and SM.mask_col(cfg) is not None
            assert (SM.KINDS["eval_mix"].pre(cfg, st, pos_masked) is not None) == refused
            assert SM.KINDS["eval_mix"].pre(cfg, st, pos_lps) is None
    # what the two new queries leave resident
    x_resident = {"gv_mix": "bp_gv_mix leaves the chunk as the resident window chunk, without targets, as bp_eval_mix does",
                  "eval_mix_logmmse": HEADER_RESIDENT["forward"][2]}
    assert "bp_eval_mix[_logmmse]" in x_resident["eval_mix_logmmse"]
    for kind, quote in x_resident.items():
        assert quote in HEADER, quote
        for cfg in SM.CONFIGS:
            st = SM.fresh_state()
            SM.KINDS[kind].apply(cfg, st, 0)
            assert (st["windows"], st["has_targ"], st["maker_kind"], st["rows"]) == (True, False, kind, SM.mix_rows(SM.QUERY_CLEAN))
    queries = [n for n in SM.NEW_KINDS if not SM.KINDS[n].training and n not in SM.NO_FRESH]
    assert queries == sorted(x_resident, reverse=True)


@pytest.mark.parametrize("cid", XIDS)
def test_every_switch_setting_is_read_by_every_kind_that_reads_it(cid):
    """From the model alone: each kind that reads the noise-aware mode succeeds under both modes, each kind that reads
    post-processing under every setting the configuration has, profile_step and time_kernel are each followed by every training
    kind (where they can succeed: by a call that succeeds behind one that did), every score width follows every other, and
    bp_time_kernel runs every kernel id the net allows."""
    cfg = SM.BY_ID[cid]
    nat, post, behind = collections.defaultdict(set), collections.defaultdict(set), collections.defaultdict(set)
    widths, which, stages, trackers, targets = set(), set(), set(), set(), set()
    for wid, steps in _x_all_steps(cfg):
        last = None
        for a, b in zip(steps, steps[1:]):
            if a.kind in ("profile_step", "time_kernel") and (cfg.dtype == 1 or a.status == b.status == SM.BP_OK):
                behind[a.kind].add(b.kind)
        for s in steps:
            if s.status != SM.BP_OK:
                continue
            c = SM.choice(cfg, s.pos, s.kind)
            if s.kind in SM.READS_NAT:
                nat[s.kind].add(s.before["nat"])
            if s.kind in SM.READS_POST and (s.kind != "gv_mix" or c["stage"] == "post"):
                post[s.kind].add(s.before["post"])
            if s.kind == "time_kernel":
                which.add(c["which"])
            if s.kind == "gv_mix":
                stages.add(c["stage"])
            if s.kind == "eval_mix":
                targets.add((c["masked"], s.before["post"] > 0))
            if s.kind == "eval_mix_logmmse":
                trackers.add(c["noise"])
            if "width" in c:
                if last is not None:
                    widths.add((last, c["width"]))
                last = c["width"]
    for k in SM.READS_NAT:
        assert nat[k] == {0, 1}, (cid, k, nat[k])
    for k in SM.READS_POST:
        assert post[k] == set(range(len(SM.post_settings(cfg)))), (cid, k, post[k])
    for k in ("profile_step", "time_kernel"):
        assert set(SM.TRAINING_KINDS) <= behind[k], (cid, k, set(SM.TRAINING_KINDS) - behind[k])
    assert SM.TRAINING_KINDS == ["train", "train_windows", "upload_train", "train_resident", "train_mix"]
    assert widths == set((a, b) for a in SM.WIDTHS for b in SM.WIDTHS) and SM.WIDTHS == (3, 5, 7)
    assert which == (set() if cfg.dtype == 1 else set(SM.time_ids(cfg))), (cid, which)
    assert stages == {"raw", "post"} and trackers == {None, "spp"}
    # an eval_mix that succeeds on post-processed rows, and on the nets with mask columns one on the mask target without them
    assert (False, True) in targets and (SM.mask_col(cfg) is None or (True, False) in targets)
    assert len(SM.post_settings(cfg)) == (2 if SM.mask_col(cfg) is None else 4) and SM.post_settings(cfg)[0] == (False, None)


def test_configuration_d_is_what_the_extended_table_needs():
    d = SM.BY_ID["D"]
    assert len(d.ls) == 4 and d.dtype == 0 and d.ls[0] == (SM.CONTEXT + 1) * SM.FEA_DIM and d.ls[-1] == 2 * SM.FEA_DIM + SM.N_CEPS
    assert SM.mask_col(d) == SM.FEA_DIM + SM.N_CEPS == d.outs[0][1] and d.outs[0][0] == 1      # logistic on the mask columns alone
    assert [SM.mask_col(SM.BY_ID[c]) for c in "ABC"] == [SM.FEA_DIM, None, SM.FEA_DIM]
    cor = SM.corpus(SM.EXTENDED, d)
    assert cor["aux"]["n_ceps"] == SM.N_CEPS and len(cor["rirs"]) == 2 and all(24 <= len(h) <= 48 for h in cor["rirs"])
    assert len(cor["pair_clean"]) == len(cor["pair_rir"]) == 2 and max(cor["pair_rir"]) < len(cor["rirs"])
    for c in SM.WALK.configs:                                        # the old configurations' corpus is the old corpus
        assert sorted(SM.corpus(SM.EXTENDED, c)) == sorted(SM.corpus(SM.WALK, c)) == ["clean", "inv_std", "mean", "noise"]
    # the derived entries are as long as the sentences the sizes were chosen with: two bunches and a part, 41 query frames
    n = len(SM.CLEAN_LEN)
    lens = SM.CLEAN_LEN + [SM.CLEAN_LEN[c] for c in cor["pair_clean"]]
    for plan_clean, legacy in ((SM.plan_train_clean(d), SM.train_clean(d)), (SM.plan_query_clean(d), SM.QUERY_CLEAN)):
        assert [lens[c] for c in plan_clean] == [SM.CLEAN_LEN[c] for c in legacy] and any(c >= n for c in plan_clean)
    for kind in ("train_mix", "cv_mix", "mix_features", "eval_mix", "gv_mix"):
        assert any(r[0] >= n for r in SM.call_data(SM.EXTENDED, d, 10, 7, kind)["plan"]), kind
    rows = SM.mix_rows(SM.train_clean(d))
    assert rows // d.B == 2 and rows % d.B and len(SM.call_data(SM.EXTENDED, d, 10, 7, "train_mix")["order"]) == rows
    t = SM.call_data(SM.EXTENDED, d, 10, 7, "train")["t"]                  # targets of the logistic columns in [0, 1], the others free
    assert t[:, SM.mask_col(d):].min() >= 0 and t[:, SM.mask_col(d):].max() <= 1 and t[:, :SM.mask_col(d)].min() < 0
    # call_data is a function of (configuration, walk, position): twice the same bytes
    for kind in SM.kinds_of(SM.EXTENDED, d):
        a, b = SM.call_data(SM.EXTENDED, d, 11, 9, kind), SM.call_data(SM.EXTENDED, d, 11, 9, kind)
        assert sorted(a) == sorted(b) and all(repr(a[k]) == repr(b[k]) for k in a), kind


# ------------------------------------------------------------------ 7. no entry point outside
def test_every_handle_function_of_the_header_is_classified():
    assert SM.api_problems(SM.API, SM.KINDS, RAW_HEADER) == []
    fns = re.findall(r"\b(bp_\w+)\s*\(\s*bp_handle\s*\*", re.sub(r"/\*.*?\*/", " ", RAW_HEADER, flags=re.S))
    assert len(fns) == len(set(fns)) == len(SM.API) >= 50 and "bp_create" not in fns and "bp_stream_push" not in fns
    for fn, v in SM.API.items():
        if isinstance(v, list):
            assert v and len(set(v)) == len(v), fn
            continue
        reason, path = v[0], v[1]
        word = v[2] if len(v) > 2 else fn[3:] + "("
        assert reason.strip() and "\n" not in reason, fn
        assert os.path.exists(os.path.join(ROOT, path)), (fn, path)
        assert word in open(os.path.join(ROOT, path)).read(), (fn, path, word)
    # the kinds an entry names are the kinds whose call makes it: the binding's method stands in walk_harness.execute / load / make
    harness = open(os.path.join(ROOT, "tests", "walk_harness.py")).read()
    for fn in ("bp_set_nat", "bp_set_post", "bp_gv_mix", "bp_eval_mix_logmmse", "bp_time_kernel", "bp_profile_step", "bp_set_mix_aux",
               "bp_set_mix_reverb"):
        assert "g.%s(" % fn[3:] in harness, fn
    # a new symbol without a row, a row without its symbol, and every new kind taken out of the table: each is named
    assert SM.api_problems(SM.API, SM.KINDS, RAW_HEADER + "\nint bp_new_call(bp_handle *h, int n);\n") == ["unclassified entry point bp_new_call"]
    less = collections.OrderedDict((k, v) for k, v in SM.API.items() if k != "bp_gv_mix")
    assert SM.api_problems(less, SM.KINDS, RAW_HEADER) == ["unclassified entry point bp_gv_mix", "no entry point names the kind gv_mix"]
    for gone in SM.NEW_KINDS:
        table = collections.OrderedDict((k, v) for k, v in SM.KINDS.items() if k != gone)
        problems = SM.api_problems(SM.API, table, RAW_HEADER)
        assert problems and all(p.endswith("names the kind %s, which the table does not have" % gone) for p in problems), (gone, problems)
    # ... and the old table alone leaves the six outside, by name
    old = SM.api_problems(SM.API, LK, RAW_HEADER)
    assert sorted(set(p.split("the kind ")[1].split(",")[0] for p in old)) == sorted(SM.NEW_KINDS)


# ------------------------------------------------------------------ 8. the extended GPU tests and their figures
def test_every_extended_gpu_test_exists_and_is_not_skipped():
    mod = importlib.import_module("test_sequence_gpu")
    fn = mod.test_extended_walk
    marks = [mod.pytestmark] + list(getattr(fn, "pytestmark", []))
    assert any(m.name == "gpu" for m in marks) and not any(m.name in ("skip", "skipif", "xfail") for m in marks)
    ids = [i for m in marks if m.name == "parametrize" for i in m.kwargs["ids"]]
    assert ["tests/test_sequence_gpu.py::test_extended_walk[%s]" % i for i in ids] == SM.gpu_tests(SM.EXTENDED)


def test_committed_numbers_hold_zero_differing_words_for_every_extended_walk_under_ten_seconds():
    num = json.load(open(NUMBERS))["tests"]
    for cfg in SM.CONFIGS:
        for wid in SM.walk_ids(SM.EXTENDED, cfg):
            e = num.get(SM.test_id(SM.EXTENDED, cfg, wid))
            assert e is not None, "no measured figure for %s" % SM.test_id(SM.EXTENDED, cfg, wid)
            steps = SM.run_model(SM.EXTENDED, cfg, SM.walk_calls(SM.EXTENDED, cfg, wid)[1])
            assert e["words_differing"] == 0 and e["state_vs_replay"] == 0 and e["query_vs_fresh"] == 0 and e["second_pass"] == 0
            assert e["calls"] == len(steps) and e["expected_errors"] == sum(1 for s in steps if s.status != SM.BP_OK)
            assert e["checkpoints"] == sum(1 for s in steps if s.kind == "checkpoint" and s.status == SM.BP_OK)
            assert e["queries_compared"] == sum(1 for s in steps if s.status == SM.BP_OK and not SM.KINDS[s.kind].training
                                                and s.kind not in SM.NO_FRESH)
            assert e["replay_loads"] >= 0 and (e["queries_compared"] > 0 or wid == "xmeasure")
            assert e["seconds"] < 10.0, (SM.test_id(SM.EXTENDED, cfg, wid), e["seconds"])
