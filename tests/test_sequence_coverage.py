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

import pytest

import dispatch_np as D
import sequence_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NUMBERS = os.path.join(ROOT, "profiles", "sequence_parity_numbers.json")
# (the comment text of the header on one line: the ` * ` that starts a comment line goes, a `*` inside a name stays)
HEADER = re.sub(r"\s+", " ", re.sub(r"\n \*(?=\s)", " ", open(os.path.join(ROOT, "include", "bp_c_api.h")).read()))


# ------------------------------------------------------------------ 1. the pairs
def missing_and_repeated(cfg, pieces):
    ks = SM.kinds_of(cfg)
    seen = collections.Counter((a, b) for p in pieces for (_, a), (_, b) in zip(p, p[1:]))
    return sorted((a, b) for a in ks for b in ks if seen[(a, b)] == 0), sorted(k for k, n in seen.items() if n > 1)


@pytest.mark.parametrize("cfg", SM.CONFIGS, ids=[c.id for c in SM.CONFIGS])
def test_the_closed_walk_takes_every_ordered_pair_once(cfg):
    ks = SM.kinds_of(cfg)
    assert len(ks) == (19 if len(cfg.outs) > 1 else 18) and len(set(ks)) == len(ks)
    pieces = SM.pieces(cfg)
    assert sum(len(p) - 1 for p in pieces) == len(ks) ** 2
    assert missing_and_repeated(cfg, pieces) == ([], [])
    assert sorted(SM.pair_table(cfg)) == sorted((a, b) for a in ks for b in ks)
    for i in range(len(pieces) - 1):                            # a piece starts with the call the one before it ended with
        assert pieces[i][-1] == pieces[i + 1][0]
    assert pieces[0][0][1] == pieces[-1][-1][1]                # closed
    # the ids the GPU test is parametrised with are the walks of the model
    for wid in SM.walk_ids(cfg):
        walk, calls = SM.walk_calls(cfg, wid)
        assert calls == (pieces[int(wid[6:] or 0)] if walk == 0 else SM.random_walk(cfg, walk - 1))
        assert [p for p, _ in calls] == list(range(calls[0][0], calls[0][0] + len(calls)))


@pytest.mark.parametrize("cfg", SM.CONFIGS, ids=[c.id for c in SM.CONFIGS])
def test_a_removed_call_is_noticed_and_named(cfg):
    pieces = SM.pieces(cfg)
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
    for cfg in SM.CONFIGS:
        ps = SM.pieces(cfg, n_pieces)
        assert len(ps) == n_pieces and missing_and_repeated(cfg, ps) == ([], [])
        for i in range(n_pieces - 1):
            assert ps[i][-1] == ps[i + 1][0]
        table = SM.pair_table(cfg, n_pieces)
        assert len(table) == len(SM.kinds_of(cfg)) ** 2 and all(len(v) == 1 for v in table.values())
        assert set(v[0] for v in table.values()) == set("closed%d" % i for i in range(n_pieces))


def test_random_walks_are_seeded_and_differ():
    for cfg in SM.CONFIGS:
        walks = [SM.random_walk(cfg, s) for s in range(SM.N_RANDOM)]
        assert all(len(w) == SM.RANDOM_LEN == 60 for w in walks) and SM.N_RANDOM == 4
        assert len(set(tuple(w) for w in walks)) == SM.N_RANDOM and walks[0] == SM.random_walk(cfg, 0)


# ------------------------------------------------------------------ 2. successes and expected errors
def _steps(cfg):
    return [s for wid in SM.walk_ids(cfg) if wid.startswith("closed") for s in SM.run_model(cfg, SM.walk_calls(cfg, wid)[1])]


def test_every_kind_succeeds_and_every_precondition_fails_somewhere():
    seen = collections.defaultdict(set)
    for cfg in SM.CONFIGS:
        per = collections.defaultdict(set)
        for s in _steps(cfg):
            per[s.kind].add(s.status)
            seen[s.kind].add(s.status)
            if s.status != SM.BP_OK:                            # a failed call leaves the model state as it was
                assert s.before == s.after and s.status in SM.KINDS[s.kind].fail.values()
        # every configuration trains on a resident chunk and takes its gradient, and meets both refusals of each
        for kind in ("train_resident", "grads_resident"):
            assert per[kind] == {SM.BP_OK, SM.BP_ERR_ARG, SM.BP_ERR_STATE}, (cfg.id, kind, per[kind])
        assert per["set_forward"] == ({SM.BP_ERR_ARG} if cfg.dtype == 1 else {SM.BP_OK}), cfg.id
    for name, k in SM.KINDS.items():
        assert SM.BP_OK in seen[name], name
        assert (k.pre is SM._pre_none) == (not k.fail), name
        assert seen[name] == {SM.BP_OK} | set(k.fail.values()), (name, seen[name])
        assert set(k.fail.values()) <= {SM.BP_ERR_ARG, SM.BP_ERR_STATE}
    assert [n for n, k in SM.KINDS.items() if k.fail] == ["train_resident", "grads_resident", "set_forward"]


def test_the_replay_trains_on_chunks_that_queries_left():
    """train_resident behind mix_features and behind the gradient upload is legal: the replay loads those chunks (LOADABLE)."""
    for cfg in SM.CONFIGS:
        for kind in ("train_resident", "grads_resident"):
            makers = collections.Counter(s.before["maker_kind"] for s in _steps(cfg) if s.kind == kind and s.status == SM.BP_OK)
            assert set(SM.LOADABLE) <= set(makers), (cfg.id, kind, makers)
            assert all(SM.KINDS[m].training or m in SM.LOADABLE for m in makers), makers
            # stacked and window chunks, made by training calls and by queries
            assert set(makers) == {"train", "train_windows", "upload_train", "train_mix", "mix_features", "grads"} or kind == "train_resident", (cfg.id, makers)
        refused = set(s.before["maker_kind"] for s in _steps(cfg) if s.kind == "grads_resident" and s.status == SM.BP_ERR_STATE)
        assert {"forward", "cv"} & refused and {"cv_windows", "cv_mix", "enhance", "eval_mix"} & refused, (cfg.id, refused)   # stacked and window
    assert sorted(SM.LOADABLE) == sorted(n for n, k in SM.KINDS.items() if not k.training and _after(n)["has_targ"])


def _after(kind, cfg=SM.CONFIGS[0]):
    st = SM.fresh_state()
    SM.KINDS[kind].apply(cfg, st, 0)
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
    bf16 = [c for c in SM.CONFIGS if c.dtype == 1][0]
    for kind, state, status, quote in HEADER_STATUS:
        assert quote in HEADER, quote
        assert status == SM.BP_OK or SM.STATUS_NAMES[status] in quote
        for cfg in SM.CONFIGS:
            if kind == "set_forward" and cfg is not bf16:
                assert SM.KINDS[kind].pre(cfg, SM.fresh_state()) is None
                continue
            why = SM.KINDS[kind].pre(cfg, dict(SM.fresh_state(), **state))
            assert (SM.BP_OK if why is None else SM.KINDS[kind].fail[why]) == status, (kind, state, cfg.id)
    for name, k in SM.KINDS.items():                            # every status the table can return is held to a sentence
        assert set(k.fail.values()) <= set(st for kind, _, st, _ in HEADER_STATUS if kind == name), name
    assert "The handle is unchanged after either error." in HEADER and "the handle is unchanged after an error" in HEADER


def test_what_a_query_leaves_resident_is_what_the_header_says():
    queries = [n for n, k in SM.KINDS.items() if not k.training and n not in ("set_forward", "checkpoint", "grads_resident")]
    assert sorted(queries) == sorted(HEADER_RESIDENT)
    for kind, (windows, has_targ, quote) in HEADER_RESIDENT.items():
        assert quote in HEADER, quote
        for cfg in SM.CONFIGS:
            st = _after(kind, cfg)
            assert (st["windows"], st["has_targ"], st["maker_kind"]) == (windows, has_targ, kind), kind
            assert 0 < st["rows"] <= SM.CAP
    for cfg in SM.CONFIGS:                                      # the sizes: every training chunk has two bunches and a part
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
    for cfg in SM.CONFIGS:
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
    for cfg in SM.CONFIGS:
        assert cfg.ls[0] == (SM.CONTEXT + 1) * SM.FEA_DIM and cfg.ls[-1] in (SM.FEA_DIM, 2 * SM.FEA_DIM)


def test_every_named_gpu_test_exists_and_is_not_skipped():
    named = SM.GPU_TESTS + ["tests/test_sequence_gpu.py::test_calls_that_need_targets_refuse_a_stacked_chunk_without_them",
                            "tests/test_dp_life_gpu.py::test_detached_handle_holds_the_gathered_momentum_state",
                            "tests/test_dp_life_gpu.py::test_detach_gathers_without_a_collective_read_before_it",
                            "tests/test_dp_life_gpu.py::test_life_equals_one_attachment_and_one_rank"]
    assert len(SM.GPU_TESTS) == len(SM.CONFIGS) * (SM.N_PIECES + SM.N_RANDOM)
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
    """profiles/sequence_parity_numbers.json: `python tests/sequence_model.py numbers <parity JSON> <out>` behind a -m gpu run."""
    num = json.load(open(NUMBERS))["tests"]
    for cfg in SM.CONFIGS:
        for wid in SM.walk_ids(cfg):
            e = num.get(SM.test_id(cfg, wid))
            assert e is not None, "no measured figure for %s" % SM.test_id(cfg, wid)
            steps = SM.run_model(cfg, SM.walk_calls(cfg, wid)[1])
            assert e["words_differing"] == 0 and e["state_vs_replay"] == 0 and e["query_vs_fresh"] == 0 and e["second_pass"] == 0
            assert e["calls"] == len(steps)
            assert e["expected_errors"] == sum(1 for s in steps if s.status != SM.BP_OK)
            assert e["checkpoints"] == sum(1 for s in steps if s.kind == "checkpoint")
            assert e["queries_compared"] == sum(1 for s in steps if s.status == SM.BP_OK and not SM.KINDS[s.kind].training
                                                and s.kind not in ("checkpoint", "set_forward"))
            assert e["queries_compared"] > 0 and e["replay_loads"] >= 0
    life = num["tests/test_dp_life_gpu.py::test_detached_handle_holds_the_gathered_momentum_state"]
    assert set(life["d2_vs_d1_words_differing"].values()) == {0} and life["d1_nonzero_words"] > 0
    blind = num["tests/test_dp_life_gpu.py::test_detach_gathers_without_a_collective_read_before_it"]
    assert set(blind["detached_vs_collective_read_words_differing"].values()) == {0}
    end = num["tests/test_dp_life_gpu.py::test_life_equals_one_attachment_and_one_rank"]
    assert end["life_vs_one_attachment_words_differing"] == 0 and end["life_rank0_vs_rank1_words_differing"] == 0
    assert max(end["life_vs_one_rank_global_bunch"].values()) < end["strict_bar"] == 1e-5
