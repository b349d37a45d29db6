"""What the walks of the family SIZE of tests/size_model.py reach -- checked without a GPU, from the allocation policy of csrc/bp_mem.h alone.

Here: sequence_model's walks still carry the data they carried before tests/walk_harness.py was split off (a digest); the families
are the ones BUFFERS gives; every ordered pair of (kind, size) nodes of every family is run by a named GPU test, and a removed call or
size opens cells by name; L regrows every buffer behind M; every buffer is regrown at least twice per configuration and followed by
a smaller call of every kind that sizes it; the training calls train 0, 1, 2 and an odd count >= 3 of bunches and start behind both
parities of staged bunches; BUFFERS names every Buf and every growing call site of the sources; the dye and its exemptions; the GPU
tests exist; the committed figures hold zero differing words."""
import collections
import glob
import hashlib
import importlib
import json
import os
import re

import numpy as np
import pytest

import sequence_model as SM
import size_model as ZM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dnn-for-speech-enhancement_amd", "csrc")
NUMBERS = os.path.join(ROOT, "profiles", "size_parity_numbers.json")
X_NUMBERS = os.path.join(ROOT, "profiles", "xsize_parity_numbers.json")
IDS = [c.id for c in ZM.SIZE.configs]
LB = ZM.view(ZM.SIZE)                                          # BUFFERS as the family SIZE sees it
SIZED = list(ZM.SIZE.sizes)
UNSIZED = [k for k in ZM.SIZE.kinds if k not in ZM.SIZE.sizes]
SENTENCES = tuple(k for k in ZM.SENTENCES if k in ZM.SIZE.kinds)
GPU_TESTS, X_GPU_TESTS = SM.gpu_tests(ZM.SIZE), SM.gpu_tests(ZM.XSIZE)


# ------------------------------------------------------------------ 0. the old walks, byte for byte
def _feed(h, v):
    if isinstance(v, dict):
        for k in sorted(v):
            h.update(k.encode())
            _feed(h, v[k])
    elif isinstance(v, (list, tuple)):
        h.update(b"[%d]" % len(v))
        for x in v:
            _feed(h, x)
    elif isinstance(v, np.ndarray):
        h.update(str(v.dtype).encode() + str(v.shape).encode() + np.ascontiguousarray(v).tobytes())
    else:
        h.update(repr(v).encode())


def test_the_sequence_walks_carry_the_ids_and_bytes_they_carried_before_the_harness_was_shared():
    """The digest was recorded on the parent commit, before test_sequence_gpu.py was moved onto walk_harness.py: ids, kinds, statuses,
    the corpus and every call's data of the fifteen walks."""
    h = hashlib.sha256()
    for cfg in ZM.SIZE.configs:
        _feed(h, SM.corpus(SM.WALK, cfg))
        for wid in SM.walk_ids(SM.WALK, cfg):
            walk, calls = SM.walk_calls(SM.WALK, cfg, wid)
            h.update(SM.test_id(SM.WALK, cfg, wid).encode())
            for s in SM.run_model(SM.WALK, cfg, calls):
                h.update(("%d %s %d" % (s.pos, s.kind, s.status)).encode())
                _feed(h, SM.call_data(SM.WALK, cfg, walk, s.pos, s.kind))
    assert h.hexdigest() == "36b0a2e5bf41a73c89549a03e1237f954490a40803895205f2e53bce8cfae709"
    assert SM.CAP == 256 and SM.n_pieces(SM.WALK)["closed"] == 1 and len(SM.gpu_tests(SM.WALK)) == 15
    src = open(os.path.join(ROOT, "tests", "test_sequence_gpu.py")).read()
    assert "def test_walk(pkg, parity_record, cid, wid)" in src and 'ids=["%s-%s" % p for p in PARAMS]' in src


# ------------------------------------------------------------------ 1. families and pairs
def test_the_families_are_the_ones_the_buffers_give():
    fam = ZM.families()
    assert list(fam) == list(ZM.FAMILY_IDS)
    assert set(fam["stacked pair"]) == set(ZM.STACKED)
    assert set(fam["wset.r[0]"]) == set(ZM.WINDOWS + SENTENCES) and len(fam["wset.r[0]"]) == 8
    assert set(fam["out_chunk"]) == {"forward", "cv", "cv_windows", "cv_mix", "enhance", "eval_mix", "stream"}
    # every buffer's kinds lie inside a family: all their pairs are walked (the mixing, evaluation and signal-layer buffers inside
    # the staging sets')
    for name, b in LB.items():
        assert any(set(b.ask) <= set(ks) for ks in fam.values()), name
    for name in ("in_d", "x", "lps", "ev_Y", "wave[0]"):
        assert set(LB[name].ask) < set(fam["wset.r[0]"])
    assert sorted(SIZED + UNSIZED) == sorted(ZM.SIZE.kinds) and set(k for ks in fam.values() for k in ks) == set(SIZED)
    assert UNSIZED == ["train_resident", "preset", "set_output", "grads_resident", "set_forward", "checkpoint"]


def _missing(cfg, fid, pieces):
    ns = SM.nodes(ZM.SIZE, cfg, fid)
    seen = collections.Counter((a[1:], b[1:]) for p in pieces for a, b in zip(p, p[1:]))
    return sorted((a, b) for a in ns for b in ns if seen[(a, b)] == 0), sorted(k for k, n in seen.items() if n > 1)


@pytest.mark.parametrize("cid", IDS)
def test_every_ordered_pair_of_sized_calls_of_a_family_is_run_by_a_named_gpu_test(cid):
    cfg = SM.BY_ID[cid]
    for fid in ZM.FAMILY_IDS.values():
        ns = SM.nodes(ZM.SIZE, cfg, fid)
        assert len(ns) == sum(len(ZM.GOOD) - (k in ZM.NO_Z) for k in ZM.family_of(fid))
        ps = SM.pieces(ZM.SIZE, cfg, fid)
        assert _missing(cfg, fid, ps) == ([], [])
        for i in range(len(ps) - 1):
            assert ps[i][-1] == ps[i + 1][0]
        assert ps[0][0][1:] == ps[-1][-1][1:]
        table = SM.pair_table(ZM.SIZE, cfg, fid)
        assert sorted(table) == sorted((a, b) for a in ns for b in ns)
        assert all(len(v) == 1 and SM.test_id(ZM.SIZE, cfg, v[0]) in GPU_TESTS for v in table.values())
        for at in (1, len(ps[0]) // 2):                          # a removed call opens cells, by name
            cut = [list(p) for p in ps]
            gone = cut[0].pop(at)
            missing, _ = _missing(cfg, fid, cut)
            assert missing and set(missing) <= {(ps[0][at - 1][1:], gone[1:]), (gone[1:], ps[0][at + 1][1:])}
        # ... and so does a removed size
        k0 = ZM.family_of(fid)[0]
        cut = [[c for c in p if c[1:] != (k0, "L")] for p in ps]
        missing, _ = _missing(cfg, fid, cut)
        assert len(set(m for m in missing if (k0, "L") in m)) == 2 * len(ns) - 1
    for wid in SM.walk_ids(ZM.SIZE, cfg):
        walk, calls = SM.walk_calls(ZM.SIZE, cfg, wid)
        assert [c[0] for c in calls] == list(range(calls[0][0], calls[0][0] + len(calls)))
        assert all(k in SM.kinds_of(ZM.SIZE, cfg) and z in ZM.sizes_of(k) for _, k, z in calls)
    assert len(set(w for c in ZM.SIZE.configs for w, _ in [SM.walk_calls(ZM.SIZE, c, x) for x in SM.walk_ids(ZM.SIZE, c)])) == len(SM.n_pieces(ZM.SIZE)) + 1 + ZM.SIZE.n_random


@pytest.mark.parametrize("cid", IDS)
def test_over_follows_every_other_size_of_its_kind_and_fails_with_the_state_unchanged(cid):
    cfg = SM.BY_ID[cid]
    steps = SM.run_model(ZM.SIZE, cfg, ZM.over_walk(cfg))
    behind = set((a.kind, a.size) for a, b in zip(steps, steps[1:]) if b.size == "OVER" and b.kind == a.kind)
    assert behind == set((k, z) for k in SIZED for z in ZM.sizes_of(k) if z != "OVER")
    in_random = [s for r in range(ZM.SIZE.n_random) for s in SM.run_model(ZM.SIZE, cfg, SM.random_walk(ZM.SIZE, cfg, r)) if s.size == "OVER"]
    assert len(in_random) >= 4
    for s in steps + in_random:
        if s.size == "OVER":
            assert s.status == SM.BP_ERR_ARG and s.before == s.after
            assert ZM.shape(cfg, s.kind, "OVER").rows == ZM.CAP + 1 and ZM.shape(cfg, s.kind, "FULL").rows == ZM.CAP
    walks = [SM.random_walk(ZM.SIZE, cfg, r) for r in range(ZM.SIZE.n_random)]
    assert ZM.SIZE.n_random == 4 and all(len(w) == SM.RANDOM_LEN for w in walks) and len(set(map(tuple, walks))) == 4
    seen = set(k for w in walks for _, k, _ in w)
    assert set(UNSIZED) & seen >= {"train_resident", "grads_resident", "checkpoint", "preset"}


# ------------------------------------------------------------------ 2. the sizes
@pytest.mark.parametrize("cid", IDS)
def test_the_size_classes_are_what_the_model_says(cid):
    cfg, B = SM.BY_ID[cid], SM.BY_ID[cid].B
    for k in SIZED:
        sh = {z: ZM.shape(cfg, k, z) for z in ZM.sizes_of(k)}
        assert ("Z" in sh) == (k not in ZM.NO_Z)
        if "Z" in sh:
            assert sh["Z"].n < B and sh["Z"].bunches == 0 and (sh["Z"].n == 1 or sh["Z"].T == [2] and ZM.len_of(2) == 1)
        assert sh["ONE"].n == B and sh["FULL"].rows == ZM.CAP and sh["OVER"].rows == ZM.CAP + 1 and not sh["OVER"].ok
        if k != "stream":
            nb = ZM.large(cfg, k)
            assert nb >= 3 and nb % 2 == 1 and sh["L"].n == nb * B + B // 2 and sh["L"].rows < ZM.CAP
        if k in SENTENCES and k != "stream":                # more sentences AND one long sentence
            assert len(sh["L"].T) == ZM.N_SHORT + 1 > len(sh["M"].T) and max(sh["L"].T) > max(sh["M"].T)
        if SM.KINDS[k].training:
            extra = 1 if k == "upload_train" else 0
            assert [sh[z].bunches for z in ZM.GOOD] == [0, 1, 2 + extra, sh["L"].n // B + extra, sh["FULL"].n // B + extra]
    # M is sequence_model's size
    assert ZM.shape(cfg, "train", "M").n == SM.train_rows(cfg) and ZM.shape(cfg, "forward", "M").n == SM.query_rows(cfg)
    assert ZM.shape(cfg, "train_mix", "M").n == SM.mix_rows(SM.train_clean(cfg)) and ZM.shape(cfg, "cv_mix", "M").n == SM.mix_rows(SM.QUERY_CLEAN)
    assert ZM.shape(cfg, "stream", "M").pushes[2] == [[b] for b in SM.STREAM_BLOCKS] and ZM.shape(cfg, "stream", "M").resident == SM.frames_of(SM.STREAM_LEN)
    z, l = ZM.shape(cfg, "stream", "Z"), ZM.shape(cfg, "stream", "L")
    assert z.n_sent == 1 and z.pushes[2] == [[1]]
    assert l.n_sent == 4 and all(0.97 * l.pushes[1] <= sum(b) <= l.pushes[1] for b in l.pushes[2]) and l.rows <= ZM.CAP
    # the corpus: sequence_model's recordings first (the same lengths), every entry within one chunk
    cor = SM.corpus(ZM.SIZE, cfg)
    assert [len(x) for x in cor["clean"][:4]] == SM.CLEAN_LEN and [len(x) for x in cor["noise"]] == SM.NOISE_LEN
    assert all(SM.frames_of(len(x)) <= ZM.CAP for x in cor["clean"])
    for (T, dyed), i in cor["index"].items():
        assert SM.frames_of(len(cor["clean"][i])) == T and bool(np.isnan(cor["clean"][i]).all()) == dyed and bool(np.isfinite(cor["clean"][i]).all()) != dyed


@pytest.mark.parametrize("cid", IDS)
def test_l_regrows_every_buffer_behind_m(cid):
    """The claim of the size class L, from the policy: behind an M call of the kind (on a fresh handle or a regrown one the block then
    holds grown(M's request)), the L call asks for more."""
    cfg = SM.BY_ID[cid]
    checked = 0
    for name, b in LB.items():
        assert (name in ZM.NEVER) == ZM.never_regrows(cfg, name, LB), name
        for k in b.ask:
            m, l = ZM.asks(cfg, name, ZM.shape(cfg, k, "M")), ZM.asks(cfg, name, ZM.shape(cfg, k, "L"))
            if name in ZM.NEVER or m == 0:
                continue
            if (k, name) in ZM.L_EXEMPT:
                assert l <= ZM.POLICY[b.policy](m), "no longer exempt: %s %s" % (k, name)
                continue
            assert l > ZM.POLICY[b.policy](m), (cid, k, name, m, l)
            checked += 1
            if ZM.large(cfg, k) > 3 and k != "stream":           # and no smaller odd bunch count would do for the kind
                assert any(ZM.asks(cfg, n2, ZM.shape(cfg, k, "L", ZM.large(cfg, k) - 2)) <= ZM.POLICY[b2.policy](ZM.asks(cfg, n2, ZM.shape(cfg, k, "M")))
                           for n2, b2 in LB.items() if k in b2.ask and n2 not in ZM.NEVER and ZM.asks(cfg, n2, ZM.shape(cfg, k, "M")) > 0) \
                    or ZM.shape(cfg, k, "L", ZM.large(cfg, k) - 2).T[0] < 2
    assert checked >= 40
    assert ZM.NEVER == ("stacked pair", "stage tiles", "in_d", "gain", "in_pin") and list(ZM.L_EXEMPT) == [("stream", "wset.r[2]")]
    assert ZM.grown(1000) == 1000 + 250 + 4096 and ZM.grown_frames(100) == 189
    mem = open(os.path.join(CSRC, "bp_mem.h")).read()
    assert "if (n <= bytes) return BP_OK;" in mem and "alloc(n + n / 4 + 4096, pin)" in mem
    step = open(os.path.join(CSRC, "bp_step.hip")).read()
    assert "if ((size_t)n_frames <= h->out_chunk_frames) return BP_OK;" in step and "(size_t)n_frames + (size_t)n_frames / 4 + 64" in step


@pytest.mark.parametrize("cid", IDS)
def test_every_buffer_is_regrown_twice_and_followed_by_a_smaller_call_of_every_kind_that_sizes_it(cid):
    cfg = SM.BY_ID[cid]
    regrows, smaller = collections.Counter(), collections.defaultdict(set)
    for wid, _, calls in SM.all_walks(ZM.SIZE, cfg):
        sim = ZM.simulate(ZM.SIZE, cfg, calls)
        regrows.update(sim.regrows)
        for n, ks in sim.smaller.items():
            smaller[n] |= set(k for k, _ in ks)
    for name, b in LB.items():
        if name in ZM.NEVER:
            assert regrows[name] == 0
            continue
        assert regrows[name] >= 2, (cid, name, regrows[name])
        assert smaller[name] == set(b.ask), (cid, name, set(b.ask) - smaller[name])
    # the fixed blocks never regrow, but shrink they do: behind a FULL call of a kind comes a smaller call of every kind of the family
    for fid in ("stacked",):
        ks = ZM.family_of(fid)
        pairs = set((a[1:], b[1:]) for p in SM.pieces(ZM.SIZE, cfg, fid) for a, b in zip(p, p[1:]))
        assert all(((k, "FULL"), (k2, z)) in pairs for k in ks for k2 in ks for z in ZM.sizes_of(k2) if z not in ("FULL", "OVER"))


@pytest.mark.parametrize("cid", IDS)
def test_training_calls_train_0_1_2_and_an_odd_count_of_bunches_behind_both_tile_parities(cid):
    """Which paths stage (size_model.STAGING): window chunks always, stacked chunks when visible dropout is on.  The tile a training
    call starts in follows the bunches staged on those paths before it, modelled as their count modulo 2."""
    cfg = SM.BY_ID[cid]
    assert ZM.STAGING == "window chunks always, stacked chunks when visible dropout is on"
    step = open(os.path.join(CSRC, "bp_step.hip")).read()
    assert "return h->th_vis ? ensure_stage_tiles(h) : BP_OK;" in step and "if (h->res.windows) HIPCHK(stage_bunch(h, first, fb, false));" in step
    counts, parity = collections.defaultdict(set), collections.defaultdict(set)
    for wid, _, calls in SM.all_walks(ZM.SIZE, cfg):
        staged = 0
        for s in SM.run_model(ZM.SIZE, cfg, calls):
            d = s.after["bunches"] - s.before["bunches"]
            stages = s.after["windows"] or SM.PRESETS[s.before["preset"]][3] == 1
            if SM.KINDS[s.kind].training and s.kind in SIZED and s.status == SM.BP_OK:
                counts[s.kind].add(d)
                parity[s.kind].add(staged % 2)
            if d and stages:
                staged += d
    for k in ("train", "train_windows", "upload_train", "train_mix"):
        c = counts[k] if k != "upload_train" else set(x - (1 if x >= 3 else 0) for x in counts[k])
        assert {0, 1, 2} <= c and any(x >= 3 and x % 2 for x in c), (cid, k, sorted(counts[k]))
        assert parity[k] == {0, 1}, (cid, k)
        assert max(c) == ZM.shape(cfg, k, "FULL").n // cfg.B             # the chunk filled to capacity
    assert SM.idle(ZM.SIZE, cfg, SM.run_model(ZM.SIZE, cfg, [(0, "train", "Z")])[0]) and not SM.idle(ZM.SIZE, cfg, SM.run_model(ZM.SIZE, cfg, [(0, "train", "ONE")])[0])
    assert not SM.idle(ZM.SIZE, cfg, SM.run_model(ZM.SIZE, cfg, [(0, "forward", "Z")])[0])


# ------------------------------------------------------------------ 3. BUFFERS against the sources (a text scan)
def _sources():
    return sorted(glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "*.hip")))


def test_buffers_names_every_buf_and_every_growing_call_site_of_the_sources():
    members, grown_args, sites = set(), set(), collections.Counter()
    for path in _sources():
        text = open(path).read()
        for m in re.finditer(r"\bBuf\s+([^;()=]+);", text):
            for name in m.group(1).split(","):
                name = name.strip()
                if name and name[0] not in "&*":
                    members.add(re.sub(r"\[.*", "", name))
        members.update(re.findall(r"vector<Buf>\s+(\w+)", text))
        for m in re.finditer(r"(?<![\w])(wave_grow|wset_reserve|out_chunk_reserve)\(([^;]*);", text):
            line = text[text.rfind("\n", 0, m.start()) + 1:m.start()]
            if re.search(r"\b(int|inline)\s*$", line):          # the definition or the declaration
                continue
            sites[(os.path.basename(path), m.group(1))] += 1
            if m.group(1) == "wave_grow":
                grown_args.update(re.sub(r"\[.*", "", a) for a in re.findall(r"\{\s*(?:ms|h)->([\w\[\]]+)\s*,", m.group(2)))
    known = set(b.member for b in LB.values()) | set(ZM.unmodelled(ZM.SIZE)) | set(ZM.OTHER_BUFS)
    assert members - known == set(), "a Buf without a row in size_model: %s" % sorted(members - known)
    assert known - members == set(), "size_model names a Buf the sources no longer hold: %s" % sorted(known - members)
    table = set(b.member for b in LB.values() if b.site.startswith("wave_grow")) | set(ZM.unmodelled(ZM.SIZE))
    assert grown_args == table, (sorted(grown_args - table), sorted(table - grown_args))
    assert dict(sites) == ZM.SITES, dict(sites)
    assert set(b.site.split(":")[0] for b in LB.values()) == {"dev_alloc", "wset_reserve", "out_chunk_reserve", "wave_grow"}
    # wset_reserve takes the four blocks of a set, in the order of the rows
    step = open(os.path.join(CSRC, "bp_step.hip")).read()
    assert "{{rw[0], rows_b, false}, {rw[1], targ_b, false}, {rw[2], nat_b, false}, {rw[3], tab_b, false}}" in step
    assert [n for n in LB if n.startswith("wset.r[")] == ["wset.r[%d]" % i for i in range(4)]
    # the whole table (size_model.BUFFERS, which the family XSIZE reads) over the same sources: ev_gain has a row, every nat_b expression is restated by the
    # wset.r[2] row (static and dynamic, with and without a kept spectrum, a stream's), every window_reserve site is counted; a new
    # expression or a new site fails by name (tests/test_xsize_coverage.py applies the mutants)
    found = ZM.scan({os.path.basename(p): open(p).read() for p in _sources()})
    assert found["members"] == members and found["grown_args"] == grown_args and found["sites"] == dict(sites)
    assert ZM.scan_problems(found) == []
    assert sorted(found["nat_b"]) == ["bp_mix.hip", "bp_step.hip", "bp_stream.hip", "bp_wave.hip"] == sorted(ZM.NAT_EXPR)
    assert found["reserve"] == {"bp_mix.hip": 1, "bp_stream.hip": 1, "bp_wave.hip": 1} == ZM.WINDOW_RESERVE_SITES
    assert "ev_gain" in ZM.BUFFERS and "ev_gain" not in ZM.UNMODELLED and set(ZM.UNMODELLED) < set(ZM.unmodelled(ZM.SIZE))


# ------------------------------------------------------------------ 4. the dye
def test_queries_at_l_and_full_are_dyed_and_training_stays_finite():
    assert ZM.FINITE_DYE == () and ZM.DYED == ("L", "FULL")
    for cfg in ZM.SIZE.configs:
        cor = SM.corpus(ZM.SIZE, cfg)
        for k in SIZED:
            for z in ZM.sizes_of(k):
                if z == "OVER" and k in ("train_mix",):
                    continue
                d = SM.call_data(ZM.SIZE, cfg, 0, 5, k, z)
                arrays = []
                for key in ("x", "fea", "nat"):
                    if key in d:
                        arrays.append(d[key])
                arrays += list(d.get("sentences", [])) + [a for blk in d.get("blocks", []) for a in blk]
                arrays += [cor["clean"][r[0]] for r in d.get("plan", [])]
                has_nan = any(np.isnan(a).any() for a in arrays)
                assert has_nan == ZM.dyed(k, z) == (z in ZM.DYED and not SM.KINDS[k].training), (cfg.id, k, z)
                if has_nan and k not in SM.LOADABLE:
                    assert all(np.isnan(a).all() for a in arrays), (cfg.id, k, z)
                if "t" in d:
                    assert np.isfinite(d["t"]).all()
        # the chunks that can be trained on keep the rows a train_resident(0, B) or the gradient reads finite
        for z in ZM.DYED:
            d = SM.call_data(ZM.SIZE, cfg, 0, 5, "grads", z)
            assert np.isfinite(d["x"][:cfg.B + 3]).all() and np.isnan(d["x"][cfg.B + 3:]).all() and d["first"] == 3
            p = SM.call_data(ZM.SIZE, cfg, 0, 5, "mix_features", z)["plan"]
            first = cor["clean"][p[0][0]]
            assert np.isfinite(first).all() and SM.frames_of(len(first)) >= cfg.B and all(np.isnan(cor["clean"][r[0]]).all() for r in p[1:])
    assert sorted(SM.LOADABLE) == ["grads", "mix_features"]


# ------------------------------------------------------------------ 5. the GPU tests and the figures of a run
def test_every_named_gpu_test_exists_and_is_not_skipped():
    mod = importlib.import_module("test_size_gpu")
    fn = mod.test_size_walk
    marks = [mod.pytestmark] + list(getattr(fn, "pytestmark", []))
    assert any(m.name == "gpu" for m in marks) and not any(m.name in ("skip", "skipif", "xfail") for m in marks)
    ids = [i for m in marks if m.name == "parametrize" for i in m.kwargs["ids"]]
    assert ["tests/test_size_gpu.py::test_size_walk[%s]" % i for i in ids] == GPU_TESTS
    assert len(GPU_TESTS) == len(ZM.SIZE.configs) * (sum(SM.n_pieces(ZM.SIZE).values()) + 1 + ZM.SIZE.n_random)
    src = open(os.path.join(ROOT, "tests", "test_size_gpu.py")).read() + open(os.path.join(ROOT, "tests", "walk_harness.py")).read()
    assert "pytest.skip" not in src and "xfail" not in src and "importorskip" not in src


def test_committed_numbers_hold_zero_differing_words_for_every_walk_under_ten_seconds():
    """profiles/size_parity_numbers.json: `python tests/sequence_model.py numbers size <parity JSON> <out>` behind a -m gpu run."""
    num = json.load(open(NUMBERS))["tests"]
    for cfg in ZM.SIZE.configs:
        for wid in SM.walk_ids(ZM.SIZE, cfg):
            e = num.get(SM.test_id(ZM.SIZE, cfg, wid))
            assert e is not None, "no measured figure for %s" % SM.test_id(ZM.SIZE, cfg, wid)
            steps = SM.run_model(ZM.SIZE, cfg, SM.walk_calls(ZM.SIZE, cfg, wid)[1])
            assert e["words_differing"] == 0 and e["state_vs_replay"] == 0 and e["query_vs_fresh"] == 0 and e["second_pass"] == 0
            assert e["idle_training"] == 0 and e["idle_trainings"] == sum(1 for s in steps if SM.idle(ZM.SIZE, cfg, s))
            assert e["calls"] == len(steps) and e["expected_errors"] == sum(1 for s in steps if s.status != SM.BP_OK)
            assert e["queries_compared"] == sum(1 for s in steps if s.status == SM.BP_OK and not SM.KINDS[s.kind].training
                                                and s.kind not in ("checkpoint", "set_forward"))
            assert e["seconds"] < 10.0, (SM.test_id(ZM.SIZE, cfg, wid), e["seconds"])
    # profiles/xsize_parity_numbers.json: `python tests/sequence_model.py numbers xsize <parity JSON> <out>` behind a -m gpu run of
    # the walks of the family XSIZE
    num = json.load(open(X_NUMBERS))["tests"]
    assert sorted(num) == sorted(X_GPU_TESTS)
    for cfg in ZM.XSIZE.configs:
        for wid in SM.walk_ids(ZM.XSIZE, cfg):
            e = num.get(SM.test_id(ZM.XSIZE, cfg, wid))
            assert e is not None, "no measured figure for %s" % SM.test_id(ZM.XSIZE, cfg, wid)
            steps = SM.run_model(ZM.XSIZE, cfg, SM.walk_calls(ZM.XSIZE, cfg, wid)[1])
            assert e["words_differing"] == 0 and e["state_vs_replay"] == 0 and e["query_vs_fresh"] == 0 and e["second_pass"] == 0
            assert e["idle_training"] == 0 and e["idle_trainings"] == sum(1 for s in steps if SM.idle(ZM.XSIZE, cfg, s))
            assert e["calls"] == len(steps) and e["expected_errors"] == sum(1 for s in steps if s.status != SM.BP_OK)
            assert e["checkpoints"] == sum(1 for s in steps if s.kind == "checkpoint" and s.status == SM.BP_OK)
            assert e["queries_compared"] == sum(1 for s in steps if s.status == SM.BP_OK and not SM.KINDS[s.kind].training
                                                and s.kind not in SM.NO_FRESH)
            assert e["seconds"] < 10.0, (SM.test_id(ZM.XSIZE, cfg, wid), e["seconds"])
