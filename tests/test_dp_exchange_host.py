"""What tests/test_dp_exchange_gpu.py rests on, checked without a GPU.

  1. The case table of tests/dp_exchange_np.py claims every (transport, feature) cell the exchange code can reach; a cell it cannot
     reach carries the arithmetic that shows it.  Taking a case out opens cells, and the check names them.
  2. The bars separate right from wrong.  The oracle's shard gradients stand in for the device (Oracle.grads on rank p's rows with
     scale_frames = the global minibatch, as tests/test_rank_offset_gpu.py makes them), the restated reduce and the oracle's fp32 update for
     the exchange kernel.  On the rows held bit for bit (step one: D = -(s / Bg)) each of seven wrong exchanges changes at least one
     word the GPU test compares, in every segment it touches; on the restated rows (step two) the five wrong updates of
     update_cases.MUTANTS lie at least MUTANT_FACTOR bars from the right one, and the right one inside the bar.
  3. The restated reduce is deterministic, and its bf16 rounding is the suite's other restatement (torch_ref.bf16_round) on random
     words, on every tie, and keeps a NaN a NaN as bp_dp_f2bf does.

`python tests/test_dp_exchange_host.py` prints the tables of DESIGN.md 2."""
import numpy as np
import pytest

import dp_exchange_np as X
import update_cases as UC
from dp_worker import case_data, shard_rows

ROWS = {}          # run id -> measured values


def _shard_grads(O, c, W, b, x, t, call):
    """[(gw, gb) of rank p] for global minibatch `call` (0, 1): the stand-in for what each rank's store kernels leave."""
    Bg = c.B * c.world
    out = []
    for p in range(c.world):
        rows = shard_rows(x.shape[0], Bg, c.world, p)[call * c.B:(call + 1) * c.B]
        o = O.Oracle(c.ls, c.B, 1.0, 0.5, 0.0, W, b, compute_dtype=c.dtype)
        gw, gb, _, _ = o.grads(x[rows], t[rows], scale_frames=Bg)
        out.append((gw, gb))
    return out


def _words(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _changed(ls, right, wrong):
    """Words per layer in which two reduced segments differ where the GPU test can see them (no pad rows or columns), after the
    exact step -(s / Bg) -- a sign or a power of two changes every word or none."""
    (rw, rb), (mw, mb) = X.unflatten(ls, right), X.unflatten(ls, wrong)
    return [int((_words(rw[l]) != _words(mw[l])).sum() + (_words(rb[l]) != _words(mb[l])).sum()) for l in range(1, len(ls))]


def measure(O, c, transport):
    h = UC.hyper(c.hset, c.dtype)
    Bg, L = c.B * c.world, len(c.ls)
    W0, b0, x, t = case_data(X.worker_case(c, transport, h, "host"))
    # ---- step one, bit for bit
    g1 = _shard_grads(O, c, W0, b0, x, t, 0)
    flat1 = [X.flatten(c.ls, gw, gb) for gw, gb in g1]
    s1 = X.reduce_flat(flat1, c.world, transport)
    again = X.reduce_flat(flat1, c.world, transport)
    assert all(np.array_equal(_words(a), _words(b)) for a, b in zip(s1, again)), (c.id, "the restated reduce is not deterministic")
    # (slice by slice or on the whole tensor: the same sum, which is how the GPU test forms it)
    whole = [X.ordered_sum([flat1[p][i] for p in range(c.world)], transport) for i in range(L - 1)]
    assert all(np.array_equal(_words(a), _words(b)) for a, b in zip(s1, whole)), c.id
    step1 = [X.exact_step(s, Bg) for s in s1]
    row = {"word_mutants": {}}
    for m in X.WORD_MUTANTS:
        if X.mutant_applies(m, c.world, transport):
            row["word_mutants"][m] = _changed(c.ls, step1, [X.exact_step(s, Bg) for s in X.reduce_flat(flat1, c.world, transport, mutant=m)])
    D1, d1 = X.unflatten(c.ls, step1)
    W1 = [None] + [(np.asarray(W0[l], np.float32).reshape(D1[l].shape) + D1[l]).astype(np.float32) for l in range(1, L)]
    b1 = [None] + [(np.asarray(b0[l], np.float32).reshape(-1) + d1[l]).astype(np.float32) for l in range(1, L)]
    # ---- step two, restated
    g2 = _shard_grads(O, c, W1, b1, x, t, 1)
    s2w, s2b = X.unflatten(c.ls, X.reduce_flat([X.flatten(c.ls, gw, gb) for gw, gb in g2], c.world, transport))
    dev = O.Oracle(c.ls, Bg, h.lr, h.m, h.wc, W1, b1, momentum_rule=h.rule)
    for l in range(1, L):
        dev.dW[l][...] = D1[l]
        dev.db[l][...] = d1[l]
    dev.update([None] + [np.ascontiguousarray(g) for g in s2w[1:]], [None] + [np.ascontiguousarray(g) for g in s2b[1:]], Bg)
    want = UC.restate(h, Bg, W1, b1, D1, d1, s2w, s2b)
    row["reference"] = UC.errors((dev.dW, dev.db, dev.W, dev.b), want)[0]
    row["mutants"] = {m: UC.errors(UC.restate(h, Bg, W1, b1, D1, d1, s2w, s2b, mutant=m), want)[0] for m in UC.MUTANTS}
    return row


def tables(rows):
    w = lambda e: max(e.values())
    out = ["| run | set | " + " | ".join(m.replace("_", " ") for m in X.WORD_MUTANTS) + " |", "|---|---|" + "---|" * len(X.WORD_MUTANTS)]
    for rid, r in rows.items():
        out.append("| `%s` | %s | %s |" % (rid, r["set"], " | ".join("/".join(str(n) for n in r["word_mutants"][m]) if m in r["word_mutants"] else "-"
                                                                     for m in X.WORD_MUTANTS)))
    out += ["", "| run | set | reference | " + " | ".join(UC.MUTANTS) + " |", "|---|---|---|" + "---|" * len(UC.MUTANTS)]
    for rid, r in rows.items():
        out.append("| `%s` | %s | %.1e | %s |" % (rid, r["set"], w(r["reference"]), " | ".join("%.1e" % w(r["mutants"][m]) for m in UC.MUTANTS)))
    if rows:
        out.append("worst reference %.1e, nearest mutant %.1e (bar %.0e, mutants must be beyond %.0e)" % (
            max(w(r["reference"]) for r in rows.values()), min(w(r["mutants"][m]) for r in rows.values() for m in UC.MUTANTS), UC.BAR,
            UC.MUTANT_FACTOR * UC.BAR))
    return "\n".join(out)


@pytest.fixture(scope="module", autouse=True)
def _print_tables():
    yield
    print("\n" + tables(ROWS))


# ------------------------------------------------------------------ 1. the table
def test_every_reachable_cell_is_claimed():
    empty = X.empty_cells()
    assert not empty, "no case reaches (transport, feature): %s" % empty
    for t in sorted({t for _, t in X.RUNS}):
        for f, why in X.unreachable(t).items():
            assert f in X.FEATURES and why, (t, f)
            assert not any(f in X.claims(c, tt) for c, tt in X.RUNS if tt == t), (t, f, "is listed as out of reach and a case claims it")


def test_a_case_taken_out_opens_cells_by_name():
    """The coverage check bites: without the three-rank ragged net no transport has a short last slice, without the bunch of 128 none
    the in-kernel hand-off, and a transport nobody listed anything for must have every feature claimed."""
    without = lambda cid: X.empty_cells([(c, t) for c, t in X.RUNS if c.id != cid])
    assert set(without("ragged_w3")) == {(t, "short_last_slice") for t in X.NATIVE}
    assert set(without("handoff_b128_w2")) == {(t, "handoff_in_kernel") for t in X.NATIVE}
    assert (X.PULL, "grid_cap_layer1") in without("wide_w2")
    new = X.empty_cells(X.RUNS + [(X.BY_ID["ragged_w1"], 4)])
    assert (4, "world_2") in new and (4, "push_several_passes") in new, new


def test_the_table_is_what_was_asked_for():
    import test_dp_native
    runs = {(c.id, t) for c, t in X.RUNS}
    for t in X.NATIVE:
        assert {c.world for c, tt in X.RUNS if tt == t} == {1, 2, 3, 4}
        assert any(c.dtype == 1 for c, tt in X.RUNS if tt == t)
        assert ("handoff_b128_w2", t) in runs and X.handoff(X.BY_ID["handoff_b128_w2"], t) == "in_kernel"
    assert all(c.world == 1 for c, t in X.RUNS if t == X.RCCL) and any(t == X.RCCL for _, t in X.RUNS)
    assert all(c.world <= test_dp_native.MAX_RANKS for c in X.CASES)
    # the wide net: every slice of layer 2 takes several passes of 128 workgroups with a partial last one
    sg = X.segments(X.WIDE)[1]
    assert (sg.ld_prev, sg.ld_cur) == (2048, 1088)
    for w in (2, 3, 4):
        for lo, hi in X.slices(sg.cnt4, w)[1]:
            assert hi - lo > 131072 and X.grid(hi - lo, 2) == 128 and X.passes(hi - lo, 128) > 1 and X.partial_last_pass(hi - lo, 128)
    # the ragged net: a short last slice in EVERY layer at three ranks -- and nowhere at 1, 2, 4 ranks, for any net
    assert X.short_at(X.RAGGED, 3) == list(range(1, len(X.RAGGED)))
    assert X.short_at([70, 65, 130, 33], 3) == [3]
    widths = range(64, 64 * 70, 64)
    assert all((lp * lc + lc) // 4 % 16 == 0 for lp in widths for lc in widths)
    assert min(sg.cnt4 for c in X.CASES for sg in X.segments(c.ls)) == X.SMALLEST_SEGMENT4 == 1040
    # the hyper sets alternate, and both reach every transport
    for t in X.NATIVE:
        assert {c.hset for c, tt in X.RUNS if tt == t} == {"A", "B"}


def test_first_call_is_an_exact_scaling():
    """c1 = 1 in float32 under either rule, weight cost 0: update_delta is 0 - 1 * (s / Bg + 0 * w)."""
    for rule in (0, 1):
        f = X.first_hyper(rule)
        c1 = np.float32(f["lr"]) if rule == 1 else (np.float32(1) - np.float32(f["m"])) * np.float32(f["lr"])
        assert c1 == np.float32(1) and f["wc"] == 0.0


# ------------------------------------------------------------------ 2. the bars
@pytest.mark.parametrize("c,transport", X.RUNS, ids=X.RUN_IDS)
def test_bars_separate_right_from_wrong(oracle_mod, parity_record, c, transport):
    rid = "%s-t%d" % (c.id, transport)
    row = ROWS[rid] = dict(measure(oracle_mod, c, transport), set=c.hset)
    parity_record(**row)
    for m, per_layer in row["word_mutants"].items():
        assert min(per_layer) >= 1, (rid, "the wrong exchange", m, "changes no word the GPU test compares in a layer: per layer", per_layer)
    bad = {k: v for k, v in row["reference"].items() if not v < UC.BAR}
    assert not bad, (rid, "outside %.0e" % UC.BAR, bad)
    for m, e in row["mutants"].items():
        assert max(e.values()) >= UC.MUTANT_FACTOR * UC.BAR, (rid, "mutant", m, "is only", max(e.values()), "away", e)


def test_word_mutants_run_where_they_mean_something():
    ran = {m: {(c.world, t) for c, t in X.RUNS if X.mutant_applies(m, c.world, t)} for m in X.WORD_MUTANTS}
    assert {w for w, _ in ran["reverse_order"]} == {3, 4}
    assert {t for _, t in ran["bf16_truncated"]} == {t for _, t in ran["bf16_not_rounded"]} == {X.PUSH_BF16}
    assert all(ran[m] for m in X.WORD_MUTANTS)


# ------------------------------------------------------------------ 3. the rounding
def test_bf16_rounding_is_the_suites_other_restatement():
    from torch_ref import bf16_round
    rng = np.random.default_rng(3)
    u = rng.integers(0, 1 << 32, size=200000, dtype=np.uint64).astype(np.uint32)
    hi = rng.integers(0, 1 << 16, size=4096, dtype=np.uint64).astype(np.uint32) << np.uint32(16)
    ties = np.concatenate([hi | np.uint32(0x8000), hi | np.uint32(0x7FFF), hi | np.uint32(0x8001), hi])      # the tie, and its neighbours
    every_tie = (np.arange(1 << 16, dtype=np.uint32) << np.uint32(16)) | np.uint32(0x8000)
    u = np.concatenate([u, ties, every_tie])
    u = u[(u & np.uint32(0x7FFFFFFF)) < np.uint32(0x7F800000)]              # finite words (the other restatement has no NaN rule)
    x = u.view(np.float32)
    got = X.bf16_round(x)
    assert np.array_equal(got.astype(np.float64).view(np.uint64), bf16_round(x).view(np.uint64))
    assert not (got.view(np.uint32) & np.uint32(0xFFFF)).any()
    t = every_tie[(every_tie & np.uint32(0x7FFFFFFF)) < np.uint32(0x7F800000)]
    assert not ((X.f2bf_bits(t)) & np.uint32(1)).any(), "a tie goes to the even neighbour"
    # between two bf16 neighbours, never further than half their distance
    fin = np.isfinite(got)
    lo = (u & np.uint32(0xFFFF0000)).view(np.float32).astype(np.float64)
    up = ((u & np.uint32(0xFFFF0000)) + np.uint32(0x10000)).view(np.float32).astype(np.float64)
    ok = fin & np.isfinite(up)
    assert (np.abs(got.astype(np.float64) - x.astype(np.float64))[ok] <= (np.abs(up - lo) / 2)[ok]).all()
    # NaN stays NaN, infinities stay themselves (bp_dp_f2bf)
    nan = np.array([0x7FC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0x7F80FFFF], np.uint32)
    assert np.isnan(X.bf16_round(nan.view(np.float32))).all()
    inf = np.array([0x7F800000, 0xFF800000], np.uint32)
    assert np.array_equal(X.bf16_round(inf.view(np.float32)).view(np.uint32), inf)
    # the two wrong roundings are wrong somewhere
    assert (X.bf16_round(x, "truncate") != got).any() and (X.bf16_round(x, "none") != got).any()


def test_numbers_file_has_a_figure_under_its_bar_for_every_run():
    """profiles/dp_exchange_parity_numbers.json is what an MI355X run of the GPU file measured: every run of the table is in it, with
    0 unequal words in step one (at most 1 ulp at three ranks) and a step-two distance under the bar."""
    import json
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "dp_exchange_parity_numbers.json")
    runs = json.load(open(path))["runs"]
    assert sorted(runs) == sorted(X.RUN_IDS)
    for rid, r in runs.items():
        exact = r["global_minibatch"] & (r["global_minibatch"] - 1) == 0
        assert r["step_one"]["largest_ulps"] <= (0 if exact else 1) and (not exact or r["step_one"]["unequal_total"] == 0), rid
        assert r["step_two"]["worst"] < UC.BAR and r["step_two"]["bar"] == UC.BAR, rid
        assert r["handoff"] == X.handoff(X.BY_ID[rid.rsplit("-t", 1)[0]], int(rid.rsplit("-t", 1)[1])), rid


def test_ulps():
    a = np.array([1.0, -1.0, 0.0, -0.0, 1e-45], np.float32)
    b = np.array([np.nextafter(np.float32(1), np.float32(2)), np.nextafter(np.float32(-1), np.float32(-2)), -0.0, 0.0, -1e-45], np.float32)
    assert X.ulps(a, b).tolist() == [1, 1, 0, 0, 2]


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import oracle as O
    O.build()
    for c, t in X.RUNS:
        ROWS["%s-t%d" % (c.id, t)] = dict(measure(O, c, t), set=c.hset)
    print(X.table_markdown() + "\n\n" + tables(ROWS))
