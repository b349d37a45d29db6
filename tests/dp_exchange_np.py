"""The data-parallel exchange restated (no GPU, nothing from the product): the slicing of bp_dp_attach_ex, the launch shapes of
dp_update_grid / dp_push_layer, the hand-off predicate of step_wgrads_count, the ordered reduce of bp_dp_reduce_update<WORLD, GBF16>
with the bf16 rounding of bp_dp_push<true>, and -- from these -- which feature of that code which case of the table below reaches.

    segment l   [W_l | b_l] in the flat gradient buffer: ld_prev * ld_cur + ld_cur floats, widths padded to 64; W_l ends at w_end
    slicing     cnt4 = g_cnt / 4, per4 = ceil(cnt4 / world), slice r = [min(per4 r, cnt4), min(per4 (r + 1), cnt4)) float4
    update grid min(ceil(n4 / 1024), 224 for layer 1 else 128) workgroups of 256 threads, 4 float4 per thread and pass
    push grid   the same rule on the whole segment; the kernel walks slice after slice with that grid
    reduce      s = ((G_0 + G_1) + ...) + G_{world-1} in float32; transport 3: every G_p rounded to bf16 (nearest even) first
    update      update_cases.restate (float64), or, from zero momentum with weight cost 0 and c1 = 1, D = -(s / Bg) to the bit

ARITHMETIC THE TABLE RESTS ON.  Padded widths are multiples of 64, so cnt4 = 16 a (64 b + 1) with a = ld_cur / 64, b = ld_prev / 64:
always a multiple of 16.  Worlds 1, 2 and 4 therefore cut every segment into equal slices, whatever the net (`cnt4 % 4 != 0` does not
exist); a short last slice needs a world that is no power of two -- 3 in this suite, where cnt4 % 3 = a (b + 1) % 3.  An empty
slice needs per4 (world - 1) >= cnt4 with per4 < cnt4 / world + 1, so cnt4 < world (world - 1) <= 56 at up to 8 ranks, and the smallest
segment there is (64 x 64 + 64) / 4 = 1040 float4.

tests/test_dp_exchange_host.py holds the table to these statements; tests/test_dp_exchange_gpu.py runs it."""
import collections

import numpy as np

PULL, RCCL, PUSH, PUSH_BF16 = 0, 1, 2, 3
THREADS, UNROLL = 256, 4                       # bp_dp_reduce_update / bp_dp_push: one float4 per thread, U = 4 per pass
GRID_CAP_LAYER1, GRID_CAP_OTHER = 224, 128
SMALLEST_SEGMENT4 = (64 * 64 + 64) // 4


def pad64(v):
    return (v + 63) & ~63


Segment = collections.namedtuple("Segment", ["layer", "ld_prev", "ld_cur", "g_cnt", "w_end", "cnt4"])


def segments(ls):
    """Segment of every weight layer (list index = layer - 1); w_end is relative to the segment's start."""
    out = []
    for l in range(1, len(ls)):
        lp, lc = pad64(ls[l - 1]), pad64(ls[l])
        out.append(Segment(l, lp, lc, lp * lc + lc, lp * lc, (lp * lc + lc) // 4))
    return out


def slices(cnt4, world):
    """(per4, [(lo, hi) float4 of rank r])"""
    per4 = (cnt4 + world - 1) // world
    return per4, [(min(per4 * r, cnt4), min(per4 * (r + 1), cnt4)) for r in range(world)]


def grid(n4, layer):
    g = min((n4 + THREADS * UNROLL - 1) // (THREADS * UNROLL), GRID_CAP_LAYER1 if layer == 1 else GRID_CAP_OTHER)
    return max(g, 1)


def capped(n4, layer):
    return (n4 + THREADS * UNROLL - 1) // (THREADS * UNROLL) > (GRID_CAP_LAYER1 if layer == 1 else GRID_CAP_OTHER)


def passes(n4, g):
    return (n4 + UNROLL * g * THREADS - 1) // (UNROLL * g * THREADS)


def partial_last_pass(n4, g):
    return n4 % (UNROLL * g * THREADS) != 0


def handoff(case, transport):
    """'in_kernel': the weight-gradient launch counts its tiles and the exchange stream waits beside it; 'events' otherwise."""
    ok = transport != RCCL and case.dtype == 0 and case.B in (128, 256, 512) and len(case.ls) - 1 <= 4
    return "in_kernel" if ok else "events"


# ------------------------------------------------------------------ bf16, on the uint32 view
def f2bf_bits(u):
    """bp_dp_f2bf on uint32 words: round to nearest even, a NaN stays a NaN (quiet bit set)."""
    u = np.asarray(u, np.uint32)
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    r = (u + (np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1)))) >> np.uint32(16)     # (no carry out: non-NaN words are <= 0xFF800000)
    return np.where(nan, (u >> np.uint32(16)) | np.uint32(0x40), r).astype(np.uint32)


def bf16_round(x, mode="nearest_even"):
    """float32 -> bf16 -> float32.  mode 'truncate' and 'none' are the two wrong contributions of the mutant table."""
    x = np.ascontiguousarray(x, np.float32)
    if mode == "none":
        return x.copy()
    u = x.view(np.uint32)
    h = f2bf_bits(u) if mode == "nearest_even" else u >> np.uint32(16)
    return (h << np.uint32(16)).astype(np.uint32).view(np.float32).reshape(x.shape)


def ordered_sum(parts, transport, rounding="nearest_even", order=None):
    """s = ((G_0 + G_1) + ...) + G_{world-1}, float32 after every addition; elementwise, so any layout (flat, padded, unpadded)."""
    parts = [np.ascontiguousarray(p, np.float32) for p in parts]
    if transport == PUSH_BF16:
        parts = [bf16_round(p, rounding) for p in parts]
    order = list(range(len(parts))) if order is None else list(order)
    s = parts[order[0]].copy()
    for p in order[1:]:
        s = (s + parts[p]).astype(np.float32)
    return s


def exact_step(s, n):
    """update_delta from zero momentum with weight cost 0 and c1 = 1: 0 - 1 * (s / n + 0 * w) = -(s / n), one rounding (the division)."""
    return (-(np.asarray(s, np.float32) / np.float32(n))).astype(np.float32)


def ulps(a, b):
    """Distance of two float32 arrays in units of the last place (both zeros are the same number)."""
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


# ------------------------------------------------------------------ the flat layout, for the mutants that move whole words
def flatten(ls, gw, gb):
    """Per layer (list index = layer - 1) the padded segment [ld_prev x ld_cur | ld_cur] of unpadded gw[l] [prev][cur], gb[l]."""
    out = []
    for sg in segments(ls):
        l = sg.layer
        f = np.zeros(sg.g_cnt, np.float32)
        w = f[:sg.w_end].reshape(sg.ld_prev, sg.ld_cur)
        w[:ls[l - 1], :ls[l]] = np.asarray(gw[l], np.float32).reshape(ls[l - 1], ls[l])
        f[sg.w_end:sg.w_end + ls[l]] = np.asarray(gb[l], np.float32).reshape(-1)
        out.append(f)
    return out


def unflatten(ls, flat):
    """The inverse view: ([None, W_1, ...], [None, b_1, ...]) without the pad rows and columns."""
    gw, gb = [None], [None]
    for sg, f in zip(segments(ls), flat):
        l = sg.layer
        gw.append(f[:sg.w_end].reshape(sg.ld_prev, sg.ld_cur)[:ls[l - 1], :ls[l]].copy())
        gb.append(f[sg.w_end:sg.w_end + ls[l]].copy())
    return gw, gb


WORD_MUTANTS = ("contribution_left_out", "contribution_counted_twice", "slot_of_next_rank", "reverse_order", "bf16_truncated",
                "bf16_not_rounded", "first_float4_of_neighbour_slice")


def mutant_applies(mutant, world, transport):
    """Where a wrong exchange computes something else than the right one at all: summing backwards is the same sum for two ranks --
    and for bf16 contributions: 8 significant bits each, so the float32 sum of up to four of them is exact, in any order, unless
    their exponents lie more than 14 apart --, the bf16 mutants exist in transport 3 only, a slice has a neighbour from two ranks on."""
    if mutant == "reverse_order":
        return world >= 3 and transport != PUSH_BF16
    if mutant in ("bf16_truncated", "bf16_not_rounded"):
        return transport == PUSH_BF16
    if mutant == "first_float4_of_neighbour_slice":
        return world >= 2
    return True


def reduce_flat(flat_by_rank, world, transport, mutant=None):
    """The reduce-scatter on padded segments, slice by slice as the owners run it: flat_by_rank[p][layer - 1] -> [s per layer].
    mutant: one of WORD_MUTANTS.  The word mutants hit the slice of the LAST owner (the short one where there is one) and rank 0's
    contribution; a receive slot read one slot further holds the next rank's contribution, and zeros behind the last slot."""
    assert mutant is None or mutant in WORD_MUTANTS, mutant
    rounding = {"bf16_truncated": "truncate", "bf16_not_rounded": "none"}.get(mutant, "nearest_even")
    out = []
    for i in range(len(flat_by_rank[0])):
        cnt4 = flat_by_rank[0][i].size // 4
        _, sl = slices(cnt4, world)
        s = np.zeros(4 * cnt4, np.float32)
        for r, (lo, hi) in enumerate(sl):
            parts = [flat_by_rank[p][i][4 * lo:4 * hi] for p in range(world)]
            order = None
            if r == world - 1:
                if mutant == "contribution_left_out":
                    parts[0] = np.zeros_like(parts[0])
                elif mutant == "contribution_counted_twice":
                    parts[0] = (bf16_round(parts[0]) if transport == PUSH_BF16 else parts[0]) * np.float32(2)
                elif mutant == "slot_of_next_rank":
                    parts[0] = parts[1] if world > 1 else np.zeros_like(parts[0])
            if mutant == "reverse_order":
                order = range(world - 1, -1, -1)
            s[4 * lo:4 * hi] = ordered_sum(parts, transport, rounding, order)
        if mutant == "first_float4_of_neighbour_slice":
            right = s.copy()
            for r in range(1, world):
                (lo, _), (plo, _) = sl[r], sl[r - 1]
                s[4 * lo:4 * lo + 4] = right[4 * plo:4 * plo + 4]
        out.append(s)
    return out


# ------------------------------------------------------------------ the case table
Case = collections.namedtuple("Case", ["id", "ls", "B", "world", "dtype", "hset"])

FEATURES = ("short_last_slice", "slices_all_equal", "one_partial_pass", "several_passes_partial_last", "grid_cap_layer1",
            "grid_cap_other_layers", "push_several_passes", "w_end_inside_last_slice", "handoff_in_kernel", "handoff_events",
            "compute_fp32", "compute_bf16", "world_1", "world_2", "world_3", "world_4")


def short_at(ls, world):
    return [sg.layer for sg in segments(ls) if sg.cnt4 % world]


def pick_ragged(candidates):
    """The first net whose every segment has a short last slice at world 3 (cnt4 % 3 != 0 in every layer)."""
    for ls in candidates:
        if len(short_at(ls, 3)) == len(ls) - 1:
            return ls
    raise AssertionError("no candidate is ragged in every layer at world 3")


# 70-65-130-33 (the older DP tests' odd net) has a short slice in its last layer only; the next two in one layer each
RAGGED = pick_ragged([[70, 65, 130, 33], [70, 65, 33], [40, 130, 33], [40, 200, 50, 33]])
# layer 1 1088 x 2048, layer 2 2048 x 1088 padded: 557 568 and 557 328 float4.  Layer 2's slices at worlds 2, 3, 4 (278 664, 185 776,
# 139 332) all exceed the 131 072 float4 one pass of 128 workgroups covers; layer 1's slice at world 2 (278 784) exceeds the 229 376 of
# 224 workgroups, at worlds 3 and 4 it runs uncapped in one partial pass
WIDE = [1030, 2040, 1030, 40]
HANDOFF = [70, 65, 130, 33]                    # bunch 128, three weight layers, fp32: the tile-counting launch
BF16 = [70, 130, 200, 40]


def _table():
    cases, sets = [], ("A", "B")
    def add(name, ls, B, world, dtype=0):
        cases.append(Case(name, ls, B, world, dtype, sets[len(cases) % 2]))
    for w in (1, 2, 3, 4):
        add("ragged_w%d" % w, RAGGED, 32, w)
    for w in (2, 3, 4):
        add("wide_w%d" % w, WIDE, 32, w)
    add("handoff_b128_w2", HANDOFF, 128, 2)
    add("bf16_w2", BF16, 32, 2, dtype=1)
    # RCCL's only world on one device; its update kernel takes the same grids.  (Bunch 128: at a global minibatch of 32 the weight
    # cost moves this net's update by 2e-3 only, 200 bars; the hand-off under RCCL is the event one at any bunch)
    add("wide_w1", WIDE, 128, 1)
    add("bf16_w1", BF16, 64, 1, dtype=1)
    return cases


CASES = _table()
BY_ID = {c.id: c for c in CASES}
NATIVE = (PULL, PUSH, PUSH_BF16)
RCCL_IDS = ("wide_w1", "bf16_w1")              # (one communicator each: RCCL's start-up is most of a run's time)
RUNS = [(c, t) for c in CASES if c.id not in RCCL_IDS for t in NATIVE] + [(BY_ID[i], RCCL) for i in RCCL_IDS]
RUN_IDS = ["%s-t%d" % (c.id, t) for c, t in RUNS]


def claims(case, transport):
    """The features of the exchange code this case reaches under this transport."""
    got = {"world_%d" % case.world, "compute_bf16" if case.dtype else "compute_fp32", "handoff_" + handoff(case, transport)}
    for sg in segments(case.ls):
        per4, sl = slices(sg.cnt4, case.world)
        lens = [hi - lo for lo, hi in sl]
        got.add("slices_all_equal" if len(set(lens)) == 1 else "short_last_slice")
        assert len(set(lens[:-1])) <= 1 and 0 < lens[-1] <= per4, (case.id, sg.layer, lens)
        for n4 in lens:
            g = grid(n4, sg.layer)
            if capped(n4, sg.layer):
                got.add("grid_cap_layer1" if sg.layer == 1 else "grid_cap_other_layers")
            if partial_last_pass(n4, g):
                got.add("one_partial_pass" if passes(n4, g) == 1 else "several_passes_partial_last")
        if transport in (PUSH, PUSH_BF16) and any(passes(n4, grid(sg.cnt4, sg.layer)) > 1 for n4 in lens):
            got.add("push_several_passes")
        lo, hi = sl[-1]
        if 4 * lo < sg.w_end < 4 * hi:
            got.add("w_end_inside_last_slice")
    return got


def unreachable(transport):
    """{feature: why the code cannot get there under this transport}.  Everything else must be claimed by a case."""
    if transport == PULL:
        return {"push_several_passes": "the pull form launches no bp_dp_push"}
    if transport == RCCL:
        return {"push_several_passes": "the RCCL transport launches no bp_dp_push",
                "handoff_in_kernel": "bp_dp_attach_ex: counters_ok = transport != BP_DP_TRANSPORT_RCCL",
                "short_last_slice": "bp_dp_attach_ex refuses per4 * world != cnt4 under RCCL, and refuses a world that is no power of two: "
                                    "cnt4 is a multiple of 16, so every world it accepts up to 8 cuts equal slices",
                "world_2": "RCCL refuses two ranks of one communicator on one device",
                "world_3": "bp_dp_attach_ex: the RCCL transport needs a world of 1, 2, 4 or 8",
                "world_4": "RCCL refuses two ranks of one communicator on one device"}
    return {}


def required(transport):
    no = unreachable(transport)
    return [f for f in FEATURES if f not in no]


def empty_cells(runs=None):
    """[(transport, feature)] the code can reach and no run of the table claims."""
    runs = RUNS if runs is None else runs
    have = collections.defaultdict(set)
    for c, t in runs:
        have[t] |= claims(c, t)
    return [(t, f) for t in sorted(have) for f in required(t) if f not in have[t]]


# ------------------------------------------------------------------ what a rank process runs (tests/dp_worker.py, "exchange": true)
def first_hyper(rule):
    """Call 1: weight cost 0 and c1 = 1, so that from zero momentum the update is the scaling -(s / Bg) and nothing else."""
    return dict(rule=rule, m=0.5, wc=0.0, lr=1.0 if rule == 1 else 2.0)


def worker_case(case, transport, hyper2, key):
    d = dict(ls=case.ls, B=case.B, world=case.world, nb=2, key=key, transport=transport, compute_dtype=case.dtype, exchange=True,
             hyper2=dict(m=hyper2.m, wc=hyper2.wc, lr=hyper2.lr))
    d.update(first_hyper(hyper2.rule))
    return d


def table_markdown():
    short = {"short_last_slice": "short last", "slices_all_equal": "equal", "one_partial_pass": "1 partial pass",
             "several_passes_partial_last": "n passes, partial last", "grid_cap_layer1": "cap 224", "grid_cap_other_layers": "cap 128",
             "push_several_passes": "push n passes", "w_end_inside_last_slice": "w_end in last", "handoff_in_kernel": "in-kernel",
             "handoff_events": "events", "compute_fp32": "fp32", "compute_bf16": "bf16"}
    out = ["| feature | " + " | ".join("transport %d" % t for t in (PULL, RCCL, PUSH, PUSH_BF16)) + " |", "|---|---|---|---|---|"]
    for f in FEATURES:
        row = []
        for t in (PULL, RCCL, PUSH, PUSH_BF16):
            who = [c.id for c, tt in RUNS if tt == t and f in claims(c, t)]
            row.append("`%s`%s" % (who[0], " +%d" % (len(who) - 1) if len(who) > 1 else "") if who else ("-" if f in unreachable(t) else "EMPTY"))
        out.append("| %s | %s |" % (short.get(f, f.replace("_", " ")), " | ".join(row)))
    return "\n".join(out)


def numbers_from_records(gpu_tests, host_tests):
    """profiles/dp_exchange_parity_numbers.json from the parity JSONs of `pytest tests/test_dp_exchange_gpu.py -m gpu` and of
    `pytest tests/test_dp_exchange_host.py`: per run the unequal words of step one, the distances of step two, the time; the mutant
    table of the CPU run."""
    pick = lambda tests, name: {k.split("[", 1)[1][:-1]: v for k, v in tests.items() if name in k}
    runs, cross, host = (pick(gpu_tests, "test_exchange_on_the_ranks_own_gradients"), pick(gpu_tests, "test_transports_of_one_case"),
                         pick(host_tests, "test_bars_separate_right_from_wrong"))
    missing = [i for i in RUN_IDS if i not in runs or i not in host]
    assert not missing, "no record of %s" % missing
    slow = max(runs, key=lambda i: runs[i]["seconds"])
    w3 = [i for i in runs if runs[i]["world"] == 3]
    return {"summary": {"runs": len(runs), "unequal_words_step_one": sum(r["step_one"]["unequal_total"] for r in runs.values()),
                        "words_compared_step_one": sum(r["step_one"]["words"] for r in runs.values()),
                        "world_3_division": {"runs": w3, "unequal_words": sum(runs[i]["step_one"]["unequal_total"] for i in w3),
                                             "largest_ulps": max(runs[i]["step_one"]["largest_ulps"] for i in w3),
                                             "words": sum(runs[i]["step_one"]["words"] for i in w3)},
                        "largest_step_two_distance": max(r["step_two"]["worst"] for r in runs.values()),
                        "step_two_bar": runs[slow]["step_two"]["bar"],
                        "seconds_in_rank_processes": sum(r["seconds"] for r in runs.values()), "slowest_run": [slow, runs[slow]["seconds"]]},
            "runs": runs, "transports_of_one_case": cross, "cpu_mutant_tables": host}


if __name__ == "__main__":
    import json
    import os
    import sys
    if sys.argv[1:2] == ["numbers"]:         # python tests/dp_exchange_np.py numbers <parity JSON of the -m gpu run> <parity JSON of the host test>
        gpu, host = json.load(open(sys.argv[2])), json.load(open(sys.argv[3]))             # [<label>=<parity JSON of the same run on a mutant library> ...]
        out = numbers_from_records(gpu["tests"], host["tests"])
        out["written"] = gpu.get("written")
        for arg in sys.argv[4:]:
            label, src = arg.split("=", 1)
            runs = {k.split("[", 1)[1][:-1]: v for k, v in json.load(open(src))["tests"].items() if "test_exchange_on_the_ranks_own_gradients" in k}
            out.setdefault("mutant_libraries_on_the_device", {})[label] = {
                "runs_with_unequal_words_in_step_one": sorted(i for i, r in runs.items() if r["step_one"]["unequal_total"]),
                "runs_outside_the_bar_in_step_two": sorted(i for i, r in runs.items() if not r["step_two"]["worst"] < r["step_two"]["bar"]),
                "runs_that_meet_every_bar": sorted(i for i, r in runs.items() if not r["step_one"]["unequal_total"] and r["step_two"]["worst"] < r["step_two"]["bar"])}
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "dp_exchange_parity_numbers.json")
        json.dump(out, open(path, "w"), indent=1, sort_keys=True)
        print(json.dumps(out["summary"], indent=1))
    print(table_markdown())
    print("empty cells:", empty_cells())
