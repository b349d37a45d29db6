"""The run-time switches of the forward epilogues and, for every forward kernel that carries one, the GPU test that runs the kernel
with the switch on against a reference (tests/test_switch_coverage.py checks the table without a GPU; tests/dispatch_np.py says
which kernels a run launches).  The dispatch matrix counts template instantiations; its 24 cases leave these switches at rest.

  dropout  hidden dropout: the Philox words of drop_words4 by (row, unit) of each tile layout     the hidden-forward kernels
  offset   rank_frame_offset & 3 != 0: the two-block branches 1, 2, 3 of drop_words4              the same, and both staging forms
  alpha    keep-scaling, alpha = 1 - omit: forward and CV on a handle with dropout configured     every forward kernel
  loss     output_loss 1: d *= o (1 - o) on the logistic columns                                  the logistic output kernels

A Run is one call sequence of one test on one handle configuration: out = None or (linear_cols, loss); drop = None or the omit
probabilities; calls out of "step" (fused training), "grads" (gradient store), "forward", "cv"; offset = rank_frame_offset;
upload = "stacked" or "windows".  Existing tests are listed with the configurations they have (their case lists are imported), new
ones are marked new: tests/test_switch_coverage.py asks the committed figures of a GPU run for each of them.

The second half holds the shard problems of tests/test_rank_offset_gpu.py and their mutants, shared with the CPU check."""
import collections

import numpy as np

import dispatch_cases as DC
import dispatch_np as D

SWITCHES = ("dropout", "offset", "alpha", "loss")
Run = collections.namedtuple("Run", ["test", "ls", "B", "dtype", "out", "drop", "calls", "offset", "upload", "new"])
OMIT = dict(visible_omit=0.1, hid_omit=0.2)           # what every existing dropout test configures


def _run(test, ls, B, dtype, calls, out=None, drop=None, offset=0, upload="stacked", new=False):
    return Run(test, list(ls), int(B), int(dtype), out, drop, tuple(calls), int(offset), upload, new)


# ------------------------------------------------------------------ the shard problems of tests/test_rank_offset_gpu.py
# One handle per bunch size B = 1, 2, 3 (mod 4) with global_bunchsize 2B and rank_frame_offset B: the second of two ranks.  Sigmoid
# hidden layers, visible_omit 0.1.  hid_omit: 0.2 unless a mutant then moves a tensor of the reference gradient by less than twice
# the bf16 bar (tests/test_switch_coverage.py::test_rank_offset_mutants_are_visible prints the ratios; DESIGN.md 2 has them).
Shard = collections.namedtuple("Shard", ["id", "ls", "dtype", "bunches", "hid_omit", "reaches"])
SHARDS = [
    Shard("f32_32x32", [70, 65, 130, 33], 0, (25, 26, 27), 0.2, "fp32 32x32 forward"),
    Shard("f32_32x64", [70, 600, 520, 40], 0, (25, 26, 27), 0.2, "both fp32 32x64 forwards (tags 1 and 0)"),
    Shard("bf_rows32", [70, 130, 40], 1, (25, 26, 27), 0.2, "bf16 32-row forward"),
    Shard("bf_rows64", [130, 6600, 40], 1, (301, 302, 303), 0.2, "bf16 64-row forward"),
    Shard("bf_rows128", [70, 2100, 2000, 40], 1, (1001, 1002, 1003), 0.5, "bf16 128-row register-staged and LDS-DMA forwards"),
]
SHARD_BY_ID = {s.id: s for s in SHARDS}
SHARD_SEED = 20261
SHARD_RUNS = [(s.id, B) for s in SHARDS for B in s.bunches]
WINDOW_SHARD = ("f32_32x32", 27)                      # the window upload of the same shard: offset 27 = 3 (mod 4)
BF16_BAR = 2e-2
MUTANTS = ("hidden masks at offset + 1", "all masks at offset 0", "row and unit exchanged")


def shard_drop(s):
    return dict(visible_omit=0.1, hid_omit=s.hid_omit)


def shard_case(s, B):
    return DC.Case("%s-%d" % (s.id, B), s.ls, B, s.dtype, 1, None, None, s.reaches)


def shard_masks(s, B, mutant=None, step=0):
    """The masks of the shard's rows from tests/philox_np.py: global frame = row + B.  mutant: one of MUTANTS."""
    from philox_np import drop_mask
    out = []
    for l in range(len(s.ls) - 1):
        p, off = (0.1 if l == 0 else s.hid_omit), B
        if mutant == MUTANTS[0] and l > 0:
            off = B + 1
        if mutant == MUTANTS[1]:
            off = 0
        if mutant == MUTANTS[2]:                                   # the key's row and unit change places: the mask of the transposed problem
            out.append(np.ascontiguousarray(drop_mask(SHARD_SEED, step, l, s.ls[l], B, p, frame_off=off).T))
        else:
            out.append(drop_mask(SHARD_SEED, step, l, B, s.ls[l], p, frame_off=off))
    return out


def shard_oracle(s, B, W, b, acc_double=False):
    from oracle import oracle as O
    return O.Oracle(s.ls, B, 1.0, 0.5, 0.0, W, b, activation=1, compute_dtype=s.dtype, acc_double=acc_double, dropoutflag=1,
                    seed=SHARD_SEED, **shard_drop(s))


def shard_reference(s, B, masks=None, acc_double=False):
    """(W, b, x, t, masks, (gw, gb, ys)): the oracle's gradient of the shard's B rows at scale 2 / (2B), with its own masks drawn at
    global frame B unless masks are given."""
    W, b, x, t = DC.case_data(shard_case(s, B), B)
    o = shard_oracle(s, B, W, b, acc_double)
    if masks is None:
        masks = [o.fill_mask(0, l, B, gframe0=B) for l in range(len(s.ls) - 1)]
    gw, gb, ys, _ = o.grads(x, t, masks=masks, scale_frames=2 * B)
    return W, b, x, t, masks, (gw, gb, ys)


def distance(dtype, a, ref):
    """The error norm of the dispatch matrix: fp32 max|a - ref| / max|ref|, bf16 rms."""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    if dtype == 0:
        return float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-30))
    return float(np.sqrt(((a - ref) ** 2).sum()) / max(np.sqrt((ref ** 2).sum()), 1e-30))


def window_problem(B):
    """A chunk of 2B samples of the f32_32x32 shard as raw frames + tables (14 bins x 5 frames = 70 inputs) and the same stacked."""
    s = SHARD_BY_ID[WINDOW_SHARD[0]]
    D_, ctx, n, nf = 14, 5, 2 * B, 90
    assert D_ * ctx == s.ls[0]
    rng = np.random.default_rng(53)
    fea = rng.normal(size=(nf, D_)).astype(np.float32)
    tg = rng.normal(size=(nf, s.ls[-1])).astype(np.float32)
    ws = rng.integers(0, nf - ctx + 1, size=n).astype(np.int32)
    tf = rng.integers(0, nf, size=n).astype(np.int32)
    rows = np.ascontiguousarray(np.stack([fea[w:w + ctx].reshape(-1) for w in ws]))
    return fea, tg, ctx, ws, tf, rows, np.ascontiguousarray(tg[tf])


# ------------------------------------------------------------------ the runs
def _existing_runs():
    import exact_data as X
    import test_dp_native as TDN
    import test_gpu_parity as TGP
    import test_output_act_gpu as TOA
    runs = []
    for ls, B, nb, act, rule, wc, drop in TGP.CASES:
        runs.append(_run("tests/test_gpu_parity.py::test_train_matches_oracle", ls, B, 0, ("step", "cv", "forward"), drop=OMIT if drop else None))
    for ls, B, nb, act, rule, wc, drop in TGP.BF_CASES:
        runs.append(_run("tests/test_gpu_parity.py::test_bf16_step_matches_bf16_oracle", ls, B, 1, ("forward", "step", "cv"), drop=OMIT if drop else None))
    for name, ls, B, world, nb, extra in TDN.CASES:
        for r in range(world):                                     # rank r's handle; rank 0 also runs CV and a forward
            runs.append(_run("tests/test_dp_native.py::test_native_dp_matches_global_bunch_oracle[%s]" % name, ls, B, extra.get("compute_dtype", 0),
                             ("step", "cv", "forward") if r == 0 else ("step",), drop=OMIT if extra.get("drop") else None, offset=r * B))
    S, SH = TOA.SMALL, TOA.SHIPPED
    oa = "tests/test_output_act_gpu.py::"
    runs += [
        _run(oa + "test_small_net_gradient_matches_float64_autograd[lin16-mse]", S, 64, 0, ("grads",), out=(16, 1)),
        _run(oa + "test_small_net_ten_step_trajectory[all-logistic-mse]", S, 64, 0, ("step",), out=(0, 1)),
        _run(oa + "test_shipped_geometry_multi_objective_gradient_on_the_split_path", SH, 128, 0, ("grads",), out=(129, 0), drop=OMIT),
        _run(oa + "test_shipped_geometry_ten_steps_small_lrate", SH, 128, 0, ("step", "forward"), out=(129, 0), drop=OMIT),
        _run(oa + "test_cv_and_forward_are_post_activation[small]", S, 64, 0, ("cv", "forward"), out=(16, 0), drop=OMIT),
        _run(oa + "test_cv_and_forward_are_post_activation[shipped]", SH, 128, 0, ("cv", "forward"), out=(129, 0), drop=OMIT),
        _run(oa + "test_bf16_logistic_gradient_on_the_split_path", [300, 1024, 1024, 257], 256, 1, ("grads",), out=(100, 0), drop=OMIT),
    ]
    drop = dict(visible_omit=X.DROP["visible_omit"], hid_omit=X.DROP["hid_omit"])
    for cid in X.DROPOUT_CASES:
        c = DC.BY_ID[cid]
        new = cid == "bf_rows64"
        runs.append(_run("tests/test_exact_gpu.py::test_gradient_store_is_exact[%s-dropout]" % cid, c.ls, c.B, c.dtype, ("grads",), c.out, drop, new=new))
        runs.append(_run("tests/test_exact_gpu.py::test_fused_step_is_exact[%s-dropout]" % cid, c.ls, c.B, c.dtype, ("step",), c.out, drop, new=new))
    for cid in X.SHARD_CASES:
        c = DC.BY_ID[cid]
        runs.append(_run("tests/test_exact_gpu.py::test_shard_gradient_store_is_exact[%s]" % cid, c.ls, c.B, c.dtype, ("grads",), c.out, drop,
                         offset=X.shard_of(cid)[0], new=True))
    return runs


def _new_runs():
    dg = "tests/test_dispatch_gpu.py::"
    runs = []
    for c in DC.LOSS1_CASES:
        for test, call in (("test_gradient_store_loss1", "grads"), ("test_fused_step_loss1", "step"), ("test_short_trajectory_loss1", "step")):
            runs.append(_run("%s%s[%s]" % (dg, test, c.id), c.ls, c.B, c.dtype, (call,), c.out, new=True))
    for c in DC.CASES:
        runs.append(_run("%stest_forward_and_cv_keep_scaled[%s]" % (dg, c.id), c.ls, c.B, c.dtype, ("forward", "cv"), c.out,
                         dict(visible_omit=DC.KEEP_DROP["visible_omit"], hid_omit=DC.KEEP_DROP["hid_omit"]), new=True))
    for sid, B in SHARD_RUNS:
        s = SHARD_BY_ID[sid]
        runs.append(_run("tests/test_rank_offset_gpu.py::test_shard_gradient_at_an_unaligned_offset[%s-%d]" % (sid, B), s.ls, B, s.dtype,
                         ("grads",), drop=shard_drop(s), offset=B, new=True))
    s = SHARD_BY_ID[WINDOW_SHARD[0]]
    runs.append(_run("tests/test_rank_offset_gpu.py::test_window_staging_at_an_unaligned_offset", s.ls, WINDOW_SHARD[1], s.dtype, ("grads",),
                     drop=shard_drop(s), offset=WINDOW_SHARD[1], upload="windows", new=True))
    return runs


_RUNS = []


def runs():
    if not _RUNS:
        _RUNS.extend(_existing_runs() + _new_runs())
    return list(_RUNS)


# ------------------------------------------------------------------ what a run launches with a switch on
def _forward_names(ls, B, dtype, out_act):
    c = D.Config(ls, B, dtype, out_act)
    fwd = D.fwd_bf16 if c.bf else D.fwd_fp32
    return set(fwd(c, l).name for l in range(1, c.L - 1)), fwd(c, c.L - 1).name


def switched_on(run):
    """{switch: the forward kernels that run launches with the switch on}, from tests/dispatch_np.py alone."""
    hidden, output = _forward_names(run.ls, run.B, run.dtype, 1 if run.out else 0)
    trains = "step" in run.calls or "grads" in run.calls
    on = {s: set() for s in SWITCHES}
    if run.drop and run.drop["hid_omit"] > 0 and trains:
        on["dropout"] = set(hidden)
        if run.offset & 3:
            on["offset"] = set(hidden)
    if run.drop and ("forward" in run.calls or "cv" in run.calls):
        on["alpha"] = hidden | {output}
    if run.out is not None and run.out[1] == 1 and trains:
        on["loss"] = {output}
    return on


def staging_form(run):
    """The staging form a training run masks its visible layer through at an unaligned offset, or None: "stage_rows_block"
    (stacked chunk, visible dropout on) or "bp_stage_bunch" (window chunk)."""
    if not (run.drop and run.drop["visible_omit"] > 0 and run.offset & 3 and ("step" in run.calls or "grads" in run.calls)):
        return None
    return "bp_stage_bunch" if run.upload == "windows" else "stage_rows_block"


def carriers():
    """{switch: the kernels that carry it}: every kernel of the kind that a case of the dispatch matrix launches."""
    hidden, output, logistic = set(), set(), set()
    for c in DC.CASES:
        h, o = _forward_names(c.ls, c.B, c.dtype, 1 if c.out else 0)
        hidden |= h
        output.add(o)
        if c.out is not None:
            logistic.add(o)
    return {"dropout": hidden, "offset": hidden, "alpha": hidden | output, "loss": logistic}


def cells(all_runs=None):
    """{(switch, kernel): [tests]} and, for the offset switch, {(kernel, branch 1 .. 3): [tests]} and {staging form: [tests]}."""
    all_runs = runs() if all_runs is None else all_runs
    table = {(s, k): [] for s, ks in carriers().items() for k in ks}
    branches = {(k, br): [] for k in carriers()["offset"] for br in (1, 2, 3)}
    staging = {"stage_rows_block": [], "bp_stage_bunch": []}
    for r in all_runs:
        for s, ks in switched_on(r).items():
            for k in ks:
                table.setdefault((s, k), []).append(r.test)          # (a kernel outside the dispatch matrix: the coverage test names it)
                if s == "offset":
                    branches.setdefault((k, r.offset & 3), []).append(r.test)
        if staging_form(r):
            staging[staging_form(r)].append(r.test)
    return table, branches, staging


def short(kernel):
    return kernel[5:kernel.rindex("(")].replace("GemmKernel", "K")


# ------------------------------------------------------------------ the figures of a GPU run
def figure(record):
    """(text, value, bar) of a test from the record it left in the parity JSON (conftest.py): the worst error / bar ratio over every
    {"errors", "bar" or "bars"} entry, or the number of unequal words of a bit-for-bit test (bar 0).  None without either."""
    worst, unequal = None, None
    for entry in (record or {}).values():
        if not isinstance(entry, dict):
            continue
        if "unequal" in entry:
            unequal = (unequal or 0) + int(sum(entry["unequal"].values()))
        if "errors" in entry:
            for k, v in entry["errors"].items():
                bar = entry["bars"][k] if "bars" in entry else entry["bar"]
                if worst is None or v / bar > worst[1] / worst[2]:
                    worst = (k, float(v), float(bar))
    if unequal:                                                    # unequal words outweigh any error figure
        return "%d words unequal / 0" % unequal, unequal, 0
    if worst is not None:
        return "%s %.1e / %.0e" % worst, worst[1], worst[2]
    if unequal is not None:
        return "0 words unequal / 0", 0, 0
    return None


def new_tests():
    return sorted(set(r.test for r in runs() if r.new))


def numbers_from_records(tests):
    out = {"figures": {}, "tests": {}}
    for t in new_tests():
        fig = figure(tests.get(t))
        assert fig is not None, "no record of %s in the parity JSON" % t
        out["figures"][t] = fig[0]
        out["tests"][t] = tests[t]
    return out


def markdown_table():
    """kernel x switch -> a test that runs it with the switch on (and how many more do), for DESIGN.md 2; `-`: the kernel does
    not carry the switch.  The offset column holds one test per branch 1, 2, 3."""
    table, branches, staging = cells()

    def cell(ts):
        ts = sorted(set(t.split("::")[1] for t in ts), key=lambda t: (not any(m in t for m in ("loss1", "keep_scaled", "shard", "window", "rows64-dropout")), t))
        return "`%s`%s" % (ts[0], " +%d" % (len(ts) - 1) if len(ts) > 1 else "")
    rows = ["| kernel | dropout | offset, branches 1 / 2 / 3 | alpha | loss |", "|---|---|---|---|---|"]
    for k in sorted(carriers()["alpha"]):
        line = [cell(table[(s, k)]) if (s, k) in table else "-" for s in ("dropout",)]
        line.append("<br>".join(cell(branches[(k, br)]) for br in (1, 2, 3)) if (k, 1) in branches else "-")
        line += [cell(table[(s, k)]) if (s, k) in table else "-" for s in ("alpha", "loss")]
        rows.append("| `%s` | %s |" % (short(k), " | ".join(line)))
    for form, ts in sorted(staging.items()):
        rows.append("| staging: `%s` | - | %s | - | - |" % (form, cell(ts)))
    return "\n".join(rows)


if __name__ == "__main__":
    import json
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    path = os.path.join(root, "profiles", "switch_parity_numbers.json")
    if sys.argv[1:2] == ["numbers"]:                               # python tests/switch_cases.py numbers <parity JSON of a -m gpu run>
        src = json.load(open(sys.argv[2]))
        out = numbers_from_records(src["tests"])
        out["written"] = src.get("written")
        json.dump(out, open(path, "w"), indent=1, sort_keys=True)
    print(markdown_table())
