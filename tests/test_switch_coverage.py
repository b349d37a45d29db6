"""Every run-time switch of the forward epilogues has run, switched on, in every forward kernel that carries it, against a
reference -- checked without a GPU.

tests/switch_cases.py lists the runs (test, handle configuration, calls); tests/dispatch_np.py says which forward kernels a run
launches, and the kernels that carry a switch are those the cases of tests/dispatch_cases.py launch: a new template instantiation
opens a cell and fails here with its name.  There is no allowlist.  Also here, from the references alone: the mutants that the new
GPU tests must be able to see (the kernel ignores `loss`; the kernel ignores `alpha`; masks drawn at a wrong offset or with row and
unit exchanged) are far enough from the truth, and the committed figures of a GPU run (profiles/switch_parity_numbers.json) hold one
below its bar for every new test."""
import importlib
import itertools
import json
import os

import numpy as np
import pytest

import dispatch_cases as DC
import dispatch_np as D
import switch_cases as SC
from util import TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NUMBERS = os.path.join(ROOT, "profiles", "switch_parity_numbers.json")


@pytest.fixture(scope="module", autouse=True)
def _oracle_built():
    from oracle import oracle as O
    O.build()


# ------------------------------------------------------------------ 1. the table
def _empty(all_runs):
    table, branches, staging = SC.cells(all_runs)
    return ([(s, SC.short(k)) for (s, k), ts in sorted(table.items()) if not ts],
            [(SC.short(k), br) for (k, br), ts in sorted(branches.items()) if not ts],
            [f for f, ts in sorted(staging.items()) if not ts])


def test_the_carriers_come_from_the_dispatch_matrix():
    car = SC.carriers()
    assert len(car["dropout"]) == 7 and car["offset"] == car["dropout"] and len(car["alpha"]) == 21 and len(car["loss"]) == 7
    every = set().union(*[D.case_kernels(c.ls, c.B, c.dtype, 1 if c.out else 0) for c in DC.CASES])
    assert car["alpha"] <= every and car["loss"] <= car["alpha"] and not car["dropout"] & car["loss"]
    for r in SC.runs():                                              # no run launches a forward kernel that the matrix does not know
        for s, ks in SC.switched_on(r).items():
            assert ks <= car[s], (r.test, s, sorted(ks - car[s]))


def test_every_cell_has_a_run():
    cells, branches, staging = _empty(SC.runs())
    assert not cells, "no test runs these kernels with the switch on (switch, kernel): %s" % cells
    assert not branches, "no test runs these kernels in this two-block branch of drop_words4 (kernel, offset & 3): %s" % branches
    assert not staging, "no test stages a bunch at an unaligned offset through: %s" % staging


def test_without_the_new_runs_the_cells_are_empty_and_named():
    """What the new tests are for: the older runs alone leave these cells empty, and the check above would name each of them."""
    old = [r for r in SC.runs() if not r.new]
    cells, branches, staging = _empty(old)
    per = {s: sorted(k for sw, k in cells if sw == s) for s in SC.SWITCHES}
    assert per["dropout"] == ["bp_gemm_bf16<0, 64, true, false, 1>"]
    assert len(per["offset"]) == 6 and "bp_gemm<32, 32, 64, 1, 1, true, false, 0, 0>" not in per["offset"]
    assert per["alpha"] == sorted(["bp_gemm_bf16<0, 64, true, false, 1>", "bp_gemm_bf16<0, 128, true, false, 1>",
                                   "bp_gemm<32, 64, 64, 1, 2, true, false, 1, 0>", "bp_gemm<32, 64, 64, 1, 2, true, false, 7, 0>",
                                   "bp_gemm_bf16<1, 64, true, false, 1>", "bp_gemm_bf16<1, 128, true, false, 1>",
                                   "bp_gemm_bf16<5, 32, true, false, 1>", "bp_gemm_bf16<5, 32, true, false, 4>",
                                   "bp_gemm_bf16<5, 64, true, false, 1>", "bp_gemm_bf16<5, 128, true, false, 1>"])
    assert len(per["loss"]) == 6 and "bp_gemm<32, 32, 64, 1, 1, true, false, 7, 0>" not in per["loss"]
    assert ("bp_gemm<32, 32, 64, 1, 1, true, false, 0, 0>", 3) in branches and len(branches) == 19      # branch 3 ran nowhere
    assert staging == ["bp_stage_bunch"]
    # every group of new runs is needed: without it a cell opens
    groups = {"loss1": "_loss1[", "keep_scaled": "keep_scaled[", "exact bf_rows64": "[bf_rows64-dropout]", "shards": "test_shard_gradient",
              "window": "test_window_staging"}
    for name, mark in groups.items():
        rest = [r for r in SC.runs() if not (r.new and mark in r.test)]
        assert len(rest) < len(SC.runs()), name
        if name == "exact bf_rows64":                                # (the shards fill its cell too, at the 2e-2 bar: it adds the bit-for-bit form)
            continue
        assert any(_empty(rest)), "the new runs %r fill no cell of their own" % name


def _ids_of(mod, name):
    fn = getattr(mod, name)
    axes = []
    for m in getattr(fn, "pytestmark", []):
        if m.name == "parametrize":
            given = m.kwargs.get("ids")
            if given is None and not all(isinstance(v, (str, int)) for v in m.args[1]):
                return None
            axes.append([str(v) for v in (m.args[1] if given is None else given)])
    if axes:
        return set("-".join(c) for c in itertools.product(*axes))
    args = fn.__code__.co_varnames[:fn.__code__.co_argcount]
    if "case" in args:
        return set(c.id for c in DC.CASES)
    if "loss1_case" in args:
        return set(c.id for c in DC.LOSS1_CASES)
    return None


def test_every_named_test_exists():
    mods = {}
    for t in sorted(set(r.test for r in SC.runs())):
        path, test = t.split("::")
        assert os.path.exists(os.path.join(ROOT, path)), t
        mod = mods.setdefault(path, importlib.import_module(path[len("tests/"):-len(".py")]))
        name = test.split("[")[0]
        fn = getattr(mod, name, None)
        assert callable(fn), "%s has no test %s" % (path, name)
        marks = getattr(mod, "pytestmark", [])
        marks = (marks if isinstance(marks, list) else [marks]) + list(getattr(fn, "pytestmark", []))
        assert any(m.name == "gpu" for m in marks), t
        assert not any(m.name in ("skip", "skipif", "xfail") for m in marks), t
        ids = _ids_of(mod, name)
        if "[" in test:
            assert ids is not None and test[test.index("[") + 1:-1] in ids, "%s: no such id in %s" % (t, path)
    new = SC.new_tests()
    assert len(new) == 3 * 7 + 24 + 2 + 2 + len(SC.SHARD_RUNS) + 1, len(new)    # loss 1, keep, exact dropout, exact shards, shards, window


def test_the_shards_reach_their_kernels_and_keep_the_padded_bunch():
    want = {"f32_32x32": {D.n_gemm(32, 32, 64, 1, 1, True, False, 0)},
            "f32_32x64": {D.n_gemm(32, 64, 64, 1, 2, True, False, 0, 1), D.n_gemm(32, 64, 64, 1, 2, True, False, 0, 0)},
            "bf_rows32": {D.n_bf(0, 32, True)}, "bf_rows64": {D.n_bf(0, 64, True)},
            "bf_rows128": {D.n_bf(0, 128, True), D.n_bf(0, 128, True, True)}}
    for s in SC.SHARDS:
        assert sorted(B & 3 for B in s.bunches) == [1, 2, 3] and len(set(D.pad64(B) for B in s.bunches)) == 1, s.id
        for B in s.bunches:
            assert SC._forward_names(s.ls, B, s.dtype, 0)[0] == want[s.id], (s.id, B)
    assert set().union(*want.values()) == SC.carriers()["offset"]


# ------------------------------------------------------------------ 2. the mutants, from the references alone
def _logistic_grads(c, x, t, loss):
    import output_ref as R
    W, b, _, _ = DC.case_data(c, 1)
    if c.dtype == 1:
        return R.bf16_logistic_grads(c.ls, W, b, x, t, c.act, c.out[0], loss)[:2]
    return R.ref_grads(c.ls, W, b, x, t, act=c.act, lin=c.out[0], loss=loss)[:2]


def test_a_kernel_that_ignores_the_loss_is_far_from_the_reference():
    """The reference gradient at loss 0 against the one at loss 1, per tensor, in the norm and at the bar that
    test_dispatch_gpu.test_gradient_store_loss1 applies: at least 100 x the fp32 bar, 5 x the bf16 bar."""
    smallest = {}
    for c in DC.LOSS1_CASES:
        assert c.out[1] == 1 and DC.BY_ID[c.id[:-4]].out == (c.out[0], 0)
        _, _, x, t = DC.case_data(c, c.B)
        (w0, b0), (w1, b1) = _logistic_grads(c, x, t, 0), _logistic_grads(c, x, t, 1)
        bar = TOL if c.dtype == 0 else 2e-2
        ratios = [SC.distance(c.dtype, a[l], r[l]) / bar for l in range(1, len(c.ls)) for a, r in ((w0, w1), (b0, b1))]
        smallest[c.id] = min(ratios)
        assert min(ratios) >= (100.0 if c.dtype == 0 else 5.0), (c.id, ratios)
    print("loss ignored: smallest distance / bar per case", {k: "%.0f" % v for k, v in smallest.items()})


def _forward_ref(c, W, b, x, drop):
    import output_ref as R
    from oracle import oracle as O
    keep = DC.keep_scales(c, drop) if drop else None
    if c.out is None:
        return O.Oracle(c.ls, c.B, 1.0, 0.5, 0.0, W, b, activation=c.act, compute_dtype=c.dtype, **(drop or {})).forward(x)
    if c.dtype == 1:
        return R.bf16_logistic_grads(c.ls, W, b, x, None, c.act, c.out[0], 0, keep=keep)[3]
    import torch
    with torch.no_grad():
        return R.ref_forward(c.ls, W, b, x, act=c.act, lin=c.out[0], keep=keep)[4].numpy()


def test_a_kernel_that_ignores_alpha_is_far_from_the_reference():
    """The reference forward with keep 1 against the one with the true keep scales, on the B + 3 frames that
    test_forward_and_cv_keep_scaled forwards: at least 100 x the fp32 bar (1e-4), 5 x the bf16 bar (2e-3)."""
    smallest = {}
    for c in DC.CASES:
        W, b, x, _ = DC.case_data(c, c.B + 3)
        true, one = _forward_ref(c, W, b, x, DC.KEEP_DROP), _forward_ref(c, W, b, x, None)
        bar = TOL if c.dtype == 0 else 2e-3
        smallest[c.id] = SC.distance(0, one, true) / bar
        assert smallest[c.id] >= (100.0 if c.dtype == 0 else 5.0), (c.id, smallest[c.id])
    print("alpha ignored: distance / bar per case", {k: "%.0f" % v for k, v in smallest.items()})


def test_the_bf16_keep_restatement_is_the_bf16_oracle():
    """output_ref.bf16_logistic_grads(keep=...) with no logistic column against the bf16 oracle's keep-scaled forward, linear nets
    with ReLU and with Sigmoid: the 2e-3 of the forward bar, and far closer than the unscaled forward."""
    import output_ref as R
    from oracle import oracle as O
    for cid in ("bf_b512", "bf_out_split"):
        c = DC.BY_ID[cid]
        W, b, x, _ = DC.case_data(c, 67)
        o = O.Oracle(c.ls, c.B, 1.0, 0.5, 0.0, W, b, activation=c.act, compute_dtype=1, **DC.KEEP_DROP).forward(x)
        mine = R.bf16_logistic_grads(c.ls, W, b, x, None, c.act, c.ls[-1], 0, keep=DC.keep_scales(c))[3]
        plain = R.bf16_logistic_grads(c.ls, W, b, x, None, c.act, c.ls[-1], 0)[3]
        print(cid, "keep restatement against the bf16 oracle %.2e, unscaled %.2e" % (SC.distance(0, mine, o), SC.distance(0, plain, o)))
        assert SC.distance(0, mine, o) < 2e-3 / 4 and SC.distance(0, plain, o) > 1e-2


@pytest.mark.parametrize("sid", [s.id for s in SC.SHARDS])
def test_rank_offset_mutants_are_visible(sid):
    """Masks drawn at offset + 1 in the hidden layers, all masks at offset 0, and row and unit exchanged in the key: each moves
    every weight gradient and every hidden layer's bias gradient of the reference by at least twice the bar the GPU test applies
    (bf16 2e-2 rms; fp32 1e-4, the looser of its two).  The output layer's bias gradient is the column sum of (o - t) over the
    bunch, a wrong mask moves it by noise that averages out over the rows: its ratio is printed, not asserted.  The three
    implementations of the keying agree on the true masks."""
    s = SC.SHARD_BY_ID[sid]
    B, L = s.bunches[-1], len(s.ls)
    bar = TOL if s.dtype == 0 else SC.BF16_BAR
    _, _, _, _, masks, (gw, gb, _) = SC.shard_reference(s, B)
    mine = SC.shard_masks(s, B)
    glob = [SC.shard_oracle(s, 2 * B, *DC.case_data(SC.shard_case(s, B), 1)[:2]).fill_mask(0, l, 2 * B) for l in range(L - 1)]
    for l in range(L - 1):
        assert np.array_equal(masks[l], mine[l]) and np.array_equal(masks[l], glob[l][B:]), l
        assert not np.array_equal(masks[l], glob[l][:B])
    smallest = {}
    for m in SC.MUTANTS:
        _, _, _, _, _, (mw, mb, _) = SC.shard_reference(s, B, masks=SC.shard_masks(s, B, m))
        asserted = [SC.distance(s.dtype, mw[l], gw[l]) / bar for l in range(1, L)] + [SC.distance(s.dtype, mb[l], gb[l]) / bar for l in range(1, L - 1)]
        smallest[m] = (min(asserted), SC.distance(s.dtype, mb[L - 1], gb[L - 1]) / bar)
        assert min(asserted) >= 2.0, (sid, m, asserted)
    print(sid, "B", B, "hid_omit", s.hid_omit, "smallest distance / bar (asserted tensors, output bias):",
          {m: "%.1f, %.2f" % v for m, v in smallest.items()})


# ------------------------------------------------------------------ 3. the figures of a GPU run
def test_committed_numbers_hold_a_figure_below_its_bar_for_every_new_test():
    """profiles/switch_parity_numbers.json: `python tests/switch_cases.py numbers <parity JSON>` behind a -m gpu run."""
    num = json.load(open(NUMBERS))
    for t in SC.new_tests():
        fig = SC.figure(num["tests"].get(t))
        assert fig is not None, "no measured figure for %s" % t
        text, value, bar = fig
        assert num["figures"][t] == text
        assert np.isfinite(value) and (value < bar or value == bar == 0), (t, text)
