"""The constructions of tests/bf16_iso.py, proved on the CPU (no GPU): with the numpy model of the bf16 step standing in for the
device, (1) every observation IS the hidden tensor it claims to show, in two summation orders, and the model sits inside every
bar; (2) wrong kernels miss the bars; (3) the data can show a defect; (4) every bf16 GEMM-family kernel the dispatch matrix reaches
is the kernel under test of an isolation case, by name and at the stated layer; (5) the committed figures of the GPU run hold a
ratio of at most 1 for every GPU test."""
import json
import os

import numpy as np
import pytest

import bf16_iso as I
import dispatch_cases as DC
import dispatch_np as D

NUMBERS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bf16_iso_parity_numbers.json")
# ascending k in slabs of 1 (the k-chain) where the net is small, of 8 elsewhere (the chain over a 2048 x 2048 product is minutes of
# numpy; the constructions do not depend on the order at all, which is what the second, very different order is there to show);
# and descending 16-wide blocks
SMALL = lambda c: max(c.ls) <= 200 and c.B <= 200
ORDERS = [("ascending", lambda c: (1 if SMALL(c) else 8, False)), ("reversed 16-wide blocks", lambda c: (16, True))]


# ------------------------------------------------------------------ 1. soundness, 3. the data
@pytest.mark.parametrize("cid", [c.id for c in I.CASES])
def test_observations_are_the_hidden_tensors_and_the_data_can_show_a_defect(cid):
    c, p = I.BY_ID[cid], I.problem(cid)
    for order, args in ORDERS:
        keep = []
        res = I.run_case(c, I.model_factory(*args(c), keep=keep))
        assert res.claims or c.family == "U"
        for name, arr in res.claims:                                   # bit for bit: what the test reads is the hidden tensor
            assert np.array_equal(np.asarray(arr, np.float32), keep[0].hidden[name]), (cid, order, name)
        over = {k: v for k, v in res.ratios().items() if not v <= 1.0}
        assert not over, (cid, order, "the unmutated model misses a bar", over)
    fig = res.figures
    if c.family in I.HALF_ULP_FAMILIES:
        assert fig["slack_share"] >= 0.95, (cid, fig)                 # slack < 1/4 of the half ulp
    if "relu_live" in fig and c.act == 0:
        assert 0.25 <= fig["relu_live"] <= 0.75, (cid, fig)
    assert fig.get("dead_blocks", 0) == 0, (cid, fig)
    if "tie_distance" in fig:
        assert fig["tie_distance"] >= 2.0 ** 8, (cid, fig)
    a, b = I.smallest_operands(c, p)
    assert a >= 2.0 ** -20 and b >= 2.0 ** -20 and a * b >= 2.0 ** -20, (cid, a, b)
    print(cid, fig)


def test_family_c_holds_every_kind_of_input():
    p = I.problem("C_convert")
    u = p.x.view(np.uint32)
    assert (p.kind == 1).sum() > 100 and (p.kind == 2).sum() > 100
    assert ((u[p.kind == 1] & 0x1FFFF) == 0x08000).all() and ((u[p.kind == 2] & 0x1FFFF) == 0x18000).all()
    assert (u == 0x7F7F7FFF).any() and (u == 0x7F7F0000).any() and (u == 0).any() and np.isfinite(I.bf16_round(p.x)).all() and (p.x >= 0).all()


# ------------------------------------------------------------------ 2. the bars see wrong kernels
def _mutant_cases(family):
    """The smallest cases of the family: one per epilogue form."""
    return [c for c in I.CASES if c.family == family and I.D.pad64(c.B) <= 128 and max(c.ls) <= 200]


@pytest.mark.parametrize("mutant,family", [(m, f) for m, fams in I.MUTANTS.items() for f in fams])
def test_a_wrong_kernel_misses_the_bar(mutant, family):
    cases = _mutant_cases(family)
    assert cases
    for c in cases:
        res = I.run_case(c, I.model_factory(16, True, mutant=mutant))
        main = res.checks[0]
        worst, q = I.ratio_of(main)
        share = I.share_over(main)
        print(mutant, c.id, main.name, "error / bar %.3g, %.1f %% of the live elements over" % (worst, 100 * share))
        assert worst > 1.0, (mutant, c.id)
        if mutant == "truncating_store":
            assert share >= 0.25, (c.id, share)
        if mutant == "ties_away_from_zero":                            # every tie with an even lower neighbour goes the other way
            kind = I.problem(c.id).kind
            assert (q[kind == 1] > 1.0).all() and not (q[kind != 1] > 1.0).any(), c.id
        if mutant == "k_slab_dropped":                                 # one 16-wide slab of the reduction is a visible share of every element
            assert share >= 0.9, (c.id, share)


# ------------------------------------------------------------------ 4. coverage, no allowlist
def test_every_bf16_kernel_of_the_dispatch_matrix_is_under_test_by_name():
    reached = set()
    for c in DC.CASES:
        if c.dtype == 1:
            reached |= set(k for k in D.case_kernels(c.ls, c.B, 1, 1 if c.out else 0)
                           if D.family(k) in ("bp_gemm_bf16", "bp_wgrad_dma_bf16_six", "bp_wgrad_dma_bf16_store"))
    assert len(reached) >= 30
    under_test = {}
    for c in I.CASES:
        if c.family == "C":
            continue
        assert I.launch_at(c) == c.kernel, (c.id, "dispatch puts", I.launch_at(c), "at layer %d" % c.layer)
        call = {"U": "step", "W": "grads", "D": "grads", "E": "grads", "T": "grads"}.get(c.family, "forward")
        assert c.kernel in D.kernels(c.ls, c.B, 1, 1 if c.out else 0, call), (c.id, call)
        fam = D.family(c.kernel)
        if fam == "bp_gemm_bf16":
            epi = int(c.kernel[c.kernel.index("<") + 1:].split(",")[0])
            assert epi in I.FAMILY_EPI[c.family], (c.id, c.kernel)
        else:
            assert (fam, c.family) in (("bp_wgrad_dma_bf16_six", "U"), ("bp_wgrad_dma_bf16_store", "W")), (c.id, c.kernel)
        under_test.setdefault(c.kernel, []).append(c.id)
    missing = sorted(reached - set(under_test))
    assert not missing, ("no isolation case has these as its kernel under test", missing)
    # the transposed copy and the delta store ride on the same launches: every hidden forward has a T case, every output forward an E case
    for k, ids in under_test.items():
        fams = set(I.BY_ID[i].family for i in ids)
        assert fams in ({"F", "T"}, {"O", "E"}, {"D"}, {"W"}, {"U"}), (k, ids)


def test_depth_and_raggedness():
    for c in I.CASES:
        if "true, 1>" in c.kernel and c.family != "C" and D.family(c.kernel) == "bp_gemm_bf16":        # LDS-DMA form: the ring of 4 wraps
            k = D.pad64(c.ls[0]) if c.family in ("F", "T") else D.pad64(c.ls[2])
            assert k >= 512, (c.id, k)
    for epi in range(6):
        ragged = [c for c in I.CASES if c.kernel.startswith("void bp_gemm_bf16<%d, 32," % epi) and all(v % 64 for v in c.ls) and c.B % 32]
        assert ragged, ("no 32-row case of epilogue %d ends inside a tile" % epi)


# ------------------------------------------------------------------ 5. the committed figures
def test_committed_numbers_hold_every_ratio_below_one_for_every_gpu_test():
    """profiles/bf16_iso_parity_numbers.json: `python tests/bf16_iso.py numbers <parity JSON>` behind a -m gpu run."""
    num = json.load(open(NUMBERS))["tests"]
    for c in I.CASES:
        e = num.get(I.GPU_TEST % c.id)
        assert e is not None, "no measured figures for %s" % (I.GPU_TEST % c.id)
        assert e["kernel"] == c.kernel, c.id
        assert e["error_over_bar"], c.id
        for name, r in e["error_over_bar"].items():
            assert np.isfinite(r) and 0.0 <= r <= 1.0, (c.id, name, r)
