"""Unaligned rank offsets in every hidden-forward kernel and both staging forms (-m gpu).  One GPU, no group: the handles are shard
handles (bunchsize B, global_bunchsize 2B, rank_frame_offset B -- the second of two ranks) and only grads_resident is called.

drop_words4 (csrc/bp_device.h) draws the dropout words of four consecutive rows from one Philox block when rank_frame_offset is a
multiple of 4 and from two blocks otherwise, in three branches (offset & 3 = 1, 2, 3), with the row and the unit of each tile
layout.  tests/switch_cases.py has the five shapes (one per hidden-forward tile layout) and three bunch sizes each, B = 1, 2, 3
(mod 4); tests/test_switch_coverage.py checks on the CPU that masks drawn at a wrong offset or with row and unit exchanged move
the reference gradient by at least twice the bar.

Reference: oracle.Oracle(...).grads(x, t, masks=[fill_mask(0, l, B, gframe0=B)], scale_frames=2B); the same masks once more from
tests/philox_np.py, asserted equal.  fp32: every hidden layer's output is 0.0 exactly where the mask drops (a Sigmoid is never 0,
so this compares every mask bit) and the gradient meets the one-bunch bar of test_dispatch_gpu.test_gradient_store (1e-5 where the
oracle's spread supports it, else 1e-4).  bf16: 2e-2 rms per tensor.  Window staging: the gradient of a window chunk equals, bit for
bit, that of the same rows uploaded stacked."""
import numpy as np
import pytest

import dispatch_cases as DC
import switch_cases as SC
from util import TOL

pytestmark = pytest.mark.gpu


def _mk(pkg, s, B, W, b, cap):
    return pkg.BP_GPU(2, len(s.ls), s.ls, B, 1.0, 0.5, 0.0, W, b, activation=1, compute_dtype=s.dtype, dropoutflag=1, seed=SC.SHARD_SEED,
                      global_bunchsize=2 * B, rank_frame_offset=B, max_chunk_frames=cap, **SC.shard_drop(s))


@pytest.mark.parametrize("sid,B", SC.SHARD_RUNS, ids=["%s-%d" % r for r in SC.SHARD_RUNS])
def test_shard_gradient_at_an_unaligned_offset(pkg, oracle_mod, parity_record, sid, B):
    s = SC.SHARD_BY_ID[sid]
    L = len(s.ls)
    assert B & 3, "the offset of the shard is its bunch size"
    W, b, x, t, masks, (rw, rb, _) = SC.shard_reference(s, B)
    for l, m in enumerate(SC.shard_masks(s, B)):                     # the third implementation of the keying agrees with the oracle's
        assert np.array_equal(m, masks[l]), ("mask of layer", l)
    g = _mk(pkg, s, B, W, b, cap=B)
    g.upload_chunk(x, t)
    g.grads_resident(0)
    gw, gb = g.read_grads()
    ys = [g.read_layer_output(l) for l in range(1, L - 1)] if s.dtype == 0 else []
    g.close()
    unequal = {}
    for l, y in enumerate(ys, 1):                                    # fp32: every mask bit
        unequal["mask bits of layer %d" % l] = int(((y == 0) != (masks[l] == 1)).sum())
    if s.dtype == 0:
        _, _, _, _, _, (dw, db, _) = SC.shard_reference(s, B, masks=masks, acc_double=True)
        spread = max(SC.distance(0, a[l], d[l]) for l in range(1, L) for a, d in ((rw, dw), (rb, db)))
        bar = 1e-5 if DC.strict_bar(spread) else TOL
    else:
        spread, bar = None, SC.BF16_BAR
    errs = {}
    for l in range(1, L):
        errs["G%d" % l], errs["gb%d" % l] = SC.distance(s.dtype, gw[l], rw[l]), SC.distance(s.dtype, gb[l], rb[l])
    print(sid, B, "offset branch", B & 3, errs, "bar", bar, "oracle spread", spread, unequal)
    parity_record(gradient={"errors": errs, "bar": bar, "oracle_spread_fp32_vs_fp64_accumulation": spread}, masks={"unequal": unequal})
    assert not any(unequal.values()), (sid, B, unequal)
    assert all(v < bar for v in errs.values()), (sid, B, errs, bar)


def test_window_staging_at_an_unaligned_offset(pkg, parity_record):
    """bp_stage_bunch stacks and masks the rows of a window chunk itself (visible dropout on, offset 27 = 3 mod 4): the gradient of
    the chunk's second bunch equals, bit for bit, that of the same rows uploaded stacked (stage_rows_block), which the test above
    holds to the oracle at this shape."""
    sid, B = SC.WINDOW_SHARD
    s = SC.SHARD_BY_ID[sid]
    assert B & 3 == 3
    W, b, _, _ = DC.case_data(SC.shard_case(s, B), 1)
    fea, tg, ctx, ws, tf, rows, trows = SC.window_problem(B)
    got = []
    for windows in (False, True):
        g = _mk(pkg, s, B, W, b, cap=2 * B)
        if windows:
            g.upload_chunk_windows(fea, tg, ctx, ws, tf)
        else:
            g.upload_chunk(rows, trows)
        g.grads_resident(B)
        got.append(g.read_grads(padded=True))
        g.close()
    unequal = {}
    for l in range(1, len(s.ls)):
        unequal["G%d" % l] = int((got[0][0][l] != got[1][0][l]).sum())
        unequal["gb%d" % l] = int((got[0][1][l] != got[1][1][l]).sum())
        assert got[0][0][l].any() and np.isfinite(got[0][0][l]).all()
    print("window against stacked upload, unequal words:", unequal)
    parity_record(window_vs_stacked={"unequal": unequal})
    assert not any(unequal.values()), unequal
