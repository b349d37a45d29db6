"""One handle held to fresh replays across calls of CHANGING size: the walks of the family SIZE of tests/size_model.py (-m gpu).  The
procedure is that of tests/test_sequence_gpu.py (tests/walk_harness.py, walk_test: the subject S, the replay R of the training calls, a
fresh handle per query), every comparison is between two runs of the same library and bit for bit (uint32 words), so there is no
tolerance in this file.

What only exists with sizes:
  * a handle of capacity 1024 is regrown and shrunk along the walk (size_model.BUFFERS says which buffers and when), while every
    fresh handle allocates for its one call;
  * the queries at L and FULL are dyed with NaN: what a smaller call behind them returns is compared with a fresh handle that never
    saw a NaN, and the weights at the end of the walk must be finite;
  * a training call of size Z trains nothing: the replay leaves it out, so a word or a position of the dropout stream that it moved
    shows in the next training call and at the end of the walk, and on the second pass W, b, dW, db are read on both sides of it;
  * a call of CAP + 1 rows returns BP_ERR_ARG with a message that names the capacity, and the call behind it matches a fresh handle.
Per configuration: the closed walk of every family in pieces (every ordered pair of the family's (kind, size) nodes once), OVER once
behind every other size of its kind, and four seeded random walks over all nodes."""
import pytest

import sequence_model as SM
import size_model as ZM
import walk_harness as H

pytestmark = pytest.mark.gpu

PARAMS = [(c.id, w) for c in ZM.SIZE.configs for w in SM.walk_ids(ZM.SIZE, c)]


@pytest.mark.parametrize("cid,wid", PARAMS, ids=["%s-%s" % p for p in PARAMS])
def test_size_walk(pkg, parity_record, cid, wid):
    H.walk_test(pkg, parity_record, ZM.SIZE, cid, wid)
