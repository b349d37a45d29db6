"""One handle held to fresh replays across calls of CHANGING size, over the whole table: the walks of the family XSIZE of
tests/size_model.py (-m gpu).  The procedure is tests/walk_harness.py's (walk_test: the subject S, the replay R of the training calls,
a fresh handle per query), every comparison is between two runs of the same library and bit for bit (uint32 words; the double sums of
gv_mix as uint64), so there is no tolerance in this file.

What tests/test_size_gpu.py does not reach, per configuration A, B, C and D on a handle of capacity 1024:
  * `ev`: every ordered pair of (kind, size) over eval_mix, gv_mix, eval_mix_logmmse and mix_features -- the one wave_grow list of
    eval_mix_run asked three ways (gv_mix: 0 bytes of ev_syn, ev_ola, lps; the log-MMSE call alone sizes ev_gain and reserves no
    out_chunk), with the score width 3 / 5 / 7, the GV stage and the tracker by position;
  * `nat`: every ordered pair of (kind, size, noise-aware mode) over the kinds that read the mode at Z, M and L, a set_nat in front
    of every call whose mode is not the handle's: the noise-aware rows regrown in dynamic mode behind a static call and the
    reverse, a small dynamic call in the remains of a large NaN-dyed one, the spectrum behind the rows of a call that keeps none
    at an offset that moves with the frames;
  * `xover`: CAP + 1 rows in dynamic mode (and of the two new sized kinds in static mode) behind every other size of the kind;
    `xfull`: ONE and FULL in dynamic mode against Z in the other mode;
  * `xmeasure<size>`: bp_time_kernel behind a stacked chunk and bp_profile_step behind a window chunk of every size, each in front
    of every training kind, and a query at L behind a timing run;
  * four seeded random walks over all nodes of the extended table.
The refusals the model predicts (CAP + 1 rows, a mask target under post-processing, the measurement calls on a bf16 handle or
behind a chunk of fewer rows than a bunch) are host-side checks; none of them touches the device."""
import pytest

import sequence_model as SM
import size_model as ZM
import walk_harness as H

pytestmark = pytest.mark.gpu

PARAMS = [(c.id, w) for c in ZM.XSIZE.configs for w in SM.walk_ids(ZM.XSIZE, c)]


@pytest.mark.parametrize("cid,wid", PARAMS, ids=["%s-%s" % p for p in PARAMS])
def test_xsize_walk(pkg, parity_record, cid, wid):
    H.walk_test(pkg, parity_record, ZM.XSIZE, cid, wid)
