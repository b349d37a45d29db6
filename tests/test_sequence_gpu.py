"""One handle held to fresh replays over the walks of the families WALK and EXTENDED of tests/sequence_model.py (-m gpu; the body of
both tests is walk_harness.walk_test).  Every comparison is between two runs of the same library and is bit for bit; there is no
tolerance in this file.

Per walk three long-lived handles take part, all made from the same weights and seed:
  S   the subject: the whole walk, no read beyond the walk's own (pass 1)
  R   the replay: the training kinds and the checkpoints of the walk alone; W, b, dW, db of S equal R's as uint32 at every
      checkpoint and at the end.  (A train_resident of S that trains on the chunk a QUERY left with targets -- mix_features, the
      gradient upload -- makes R load that chunk first.)
  S2  a second subject on the same walk (pass 2) that reads its weights before each query: a fresh handle F is made from them
      with the model's switches and the corpus, makes only that call, and every array it returns equals what S returned in pass 1;
      so does what S2 itself returns.  For the gradient query F is first brought to S's position of the dropout stream by bunches
      at lrate = momentum = weightcost = 0 (they leave the weights as they were, which is checked).  For grads_resident, the gradient
      of whatever is resident, F is also given the chunk of the call that made it resident on S (walk_harness.load).
Every expected error is a host-side check: its status and a non-empty message are checked on S and S2, and the checkpoints behind it
still equal R, which never made the call."""
import pytest

import sequence_model as SM
import walk_harness as H

pytestmark = pytest.mark.gpu

PARAMS = [(c.id, w) for c in SM.WALK.configs for w in SM.walk_ids(SM.WALK, c)]
_make, _state, _differing = H.make, H.state, H.differing


@pytest.mark.parametrize("cid,wid", PARAMS, ids=["%s-%s" % p for p in PARAMS])
def test_walk(pkg, parity_record, cid, wid):
    H.walk_test(pkg, parity_record, SM.WALK, cid, wid)


XPARAMS = [(c.id, w) for c in SM.EXTENDED.configs for w in SM.walk_ids(SM.EXTENDED, c)]


@pytest.mark.parametrize("cid,wid", XPARAMS, ids=["%s-%s" % p for p in XPARAMS])
def test_extended_walk(pkg, parity_record, cid, wid):
    """The same procedure over the whole of sequence_model.KINDS: the noise-aware mode and post-processing as switches, bp_gv_mix and the
    log-MMSE evaluation among the queries, every score width, bp_time_kernel and bp_profile_step between the training calls, and
    configuration D (four layers, MFCC columns, reverberated corpus entries).  bp_profile_step is replayed as the bunch of
    bp_train_resident it is said to be; bp_time_kernel and set_post are left out of the replay."""
    H.walk_test(pkg, parity_record, SM.EXTENDED, cid, wid)


def test_calls_that_need_targets_refuse_a_stacked_chunk_without_them(pkg):
    """Host-side checks, none reaches the device: after forward(x) and after CrossValid the stacked target buffer holds an OLDER
    chunk's rows, and bp_grads_resident, bp_train_resident_masked, bp_profile_step and bp_train_resident return BP_ERR_STATE (the
    walks run only the first and the last).  Behind each refusal the handle trains like one that never made the calls."""
    cfg = SM.BY_ID["A"]
    cor, B = SM.corpus(SM.WALK, cfg), cfg.B
    W0, b0 = pkg.glorot_net(cfg.ls, seed=5, beta=0.5)
    a, ref = (_make(pkg, cfg, W0, b0, SM.fresh_state(), cor) for _ in range(2))
    d0, d1, d2 = (SM.call_data(SM.WALK, cfg, 9, p, "train") for p in range(3))
    masks = [None] * (len(cfg.ls) - 1)
    try:
        for g in (a, ref):
            g.train(d0["x"].shape[0], d0["x"], d0["t"])
            g.train(d1["x"].shape[0], d1["x"], d1["t"])
        for query in (lambda: a.forward(d2["x"]), lambda: a.CrossValid(d2["x"].shape[0], d2["x"], d2["t"])):
            query()
            for call in (lambda: a.grads_resident(0), lambda: a.train_resident_masked(0, B, masks), lambda: a.profile_step(0, 1),
                         lambda: a.train_resident(0, B)):
                with pytest.raises(pkg.BPError, match=r"without targets.*\(status -3\)"):
                    call()
        # the legal side: the same rows with their targets
        a.upload_chunk(d2["x"], d2["t"])
        ref.upload_chunk(d2["x"], d2["t"])
        for g in (a, ref):
            g.grads_resident(0)
            g.train_resident_masked(0, B, masks)
            g.profile_step(B, 1)
            g.train_resident(0, B)
        assert _differing(_state(a), _state(ref), "after the refusals") == 0
        ga, gr = a.read_grads(), ref.read_grads()
        assert _differing(ga[0][1:] + ga[1][1:], gr[0][1:] + gr[1][1:], "gradients") == 0
    finally:
        a.close()
        ref.close()
