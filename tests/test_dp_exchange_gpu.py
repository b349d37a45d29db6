"""The data-parallel exchange held to the ranks' OWN stored gradients (-m gpu): bp_dp_push<GBF16>, bp_dp_reduce_update<WORLD, GBF16>,
the weights | biases boundary w_end and the slicing of bp_dp_attach_ex, for every run of tests/dp_exchange_np.py's table (which says
which feature of that code each run reaches; tests/test_dp_exchange_host.py shows that no reachable cell is empty and that the bars
below separate the right exchange from seven wrong ones and the right update from five).

Rank processes come from test_dp_native.run_case with tests/dp_worker.py in its "exchange" mode: two training calls of exactly one
global minibatch each, and after each call the rank's own read_grads(), get_weights() and the collective get_deltas().

  replication   every rank reports the same bits for W, b, dW, db after both calls, and ran 2 minibatches
  hand-off      every rank's dp_handoff is the one the restatement claims
  step one      from zero momentum with weight cost 0 and c1 = 1: dW, db == -(s / float32(Bg)) and W1 == W0 + D1 as float32 WORDS, s the
                restated sum ((G_0 + G_1) + ...) + G_{world-1} of the ranks' gradients, each rounded to bf16 first under transport 3.
                Worlds 1, 2, 4 (Bg a power of two: the division is exact): 0 unequal words.  World 3 (Bg = 96): held at 1 ulp, the
                count of unequal words and the largest distance recorded -- the module's figures say whether the device divides as IEEE does
  step two      under hyper set A or B of update_cases: update_cases.restate in float64 from the device's (W1, b1, D1, d1) and the
                restated sum of the second gradients against (D2, d2, W2, b2), bar update_cases.BAR = 1e-5 of max|expected| per tensor
  transports    0 and 2 of one case agree bit for bit in everything; 3 differs from 2 in at least one word of step one

A rank that ends with the library's timeout message fails its run with that message; nothing retries it."""
import hashlib
import time

import numpy as np
import pytest

import dp_exchange_np as X
import update_cases as UC
from test_dp_native import run_case

pytestmark = pytest.mark.gpu
STATE = ("W", "b", "dW", "db")
_DONE = {}          # (case id, transport) -> what the cross-transport checks need of rank 0


def _neq(a, b):
    """Unequal float32 words; the two zeros are one number (0 - 0 is +0 where -(0) is -0)."""
    return int(np.count_nonzero(np.asarray(a, np.float32).reshape(-1) != np.asarray(b, np.float32).reshape(-1)))


def _spawn(c, transport):
    h = UC.hyper(c.hset, c.dtype)
    extra = X.worker_case(c, transport, h, None)
    for k in ("ls", "B", "world", "nb", "key"):
        del extra[k]
    t0 = time.time()
    try:
        wc, (W0, b0, _, _), res = run_case("x-%s-t%d" % (c.id, transport), c.ls, c.B, c.world, 2, extra, timeout=180)
    except AssertionError as e:
        if "timed out" in str(e):
            pytest.fail("%s transport %d: a rank ended with the library's timeout message\n%s" % (c.id, transport, e))
        raise
    return h, W0, b0, res, run_case.last_info, time.time() - t0


def run(c, transport, record=None):
    """One run of the table, checked; made once (a run that failed is not made again for the cross-transport tests)."""
    key = (c.id, transport)
    if key not in _DONE:
        _DONE[key] = {"error": "the run did not end"}
        try:
            _checked(c, transport, record)
        except BaseException as e:
            if "fails" not in _DONE[key]:
                _DONE[key] = {"error": repr(e)[:2000]}
            raise
    if "error" in _DONE[key]:
        pytest.fail("%s transport %d failed in its own test: %s" % (c.id, transport, _DONE[key]["error"]))
    return _DONE[key]


def _checked(c, transport, record):
    h, W0, b0, res, info, seconds = _spawn(c, transport)
    L, Bg, rid = len(c.ls), c.B * c.world, "%s-t%d" % (c.id, transport)
    layers = range(1, L)
    numbers = {"seconds": seconds, "world": c.world, "global_minibatch": Bg, "hyper_set": c.hset, "handoff": info[0]["handoff"]}
    fails = []
    # ---- replication, epochs, hand-off
    names = ["%s%d_%d" % (n, l, k) for n in STATE for l in layers for k in (1, 2)]
    for r in range(c.world):
        assert int(res[r]["epochs"]) == 2, (rid, "rank", r, "ran", int(res[r]["epochs"]), "minibatches")
        assert info[r]["handoff"] == X.handoff(c, transport), (rid, "rank", r, "reports the hand-off", info[r]["handoff"])
        for n in names:
            assert np.array_equal(res[0][n].view(np.uint32), res[r][n].view(np.uint32)), (rid, "rank", r, "differs from rank 0 in", n)
    r0 = res[0]
    # ---- step one: the ordered sum and nothing else, to the bit
    unequal, worst_ulp = {}, 0
    for l in layers:
        for G, D, P, P0 in (("G", "dW", "W", W0[l]), ("g", "db", "b", b0[l])):
            s = X.ordered_sum([res[p]["%s%d_1" % (G, l)] for p in range(c.world)], transport)
            want, got = X.exact_step(s, Bg), r0["%s%d_1" % (D, l)]
            unequal["%s%d" % (D, l)] = _neq(got, want)
            worst_ulp = max(worst_ulp, int(X.ulps(got, want.reshape(got.shape)).max()))
            p1 = (np.asarray(P0, np.float32).reshape(got.shape) + got).astype(np.float32)
            unequal["%s%d" % (P, l)] = _neq(r0["%s%d_1" % (P, l)], p1)
            assert np.abs(got).max() > 0, (rid, D, l, "did not move")
    numbers["step_one"] = {"unequal_words": unequal, "unequal_total": sum(unequal.values()), "largest_ulps": worst_ulp,
                           "words": int(sum(r0["%s%d_1" % (n, l)].size for n in STATE for l in layers))}
    exact_division = Bg & (Bg - 1) == 0
    if exact_division:
        if any(unequal.values()):
            fails.append("step one: unequal words %s (largest distance %d ulps)" % ({k: v for k, v in unequal.items() if v}, worst_ulp))
    else:
        bad = {k: v for k, v in unequal.items() if v and k[0] != "d"}          # W1 = W0 + D1 has no division in it
        if worst_ulp > 1 or bad:
            fails.append("step one at a global minibatch of %d: largest distance %d ulps (bar 1), unequal sums W0 + D1 %s" % (Bg, worst_ulp, bad))
    # ---- step two: every term of the update, restated from the device's own operands
    st = lambda nm, k: [None] + [r0["%s%d_%d" % (nm, l, k)] for l in layers]
    s2w = [None] + [X.ordered_sum([res[p]["G%d_2" % l] for p in range(c.world)], transport) for l in layers]
    s2b = [None] + [X.ordered_sum([res[p]["g%d_2" % l] for p in range(c.world)], transport) for l in layers]
    want = UC.restate(h, Bg, st("W", 1), st("b", 1), st("dW", 1), st("db", 1), s2w, s2b)
    errs, _ = UC.errors((st("dW", 2), st("db", 2), st("W", 2), st("b", 2)), want)
    numbers["step_two"] = {"errors": errs, "worst": max(errs.values()), "bar": UC.BAR, "hyper": h._asdict()}
    for k, v in errs.items():
        if not v < UC.BAR:
            fails.append("step two %s: %.3e (bar %.0e)" % (k, v, UC.BAR))
    print(rid, numbers)
    if record:
        record(**numbers)
    keep = {"hash": {n: hashlib.sha1(np.ascontiguousarray(r0[n]).tobytes()).hexdigest() for n in names},
            "step_one": {n: r0[n] for n in names if n.endswith("_1") and n[0] == "d"}, "fails": fails}
    _DONE[(c.id, transport)] = keep
    assert not fails, (rid, fails)


@pytest.mark.parametrize("c,transport", X.RUNS, ids=X.RUN_IDS)
def test_exchange_on_the_ranks_own_gradients(parity_record, c, transport):
    run(c, transport, parity_record)


NATIVE_CASES = [c for c in X.CASES if (c, X.PUSH) in X.RUNS]


@pytest.mark.parametrize("c", NATIVE_CASES, ids=[c.id for c in NATIVE_CASES])
def test_transports_of_one_case(parity_record, c):
    """Pull and push form sum the same slices in the same order: the same bits in every tensor after both calls.  bf16 gradient
    segments really are a reduced-precision exchange: step one differs from the push form's somewhere."""
    def get(t):
        try:
            return run(c, t)
        except AssertionError:              # (a run that missed a bar has failed in its own test; its arrays still compare)
            if "hash" not in _DONE[(c.id, t)]:
                raise
            return _DONE[(c.id, t)]
    pull, push, bf = get(X.PULL), get(X.PUSH), get(X.PUSH_BF16)
    differ = sorted(n for n in pull["hash"] if pull["hash"][n] != push["hash"][n])
    words = sum(int(np.count_nonzero(push["step_one"][n].view(np.uint32) != bf["step_one"][n].view(np.uint32))) for n in push["step_one"])
    parity_record(pull_vs_push_tensors_that_differ=differ, bf16_segments_vs_push_step_one_words_that_differ=words)
    assert not differ, (c.id, "push form differs from pull form in", differ)
    assert words >= 1, (c.id, "transport 3 gives the bits of transport 2: nothing was rounded to bf16")
