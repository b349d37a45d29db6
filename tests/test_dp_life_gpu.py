"""The data-parallel life of one handle (-m gpu): two ranks sharing the device attach, train, change the hyper-parameters, train,
gather the momentum state, DETACH, read the momentum state again, attach again over the push transport with a new key, train and
detach (tests/dp_life_worker.py).

Under more than one rank the momentum state is sharded: each rank updates its slices and the others go stale.  An explicit
bp_dp_detach gathers them before it unmaps the peers, so what a detached handle returns (D2) is what the collective read returned
just before (D1), bit for bit; the end of the life equals, bit for bit, that of two ranks that attach once and make the same training
calls and the same preset change (push and pull are the same bits, test_native_dp_matches_global_bunch_oracle holds that); and it
is within the strict bar 1e-5 of test_dp_native.py of ONE rank that trains the global bunch.

Three processes hold the device at a time: two ranks and the test's own."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from test_dp_native import HERE, MAX_RANKS
from util import relerr

pytestmark = pytest.mark.gpu

LS, LOCAL_B, WORLD, BUNCHES = [70, 65, 130, 33], 25, 2, 6
STRICT_BAR = 1e-5           # test_dp_native.py: the sharded run against the unsharded run of the same library


def run_life(mode, world, B, timeout=120):
    """The ranks of one run -> one dict of arrays per rank."""
    assert world + 1 <= 3 and world <= MAX_RANKS
    c = dict(ls=LS, B=B, world=world, nb=BUNCHES, mode=mode, key="life%d-%s%d" % (os.getpid(), mode, world),
             lr=1.0, m=0.9, wc=0.0625, act=1, rule=1)
    with tempfile.TemporaryDirectory() as td:
        cj = os.path.join(td, "case.json")
        json.dump(c, open(cj, "w"))
        env = dict(os.environ, BP_DP_TIMEOUT_S="60", HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "dp_life_worker.py"), cj, str(r), td], env=env,
                                  stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(world)]
        outs = []
        for p in procs:
            try:
                o, _ = p.communicate(timeout=timeout)
            except subprocess.TimeoutExpired:
                for q in procs:
                    q.kill()
                for q in procs:                                 # reaped before the failure is reported: nothing keeps the device open
                    q.wait()
                raise
            outs.append(o.decode(errors="replace"))
        for r, p in enumerate(procs):
            assert p.returncode == 0, "rank %d failed:\n%s" % (r, outs[r][-3000:])
        return [dict(np.load(os.path.join(td, "rank%d.npz" % r))) for r in range(world)]


def _words(a, b):
    return int(np.count_nonzero(np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)))


@pytest.fixture(scope="module")
def life():
    return run_life("life", WORLD, LOCAL_B)


@pytest.fixture(scope="module")
def once():
    return run_life("once", WORLD, LOCAL_B)


def test_detached_handle_holds_the_gathered_momentum_state(life, parity_record):
    """D2 (bp_get_deltas after bp_dp_detach, local) == D1 (the collective read before it) on both ranks, and the ranks agree."""
    names = sorted(k for k in life[0] if k.startswith("D1_"))
    assert len(names) == 2 * (len(LS) - 1)
    differing = {r: sum(_words(life[r][k], life[r]["D2_" + k[3:]]) for k in names) for r in range(WORLD)}
    across = sum(_words(life[0][k], life[1][k]) for k in names)
    moved = sum(int(np.count_nonzero(life[0][k])) for k in names)
    parity_record(d2_vs_d1_words_differing=differing, d1_rank0_vs_rank1_words_differing=across, d1_nonzero_words=moved)
    assert moved > 0 and across == 0
    assert differing == {r: 0 for r in range(WORLD)}, "bp_get_deltas after bp_dp_detach differs from the gathered state (rank: words) %s" % differing


def test_detach_gathers_without_a_collective_read_before_it(once, parity_record):
    """In the life above the collective read D1 has itself left the gathered state in each rank's arena, so D2 == D1 holds even
    where the detach gathers nothing.  Here the ranks detach straight after training: what the detached handle returns must still
    be the gathered state, that of two ranks that made the same calls and read it collectively."""
    blind = run_life("blind", WORLD, LOCAL_B)
    names = sorted(k for k in once[0] if k.startswith("D1_"))
    differing = {r: sum(_words(blind[r]["D2_" + k[3:]], once[r][k]) for k in names) for r in range(WORLD)}
    parity_record(detached_vs_collective_read_words_differing=differing)
    assert differing == {r: 0 for r in range(WORLD)}, "bp_dp_detach left stale momentum slices (rank: words) %s" % differing


def test_life_equals_one_attachment_and_one_rank(life, once, parity_record):
    one = run_life("once", 1, LOCAL_B * WORLD)
    end = sorted(k for k in life[0] if k.startswith("end"))
    assert len(end) == 4 * (len(LS) - 1)
    assert int(life[0]["epochs"]) == 2 and int(once[0]["epochs"]) == BUNCHES        # (the second attachment counts its own minibatches)
    ranks = sum(_words(life[0][k], life[1][k]) for k in end)
    vs_once = sum(_words(life[r][k], once[r][k]) for r in range(WORLD) for k in end + sorted(k for k in life[0] if k.startswith("D1_")))
    strict = {k: relerr(life[0][k], one[0][k]) for k in end}
    print("life vs one rank with the global bunch:", {k: "%.1e" % v for k, v in strict.items()})
    parity_record(life_rank0_vs_rank1_words_differing=ranks, life_vs_one_attachment_words_differing=vs_once,
                  life_vs_one_rank_global_bunch=strict, strict_bar=STRICT_BAR)
    assert ranks == 0 and vs_once == 0, (ranks, vs_once)
    for k, v in strict.items():
        assert v < STRICT_BAR, (k, v)
