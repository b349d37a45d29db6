"""One rank of the data-parallel LIFE of a handle: attach, train, change the hyper-parameters, train, read the momentum state,
detach, read it again, attach again over another transport, train, read, detach.  Spawned by tests/test_dp_life_gpu.py, one process
per rank; the ranks share one device.

    python tests/dp_life_worker.py <case.json> <rank> <outdir>

case["mode"]: "life" (the whole life), "once" (attach once, the same training calls and the same preset change) or "blind" (the life
up to the read after the detach, WITHOUT the collective read before it: that read leaves the gathered state in the local arena, and
the detach has to produce it by itself)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

from dp_worker import case_data, shard_rows   # noqa: E402

TRANSPORT_NATIVE, TRANSPORT_PUSH = 0, 2


def main():
    c = json.load(open(sys.argv[1]))
    rank, outdir = int(sys.argv[2]), sys.argv[3]
    import dnnse_amd
    ls, B, world, life, blind = c["ls"], c["B"], c["world"], c["mode"] == "life", c["mode"] == "blind"
    W, b, x, t = case_data(c)
    g = dnnse_amd.BP_GPU(world, len(ls), ls, B, c["lr"], c["m"], c["wc"], W, b, device=0, global_bunchsize=B * world,
                         rank_frame_offset=rank * B, max_chunk_frames=max(4 * B, 64), activation=c["act"], momentum_rule=c["rule"],
                         dropoutflag=1, visible_omit=0.1, hid_omit=0.2, seed=99)
    idx = shard_rows(x.shape[0], B * world, world, rank)        # this rank's rows of every global bunch, bunch after bunch

    def train(first_bunch, n_bunches):
        rows = idx[first_bunch * B:(first_bunch + n_bunches) * B]
        g.train(rows.size, x[rows], t[rows])

    out = {}

    def keep(tag, pair):
        for l in range(1, len(ls)):
            out["%s_W%d" % (tag, l)], out["%s_b%d" % (tag, l)] = pair[0][l], pair[1][l]

    g.dp_attach(world, rank, c["key"], transport=TRANSPORT_NATIVE)
    train(0, 2)
    g.lrate, g.momentum = c["lr"] * 0.5, 0.5                    # the same on every rank; train() pushes them
    train(2, 2)
    if blind:
        g.dp_detach()
        keep("D2", g.get_deltas())
        np.savez(os.path.join(outdir, "rank%d.npz" % rank), **out)
        g.close()
        return
    keep("D1", g.get_deltas())                                  # collective: gathers the sharded momentum state
    if life:
        g.dp_detach()
        keep("D2", g.get_deltas())                              # local: what the detached handle holds
        g.dp_attach(world, rank, c["key"] + "-again", transport=TRANSPORT_PUSH)
    train(4, 2)
    keep("end", g.get_weights())
    keep("endD", g.get_deltas())
    out["epochs"] = np.int64(g.dp_info()[2])
    np.savez(os.path.join(outdir, "rank%d.npz" % rank), **out)
    g.dp_detach()
    g.close()


if __name__ == "__main__":
    main()
