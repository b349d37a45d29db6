"""One rank of a data-parallel run with the logistic output layer (bp_set_output), spawned by tests/test_output_act_gpu.py, one
process per rank on one device, native transport.

    python tests/output_act_dp_worker.py <case.json> <rank> <outdir>
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")


def case_data(c):
    """Weights, inputs and [linear | binary mask] targets every rank and the checking test derive identically."""
    import dnnse_amd
    ls, lin = c["ls"], c["lin"]
    W, b = dnnse_amd.glorot_net(ls, seed=5, beta=1.0)
    rng = np.random.default_rng(17)
    b = [None] + [rng.normal(size=ls[l]).astype(np.float32) * 0.1 for l in range(1, len(ls))]
    n = c["nb"] * c["B"] * c["world"]
    x = rng.normal(size=(n, ls[0])).astype(np.float32)
    t = np.empty((n, ls[-1]), np.float32)
    t[:, :lin] = rng.normal(size=(n, lin))
    t[:, lin:] = rng.random((n, ls[-1] - lin)) < 0.4
    return W, b, x, t


def shard_rows(n_frames, global_bunch, world, rank):
    lb = global_bunch // world
    nb = n_frames // global_bunch
    return (np.arange(nb)[:, None] * global_bunch + rank * lb + np.arange(lb)[None, :]).reshape(-1)


def main():
    c = json.load(open(sys.argv[1]))
    rank, outdir = int(sys.argv[2]), sys.argv[3]
    import dnnse_amd
    ls, B, world = c["ls"], c["B"], c["world"]
    W, b, x, t = case_data(c)
    g = dnnse_amd.BP_GPU(world, len(ls), ls, B, 0.5, 0.5, 0.0, W, b, activation=1, device=0, global_bunchsize=B * world,
                         rank_frame_offset=rank * B, max_chunk_frames=c["nb"] * B, output_activation=1, output_linear_cols=c["lin"])
    g.dp_attach(world, rank, c["key"], transport=0)
    idx = shard_rows(x.shape[0], B * world, world, rank)
    g.train(idx.size, x[idx], t[idx])
    w, bb = g.get_weights()
    out = {}
    for l in range(1, len(ls)):
        out["W%d" % l], out["b%d" % l] = w[l], bb[l]
    np.savez(os.path.join(outdir, "rank%d.npz" % rank), **out)
    g.dp_detach()
    g.close()


if __name__ == "__main__":
    main()
