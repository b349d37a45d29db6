"""Time per CD-1 bunch of the pre-training path (bp_rbm_train_chunk) for the two RBM shapes of the 1548-2048x3-129 net: 1548 -> 2048
(Gaussian visibles, RBM 1) and 2048 -> 2048 (Bernoulli visibles, RBM 2 of the stack 1548-2048-2048, so its bunch includes the
mean-field pass through RBM 1), at bunch 128 and 256.  Beside each: bp_train_resident's time per step of the sigmoid net [V, H, V]
at the same bunch, in the same process, the two alternating.

What is timed: a host clock around a call that ends in a device synchronise.  bp_rbm_train_chunk uploads its rows first (pageable
host memory, --bunches x B x 1548 floats), so `rbm_ms_per_bunch` is the call over its bunches, UPLOAD INCLUDED; bp_train_resident
runs on a chunk already on the device.  Kernel time alone comes from a profiler run of this script (tools/README.md).
`flops_per_bunch` = 10 B V H (two up passes, the down pass, the statistics over 2 B rows) and `pct_of_mfma_peak` sets it against
the 157.3 TF the project uses as the fp32 MFMA peak; for RBM 2 the mean-field pass through RBM 1 adds 2 B 1548 2048 that the figure
does not count.  Rep 0 of every call is a warm-up; median and spread (min .. max) of --reps.  One JSON line per configuration;
--out appends them to a file.

    python tools/bench_rbm.py [--reps 7] [--bunches 100] [--out profiles/rbm_bench.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dnnse_amd  # noqa: E402

PEAK_TF = 157.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--bunches", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sizes = [1548, 2048, 2048]
    rng = np.random.default_rng(0)
    W = [None] + [(0.01 * rng.standard_normal((sizes[l - 1], sizes[l]))).astype(np.float32) for l in (1, 2)]
    c = [None] + [np.zeros(sizes[l], np.float32) for l in (1, 2)]
    lines = []
    for B in (128, 256):
        n = a.bunches * B
        x = rng.standard_normal((n, sizes[0])).astype(np.float32)
        s = dnnse_amd.rbm_open(0, sizes, B, W, c, seed=1, max_chunk_frames=n)
        for layer in (1, 2):
            V, H = sizes[layer - 1], sizes[layer]
            ls = [V, H, V]
            Wn, bn = dnnse_amd.glorot_net(ls, seed=1, beta=0.5)
            g = dnnse_amd.BP_GPU(1, 3, ls, B, 0.01, 0.5, 0.0, Wn, bn, activation=1, max_chunk_frames=n)
            g.fill_chunk_synthetic(n)
            t_rbm, t_step, ev_step = [], [], []
            for r in range(a.reps + 1):
                t0 = time.perf_counter()
                s.train(layer, x)
                t1 = time.perf_counter()
                g.train_resident(0, n)
                g.sync()
                t2 = time.perf_counter()
                if r:
                    t_rbm.append((t1 - t0) / a.bunches)
                    t_step.append((t2 - t1) / a.bunches)
                    ms, nb = g.last_train_ms()
                    ev_step.append(ms / nb)
            g.close()
            flops = 10.0 * B * V * H
            med = float(np.median(t_rbm))
            ms = lambda v: 1e3 * float(v)
            res = {"what": "CD-1 bunch, bp_rbm_train_chunk (upload included) beside bp_train_resident of [V, H, V]", "V": V, "H": H, "bunch": B,
                   "visible": "gaussian" if layer == 1 else "bernoulli", "bunches_per_call": a.bunches, "reps": a.reps,
                   "rbm_ms_per_bunch": ms(med), "rbm_ms_min": ms(min(t_rbm)), "rbm_ms_max": ms(max(t_rbm)),
                   "flops_per_bunch": flops, "rbm_tflops": flops / med / 1e12, "pct_of_mfma_peak": 100.0 * flops / med / 1e12 / PEAK_TF,
                   "step_ms_per_bunch": ms(np.median(t_step)), "step_ms_min": ms(min(t_step)), "step_ms_max": ms(max(t_step)),
                   "step_event_ms_per_bunch": float(np.median(ev_step)), "rbm_over_step": med / float(np.median(t_step))}
            print(json.dumps(res))
            lines.append(res)
        s.close()
    if a.out:
        with open(a.out, "a") as f:
            for res in lines:
                f.write(json.dumps(res, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
