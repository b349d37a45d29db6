"""Frames per second of bp_train_mix (mixtures made on the device, then the training step) against bp_train_resident on the
same resident chunk (the step alone), on the shipped enhancement net (1548-2048x3-129: 11 frames of 129 bins + the noise-aware
block), bunch 256, dropout on.  The chunk: 100 clean sentences of 6 s at 8 kHz, each mixed with one of 4 noise recordings of
60 s: 37 600 frames, 146 full bunches.  The two calls alternate, each timed to its synchronisation.  One JSON line.  Kernel
times come from running it under `rocprofv3 --kernel-trace --stats -- python tools/bench_mix.py` (bp_mix_* and bp_wave_*
against the step's kernels).

    python tools/bench_mix.py [--reps 10] [--compute fp32|bf16]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--compute", default="fp32", choices=["fp32", "bf16"])
    ap.add_argument("--sentences", type=int, default=100)
    a = ap.parse_args()
    D, ctx, toff, rate, B = 129, 11, 5, 8000, 256
    ls = [(ctx + 1) * D, 2048, 2048, 2048, D]
    W, b = dnnse_amd.glorot_net(ls, seed=1, beta=0.5)
    rng = np.random.default_rng(0)
    n = 6 * rate
    clean = [np.round(rng.normal(0, 3000, n)).astype(np.float32) for _ in range(a.sentences)]
    noise = [np.round(rng.normal(0, 2000, 60 * rate)).astype(np.float32) for _ in range(4)]
    frames = a.sentences * ((n - 1) // (D - 1) + 2)
    g = dnnse_amd.BP_GPU(1, len(ls), ls, B, 0.001, 0.5, 0.0, W, b, dropoutflag=1, visible_omit=0.1, hid_omit=0.2,
                         max_chunk_frames=frames + a.sentences * (ctx - 1), compute_dtype=1 if a.compute == "bf16" else 0)
    g.set_mix_corpus(clean, noise, np.full(D, 10.0, np.float32), np.full(D, 0.25, np.float32), ctx, toff, "lps")
    t_mix, t_res = [], []
    for r in range(a.reps + 1):                                    # (rep 0: warm-up -- buffers, code objects)
        plan = dnnse_amd.mix_plan(r, a.sentences, 1, [x.size for x in noise], [-5, 0, 5, 10, 15, 20])
        order = dnnse_amd.mix_shuffle(r, 0, frames)
        t0 = time.perf_counter()
        g.train_mix(plan, order)
        g.sync()
        t1 = time.perf_counter()
        g.train_resident(0, frames)                                # the same chunk, the step alone
        g.sync()
        t2 = time.perf_counter()
        if r:
            t_mix.append(t1 - t0)
            t_res.append(t2 - t1)
    g.close()
    m, s = float(np.median(t_mix)), float(np.median(t_res))
    print(json.dumps({"what": "bp_train_mix vs bp_train_resident", "compute": a.compute, "frames": frames, "bunches": frames // B,
                      "mix_ms_median": 1e3 * m, "resident_ms_median": 1e3 * s, "mix_frames_per_s": frames / m,
                      "resident_frames_per_s": frames / s, "mix_over_resident": m / s}))


if __name__ == "__main__":
    main()
