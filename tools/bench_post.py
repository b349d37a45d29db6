"""Time of bp_eval_mix with post-processing of the LPS estimate on (bp_set_post: GV equalisation and the mask gate, fused into the
synthesis) against the same call with it off, in the setting of tools/bench_eval.py: 100 clean sentences of 6 s at 8 kHz, 4 noise
recordings of 60 s, the multi-objective net 1548-2048x3-258 ([LPS | mask], logistic mask block), bunch 256.  The two calls alternate
in one process, each timed to its synchronisation; median of --reps and the spread (min .. max) of each.  One bp_gv_mix over the same
plan is timed beside them, and the factors it gives are the ones the "on" calls run with.  One JSON line; --out also writes it to a
file.

    python tools/bench_post.py [--reps 10] [--compute fp32|bf16] [--out profiles/post_bench.json]
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
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    D, ctx, toff, rate, B = 129, 11, 5, 8000, 256
    ls = [(ctx + 1) * D, 2048, 2048, 2048, 2 * D]
    W, b = dnnse_amd.glorot_net(ls, seed=1, beta=0.5)
    rng = np.random.default_rng(0)
    n = 6 * rate
    clean = [np.round(rng.normal(0, 3000, n)).astype(np.float32) for _ in range(a.sentences)]
    noise = [np.round(rng.normal(0, 2000, 60 * rate)).astype(np.float32) for _ in range(4)]
    frames = a.sentences * ((n - 1) // (D - 1) + 2)
    mean, istd = np.full(D, 10.0, np.float32), np.full(D, 0.25, np.float32)
    g = dnnse_amd.BP_GPU(1, len(ls), ls, B, 0.0, 0.0, 0.0, W, b, max_chunk_frames=frames + a.sentences * (ctx - 1),
                         compute_dtype=1 if a.compute == "bf16" else 0, output_activation=1, output_linear_cols=D)
    g.set_mix_corpus(clean, noise, mean, istd, ctx, toff, "lps+ibm")
    plan = dnnse_amd.mix_plan(0, a.sentences, 1, [x.size for x in noise], [-5, 0, 5, 10, 15, 20])
    g.gv_mix(plan)                                                 # warm-up: the part-sum block, code objects
    t0 = time.perf_counter()
    st = g.gv_mix(plan)
    t_gv = time.perf_counter() - t0
    center, scale = dnnse_amd.gv_factors(st, "indep")
    t_off, t_on = [], []
    for r in range(a.reps + 1):                                    # (rep 0: warm-up -- buffers, code objects)
        g.set_post(None)
        t0 = time.perf_counter()
        off = g.eval_mix(plan, rate)
        t1 = time.perf_counter()
        g.set_post(gv_center=center, gv_scale=scale, mask_col=D, mask_lo=0.3, mask_hi=0.7, mask_weight=0.5)
        t2 = time.perf_counter()
        on = g.eval_mix(plan, rate)
        t3 = time.perf_counter()
        if r:
            t_off.append(t1 - t0)
            t_on.append(t3 - t2)
    g.close()
    ms = lambda v: 1e3 * float(v)
    res = {"what": "bp_eval_mix with bp_set_post on vs off", "compute": a.compute, "mixtures": a.sentences, "frames": frames,
           "off_ms_median": ms(np.median(t_off)), "off_ms_min": ms(min(t_off)), "off_ms_max": ms(max(t_off)),
           "on_ms_median": ms(np.median(t_on)), "on_ms_min": ms(min(t_on)), "on_ms_max": ms(max(t_on)),
           "on_over_off": float(np.median(t_on) / np.median(t_off)), "gv_mix_ms": ms(t_gv), "gv_scale": float(scale[0]),
           "enhanced_mean_off": np.nanmean(off["enhanced"], axis=0).tolist(), "enhanced_mean_on": np.nanmean(on["enhanced"], axis=0).tolist()}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
