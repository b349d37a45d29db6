"""Time of bp_set_mix_reverb (the reverberant entries of the mixing corpus, made on the device by bp_mix_reverb_fir) beside one
bp_train_mix over the same sentences, so that a reader sees what reverberation adds to an epoch.  The workload: 200 clean
sentences of 4 s at 8 kHz, room impulse responses of 500, 2000 and 4000 taps (direct path at tap 40, exponential tail) paired by
bp_mix_reverb_pairs, target early (50 ms = 400 taps): both signals are made.  The FMA count is that of the definition: one
double FMA per tap and output sample whose source sample lies inside the sentence.  bp_train_mix runs on the derived entries, on
the shipped enhancement net (1548-2048x3-129), bunch 256, dropout on.  The two calls alternate, each timed to its
synchronisation; medians.  One JSON line.

    python tools/bench_reverb.py [--reps 7] [--compute fp32|bf16] [--target early|reverberant]
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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--compute", default="fp32", choices=["fp32", "bf16"])
    ap.add_argument("--target", default="early", choices=["early", "reverberant"])
    ap.add_argument("--sentences", type=int, default=200)
    a = ap.parse_args()
    D, ctx, toff, rate, B, d = 129, 11, 5, 8000, 256, 40
    ls = [(ctx + 1) * D, 2048, 2048, 2048, D]
    W, b = dnnse_amd.glorot_net(ls, seed=1, beta=0.5)
    rng = np.random.default_rng(0)
    n = 4 * rate
    clean = [np.round(rng.normal(0, 3000, n)).astype(np.float32) for _ in range(a.sentences)]
    noise = [np.round(rng.normal(0, 2000, 60 * rate)).astype(np.float32) for _ in range(4)]
    rirs = []
    for Lh in (500, 2000, 4000):
        h = (rng.normal(0, 0.1, Lh) * np.exp(-np.arange(Lh) / (Lh / 6.0))).astype(np.float32)
        h[:d] = 0.0
        h[d] = 1.0
        rirs.append(h)
    pair_rir = dnnse_amd.mix_reverb_pairs(0, a.sentences, len(rirs))
    j = [np.arange(h.size) for h in rirs]
    fma_of = [int(np.maximum(0, n - np.abs(d - jj)).sum()) for jj in j]          # terms with 0 <= i + d - j < n
    fma = sum(fma_of[k] for k in pair_rir)
    frames = a.sentences * ((n - 1) // (D - 1) + 2)
    g = dnnse_amd.BP_GPU(1, len(ls), ls, B, 0.001, 0.5, 0.0, W, b, dropoutflag=1, visible_omit=0.1, hid_omit=0.2,
                         max_chunk_frames=frames + a.sentences * (ctx - 1), compute_dtype=1 if a.compute == "bf16" else 0)
    g.set_mix_corpus(clean, noise, np.full(D, 10.0, np.float32), np.full(D, 0.25, np.float32), ctx, toff, "lps")
    pc = np.arange(a.sentences)
    t_rev, t_mix = [], []
    for r in range(a.reps + 1):                                    # (rep 0: warm-up -- buffers, code objects)
        plan = dnnse_amd.mix_plan(r, a.sentences, 1, [x.size for x in noise], [-5, 0, 5, 10, 15, 20])
        plan["clean"] += a.sentences
        order = dnnse_amd.mix_shuffle(r, 0, frames)
        g.sync()
        t0 = time.perf_counter()
        g.set_mix_reverb(rirs, pc, pair_rir, a.target, 50 * rate // 1000)      # (returns synchronised)
        t1 = time.perf_counter()
        g.train_mix(plan, order)
        g.sync()
        t2 = time.perf_counter()
        if r:
            t_rev.append(t1 - t0)
            t_mix.append(t2 - t1)
    g.close()
    rv, m = float(np.median(t_rev)), float(np.median(t_mix))
    print(json.dumps({"what": "bp_set_mix_reverb beside bp_train_mix", "compute": a.compute, "target": a.target, "sentences": a.sentences,
                      "samples": a.sentences * n, "taps": [int(h.size) for h in rirs],
                      "pairs_per_response": np.bincount(pair_rir, minlength=len(rirs)).tolist(), "fma": fma,
                      "reverb_ms_median": 1e3 * rv, "reverb_gfma_per_s": 1e-9 * fma / rv, "frames": frames,
                      "train_mix_ms_median": 1e3 * m, "reverb_over_train_mix": rv / m}))


if __name__ == "__main__":
    main()
