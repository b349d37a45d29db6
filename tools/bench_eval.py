"""Time of bp_eval_mix (mixtures made on the device, enhanced with the net, and the noisy and enhanced sentences scored: SSNR,
LSD, STOI) against bp_enhance_waves on the same mixtures (enhancement alone), in the setting of tools/bench_mix.py: 100 clean
sentences of 6 s at 8 kHz, 4 noise recordings of 60 s, the shipped enhancement net (1548-2048x3-129: 11 frames of 129 bins +
the noise-aware block), bunch 256.  The two calls alternate, each timed to its synchronisation; median of --reps.  One JSON
line.  Kernel times come from running it under `rocprofv3 --kernel-trace --stats -- python tools/bench_eval.py` (bp_eval_*
against the forward's kernels).

--extended: the five-column bp_eval_mix_ext (ESTOI and SI-SDR beside the three) against the three-column bp_eval_mix on the same
mixtures instead: the two alternate in one process, each timed to its synchronisation; both medians and their ratio.

--full: the seven-column bp_eval_mix_ext (LLR and cepstral distance behind the five) against the five-column call on the same
mixtures, alternating in the same way.  The new kernels' share: `rocprofv3 --kernel-trace --stats -- python tools/bench_eval.py
--full` (bp_eval_lpc, bp_eval_lpcrank, bp_eval_lpcsum against the other bp_eval_* kernels).

--all: the nine-column bp_eval_mix_ext (fwSegSNR and WSS behind the seven) against the seven-column call on the same mixtures,
alternating in the same way.  The new kernels' share: `rocprofv3 --kernel-trace --stats -- python tools/bench_eval.py --all`
(bp_eval_cb, bp_eval_cbsum and the second bp_eval_lpcrank against the other bp_eval_* kernels; bp_eval_bands also does one FFT
per frame and signal).

    python tools/bench_eval.py [--reps 10] [--compute fp32|bf16] [--extended | --full | --all]
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
    ap.add_argument("--extended", action="store_true", help="time bp_eval_mix_ext with five columns beside bp_eval_mix")
    ap.add_argument("--full", action="store_true", help="time bp_eval_mix_ext with seven columns beside the five-column call")
    ap.add_argument("--all", action="store_true", help="time bp_eval_mix_ext with nine columns beside the seven-column call")
    a = ap.parse_args()
    D, ctx, toff, rate, B = 129, 11, 5, 8000, 256
    ls = [(ctx + 1) * D, 2048, 2048, 2048, D]
    W, b = dnnse_amd.glorot_net(ls, seed=1, beta=0.5)
    rng = np.random.default_rng(0)
    n = 6 * rate
    clean = [np.round(rng.normal(0, 3000, n)).astype(np.float32) for _ in range(a.sentences)]
    noise = [np.round(rng.normal(0, 2000, 60 * rate)).astype(np.float32) for _ in range(4)]
    frames = a.sentences * ((n - 1) // (D - 1) + 2)
    mean, istd = np.full(D, 10.0, np.float32), np.full(D, 0.25, np.float32)
    g = dnnse_amd.BP_GPU(1, len(ls), ls, B, 0.0, 0.0, 0.0, W, b, max_chunk_frames=frames + a.sentences * (ctx - 1),
                         compute_dtype=1 if a.compute == "bf16" else 0)
    g.set_mix_corpus(clean, noise, mean, istd, ctx, toff, "lps")
    plan = dnnse_amd.mix_plan(0, a.sentences, 1, [x.size for x in noise], [-5, 0, 5, 10, 15, 20])
    mix = np.split(g.mix_features(plan)["pcm"], np.cumsum([x.size for x in clean])[:-1])
    if a.extended:
        t3, t5 = [], []
        for r in range(a.reps + 1):                                # (rep 0: warm-up -- buffers, code objects)
            t0 = time.perf_counter()
            ev3 = g.eval_mix(plan, rate)
            t1 = time.perf_counter()
            ev5 = g.eval_mix(plan, rate, extended=True)
            t2 = time.perf_counter()
            if r:
                t3.append(t1 - t0)
                t5.append(t2 - t1)
        g.close()
        same = all(np.array_equal(ev5[k][:, :3].view(np.uint32), ev3[k].view(np.uint32)) for k in ("noisy", "enhanced"))
        m3, m5 = float(np.median(t3)), float(np.median(t5))
        print(json.dumps({"what": "bp_eval_mix_ext (5 columns) vs bp_eval_mix (3 columns)", "compute": a.compute, "mixtures": a.sentences,
                          "frames": frames, "basic_ms_median": 1e3 * m3, "extended_ms_median": 1e3 * m5, "extended_over_basic": m5 / m3,
                          "columns_0_to_2_same_bits": same, "noisy_mean": np.nanmean(ev5["noisy"], axis=0).tolist(),
                          "enhanced_mean": np.nanmean(ev5["enhanced"], axis=0).tolist()}))
        return
    if a.full:
        t5, t7 = [], []
        for r in range(a.reps + 1):                                # (rep 0: warm-up -- buffers, code objects)
            t0 = time.perf_counter()
            ev5 = g.eval_mix(plan, rate, extended=True)
            t1 = time.perf_counter()
            ev7 = g.eval_mix(plan, rate, extended="full")
            t2 = time.perf_counter()
            if r:
                t5.append(t1 - t0)
                t7.append(t2 - t1)
        g.close()
        same = all(np.array_equal(ev7[k][:, :5].view(np.uint32), ev5[k].view(np.uint32)) for k in ("noisy", "enhanced"))
        m5, m7 = float(np.median(t5)), float(np.median(t7))
        print(json.dumps({"what": "bp_eval_mix_ext (7 columns) vs bp_eval_mix_ext (5 columns)", "compute": a.compute, "mixtures": a.sentences,
                          "frames": frames, "extended_ms_median": 1e3 * m5, "full_ms_median": 1e3 * m7, "full_over_extended": m7 / m5,
                          "columns_0_to_4_same_bits": same, "noisy_mean": np.nanmean(ev7["noisy"], axis=0).tolist(),
                          "enhanced_mean": np.nanmean(ev7["enhanced"], axis=0).tolist()}))
        return
    if a.all:
        t7, t9 = [], []
        for r in range(a.reps + 1):                                # (rep 0: warm-up -- buffers, code objects)
            t0 = time.perf_counter()
            ev7 = g.eval_mix(plan, rate, extended="full")
            t1 = time.perf_counter()
            ev9 = g.eval_mix(plan, rate, extended="all")
            t2 = time.perf_counter()
            if r:
                t7.append(t1 - t0)
                t9.append(t2 - t1)
        g.close()
        same = all(np.array_equal(ev9[k][:, :7].view(np.uint32), ev7[k].view(np.uint32)) for k in ("noisy", "enhanced"))
        m7, m9 = float(np.median(t7)), float(np.median(t9))
        print(json.dumps({"what": "bp_eval_mix_ext (9 columns) vs bp_eval_mix_ext (7 columns)", "compute": a.compute, "mixtures": a.sentences,
                          "frames": frames, "full_ms_median": 1e3 * m7, "all_ms_median": 1e3 * m9, "all_over_full": m9 / m7,
                          "columns_0_to_6_same_bits": same, "noisy_mean": np.nanmean(ev9["noisy"], axis=0).tolist(),
                          "enhanced_mean": np.nanmean(ev9["enhanced"], axis=0).tolist()}))
        return
    t_eval, t_enh = [], []
    for r in range(a.reps + 1):                                    # (rep 0: warm-up -- buffers, code objects)
        t0 = time.perf_counter()
        ev = g.eval_mix(plan, rate)
        t1 = time.perf_counter()
        g.enhance_waves(mix, mean, istd, ctx, toff)                # the same mixtures, enhancement alone
        t2 = time.perf_counter()
        if r:
            t_eval.append(t1 - t0)
            t_enh.append(t2 - t1)
    g.close()
    m, s = float(np.median(t_eval)), float(np.median(t_enh))
    print(json.dumps({"what": "bp_eval_mix vs bp_enhance_waves", "compute": a.compute, "mixtures": a.sentences, "frames": frames,
                      "eval_ms_median": 1e3 * m, "enhance_ms_median": 1e3 * s, "eval_over_enhance": m / s,
                      "noisy_mean": np.nanmean(ev["noisy"], axis=0).tolist(), "enhanced_mean": np.nanmean(ev["enhanced"], axis=0).tolist()}))


if __name__ == "__main__":
    main()
