"""Wall time of the log-MMSE baseline (bp_logmmse_waves, bp_eval_mix_logmmse) against the net's calls on the same audio
(bp_enhance_waves, bp_eval_mix), in the setting of tools/bench_enhance.py and tools/bench_eval.py: 100 sentences of 6 s at 8 kHz,
4 noise recordings of 60 s, the shipped enhancement net (1548-2048x3-129: 11 frames of 129 bins + the noise-aware block), bunch
256.  The four calls alternate, each timed to its synchronisation; median of --reps.  One JSON line.  bp_logmmse_gain's own time
comes from running it under `rocprofv3 --kernel-trace --stats -- python tools/bench_logmmse.py` (against bp_wave_analysis,
bp_wave_synthesis and bp_wave_overlap around it).

--noise spp times the two log-MMSE calls with the MMSE-SPP noise tracker (bp_logmmse_waves_nt, bp_eval_mix_logmmse_nt,
INTEGRATION.md 1n) beside the VAD-gated ones, on the same audio and in the same alternation.

    python tools/bench_logmmse.py [--reps 10] [--compute fp32|bf16] [--noise spp]
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
    ap.add_argument("--noise", default=None, choices=["spp"], help="also time the calls with the noise tracker")
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
    t = {"logmmse_waves": [], "enhance_waves": [], "eval_mix_logmmse": [], "eval_mix": []}
    if a.noise:
        t.update({"logmmse_waves_" + a.noise: [], "eval_mix_logmmse_" + a.noise: []})
    for r in range(a.reps + 1):                                    # (rep 0: warm-up -- buffers, code objects)
        t0 = time.perf_counter()
        dnnse_amd.logmmse_waves(0, D, mix)
        t1 = time.perf_counter()
        g.enhance_waves(mix, mean, istd, ctx, toff)                # the same mixtures through the net
        t2 = time.perf_counter()
        lm = g.eval_mix_logmmse(plan, rate)
        t3 = time.perf_counter()
        ev = g.eval_mix(plan, rate)
        t4 = time.perf_counter()
        dts = [t1 - t0, t2 - t1, t3 - t2, t4 - t3]
        if a.noise:
            dnnse_amd.logmmse_waves(0, D, mix, noise=a.noise)
            t5 = time.perf_counter()
            lmn = g.eval_mix_logmmse(plan, rate, noise=a.noise)
            dts += [t5 - t4, time.perf_counter() - t5]
        if r:
            for k, dt in zip(t, dts):
                t[k].append(dt)
    g.close()
    ms = {k + "_ms_median": 1e3 * float(np.median(v)) for k, v in t.items()}
    out = {"what": "log-MMSE baseline vs the net's calls", "compute": a.compute, "sentences": a.sentences, "frames": frames,
           "audio_s": a.sentences * 6.0}
    out.update(ms)
    out.update({"noisy_mean": np.nanmean(ev["noisy"], axis=0).tolist(), "logmmse_mean": np.nanmean(lm["enhanced"], axis=0).tolist(),
                "net_mean": np.nanmean(ev["enhanced"], axis=0).tolist()})
    if a.noise:
        out["logmmse_%s_mean" % a.noise] = np.nanmean(lmn["enhanced"], axis=0).tolist()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
