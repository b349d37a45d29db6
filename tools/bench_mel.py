"""What the MFCC auxiliary target (bp_set_mix_aux) costs a training call: bp_train_mix with the target row
[LPS | MFCC] against bp_train_mix with [LPS] alone, on the same mixtures, in the setting of tools/bench_mix.py (the shipped
enhancement net 1548-2048x3-129, bunch 256, dropout on; 100 clean sentences of 6 s at 8 kHz, 4 noise recordings of 60 s: 37 600
frames, 146 full bunches).  The two handles differ in the width of the output layer alone (129 | 129 + 13); their calls alternate,
each timed to its synchronisation, and the medians are reported.  Beside it: bp_wave_mfcc (all three outputs, and the coefficients
alone) against bp_wave_lps on the same clean sentences, host copies included.  Informational: no pass bar.  One JSON line.

    python tools/bench_mel.py [--reps 10] [--compute fp32|bf16] [--out profiles/mel_bench.json]
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
    mel = dnnse_amd.mel_params(rate)                               # 26 filters, 13 coefficients from c0, lifter 22
    rng = np.random.default_rng(0)
    n = 6 * rate
    clean = [np.round(rng.normal(0, 3000, n)).astype(np.float32) for _ in range(a.sentences)]
    noise = [np.round(rng.normal(0, 2000, 60 * rate)).astype(np.float32) for _ in range(4)]
    frames = a.sentences * ((n - 1) // (D - 1) + 2)
    g = {}
    for aux in (False, True):
        ls = [(ctx + 1) * D, 2048, 2048, 2048, D + (mel.n_ceps if aux else 0)]
        W, b = dnnse_amd.glorot_net(ls, seed=1, beta=0.5)
        g[aux] = dnnse_amd.BP_GPU(1, len(ls), ls, B, 0.001, 0.5, 0.0, W, b, dropoutflag=1, visible_omit=0.1, hid_omit=0.2,
                                  max_chunk_frames=frames + a.sentences * (ctx - 1), compute_dtype=1 if a.compute == "bf16" else 0)
        g[aux].set_mix_aux(mel if aux else None)
        g[aux].set_mix_corpus(clean, noise, np.full(D, 10.0, np.float32), np.full(D, 0.25, np.float32), ctx, toff, "lps")
    t = {False: [], True: []}
    for r in range(a.reps + 1):                                    # (rep 0: warm-up -- buffers, code objects)
        plan = dnnse_amd.mix_plan(r, a.sentences, 1, [x.size for x in noise], [-5, 0, 5, 10, 15, 20])
        order = dnnse_amd.mix_shuffle(r, 0, frames)
        for aux in ((False, True) if r % 2 else (True, False)):
            t0 = time.perf_counter()
            g[aux].train_mix(plan, order)
            g[aux].sync()
            if r:
                t[aux].append(time.perf_counter() - t0)
    for h in g.values():
        h.close()
    w = {"lps": [], "mfcc_all": [], "mfcc": []}
    for r in range(a.reps + 1):
        for k in (("lps", "mfcc_all", "mfcc") if r % 2 else ("mfcc", "mfcc_all", "lps")):
            t0 = time.perf_counter()
            if k == "lps":
                dnnse_amd.wave_lps(0, D, clean)
            else:
                dnnse_amd.wave_mfcc(0, D, clean, mel, return_logmel=k == "mfcc_all", return_power=k == "mfcc_all")
            if r:
                w[k].append(time.perf_counter() - t0)
    off, on = float(np.median(t[False])), float(np.median(t[True]))
    res = {"what": "bp_train_mix with and without the MFCC auxiliary target; bp_wave_mfcc beside bp_wave_lps", "compute": a.compute,
           "frames": frames, "bunches": frames // B, "reps": a.reps, "n_mel": int(mel.n_mel), "n_ceps": int(mel.n_ceps),
           "train_mix_ms_median": 1e3 * off, "train_mix_aux_ms_median": 1e3 * on, "aux_over_plain": on / off,
           "train_mix_ms_min_max": [1e3 * min(t[False]), 1e3 * max(t[False])], "train_mix_aux_ms_min_max": [1e3 * min(t[True]), 1e3 * max(t[True])],
           "wave_lps_ms_median": 1e3 * float(np.median(w["lps"])), "wave_mfcc_all_outputs_ms_median": 1e3 * float(np.median(w["mfcc_all"])),
           "wave_mfcc_ms_median": 1e3 * float(np.median(w["mfcc"]))}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
