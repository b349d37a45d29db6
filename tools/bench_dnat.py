"""Wall time of the dynamic noise-aware input (bp_set_nat) against the static one, on the shipped enhancement
net (1548-2048x3-129: 11 frames of 129 bins + the noise-aware block) and the same 100 mixtures of 6 s at 8 kHz: bp_enhance_waves on
the mixed samples and bp_train_mix on the plan, the two modes alternating call by call on one handle.  One JSON line: the median
of --reps per call and mode, and the dynamic / static ratios.  The tracker's own time comes from running it under
`rocprofv3 --kernel-trace --stats -- python tools/bench_dnat.py` (bp_wave_dnat against bp_wave_nat).

    python tools/bench_dnat.py [--reps 10] [--mixtures 100] [--seconds 6]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dnnse_amd  # noqa: E402

MODES = ("static", "dynamic")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--mixtures", type=int, default=100)
    ap.add_argument("--seconds", type=float, default=6.0)
    a = ap.parse_args()
    D, ctx, toff, rate = 129, 11, 5, 8000
    ls = [(ctx + 1) * D, 2048, 2048, 2048, D]
    W, b = dnnse_amd.glorot_net(ls, seed=1, beta=0.5)
    rng = np.random.default_rng(0)
    n = int(a.seconds * rate)
    clean = [np.round(rng.normal(0, 3000, n)).astype(np.float32) for _ in range(a.mixtures)]
    noise = [np.round(rng.normal(0, 1000, 20 * rate)).astype(np.float32) for _ in range(4)]
    frames = a.mixtures * ((n - 1) // (D - 1) + 2)
    rows = frames + a.mixtures * (ctx - 1)
    g = dnnse_amd.BP_GPU(1, len(ls), ls, 1024, 1e-4, 0.5, 0.0, W, b, dropoutflag=1, visible_omit=0.1, hid_omit=0.2,
                         max_chunk_frames=rows)
    mean, istd = np.full(D, 10.0, np.float32), np.full(D, 0.25, np.float32)
    g.set_mix_corpus(clean, noise, mean, istd, ctx, toff)
    plan = dnnse_amd.mix_plan(1, a.mixtures, 1, [x.size for x in noise], [-5, 0, 5, 10])
    lens = [clean[c].size for c in plan["clean"]]
    xs = np.split(g.mix_features(plan)["pcm"], np.cumsum(lens)[:-1])

    def enhance():
        g.enhance_waves(xs, mean, istd, ctx, toff)

    def train():
        g.train_mix(plan)
        g.sync()

    # (the library reports the partial last bunch of every training call on stdout, as the reference does: keep this tool's
    # stdout to its one line)
    sys.stdout.flush()
    keep = os.dup(1)
    null = os.open(os.devnull, os.O_WRONLY)
    os.dup2(null, 1)
    out = {"what": "dynamic against static noise-aware input, wall time", "mixtures": a.mixtures, "audio_s": a.mixtures * a.seconds,
           "frames": frames, "reps": a.reps}
    for name, call in (("enhance_waves", enhance), ("train_mix", train)):
        ts = {m: [] for m in MODES}
        for m in MODES:                                          # warm-up: buffers of both sizes, code objects
            g.set_nat(m)
            call()
        for _ in range(a.reps):
            for m in MODES:
                g.set_nat(m)
                t0 = time.perf_counter()
                call()
                ts[m].append(time.perf_counter() - t0)
        med = {m: 1e3 * float(np.median(ts[m])) for m in MODES}
        out[name] = {"static_ms_median": med["static"], "dynamic_ms_median": med["dynamic"],
                     "static_ms_min": 1e3 * float(np.min(ts["static"])), "dynamic_ms_min": 1e3 * float(np.min(ts["dynamic"])),
                     "dynamic_over_static": med["dynamic"] / med["static"]}
    g.close()
    ctypes.CDLL(None).fflush(None)                               # (what the C library still buffers goes where the rest went)
    os.dup2(keep, 1)
    os.close(keep)
    os.close(null)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
