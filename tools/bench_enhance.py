"""Wall time of bp_enhance_waves on the shipped enhancement net (1548-2048x3-129: 11 frames of 129 bins + the noise-aware
block), for 10 minutes of 8 kHz audio in one call: 100 sentences of 6 s.  One JSON line.  Kernel times come from running it
under `rocprofv3 --kernel-trace --stats -- python tools/bench_enhance.py` (bp_wave_* against the forward's GEMM kernels).

    python tools/bench_enhance.py [--reps 10] [--compute fp32|bf16] [--forward default|rowinv]
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
    ap.add_argument("--forward", default="default", choices=["default", "rowinv"], help="the kernels of the inference forward (bp_set_forward)")
    ap.add_argument("--sentences", type=int, default=100)
    ap.add_argument("--seconds", type=float, default=6.0)
    a = ap.parse_args()
    D, ctx, toff, rate = 129, 11, 5, 8000
    ls = [(ctx + 1) * D, 2048, 2048, 2048, D]
    W, b = dnnse_amd.glorot_net(ls, seed=1, beta=0.5)
    rng = np.random.default_rng(0)
    n = int(a.seconds * rate)
    xs = [np.round(rng.normal(0, 3000, n)).astype(np.float32) for _ in range(a.sentences)]
    frames = a.sentences * ((n - 1) // (D - 1) + 2)
    rows = frames + a.sentences * (ctx - 1)
    g = dnnse_amd.BP_GPU(1, len(ls), ls, 1024, 0.0, 0.0, 0.0, W, b, dropoutflag=1, visible_omit=0.1, hid_omit=0.2,
                         max_chunk_frames=rows, compute_dtype=1 if a.compute == "bf16" else 0)
    g.set_forward(dnnse_amd.FORWARD_ROWINV if a.forward == "rowinv" else dnnse_amd.FORWARD_DEFAULT)
    mean, istd = np.full(D, 10.0, np.float32), np.full(D, 0.25, np.float32)
    g.enhance_waves(xs, mean, istd, ctx, toff)                     # warm-up: buffers, code objects
    ts = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        g.enhance_waves(xs, mean, istd, ctx, toff)
        ts.append(time.perf_counter() - t0)
    g.close()
    audio_s = a.sentences * a.seconds
    fwd_flop = 2.0 * frames * sum(ls[l - 1] * ls[l] for l in range(1, len(ls)))
    print(json.dumps({"what": "bp_enhance_waves wall time", "compute": a.compute, "forward": a.forward, "audio_s": audio_s, "frames": frames,
                      "ms_median": 1e3 * float(np.median(ts)), "ms_min": 1e3 * float(np.min(ts)),
                      "x_realtime": audio_s / float(np.median(ts)), "forward_gflop": fwd_flop / 1e9}))


if __name__ == "__main__":
    main()
