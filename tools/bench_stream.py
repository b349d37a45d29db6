"""Wall time per push of a streaming session (bp_stream_push) on the shipped enhancement net (1548-2048x3-129: 11 frames of
129 bins + the noise-aware block, look-ahead 5 frames), against the only thing a caller without streaming could do with the same
audio: one bp_enhance_waves call on n_chan pseudo-sentences of one block.  (That call does not compute the same thing -- every
block gets replicated edge frames, a noise-aware row of its own and a window seam -- it is the cost comparison.)

Grid: bunchsize 32 and 64, n_chan 1 / 8 / 64, blocks of hop and 4 hop samples at 8 kHz.  Per cell: warm-up (the sentence start,
until every push returns a full block), then --rounds rounds that ALTERNATE --pushes streaming pushes with as many
bp_enhance_waves calls, so that clock and load drift hit both alike.  One JSON line per cell: median and 99th-percentile wall
time per call and audio seconds per wall second.  The launches and the two copies of a push show under
`rocprofv3 --kernel-trace --memory-copy-trace -- python tools/bench_stream.py --cells 1` (profiles/).

    python tools/bench_stream.py [--rounds 5] [--pushes 200] [--compute fp32|bf16] [--cells N]
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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--pushes", type=int, default=200)
    ap.add_argument("--compute", default="fp32", choices=["fp32", "bf16"])
    ap.add_argument("--cells", type=int, default=0, help="only the first N cells of the grid (0: all)")
    a = ap.parse_args()
    D, ctx, toff, rate = 129, 11, 5, 8000
    hop = D - 1
    ls = [(ctx + 1) * D, 2048, 2048, 2048, D]
    W, b = dnnse_amd.glorot_net(ls, seed=1, beta=0.5)
    mean, istd = np.full(D, 10.0, np.float32), np.full(D, 0.25, np.float32)
    rng = np.random.default_rng(0)
    cells = [(B, nc, k) for B in (32, 64) for nc in (1, 8, 64) for k in (1, 4)]
    for B, nc, k in cells[:a.cells or len(cells)]:
        block = k * hop
        g = dnnse_amd.BP_GPU(1, len(ls), ls, B, 0.0, 0.0, 0.0, W, b, dropoutflag=1, visible_omit=0.1, hid_omit=0.2,
                             max_chunk_frames=4096, compute_dtype=1 if a.compute == "bf16" else 0)
        s = g.stream_open(mean, istd, ctx, toff, n_chan=nc, max_push_samples=nc * block)
        n_push = a.rounds * a.pushes + 16
        feed = np.round(rng.normal(0, 3000, (n_push, nc, block))).astype(np.float32)
        for p in range(16):                                          # warm-up: past the sentence start (6 frames + the look-ahead)
            out = s.push(list(feed[p]))
        assert all(o.size == block for o in out)
        g.enhance_waves(list(feed[0]), mean, istd, ctx, toff)
        t_push, t_off = [], []
        p = 16
        for _ in range(a.rounds):
            for _ in range(a.pushes):
                blocks = list(feed[p])
                t0 = time.perf_counter()
                s.push(blocks)
                t_push.append(time.perf_counter() - t0)
                p += 1
            for q in range(a.pushes):
                blocks = list(feed[p - a.pushes + q])
                t0 = time.perf_counter()
                g.enhance_waves(blocks, mean, istd, ctx, toff)
                t_off.append(time.perf_counter() - t0)
        s.close()
        g.close()
        audio = nc * block / rate
        row = {"what": "bp_stream_push vs bp_enhance_waves on the same audio per call", "compute": a.compute, "bunchsize": B,
               "n_chan": nc, "block_samples": block, "frames_per_push": nc * k, "calls": len(t_push)}
        for tag, ts in (("push", t_push), ("offline", t_off)):
            ts = np.asarray(ts)
            row["%s_us_median" % tag] = 1e6 * float(np.median(ts))
            row["%s_us_p99" % tag] = 1e6 * float(np.percentile(ts, 99))
            row["%s_x_realtime" % tag] = audio / float(np.median(ts))
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
