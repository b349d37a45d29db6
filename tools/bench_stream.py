"""Wall time per push of a streaming session (bp_stream_push) on the shipped enhancement net (1548-2048x3-129: 11 frames of
129 bins + the noise-aware block, look-ahead 5 frames), against the only thing a caller without streaming could do with the same
audio: one bp_enhance_waves call on n_chan pseudo-sentences of one block.  (That call does not compute the same thing -- every
block gets replicated edge frames, a noise-aware row of its own and a window seam -- it is the cost comparison.)

Grid: bunchsize 32 and 64, n_chan 1 / 8 / 64, blocks of hop and 4 hop samples at 8 kHz.  Per cell: warm-up (the sentence start,
until every push returns a full block), then --rounds rounds that ALTERNATE --pushes streaming pushes with as many
bp_enhance_waves calls, so that clock and load drift hit both alike.  One JSON line per cell: median and 99th-percentile wall
time per call and audio seconds per wall second.  The launches and the two copies of a push show under
`rocprofv3 --kernel-trace --memory-copy-trace -- python tools/bench_stream.py --cells 1` (profiles/).

--forward rowinv measures a stream opened in FORWARD_ROWINV (it packs its channels; the bp_enhance_waves calls run in that mode
too); --forward both opens one stream per mode on the same handle, feeds both the same audio and alternates them round by round
(which mode goes first changes with the round): per mode the median and p99 over all pushes and the median of every round -- the
run-to-run spread -- and the ratio of the medians.  A tool, not a yardstick.

    python tools/bench_stream.py [--rounds 5] [--pushes 200] [--compute fp32|bf16] [--cells N] [--forward default|rowinv|both]
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
    ap.add_argument("--forward", default="default", choices=["default", "rowinv", "both"])
    a = ap.parse_args()
    D, ctx, toff, rate = 129, 11, 5, 8000
    hop = D - 1
    ls = [(ctx + 1) * D, 2048, 2048, 2048, D]
    W, b = dnnse_amd.glorot_net(ls, seed=1, beta=0.5)
    mean, istd = np.full(D, 10.0, np.float32), np.full(D, 0.25, np.float32)
    rng = np.random.default_rng(0)
    cells = [(B, nc, k) for B in (32, 64) for nc in (1, 8, 64) for k in (1, 4)]
    codes = {"default": dnnse_amd.FORWARD_DEFAULT, "rowinv": dnnse_amd.FORWARD_ROWINV}
    modes = ["default", "rowinv"] if a.forward == "both" else [a.forward]
    for B, nc, k in cells[:a.cells or len(cells)]:
        block = k * hop
        g = dnnse_amd.BP_GPU(1, len(ls), ls, B, 0.0, 0.0, 0.0, W, b, dropoutflag=1, visible_omit=0.1, hid_omit=0.2,
                             max_chunk_frames=4096, compute_dtype=1 if a.compute == "bf16" else 0)
        streams = {}
        for m in modes:                                              # a stream keeps the mode of its open
            g.set_forward(codes[m])
            streams[m] = g.stream_open(mean, istd, ctx, toff, n_chan=nc, max_push_samples=nc * block)
        n_push = a.rounds * a.pushes + 16
        feed = np.round(rng.normal(0, 3000, (n_push, nc, block))).astype(np.float32)
        for m in modes:
            for p in range(16):                                      # warm-up: past the sentence start (6 frames + the look-ahead)
                out = streams[m].push(list(feed[p]))
            assert all(o.size == block for o in out)
            g.set_forward(codes[m])
            g.enhance_waves(list(feed[0]), mean, istd, ctx, toff)
        t_push, t_off = {m: [] for m in modes}, {m: [] for m in modes}
        p = 16
        for r in range(a.rounds):
            order = modes[::-1] if r % 2 else modes
            for m in order:
                for q in range(a.pushes):
                    blocks = list(feed[p + q])
                    t0 = time.perf_counter()
                    streams[m].push(blocks)
                    t_push[m].append(time.perf_counter() - t0)
            for m in order:
                g.set_forward(codes[m])
                for q in range(a.pushes):
                    blocks = list(feed[p + q])
                    t0 = time.perf_counter()
                    g.enhance_waves(blocks, mean, istd, ctx, toff)
                    t_off[m].append(time.perf_counter() - t0)
            p += a.pushes
        for m in modes:
            streams[m].close()
        g.close()
        audio = nc * block / rate
        row = {"what": "bp_stream_push vs bp_enhance_waves on the same audio per call", "compute": a.compute, "forward": a.forward,
               "bunchsize": B, "n_chan": nc, "block_samples": block, "frames_per_push": nc * k, "calls": a.rounds * a.pushes}
        for m in modes:
            pre = m + "_" if len(modes) > 1 else ""
            for tag, ts in (("push", t_push[m]), ("offline", t_off[m])):
                ts = np.asarray(ts)
                row["%s%s_us_median" % (pre, tag)] = 1e6 * float(np.median(ts))
                row["%s%s_us_p99" % (pre, tag)] = 1e6 * float(np.percentile(ts, 99))
                row["%s%s_x_realtime" % (pre, tag)] = audio / float(np.median(ts))
            row["%spush_us_round_medians" % pre] = [1e6 * float(np.median(c)) for c in np.split(np.asarray(t_push[m]), a.rounds)]
        if len(modes) > 1:
            row["rowinv_over_default_push_median"] = row["rowinv_push_us_median"] / row["default_push_us_median"]
            row["rowinv_over_default_push_p99"] = row["rowinv_push_us_p99"] / row["default_push_us_p99"]
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
