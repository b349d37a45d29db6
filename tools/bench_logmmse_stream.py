"""Wall time per push of a log-MMSE stream (bp_lmstream_push): 1, 8 and 64 channels x blocks of 20 ms at 8 kHz (160 samples),
fea_dim 129.  Beside it, on the same audio per call: bp_logmmse_waves on n_chan pseudo-sentences of one block (what a caller
without the stream could do; it does not compute the same thing -- every block gets a noise start of its own), and the net's
packed stream (bp_stream_push opened in FORWARD_ROWINV) in the setting of tools/bench_stream.py: the shipped enhancement net
1548-2048x3-129, bunch 32.

Per cell: warm-up past the sentence start, then --rounds rounds that ALTERNATE --pushes calls of each of the three, so that clock
and load drift hit all alike.  One JSON line per cell -- median and 99th-percentile wall time per call, audio seconds per wall
second -- and the lines together as a JSON file (--out, default profiles/bench_logmmse_stream.json).  The one launch and the two
copies of a push show under `rocprofv3 --kernel-trace --stats -- python tools/bench_logmmse_stream.py --only-stream`.
A tool, not a yardstick.

--noise spp adds a stream opened with the MMSE-SPP noise tracker (bp_lmstream_open_nt) to the alternation: the
same pushes, one more column per cell.

    python tools/bench_logmmse_stream.py [--rounds 5] [--pushes 200] [--only-stream] [--noise spp] [--out FILE]
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
    ap.add_argument("--only-stream", action="store_true", help="only the log-MMSE stream's pushes (for a kernel trace)")
    ap.add_argument("--noise", default=None, choices=["spp"], help="also time a stream with the noise tracker")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_logmmse_stream.json"))
    a = ap.parse_args()
    D, ctx, toff, rate, block, B = 129, 11, 5, 8000, 160, 32
    ls = [(ctx + 1) * D, 2048, 2048, 2048, D]
    mean, istd = np.full(D, 10.0, np.float32), np.full(D, 0.25, np.float32)
    rng = np.random.default_rng(0)
    g = None
    if not a.only_stream:
        W, b = dnnse_amd.glorot_net(ls, seed=1, beta=0.5)
        g = dnnse_amd.BP_GPU(1, len(ls), ls, B, 0.0, 0.0, 0.0, W, b, dropoutflag=1, visible_omit=0.1, hid_omit=0.2, max_chunk_frames=4096)
        g.set_forward(dnnse_amd.FORWARD_ROWINV)
    rows = []
    for nc in (1, 8, 64):
        n_push = a.rounds * a.pushes + 16
        feed = np.round(rng.normal(0, 3000, (n_push, nc, block))).astype(np.float32)
        lm = dnnse_amd.logmmse_stream_open(0, D, n_chan=nc, max_push_samples=nc * block)
        lmn = dnnse_amd.logmmse_stream_open(0, D, n_chan=nc, max_push_samples=nc * block, noise=a.noise) if a.noise else None
        net = None if g is None else g.stream_open(mean, istd, ctx, toff, n_chan=nc, max_push_samples=nc * block)
        for p in range(16):                                          # warm-up: past the noise start and the net's look-ahead
            lm.push(list(feed[p]))
            if lmn is not None:
                lmn.push(list(feed[p]))
            if net is not None:
                net.push(list(feed[p]))
                dnnse_amd.logmmse_waves(0, D, list(feed[p]))
        t = {"lmstream_push": [], "lmstream_push_spp": [], "logmmse_waves": [], "net_packed_push": []}
        p = 16
        for r in range(a.rounds):
            for what, call in (("lmstream_push", lm.push), ("lmstream_push_spp", None if lmn is None else lmn.push), ("logmmse_waves", lambda bl: dnnse_amd.logmmse_waves(0, D, bl)),
                               ("net_packed_push", None if net is None else net.push)):
                if call is None or (a.only_stream and not what.startswith("lmstream_push")):
                    continue
                for q in range(a.pushes):
                    blocks = list(feed[p + q])
                    t0 = time.perf_counter()
                    call(blocks)
                    t[what].append(time.perf_counter() - t0)
            p += a.pushes
        lm.close()
        if lmn is not None:
            lmn.close()
        if net is not None:
            net.close()
        audio = nc * block / rate
        row = {"what": "bp_lmstream_push vs bp_logmmse_waves vs the net's packed bp_stream_push on the same audio per call",
               "fea_dim": D, "n_chan": nc, "block_samples": block, "calls": a.rounds * a.pushes}
        for what, ts in t.items():
            if not ts:
                continue
            ts = np.asarray(ts)
            row[what + "_us_median"] = 1e6 * float(np.median(ts))
            row[what + "_us_p99"] = 1e6 * float(np.percentile(ts, 99))
            row[what + "_x_realtime"] = audio / float(np.median(ts))
            row[what + "_us_round_medians"] = [1e6 * float(np.median(c)) for c in np.split(ts, a.rounds)]
        print(json.dumps(row), flush=True)
        rows.append(row)
    if g is not None:
        g.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
