"""Wall time of the sample-rate converter (bp_resample_waves) on the three loads a corpus brings:

  speech 16000 -> 8000   200 sentences x 6 s    (TIMIT-like speech for the shipped 8 kHz net; p/q = 1/2)
  speech 44100 -> 16000  200 sentences x 6 s    (CD-rate material; p/q = 160/441)
  noise  19980 -> 16000  one recording of 5 min (a NOISEX-92 file; p/q = 800/999)

Per load: --warmup calls, then --calls timed calls of the whole C-ABI call (host packing, one host->device copy, the launch, one
device->host copy, the synchronisation).  Reported: median and 99th-percentile wall time per call and input and output samples per
second of the whole call.  One JSON line per load.  The call has no handle and so no timer of its own: the rate without the copies
is the kernel's duration in a `rocprofv3 --kernel-trace -- python tools/bench_resample.py --calls 3` run (one bp_wave_resample
dispatch per call, the loads in the order above); profiles/resample_bench.jsonl holds both.  A tool, not a yardstick.

    python tools/bench_resample.py [--calls 10] [--warmup 2] [--loads N]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dnnse_amd  # noqa: E402

LOADS = [("speech 200 x 6 s", 16000, 8000, 200, 6.0), ("speech 200 x 6 s", 44100, 16000, 200, 6.0), ("noise 1 x 300 s", 19980, 16000, 1, 300.0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--loads", type=int, default=0, help="only the first N loads (0: all)")
    a = ap.parse_args()
    lib = dnnse_amd.load_library()
    rng = np.random.default_rng(0)
    for what, rate_in, rate_out, n_sent, seconds in LOADS[:a.loads or len(LOADS)]:
        p, q = dnnse_amd.resample_ratio(rate_in, rate_out)
        n = int(round(seconds * rate_in))
        lens = np.full(n_sent, n, np.int32)
        pcm = np.round(rng.normal(0, 3000, n_sent * n)).astype(np.float32)
        n_out = n_sent * dnnse_amd.resample_len(n, p, q)
        out = np.empty(n_out, np.float32)
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
        args = (0, rate_in, rate_out, None, n_sent, lens.ctypes.data_as(ip), pcm.ctypes.data_as(fp), out.ctypes.data_as(fp))
        ts = []
        for k in range(a.warmup + a.calls):
            t0 = time.perf_counter()
            rc = lib.bp_resample_waves(*args)
            dt = time.perf_counter() - t0
            if rc != 0:
                raise SystemExit(lib.bp_last_error().decode())
            if k >= a.warmup:
                ts.append(dt)
        ts = np.asarray(ts)
        med = float(np.median(ts))
        zeros = 16
        print(json.dumps({
            "what": "bp_resample_waves, whole call (packing + H2D + kernel + D2H + sync)", "load": what, "rate_in": rate_in, "rate_out": rate_out,
            "p": p, "q": q, "sentences": n_sent, "samples_in": int(n_sent * n), "samples_out": int(n_out), "calls": a.calls,
            "taps": 2 * zeros * max(p, q) + 1, "terms_per_output": (2 * zeros * max(p, q) + 1) / float(p),
            "call_ms_median": 1e3 * med, "call_ms_p99": 1e3 * float(np.percentile(ts, 99)), "call_ms_min": 1e3 * float(ts.min()),
            "in_samples_per_s": n_sent * n / med, "out_samples_per_s": n_out / med, "x_realtime": n_sent * seconds / med,
            "bytes_copied": int(4 * (n_sent * n + n_out)),
        }), flush=True)


if __name__ == "__main__":
    main()
