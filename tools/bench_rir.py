"""Time of bp_rir_image (simulated room impulse responses, made on the device by bp_rir_image_taps) beside the bp_set_mix_reverb
that consumes its output, in the setting of tools/bench_reverb.py: 200 clean sentences of 4 s, 200 rooms drawn by bp_rir_rooms
from the default ranges, one response per sentence, target early (50 ms).  Four workloads: 8 kHz and 16 kHz, responses of 400 and
800 ms, the default window (8 ms).  The image count is that of the boxes (bp_rir_orders); the term count is what the definition
asks for, one a w(j - tau) per image and tap its window reaches inside the response.  The two calls alternate, each timed to its
synchronisation; medians.  One JSON line per workload.

    python tools/bench_rir.py [--reps 7] [--rooms 200] [--only 8000x400]
    python tools/bench_rir.py --once 16000x400      # one bp_rir_image and nothing else (for a kernel trace)
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

WORKLOADS = [(8000, 400), (8000, 800), (16000, 400), (16000, 800)]


def _images(rooms, rate, taps):
    return sum(dnnse_amd.rir_orders(r, rate, taps)[1] for r in rooms)


def one(rate, ms, a):
    D, ctx, toff = 129, 11, 5
    taps = int(np.floor(ms * rate / 1000.0 + 0.5))
    rooms = dnnse_amd.rir_rooms(0, a.rooms)
    lens = [taps] * a.rooms
    if a.once:
        dnnse_amd.rir_image(0, rate, rooms, lens)
        return None
    ls = [ctx * D, 64, D]                                          # (the net is not run: a small one)
    W, b = dnnse_amd.glorot_net(ls, seed=1, beta=0.5)
    rng = np.random.default_rng(0)
    n = 4 * rate
    clean = [np.round(rng.normal(0, 3000, n)).astype(np.float32) for _ in range(a.rooms)]
    noise = [np.round(rng.normal(0, 2000, 4 * rate)).astype(np.float32)]
    g = dnnse_amd.BP_GPU(1, len(ls), ls, 256, 0.001, 0.5, 0.0, W, b, max_chunk_frames=1024)
    g.set_mix_corpus(clean, noise, np.full(D, 10.0, np.float32), np.full(D, 0.25, np.float32), ctx, toff, "lps")
    pc = np.arange(a.rooms)
    t_img, t_rev, rirs = [], [], None
    for r in range(a.reps + 1):                                    # (rep 0: warm-up -- code objects)
        g.sync()
        t0 = time.perf_counter()
        rirs = dnnse_amd.rir_image(0, rate, rooms, lens)            # (returns synchronised)
        t1 = time.perf_counter()
        g.set_mix_reverb(rirs, pc, pc, "early", 50 * rate // 1000)  # (returns synchronised)
        t2 = time.perf_counter()
        if r:
            t_img.append(t1 - t0)
            t_rev.append(t2 - t1)
    g.close()
    tw = dnnse_amd.rir_window_default(rate)
    reach = (taps + tw / 2.0) * 343.0 / rate                        # images inside the reach: the ball's volume over the room's
    inside = sum(4.0 / 3.0 * np.pi * reach ** 3 / float(np.prod(r["L"])) for r in rooms)
    im, rv = float(np.median(t_img)), float(np.median(t_rev))
    peak = [int(np.argmax(np.abs(h))) for h in rirs]
    return {"what": "bp_rir_image beside bp_set_mix_reverb", "rate": rate, "rir_ms": ms, "taps": taps, "window_taps": tw, "rooms": a.rooms,
            "box_images": _images(rooms, rate, taps), "images_in_reach_estimate": int(inside), "terms_estimate": int(inside * tw),
            "rir_image_ms_median": 1e3 * im, "rir_image_ms_min": 1e3 * min(t_img), "set_mix_reverb_ms_median": 1e3 * rv,
            "image_over_reverb": im / rv, "gterms_per_s": 1e-9 * inside * tw / im,
            "peak_tap_median": float(np.median(peak)), "sentences": a.rooms, "samples_per_sentence": n}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rooms", type=int, default=200)
    ap.add_argument("--only", default="")
    ap.add_argument("--once", default="")
    a = ap.parse_args()
    pick = a.once or a.only
    for rate, ms in WORKLOADS:
        if pick and pick != "%dx%d" % (rate, ms):
            continue
        out = one(rate, ms, a)
        if out:
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
