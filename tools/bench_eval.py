"""Time of bp_eval_mix (mixtures made on the device, enhanced with the net, and the noisy and enhanced sentences scored: SSNR,
LSD, STOI) against bp_enhance_waves on the same mixtures (enhancement alone), in the setting of tools/bench_mix.py: 100 clean
sentences of 6 s at 8 kHz, 4 noise recordings of 60 s, the shipped enhancement net (1548-2048x3-129: 11 frames of 129 bins +
the noise-aware block), bunch 256.  The two calls alternate, each timed to its synchronisation; median of --reps.  One JSON
line.  Kernel times come from running it under `rocprofv3 --kernel-trace --stats -- python tools/bench_eval.py` (bp_eval_*
against the forward's kernels).

--extended, --full, --all: bp_eval_mix_ext with five, seven or nine score columns against the call of the next narrower width on the
same mixtures instead (WIDER below), alternating in the same way; both medians, their ratio, and whether the narrower call's
columns hold the same bits.  The added kernels' share: the same `rocprofv3` line with the flag.

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


# A width of the score rows: its name in the JSON keys, its columns, eval_mix's extended= value.  --flag: (narrower, wider)
BASIC, EXTENDED, FULL, ALL = ("basic", 3, False), ("extended", 5, True), ("full", 7, "full"), ("all", 9, "all")
WIDER = {"extended": (BASIC, EXTENDED), "full": (EXTENDED, FULL), "all": (FULL, ALL)}


def alternate(reps, first, second):
    """The two calls in turn, each timed to its synchronisation: the median seconds of either over reps turns (after one warm-up
    turn: buffers, code objects) and their last results."""
    t = [], []
    for r in range(reps + 1):
        t0 = time.perf_counter()
        x = first()
        t1 = time.perf_counter()
        y = second()
        t2 = time.perf_counter()
        if r:
            t[0].append(t1 - t0)
            t[1].append(t2 - t1)
    return float(np.median(t[0])), float(np.median(t[1])), x, y


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
    row = next((WIDER[f] for f in WIDER if getattr(a, f)), None)
    head = {"compute": a.compute, "mixtures": a.sentences, "frames": frames}
    if row:
        (nlo, clo, xlo), (nhi, chi, xhi) = row
        mlo, mhi, evlo, ev = alternate(a.reps, lambda: g.eval_mix(plan, rate, extended=xlo), lambda: g.eval_mix(plan, rate, extended=xhi))
        same = all(np.array_equal(ev[k][:, :clo].view(np.uint32), evlo[k].view(np.uint32)) for k in ("noisy", "enhanced"))
        line = {"what": "bp_eval_mix_ext (%d columns) vs %s (%d columns)" % (chi, "bp_eval_mix_ext" if xlo else "bp_eval_mix", clo), **head,
                nlo + "_ms_median": 1e3 * mlo, nhi + "_ms_median": 1e3 * mhi, "%s_over_%s" % (nhi, nlo): mhi / mlo,
                "columns_0_to_%d_same_bits" % (clo - 1): same}
    else:                                                          # the same mixtures, enhancement alone
        m, s, ev, _ = alternate(a.reps, lambda: g.eval_mix(plan, rate), lambda: g.enhance_waves(mix, mean, istd, ctx, toff))
        line = {"what": "bp_eval_mix vs bp_enhance_waves", **head, "eval_ms_median": 1e3 * m, "enhance_ms_median": 1e3 * s, "eval_over_enhance": m / s}
    g.close()
    print(json.dumps({**line, "noisy_mean": np.nanmean(ev["noisy"], axis=0).tolist(), "enhanced_mean": np.nanmean(ev["enhanced"], axis=0).tolist()}))


if __name__ == "__main__":
    main()
