#!/usr/bin/env python3
"""bench.py -- training frames/sec of the frame-wise DNN step (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W
    (N>1: either exactly that -- the script then forks its N ranks itself, rank r on device r % visible devices -- or
    under a launcher: python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...;
    a --gpus that disagrees with the number of ranks is refused, so an N-GPU line is never printed from fewer ranks)

Workload at every N (weak scaling, per-GPU work fixed): BASELINE.json configs[1] = C2:
2827->2048->2048->2048->257 (257x11 stacked input), ReLU + dropout 0.1/0.2, fp32, 256 frames
per GPU per step, lrate 1, momentum 0.5, synthetic N(0,1) frames resident in HBM (generated on
device), Glorot*0.5 weights.  A step = forward + backward + momentum update of one bunch
(train_bunch_single, BP_GPU.cu:484-673).  For N>1 the global bunch is N*256 frames and the
gradient exchange is the LIBRARY's own (bp_dp_attach: hipIpc peer reduce-scatter + sharded fused
update + all-gather, include/bp_c_api.h) AND the same step over RCCL reduce-scatter/all-gather, timed back to back in the
one run: the line carries `exchange: {native, rccl, chosen}` and its value is the faster transport (--exchange native|rccl
times one only) -- the barrier around the timed region and the max over ranks go through the same group's shared-memory
rendezvous (bp_dp_barrier / bp_dp_allgather); no torch.distributed, no gloo.  The line lists what every rank attached
to (device ordinal, PCI bus id).

Timing protocol: `prewarm_s` seconds of real, untimed training steps first (a freshly leased GPU
needs that long to reach its sustained clocks; reported in the line), then W untimed warm-up
steps, then EXACTLY K timed steps between barrier+synchronize pairs.  Nothing is skipped in the
timed region.  Prints ONE JSON line on rank 0.  With one process the clock-driven part of the
pre-warm runs on a handle of its own and the timed handle gets a fixed 200 steps of it: what the
timed handle holds after its last step depends on the arguments alone.

A plain run does only what the headline needs.  --full adds everything else, as one line: the
sustained rate, the in-step roofline and measured peaks, this run's own rocprofv3 passes, the other
configurations (c5_bf16, c1_end_to_end, c3_nat, c2_window_chunk, dp_world1) and the CPU baseline
(--no-extras / --no-cpu-baseline leave parts of that out again).  --dump-outputs DIR writes, after
the timed steps, what the last timed step left for a caller of the step (the trained weights and
biases, float32 .npy), so that two builds can be compared output for output.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC: needed for hipIpc across processes on this driver
os.environ.setdefault("BP_DP_TIMEOUT_S", "120")            # attach / exchange time budget of the library (its default: 60 s)

import numpy as np  # noqa: E402

LAYERS = [257 * 11, 2048, 2048, 2048, 257]
BUNCH = 256
CHUNK = 102400            # frames resident per chunk (finetune_..._NAT.pl:39 traincache)
PEAK_MFMA_F32_TF = 157.3  # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 dense peak (spec, 2.4 GHz)
PEAK_HBM_GBS = 8000.0     # spec
C5_LAYERS = [257 * 11, 4096, 4096, 4096, 4096, 4096, 257]   # BASELINE.json configs[4], per-GPU shard of 512 frames
C5_BUNCH = 512
PREWARM_FIXED_STEPS = 200  # one process: the pre-warm's last steps, on the timed handle (a fixed count: --dump-outputs)


def n_params(ls):
    return sum(ls[i - 1] * ls[i] for i in range(1, len(ls)))


def flops_per_frame(ls):
    return 6 * n_params(ls) - 2 * ls[0] * ls[1]


def wgrad_flops_per_step(ls, B):
    return 2.0 * B * n_params(ls)


def cpu_baseline(W, b, budget_s=12.0, max_steps=64):
    """The oracle (C restatement, OpenMP) timed on this box's host cores on a bounded sample of
    the same workload: whole C2 training steps (dropout on) until ~budget_s of CPU time."""
    from oracle import oracle as O
    O.build()
    o = O.Oracle(LAYERS, BUNCH, 1.0, 0.5, 0.0, W, b, dropoutflag=1, visible_omit=0.1, hid_omit=0.2, seed=1)
    rng = np.random.default_rng(20260927)
    x = rng.standard_normal((BUNCH, LAYERS[0]), dtype=np.float32)
    t = rng.standard_normal((BUNCH, LAYERS[-1]), dtype=np.float32)
    o.train_bunch(x, t)                      # warm-up (page in, thread pool)
    # thread count: the fastest of a quick probe (a container may show 256 CPUs and grant far fewer: spinning
    # OpenMP threads then make "all cores" the SLOWEST choice by two orders of magnitude)
    ncpu = os.cpu_count() or 1
    probe = {}
    if "OMP_NUM_THREADS" not in os.environ:
        for nt in [c for c in (8, 16, 32, 64, 128, 256) if c <= ncpu] or [ncpu]:
            O.set_threads(nt)
            o.train_bunch(x, t)
            t1 = time.perf_counter(); o.train_bunch(x, t); probe[nt] = time.perf_counter() - t1
            if probe[nt] > 4 * min(probe.values()):
                break
        cores = min(probe, key=probe.get)
        O.set_threads(cores)
    else:
        cores = int(os.environ["OMP_NUM_THREADS"])
    n, t0 = 0, time.perf_counter()
    while n < max_steps and (time.perf_counter() - t0) < budget_s:
        o.train_bunch(x, t)
        n += 1
    dt = time.perf_counter() - t0
    res = {"value": n * BUNCH / dt, "unit": "frames/s", "cores": cores, "kind": "port",
           "sample": "%d full C2 training steps (256 frames each, fp32, dropout on) of oracle/bp_oracle.c "
                     "(cache-blocked AVX GEMMs, OpenMP, %d threads = fastest of the probe %s on %d visible CPUs), %.1f s"
                     % (n, cores, {k: round(v, 3) for k, v in probe.items()}, ncpu, dt)}
    try:
        res["c1"] = cpu_baseline_c1(O, cores)
    except Exception as e:
        res["c1"] = {"error": str(e)[:200]}
    try:
        res["torch_cpu_not_the_reference"] = torch_cpu_line(W, b, budget_s=min(6.0, budget_s / 2))
    except Exception as e:                   # a labelled extra, never fatal
        res["torch_cpu_not_the_reference"] = {"error": str(e)[:200]}
    return res


C1_LAYERS, C1_BUNCH = [257, 512, 257], 128     # BASELINE.json configs[0]: 1x512 Sigmoid, 257-bin single-frame input, 128-frame minibatches


def cpu_baseline_c1(O, cores, frames=36000, budget_s=4.0):
    """SURVEY 8(d) "CPU baseline ... frames/s for C1 (full)": the oracle on the C1 shape over a whole synthetic training
    pass the size of c1_end_to_end's Pfile pair (120 sentences x 300 frames = 281 minibatches of 128, Sigmoid, classic
    momentum, no dropout), host wall clock around the pass as the reference times its passes (BPtrain.cc:25-26,91-92)."""
    import dnnse_amd
    W, b = dnnse_amd.glorot_net(C1_LAYERS, seed=1, beta=0.5)
    rng = np.random.default_rng(20260927)
    nb = frames // C1_BUNCH
    x = rng.standard_normal((nb * C1_BUNCH, C1_LAYERS[0]), dtype=np.float32)
    t = rng.standard_normal((nb * C1_BUNCH, C1_LAYERS[-1]), dtype=np.float32)
    best = None
    for nt in sorted({1, min(cores, 4), cores}):           # a 0.26 M-parameter net: fewer threads can be faster than the C2 choice
        O.set_threads(nt)
        o = O.Oracle(C1_LAYERS, C1_BUNCH, 0.01, 0.5, 0.0, W, b, activation=1, momentum_rule=1)
        o.train_bunch(x[:C1_BUNCH], t[:C1_BUNCH])
        t0 = time.perf_counter()
        done = 0
        while done < nb and time.perf_counter() - t0 < budget_s:
            o.train_bunch(x[done * C1_BUNCH:(done + 1) * C1_BUNCH], t[done * C1_BUNCH:(done + 1) * C1_BUNCH], gen_masks=False)
            done += 1
        dt = time.perf_counter() - t0
        if best is None or done * C1_BUNCH / dt > best["value"]:
            best = {"value": done * C1_BUNCH / dt, "unit": "frames/s", "cores": nt, "kind": "port",
                    "sample": "%d of %d minibatches (128 frames, 257->512->257 Sigmoid, classic momentum) of one synthetic C1 training pass, "
                              "oracle/bp_oracle.c on %d threads, %.2f s" % (done, nb, nt, dt)}
    O.set_threads(cores)
    return best


def torch_cpu_line(W, b, budget_s=6.0):
    """Same C2 step written with torch CPU ops (vendor BLAS under torch.mm): NOT the reference and not
    the oracle -- a labelled second opinion on what this box's host cores can do with a tuned SGEMM."""
    import torch
    Ws = [None] + [torch.from_numpy(np.ascontiguousarray(W[l])) for l in range(1, len(LAYERS))]
    bs = [None] + [torch.from_numpy(np.ascontiguousarray(b[l])) for l in range(1, len(LAYERS))]
    dW = [None] + [torch.zeros_like(w) for w in Ws[1:]]
    db = [None] + [torch.zeros_like(v) for v in bs[1:]]
    g = torch.Generator().manual_seed(1)
    x = torch.randn(BUNCH, LAYERS[0], generator=g)
    t = torch.randn(BUNCH, LAYERS[-1], generator=g)
    L, m, lr = len(LAYERS), 0.5, 1.0

    def step():
        ys = [x * (torch.rand(x.shape, generator=g) >= 0.1)]
        for l in range(1, L):
            z = torch.addmm(bs[l], ys[-1], Ws[l])
            ys.append(torch.relu(z) * (torch.rand(z.shape, generator=g) >= 0.2) if l < L - 1 else z)
        dx = (2.0 / BUNCH) * (ys[-1] - t)
        for l in range(L - 1, 0, -1):
            dprev = (dx @ Ws[l].t()) * (ys[l - 1] > 0) if l > 1 else None
            G = ys[l - 1].t() @ dx
            dW[l].mul_(m).sub_((1 - m) * lr * (G / BUNCH)); Ws[l].add_(dW[l])
            db[l].mul_(m).sub_((1 - m) * lr * (dx.sum(0) / BUNCH)); bs[l].add_(db[l])
            dx = dprev
    step()
    n, t0 = 0, time.perf_counter()
    while n < 200 and time.perf_counter() - t0 < budget_s:
        step(); n += 1
    dt = time.perf_counter() - t0
    return {"value": n * BUNCH / dt, "unit": "frames/s", "threads": torch.get_num_threads(),
            "sample": "%d C2 steps with torch CPU ops, %.1f s" % (n, dt)}


def kernel_source_stamp():
    """sha256[:16] over the kernel sources, as tools/profile_r06.sh stamps its PMC summaries: tells whether a traffic
    figure read from profiles/ was measured on the kernels this run executes."""
    import glob
    import hashlib
    d = os.path.join(ROOT, "dnn-for-speech-enhancement_amd", "csrc")
    h = hashlib.sha256()
    for f in sorted(glob.glob(os.path.join(d, "*.h"))) + sorted(glob.glob(os.path.join(d, "*.hip"))):
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def profiled_traffic(fname, match):
    """(bytes per launch, stamp dict) of the first kernel whose key satisfies `match` in a tools/pmc_summary.py file."""
    try:
        pm = json.load(open(os.path.join(ROOT, "profiles", fname)))
    except Exception:
        return None, None
    note = pm.get("note", "")
    stamp = note.split("sha256[:16] ")[1].split(";")[0] if "sha256[:16] " in note else None
    for k, v in pm.get("kernels", {}).items():
        if match(k) and "fetch_MB_corrected_x2" in v and "write_MB" in v:
            return (v["fetch_MB_corrected_x2"] + v["write_MB"]) * 1e6, {"source": "profiles/" + fname, "kernel": k, "sources_sha": stamp,
                                                                      "matches_current_kernel_sources": stamp == kernel_source_stamp() if stamp else None}
    return None, None


def c5_line(dnnse_amd, dev, steps=40):
    """BASELINE.json configs[4] per-GPU shape (2827->4096x5->257, 512 frames per GPU, bf16 operands, fp32
    master weights) on this one GPU: step time and its HBM roofline (the step is HBM-bound)."""
    W, b = dnnse_amd.glorot_net(C5_LAYERS, seed=1, beta=0.5)
    g = dnnse_amd.BP_GPU(1, len(C5_LAYERS), C5_LAYERS, C5_BUNCH, 1.0, 0.5, 0.0, W, b, device=dev,
                         max_chunk_frames=16 * C5_BUNCH, compute_dtype=1)
    g.fill_chunk_synthetic(16 * C5_BUNCH, 20260927)
    for _ in range(3):
        g.train_resident(0, 16 * C5_BUNCH)
    g.sync()
    t0 = time.perf_counter()
    done = 0
    while done < steps:
        k = min(16, steps - done)
        g.train_resident(0, k * C5_BUNCH)
        done += k
    g.sync()
    dt = (time.perf_counter() - t0) / steps
    g.close()
    P = n_params(C5_LAYERS)
    # algorithmic bytes per step of the bf16 mode (lower figure): bf16 weights read by fwd and dgrad
    # (2P + 2(P - s0 s1)), fp32 W and delta read + written by the fused update (16P), bf16 shadow refresh (2P)
    alg = 22.0 * P - 2.0 * C5_LAYERS[0] * C5_LAYERS[1]
    # HBM-side bytes of the step from the committed PMC pass (tools/profile_r06.sh): every kernel of one step summed
    traffic, tstamp = None, None
    try:
        c5_file = next(f for f in ("r06_c5_pmc_hbm_traffic.json", "r05_c5_pmc_hbm_traffic.json", "r04_c5_pmc_hbm_traffic.json") if os.path.exists(os.path.join(ROOT, "profiles", f)))
        pm = json.load(open(os.path.join(ROOT, "profiles", c5_file)))
        tot, steps_prof = 0.0, None
        for k, v in pm["kernels"].items():
            if k.startswith(("void bp_gemm_bf16", "void bp_wgrad_dma_bf16", "bp_bias_bf16", "bp_to_bf16_both")) and "fetch_MB_corrected_x2" in v and "write_MB" in v:
                tot += (v["fetch_MB_corrected_x2"] + v["write_MB"]) * 1e6 * v["launches"]
                if k.startswith("void bp_wgrad_dma_bf16") and ("false" in k or "_six" in k):
                    steps_prof = v["launches"]                     # ONE grouped wgrad launch per step
        if steps_prof:
            note = pm.get("note", "")
            st = note.split("sha256[:16] ")[1].split(";")[0] if "sha256[:16] " in note else None
            traffic = tot / steps_prof
            tstamp = {"source": "profiles/" + c5_file, "sources_sha": st, "matches_current_kernel_sources": st == kernel_source_stamp() if st else None}
    except Exception:
        pass
    return {"workload": "configs[4] per-GPU shape: 2827->4096x5->257, 512 frames/GPU/step, bf16 operands, fp32 master W/delta, 1 GPU",
            "dtype": "bf16", "ms_per_step": 1e3 * dt, "value": C5_BUNCH / dt, "unit": "frames/s",
            "roofline": {"bound": "hbm", "achieved": alg / dt / 1e9, "peak": PEAK_HBM_GBS, "unit": "GB/s",
                         "frac": alg / dt / 1e9 / PEAK_HBM_GBS, "algorithmic_bytes_per_step": alg, "traffic": traffic, "traffic_stamp": tstamp},
            "frac_of_bf16_mfma_peak": flops_per_frame(C5_LAYERS) * C5_BUNCH / dt / 2.5e15}


C3_LAYERS = [257 * 12, 2048, 2048, 2048, 257]               # BASELINE.json configs[2]: 11 stacked frames + the appended noise estimate (NAT)


def _timed_resident(g, bunch, chunk, steps, warm=80):
    nb = chunk // bunch
    done = 0
    while done < warm:
        k = min(nb, warm - done); g.train_resident(0, k * bunch); done += k
    g.sync()
    t0 = time.perf_counter()
    done = 0
    while done < steps:
        k = min(nb, steps - done); g.train_resident(0, k * bunch); done += k
    g.sync()
    return (time.perf_counter() - t0) / steps


def c3_line(dnnse_amd, dev, steps=600):
    """BASELINE.json configs[2] (C3): the C2 net with the noise-aware input (3084 wide = 11 x 257 + 257; what makes the
    width: Interface.cc:759-787), ReLU, NO dropout, 256 frames per step, fp32, one GPU; BASELINE.md ceiling 2.00 M frames/s."""
    W, b = dnnse_amd.glorot_net(C3_LAYERS, seed=1, beta=0.5)
    chunk = 100 * BUNCH
    g = dnnse_amd.BP_GPU(1, len(C3_LAYERS), C3_LAYERS, BUNCH, 1.0, 0.5, 0.0, W, b, device=dev, max_chunk_frames=chunk)
    g.fill_chunk_synthetic(chunk, 20260927)
    dt = _timed_resident(g, BUNCH, chunk, steps)
    g.close()
    return {"workload": "configs[2] C3: 3084->2048->2048->2048->257 ReLU (noise-aware input, no dropout), fp32, 256 frames/step, resident chunk, 1 GPU",
            "dtype": "f32", "ms_per_step": 1e3 * dt, "value": BUNCH / dt, "unit": "frames/s", "steps": steps,
            "step_frac_of_mfma_peak": flops_per_frame(C3_LAYERS) * BUNCH / dt / 1e12 / PEAK_MFMA_F32_TF}


def windows_line(dnnse_amd, dev, n=51200, reps=3):
    """What `bptrain` really runs: C2 trained from RAW frames + index tables (bp_train_chunk_windows; every bunch
    stacks and masks its own rows on the device, bp_stage_bunch) -- wall clock per chunk INCLUDING the upload, best of `reps`."""
    D, ctx = 257, 11
    rs = np.random.default_rng(3)
    W, b = dnnse_amd.glorot_net(LAYERS, seed=1, beta=0.5)
    n_frames = n + 4000
    fea = rs.standard_normal((n_frames, D), dtype=np.float32)
    tg = rs.standard_normal((n_frames, D), dtype=np.float32)
    ws = rs.integers(0, n_frames - ctx + 1, size=n).astype(np.int32)
    tf = (ws + ctx // 2).astype(np.int32)
    g = dnnse_amd.BP_GPU(1, len(LAYERS), LAYERS, BUNCH, 0.001, 0.5, 0.0, W, b, device=dev, max_chunk_frames=n, dropoutflag=1,
                         visible_omit=0.1, hid_omit=0.2, seed=1)
    times = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        g.train_windows(fea, tg, ctx, ws, tf)
        g.sync()
        times.append(time.perf_counter() - t0)
    g.close()
    best = min(times[1:])
    return {"workload": "C2 from a window chunk: %d samples as raw frames (%d x 257) + index tables, stacked + masked per bunch on the device; "
                        "upload included (pageable host memory)" % (n, n_frames),
            "dtype": "f32", "s_per_chunk_incl_upload": best, "value": n / best, "unit": "frames/s", "ms_per_bunch": 1e3 * best / (n // BUNCH)}


def dp_world1_line(dnnse_amd, dev, W, b, steps=600):
    """C2 through the data-parallel exchange path with a group of ONE rank (all that one GPU can time): gradient store ->
    flags -> sharded update on the exchange stream -> weights gathered before the next forward (bp_dp_attach), against the
    fused single-device step.  The gap is what the exchange machinery costs before any byte crosses xGMI.  The line is the default
    exchange (reduce-scatter by peer reads); `push_form` beside it is the same step with the reduce-scatter by peer writes
    (transport 2), which at world 1 pays one more pass over the gradient segments (local copy into the receive slot)."""
    chunk = 100 * BUNCH
    out = {}
    for name, tr in (("pull", 0), ("push", 2)):
        g = dnnse_amd.BP_GPU(1, len(LAYERS), LAYERS, BUNCH, 1.0, 0.5, 0.0, W, b, device=dev, max_chunk_frames=chunk, dropoutflag=1,
                             visible_omit=0.1, hid_omit=0.2, seed=20260927, global_bunchsize=BUNCH, rank_frame_offset=0)
        g.dp_attach(1, 0, "bench-w1-%s-%d-%d" % (name, os.getpid(), int(time.time())), transport=tr)
        g.fill_chunk_synthetic(chunk, 20260927)
        out[name] = _timed_resident(g, BUNCH, chunk, steps)
        g.dp_detach()
        g.close()
    dt = out["pull"]
    return {"workload": "C2 (as the headline line) through the in-library exchange path, world size 1, 1 GPU", "dtype": "f32",
            "ms_per_step": 1e3 * dt, "value": BUNCH / dt, "unit": "frames/s", "steps": steps,
            "push_form": {"ms_per_step": 1e3 * out["push"], "value": BUNCH / out["push"], "unit": "frames/s"}}


def c1_end_to_end_line():
    """BASELINE.json configs[0] (the plumbing configuration): 1x512 Sigmoid net on 257-bin single-frame input, 128-frame
    minibatches, END TO END through the reference's file formats -- synthetic Pfile pair -> reader / chunker / shuffle ->
    the BPtrain-compatible binary -> trainer -> .wts file.  (The reference has no CPU trainer; here the step
    itself runs on the MI355X and the host half is the part that is pinned byte for byte to the reference.)"""
    import re
    import struct
    import subprocess
    import tempfile
    exe = os.path.join(ROOT, "dnn-for-speech-enhancement_amd", "bptrain")
    D, nsent, flen = 257, 120, 300
    rs = np.random.default_rng(3)
    n = nsent * flen

    def write_pfile(path, data):
        hdr = ("-pfile_header version 0 size 32768\n-num_sentences %d\n-num_frames %d\n-first_feature_column 2\n"
               "-num_features %d\n-end\n" % (nsent, n, data.shape[1])).encode()
        rec = np.empty((n, data.shape[1] + 2), dtype=">u4")
        rec[:, 0] = np.repeat(np.arange(nsent), flen); rec[:, 1] = np.tile(np.arange(flen), nsent)
        rec[:, 2:] = data.astype(">f4").view(">u4")
        with open(path, "wb") as f:
            f.write(hdr + b"\0" * (32768 - len(hdr))); f.write(rec.tobytes())
            f.write((np.arange(nsent + 1) * flen).astype(">i4").tobytes())

    with tempfile.TemporaryDirectory() as td:
        fea = rs.standard_normal((n, D), dtype=np.float32)
        write_pfile(os.path.join(td, "f.pfile"), fea); write_pfile(os.path.join(td, "t.pfile"), rs.standard_normal((n, D), dtype=np.float32))
        with open(os.path.join(td, "n.norm"), "w") as f:
            f.write("<mean>\n" + "".join("%.9g\n" % v for v in fea.mean(0)) + "<inverse std>\n" + "".join("%.9g\n" % v for v in 1.0 / fea.std(0)))
        args = ["fea_file=%s/f.pfile" % td, "targ_file=%s/t.pfile" % td, "norm_file=%s/n.norm" % td, "outwts_file=%s/w" % td,
                "log_file=%s/log" % td, "train_sent_range=0-%d" % (nsent - 11), "cv_sent_range=%d-%d" % (nsent - 10, nsent - 1),
                "fea_dim=257", "fea_context=1", "targ_offset=0", "dropoutflag=0", "traincache=16384", "bunchsize=128", "gpu_used=1",
                "init_randem_seed=1", "momentum=0.5", "weightcost=0", "lrate=0.01", "visible_omit=0", "hid_omit=0",
                "layersizes=257,512,257", "activation=sigmoid", "momentum_rule=classic"]
        t0 = time.perf_counter()
        r = subprocess.run([exe] + args, capture_output=True, text=True)
        wall = time.perf_counter() - t0
        txt = open(os.path.join(td, "log")).read()
        m = re.search(r"Training pass: (\d+) samples in ([0-9.]+) s", txt)
        wts = os.path.getsize(os.path.join(td, "w"))
    return {"workload": "configs[0] C1: 257->512->257 Sigmoid, 128-frame minibatches, synthetic Pfile pair (120 x 300 frames) -> bptrain -> .wts",
            "returncode_1_is_success": r.returncode, "train_samples": int(m.group(1)) if m else None,
            "frames_per_s_reader_upload_gpu": (int(m.group(1)) / float(m.group(2))) if m and float(m.group(2)) > 0 else None,
            "process_wall_s": wall, "wts_bytes": wts}


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--prewarm-s", type=float, default=1.5, help="seconds of real untimed training steps before the warm-up")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline does not need: sustained rate, in-step roofline, measured peaks, this run's own "
                         "rocprofv3 passes, the other configurations and the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write the weights and biases the last timed step left as DIR/W<l>.npy, DIR/b<l>.npy "
                         "(float32; one process only)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip the C5 line, the measured peaks and the live counter passes")
    ap.add_argument("--sustained-s", type=float, default=4.0, help="with --full: seconds of the additional sustained-rate measurement (0 = skip)")
    ap.add_argument("--chunk", type=int, default=CHUNK)
    ap.add_argument("--exchange", choices=["all", "both", "native", "native_push", "native_push_bf16", "rccl"], default="all",
                    help="transport of the data-parallel exchange (N > 1): the library's peer kernels, RCCL reduce-scatter/all-gather, or "
                         "(default) BOTH timed back to back in this one run, the faster one being the line's value")
    ap.add_argument("--force-dp", action="store_true", help="run the exchange path at N = 1 (world-1 group)")
    ap.add_argument("--launch-check", action="store_true",
                    help="only launch the N ranks, let them meet through the rendezvous and walk the transport-selection flow with "
                         "stand-in timings (no GPU work; CPU-testable)")
    return ap.parse_args()


def launch_ranks(args):
    """`python bench.py --gpus N` without a launcher around it: fork the N ranks ourselves, one process per GPU (rank r
    on device r % visible devices), the way `bptrain gpu_used=N` does (donor of the shape: the reference drives its G
    devices from one host, BP_GPU.cu:29-36,269-277).  The ranks find each other through the library's shared-memory
    rendezvous; rank 0 prints the JSON line, which is passed through as this process's last stdout line."""
    import subprocess
    key = "bench-%d-%d" % (os.getpid(), int(time.time()))
    procs = []
    for r in range(args.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.gpus), BENCH_KEY=key, BENCH_SELF_LAUNCHED="1")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=subprocess.PIPE if r == 0 else None))
    out0 = procs[0].communicate()[0].decode(errors="replace")
    rcs = [p.wait() for p in procs]
    sys.stdout.write(out0)
    sys.stdout.flush()
    if any(rcs):
        sys.stderr.write("bench.py: rank exit codes %s\n" % rcs)
        sys.exit(1)


def choose(out):
    ok = {k: v for k, v in out.items() if isinstance(v, dict) and "ms_per_step" in v}
    return min(ok, key=lambda k: ok[k]["ms_per_step"]) if ok else None


def run_exchanges(plan, attach, detach, timed, group_failed, guard=None):
    """The N > 1 flow: every transport in `plan` is attached AS A GROUP (a failure seen by one rank alone -- a timeout, a
    self-test verdict -- is all-gathered first, so the ranks always agree on what runs next: ADVICE r3), timed, detached.
    Returns ({transport: timing dict | {"error": ...}}, chosen transport or None).  The callbacks are the GPU-side pieces;
    --launch-check passes stand-ins, which is how this control flow is covered on the CPU (tests/test_bench_host.py).
    guard(tr, out_so_far) -> cancel(): armed around every transport AFTER one has already been timed -- a collective library
    that hangs in its bootstrap must not cost the run the number it already has (the watchdog prints the line and ends the rank)."""
    out = {}
    for tr in plan:
        have = choose(out) is not None
        cancel = guard(tr, dict(out)) if (guard and have) else None
        try:
            err = attach(tr)                              # None, or this rank's error text
            n_failed = group_failed(tr, err)
            if n_failed:
                if err is None:
                    detach(tr, broken=True)               # attached here, but a peer was not: leave that group
                out[tr] = {"error": "attach failed on %d rank(s): %s" % (int(n_failed), err or "on a peer")}
                continue
            out[tr] = timed(tr)
            detach(tr, broken=False)
        except Exception as e:                            # noqa: BLE001
            # a later transport that RAISES (a timeout inside timed()/detach(), the verdict rendezvous) must not cost the run the
            # number an earlier one already has; with nothing measured yet there is nothing to protect: propagate
            if not have:
                raise
            out[tr] = {"error": "%s: %s" % (type(e).__name__, e)}
        finally:
            if cancel:
                cancel()
    return out, choose(out)


def live_pmc(counters, timeout_s=150.0):
    """One `rocprofv3 --pmc <counters>` pass over a short run of THIS script (C2 headline steps, no extras), on this box, now:
    {"<kernel> grid=<n>": {counter: median over launches}} or None.  Separate passes per counter set and no tracing next to
    --pmc, as MI355X_MICROARCH.md prescribes."""
    import csv
    import glob
    import shutil
    import statistics
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return None
    with tempfile.TemporaryDirectory(dir="/tmp") as td:
        cmd = [exe, "--pmc"] + list(counters) + ["--output-format", "csv", "-d", td, "-o", "p", "--", sys.executable, os.path.abspath(__file__),
                                                 "--steps", "10", "--warmup", "5", "--no-cpu-baseline", "--no-extras", "--prewarm-s", "0",
                                                 "--sustained-s", "0", "--chunk", "5120"]
        env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
        env["TMPDIR"] = "/tmp"
        try:
            subprocess.run(cmd, cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=timeout_s)
        except Exception:
            return None
        acc = {}
        for f in glob.glob(os.path.join(td, "**", "*counter_collection.csv"), recursive=True):
            for r in csv.DictReader(open(f)):
                k = "%s grid=%s" % (r["Kernel_Name"].split("(")[0], r.get("Grid_Size", "?"))
                acc.setdefault(k, {}).setdefault(r["Counter_Name"], []).append(float(r["Counter_Value"]))
    return {k: {c: statistics.median(v) for c, v in cs.items()} for k, cs in acc.items()} or None


def live_kernel_stats(timeout_s=150.0):
    """One `rocprofv3 --kernel-trace --stats` pass over a short run of THIS script (the C2 headline steps, no extras), on this box, now:
    {kernel name: (average ns, calls)} or None.  The HEADLINE roofline figure is the dominant kernel's average from this pass."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return None
    with tempfile.TemporaryDirectory(dir="/tmp") as td:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", td, "-o", "kt", "--", sys.executable, os.path.abspath(__file__),
               "--steps", "200", "--warmup", "20", "--no-cpu-baseline", "--no-extras", "--prewarm-s", "0.5", "--sustained-s", "0", "--chunk", "5120"]
        env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
        env["TMPDIR"] = "/tmp"
        try:
            subprocess.run(cmd, cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=timeout_s)
        except Exception:
            return None
        out = {}
        for f in glob.glob(os.path.join(td, "**", "*kernel_stats.csv"), recursive=True):
            for r in csv.DictReader(open(f)):
                out[r["Name"]] = (float(r["AverageNs"]), int(r["Calls"]))
    return out or None


def _pick(pmc, pred):
    for k, v in (pmc or {}).items():
        if pred(k):
            return k, v
    return None, None


def live_counters():
    """HBM-side traffic of the dominant launch and counter-based MFMA utilisation, measured in THIS run:
    three short rocprofv3 --pmc passes (FETCH_SIZE | WRITE_SIZE | SQ_VALU_MFMA_BUSY_CYCLES + SQ_BUSY_CU_CYCLES)."""
    is_wgrad = lambda k: k.startswith("void bp_wgrad_dma<16, 4, 4, 256, false>")          # noqa: E731
    is_hidden = lambda k: k.startswith("void bp_gemm<32, 64, 64, 1, 2, true, false, 0, 0>")   # noqa: E731  (EPI 0 = hidden forward, TAG 0 = layers 2..L-2)
    out = {}
    ks = live_kernel_stats()
    if ks:
        k = next((n for n in ks if is_wgrad(n)), None)
        if k:
            out["wgrad_kernel_ns"] = ks[k][0]
            out["wgrad_kernel_calls"] = ks[k][1]
        out["kernel_avg_us"] = {n.split("(")[0][:72]: round(v[0] * 1e-3, 3) for n, v in ks.items() if v[1] >= 100}
        kh = next((n for n in ks if is_hidden(n)), None)
        if kh:
            out["hidden_kernel_ns"] = ks[kh][0]
    fe, wr = live_pmc(["FETCH_SIZE"]), live_pmc(["WRITE_SIZE"])
    kf, vf = _pick(fe, is_wgrad)
    kw, vw = _pick(wr, is_wgrad)
    if vf and vw and "FETCH_SIZE" in vf and "WRITE_SIZE" in vw:
        out["traffic_bytes"] = (2.0 * vf["FETCH_SIZE"] + vw["WRITE_SIZE"]) * 1024.0       # KB units; FETCH doubled (gfx950 note in the guide)
        out["traffic_detail"] = {"kernel": kf, "FETCH_SIZE_KB_median": vf["FETCH_SIZE"], "WRITE_SIZE_KB_median": vw["WRITE_SIZE"],
                                 "how": "rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE, separate passes of `bench.py --steps 10 --warmup 5 --no-extras` "
                                        "run by this process on this box; FETCH_SIZE doubled per MI355X_MICROARCH.md (gfx950 tallies wide reads at half)"}
    sq = live_pmc(["SQ_VALU_MFMA_BUSY_CYCLES", "SQ_BUSY_CU_CYCLES"])
    util = {}
    for name, pred in (("hidden_fwd_2048x2048", is_hidden), ("wgrad_update_grouped", is_wgrad)):
        k, v = _pick(sq, pred)
        if v and v.get("SQ_BUSY_CU_CYCLES"):
            util[name] = {"kernel": k, "mfma_busy_frac": v["SQ_VALU_MFMA_BUSY_CYCLES"] / (4.0 * v["SQ_BUSY_CU_CYCLES"]),
                          "SQ_VALU_MFMA_BUSY_CYCLES": v["SQ_VALU_MFMA_BUSY_CYCLES"], "SQ_BUSY_CU_CYCLES": v["SQ_BUSY_CU_CYCLES"]}
    if util:
        out["mfma_util"] = util
        out["mfma_util_how"] = ("SQ_VALU_MFMA_BUSY_CYCLES / (4 SIMDs x SQ_BUSY_CU_CYCLES): the fraction of SIMD-cycles of BUSY CUs with an MFMA in "
                                "flight (rocprofv3's derived MfmaUtil divides by GRBM_GUI_ACTIVE, which under PMC serialisation includes dispatch idle)")
    return out


def committed_mfma_util():
    """profiles/r05_mfma_util.json (tools/pmc_sq_summary.py): the same ratio from the committed SQ pass, with its source stamp."""
    try:
        name = next(f for f in ("r06_mfma_util.json", "r05_mfma_util.json") if os.path.exists(os.path.join(ROOT, "profiles", f)))
        j = json.load(open(os.path.join(ROOT, "profiles", name)))
        return {"source": "profiles/" + name, "sources_sha": j.get("sources_sha"),
                "matches_current_kernel_sources": j.get("sources_sha") == kernel_source_stamp(), "kernels": j.get("kernels")}
    except Exception:
        return None


def make_guard(rank, make_line):
    """Watchdog around a further transport once one has been timed (run_exchanges): after BENCH_WATCHDOG_S seconds (default 330:
    clearly MORE than the library's attach budget BP_DP_TIMEOUT_S = 120 s plus the 120 s of the verdict rendezvous, so that a peer
    that merely times out surfaces as an exception -- caught by run_exchanges -- and the watchdog is left for real hangs)
    rank 0 prints the line from what was measured before, every rank ends.  A thread, not a signal: the hang this is for sits
    inside a foreign call (a collective library's bootstrap), where Python never gets to run a signal handler."""
    import threading
    limit = float(os.environ.get("BENCH_WATCHDOG_S", "330"))

    def guard(tr, out_so_far):
        def fire():
            out = dict(out_so_far)
            out[tr] = {"error": "no result within %.0f s (watchdog); the line reports what was measured before it" % limit}
            if rank == 0:
                try:
                    import ctypes
                    ctypes.CDLL(None).fflush(None)
                except Exception:
                    pass
                print(json.dumps(make_line(out, choose(out))), flush=True)
            os._exit(0)
        t = threading.Timer(limit, fire)
        t.daemon = True
        t.start()
        return t.cancel
    return guard


def main():
    args = parse_args()
    if args.gpus < 1:
        sys.exit("bench.py: --gpus must be >= 1")
    if args.dump_outputs and (args.gpus > 1 or args.force_dp or os.environ.get("BENCH_FORCE_DP") == "1"):
        # a group's handle is attached and timed once per transport: its last step is not one fixed computation
        sys.exit("bench.py: --dump-outputs needs one process without the exchange path (--gpus 1, no --force-dp)")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return launch_ranks(args)                              # no launcher around us: become one
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", str(rank)))
    if world != args.gpus:
        # never print an N-GPU line from fewer ranks (or the other way round)
        sys.exit("bench.py: --gpus %d but WORLD_SIZE=%d: launch with --nproc-per-node equal to --gpus, or with no launcher at all" % (args.gpus, world))
    # the job's rendezvous key: ours when self-launched, else derived from what every rank of a torch.distributed.run
    # launch shares (master port + the agent's pid)
    key = os.environ.get("BENCH_KEY") or "bench-%s-%d" % (os.environ.get("MASTER_PORT", "0"), os.getppid() if world > 1 else os.getpid())

    import dnnse_amd

    dp = world > 1 or args.force_dp or os.environ.get("BENCH_FORCE_DP") == "1"
    # N > 1: every exchange the library has, timed in ONE run -- native (reduce-scatter by peer reads), native_push (by peer writes into
    # the owners' receive buffers), rccl; "both" = the two of round 5 (native, rccl).  native_push_bf16 (gradient segments rounded to bf16
    # on the way out: half the bytes, NOT result-equivalent) only on request: it must never become `chosen` by being faster
    every = ["native", "native_push", "rccl"]
    plan = (every if args.exchange == "all" else (["native", "rccl"] if args.exchange == "both" else [args.exchange])) if world > 1 else \
        (["native" if args.exchange in ("all", "both") else args.exchange] if dp else [])

    def group_failed(tr, err):
        """how many ranks failed to attach `tr` (every rank gets the same answer)"""
        if world == 1:
            return 1 if err else 0
        rv = dnnse_amd.Rendezvous("%s-verdict-%s" % (key, tr), world, rank, timeout_s=120.0)
        n = sum(rv.allgather_f64(1.0 if err else 0.0))
        rv.close()
        return n

    if args.launch_check:
        rv = dnnse_amd.Rendezvous(key + "-lc", world, rank, timeout_s=60.0)
        pids = rv.allgather_f64(float(os.getpid()))
        rv.barrier()
        # the transport-selection flow with stand-ins for the GPU side: BENCH_FAKE_FAIL="native:1" makes rank 1's native attach
        # fail, BENCH_FAKE_MS="native:0.31,rccl:0.29" are the stand-in step times
        fail_spec = dict(x.split(":") for x in os.environ.get("BENCH_FAKE_FAIL", "").split(",") if ":" in x)
        ms_spec = {k: float(v) for k, v in (x.split(":") for x in os.environ.get("BENCH_FAKE_MS", "native:0.30,rccl:0.35").split(",") if ":" in x)}
        hang_spec = dict(x.split(":") for x in os.environ.get("BENCH_FAKE_HANG", "").split(",") if ":" in x)   # "rccl:1": rank 1 never returns from attaching rccl
        log = []

        def lc_line(ex, chosen):
            return {"launch_check": True, "n_gpus": world, "ranks": list(range(world)), "pids": [int(p) for p in pids],
                    "self_launched": os.environ.get("BENCH_SELF_LAUNCHED") == "1", "exchange": dict(ex, chosen=chosen), "detaches": log}

        def lc_attach(tr):
            if hang_spec.get(tr) == str(rank):
                time.sleep(1e6)
            return "stand-in failure" if fail_spec.get(tr) == str(rank) else None
        raise_spec = dict(x.split(":") for x in os.environ.get("BENCH_FAKE_RAISE", "").split(",") if ":" in x)   # "rccl:0": rank 0's timed region of rccl raises

        def lc_timed(tr):
            if raise_spec.get(tr) == str(rank):
                raise RuntimeError("stand-in: exchange timed out on the device")
            return {"ms_per_step": ms_spec.get(tr, 1.0), "steps": args.steps}
        ex, chosen = run_exchanges(plan, attach=lc_attach,
                                   detach=lambda tr, broken: log.append(("detach", tr, broken)),
                                   timed=lc_timed,
                                   group_failed=group_failed, guard=make_guard(rank, lc_line))
        if rank == 0:
            print(json.dumps(lc_line(ex, chosen)), flush=True)
        rv.close()
        return

    import torch                                              # device synchronisation only; no torch.distributed anywhere

    ndev = dnnse_amd.device_count()
    dev = local_rank % max(ndev, 1)
    torch.cuda.set_device(dev)
    if world > 1:
        # the ranks of a fresh box can come out of their first `import torch` tens of seconds apart: meet here (host only, generous
        # budget) so that they enter the group attach -- whose budget is the library's -- together
        rv0 = dnnse_amd.Rendezvous(key + "-start", world, rank, timeout_s=900.0)
        rv0.barrier()
        rv0.close()

    W, b = dnnse_amd.glorot_net(LAYERS, seed=1, beta=0.5)    # Gen_rand_net flag=1, beta=0.5 recipe
    chunk = max(BUNCH, (args.chunk // BUNCH) * BUNCH)
    kw = dict(dropoutflag=1, visible_omit=0.1, hid_omit=0.2, seed=20260927, device=dev, max_chunk_frames=chunk)
    if dp:
        kw.update(global_bunchsize=BUNCH * world, rank_frame_offset=rank * BUNCH)

    def new_handle():
        h = dnnse_amd.BP_GPU(world, len(LAYERS), LAYERS, BUNCH, 1.0, 0.5, 0.0, W, b, **kw)
        h.fill_chunk_synthetic(chunk, 20260927 + rank)        # each rank holds its own shard of every bunch
        h.sync()
        return h

    g = new_handle()
    nb_chunk = chunk // BUNCH
    state = {"pos": 0, "attached": False}

    def barrier():
        g.sync()
        torch.cuda.synchronize(dev)
        if state["attached"]:
            g.dp_barrier()                                    # host barrier of the group's rendezvous block

    def max_over_ranks(v):
        return max(g.dp_allgather_f64(v, world)) if state["attached"] else v

    def run(nsteps):
        done, pos = 0, state["pos"]
        while done < nsteps:
            k = min(nsteps - done, nb_chunk - pos)
            g.train_resident(pos * BUNCH, k * BUNCH)
            done += k
            pos = (pos + k) % nb_chunk
        state["pos"] = pos

    def prewarm():
        """untimed pre-warm on g: real steps for --prewarm-s seconds, the same count on every rank -> (seconds, steps)"""
        t0, prewarm_steps = time.perf_counter(), 0
        if args.prewarm_s > 0:
            run(200); g.sync(); prewarm_steps = 200
            per = (time.perf_counter() - t0) / 200
            extra = int(max_over_ranks(float(int(max(0.0, args.prewarm_s - (time.perf_counter() - t0)) / per))))
            if extra > 0:
                run(extra); g.sync(); prewarm_steps += extra
        return time.perf_counter() - t0, prewarm_steps

    warmed = None
    if not dp and args.prewarm_s > 0:
        # The pre-warm's step count follows the clock, so it runs on a handle of its own; the timed handle g, made before it so
        # that the GPU does not idle in between, gets a fixed PREWARM_FIXED_STEPS instead (after an idle pause the step needs
        # ~75 steps to come back to speed).  The last timed step is then the same computation in every run with these
        # arguments (--dump-outputs), whatever the clock did.
        timed_g, g = g, new_handle()
        prewarm_s, prewarm_steps = prewarm()
        g.close()
        g, state["pos"] = timed_g, 0
        t0 = time.perf_counter()
        run(PREWARM_FIXED_STEPS); g.sync()
        warmed = (prewarm_s + time.perf_counter() - t0, prewarm_steps + PREWARM_FIXED_STEPS)

    def dump_outputs(d):
        """--dump-outputs: what a caller of the timed step receives after its last step -- the trained weights W<l> [in][out]
        and biases b<l>, l = 1..L-1 (returnWeights), float32: 14.7 M values, 59 MB for C2"""
        os.makedirs(d, exist_ok=True)
        ws, bs = g.get_weights()
        for l in range(1, len(LAYERS)):
            np.save(os.path.join(d, "W%d.npy" % l), ws[l])
            np.save(os.path.join(d, "b%d.npy" % l), bs[l])

    def timed(tr=None):
        """untimed pre-warm (real steps, the same count on every rank), W warm-up steps, EXACTLY K timed steps between barriers"""
        prewarm_s, prewarm_steps = warmed if warmed is not None else prewarm()
        run(args.warmup)
        barrier()
        t0 = time.perf_counter()
        run(args.steps)
        barrier()
        dt = max_over_ranks(time.perf_counter() - t0)
        r = {"ms_per_step": 1e3 * dt / args.steps, "value": args.steps * BUNCH * world / dt, "unit": "frames/s", "steps": args.steps,
             "prewarm_s": prewarm_s, "prewarm_steps": prewarm_steps, "dt": dt}
        if args.dump_outputs:
            dump_outputs(args.dump_outputs)
        if tr is not None:
            # what each rank attached to, as the library saw it: a reader can check N ranks on N devices
            table = []
            for p in range(world):
                pdev, pci, _tr, aq = g.dp_peer_info(p)
                table.append({"rank": p, "device": pdev, "pci_bus_id": pci})
            r.update(ranks=table, distinct_devices=len(set(x["pci_bus_id"] for x in table)), dp_acquire_mode=g.dp_peer_info(0)[3],
                     dp_handoff="tile counters inside the wgrad launch" if g.dp_handoff() else "event + kernel boundary")
            dp_world, dp_rank, _ = g.dp_info()
            assert dp_world == world and dp_rank == rank
        # ---- sustained rate (an extra field, not `value`): the same steps for --sustained-s seconds, so that clocks, power and
        # temperature are at their steady state -- and so that whoever samples the GPU's busy counter during this run sees it
        if args.full and args.sustained_s > 0 and not args.no_extras:
            n_sus = int(max_over_ranks(float(max(1, int(args.sustained_s / (dt / args.steps))))))      # same count on every rank
            barrier()
            t1 = time.perf_counter()
            run(n_sus)
            barrier()
            dt_s = max_over_ranks(time.perf_counter() - t1)
            r["sustained"] = {"seconds": dt_s, "steps": n_sus, "value": n_sus * BUNCH * world / dt_s, "unit": "frames/s", "ms_per_step": 1e3 * dt_s / n_sus}
        return r

    def attach(tr):
        # The native exchange checks its memory-model assumptions on the group's real devices at attach and refuses to run when they
        # do not hold; RCCL may be missing or refuse the topology.  Either is reported in the line, never fatal while one transport works.
        try:
            g.dp_attach(world, rank, "%s-%s" % (key, tr), transport={"native": 0, "rccl": 1, "native_push": 2, "native_push_bf16": 3}[tr])
            state["attached"] = True
            return None
        except dnnse_amd.BPError as e:
            return str(e)[:200]

    def detach(tr, broken):
        state["attached"] = False
        try:
            g.dp_detach()
        except dnnse_amd.BPError:
            if not broken:                                    # (a broken group's closing barrier cannot complete: expected)
                raise

    def make_line(exchange, chosen, head=None):
        """the JSON line's common part; dp: from the transports timed so far (also what the watchdog prints)"""
        if head is None:
            head = exchange[chosen]
        res = {
            "metric": "training frames/sec (257x11 input, 3x2048 DNN)", "value": head["value"], "unit": "frames/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": head["ms_per_step"],
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "prewarm_s": head["prewarm_s"], "prewarm_steps": head["prewarm_steps"], "sustained": head.get("sustained"),
            "config": {"workload": "C2: 2827->2048->2048->2048->257 ReLU+dropout(0.1/0.2), fp32, %d frames/GPU/step "
                                   "(global bunch %d), lrate 1, momentum 0.5, %d-frame chunk resident in HBM"
                                   % (BUNCH, BUNCH * world, chunk),
                       "parallelism": "dp%d" % world, "frames_per_gpu_per_step": BUNCH, "global_bunch": BUNCH * world,
                       "exchange": ({"rccl": "RCCL reduce-scatter + sharded update + all-gather (bp_dp_attach_ex)",
                                     "native_push": "in-library hipIpc reduce-scatter by peer WRITES + sharded update + all-gather (bp_dp_attach_ex, push form)"}
                                    .get(chosen, "in-library hipIpc reduce-scatter by peer reads + sharded update + all-gather (bp_dp_attach)") if dp else "none"),
                       "launcher": "self (bench.py forked its ranks)" if os.environ.get("BENCH_SELF_LAUNCHED") == "1" else
                                   ("torch.distributed.run" if world > 1 else "single process")},
        }
        if dp:
            # north_star names RCCL; the library's default is its own peer kernels: ONE run answers which is faster here
            res["exchange"] = {k: ({kk: vv for kk, vv in v.items() if kk in ("ms_per_step", "value", "steps", "error", "dp_acquire_mode", "dp_handoff", "sustained")})
                               for k, v in exchange.items()}
            res["exchange"]["chosen"] = chosen
            res["exchange"]["note"] = "every transport listed was attached by the whole group and timed with the same protocol in this run; value = the faster one"
            res["ranks"] = head["ranks"]
            res["distinct_devices"] = head["distinct_devices"]
            res["dp_acquire_mode"] = head["dp_acquire_mode"]
        res["step_frac_of_mfma_peak"] = flops_per_frame(LAYERS) * head["value"] / world / 1e12 / PEAK_MFMA_F32_TF
        return res

    exchange, chosen = None, None
    if dp:
        exchange, chosen = run_exchanges(plan, attach, detach, timed, group_failed, guard=make_guard(rank, make_line))
        if chosen is None:
            raise dnnse_amd.BPError("no data-parallel transport could be attached: %s" % json.dumps(exchange))
        res = make_line(exchange, chosen)
    else:
        res = make_line(None, None, head=timed(None))
    value = res["value"]
    if rank == 0 and not dp and args.full:
        # ---- roofline of the TIME-DOMINANT kernel: the grouped wgrad + fused momentum update of all layers
        # (bp_wgrad_dma<16,4,4,256>, LDS-DMA staged, one grouped launch per step, ~35 % of the step).  achieved = algorithmic FLOPs per launch (2*B*P: every layer's G = y^T.dEdX) / its average duration
        # INSIDE the step, measured live with HIP events on the launch stream (bp_profile_step: an event after every
        # launch of 100 real training steps).  The rocprofv3 --kernel-trace --stats summary of this same command is
        # committed under profiles/ (its average for that kernel is the cross-check).
        prof = g.profile_step(0, min(100, nb_chunk))
        wg_ms = prof["wgrad_update_grouped"][0]
        wg_fl = wgrad_flops_per_step(LAYERS, BUNCH)
        ach = wg_fl / (wg_ms * 1e-3) / 1e12
        P = n_params(LAYERS)
        # algorithmic bytes of that launch: W and delta read + written (16P) + every layer's activations and dEdX read once
        alg_bytes = 16.0 * P + 4.0 * BUNCH * (sum(LAYERS[:-1]) + sum(LAYERS[1:]))
        # HBM-side bytes of that launch from the committed PMC pass (tools/profile_r06.sh), stamped with the kernel sources it was
        # taken on; replaced further down by THIS run's own counter passes when they succeed
        traffic, tstamp = None, None
        for name in ("r06_pmc_hbm_traffic.json", "r05_pmc_hbm_traffic.json", "r04_pmc_hbm_traffic.json"):
            traffic, tstamp = profiled_traffic(name, lambda k: "bp_wgrad_dma" in k and "bf16" not in k and "grid=" in k and int(k.split("grid=")[1]) > 500000)
            if traffic is not None:
                break
        # cross-check against the committed rocprofv3 --kernel-trace --stats summary of this same command
        rk_ms, rk_file = None, None
        try:
            import csv
            rk_file = next(f for f in ("r06_bench_kernel_stats.csv", "r05_bench_kernel_stats.csv", "r04_bench_kernel_stats.csv") if os.path.exists(os.path.join(ROOT, "profiles", f)))
            for row in csv.DictReader(open(os.path.join(ROOT, "profiles", rk_file))):
                if row["Name"].startswith("void bp_wgrad_dma<16, 4, 4, 256") and "true" not in row["Name"]:     # (the fused-update form)
                    rk_ms = float(row["AverageNs"]) * 1e-6
        except Exception:
            rk_ms = None
        # ONE headline definition: roofline.achieved / frac = algorithmic FLOPs of the dominant launch / its rocprofv3
        # --kernel-trace average / 157.3 TF -- from THIS run's own rocprofv3 pass when it succeeds (further down), else from the committed
        # summary of the same command, else (no profiler, no file) from the in-step events.  The in-step event figure (kernel + the ~3 us
        # dependent-launch boundary in front of it) is always reported beside it as `in_step_events`.
        ev = {"kernel_ms": wg_ms, "achieved": ach, "frac": ach / PEAK_MFMA_F32_TF,
              "measured_by": "HIP events inside 100 real steps on the launch stream (bp_profile_step): previous event -> own event, i.e. the kernel "
                             "plus the ~3 us dependent-launch boundary in front of it"}
        head_ms, head_src = (rk_ms, "profiles/%s (committed rocprofv3 --kernel-trace --stats average of the same command, another box)" % rk_file) if rk_ms \
            else (wg_ms, "in-step HIP events (no rocprofv3 figure available)")
        res["roofline"] = {
            "bound": "mfma", "kernel": "bp_wgrad_dma<16,4,4,256> (wgrad + fused momentum update of all 4 layers, one grouped launch per step)",
            "achieved": wg_fl / (head_ms * 1e-3) / 1e12, "peak": PEAK_MFMA_F32_TF, "unit": "TFLOP/s", "frac": wg_fl / (head_ms * 1e-3) / 1e12 / PEAK_MFMA_F32_TF,
            "definition": "algorithmic FLOPs of the launch (2*B*P) / rocprofv3 --kernel-trace average duration of the kernel / 157.3 TFLOP/s",
            "traffic": traffic, "traffic_stamp": tstamp, "algorithmic_flops": wg_fl, "algorithmic_bytes": alg_bytes,
            "kernel_ms": head_ms, "kernel_ms_source": head_src,
            "in_step_events": ev,
            "rocprof_committed": {"kernel_ms": rk_ms, "frac": (wg_fl / (rk_ms * 1e-3) / 1e12 / PEAK_MFMA_F32_TF) if rk_ms else None,
                                  "source": "profiles/%s" % rk_file if rk_ms else None},
            "kernels_in_step_ms": {k: v[0] for k, v in prof.items()}, "launches_per_step": {k: v[1] for k, v in prof.items()},
            "hidden_fwd_2048x2048": {"achieved": 2.0 * BUNCH * 2048 * 2048 / (prof["fwd_hidden"][0] * 1e-3) / 1e12,
                                     "frac": 2.0 * BUNCH * 2048 * 2048 / (prof["fwd_hidden"][0] * 1e-3) / 1e12 / PEAK_MFMA_F32_TF,
                                     "unit": "TFLOP/s", "note": "north_star's 2048x2048 hidden GEMM, in-step"},
            # skinny layers: achieved GB/s = 4*(prev*cur + B*prev + B*cur) / t, in-step
            "skinny_layers_GBs": {
                "fwd_l1_2827x2048": 4.0 * (LAYERS[0] * LAYERS[1] + BUNCH * (LAYERS[0] + LAYERS[1])) / (prof["fwd_l1"][0] * 1e-3) / 1e9,
                "fwd_out_2048x257": 4.0 * (LAYERS[-2] * LAYERS[-1] + BUNCH * (LAYERS[-2] + LAYERS[-1])) / (prof["fwd_out"][0] * 1e-3) / 1e9},
        }
        cm = committed_mfma_util()
        if cm:
            res["roofline"]["mfma_util_committed"] = cm
            hk = next((v for k, v in (cm.get("kernels") or {}).items() if k.startswith(("void bp_gemm<32, 64, 64, 1, 2, true, false, 0, 0>", "void bp_gemm<32, 64, 64, 1, 2, true, false, 0, 1, 0, 0>"))), None)
            if hk:
                res["roofline"]["hidden_fwd_2048x2048"]["mfma_busy_frac"] = hk.get("mfma_busy_frac")
                res["roofline"]["hidden_fwd_2048x2048"]["mfma_busy_frac_source"] = cm["source"]
        if not args.no_extras:
            # north_star's GEMM once more from BACK-TO-BACK launches of the same kernel (bp_time_kernel: no event between the
            # launches, so no serialised dispatch in the figure): the number to hold against ">= 60 %"
            try:
                hb = g.time_kernel(0, 400)
                db = g.time_kernel(1, 400)
                fl = 2.0 * BUNCH * 2048 * 2048
                res["roofline"]["hidden_fwd_2048x2048"]["back_to_back"] = {
                    "kernel_ms": hb, "achieved": fl / (hb * 1e-3) / 1e12, "frac": fl / (hb * 1e-3) / 1e12 / PEAK_MFMA_F32_TF, "unit": "TFLOP/s",
                    "note": "400 back-to-back launches of the hidden forward GEMM (bias + ReLU + Philox dropout epilogue), HIP events around the batch"}
                res["roofline"]["hidden_dgrad_2048x2048_back_to_back"] = {
                    "kernel_ms": db, "achieved": fl / (db * 1e-3) / 1e12, "frac": fl / (db * 1e-3) / 1e12 / PEAK_MFMA_F32_TF, "unit": "TFLOP/s"}
            except Exception as e:
                res["roofline"]["hidden_fwd_2048x2048"]["back_to_back"] = {"error": str(e)[:200]}
            mf, cp = g.measure_peaks()
            res["roofline"]["peak_measured"] = {"mfma_f32_TFLOPs": mf, "hbm_copy_GBs": cp,
                                                "frac_of_measured_mfma": res["roofline"]["achieved"] / mf if mf > 0 else None,
                                                "note": "bare v_mfma_f32_32x32x2_f32 loop and 1 GiB float4 copy, this device, this process"}
    g.close()
    if rank == 0 and not dp and args.full and not args.no_extras:
        # ---- THIS run's own counter passes (the handle is closed: the child processes have the GPU to themselves)
        try:
            lc = live_counters()
        except Exception as e:
            lc = {"error": str(e)[:200]}
        if lc.get("wgrad_kernel_ns"):
            rf = res["roofline"]
            rf["kernel_ms"] = lc["wgrad_kernel_ns"] * 1e-6
            rf["kernel_ms_source"] = ("rocprofv3 --kernel-trace --stats pass of `bench.py --steps 200 --warmup 20 --no-extras` run by this process on this box "
                                      "(%d launches)" % lc["wgrad_kernel_calls"])
            rf["achieved"] = rf["algorithmic_flops"] / (rf["kernel_ms"] * 1e-3) / 1e12
            rf["frac"] = rf["achieved"] / PEAK_MFMA_F32_TF
            rf["kernel_avg_us_this_run"] = lc.get("kernel_avg_us")
            if lc.get("hidden_kernel_ns"):
                # north_star's GEMM by the same definition: its rocprofv3 average INSIDE the training step (the in-step event figure,
                # which carries the launch boundary, moves to in_step_events)
                hf = rf["hidden_fwd_2048x2048"]
                hf["in_step_events"] = {"achieved": hf["achieved"], "frac": hf["frac"]}
                hf["kernel_ms"] = lc["hidden_kernel_ns"] * 1e-6
                hf["achieved"] = 2.0 * BUNCH * 2048 * 2048 / (hf["kernel_ms"] * 1e-3) / 1e12
                hf["frac"] = hf["achieved"] / PEAK_MFMA_F32_TF
                hf["note"] = "north_star's 2048x2048 hidden GEMM: rocprofv3 --kernel-trace average of the kernel inside the training step (this run's own pass)"
            if isinstance(rf.get("peak_measured"), dict) and rf["peak_measured"].get("mfma_f32_TFLOPs"):
                rf["peak_measured"]["frac_of_measured_mfma"] = rf["achieved"] / rf["peak_measured"]["mfma_f32_TFLOPs"]
        if lc.get("traffic_bytes"):
            res["roofline"]["traffic_committed"] = {"traffic": res["roofline"]["traffic"], "traffic_stamp": res["roofline"]["traffic_stamp"]}
            res["roofline"]["traffic"] = lc["traffic_bytes"]
            res["roofline"]["traffic_stamp"] = dict(lc["traffic_detail"], measured_in_this_run=True)
        if lc.get("mfma_util"):
            res["roofline"]["mfma_util"] = dict(lc["mfma_util"], how=lc["mfma_util_how"], measured_in_this_run=True)
            if "hidden_fwd_2048x2048" in lc["mfma_util"]:
                res["roofline"]["hidden_fwd_2048x2048"]["mfma_busy_frac"] = lc["mfma_util"]["hidden_fwd_2048x2048"]["mfma_busy_frac"]
                res["roofline"]["hidden_fwd_2048x2048"]["mfma_busy_frac_source"] = "rocprofv3 --pmc pass of this run"
        if "error" in lc:
            res["roofline"]["live_counters_error"] = lc["error"]
        try:
            res["c5_bf16"] = c5_line(dnnse_amd, dev)
        except Exception as e:
            res["c5_bf16"] = {"error": str(e)[:300]}
        try:
            res["c1_end_to_end"] = c1_end_to_end_line()
        except Exception as e:
            res["c1_end_to_end"] = {"error": str(e)[:300]}
        for name, fn in (("c3_nat", lambda: c3_line(dnnse_amd, dev)), ("c2_window_chunk", lambda: windows_line(dnnse_amd, dev)),
                         ("dp_world1", lambda: dp_world1_line(dnnse_amd, dev, W, b))):
            try:
                res[name] = fn()
            except Exception as e:
                res[name] = {"error": str(e)[:300]}
        if isinstance(res.get("dp_world1"), dict) and "ms_per_step" in res["dp_world1"]:
            res["dp_world1"]["vs_fused_step"] = res["dp_world1"]["ms_per_step"] / res["ms_per_step"]
    if rank == 0:
        if world == 1 and not dp and args.full and not args.no_cpu_baseline:
            res["cpu_baseline"] = cpu_baseline(W, b)
        try:                                   # anything native code left in C stdio goes out first,
            import ctypes                      # so that the JSON line is the last thing on stdout
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
