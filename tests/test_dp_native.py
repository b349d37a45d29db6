"""In-library data-parallel exchange (bp_dp_attach: hipIpc reduce-scatter + sharded fused update +
all-gather behind the C ABI) with N PROCESSES SHARING ONE GPU -- the functional test of
BASELINE.json configs[3] that fits a 1-GPU box: C4's real shape is 8 ranks x 256 frames, global
bunch 2048.  A run of the suite keeps at most MAX_RANKS rank processes on the GPU at once (with the
test process itself, at most six processes hold the device), so configs[3]'s global bunch of 2048
frames runs here as 4 ranks x 512 frames.  Checks: every rank ends with bit-identical weights AND (gathered) momentum state, and
that state equals the oracle trained on the GLOBAL bunch within 1e-4 (only the summation order of
the gradient differs; reference semantics: BP_GPU.cu:775-908)."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from util import TOL, relerr
from flip_accounting import K_FP64, fp64_bounded

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
MAX_RANKS = 4          # rank processes with the GPU open at one time (the test process holds it too)
sys.path.insert(0, HERE)

CASES = [
    # name, layersizes, local B, world, global bunches, extras
    ("tiny2", [12, 7, 5, 3], 4, 2, 4, {}),
    ("odd3_dropout_unaligned", [70, 65, 130, 33], 25, 3, 3, {"drop": True, "wc": 0.01, "act": 1, "tail": 31}),   # bunch 75: offsets 25, 50
    # the same net under a weight cost and a momentum that matter (tests/update_cases.py says why wc 0.01 at m 0.5 does not bind): the
    # weights | biases boundary inside a segment of the sharded update, rule 1
    ("odd3_wc_rule1", [70, 65, 130, 33], 25, 3, 3, {"act": 1, "rule": 1, "m": 0.9, "wc": 0.0625}),
    ("nat4_classic", [1548, 256, 192, 129], 16, 4, 4, {"drop": True, "rule": 1}),
    ("c4_4x512", [2827, 2048, 2048, 2048, 257], 512, 4, 2, {"beta": 0.5}),           # configs[3]'s net and global bunch, 4 ranks
    # configs[3]'s net and global bunch on 4 ranks, SIX global minibatches at lrate 0.02: outputs, weights and biases at PLAIN 1e-4 against the oracle with no
    # fp64 clause at all ("plain"); the momentum state (flip effect, independent of lrate) faces the strict same-library check only
    ("c4_4x512_small_lrate", [2827, 2048, 2048, 2048, 257], 512, 4, 6, {"beta": 0.5, "lr": 0.02, "plain": True}),
    ("c2_world1", [2827, 2048, 257], 256, 1, 2, {"drop": True}),                     # exchange path with a single rank
    # BP_DP_TRANSPORT_NATIVE_PUSH (transport 2): the reduce-scatter by peer WRITES into the owners' receive buffers
    ("push_tiny2", [12, 7, 5, 3], 4, 2, 4, {"transport": 2}),
    ("push_odd3_dropout_unaligned", [70, 65, 130, 33], 25, 3, 3, {"drop": True, "wc": 0.01, "act": 1, "tail": 31, "transport": 2}),
    ("push_odd3_wc_rule1", [70, 65, 130, 33], 25, 3, 3, {"act": 1, "rule": 1, "m": 0.9, "wc": 0.0625, "transport": 2}),
    ("push_c4_4x512", [2827, 2048, 2048, 2048, 257], 512, 4, 2, {"beta": 0.5, "transport": 2}),   # configs[3]'s net and global bunch, in-kernel hand-off
    ("push_c2_world1", [2827, 2048, 257], 256, 1, 2, {"drop": True, "transport": 2}),
    ("push_bf16_2", [300, 256, 128, 64], 64, 2, 2, {"compute_dtype": 1, "lr": 0.5, "transport": 2}),        # event hand-off
    ("bf16_2", [300, 256, 128, 64], 64, 2, 2, {"compute_dtype": 1, "lr": 0.5}),
    ("bf16_dma_2", [300, 256, 128, 64], 128, 2, 2, {"compute_dtype": 1, "lr": 0.5, "drop": True}),   # bunch 128: the LDS-DMA gradient-store kernel
]


def run_case(name, ls, B, world, nb, extra, timeout=600):
    from dp_worker import case_data
    assert world <= MAX_RANKS, (name, world)
    c = dict(ls=ls, B=B, world=world, nb=nb, key="t%d-%s" % (os.getpid(), name))
    c.update(extra)
    with tempfile.TemporaryDirectory() as td:
        cj = os.path.join(td, "case.json")
        json.dump(c, open(cj, "w"))
        env = dict(os.environ, BP_DP_TIMEOUT_S="60", HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "dp_worker.py"), cj, str(r), td], env=env,
                                  stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(world)]
        outs = []
        for p in procs:
            try:
                o, _ = p.communicate(timeout=timeout)
            except subprocess.TimeoutExpired:
                for q in procs:
                    q.kill()
                raise
            outs.append(o.decode(errors="replace"))
        for r, p in enumerate(procs):
            assert p.returncode == 0, "rank %d failed:\n%s" % (r, outs[r][-3000:])
        res = [dict(np.load(os.path.join(td, "rank%d.npz" % r))) for r in range(world)]
        info = [json.load(open(os.path.join(td, "rank%d.json" % r))) for r in range(world)]
    run_case.last_info = info
    return c, case_data(c), res


def forward_of_returned_weights_unequal(pkg, c, r0, x):
    """A handle made as dp_worker.py makes its own (layer sizes, bunch, activation, compute_dtype, dropout scales), but on one rank
    and unattached, from rank 0's returned W, b: the number of words in which its forward differs from rank 0's `out`."""
    ls, B = c["ls"], c["B"]
    kw = dict(activation=c.get("act", 0), momentum_rule=c.get("rule", 0), compute_dtype=c.get("compute_dtype", 0))
    if c.get("drop"):
        kw.update(dropoutflag=1, visible_omit=0.1, hid_omit=0.2, seed=99)
    W = [None] + [r0["W%d" % l] for l in range(1, len(ls))]
    b = [None] + [r0["b%d" % l] for l in range(1, len(ls))]
    n_cv = r0["out"].shape[0]
    g = pkg.BP_GPU(1, len(ls), ls, B, c.get("lr", 1.0), c.get("m", 0.5), c.get("wc", 0.0), W, b, max_chunk_frames=max(4 * B, 64), **kw)
    out = g.forward(x[:n_cv])
    g.close()
    return int(np.count_nonzero(out != r0["out"]))


@pytest.mark.parametrize("name,ls,B,world,nb,extra", CASES, ids=[c[0] for c in CASES])
def test_native_dp_matches_global_bunch_oracle(pkg, oracle_mod, parity_record, name, ls, B, world, nb, extra):
    c, (W, b, x, t), res = run_case(name, ls, B, world, nb, extra)
    L = len(ls)
    # 1. replicated state is bit-identical on every rank
    for r in range(1, world):
        for k in res[0]:
            assert np.array_equal(res[0][k], res[r][k]), (name, "rank", r, k)
    assert int(res[0]["epochs"]) == nb
    # 1b. the forward rank 0 ran on its trained, attached handle is, bit for bit, the forward of a plain handle made from the
    # weights it returned (bf16 rows: the shadow bf_shadow wrote after the sharded update against the one made at creation)
    shadow_unequal = forward_of_returned_weights_unequal(pkg, c, res[0], x)
    parity_record(forward_of_returned_weights_unequal_words=shadow_unequal)
    assert shadow_unequal == 0, (name, "rank 0's forward differs from a handle made from its returned weights in", shadow_unequal, "words")
    # 2. == the oracle on the global bunch
    kw = dict(activation=c.get("act", 0), momentum_rule=c.get("rule", 0))
    bf = c.get("compute_dtype", 0) == 1
    if bf:
        kw["compute_dtype"] = 1
    if c.get("drop"):
        kw.update(dropoutflag=1, visible_omit=0.1, hid_omit=0.2, seed=99)
    o = oracle_mod.Oracle(ls, B * world, c.get("lr", 1.0), c.get("m", 0.5), c.get("wc", 0.0), W, b, **kw)
    assert o.train(x, t) == nb
    tol = 2e-2 if bf else TOL
    # the contract of north_star is on OUTPUTS: the trained network's forward on fresh frames, plain tolerance
    n_cv = min(x.shape[0], 3 * B + 1)
    e_out = relerr(res[0]["out"], o.forward(x[:n_cv]))
    print(name, "forward output after training, rel.err vs oracle: %.2e" % e_out)
    plain = bool(extra.get("plain"))
    if plain:
        assert e_out < tol, (name, "plain bar on the outputs", e_out)
    if not e_out < tol:                                  # full-size nets only: bounded against the fp64-accumulated trajectory (see below)
        assert max(ls) >= 1024, (name, e_out)
        o64 = oracle_mod.Oracle(ls, B * world, c.get("lr", 1.0), c.get("m", 0.5), c.get("wc", 0.0), W, b, acc_double=True, **kw)
        assert o64.train(x, t) == nb
        r64, r32 = o64.forward(x[:n_cv]).astype(np.float64), o.forward(x[:n_cv]).astype(np.float64)
        parity_record(out_dist_to_fp64={"gpu": np.abs(res[0]["out"] - r64).max(), "fp32_oracle": np.abs(r32 - r64).max(), "max_fp64": np.abs(r64).max()})
        assert fp64_bounded(np.abs(res[0]["out"] - r64).max(), np.abs(r32 - r64).max(), np.abs(r64).max(), tol), (name, e_out)
    worst = {}
    for l in range(1, L):
        for nm, a, ref in (("W", res[0]["W%d" % l], o.W[l]), ("b", res[0]["b%d" % l], o.b[l]),
                           ("dW", res[0]["dW%d" % l], o.dW[l]), ("db", res[0]["db%d" % l], o.db[l])):
            worst["%s%d" % (nm, l)] = relerr(a.reshape(np.asarray(ref).shape), ref)
    print(name, "rel.err vs global-bunch oracle:", {k: "%.2e" % v for k, v in worst.items()})
    parity_record(case=name, world=world, local_bunch=B, steps=nb, out_vs_oracle=e_out, state_vs_global_bunch_oracle=dict(worst),
                  bar="bf16 2e-2 (rms for the momentum state)" if bf else "plain 1e-4; fp64-bounded (K=%g) only for tensors listed under bounded_against_fp64" % K_FP64)
    if bf:   # bf16 gradients: single elements move by per cents of the largest one with the summation order; rms criterion
        from test_gpu_parity import relerr_rms     # (same bar as tests/test_gpu_parity.py::test_bf16_step_matches_bf16_oracle)
        for l in range(1, L):
            assert worst["W%d" % l] < tol and worst["b%d" % l] < tol, (name, l, worst)
            assert relerr_rms(res[0]["dW%d" % l], o.dW[l]) < tol and relerr_rms(res[0]["db%d" % l].reshape(-1), np.asarray(o.db[l]).reshape(-1)) < tol, (name, l)
        worst = {}
    if plain:                                            # weights and biases raw at the plain bar, no fallback; momentum state: strict check (3.) only
        for k, v in worst.items():
            assert k.startswith("d") or v < tol, (name, "plain bar", k, v)
        worst = {k: v for k, v in worst.items() if not k.startswith("d")}
    bad = {k: v for k, v in worst.items() if not v < tol}
    # State tensors of the full-size nets are discontinuous functions of fp32 rounding: about one of the ~1.5 M hidden
    # pre-activations per bunch lies within rounding of 0, and whether its ReLU is on decides one frame's contribution
    # to a whole column of G (seen as ~1e-2 of max|delta|, ~2e-4 of max|W|) under ANY summation order, the
    # reference's own included.  For exactly the tensors that miss the plain bar, by name, the bar is the fp64-accumulated
    # oracle: at most K_FP64 (= 2, tests/flip_accounting.py says why) times as far from it as the fp32 restatement of the reference is.  Small nets must meet the plain bar.
    assert not bad or max(ls) >= 1024, (name, bad)
    if bad:
        o64 = oracle_mod.Oracle(ls, B * world, c.get("lr", 1.0), c.get("m", 0.5), c.get("wc", 0.0), W, b, acc_double=True, **kw)
        assert o64.train(x, t) == nb
        bounded = {}
        for k in bad:
            l = int(k[-1])
            a = res[0][k]
            r32 = {"dW": o.dW, "db": o.db, "b": o.b, "W": o.W}[k[:-1]][l]
            r64 = np.asarray({"dW": o64.dW, "db": o64.db, "b": o64.b, "W": o64.W}[k[:-1]][l], np.float64)
            ea = np.abs(np.asarray(a, np.float64).reshape(r64.shape) - r64).max()
            e32 = np.abs(np.asarray(r32, np.float64) - r64).max()
            print("  %s: |gpu-fp64| %.3e, |fp32 oracle-fp64| %.3e, max|fp64| %.3e" % (k, ea, e32, np.abs(r64).max()))
            bounded[k] = {"gpu_to_fp64": ea, "fp32_oracle_to_fp64": e32, "max_fp64": np.abs(r64).max(), "ratio": ea / max(e32, 1e-300)}
            assert fp64_bounded(ea, e32, np.abs(r64).max(), tol), (name, k, ea, e32)
        parity_record(bounded_against_fp64=bounded)
    co = o.crossvalid(x[:n_cv], t[:n_cv])
    assert abs(float(res[0]["cv"]) - co) < (5e-2 if bf else TOL) * abs(co)
    # 3. STRICT check with no escape hatch: the same library on ONE rank with the whole global bunch.  Forward and dgrad
    # are row-independent (same kernels, same k-order per output element), so the sharded and the unsharded run make
    # bit-identical ReLU decisions; only the order of the gradient sum over frames differs.  (The unsharded single-device
    # path faces the oracle -- with the ReLU decisions counted -- in tests/test_gpu_parity.py.)
    if world > 1 and not bf:
        _, _, one = run_case(name + "_1rank", ls, B * world, 1, nb, dict(extra, tail=extra.get("tail", 0), transport=0))
        if extra.get("transport") == 2:
            # the push form sums the same slices in the same order as the pull form: not "close", the SAME bits
            _, _, pull = run_case(name + "_pull", ls, B, world, nb, dict(extra, transport=0))
            for k in res[0]:
                assert np.array_equal(res[0][k], pull[0][k]), (name, "push form differs from pull form", k)
        strict = {}
        for k in res[0]:
            if k in ("epochs", "cv"):
                continue
            n = min(res[0][k].shape[0], one[0][k].shape[0]) if k == "out" else None
            strict[k] = relerr(res[0][k][:n], one[0][k][:n]) if k == "out" else relerr(res[0][k], one[0][k])
        print(name, "sharded vs one rank with the global bunch:", {k: "%.1e" % v for k, v in strict.items()})
        parity_record(sharded_vs_one_rank_same_library=strict, strict_bar=1e-5)
        for k, v in strict.items():
            assert v < 1e-5, (name, "sharded run differs from the unsharded run of the same library", k, v)


def test_push_form_with_bf16_gradient_segments_states_its_tolerance(oracle_mod, parity_record):
    """BP_DP_TRANSPORT_NATIVE_PUSH_BF16 ("bf16-compressed gradients halve comm but cost parity margin --
    keep as a measured option, off by default for fp32 configs"): every rank's contribution to a slice is rounded to bf16 (relative
    rounding error <= 2^-9 per element) before it crosses the fabric, the owner sums the 4 contributions in fp32.  configs[3]'s
    net and global minibatch on MAX_RANKS = 4 ranks (4 x 512 frames, lrate 1, momentum 0.5; the figures below were measured at 8 x 256).  Two references:
    (1) ONE global minibatch against the SAME library with the fp32 exchange (pull form): forward and dgrad are identical and after one
        step the momentum state IS the exchanged gradient (delta = -c1*G/n), so this isolates the rounding: STATED tolerance of the mode,
        max-norm relative to the tensor's largest element: momentum state 4e-3 (= 2^-8; measured 0.7e-3 ... 2.1e-3: eight contributions
        rounded at 2^-9 each, mostly cancelling), weights, biases and trained-net outputs 1e-4 (the update is small against the weights at a global minibatch of 2048);
    (2) TWO global minibatches against the fp32 oracle on the global minibatch: outputs, weights and biases at the plain fp32 bar 1e-4 --
        in THIS configuration the option costs no output parity; the momentum state 2e-2: the perturbed weights of step 1 make a few
        ReLU decisions of step 2 fall differently, the effect the fp32 exchange shows too at 4e-3 ... 8e-3
        (test_native_dp_matches_global_bunch_oracle[c4_4x512]) -- and rounding noise in the weights means MORE such decisions.
    That the momentum state carries a 1e-3-level error into every later step is why this is an option and not the default.
    Ranks must still end bit-identical (every owner sums the same four bf16 words in the same order)."""
    name, ls, B, world = "pushbf16_c4_4x512", [2827, 2048, 2048, 2048, 257], 512, 4
    _, _, one16 = run_case(name + "_1", ls, B, world, 1, {"beta": 0.5, "transport": 3})
    _, _, one32 = run_case(name + "_1_fp32", ls, B, world, 1, {"beta": 0.5, "transport": 0})
    vs_fp32 = {k: relerr(one16[0][k], one32[0][k]) for k in one16[0] if k not in ("epochs", "cv")}
    print(name, "ONE minibatch, bf16 gradient segments vs the fp32 exchange of the same library:", {k: "%.2e" % v for k, v in vs_fp32.items()})
    c, (W, b, x, t), res = run_case(name, ls, B, world, 2, {"beta": 0.5, "transport": 3})
    for r in range(1, world):
        for k in res[0]:
            assert np.array_equal(res[0][k], res[r][k]), (name, "rank", r, k)
    o = oracle_mod.Oracle(ls, B * world, 1.0, 0.5, 0.0, W, b)
    assert o.train(x, t) == 2
    n_cv = min(x.shape[0], 3 * B + 1)
    errs = {"out": relerr(res[0]["out"], o.forward(x[:n_cv]))}
    for l in range(1, len(ls)):
        errs["W%d" % l] = relerr(res[0]["W%d" % l], o.W[l]); errs["b%d" % l] = relerr(res[0]["b%d" % l].reshape(-1), np.asarray(o.b[l]).reshape(-1))
        errs["dW%d" % l] = relerr(res[0]["dW%d" % l], o.dW[l]); errs["db%d" % l] = relerr(res[0]["db%d" % l].reshape(-1), np.asarray(o.db[l]).reshape(-1))
    print(name, "TWO minibatches, bf16 gradient segments vs fp32 global-bunch oracle:", {k: "%.2e" % v for k, v in errs.items()})
    parity_record(case=name, world=world, local_bunch=B, one_step_vs_fp32_exchange_same_library=vs_fp32, two_steps_vs_fp32_global_bunch_oracle=errs,
                  bar="one step vs the fp32 exchange: momentum state 4e-3, everything else 1e-4; two steps vs the oracle: outputs, W, b 1e-4, momentum state 2e-2")
    for k, v in vs_fp32.items():
        assert v < (4e-3 if k.startswith("d") else TOL), ("vs fp32 exchange", k, v)
    for k, v in errs.items():
        assert v < (2e-2 if k.startswith("d") else TOL), ("vs oracle", k, v)
    assert max(vs_fp32.values()) > 1e-5                  # (and it really is a reduced-precision exchange)


def test_attach_argument_errors(pkg):
    from oracle import bp_numpy as N
    ls = [12, 7, 3]
    W, b = N.glorot_net(ls, seed=1, beta=1.0)
    g = pkg.BP_GPU(1, 3, ls, 4, 1.0, 0.5, 0.0, W, b, max_chunk_frames=16)
    with pytest.raises(pkg.BPError):
        g.dp_attach(2, 0, "bad-%d" % os.getpid())        # handle was not created for a 2-rank group
    with pytest.raises(pkg.BPError):
        g.dp_attach(9, 0, "bad-%d" % os.getpid())
    g.dp_attach(1, 0, "solo-%d" % os.getpid())            # a one-rank group is legal (exchange path, no peers)
    with pytest.raises(pkg.BPError):
        g.dp_attach(1, 0, "solo2-%d" % os.getpid())       # already attached
    assert g.dp_handoff() is False                        # 4-frame bunches: not a shape the tile-counting launch is built for
    g.dp_detach()
    g.close()


def test_handoff_mode_is_reported(pkg):
    """bp_dp_handoff: which hand-off of the gradient segments a group runs -- the first multi-GPU run must be able to say
    whether the in-kernel tile counters survived the attach-time self-test on its devices or the event path carried it."""
    from oracle import bp_numpy as N
    ls = [70, 64, 33]
    W, b = N.glorot_net(ls, seed=1, beta=1.0)
    for B, transport, expect in ((128, 0, True), (128, 1, False), (96, 0, False), (128, 2, True)):
        g = pkg.BP_GPU(1, 3, ls, B, 1.0, 0.5, 0.0, W, b, max_chunk_frames=2 * B)
        g.dp_attach(1, 0, "handoff-%d-%d-%d" % (os.getpid(), B, transport), transport=transport)
        assert g.dp_handoff() is expect, (B, transport)
        g.dp_detach()
        g.close()
    g = pkg.BP_GPU(1, 3, ls, 128, 1.0, 0.5, 0.0, W, b, max_chunk_frames=256)
    with pytest.raises(pkg.BPError):
        g.dp_handoff()                                    # not attached
    g.close()


def test_config5_shape_4_ranks_bf16_equals_single_device(oracle_mod, parity_record):
    """BASELINE.json configs[4]'s net and global minibatch: 2827->4096x5->257, bf16 operands / fp32 master weights, global minibatch
    4096 = 4 ranks x 1024 frames (4 processes sharing the GPU; configs[4] itself is 8 ranks x 512, more processes than MAX_RANKS).  Two checkers: (1) the bf16 oracle trained on the GLOBAL
    4096-frame minibatch (15 s on 8 cores) -- outputs of the trained net, weights and biases within the bf16 tolerance
    2e-2, the momentum state by the rms criterion of test_bf16_config5_shape_one_step (2e-2 plus the spread two correct
    bf16 implementations show at this depth); (2) the SAME HIP path on one device with the whole minibatch: the sharded
    run must end bit-identical on all ranks and equal the single-device run up to the fp32 summation order of the gradient."""
    ls = [2827, 4096, 4096, 4096, 4096, 4096, 257]
    extra = {"compute_dtype": 1, "beta": 0.5, "lr": 0.5}
    c8, (W, b, x, t), res8 = run_case("c5_4x1024", ls, 1024, 4, 1, extra, timeout=900)
    from test_gpu_parity import relerr_rms
    o = oracle_mod.Oracle(ls, 4096, 0.5, 0.5, 0.0, W, b, compute_dtype=1)
    assert o.train(x, t) == 1
    n_cv = res8[0]["out"].shape[0]
    vs_oracle = {"out": relerr(res8[0]["out"], o.forward(x[:n_cv]))}
    for l in range(1, len(ls)):
        vs_oracle["W%d" % l] = relerr(res8[0]["W%d" % l], o.W[l])
        vs_oracle["b%d" % l] = relerr(res8[0]["b%d" % l].reshape(-1), np.asarray(o.b[l]).reshape(-1))
        vs_oracle["dW%d(rms)" % l] = relerr_rms(res8[0]["dW%d" % l], o.dW[l])
    print("c5 4x1024 vs the bf16 oracle on the global minibatch:", {k: "%.1e" % v for k, v in vs_oracle.items()})
    for k, v in vs_oracle.items():
        assert v < (5e-2 if k.startswith("dW") else 2e-2), (k, v)
    _, _, res1 = run_case("c5_1x4096", ls, 4096, 1, 1, extra, timeout=900)
    for r in range(1, 4):
        for k in res8[0]:
            assert np.array_equal(res8[0][k], res8[r][k]), ("rank", r, k)
    worst = {}
    n_out = min(res8[0]["out"].shape[0], res1[0]["out"].shape[0])      # (the workers forward 3*B+1 frames: compare the common rows)
    for k in res1[0]:
        if k in ("epochs", "cv"):
            continue
        a, ref = (res8[0][k][:n_out], res1[0][k][:n_out]) if k == "out" else (res8[0][k], res1[0][k])
        worst[k] = relerr(a, ref)
    print("c5 4x1024 vs 1x4096:", {k: "%.1e" % v for k, v in worst.items()})
    parity_record(config="C5 4 ranks x 1024, bf16", vs_bf16_oracle_global_minibatch=vs_oracle, vs_single_device_4096=worst,
                  bar="2e-2 (5e-2 rms for the momentum state)")
    for k, v in worst.items():
        if k.startswith(("W", "b")) or k == "out":
            assert v < 2e-2, (k, v)


def test_ranks_on_distinct_devices_end_bit_identical(pkg):
    """The exchange ACROSS physical devices (hipIpc mappings of a peer DEVICE's arena over xGMI, remote write-through
    stores, remote system-scope loads): needs >= 2 visible GPUs, skipped on a 1-GPU box.  Every rank must report a
    different PCI bus id, the attach-time self-test must have passed (or have selected its fallback), all ranks end
    bit-identical and equal the one-rank run of the same library."""
    ndev = pkg.device_count()
    if ndev < 2:
        pytest.skip("needs >= 2 visible GPUs (this box has %d)" % ndev)
    world = MAX_RANKS if ndev >= MAX_RANKS else 2
    ls, B, nb = [2827, 2048, 2048, 257], 64, 3
    _, _, res = run_case("xdev", ls, B, world, nb, {"drop": True, "beta": 0.5})
    info = run_case.last_info
    buses = [i["peers"][r][1] for r, i in enumerate(info)]
    print("ranks -> PCI bus ids:", buses, "acquire mode:", info[0]["peers"][0][3])
    assert len(set(buses)) == world, buses
    for r in range(1, world):
        for k in res[0]:
            assert np.array_equal(res[0][k], res[r][k]), ("rank", r, k)
    _, _, one = run_case("xdev_1rank", ls, B * world, 1, nb, {"drop": True, "beta": 0.5})
    for k in res[0]:
        if k in ("epochs", "cv", "out"):
            continue
        assert relerr(res[0][k], one[0][k]) < 1e-5, k


def test_rccl_transport_world1(pkg, oracle_mod):
    """The RCCL transport of the same sharded step (bp_dp_attach_ex, BP_DP_TRANSPORT_RCCL) with a single rank -- what a
    1-GPU box can run of it (RCCL refuses two ranks on one device): ncclReduceScatter + sharded update + ncclAllGather
    must train exactly like the fused step."""
    ls, B, nb = [70, 64, 128, 33], 32, 3
    c, (W, b, x, t), res = run_case("rccl1", ls, B, 1, nb, {"transport": 1, "wc": 0.01})
    assert run_case.last_info[0]["peers"][0][2] == 1
    o = oracle_mod.Oracle(ls, B, 1.0, 0.5, 0.01, W, b)
    assert o.train(x, t) == nb
    for l in range(1, len(ls)):
        assert relerr(res[0]["W%d" % l], o.W[l]) < TOL and relerr(res[0]["dW%d" % l], o.dW[l]) < TOL
