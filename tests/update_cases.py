"""The momentum update with weight cost, restated in float64 from explicit operands, and what the update tests share (no GPU).

The dispatch matrix and the exact matrix run every update kernel at weightcost 0, momentum 0.5 and momentum rule 0: `wc * w`
vanishes, `m` and `1 - m` are the same number, and from zero momentum `m * d` is 0.  The two hyper sets below make every term of

    D' = m D - c1 (G / B + wc W),  W' = W + D'        (DevFunc.cu:313-318 / 306-311, 270-277; biases: wc = 0)
    c1 = (1 - m) lr  (rule 0)  |  lr  (rule 1)

matter, on every case of dispatch_cases.CASES.  The operands are taken from the implementation under test itself (its weights
before the step, its momentum state, the gradient its store kernels leave for the same weights and frames), so the update is held
without the noise of a second bf16 GEMM chain: BAR is dispatch_cases.strict_bar's 1e-5 of max|expected| per tensor.  What
separates the two sides is the summation order of the fused against the stored weight gradient over at most 1040 frames (held to
1e-6 on small nets by test_gradient_buffer_matches_oracle_and_fused_step; the oracle's own fp32 / fp64 spread on the fp32 cases is
at most 9e-7) and a few fp32 roundings of the expression.

MUTANTS are five wrong updates; tests/test_update_host.py shows on the CPU, with the oracle standing in for the device, that the
restatement is inside BAR and every mutant at least MUTANT_FACTOR x BAR outside it in every case and set -- so the GPU test
(tests/test_update_gpu.py) would see each of them."""
import collections

import numpy as np

import dispatch_cases as DC
from test_dispatch_gpu import LR

Hyper = collections.namedtuple("Hyper", ["set", "rule", "m", "wc", "lr"])

BAR = 1e-5
MUTANT_FACTOR = 1000.0
SETS = ("A", "B")
RUNS = [(c, s) for c in DC.CASES for s in SETS]
RUN_IDS = ["%s-%s" % (c.id, s) for c, s in RUNS]


def hyper(hset, dtype):
    """Set A: rule 0, m 0.9, wc 1/16, the dispatch matrix's rate of the dtype.  Set B: rule 1, m 0.75, wc 1/64, lr 0.25.  No dropout:
    the twin that supplies the gradient must see the same masks, and dropout has its own tests."""
    return Hyper("A", 0, 0.9, 0.0625, LR[dtype]) if hset == "A" else Hyper("B", 1, 0.75, 0.015625, 0.25)


MUTANTS = ("no_weight_cost", "weight_cost_on_biases", "m_is_one_minus_m", "c1_of_the_other_rule", "carried_momentum_dropped")


def restate(h, B, W, b, D, d, gw, gb, mutant=None):
    """One update in float64: lists indexed by layer (index 0 unused) in, (D', d', W', b') out.  gw, gb are the SUMS over the B
    frames, as Oracle.grads and read_grads give them.  mutant: one of MUTANTS, or None for the update as it should be."""
    assert mutant is None or mutant in MUTANTS, mutant
    f32 = lambda v: float(np.float32(v))                   # the hyper-parameters as a handle holds them (0.9 is no fp32 number)
    m, wc, wcb, rule, lr = f32(h.m), f32(h.wc), 0.0, h.rule, f32(h.lr)
    if mutant == "no_weight_cost":
        wc = 0.0
    elif mutant == "weight_cost_on_biases":
        wcb = wc
    elif mutant == "m_is_one_minus_m":
        m = 1.0 - m
    elif mutant == "c1_of_the_other_rule":
        rule = 1 - rule
    c1 = lr if rule == 1 else (1.0 - m) * lr
    carry = 0.0 if mutant == "carried_momentum_dropped" else 1.0
    f = lambda a: np.asarray(a, np.float64)
    Dn, dn, Wn, bn = [None], [None], [None], [None]
    for l in range(1, len(W)):
        Dn.append(m * carry * f(D[l]) - c1 * (f(gw[l]) / B + wc * f(W[l])))
        dn.append(m * carry * f(d[l]).reshape(-1) - c1 * (f(gb[l]).reshape(-1) / B + wcb * f(b[l]).reshape(-1)))
        Wn.append(f(W[l]) + Dn[l])
        bn.append(f(b[l]).reshape(-1) + dn[l])
    return Dn, dn, Wn, bn


def zeros_like_state(W, b):
    return ([None] + [np.zeros_like(np.asarray(w, np.float64)) for w in W[1:]],
            [None] + [np.zeros(np.asarray(v).size) for v in b[1:]])


def errors(got, expected):
    """{tensor name: max|got - expected| / max|expected|} for (D, d, W, b) state tuples; also the (name, got, expected) triples."""
    errs, triples = {}, []
    for name, a, r in zip(("dW", "db", "W", "b"), got, expected):
        for l in range(1, len(r)):
            x, y = np.asarray(a[l], np.float64).reshape(np.shape(r[l])), np.asarray(r[l], np.float64)
            errs["%s%d" % (name, l)] = float(np.abs(x - y).max() / max(np.abs(y).max(), 1e-30))
            triples.append(("%s%d" % (name, l), x, y))
    return errs, triples
