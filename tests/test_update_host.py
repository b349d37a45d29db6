"""The check of tests/test_update_gpu.py run on the CPU with the oracle standing in for the device (no GPU): per case of the
dispatch matrix and hyper set of tests/update_cases.py

  1. the stand-in trains on bunch 0 -> (W1, b1, D1, d1) and on bunch 1 -> (W2, b2, D2, d2);
  2. a twin made from (W1, b1) gives the gradient G of bunch 1;
  3. update_cases.restate from (W1, D1, G) must reproduce (D2, d2, W2, b2) within update_cases.BAR -- for fp32 cases also with an
     acc_double twin, that is with another summation order in the gradient, which is what separates the device's fused from its
     stored gradient;
  4. each of the five mutants must be at least MUTANT_FACTOR x BAR away from the restatement on at least one tensor.

So the GPU test has a bar the right update meets with room and none of the five wrong ones comes near.  The stand-in is oracle.Oracle
(oracle/bp_oracle.c: the update in fp32, the reference's association); the logistic cases, which the oracle has no output layer for,
take the gradient from tests/output_ref.py as the dispatch tests do and apply Oracle.update to it (no acc_double twin there: that
gradient is float64 already).  An acc_double twin on a bf16 case changes the rounding of the stored activations and is up to 7e-4
away (1e-7 ... 6.8e-4 over the nine linear bf16 cases) -- the reason the device test takes G from the device's own kernels and not
from the oracle.

`python tests/test_update_host.py` prints the table of DESIGN.md 2; under pytest the module prints it when its last test is done."""
import numpy as np
import pytest

import dispatch_cases as DC
import update_cases as UC

ROWS = {}          # (case id, set) -> measured values, for the table


class _Net(object):
    """The stand-in for a handle: fp32 state in an Oracle; linear-output cases train and differentiate with it, logistic ones take
    the gradient from output_ref and use the oracle's update only."""

    def __init__(self, O, c, h, W, b, acc_double=False):
        self.c, self.h = c, h
        self.o = O.Oracle(c.ls, c.B, h.lr, h.m, h.wc, W, b, activation=c.act, momentum_rule=h.rule, compute_dtype=c.dtype,
                          acc_double=acc_double)

    def grads(self, x, t):
        c = self.c
        if c.out is None:
            gw, gb, _, _ = self.o.grads(x, t)
            return gw, gb
        import output_ref as R
        if c.dtype == 1:
            gw, gb, _, _ = R.bf16_logistic_grads(c.ls, self.o.W, self.o.b, x, t, c.act, c.out[0], c.out[1])
        else:
            gw, gb, _ = R.ref_grads(c.ls, self.o.W, self.o.b, x, t, act=c.act, lin=c.out[0], loss=c.out[1])
        return gw, gb

    def train(self, x, t):
        o = self.o
        if self.c.out is None:
            assert o.train(x, t) == 1
        else:
            gw, gb = self.grads(x, t)
            o.update([None] + [np.ascontiguousarray(g, np.float32) for g in gw[1:]],
                     [None] + [np.ascontiguousarray(g, np.float32) for g in gb[1:]], self.c.B)
        return [[None] + [v.copy() for v in a[1:]] for a in (o.dW, o.db, o.W, o.b)]


def measure(O, c, hset):
    h, B = UC.hyper(hset, c.dtype), c.B
    W0, b0, x, t = DC.case_data(c, 2 * B)
    dev = _Net(O, c, h, W0, b0)
    D1, d1, W1, b1 = dev.train(x[:B], t[:B])
    s2 = dev.train(x[B:], t[B:])
    row = {}
    gw, gb = _Net(O, c, h, W1, b1).grads(x[B:], t[B:])
    want = UC.restate(h, B, W1, b1, D1, d1, gw, gb)
    row["reference"] = UC.errors(s2, want)[0]
    if c.dtype == 0 and c.out is None:
        gw2, gb2 = _Net(O, c, h, W1, b1, acc_double=True).grads(x[B:], t[B:])
        row["reference_other_order"] = UC.errors(s2, UC.restate(h, B, W1, b1, D1, d1, gw2, gb2))[0]
    row["mutants"] = {m: UC.errors(UC.restate(h, B, W1, b1, D1, d1, gw, gb, mutant=m), want)[0] for m in UC.MUTANTS}
    return row


def table(rows):
    w = lambda e: max(e.values())
    out = ["| case | set | reference | other order | " + " | ".join(UC.MUTANTS) + " |", "|---|---|---|---|" + "---|" * len(UC.MUTANTS)]
    for (cid, s), r in rows.items():
        out.append("| `%s` | %s | %.1e | %s | %s |" % (cid, s, w(r["reference"]),
                   "%.1e" % w(r["reference_other_order"]) if "reference_other_order" in r else "-",
                   " | ".join("%.1e" % w(r["mutants"][m]) for m in UC.MUTANTS)))
    if rows:
        out.append("worst reference %.1e, worst with the other summation order %.1e, nearest mutant %.1e (bar %.0e, mutants must be beyond %.0e)" % (
            max(w(r["reference"]) for r in rows.values()), max([w(r["reference_other_order"]) for r in rows.values() if "reference_other_order" in r] or [0.0]),
            min(w(r["mutants"][m]) for r in rows.values() for m in UC.MUTANTS), UC.BAR, UC.MUTANT_FACTOR * UC.BAR))
    return "\n".join(out)


@pytest.fixture(scope="module", autouse=True)
def _print_table():
    yield
    print("\n" + table(ROWS))


@pytest.mark.parametrize("c,hset", UC.RUNS, ids=UC.RUN_IDS)
def test_restatement_holds_and_mutants_miss(oracle_mod, c, hset):
    row = ROWS[(c.id, hset)] = measure(oracle_mod, c, hset)
    print(c.id, hset, row)
    for which in ("reference", "reference_other_order"):
        bad = {k: v for k, v in row.get(which, {}).items() if not v < UC.BAR}
        assert not bad, (c.id, hset, which, "outside %.0e" % UC.BAR, bad)
    for m, e in row["mutants"].items():
        assert max(e.values()) >= UC.MUTANT_FACTOR * UC.BAR, (c.id, hset, "mutant", m, "is only", max(e.values()), "away", e)


def test_hyper_sets_make_every_term_matter():
    """What the dispatch and exact matrices cannot see, by construction of their settings, the two sets can: wc != 0, m != 1 - m,
    both rules, and (1 - m) lr != lr."""
    for dt in (0, 1):
        a, b = UC.hyper("A", dt), UC.hyper("B", dt)
        assert (a.rule, b.rule) == (0, 1)
        for h in (a, b):
            assert h.wc > 0 and abs(h.m - (1 - h.m)) >= 0.5 and abs((1 - h.m) * h.lr - h.lr) > 0.1


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import oracle as O
    O.build()
    for c, s in UC.RUNS:
        ROWS[(c.id, s)] = measure(O, c, s)
    print(table(ROWS))
