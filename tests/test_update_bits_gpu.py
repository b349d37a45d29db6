"""The momentum update bit for bit, on the device's own gradient, in the kernels that may take the quotient g / ndiv as a multiply
by the exact reciprocal (update_delta<RCP>, csrc/bp_device.h; exact_rdiv, csrc/bp_handle.h) and in those that keep the division (-m gpu).

Procedure as in tests/test_update_gpu.py: a twin handle made from the same weights stores the bunch's gradient G (grads_resident /
read_grads); the tested handle trains two bunches, the first from zero momentum, the second with the momentum carried; W, dW, b, db
after each are compared with np.array_equal against a restatement in float32:

    q  = G / ndiv                    numpy's true division: the rule, whatever the kernel does
    s  = fma(wc, w, q)               float64 product + sum, rounded to float32          (biases: wc = 0)
    d' = the family's form of  m d - c1 s   (FORMS below),   w' = fl(d' + w)

A kernel family is the code one update runs through; how hipcc contracts `m d - c1 s` differs between them and is part of what
this test pins.  FAMILY was fixed by running this file on the commit BEFORE the reciprocal went in: green there, unchanged and
green with it -- that is the whole claim.  The other forms are counted and printed with every case, so a compiler that contracts
differently shows as a move from one column to another, not as noise.  One family is not held to the bit: the generic fused
kernel (GemmKernel<64,64,32>, bunches the LDS-DMA launch is not built for) sums its gradient in another order than the store
kernel the twin runs (128 x 64 x 16 tiles): on the commit before, thousands of weight words differ from every form.  Its weights
are held at update_cases.BAR against float64, as tests/test_update_gpu.py holds them, its biases to the bit.

Any word where device and emulation disagree is adjudicated with exact rational arithmetic (fractions.Fraction, round to nearest
even), so that the double rounding of the float64 fma cannot fail or hide anything; more than ADJUDICATE_MAX such words fail at
once.  The parity record carries, per case, the number of words where the emulation was not the exact value.

Cases (the smallest that reach each path): the LDS-DMA launch bp_wgrad_dma at 128, 256 (XCD tile map, then a narrow problem) and
512 frames, and walked by eight workgroups (BP_WGRAD_SLOTS=8); the generic fused kernel at 64 (multiply) and 96 frames (division);
the data-parallel update at world size 1 with 128 and 384 frames (it keeps the division: bp_dp.h says why); the bf16 update and
its bias lanes at 128 frames.  The DIVISION side of bp_wgrad_dma cannot be reached: the launch is built for 128, 256, 512 frames,
its ndiv is the global bunch, and a handle whose global bunch differs from its own (a shard of 384) trains only attached to its
group, where the store form runs and the update is bp_dp_reduce_update's.

RBM: two applied CD-1 steps of a 130 x 96 RBM at 64 (multiply) and 96 frames (division) against rbm_np's restatement at its bar;
that family is held in float64 at a tolerance on every commit, so it is not held to the bit here either."""
import collections
import fractions
import os

import numpy as np
import pytest

import rbm_np as R
import update_cases as UC

pytestmark = pytest.mark.gpu

Case = collections.namedtuple("Case", ["id", "ls", "B", "dtype", "attach", "slots", "family"])
NET, NET_XCD = [130, 192, 257], [192, 512, 257]
CASES = [
    Case("dma_b128", NET, 128, 0, False, None, "fused"),
    Case("dma_xcd_b256", NET_XCD, 256, 0, False, None, "fused"),
    Case("dma_b512", NET, 512, 0, False, None, "fused"),
    Case("generic_mul_b64", NET, 64, 0, False, None, "generic"),
    Case("generic_div_b96", NET, 96, 0, False, None, "generic"),
    Case("dp_world1_b128", NET, 128, 0, True, None, "dp"),
    Case("dp_world1_b384", NET, 384, 0, True, None, "dp"),
    Case("bf16_b128", NET, 128, 1, False, None, "bf16"),
    Case("dma_walk8_b128", NET, 128, 0, False, 8, "fused"),
]
Hyper = collections.namedtuple("Hyper", ["lr", "m", "wc", "rule"])
HYPERS = {"A": Hyper(0.3, 0.9, 0.3, 0), "B": Hyper(0.7, 0.75, 0.01, 1), "C": Hyper(0.3, 0.9, 0.0, 0)}   # nothing accidentally exact; C: wc 0

# d' = m d - c1 s as the family's kernels round it: (weights, biases)
#   sub     fl(fl(m d) - fl(c1 s))          v_pk_mul_f32 [m d, c1 s], v_sub_f32
#   fma_md  fma(m, d, -fl(c1 s))            v_mul / v_pk_mul c1 s, v_pk_fma
#   fma_cs  fma(-c1, s, fl(m d))
#   bar     not to the bit: float64 restatement at update_cases.BAR (the family's stored gradient is not its fused launch's bits)
FORMS = ("sub", "fma_md", "fma_cs")
FAMILY = {"fused": ("sub", "sub"), "generic": ("bar", "sub"), "dp": ("fma_md", "fma_md"), "bf16": ("fma_md", "sub")}
ADJUDICATE_MAX = 64

f32 = np.float32


def _fma32(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def _coef(h):
    m, lr = f32(h.m), f32(h.lr)
    return m, (lr if h.rule == 1 else (f32(1) - m) * lr), f32(h.wc)         # (update_coef, csrc/bp_handle.h: float arithmetic)


def restate(form, h, ndiv, w, d, g, is_weight):
    """(d', w') in float32 for one tensor."""
    m, c1, wc = _coef(h)
    if not is_weight:
        wc = f32(0)
    w, d, g = (np.asarray(v, np.float32).reshape(-1) for v in (w, d, g))
    q = g / f32(ndiv)
    s = _fma32(wc, w, q)
    if form == "sub":
        dn = m * d - c1 * s
    elif form == "fma_md":
        dn = _fma32(m, d, -(c1 * s))
    else:
        dn = _fma32(-c1, s, m * d)
    assert q.dtype == s.dtype == dn.dtype == np.float32
    return dn, dn + w


def _rn32(x):
    """Fraction -> the nearest float32, ties to even (finite, non-zero results)."""
    c = f32(float(x))
    cands = [c, np.nextafter(c, f32(np.inf)), np.nextafter(c, f32(-np.inf))]
    return min(cands, key=lambda v: (abs(fractions.Fraction(float(v)) - x), int(np.array([v], np.float32).view(np.uint32)[0]) & 1))


def exact_word(form, h, ndiv, w, d, g, is_weight):
    """(d', w') of one word with every rounding step done once, from exact rationals."""
    F = lambda v: fractions.Fraction(float(v))
    m, c1, wc = _coef(h)
    if not is_weight:
        wc = f32(0)
    q = f32(g) / f32(ndiv)
    s = _rn32(F(wc) * F(w) + F(q)) if F(wc) * F(w) + F(q) != 0 else f32(0)
    if form == "sub":
        t = F(_rn32(F(m) * F(d)) if F(m) * F(d) != 0 else 0) - F(_rn32(F(c1) * F(s)) if F(c1) * F(s) != 0 else 0)
    elif form == "fma_md":
        t = F(m) * F(d) - F(_rn32(F(c1) * F(s)) if F(c1) * F(s) != 0 else 0)
    else:
        t = F(_rn32(F(m) * F(d)) if F(m) * F(d) != 0 else 0) - F(c1) * F(s)
    dn = _rn32(t) if t != 0 else f32(0)
    return dn, f32(dn) + f32(w)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


def check_tensor(form, h, ndiv, w, d, g, got_d, got_w, is_weight):
    """(words where the device is not the exact value, words where the emulation was not)."""
    dn, wn = restate(form, h, ndiv, w, d, g, is_weight)
    bad = np.flatnonzero((_bits(dn) != _bits(got_d)) | (_bits(wn) != _bits(got_w)))
    if bad.size > ADJUDICATE_MAX:
        return int(bad.size), 0
    wrong = emu_off = 0
    wf, df, gf, gd, gw = (np.asarray(v, np.float32).reshape(-1) for v in (w, d, g, got_d, got_w))
    for i in bad:
        ed, ew = exact_word(form, h, ndiv, wf[i], df[i], gf[i], is_weight)
        if _bits(ed)[0] == _bits(gd[i])[0] and _bits(ew)[0] == _bits(gw[i])[0]:
            emu_off += 1
        else:
            wrong += 1
    return wrong, emu_off


def bar_error(h, ndiv, w, d, g, got_d, got_w):
    """max|got - expected| / max|expected| over (d', w') against float64, the hyper-parameters as fp32 holds them."""
    m, c1, wc = (float(v) for v in _coef(h))
    w, d, g, got_d, got_w = (np.asarray(v, np.float64).reshape(-1) for v in (w, d, g, got_d, got_w))
    dn = m * d - c1 * (g / ndiv + wc * w)
    wn = w + dn
    return max(float(np.abs(got_d - dn).max() / np.abs(dn).max()), float(np.abs(got_w - wn).max() / np.abs(wn).max()))


def _data(c):
    from oracle import bp_numpy as N
    W, b = N.glorot_net(c.ls, seed=len(c.id) + c.B, beta=0.5)
    rng = np.random.default_rng(c.B + 7)
    n = 2 * c.B
    return W, b, rng.normal(size=(n, c.ls[0])).astype(np.float32), rng.normal(size=(n, c.ls[-1])).astype(np.float32)


def _mk(pkg, c, h, W, b, slots=None):
    if slots is not None:
        os.environ["BP_WGRAD_SLOTS"] = str(slots)
    try:
        return pkg.BP_GPU(1, len(c.ls), c.ls, c.B, h.lr, h.m, h.wc, W, b, compute_dtype=c.dtype, max_chunk_frames=2 * c.B,
                          momentum_rule=h.rule)
    finally:
        if slots is not None:
            del os.environ["BP_WGRAD_SLOTS"]


def _stored_gradient(pkg, c, h, W, b, x, t):
    g = _mk(pkg, c, h, W, b)
    g.upload_chunk(x, t)
    g.grads_resident(0)
    out = g.read_grads()
    g.close()
    return out


def _state(g):
    (w, b), (dw, db) = g.get_weights(), g.get_deltas()
    return w, b, dw, db


@pytest.mark.parametrize("hset", sorted(HYPERS))
@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_two_updates_are_the_restatement_to_the_bit(pkg, parity_record, c, hset):
    h, B, L = HYPERS[hset], c.B, len(c.ls)
    W0, b0, x, t = _data(c)
    T = _mk(pkg, c, h, W0, b0, slots=c.slots)
    if c.attach:
        T.dp_attach(1, 0, "update-bits-%d-%s-%s" % (os.getpid(), c.id, hset))
    w, b = W0, b0
    dw = [None] + [np.zeros_like(np.asarray(v, np.float32)) for v in W0[1:]]
    db = [None] + [np.zeros(np.asarray(v).size, np.float32) for v in b0[1:]]
    survey, fails, emu_off_total = {}, [], 0
    for step in range(2):
        xs, ts = x[step * B:(step + 1) * B], t[step * B:(step + 1) * B]
        gw, gb = _stored_gradient(pkg, c, h, w, b, xs, ts)
        T.train(B, xs, ts)
        nw, nb, ndw, ndb = _state(T)
        for l in range(1, L):
            for kind, is_w, args in (("W", True, (w[l], dw[l], gw[l], ndw[l], nw[l])), ("b", False, (b[l], db[l], gb[l], ndb[l], nb[l]))):
                assert np.asarray(args[3]).any(), (c.id, step, kind, l, "momentum state all zero")
                held = FAMILY[c.family][0 if is_w else 1]
                for form in FORMS:
                    wrong, emu_off = check_tensor(form, h, B, *args, is_weight=is_w)
                    key = "step%d %s%d %s" % (step, kind, l, form)
                    survey[key] = wrong
                    if form == held:
                        emu_off_total += emu_off
                        if wrong:
                            fails.append("%s: %d of %d words are not the restatement" % (key, wrong, np.asarray(args[0]).size))
                if held == "bar":
                    err = bar_error(h, B, *args)
                    survey["step%d %s%d bar" % (step, kind, l)] = err
                    if not err < UC.BAR:
                        fails.append("step%d %s%d: %.3e of max|expected| (bar %.0e)" % (step, kind, l, err, UC.BAR))
        w, b, dw, db = nw, nb, ndw, ndb
    if c.attach:
        T.dp_detach()
    T.close()
    print(c.id, hset, "family", c.family, FAMILY[c.family], "words off per form", survey, "emulation off the exact value in", emu_off_total)
    parity_record(family=c.family, forms=list(FAMILY[c.family]), unequal=survey, emulation_not_exact=emu_off_total)
    assert not fails, (c.id, hset, fails)


@pytest.mark.parametrize("B", [64, 96], ids=["mul_b64", "div_b96"])
def test_rbm_applied_steps_at_the_existing_bar(pkg, parity_record, B):
    st = R.Stack("U%d" % B, (130, 96), B)
    W, cb, a = R.params(st)
    rows = R.rows(st)
    s = pkg.rbm_open(0, st.sizes, st.bunch, W, cb, a, seed=R.SEED, max_chunk_frames=R.N_BUNCHES * B)
    hy = R.HYPER["B"]
    s.set_hyper(1, lrate=hy.lrate, momentum=hy.momentum, weightcost=hy.weightcost, sample=1)
    pick = lambda g: (g[0][1], g[1][1], g[2][1])
    state = tuple(np.zeros_like(v, dtype=np.float64) for v in pick(s.get()))
    worst = {}
    for i in range(2):
        xb = rows[i * B:(i + 1) * B]
        old = pick(s.get())
        tr = s.step(1, xb)
        s.step(1, xb, apply=True)
        e, state = R.update_errors(hy, B, old, state, (tr["gw"], tr["gc"], tr["ga"]), pick(s.get()))
        print("rbm", B, i, e)
        worst.update({"%s_step%d" % (k, i): v for k, v in e.items()})
        assert all(v <= 1.0 for v in e.values()), (B, i, e)
    parity_record(**worst)
    s.close()
