"""float64 references of a net with the logistic output layer (bp_set_output), which the C oracle does not have: torch autograd of
the loss written out below, shared by tests/test_output_act_gpu.py and tests/test_dispatch_gpu.py.
    linear columns [0, lin):     L = (1/Bg) sum (o - t)^2
    logistic columns, loss 0:    L = (2/Bg) sum BCE(y, t)        (dL/dz = (2/Bg)(y - t))
    logistic columns, loss 1:    L = (1/Bg) sum (y - t)^2
Nothing from the product or from oracle/ is imported."""
import numpy as np

from philox_np import drop_mask


def ref_forward(ls, W, b, x, masks=None, act=0, lin=0, keep=None):
    """float64 torch forward; returns (parameter tensors, hidden outputs as numpy, z and y of the output layer as tensors).
    keep: CV keep-scales per weight layer (non-inverted dropout: the pre-activation is scaled)."""
    import torch
    L = len(ls)
    Wt = [None] + [torch.tensor(np.asarray(W[l], np.float64), requires_grad=True) for l in range(1, L)]
    bt = [None] + [torch.tensor(np.asarray(b[l], np.float64), requires_grad=True) for l in range(1, L)]
    h = torch.from_numpy(np.asarray(x, np.float64))
    if masks is not None:
        h = h * torch.from_numpy(1.0 - masks[0].astype(np.float64))
    ys = [h.detach().numpy()]
    for l in range(1, L):
        z = (keep[l] if keep else 1.0) * (h @ Wt[l]) + bt[l]
        if l < L - 1:
            h = torch.clamp(z, min=0.0) if act == 0 else torch.sigmoid(z)
            if masks is not None:
                h = h * torch.from_numpy(1.0 - masks[l].astype(np.float64))
            ys.append(h.detach().numpy())
    y = torch.cat([z[:, :lin], torch.sigmoid(z[:, lin:])], 1)
    return Wt, bt, ys, z, y


def ref_loss(z, y, t, lin, loss, Bg, keep_rows=None):
    import torch
    import torch.nn.functional as F
    t = torch.from_numpy(np.asarray(t, np.float64))
    r = torch.ones(z.shape[0], 1, dtype=torch.float64) if keep_rows is None else torch.from_numpy(np.asarray(keep_rows, np.float64))[:, None]
    L = (((y[:, :lin] - t[:, :lin]) ** 2) * r).sum() / Bg
    if loss == 0:                                    # BCE through the logits: softplus(z) - t z = -(t log y + (1-t) log(1-y))
        L = L + 2.0 * ((F.softplus(z[:, lin:]) - t[:, lin:] * z[:, lin:]) * r).sum() / Bg
    else:
        L = L + (((y[:, lin:] - t[:, lin:]) ** 2) * r).sum() / Bg
    return L


def ref_grads(ls, W, b, x, t, masks=None, act=0, lin=0, loss=0, Bg=None, keep_rows=None):
    Wt, bt, ys, z, y = ref_forward(ls, W, b, x, masks, act, lin)
    ref_loss(z, y, t, lin, loss, Bg or x.shape[0], keep_rows).backward()
    L = len(ls)
    return [None] + [Wt[l].grad.numpy() for l in range(1, L)], [None] + [bt[l].grad.numpy() for l in range(1, L)], ys


def _dedz(z, t, lin, loss, Bg):
    y = z.copy()
    y[:, lin:] = 1.0 / (1.0 + np.exp(-z[:, lin:]))
    d = (2.0 / Bg) * (y - t)
    if loss == 1:
        d[:, lin:] *= y[:, lin:] * (1.0 - y[:, lin:])
    return d


def _trajectory(ls, W, b, x, t, B, NS, lr, m, act, lin, loss, drop_seed=None):
    L = len(ls)
    W64 = [None] + [np.asarray(W[l], np.float64).copy() for l in range(1, L)]
    b64 = [None] + [np.asarray(b[l], np.float64).copy() for l in range(1, L)]
    dW = [None] + [np.zeros_like(W64[l]) for l in range(1, L)]
    db = [None] + [np.zeros_like(b64[l]) for l in range(1, L)]
    c1 = (1.0 - m) * lr
    for i in range(NS):
        masks = None
        if drop_seed is not None:
            masks = [drop_mask(drop_seed, i, l, B, ls[l], 0.1 if l == 0 else 0.2) for l in range(L - 1)]
        gw, gb, _ = ref_grads(ls, W64, b64, x[i * B:(i + 1) * B], t[i * B:(i + 1) * B], masks, act, lin, loss)
        for l in range(1, L):
            dW[l] = m * dW[l] - c1 * (gw[l] / B); W64[l] = W64[l] + dW[l]
            db[l] = m * db[l] - c1 * (gb[l] / B); b64[l] = b64[l] + db[l]
    return W64, b64, dW, db


def bf16_logistic_grads(ls, W, b, x, t, act=0, lin=0, loss=0, Bg=None, keep=None):
    """One bunch with bf16 STORAGE of everything a GEMM reads (input, hidden outputs, every dEdX_l, the weights) and float64
    arithmetic in between, written out by hand as torch_ref.bf16_grads is: autograd cannot express the rounding of the
    back-propagated errors.  No dropout.  Returns (gw, gb, ys, y): gradients, hidden outputs and the post-activation output.
    keep: the keep-scales of ref_forward (forward and CV of a dropout handle: the fp32 product is scaled in front of the bias; only
    with t None)."""
    from torch_ref import bf16_round
    L, Bg = len(ls), Bg or x.shape[0]
    Wb = [None] + [bf16_round(W[l]) for l in range(1, L)]
    ys = [bf16_round(np.asarray(x, np.float64))]
    for l in range(1, L):
        z = (keep[l] if keep else 1.0) * (ys[l - 1] @ Wb[l]) + np.asarray(b[l], np.float64)
        if l < L - 1:
            ys.append(bf16_round(np.maximum(z, 0.0) if act == 0 else 1.0 / (1.0 + np.exp(-z))))
    y = z.copy()
    y[:, lin:] = 1.0 / (1.0 + np.exp(-z[:, lin:]))
    if t is None:
        return None, None, ys, y
    assert keep is None, "keep-scaling belongs to forward and CV"
    dx = {L - 1: bf16_round(_dedz(z, np.asarray(t, np.float64), lin, loss, Bg))}
    for l in range(L - 1, 1, -1):
        d = (ys[l - 1] > 0) if act == 0 else ys[l - 1] * (1.0 - ys[l - 1])
        dx[l - 1] = bf16_round(d * (dx[l] @ Wb[l].T))
    return [None] + [ys[l - 1].T @ dx[l] for l in range(1, L)], [None] + [dx[l].sum(0) for l in range(1, L)], ys, y


# ------------------------------------------------------------------ the same references from a child process
# torch for ROCm maps its own HIP / HSA runtime and RCCL into the process that imports it; a test process that later initialises
# the product's RCCL transport (tests/test_dp_native.py) then finds no device.  A test file that sorts in front of that one
# therefore asks a child for the autograd numbers: `python tests/output_ref.py request.npz reply.npz`.
def in_child(op, ls, W, b, x, t=None, act=0, lin=0, loss=0, B=0, steps=0, lr=1.0, m=0.5, keep=None):
    """op "grads": (gw, gb, ys); "forward": y (keep: the keep-scales of ref_forward); "train": (W, b, dW, db) after `steps` bunches
    of B frames (rule 0, no weight cost)."""
    import os
    import subprocess
    import sys
    import tempfile
    L = len(ls)
    with tempfile.TemporaryDirectory() as tmp:
        req, rep = os.path.join(tmp, "request.npz"), os.path.join(tmp, "reply.npz")
        arrs = {"W%d" % l: np.asarray(W[l], np.float64) for l in range(1, L)}
        arrs.update({"b%d" % l: np.asarray(b[l], np.float64) for l in range(1, L)})
        if t is not None:
            arrs["t"] = np.asarray(t)
        if keep is not None:
            assert op == "forward", op
            arrs["keep"] = np.asarray([0.0] + list(keep[1:]), np.float64)
        np.savez(req, op=op, ls=np.asarray(ls), x=np.asarray(x), scalars=np.asarray([act, lin, loss, B, steps, lr, m], np.float64), **arrs)
        subprocess.check_call([sys.executable, os.path.abspath(__file__), req, rep])
        r = np.load(rep)
        r = {k: r[k] for k in r.files}
    if op == "forward":
        return r["y"]
    if op == "grads":
        return ([None] + [r["gw%d" % l] for l in range(1, L)], [None] + [r["gb%d" % l] for l in range(1, L)],
                [r["ys%d" % l] for l in range(L - 1)])
    return tuple([None] + [r["%s%d" % (k, l)] for l in range(1, L)] for k in ("W", "b", "dW", "db"))


def _serve(req, rep):
    import torch
    q = np.load(req)
    ls, op, x = [int(v) for v in q["ls"]], str(q["op"]), q["x"]
    act, lin, loss, B, steps = (int(v) for v in q["scalars"][:5])
    lr, m = float(q["scalars"][5]), float(q["scalars"][6])
    L = len(ls)
    W = [None] + [q["W%d" % l] for l in range(1, L)]
    b = [None] + [q["b%d" % l] for l in range(1, L)]
    out = {}
    if op == "forward":
        with torch.no_grad():
            out["y"] = ref_forward(ls, W, b, x, act=act, lin=lin, keep=list(q["keep"]) if "keep" in q.files else None)[4].numpy()
    elif op == "grads":
        gw, gb, ys = ref_grads(ls, W, b, x, q["t"], act=act, lin=lin, loss=loss)
        for l in range(1, L):
            out["gw%d" % l], out["gb%d" % l] = gw[l], gb[l]
        for l, y in enumerate(ys):
            out["ys%d" % l] = y
    else:
        res = _trajectory(ls, W, b, x, q["t"], B, steps, lr, m, act, lin, loss)
        for k, v in zip(("W", "b", "dW", "db"), res):
            for l in range(1, L):
                out["%s%d" % (k, l)] = v[l]
    np.savez(rep, **out)


if __name__ == "__main__":
    import sys
    _serve(sys.argv[1], sys.argv[2])
