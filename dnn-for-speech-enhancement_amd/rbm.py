"""Pre-training: stacked RBMs trained with CD-1 on the device (bp_rbm_*, include/bp_c_api.h)."""
import ctypes as C

import numpy as np

from ._abi import BPError, BPRbmConfig, BPRbmHyper, BPRbmTrace, Closing, MAXLAYER, check, flat32, load_library, ptr, ptrs, set_fields

__all__ = ["RBM_HYPER_FIELDS", "rbm_defaults", "RBMStack", "rbm_open"]

RBM_HYPER_FIELDS = [f[0] for f in BPRbmHyper._fields_]


def rbm_defaults(layer):
    """bp_rbm_defaults: the hyper-parameters a new stack holds for RBM `layer`, as a dict."""
    lib = load_library()
    h = BPRbmHyper()
    check(lib, lib.bp_rbm_defaults(int(layer), C.byref(h)))
    return {k: getattr(h, k) for k in RBM_HYPER_FIELDS}


class RBMStack(Closing):
    """A stack of RBMs on the device (bp_rbm, include/bp_c_api.h); made by rbm_open."""

    def __init__(self, lib, s, layersizes, bunchsize):
        self._lib, self._s = lib, s
        self.layersizes, self.bunchsize = list(layersizes), int(bunchsize)
        self._hyper = {l: rbm_defaults(l) for l in range(1, len(self.layersizes))}

    def _rows(self, rows, n=None):
        a = np.ascontiguousarray(rows, dtype=np.float32)
        if a.ndim != 2 or a.shape[1] != self.layersizes[0] or (n is not None and a.shape[0] != n):
            raise BPError("rows must be [%s][%d]" % ("n" if n is None else n, self.layersizes[0]))
        return a

    def _layer(self, layer):
        if not 1 <= int(layer) < len(self.layersizes):
            raise BPError("layer must lie in [1, %d]" % (len(self.layersizes) - 1))
        return int(layer)

    def hyper(self, layer):
        return dict(self._hyper[self._layer(layer)])

    def set_hyper(self, layer, **fields):
        """bp_rbm_set_hyper: the named fields (lrate, momentum, weightcost, visible, sample) change, the others stay."""
        layer = self._layer(layer)
        bad = sorted(set(fields) - set(RBM_HYPER_FIELDS))
        if bad:
            raise BPError("unknown hyper-parameter: %s" % ", ".join(bad))
        new = dict(self._hyper[layer], **fields)
        h = set_fields(BPRbmHyper(), "set_hyper", new)
        check(self._lib, self._lib.bp_rbm_set_hyper(self._s, layer, C.byref(h)))
        self._hyper[layer] = new

    def train(self, layer, rows):
        """bp_rbm_train_chunk: one CD-1 step per full bunch of rows; the sum of the bunches' reconstruction errors."""
        a = self._rows(rows)
        e = C.c_double(0.0)
        check(self._lib, self._lib.bp_rbm_train_chunk(self._s, int(layer), a.shape[0], ptr(a), C.byref(e)))
        return e.value

    def up(self, layer, rows):
        """bp_rbm_up: the mean-field output of RBM `layer`, [n][layersizes[layer]]."""
        layer = self._layer(layer)
        a = self._rows(rows)
        out = np.empty((a.shape[0], self.layersizes[layer]), np.float32)
        check(self._lib, self._lib.bp_rbm_up(self._s, layer, a.shape[0], ptr(a), ptr(out)))
        return out

    def step(self, layer, rows, apply=False):
        """bp_rbm_step on one bunch: every array of the trace (v0 p0 s0 v1 p1 gw gc ga) and recon, as a dict."""
        layer = self._layer(layer)
        a = self._rows(rows, self.bunchsize)
        V, H, B = self.layersizes[layer - 1], self.layersizes[layer], self.bunchsize
        out = dict(v0=np.empty((B, V), np.float32), p0=np.empty((B, H), np.float32), s0=np.empty((B, H), np.float32),
                   v1=np.empty((B, V), np.float32), p1=np.empty((B, H), np.float32), gw=np.empty((V, H), np.float32),
                   gc=np.empty(H, np.float32), ga=np.empty(V, np.float32))
        recon = C.c_double(0.0)
        tr = BPRbmTrace(*[ptr(out[k]) for k in ("v0", "p0", "s0", "v1", "p1", "gw", "gc", "ga")], C.pointer(recon))
        check(self._lib, self._lib.bp_rbm_step(self._s, layer, ptr(a), 1 if apply else 0, C.byref(tr)))
        out["recon"] = recon.value
        return out

    def steps(self, layer):
        n = C.c_uint(0)
        check(self._lib, self._lib.bp_rbm_steps(self._s, int(layer), C.byref(n)))
        return int(n.value)

    def get(self):
        """bp_rbm_get: (weights, hbias, vbias), lists indexed 1 .. numlayers-1 (entry 0 is None)."""
        L = len(self.layersizes)
        w, c, a = [None] * L, [None] * L, [None] * L
        for l in range(1, L):
            w[l] = np.empty((self.layersizes[l - 1], self.layersizes[l]), np.float32)
            c[l] = np.empty(self.layersizes[l], np.float32)
            a[l] = np.empty(self.layersizes[l - 1], np.float32)
        check(self._lib, self._lib.bp_rbm_get(self._s, ptrs(w), ptrs(c), ptrs(a)))
        return w, c, a

    def close(self):
        if self._s is not None:
            self._lib.bp_rbm_destroy(self._s)
            self._s = None


def rbm_open(device, layersizes, bunchsize, weights, hbias, vbias=None, seed=0, max_chunk_frames=0):
    """bp_rbm_create: weights / hbias / vbias are lists indexed 1 .. len(layersizes)-1 (vbias None or entries None: zeros)."""
    lib = load_library()
    ls = [int(x) for x in layersizes]
    cfg = BPRbmConfig()
    cfg.device, cfg.numlayers, cfg.bunchsize = int(device), len(ls), int(bunchsize)
    for i, s in enumerate(ls[:MAXLAYER]):
        cfg.layersizes[i] = s
    cfg.max_chunk_frames, cfg.seed = int(max_chunk_frames), int(seed)

    def flat(arrs, sizes, name):
        out = [None] * MAXLAYER
        for l in range(1, min(len(ls), MAXLAYER)):
            if arrs is None or l >= len(arrs) or arrs[l] is None:
                continue
            out[l] = flat32(arrs[l])
            if out[l].size != sizes(l):
                raise BPError("%s[%d] has the wrong size" % (name, l))
        return out
    w = flat(weights, lambda l: ls[l - 1] * ls[l], "weights")
    c = flat(hbias, lambda l: ls[l], "hbias")
    a = flat(vbias, lambda l: ls[l - 1], "vbias")
    s = C.c_void_p()
    check(lib, lib.bp_rbm_create(C.byref(cfg), ptrs(w), ptrs(c), ptrs(a) if vbias is not None else None, C.byref(s)))
    return RBMStack(lib, s, ls, bunchsize)
