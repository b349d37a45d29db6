"""The kernel dispatch of the training step, restated (plain Python; nothing from the product is imported).

csrc/bp_step.hip picks the GEMM-family kernels of a call from the shape of the net and the bunch: launch_fwd, prep_dgrad,
run_wgrads (fp32) and bf_launch, bf_out_splits, bf_dma_ok (bf16).  This module repeats those predicates and returns, for a handle
configuration and a call, the launches of that call as the DEMANGLED kernel names of the library's gfx950 code object, e.g.
`void bp_gemm_bf16<2, 64, false, false, 1>(BfGemmArgs, BfEpiArgs)`.  tests/test_dispatch_coverage.py holds it against the built
library and against a kernel trace of tests/test_dispatch_gpu.py; DESIGN.md 2 has the rule that goes with it.

Only the six GEMM families are named (bp_gemm, bp_gemm_multi, bp_out_split_stage, bp_wgrad_dma, bp_gemm_bf16,
bp_wgrad_dma_bf16_six / _store); the small kernels around them (staging, conversion, bias) do not depend on the shape."""

import collections

FAMILIES = ("bp_gemm", "bp_gemm_multi", "bp_out_split_stage", "bp_wgrad_dma", "bp_gemm_bf16", "bp_wgrad_dma_bf16_six",
            "bp_wgrad_dma_bf16_store")

# epilogue numbers of bp_kernels.h (EPI_*) and bp_bf16.h (BEPI_*)
EPI_FWD_HIDDEN, EPI_FWD_OUT, EPI_DGRAD, EPI_WGRAD_UPDATE, EPI_WGRAD_STORE, EPI_OUT_SPLIT, EPI_FWD_OUT_LOGI, EPI_OUT_SPLIT_LOGI = 0, 1, 2, 3, 4, 6, 7, 8
BEPI_FWD_HIDDEN, BEPI_FWD_OUT, BEPI_DGRAD, BEPI_WGRAD_UPDATE, BEPI_WGRAD_STORE, BEPI_FWD_OUT_LOGI = 0, 1, 2, 3, 4, 5
OUT_SPLITS = 4          # bp_kernels.h
BF_OUT_KS = 4           # bp_step.hip
BF_WGRAD_MAXP = 8       # bp_wgrad_dma_bf16.h: layers per grouped launch
FP32_WGRAD_GROUP = 4    # run_wgrads: problems per grouped launch (MultiArgs)


def pad64(x):
    return (x + 63) & ~63


def family(name):
    """bp_gemm_bf16 for `void bp_gemm_bf16<...>(...)`; None for a kernel outside the six families."""
    if not name.startswith("void "):
        return None
    base = name[5:].split("<", 1)[0].split("(", 1)[0]
    return base if base in FAMILIES else None


def _b(v):
    return "true" if v else "false"


def _gemm_kernel(bm, bn, bk, wm, wn, a_kc, b_kc, epi):
    return "GemmKernel<%d, %d, %d, %d, %d, %s, %s, %d>" % (bm, bn, bk, wm, wn, _b(a_kc), _b(b_kc), epi)


def n_gemm(bm, bn, bk, wm, wn, a_kc, b_kc, epi, tag=0):
    return "void bp_gemm<%d, %d, %d, %d, %d, %s, %s, %d, %d>(GemmArgs, EpiArgs)" % (bm, bn, bk, wm, wn, _b(a_kc), _b(b_kc), epi, tag)


def n_multi(*k):
    return "void bp_gemm_multi<%s >(MultiArgs)" % _gemm_kernel(*k)


def n_out_split(epi):
    return "void bp_out_split_stage<%s >(GemmArgs, EpiArgs, int, StageArgs)" % _gemm_kernel(32, 32, 64, 1, 1, True, False, epi)


def n_wgrad_dma(k, store):
    return "void bp_wgrad_dma<16, 4, 4, %d, %s>(MultiArgs)" % (k, _b(store))


def n_bf(epi, bm, bkn, dma=False, ks=1):
    return "void bp_gemm_bf16<%d, %d, %s, %s, %d>(BfGemmArgs, BfEpiArgs)" % (epi, bm, _b(bkn), _b(dma), ks)


def n_bf_six(k):
    return "void bp_wgrad_dma_bf16_six<%d, %d, %d>(BfWgradMulti)" % (k, 64 if k >= 256 else 32, 3 if k >= 256 else 4)


def n_bf_store(k):
    return "void bp_wgrad_dma_bf16_store<%d>(BfWgradMulti)" % k


# One launch: the kernel's name and the n-tile count of every problem it holds (grouped launches hold several).  Every kernel of
# the six families maps workgroups to tiles in one of two ways, by `tiles_n % 8 == 0` (one contiguous n-range per XCD, or plain).
# group: 1, 2, ... for the grouped weight-gradient launches of a bunch, 0 for everything else.
Launch = collections.namedtuple("Launch", ["name", "tiles_n", "group"])
Launch.__new__.__defaults__ = (0,)


class Config(object):
    """What bp_create / bp_set_output fix: layer sizes, bunch size, compute dtype (0 fp32, 1 bf16), output activation (0 linear,
    1 logistic)."""

    def __init__(self, ls, B, dtype=0, out_act=0):
        self.s = [int(v) for v in ls]
        self.L = len(self.s)
        self.ld = [pad64(v) for v in self.s]
        self.B = int(B)
        self.Bp = pad64(self.B)
        self.bf = int(dtype) == 1
        self.logi = int(out_act) == 1

    # bp_create: the fp32 output layer's k range is split over OUT_SPLITS workgroups per tile
    def out_splits(self):
        ld, L = self.ld, self.L
        return OUT_SPLITS if (ld[L - 1] <= 512 and ld[L - 2] >= 1024 and ld[L - 2] % 256 == 0) else 1

    def bf_out_splits(self):
        ld, L, Bp = self.ld, self.L, self.Bp
        tiles, nt = (Bp // 32) * (ld[L - 1] // 64), ld[L - 2] // 64
        return (Bp % 32 == 0 and tiles % 8 == 0 and tiles * BF_OUT_KS <= 2048 and tiles < 256 and nt >= 2 * BF_OUT_KS
                and nt % BF_OUT_KS == 0 and (Bp // 64) * (ld[L - 1] // 64) < 512
                and not (Bp % 128 == 0 and (Bp // 128) * (ld[L - 1] // 64) >= 256))

    def bf_dma_ok(self):
        return self.Bp in (128, 256, 512, 1024)


# ------------------------------------------------------------------ fp32
def fwd_fp32(c, l):
    """launch_fwd: forward of weight layer l (the name does not depend on the number of frames)."""
    cur = c.ld[l]
    if l != c.L - 1:
        if cur <= 512:
            return Launch(n_gemm(32, 32, 64, 1, 1, True, False, EPI_FWD_HIDDEN), (cur // 32,))
        return Launch(n_gemm(32, 64, 64, 1, 2, True, False, EPI_FWD_HIDDEN, 1 if l == 1 else 0), (cur // 64,))
    if c.out_splits() > 1:
        return Launch(n_out_split(EPI_OUT_SPLIT_LOGI if c.logi else EPI_OUT_SPLIT), (cur // 32,))
    epi = EPI_FWD_OUT_LOGI if c.logi else EPI_FWD_OUT
    if cur <= 512:
        return Launch(n_gemm(32, 32, 64, 1, 1, True, False, epi), (cur // 32,))
    return Launch(n_gemm(32, 64, 64, 1, 2, True, False, epi), (cur // 64,))


def dgrad_fp32(c, l):
    """prep_dgrad's cfg + launch_dgrad: dEdX_{l-1} from dEdX_l."""
    prev, cur = c.ld[l - 1], c.ld[l]
    if prev <= 512:
        return Launch(n_multi(32, 32, 64, 1, 1, True, True, EPI_DGRAD), (prev // 32,))
    if cur % 128 == 0:
        return Launch(n_multi(32, 64, 128, 1, 2, True, True, EPI_DGRAD), (prev // 64,))
    return Launch(n_multi(32, 64, 64, 1, 2, True, True, EPI_DGRAD), (prev // 64,))


def wgrads_fp32(c, fused):
    """run_wgrads over the layers 1..L-1: one launch per group of up to four problems; K = bunch size for every problem."""
    out, n, K = [], c.L - 1, c.B
    for i in range(0, n, FP32_WGRAD_GROUP):
        tn = tuple(c.ld[l] // 64 for l in range(1 + i, 1 + min(n, i + FP32_WGRAD_GROUP)))     # every wgrad tile is 64 columns wide
        if K in (128, 256, 512):
            out.append(Launch(n_wgrad_dma(K, not fused), tn, len(out) + 1))
        elif fused:
            out.append(Launch(n_multi(64, 64, 32, 2, 2, False, False, EPI_WGRAD_UPDATE), tn, len(out) + 1))
        else:
            out.append(Launch(n_multi(128, 64, 16, 2, 2, False, False, EPI_WGRAD_STORE), tn, len(out) + 1))
    return out


# ------------------------------------------------------------------ bf16
def bf_launch(c, epi, bkn, M, N, ldims_ok=True, n_limit=None):
    """bf_launch<EPI, BKN>(M, N): 128-row tiles while they give every CU a workgroup (LDS-DMA staged for the hidden forward and
    the dgrad when the n-tile count is a multiple of 8 and every leading dimension one of 8), else 64-row, else 32-row tiles."""
    tiles_n = N // 64
    if M % 128 == 0 and (M // 128) * tiles_n >= 256:
        if epi in (BEPI_FWD_HIDDEN, BEPI_DGRAD) and (tiles_n & 7) == 0 and ldims_ok and (n_limit is None or n_limit == N):
            return Launch(n_bf(epi, 128, bkn, True), (tiles_n,))
        return Launch(n_bf(epi, 128, bkn), (tiles_n,))
    if (M // 64) * tiles_n >= 512:
        return Launch(n_bf(epi, 64, bkn), (tiles_n,))
    if epi in (BEPI_FWD_OUT, BEPI_FWD_OUT_LOGI) and c.bf_out_splits() and M == c.Bp and N == c.ld[c.L - 1]:
        return Launch(n_bf(epi, 32, bkn, False, BF_OUT_KS), (tiles_n,))
    return Launch(n_bf(epi, 32, bkn), (tiles_n,))


def _ld8(*lds):
    return all(v % 8 == 0 for v in lds)


def fwd_bf16(c, l):
    """bf_fwd: always on the padded bunch (M = Bp)."""
    prev, cur = c.ld[l - 1], c.ld[l]
    if l != c.L - 1:
        return bf_launch(c, BEPI_FWD_HIDDEN, True, c.Bp, cur, _ld8(prev, cur, cur, c.Bp), cur)
    return bf_launch(c, BEPI_FWD_OUT_LOGI if c.logi else BEPI_FWD_OUT, True, c.Bp, cur)


def dgrad_bf16(c, l):
    prev, cur = c.ld[l - 1], c.ld[l]
    return bf_launch(c, BEPI_DGRAD, False, c.Bp, prev, _ld8(cur, cur, prev, c.Bp), prev)


def wgrads_bf16(c, fused):
    n = c.L - 1
    if c.bf_dma_ok():
        return [Launch((n_bf_six if fused else n_bf_store)(c.Bp), tuple(c.ld[l] // 64 for l in range(1 + i, 1 + min(n, i + BF_WGRAD_MAXP))),
                       i // BF_WGRAD_MAXP + 1)
                for i in range(0, n, BF_WGRAD_MAXP)]
    epi = BEPI_WGRAD_UPDATE if fused else BEPI_WGRAD_STORE
    return [bf_launch(c, epi, False, c.ld[l - 1], c.ld[l]) for l in range(1, n + 1)]


# ------------------------------------------------------------------ calls
def bunch(c, fused):
    """bunch(): every forward, the dgrads L-1 .. 2, then the weight gradients; the launches in order."""
    L = c.L
    fwd, dgr, wgr = (fwd_bf16, dgrad_bf16, wgrads_bf16) if c.bf else (fwd_fp32, dgrad_fp32, wgrads_fp32)
    return [fwd(c, l) for l in range(1, L)] + [dgr(c, l) for l in range(L - 1, 1, -1)] + wgr(c, fused)


def forward(c, M):
    """forward_resident on M frames (bp_forward, bp_cv_chunk): one forward per layer and bunch, the partial last bunch included."""
    fwd = fwd_bf16 if c.bf else fwd_fp32
    nb = (M + c.B - 1) // c.B
    return [fwd(c, l) for _ in range(nb) for l in range(1, c.L)]


def launches(ls, B, dtype=0, out_act=0, call="step", M=None, bunches=1):
    """The GEMM-family launches (Launch tuples) of one call on a handle (ls, B, dtype, out_act), in order, with repetitions.
    call: "step" (bp_train_* on `bunches` whole bunches, fused update), "grads" (bp_grads_resident: gradient store),
    "forward" or "cv" (on M frames)."""
    c = Config(ls, B, dtype, out_act)
    if call == "step":
        return bunch(c, True) * bunches
    if call == "grads":
        return bunch(c, False)
    if call in ("forward", "cv"):
        return forward(c, c.B if M is None else M)
    raise ValueError("unknown call %r" % (call,))


def kernels(ls, B, dtype=0, out_act=0, call="step", M=None):
    """The SET of kernel names that call launches."""
    return set(x.name for x in launches(ls, B, dtype, out_act, call, M))


def case_launches(ls, B, dtype=0, out_act=0):
    """Everything a case of the GPU matrix runs: a fused step, the gradient store, a forward."""
    return [x for call in ("step", "grads", "forward") for x in launches(ls, B, dtype, out_act, call)]


def case_kernels(ls, B, dtype=0, out_act=0):
    return set(x.name for x in case_launches(ls, B, dtype, out_act))


def tile_config(name):
    """The tile configuration behind a kernel name, epilogue left out: `GemmKernel<32, 64, 64, 1, 2, true, false>` for the fp32
    GEMMs (bp_gemm, bp_gemm_multi and bp_out_split_stage share GemmKernel), `bp_gemm_bf16 BM=64` / `BM=128 DMA` for the bf16
    ones, the family name for the LDS-DMA weight-gradient kernels."""
    fam = family(name)
    args = [a.strip() for a in name[name.index("<") + 1:name.rindex(">")].replace("GemmKernel<", "").replace(">", "").split(",")]
    if fam in ("bp_gemm", "bp_gemm_multi", "bp_out_split_stage"):
        return "GemmKernel<%s>" % ", ".join(args[:7])
    if fam == "bp_gemm_bf16":
        return "bp_gemm_bf16 BM=%s%s" % (args[1], " DMA" if args[3] == "true" else "")
    return fam


def case_paths(ls, B, dtype=0, out_act=0):
    """What a case claims, as strings: every kernel name; `<tile configuration> | xcd map` or `| plain map` for the branch of the
    tile map each problem takes; `<name> | group 2` for a second grouped weight-gradient launch; and `<tile configuration> |
    ragged` when no true width is a multiple of 64 and the bunch none of 32, so that n_true, n_limit, m_limit and the k-range of
    the weight gradients all end inside a tile."""
    ragged = all(v % 64 for v in ls) and B % 32 != 0
    out = set()
    for call in ("step", "grads", "forward"):
        for x in launches(ls, B, dtype, out_act, call):
            out.add(x.name)
            for tn in x.tiles_n:
                out.add("%s | %s map" % (tile_config(x.name), "xcd" if tn % 8 == 0 else "plain"))
            if ragged:
                out.add("%s | ragged" % tile_config(x.name))
            if x.group > 1:
                out.add("%s | group %d" % (x.name, x.group))
    return out
