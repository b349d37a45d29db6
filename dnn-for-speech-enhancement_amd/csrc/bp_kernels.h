// bp_kernels.h -- CDNA4 (gfx950) kernels of the frame-wise DNN step.
//
// One LDS-staged fp32 MFMA GEMM template (v_mfma_f32_32x32x2_f32: exact fp32, k-ordered
// fmaf chain) with the step's elementwise work fused into its epilogues, replacing the
// reference's cuBLAS Sgemm wrappers (DevFunc.h:29-67) + 10 small kernels (DevFunc.cu).
//
//   fwd   X = Y_prev . W  (+bias, act, dropout of the OUTPUT)   A=[m][k]  B=[k][n]
//   dgrad dEdX_prev = act'(y_prev) * (dEdX . W^T)               A=[m][k]  B=[n][k]
//   wgrad G = Y_prev^T . dEdX  (+ momentum update of W, b)      A=[k][m]  B=[k][n]
//
// Operand tiles live in LDS k-major ([k][m] / [k][n]) so that the MFMA operand fetch
// (lane l: A[i=l&31][k=l>>5], B[k=l>>5][j=l&31]) is a conflict-free ds_read_b32 of 32
// consecutive dwords per half-wave.  k-contiguous global operands are transposed on the way
// in (float4 global load -> 4 x ds_write_b32, odd row stride => conflict-free); m/n-contiguous
// operands go in with ds_write_b128.  Register-staged software pipeline: the global loads of k-tile
// t+2 are in flight while tile t is multiplied and tile t+1 moves into the other LDS stage; one barrier per k-tile.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "bp_device.h"

enum { EPI_FWD_HIDDEN = 0, EPI_FWD_OUT = 1, EPI_DGRAD = 2, EPI_WGRAD_UPDATE = 3, EPI_WGRAD_STORE = 4,
       EPI_OUT_SPLIT = 6 /* split-K output layer in ONE launch: k-slice partials into the slabs, the tile's last arriver sums them and runs EPI_FWD_OUT */,
       // logistic output layer (bp_set_output): EPI_FWD_OUT / EPI_OUT_SPLIT with y = 1/(1+expf(-z)) on the columns [lin_cols, n_true)
       // and the output error of EpiArgs::loss there; separate IDs, so the linear kernels keep their code and names
       EPI_FWD_OUT_LOGI = 7, EPI_OUT_SPLIT_LOGI = 8 };
static constexpr bool epi_out(int epi) { return epi == EPI_FWD_OUT || epi == EPI_FWD_OUT_LOGI; }
static constexpr bool epi_out_split(int epi) { return epi == EPI_OUT_SPLIT || epi == EPI_OUT_SPLIT_LOGI; }
static constexpr int OUT_SPLITS = 4;                       // k-slices of the narrow output layer (EPI_OUT_SPLIT)

// The k-loop loads carry NO predicates (a predicated load makes hipcc drain vmcnt at the top of
// every iteration, which serialises the prefetch).  Contract with the caller instead:
//   * every operand buffer is readable for whole tiles (rows rounded up to the tile, one extra
//     row of slack), so tile reads never leave the allocation;
//   * rows/columns past the true extents either hold zeros (layer-width padding; dEdX rows past
//     the bunch, which zero the k-tail of wgrad) or only feed accumulator rows that the
//     epilogue never stores (frames past the bunch in fwd/dgrad).
struct GemmArgs {
    const float *A, *B;
    int lda, ldb;            // leading dimensions (floats)
    int K;                   // reduction extent actually looped (rounded up to BK inside)
    int tiles_m, tiles_n;
#ifdef BP_TRACE              // development only: per-workgroup phase timestamps (tools/gemm_trace.hip)
    unsigned long long *trace;
#endif
    int k_split;             // split-K: workgroup row blockIdx.y handles k in [y*k_split, y*k_split + K)
    size_t slab_stride;      // split-K: floats between the partial-sum slabs of consecutive k-slices
    float *ks_slab; unsigned *ks_ticket;   // EPI_OUT_SPLIT: the slabs ([slice][m][n], rows ldc apart like the output) and one ticket word per tile
};

struct EpiArgs {
    float *C; int ldc;               // Y | dEdX_L | dEdX_prev | W | G
    int m_limit, n_limit;            // rows / cols of C that exist (padded extents)
    int n_true;                      // unpadded column count (pad columns are forced to 0)
    const float *bias;               // fwd
    float alpha;                     // fwd: x = alpha*acc + bias (alpha = keep in CV, BP_GPU.cu:726-746)
    int act;                         // 0 ReLU, 1 Sigmoid
    const float *aux; int ldaux;     // fwd_out: targ | dgrad: y_prev
    int lin_cols;                    // fwd_out_logi: columns [0, lin_cols) stay linear (in what was alignment padding: the layout of
                                     // the struct, and so the code of every kernel that takes it, is the same as without the field)
    float *aux2; int ldaux2;         // fwd_out: out (may be null) | wgrad_update: delta_W
    union {                          // (one word, two readers: the struct has no padding left)
        float scale;                 // fwd_out: 2/n_frames (DevFunc.cu:263)
        float rdiv;                  // wgrad update: exact_rdiv(ndiv) (bp_handle.h), 0 = keep the division; in front of mom, c1, wc, ndiv
    };
    // wgrad update (DevFunc.cu:313-318 + 270-277)
    float mom, c1, wc, ndiv;         // c1 = (1-m)*lr or lr ; ndiv = (float)n
    float *bias_w, *bias_d, *bias_g; // bias / delta_bias (update) or bias-gradient (store)
    // dropout of the produced activation (BP_GPU.cu:546-549 applied by the producer)
    uint32_t drop_thresh, seed_lo, seed_hi, step, layer;
    int frame_off;                   // global frame index of row 0 of this bunch
    const uint8_t *mask; int ldmask; // injected dropout mask of the produced activation ([row][unit] bytes, 1 = drop;
                                     // bp_train_resident_masked, parity tests only) -- replaces the Philox draw
    int loss;                        // fwd_out_logi, logistic columns: 0 dEdz = scale*(y-t) (cross-entropy), 1 ... * y*(1-y) (squared error); padding slot too
    unsigned *done;                  // wgrad store (data parallel): +1 per finished tile, for the exchange stream (bp_dp.h); may be null
};
static_assert(sizeof(EpiArgs) == 160 && offsetof(EpiArgs, aux2) == 56 && offsetof(EpiArgs, done) == 152, "lin_cols / loss must sit in padding");
// rdiv shares the word of scale: no kernel reads both (scale: the output forwards; rdiv: the fused update), every other field keeps
// its offset, and with it the forward, dgrad and output kernels keep their code behind the batched scalar head (BP_PIN_OPERANDS)
static_assert(offsetof(EpiArgs, rdiv) == 68 && offsetof(EpiArgs, scale) == 68 && offsetof(EpiArgs, mom) == 72 && offsetof(EpiArgs, ndiv) == 84,
              "rdiv lies in scale's word, in front of mom, c1, wc, ndiv");
// The operand fields of g (and whatever scalars the caller adds as further "+s"(x) operands) are wanted in scalar registers at this
// one point: their loads from the argument block then go out as ONE batch with one wait.  Left to itself hipcc reads each field
// where its first use happens to be scheduled -- A and B behind the tile map, a grouped launch's fields behind the branch that
// picks the problem -- and every such place is another scalar round trip in front of the first operand load.
typedef __attribute__((address_space(1))) const float *GlobalOperand;      // (an operand pointer that stays GLOBAL, not flat, through the asm)
#define BP_PIN_OPERANDS(g, ...) do { GlobalOperand pa_ = (GlobalOperand)(g).A, pb_ = (GlobalOperand)(g).B;                                \
        asm volatile("" : "+s"(pa_), "+s"(pb_), "+s"((g).lda), "+s"((g).ldb), "+s"((g).K), "+s"((g).tiles_m), "+s"((g).tiles_n), ##__VA_ARGS__); \
        (g).A = (const float *)pa_; (g).B = (const float *)pb_; } while (0)
// The operand side of a GEMM's arguments: all that the addresses of a workgroup's first k-tiles are formed from (GemmKernel::run reads
// these in front of everything else).  The other fields are zero in the copy: it is for run's own use, next to the g_in it was
// made from and from which run reads whatever else it needs -- never hand it to run AS g_in.
__device__ __forceinline__ GemmArgs operand_args(const GemmArgs &s)
{
    GemmArgs g{};
    g.A = s.A; g.B = s.B; g.lda = s.lda; g.ldb = s.ldb; g.K = s.K; g.tiles_m = s.tiles_m; g.tiles_n = s.tiles_n;
    return g;
}

// ------------------------------------------------------------------ epilogue of one 32x32 block
// C/D layout of v_mfma_f32_32x32x2_f32: lane l, reg r -> row (r&3) + 8*(r>>2) + 4*(l>>5), col l&31.
// Inputs the epilogue needs from memory, fetched BEFORE the k-loop so their latency hides under
// it: bias (fwd), targ (fwd_out) / y_prev (dgrad) / W (wgrad) in p0, delta_W (wgrad) in p1.
struct EpiPre { float bias; f32x16 p0, p1; };

// A pointer the compiler cannot prove wave-uniform, forced into SGPRs (so that loads/stores through it
// take the  saddr + 32-bit lane offset  form and need no per-row 64-bit address VGPRs).
template <class T>
__device__ __forceinline__ T *uniform_ptr(T *p)
{
    const unsigned long long v = (unsigned long long)p;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    typedef __attribute__((address_space(1))) T *GlobalPtr;      // keep it a GLOBAL pointer (not flat)
    return (T *)(GlobalPtr)(((unsigned long long)hi << 32) | lo);
}

// Pin a wave-uniform pointer in an SGPR pair and hide its derivation from the optimiser, so that
// `*(T*)((char*)sgpr_row_base(p) + lane_byte_offset)` is selected as  global_load v, v_off, s[base]
// instead of being reassociated into per-lane 64-bit addresses.
template <class T>
__device__ __forceinline__ T *sgpr_row_base(T *p)
{
    typedef __attribute__((address_space(1))) T *GlobalPtr;
    GlobalPtr q = (GlobalPtr)p;
    asm volatile("" : "+s"(q));
    return (T *)q;
}

// Registers [R0, R0+RN) of one 32x32 accumulator block (after an in-workgroup k-split every wave
// finishes 16/KS of the block's registers).
template <int EPI, int R0, int RN>
__device__ __forceinline__ void epilogue_fetch(const EpiArgs &e, int mb, int nb, int lane, EpiPre &p)
{
    if constexpr (EPI == EPI_WGRAD_UPDATE) {
        // natural MFMA layout (lane -> column n, registers -> rows): every W / delta load and store is two full 128-byte rows
        // uniform row base (SGPRs) + one per-lane 32-bit offset: no per-row address VGPRs.  m_limit is a
        // multiple of 32 (padded widths), so a 32-row block is wholly inside or wholly outside the matrix;
        // outside blocks read row 0 and are never stored.
        const int mbc = mb < e.m_limit ? mb : 0;
        const float *cw = uniform_ptr(e.C + (size_t)mbc * e.ldc + nb);
        const float *cd = uniform_ptr(e.aux2 + (size_t)mbc * e.ldc + nb);
        const unsigned ldc = __builtin_amdgcn_readfirstlane(e.ldc);
        const unsigned lob = 4u * ((unsigned)(4 * (lane >> 5)) * (unsigned)e.ldc + (unsigned)(lane & 31));   // bytes
#pragma unroll
        for (int r = R0; r < R0 + RN; ++r) {
            const unsigned ro = (unsigned)((r & 3) + 8 * (r >> 2)) * ldc;
            p.p0[r] = *reinterpret_cast<const float *>(reinterpret_cast<const char *>(sgpr_row_base(cw + ro)) + lob);
            p.p1[r] = *reinterpret_cast<const float *>(reinterpret_cast<const char *>(sgpr_row_base(cd + ro)) + lob);
        }
        return;
    }
    const int n = nb + (lane & 31);
    const int rbase = mb + 4 * (lane >> 5);
    static_assert(!epi_out_split(EPI), "fetched as EPI_FWD_OUT[_LOGI]");
    if constexpr (EPI == EPI_FWD_HIDDEN || epi_out(EPI)) p.bias = e.bias[n];
    if constexpr (epi_out(EPI) || EPI == EPI_DGRAD) {
        if (epi_out(EPI) && !e.C) return;
#pragma unroll
        for (int r = R0; r < R0 + RN; ++r) {
            const int m = rbase + (r & 3) + 8 * (r >> 2);
            const int mc = m < e.m_limit ? m : e.m_limit - 1;      // (rows past the matrix are never stored)
            p.p0[r] = e.aux[(size_t)mc * e.ldaux + n];
        }
    }
}

// Stores of registers [R0, R0+RN) of a block: v[r - R0] to row (r&3) + 8*(r>>2) + 4*(lane>>5), column lane&31 of the block at
// (mb, nb) of C.  A block wholly below m_limit stores through the weight gradient's form, a uniform row base in SGPRs plus one
// 32-bit lane offset, behind ONE test; a partial block tests every row and forms its 64-bit address.  Rows at or past m_limit are
// never written (the dEdX rows past the bunch stay zero for the weight gradient).  The caller has sent lanes n >= n_limit away.
template <int R0, int RN>
__device__ __forceinline__ void block_store(const EpiArgs &e, int mb, int nb, int lane, const float (&v)[RN])
{
    if (mb + 32 <= e.m_limit) {
        float *c = uniform_ptr(e.C + (size_t)mb * e.ldc + nb);
        const unsigned ldc = __builtin_amdgcn_readfirstlane(e.ldc);
        const unsigned lob = 4u * ((unsigned)(4 * (lane >> 5)) * (unsigned)e.ldc + (unsigned)(lane & 31));   // bytes
#pragma unroll
        for (int r = R0; r < R0 + RN; ++r) {
            const unsigned ro = (unsigned)((r & 3) + 8 * (r >> 2)) * ldc;
            *reinterpret_cast<float *>(reinterpret_cast<char *>(sgpr_row_base(c + ro)) + lob) = v[r - R0];
        }
        return;
    }
    const int n = nb + (lane & 31), rbase = mb + 4 * (lane >> 5);
#pragma unroll
    for (int r = R0; r < R0 + RN; ++r) {
        const int m = rbase + (r & 3) + 8 * (r >> 2);
        if (m < e.m_limit) e.C[(size_t)m * e.ldc + n] = v[r - R0];
    }
}

// RCP (EPI_WGRAD_UPDATE): the update's quotient as a multiply (update_delta<true>, bp_device.h); chosen by the caller, once for
// the tile, on e.rdiv != 0
template <int EPI, int R0, int RN, bool RCP = false>
__device__ __forceinline__ void epilogue_block(const EpiArgs &e, int mb, int nb, const f32x16 &acc, int lane,
                                               const EpiPre &p)
{
    static_assert(!RCP || EPI == EPI_WGRAD_UPDATE, "only the fused update divides");
    static_assert(RN % 4 == 0 && R0 % 4 == 0, "register range must cover whole 4-row groups");
    if constexpr (EPI == EPI_WGRAD_UPDATE || EPI == EPI_WGRAD_STORE) {
        const int n = nb + (lane & 31);
        if (n >= e.n_limit || mb >= e.m_limit) return;              // (m_limit % 32 == 0: whole block in or out)
        float *cw = uniform_ptr(e.C + (size_t)mb * e.ldc + nb);
        const unsigned ldc = __builtin_amdgcn_readfirstlane(e.ldc);
        const unsigned lob = 4u * ((unsigned)(4 * (lane >> 5)) * (unsigned)e.ldc + (unsigned)(lane & 31));   // bytes
#pragma unroll
        for (int r = R0; r < R0 + RN; ++r) {
            const unsigned ro = (unsigned)((r & 3) + 8 * (r >> 2)) * ldc;
            if constexpr (EPI == EPI_WGRAD_UPDATE) {
                float *cd = uniform_ptr(e.aux2 + (size_t)mb * e.ldc + nb);
                const float w = p.p0[r];
                const float d = update_delta<RCP>(e.mom, e.c1, e.wc, e.ndiv, e.rdiv, p.p1[r], acc[r], w);
                *reinterpret_cast<float *>(reinterpret_cast<char *>(sgpr_row_base(cd + ro)) + lob) = d;
                *reinterpret_cast<float *>(reinterpret_cast<char *>(sgpr_row_base(cw + ro)) + lob) = d + 1.0f * w;   // kernAccSum
            } else {
                // gradient tile of the data-parallel step: SYSTEM-scope write-through stores (sc0 sc1) -- once the wave has drained
                // vmcnt the tile is in memory whatever kind of allocation the gradient buffer is, which is what lets the tile count
                // of bp_wgrad_dma.h hand the segment to the peers without a kernel boundary or an L2 write-back (bp_dp.h)
                __hip_atomic_store(reinterpret_cast<float *>(reinterpret_cast<char *>(sgpr_row_base(cw + ro)) + lob), acc[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
        return;
    }
    const int n = nb + (lane & 31);
    const int rbase = mb + 4 * (lane >> 5);
    if (n >= e.n_limit) return;
    if constexpr (EPI == EPI_FWD_HIDDEN) {
        const float bn = p.bias;
        const bool live = n < e.n_true;
        float y[RN];
#pragma unroll
        for (int q = R0 / 4; q < (R0 + RN) / 4; ++q) {
            uint32_t w[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
            const int r0 = rbase + 8 * q;
            if (e.mask) {                                        // injected mask: word 0 = "drop", thresh 1 (set by the host)
#pragma unroll
                for (int j = 0; j < 4; ++j) w[j] = (r0 + j < e.m_limit && live && e.mask[(size_t)(r0 + j) * e.ldmask + n]) ? 0u : 0xFFFFFFFFu;
            } else if (e.drop_thresh) drop_words4(w, r0, n, e.frame_off, (uint32_t)e.n_true, e.layer, e.step, e.seed_lo, e.seed_hi);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                y[q * 4 + j - R0] = act_fwd(e.act, e.alpha * acc[q * 4 + j] + bn);
                if (!live || w[j] < e.drop_thresh) y[q * 4 + j - R0] = 0.0f;
            }
        }
        block_store<R0, RN>(e, mb, nb, lane, y);
    } else if constexpr (EPI == EPI_FWD_OUT) {
        const float bn = p.bias;
        const bool live = n < e.n_true;
#pragma unroll
        for (int r = R0; r < R0 + RN; ++r) {
            const int m = rbase + (r & 3) + 8 * (r >> 2);
            if (m < e.m_limit) {
                const float o = live ? e.alpha * acc[r] + bn : 0.0f;
                if (e.aux2) e.aux2[(size_t)m * e.ldaux2 + n] = o;
                if (e.C) e.C[(size_t)m * e.ldc + n] = live ? e.scale * (o - p.p0[r]) : 0.0f;   // kernSubClean
            }
        }
    } else if constexpr (EPI == EPI_FWD_OUT_LOGI) {
        // BP_GPU.cu.bak:565-630: kernSigmoid on the output, then kernSubClean on the post-sigmoid output (loss 0); loss 1 adds the
        // logistic's derivative.  Pad columns (n >= n_true) stay 0 in the output and the error: sigmoid(0) = 0.5 must not leak.
        const float bn = p.bias;
        const bool live = n < e.n_true, logi = live && n >= e.lin_cols, chain = logi && e.loss == 1;
#pragma unroll
        for (int r = R0; r < R0 + RN; ++r) {
            const int m = rbase + (r & 3) + 8 * (r >> 2);
            if (m < e.m_limit) {
                const float z = live ? e.alpha * acc[r] + bn : 0.0f;
                const float o = logi ? 1.0f / (1.0f + expf(-z)) : z;
                if (e.aux2) e.aux2[(size_t)m * e.ldaux2 + n] = o;
                if (e.C) {
                    float d = live ? e.scale * (o - p.p0[r]) : 0.0f;
                    if (chain) d *= o * (1.0f - o);
                    e.C[(size_t)m * e.ldc + n] = d;
                }
            }
        }
    } else if constexpr (EPI == EPI_DGRAD) {
        float d[RN];
#pragma unroll
        for (int r = R0; r < R0 + RN; ++r) d[r - R0] = act_bwd(e.act, p.p0[r]) * acc[r];   // kernDsigmoid*kernVecMul
        block_store<R0, RN>(e, mb, nb, lane, d);
    } else {
        static_assert(EPI == EPI_WGRAD_UPDATE || EPI == EPI_WGRAD_STORE, "epilogue without a branch");   // (wgrad returned above)
    }
}

// One lane of the fused update's bias tile: bias n from its summed gradient s (kernUpdatedelta with wc = 0 + kernAccSum).
template <bool RCP>
__device__ __forceinline__ void bias_update(const EpiArgs &e, int n, float s)
{
    const float d = update_delta<RCP>(e.mom, e.c1, 0.0f, e.ndiv, e.rdiv, e.bias_d[n], s, e.bias_w[n]);
    e.bias_d[n] = d;
    e.bias_w[n] = d + 1.0f * e.bias_w[n];
}

// EPI_OUT_SPLIT, registers [R0, R0+4) of the wave's 32x32 block.  store: this k-slice's partial sums into its slab, agent-scope
// write-through (the accesses last_arrival relies on).  sum: the OUT_SPLITS partials of the tile, added in slice order
// 0..3 whichever slice arrived last (the summation order of the two-launch form this replaces: the same bits), agent-scope loads.
template <int R0>
__device__ __forceinline__ void out_split_store(const EpiArgs &e, float *slab, int mb, int nb, const f32x16 &acc, int lane)
{
    const int n = nb + (lane & 31), rbase = mb + 4 * (lane >> 5);
    if (n >= e.n_limit) return;
#pragma unroll
    for (int r = R0; r < R0 + 4; ++r) {
        const int m = rbase + (r & 3) + 8 * (r >> 2);
        if (m < e.m_limit) __hip_atomic_store(slab + (size_t)m * e.ldc + n, acc[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
template <int R0>
__device__ __forceinline__ void out_split_sum(const EpiArgs &e, const float *slab0, size_t stride, int mb, int nb, f32x16 &acc, int lane)
{
    const int n = nb + (lane & 31), rbase = mb + 4 * (lane >> 5);
    if (n >= e.n_limit) return;
    float p[OUT_SPLITS][4];
#pragma unroll
    for (int z = 0; z < OUT_SPLITS; ++z)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int r = R0 + rr, m = rbase + (r & 3) + 8 * (r >> 2), mc = m < e.m_limit ? m : e.m_limit - 1;   // (clamped: all 16 loads unconditional)
            p[z][rr] = __hip_atomic_load(slab0 + z * stride + (size_t)mc * e.ldc + n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        float s = p[0][rr];
#pragma unroll
        for (int z = 1; z < OUT_SPLITS; ++z) s += p[z][rr];
        acc[R0 + rr] = s;
    }
}

// In-workgroup k-split (KS wave groups hold partial sums of the same 32x32 block): wave KSI keeps
// registers [KSI*16/KS, (KSI+1)*16/KS), hands the others to their owners through LDS, and finishes
// its share -- so every wave runs 1/KS of the epilogue instead of wave group 0 running all of it.
template <int KS, int KSI>
__device__ __forceinline__ void ksplit_give(const f32x16 &acc, float *red, int wq, int lane)
{
    constexpr int RN = 16 / KS;
#pragma unroll
    for (int o = 0; o < KS; ++o) {
        if (o == KSI) continue;
#pragma unroll
        for (int rr = 0; rr < RN; ++rr) red[(((wq * KS + o) * KS + KSI) * RN + rr) * 64 + lane] = acc[o * RN + rr];
    }
}
template <int KS, int KSI>
__device__ __forceinline__ void ksplit_take(f32x16 &acc, const float *red, int wq, int lane)
{
    constexpr int RN = 16 / KS;
#pragma unroll
    for (int src = 0; src < KS; ++src) {
        if (src == KSI) continue;
#pragma unroll
        for (int rr = 0; rr < RN; ++rr) acc[KSI * RN + rr] += red[(((wq * KS + KSI) * KS + src) * RN + rr) * 64 + lane];
    }
}

// ------------------------------------------------------------------ the GEMM
// Register image of one k-tile of both operands (global -> registers -> LDS staging).
template <int NVA, int NVB>
struct TileRegs { float4 a[NVA]; float4 b[NVB]; };

// BM x BN x BK workgroup tile, 4 waves arranged WM x WN x KS (KS = 4/(WM*WN) splits each
// k-tile between wave groups; partial sums meet in LDS before the epilogue).
// A_KC: A is [m][k] in memory (k contiguous) else [k][m]; B_KC: B is [n][k] else [k][n].
template <int BM, int BN, int BK, int WM, int WN, bool A_KC, bool B_KC, int EPI>
struct GemmCfg {
    static constexpr int KS = 4 / (WM * WN);
    static constexpr int TM = BM / (WM * 32), TN = BN / (WN * 32);
    static constexpr int LDA_S = A_KC ? BM + 1 : BM;
    static constexpr int LDB_S = B_KC ? BN + 1 : BN;
    static constexpr int A_STAGE = (BK * LDA_S + 3) & ~3, B_STAGE = (BK * LDB_S + 3) & ~3;
    static constexpr int NVA = BM * BK / 4 / 256, NVB = BN * BK / 4 / 256;
    static constexpr int LPS = (BK / 4 < 8) ? BK / 4 : 8;     // lanes per 128-byte row segment
    static constexpr bool BIASG = (EPI == EPI_WGRAD_UPDATE || EPI == EPI_WGRAD_STORE);
    static_assert(WM * WN * KS == 4 && TM >= 1 && TN >= 1, "wave layout");
    static_assert(BK % (2 * KS) == 0 && BK % 4 == 0, "BK");
    static_assert(NVA >= 1 && NVB >= 1, "tile too small for 256 threads");
    using Regs = TileRegs<NVA, NVB>;

    // The k-loop's index functions (tests/cpp/kloop_order_driver.cc enumerates them on the host): of every k-tile wave group ks
    // multiplies rows [ks*BK/KS, (ks+1)*BK/KS) in NK steps of two rows (lane half kh takes the odd one), step s into chain s % NCH.
    static constexpr int NCH = (TM * TN == 1) ? 2 : 1;
    static constexpr int NK = BK / KS / 2;
    static constexpr int step_row(int ks, int s) { return ks * (BK / KS) + 2 * s; }
    static constexpr int step_chain(int s) { return s % NCH; }
    // Where a k-tile's LDS traffic sits among its NK MFMA steps (tests/cpp/kloop_barrier_driver.cc holds these to the invariants
    // GemmCfg::step argues from): fragment reads run RD steps ahead of their MFMA, so the read for step s + RD is issued behind
    // MFMA s and the last one behind MFMA LAST_READ; the tile's one barrier sits behind MFMA BAR; the NP = NVA + NVB pieces that
    // stage the NEXT tile are written behind MFMA store_slot(q), all of them at or in front of BAR; the global loads stay spread
    // over the whole tile.  In the forwards (A [m][k], B [k][n]) BAR is one MFMA step in front of the tile's end: that MFMA
    // covers the first reads of the next tile.  Every other configuration keeps the barrier behind the tile's last MFMA, as do
    // tiles too short to have a step between their last read and their last MFMA: in the dgrads an earlier barrier let the
    // eight workgroups that stream one weight panel drift apart and the launch end later, and the weight gradients' k-loops
    // were longer with it (profiles/r19_kloop_barrier.txt, which also has the positions further forward: all slower).
    static constexpr bool EARLY_BAR = A_KC && !B_KC;
    static constexpr int NP = NVA + NVB;
    static constexpr int RD = NK < 4 ? NK : 4;
    static constexpr int LAST_READ = NK - RD - 1;                          // (-1: every read belongs to the first RD)
    static constexpr int BAR = (EARLY_BAR && NK > RD + 2) ? NK - 2 : NK - 1;
    static constexpr int store_slot(int q) { return (q * (BAR + 1)) / NP; }
    static constexpr int load_slot(int q) { return (q * NK) / NP; }
    static_assert(BAR > LAST_READ && BAR <= NK - 1, "the barrier's wait covers every fragment read of the tile, none of them young");

    // Addressing: uniform tile base (SGPR pair) + per-thread unsigned 32-bit BYTE offset that never changes: a load is one
    // instruction (global_load_dwordx4 v, v_off, s[base:base+1]) and the k-advance is scalar arithmetic.  Two things are needed
    // for hipcc to select that form.  The offset is unsigned bytes: a signed element offset is sign-extended and scaled, a 64-bit
    // VALU add per load with every offset held as a VGPR pair.  And it is made opaque, in place, where it is used (lane_off): the
    // zero extension then stays in the block of the load, where instruction selection can fold it into the address; hoisted out
    // of the k-loop it comes back as a VGPR pair and the same add.  Those adds were the only VALU instructions of the
    // steady-state loops, 12 per 32 MFMAs, and cost the wide forward 1.9 us of an 18.3 us k-loop (profiles/r17_kloop_pairs.txt).
    struct Offs { unsigned a[NVA]; unsigned b[NVB]; };
    static __device__ __forceinline__ unsigned lane_off(unsigned &off)
    {
        asm volatile("" : "+v"(off));
        return off;
    }
    static __device__ __forceinline__ void make_offs(Offs &o, const GemmArgs &g, int tid)
    {
#pragma unroll
        for (int i = 0; i < NVA; ++i) {
            const int f = tid + i * 256;
            if constexpr (A_KC) {
                const int l8 = f % LPS, seg = f / LPS, row = seg % BM, k4 = (seg / BM) * LPS + l8;
                o.a[i] = 4u * (unsigned)(row * g.lda + k4 * 4);
            } else {
                const int c4 = f % (BM / 4), k = f / (BM / 4);
                o.a[i] = 4u * (unsigned)(k * g.lda + c4 * 4);
            }
        }
#pragma unroll
        for (int i = 0; i < NVB; ++i) {
            const int f = tid + i * 256;
            if constexpr (B_KC) {
                const int l8 = f % LPS, seg = f / LPS, row = seg % BN, k4 = (seg / BN) * LPS + l8;
                o.b[i] = 4u * (unsigned)(row * g.ldb + k4 * 4);
            } else {
                const int c4 = f % (BN / 4), k = f / (BN / 4);
                o.b[i] = 4u * (unsigned)(k * g.ldb + c4 * 4);
            }
        }
    }
    // uniform base of k-tile k0 for each operand
    static __device__ __forceinline__ const float *base_a(const GemmArgs &g, int m0, int k0)
    {
        return A_KC ? g.A + (size_t)m0 * g.lda + k0 : g.A + (size_t)k0 * g.lda + m0;
    }
    static __device__ __forceinline__ const float *base_b(const GemmArgs &g, int n0, int k0)
    {
        return B_KC ? g.B + (size_t)n0 * g.ldb + k0 : g.B + (size_t)k0 * g.ldb + n0;
    }
    static __device__ __forceinline__ void load_a(Regs &r, int i, const float *pa, Offs &o)
    {
        r.a[i] = *reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(pa) + lane_off(o.a[i]));
    }
    static __device__ __forceinline__ void load_b(Regs &r, int i, const float *pb, Offs &o)
    {
        r.b[i] = *reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(pb) + lane_off(o.b[i]));
    }
    static __device__ __forceinline__ void load(Regs &r, const float *pa, const float *pb, Offs &o)
    {
#pragma unroll
        for (int i = 0; i < NVA; ++i) load_a(r, i, pa, o);
#pragma unroll
        for (int i = 0; i < NVB; ++i) load_b(r, i, pb, o);
    }

    // one float4 of the A / B register image -> LDS (k-major, transposing k-contiguous operands).  krows: rows of this k-tile
    // below K.  Only the weight gradients look at it: their k runs over the frames of the bunch, and the rows of y_0 behind
    // the bunch are whatever follows it in the chunk buffer -- other frames, possibly NaN or Inf, which a zero row of dEdX does
    // not cancel.  They are selected away here, where the value is on its way to LDS anyway (the load itself stays
    // unconditional).  Every other configuration has K a multiple of BK.
    static __device__ __forceinline__ void store_a(const Regs &r, int i, float *As, int tid, int krows)
    {
        const int f = tid + i * 256;
        float4 v = r.a[i];                // (a local copy keeps the register set out of scratch)
        if constexpr (BIASG && !A_KC) {
            if (f / (BM / 4) >= krows) v = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        if constexpr (A_KC) {
            const int l8 = f % LPS, seg = f / LPS, row = seg % BM, k4 = (seg / BM) * LPS + l8;
            As[(k4 * 4 + 0) * LDA_S + row] = v.x; As[(k4 * 4 + 1) * LDA_S + row] = v.y;
            As[(k4 * 4 + 2) * LDA_S + row] = v.z; As[(k4 * 4 + 3) * LDA_S + row] = v.w;
        } else {
            const int c4 = f % (BM / 4), k = f / (BM / 4);
            *reinterpret_cast<float4 *>(As + k * LDA_S + c4 * 4) = v;
        }
    }
    static __device__ __forceinline__ void store_b(const Regs &r, int i, float *Bs, int tid, float4 &bsum)
    {
        const int f = tid + i * 256;
        const float4 v = r.b[i];
        if constexpr (B_KC) {
            const int l8 = f % LPS, seg = f / LPS, row = seg % BN, k4 = (seg / BN) * LPS + l8;
            Bs[(k4 * 4 + 0) * LDB_S + row] = v.x; Bs[(k4 * 4 + 1) * LDB_S + row] = v.y;
            Bs[(k4 * 4 + 2) * LDB_S + row] = v.z; Bs[(k4 * 4 + 3) * LDB_S + row] = v.w;
        } else {
            const int c4 = f % (BN / 4), k = f / (BN / 4);
            *reinterpret_cast<float4 *>(Bs + k * LDB_S + c4 * 4) = v;
            if constexpr (BIASG) {   // every thread keeps the same 4 columns across k-tiles
                bsum.x += v.x; bsum.y += v.y; bsum.z += v.z; bsum.w += v.w;   // used by m-tile 0 only
            }
        }
    }
    static __device__ __forceinline__ void store(const Regs &r, float *As, float *Bs, int tid, float4 &bsum, int krows)
    {
#pragma unroll
        for (int i = 0; i < NVA; ++i) store_a(r, i, As, tid, krows);
#pragma unroll
        for (int i = 0; i < NVB; ++i) store_b(r, i, Bs, tid, bsum);
    }

    // One k-tile: multiply the tile resident in LDS stage (As, Bs) into acc (this wave takes
    // k-range `ks`); between the MFMAs (a) fetch the operand fragments RD steps ahead, (b) issue
    // the global loads of a later k-tile into register image rl, (c) move the NEXT k-tile
    // (register image rs) into the other LDS stage.  Everything except the first RD fragment
    // reads issues while the matrix pipe is busy, and those are not the step's own: they arrive in `f`, read by the step of
    // the tile before (by the head of GemmKernel::run for the first tile).  NCH independent accumulator chains
    // (a single dependent v_mfma_f32_32x32x2_f32 chain only reaches 90 % of the issue rate).
    //
    // A step that stages the next tile (DO_STORE) contains the k-tile's barrier, behind MFMA step BAR (in the forwards in front
    // of the tile's last MFMA, which then covers what follows), and behind it reads the first RD fragments of the NEXT tile from
    // the other stage into `f`.  Why the two stages suffice wherever BAR stands, with t the tile this step multiplies, in
    // stage t&1:
    //  - every fragment read of tile t is issued by step LAST_READ < BAR and completed by the lgkmcnt(0) in front of the
    //    barrier, so no wave still reads stage t&1 when a wave that has passed the barrier starts the next step and its
    //    ds_writes of tile t+2 overwrite it;
    //  - every ds_write of tile t+1 sits in a slot <= BAR (store_slot) and is completed by the same wait, so behind the
    //    barrier tile t+1 is whole and visible in stage (t+1)&1: the reads into `f` are reads behind the barrier that
    //    publishes their tile, and that stage is next written behind barrier t+1;
    //  - the MFMAs behind the barrier use registers only.
    // Both waits are the barrier's own: __syncthreads() is a workgroup-scope release fence, s_barrier, and an acquire fence, and
    // for LDS the release is the s_waitcnt lgkmcnt(0) in front of s_barrier, which retires this wave's ds_reads and ds_writes
    // alike; the acquire keeps the reads into `f` behind it.  A bare __builtin_amdgcn_s_barrier() here would promise neither.
    // With BAR = NK - 1 the order of the LDS instructions is the one the loop had when every step read its own first fragments;
    // what the hand-over changes there is that the reads sit in the block of the barrier, so hipcc places the scalar k-advance of
    // the next loads (ten SALU instructions) behind them, in the shadow of the LDS round trip, and no longer between the last
    // MFMA and the barrier, where every wave paid it before it arrived (-2 us per C2 step, profiles/r19_kloop_barrier.txt).
    // The last tile's step (no DO_STORE) has no barrier and leaves `f` alone.
    struct Frags { float a[RD][TM], b[RD][TN]; };
    static __device__ __forceinline__ void read_first(Frags &f, const float *As, const float *Bs, int ks, int a_off, int b_off, int kh)
    {
        const float *ap = As + (step_row(ks, 0) + kh) * LDA_S + a_off;
        const float *bp = Bs + (step_row(ks, 0) + kh) * LDB_S + b_off;
#pragma unroll
        for (int s = 0; s < RD; ++s) {
#pragma unroll
            for (int i = 0; i < TM; ++i) f.a[s][i] = ap[step_row(0, s) * LDA_S + i * 32];
#pragma unroll
            for (int j = 0; j < TN; ++j) f.b[s][j] = bp[step_row(0, s) * LDB_S + j * 32];
        }
    }
    template <bool DO_STORE, bool DO_LOAD>
    static __device__ __forceinline__ void step(const float *As, const float *Bs, f32x16 (&acc)[NCH][TM][TN], int ks,
                                                int a_off, int b_off, int kh, const Regs &rs, float *AsN, float *BsN,
                                                Regs &rl, const float *pa, const float *pb, Offs &o, int tid,
                                                float4 &bsum, int krows, Frags &f)
    {
        const float *ap = As + (step_row(ks, 0) + kh) * LDA_S + a_off;        // step s reads rows step_row(ks, s) + kh
        const float *bp = Bs + (step_row(ks, 0) + kh) * LDB_S + b_off;
        float av[NK][TM], bv[NK][TN];
        // hipcc's scheduler otherwise sinks every ds_read next to its MFMA (one exposed LDS latency
        // per pair), gathers the ds_writes in front of the barrier and the global loads + their
        // address arithmetic in front of the first MFMA; pin the intended interleave.
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s = 0; s < RD; ++s) {
#pragma unroll
            for (int i = 0; i < TM; ++i) av[s][i] = f.a[s][i];
#pragma unroll
            for (int j = 0; j < TN; ++j) bv[s][j] = f.b[s][j];
        }
        int pl = 0, ps = 0;
#pragma unroll
        for (int s = 0; s < NK; ++s) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[step_chain(s)][i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s][i], bv[s][j], acc[step_chain(s)][i][j], 0, 0, 0);
            if (s == 0) __builtin_amdgcn_sched_barrier(0);     // (the tile's first MFMA goes in front of its first reads and loads)
            if (s + RD < NK) {
#pragma unroll
                for (int i = 0; i < TM; ++i) av[s + RD][i] = ap[step_row(0, s + RD) * LDA_S + i * 32];
#pragma unroll
                for (int j = 0; j < TN; ++j) bv[s + RD][j] = bp[step_row(0, s + RD) * LDB_S + j * 32];
            }
            if constexpr (DO_LOAD) {
#pragma unroll
                for (int q = 0; q < NP; ++q) {               // load piece q goes after MFMA step load_slot(q) (spread evenly over the k-tile)
                    if (q == pl && load_slot(q) == s) {
                        if (q < NVA) load_a(rl, q, pa, o); else load_b(rl, q - NVA, pb, o);
                        ++pl;
                    }
                }
            }
            if constexpr (DO_STORE) {
#pragma unroll
                for (int q = 0; q < NP; ++q) {               // store piece q goes after MFMA step store_slot(q) (spread over [0, BAR])
                    if (q == ps && store_slot(q) == s) {
                        if (q < NVA) store_a(rs, q, AsN, tid, krows); else store_b(rs, q - NVA, BsN, tid, bsum);
                        ++ps;
                    }
                }
                if (s == BAR) {
                    __syncthreads();
                    __builtin_amdgcn_sched_barrier(0);
                    read_first(f, AsN, BsN, ks, a_off, b_off, kh);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
};

// ------------------------------------------------------------------ launch geometry shared by every GEMM family
// XCD-aware tile map: workgroup b of a problem runs on XCD b % 8 (a grouped launch keeps that true for the problem-relative index,
// pack_tiles in bp_step.hip).  With a multiple of 8 n-tiles each XCD gets a contiguous range of `per` n-panels, so the W / dEdX
// column panels it streams stay in its private L2 and are fetched into it once instead of eight times; forward and dgrad walk m
// fastest inside it (the workgroups that share an n-panel run back to back).  M_SLOW is the weight gradient's order: its few
// n-panels (dEdX columns) stay hot anyway, so it walks the m-panels (activation columns) slowly and the `per` workgroups that share
// one run back to back -- the panel is fetched into this L2 once instead of being evicted by the W / delta stream before its next use.
template <bool M_SLOW>
__device__ __forceinline__ void xcd_tile(int b, int tiles_m, int tiles_n, int &tile_m, int &tile_n)
{
    if ((tiles_n & 7) == 0) {
        const int xcd = b & 7, j = b >> 3, per = tiles_n >> 3;
        if constexpr (M_SLOW) { tile_n = xcd * per + j % per; tile_m = j / per; }
        else { tile_n = xcd * per + j / tiles_m; tile_m = j % tiles_m; }
    } else { tile_m = b % tiles_m; tile_n = b / tiles_m; }       // any other n-tile count: plain column-major order
}
// The problem of a grouped launch (MultiArgs, BfWgradMulti) that owns entry b of the concatenated tile list: problem p has the
// entries first_tile[p] .. first_tile[p + 1] - 1.  A walk over growing entries continues from the p it found last.
template <class Multi>
__device__ __forceinline__ int problem_of(const Multi &a, int b, int p)
{
    while (p + 1 < a.n && b >= a.first_tile[p + 1]) ++p;
    return p;
}

// Host side of GemmKernel::run's one-tile-per-workgroup contract, checked in front of every launch that wraps it (bp_step.hip;
// tests/cpp/one_tile_driver.cc): a problem's workgroups -- its share of the launch, the stride a walk over tiles would have --
// cover its tile list (times the k-slices of a split launch), so no tile is left to a second trip that does not exist.
static inline bool covers_tiles(long long workgroups, const GemmArgs &g, int slices = 1)
{
    return g.tiles_m >= 0 && g.tiles_n >= 0 && workgroups >= (long long)g.tiles_m * g.tiles_n * slices;
}
template <class Multi>
static inline bool multi_covers_tiles(const Multi &a)
{
    if (a.n < 1 || a.n > 4) return false;
    for (int p = 0; p < a.n; ++p)
        if (!covers_tiles((long long)a.first_tile[p + 1] - a.first_tile[p], a.g[p])) return false;
    return true;
}

// The workgroup program of one GEMM problem: workgroup `b` of the problem computes tile b of it, ONE tile per workgroup (a b at or
// past the tile count is a padding entry and returns).  Wrapped by bp_gemm (one problem per launch), bp_gemm_multi (up to four
// independent problems in one launch) and bp_out_split_stage; the host gives every problem at least as many workgroups as it has
// tiles and refuses a launch that would not (covers_tiles above).  There is no walk over further tiles: no launch of the
// library ever took a second trip, and the loop cost every body a second copy of the tile loads, a barrier and a second tile map
// (profiles/r16_gemm_tail.txt section 2).  bp_wgrad_dma, the one persistent launch, has its own walk.
template <int BM, int BN, int BK, int WM, int WN, bool A_KC, bool B_KC, int EPI>
struct GemmKernel {
    using Cfg = GemmCfg<BM, BN, BK, WM, WN, A_KC, B_KC, EPI>;
    static constexpr int KS = Cfg::KS, TM = Cfg::TM, TN = Cfg::TN;
    static constexpr int A_STAGE = Cfg::A_STAGE, B_STAGE = Cfg::B_STAGE, STAGE = A_STAGE + B_STAGE;
    static constexpr bool BIASG = Cfg::BIASG;
    static constexpr int RED = (KS > 1) ? KS * WM * WN * 16 * 64 : 0;     // k-split exchange area (floats)
    static constexpr int BIASRED = BIASG ? 256 / (BN / 4) * BN : 0;
    static constexpr int SMEM0 = (2 * STAGE > RED) ? 2 * STAGE : RED;
    static constexpr int SMEM = SMEM0 > BIASRED ? SMEM0 : BIASRED;       // floats of LDS
    // workgroups per CU the register allocator must leave room for (launch bounds)
    static constexpr int MIN_WG = (SMEM * 4 > 80 * 1024) ? 1 : 2;

static __device__ __forceinline__ void run(const GemmArgs &g_in, const EpiArgs &e_in, int b, int block_y, float *smem)
{
    using Regs = typename Cfg::Regs;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform => SGPR row bases
    constexpr int EPI_E = EPI == EPI_OUT_SPLIT ? EPI_FWD_OUT : EPI == EPI_OUT_SPLIT_LOGI ? EPI_FWD_OUT_LOGI : EPI;      // the epilogue proper
#ifdef BP_TRACE
#define TRACE(i) do { if (tid == 0 && g_in.trace) { g_in.trace[(size_t)b * 8 + (i)] = wall_clock64();           \
        if ((i) == 0) g_in.trace[(size_t)b * 8 + 6] = clock64();   /* shader-clock counter: */           \
        if ((i) == 3) g_in.trace[(size_t)b * 8 + 7] = clock64();   /* effective MHz of the run */        \
    } } while (0)
#else
#define TRACE(i) ((void)0)
#endif
#define K0_OF(t) (((t) * BK) < last_k0 ? ((t) * BK) : last_k0)
#define PA(t) Cfg::base_a(g, m0, K0_OF(t))
#define PB(t) Cfg::base_b(g, n0, K0_OF(t))
#define AS(buf) (smem + (buf) * STAGE)
#define BS(buf) (smem + (buf) * STAGE + A_STAGE)

    TRACE(0);                                     // (development build: at the entry, so that the trace's prologue contains the head)
    // ---- head: the loads of k-tiles 0 and 1 of the workgroup's tile go out before anything else.  A workgroup is alone on
    // its SIMDs when it starts, so whatever runs in front of its first load is paid as latency with nothing in flight.
    // Only the operand side of the arguments is read here (one batch of scalar loads, one wait); the epilogue's arguments, the
    // accumulators and the epilogue's own fetches follow behind the loads.
    GemmArgs g = operand_args(g_in);              // (what else a kernel needs of g_in it reads where it uses it)
    if constexpr (epi_out_split(EPI)) {      // this workgroup row's k-slice
        const size_t kz = (size_t)block_y * g_in.k_split;
        g.A += A_KC ? kz : kz * g.lda;
        g.B += B_KC ? kz : kz * g.ldb;
    }
    BP_PIN_OPERANDS(g);
    const int tiles = g.tiles_m * g.tiles_n;
    if (b >= tiles) return;                      // (padding entry of a grouped launch)
    const int nt = (g.K + BK - 1) / BK, last_k0 = (nt - 1) * BK;
    typename Cfg::Offs offs;
    Cfg::make_offs(offs, g, tid);
    int tile_m, tile_n;
    xcd_tile<BIASG>(b, g.tiles_m, g.tiles_n, tile_m, tile_n);
    const int m0 = tile_m * BM, n0 = tile_n * BN;
    // Two register images hold k-tiles t+1 (landed, being staged) and t+2 (in flight) of the software pipeline below.  Every load
    // is unconditional (past the end the tile index is clamped and the data ignored): a conditional load turns into a phi + copy
    // and hipcc then waits for it right away.
    Regs r0, r1;
    Cfg::load(r0, PA(0), PB(0), offs);
    Cfg::load(r1, PA(1), PB(1), offs);
    __builtin_amdgcn_sched_barrier(0);

    // The epilogue's arguments are read HERE, behind the loads, at an offset the optimiser does not know to be 0.  Read plainly
    // (e = e_in), their scalar loads are hoisted into the blocks in front of the tile map (a sched_barrier orders one basic block),
    // and the first use of any of them there -- hipcc spills one into a VGPR lane -- is a second full scalar wait in front of the
    // first operand load.  WHEN THE COMPILER CHANGES, rerun the listing check of profiles/r15_gemm_head.txt section 1 and look for
    // copies of r1 in front of the k-loop (profiles/r16_gemm_tail.txt section 2), and for VALU instructions in the steady-state
    // loop (profiles/r17_kloop_pairs.txt section 1: there are none, every operand load is global_load_dwordx4 v, v_off, s[base]),
    // and for the shape of a k-tile around its barrier (profiles/r19_kloop_barrier.txt section 4: one s_barrier per tile, the
    // first reads of the next tile and the scalar k-advance right behind it, nothing but an s_waitcnt lgkmcnt in front of the
    // next tile's first MFMA):
    // this asm, BP_PIN_OPERANDS, the asm in bp_gemm_multi, the one in GemmCfg::lane_off and the branch weight on the k-loop steer
    // hipcc by side effects it does not promise, and no test on a machine without a GPU holds the instruction and wait counts in
    // front of the first global_load_dwordx4 or the first MFMA, or the instruction mix of the loop.
    int behind = 0;
    asm volatile("" : "+s"(behind));
    const EpiArgs e = *reinterpret_cast<const EpiArgs *>(reinterpret_cast<const char *>(&e_in) + behind);
    const int ks = wave / (WM * WN), wq = wave % (WM * WN), wm = wq / WN, wn = wq % WN;
    const int a_off = wm * TM * 32 + (lane & 31), b_off = wn * TN * 32 + (lane & 31);
    const int kh = lane >> 5;

    float4 bsum = make_float4(0.f, 0.f, 0.f, 0.f);   // bias-gradient partial sums (wgrad; used by m-tile 0)
    const bool do_bias = BIASG && tile_m == 0;

    constexpr int NCH = Cfg::NCH;
    f32x16 accs[NCH][TM][TN];
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) accs[c][i][j][r] = 0.0f;

    // Epilogue inputs (bias / targ / y_prev / W, delta) are fetched up front so their HBM/L2 latency
    // hides under the k-loop (same lane->element map as the accumulator).
    EpiPre pre[TM][TN];
    const int mb0 = m0 + wm * TM * 32, nb0 = n0 + wn * TN * 32;
    if constexpr (KS == 1) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) epilogue_fetch<EPI_E, 0, 16>(e, mb0 + i * 32, nb0 + j * 32, lane, pre[i][j]);
    } else {
        static_assert(KS == 1 || (TM == 1 && TN == 1), "in-workgroup k-split needs one block per wave");
        if (ks == 0) epilogue_fetch<EPI_E, 0, 16 / KS>(e, mb0, nb0, lane, pre[0][0]);
        if (ks == 1) epilogue_fetch<EPI_E, 16 / KS, 16 / KS>(e, mb0, nb0, lane, pre[0][0]);
        if constexpr (KS == 4) {
            if (ks == 2) epilogue_fetch<EPI_E, 8, 4>(e, mb0, nb0, lane, pre[0][0]);
            if (ks == 3) epilogue_fetch<EPI_E, 12, 4>(e, mb0, nb0, lane, pre[0][0]);
        }
    }

    // ---- software pipeline: LDS holds tile t (double buffered), the register images r0 / r1 tiles t+1 and t+2.  One barrier per k-tile,
    // inside the step that stages the next tile (GemmCfg::step), which also reads that tile's first fragments behind it.
// multiply stage `buf`; ST: store image RS (k-tile TS) into the other stage; LD: load tile TL into image RL
#define STEP(ST, LD, buf, RS, TS, RL, TL)                                                                  \
    Cfg::template step<ST, LD>(AS(buf), BS(buf), accs, ks, a_off, b_off, kh, RS, AS((buf) ^ 1), BS((buf) ^ 1),    \
                               RL, PA(TL), PB(TL), offs, tid, bsum, g.K - (TS) * BK, frags)
    Cfg::store(r0, AS(0), BS(0), tid, bsum, g.K);
    __syncthreads();
    TRACE(1);
    typename Cfg::Frags frags;                    // the first fragments of the tile the next STEP multiplies
    Cfg::read_first(frags, AS(0), BS(0), ks, a_off, b_off, kh);
    // Invariant at the top of iteration t: LDS stage t&1 holds tile t; tile t+1 is in flight / landed in registers
    // (r1 for even t, r0 for odd t).  The iteration multiplies tile t and, between the MFMAs, issues the global loads of tile
    // t+2, moves tile t+1 into the other stage and, behind its barrier, reads the first fragments of tile t+1.  The steady-state
    // loop contains no conditionals (a conditional step makes hipcc copy the accumulators between register ranges every
    // iteration); the last one or two tiles run after.
    // The loop is marked as the expected path (every layer of a real net has three or more k-tiles).  Without the mark hipcc
    // keeps the image r1 that the head loaded in other registers than the loop's r1 and copies it over in front of the loop,
    // behind a full vmcnt(0): the first MFMA then waits for all of k-tile 1 (profiles/r16_gemm_tail.txt section 2).
    // One barrier per k-tile stays, also in the wide forward's 64-deep loop: two of its tiles per LDS stage (one barrier per 32
    // MFMAs, behind a first step of one tile) were built twice and measured 4.7 and 10.1 us per step SLOWER than this loop
    // (profiles/r17_kloop_pairs.txt section 3).  What the loop must not contain is VALU work: 12 64-bit adds per two k-tiles cost the
    // forward a tenth of its k-loop (GemmCfg::lane_off).
    int t = 0, buf = 0;
    if (__builtin_expect(nt >= 3, 1))
    for (; t + 3 <= nt; t += 2) {
        STEP(true, true, 0, r1, t + 1, r0, t + 2);
        STEP(true, true, 1, r0, t + 2, r1, t + 3);
    }
    if (nt - t == 2) {
        STEP(true, false, 0, r1, t + 1, r0, 0);
        buf = 1;
    }
    STEP(false, false, buf, r0, 0, r0, 0);    // last tile: nothing left to stage or fetch, no barrier in it
    __syncthreads();                          // (every wave is past its reads of the stages: the exchange areas below reuse them)
    TRACE(2);
#undef STEP
    // Every load issued so far has landed or is dead (the clamped image behind the last k-tile).  Said once, here: the epilogue's
    // inputs are now fetched BEHIND the first operand loads, and on the one-k-tile path no later wait covers them, so hipcc would
    // drain in front of every use of one -- also between the epilogue's own stores, waiting for each to be acknowledged.
    __builtin_amdgcn_s_waitcnt(0x0F70);           // vmcnt(0), expcnt and lgkmcnt left alone
    // fold the independent accumulator chains
    f32x16 (&acc)[TM][TN] = accs[0];
    if constexpr (NCH == 2) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] += accs[1][i][j][r];
    }

    // ---- in-workgroup k-split: exchange partial sums through LDS (smem is free after the last
    // barrier); afterwards wave group ks owns registers [ks*16/KS, (ks+1)*16/KS) of its block
    if constexpr (KS > 1) {
        if (ks == 0) ksplit_give<KS, 0>(acc[0][0], smem, wq, lane);
        if (ks == 1) ksplit_give<KS, 1>(acc[0][0], smem, wq, lane);
        if constexpr (KS == 4) {
            if (ks == 2) ksplit_give<KS, 2>(acc[0][0], smem, wq, lane);
            if (ks == 3) ksplit_give<KS, 3>(acc[0][0], smem, wq, lane);
        }
        __syncthreads();
        if (ks == 0) ksplit_take<KS, 0>(acc[0][0], smem, wq, lane);
        if (ks == 1) ksplit_take<KS, 1>(acc[0][0], smem, wq, lane);
        if constexpr (KS == 4) {
            if (ks == 2) ksplit_take<KS, 2>(acc[0][0], smem, wq, lane);
            if (ks == 3) ksplit_take<KS, 3>(acc[0][0], smem, wq, lane);
        }
        if constexpr (BIASG) __syncthreads();
    }

    // ---- bias gradient: column sums of the dEdX panel this workgroup streamed (kernAccSumrow)
    if constexpr (BIASG && !B_KC) {
        if (do_bias) {
            constexpr int CG = BN / 4, RG = 256 / CG;          // column groups x row groups
            float *red = smem;                                 // [RG][BN]
            const int c4 = tid % CG, rg = tid / CG;
            *reinterpret_cast<float4 *>(red + rg * BN + c4 * 4) = bsum;
            __syncthreads();
            if (tid < BN && (n0 + tid) < e.n_limit) {
                float s = 0.f;
#pragma unroll
                for (int r = 0; r < RG; ++r) s += red[r * BN + tid];
                const int n = n0 + tid;
                if constexpr (EPI == EPI_WGRAD_UPDATE) {
                    if (e.rdiv != 0.0f) bias_update<true>(e, n, s); else bias_update<false>(e, n, s);
                } else {
                    e.bias_g[n] = s;
                }
            }
        }
    }

    // ---- split-K across workgroups in one launch (EPI_OUT_SPLIT): every slice writes its partial tile and takes a ticket from the
    // tile's word (last_arrival); the last of the OUT_SPLITS arrivals of this launch sums the slices and runs the output epilogue,
    // the others are done.  (The slices of a tile are workgroups b, b + tiles, ... of the launch -- on one XCD, block index mod 8,
    // whenever the tile count is a multiple of 8.)
    bool finish = true;
    if constexpr (epi_out_split(EPI)) {
        static_assert(KS == 4 && OUT_SPLITS == 4, "one 32x32 block per workgroup, four registers of it per wave");
        float *mine = g_in.ks_slab + (size_t)block_y * g_in.slab_stride;
        if (ks == 0) out_split_store<0>(e, mine, mb0, nb0, acc[0][0], lane);
        if (ks == 1) out_split_store<4>(e, mine, mb0, nb0, acc[0][0], lane);
        if (ks == 2) out_split_store<8>(e, mine, mb0, nb0, acc[0][0], lane);
        if (ks == 3) out_split_store<12>(e, mine, mb0, nb0, acc[0][0], lane);
        // (the ticket's LDS word: its first barrier also puts every wave past its reads of the exchange area)
        finish = last_arrival(g_in.ks_ticket + b, reinterpret_cast<unsigned *>(smem), OUT_SPLITS);
        if (finish) {
            if (ks == 0) out_split_sum<0>(e, g_in.ks_slab, g_in.slab_stride, mb0, nb0, acc[0][0], lane);
            if (ks == 1) out_split_sum<4>(e, g_in.ks_slab, g_in.slab_stride, mb0, nb0, acc[0][0], lane);
            if (ks == 2) out_split_sum<8>(e, g_in.ks_slab, g_in.slab_stride, mb0, nb0, acc[0][0], lane);
            if (ks == 3) out_split_sum<12>(e, g_in.ks_slab, g_in.slab_stride, mb0, nb0, acc[0][0], lane);
        }
    }

    if constexpr (EPI == EPI_WGRAD_UPDATE) {
        // the fused update: multiply or divide (update_delta, bp_device.h), chosen here for the whole tile
        static_assert(KS == 1, "the update runs on whole blocks");
        if (e.rdiv != 0.0f) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    epilogue_block<EPI_E, 0, 16, true>(e, mb0 + i * 32, nb0 + j * 32, acc[i][j], lane, pre[i][j]);
        } else {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    epilogue_block<EPI_E, 0, 16, false>(e, mb0 + i * 32, nb0 + j * 32, acc[i][j], lane, pre[i][j]);
        }
    } else if constexpr (KS == 1) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
                epilogue_block<EPI_E, 0, 16>(e, mb0 + i * 32, nb0 + j * 32, acc[i][j], lane, pre[i][j]);
    } else if (finish) {
        if (ks == 0) epilogue_block<EPI_E, 0, 16 / KS>(e, mb0, nb0, acc[0][0], lane, pre[0][0]);
        if (ks == 1) epilogue_block<EPI_E, 16 / KS, 16 / KS>(e, mb0, nb0, acc[0][0], lane, pre[0][0]);
        if constexpr (KS == 4) {
            if (ks == 2) epilogue_block<EPI_E, 8, 4>(e, mb0, nb0, acc[0][0], lane, pre[0][0]);
            if (ks == 3) epilogue_block<EPI_E, 12, 4>(e, mb0, nb0, acc[0][0], lane, pre[0][0]);
        }
    }
    TRACE(3);
#undef K0_OF
#undef PA
#undef PB
#undef AS
#undef BS
#undef TRACE
}
};   // GemmKernel

// TAG only separates instantiations by name (profilers report per kernel name): 1 = input-layer forward.
template <int BM, int BN, int BK, int WM, int WN, bool A_KC, bool B_KC, int EPI, int TAG = 0>
__global__ __launch_bounds__(256, (GemmKernel<BM, BN, BK, WM, WN, A_KC, B_KC, EPI>::MIN_WG)) void bp_gemm(const GemmArgs g, const EpiArgs e)
{
    using K = GemmKernel<BM, BN, BK, WM, WN, A_KC, B_KC, EPI>;
    __shared__ __attribute__((aligned(16))) float smem[K::SMEM];
    K::run(g, e, blockIdx.x, blockIdx.y, smem);
}

// Up to 4 INDEPENDENT problems of the same tile configuration in one launch (grouped GEMM): the
// wgrad+update of several layers after the last dgrad of the step.  Each problem alone is short
// (K = bunch = 256: 16 k-tiles per workgroup) and its workgroups run in lockstep -- prologue, MFMA
// phase and the W/delta write-back each hit the chip all at once.  In one launch of ~7 rounds of
// workgroups the rounds drift apart, so the HBM phases of some overlap the MFMA phases of others
// and only one launch boundary / cold start is paid.
struct MultiArgs {
    GemmArgs g[4];
    EpiArgs e[4];
    int first_tile[5];       // first_tile[p] .. first_tile[p+1]-1 = workgroups of problem p
    int n;
};
#ifndef BP_TRACE            // (the development build's GemmArgs carries one more pointer)
// (920 bytes with EpiArgs::rdiv too: it lies in the word of EpiArgs::scale, so no problem's fields moved and the batched scalar head
// of bp_gemm_multi reads what it read)
static_assert(sizeof(MultiArgs) == 920 && offsetof(MultiArgs, first_tile) == 896 && offsetof(MultiArgs, n) == 916, "MultiArgs layout");
#endif
template <class K>
__global__ __launch_bounds__(256, K::MIN_WG) void bp_gemm_multi(const MultiArgs a)
{
    __shared__ __attribute__((aligned(16))) float smem[K::SMEM];
    // From the block index to the first operand address in ONE scalar round trip for problem 0 (the dgrad launches of the step hold
    // one problem each): the tile list and problem 0's operand fields lie at constant offsets of the argument block and are read as
    // one batch.  (Indexed with a p that is itself loaded -- problem_of, then first_tile[p], then g[p] -- every step was a dependent
    // scalar load with a full wait in front of the workgroup's first operand load.)  A later problem pays one more round trip for
    // its own fields; the epilogue's arguments are read through p behind the operand loads (K::run).
    const int b = blockIdx.x;
    int n = a.n, first = a.first_tile[0], next = a.first_tile[1];
    GemmArgs g = a.g[0];                          // (the whole struct: K::run may read any field; only those it reads are loaded)
    BP_PIN_OPERANDS(g, "+s"(n), "+s"(first), "+s"(next));
    int p = 0;
    if (n > 1 && b >= next) {                     // a later problem: walk the list
        asm volatile("");                         // (not to be speculated: it would put the indexed loads in front of every workgroup)
        p = problem_of(a, b, 1);
        g = a.g[p];
        first = a.first_tile[p]; next = a.first_tile[p + 1];
    }
    K::run(g, a.e[p], b - first, 0, smem);
}

// ------------------------------------------------------------------ small kernels
// On-device frame stacking, one bunch at a time (include/bp_c_api.h, bp_window_chunk; the host does it per chunk,
// Interface.cc:757-797).  Rows 0..rows-1 of the bunch (the caller passes the tables already offset to its first sample)
// become the input tile x [rows][ld]: `win` consecutive floats of the raw frame matrix starting at frame win_start[i]
// (a context window is contiguous in memory), then the sentence's noise-aware block, then zero padding up to ld -- with
// the visible-layer dropout of BP_GPU.cu:536-539 drawn on the way (thresh != 0; the Philox words of bp_mask_input:
// key (global frame >> 2, unit), layer 0) -- and the bunch's targets t [rows][ldt] = targ_frames[targ_frame[i]]
// (Interface.cc:792-797; t may be null).  The stacked chunk (n_samples x 2827 floats) and its masked copy are never
// materialised: what stays resident are the raw frames (11x fewer bytes) and this one L2-sized tile per bunch.
// One thread = one column x 4 consecutive rows (= one Philox block; coalesced 4-byte accesses: raw rows of 257 floats
// are not 16-byte aligned); blockIdx.y < yb_in sweeps the input columns, the rest the target columns.
struct StageArgs {
    float *x; int ld, width;                      // staged input tile [rows][ld], unpadded width
    const float *fea; int fea_dim, win;           // raw frames [n_frames][fea_dim]; win = context * fea_dim floats per window
    const float *nat; const int *win_start, *nat_row;   // noise-aware rows; per-sample tables (already offset to the bunch's first sample); win_start == null: stacked rows (stage_rows_block)
    int rows; uint32_t thresh; int frame_off; uint32_t seed_lo, seed_hi, step;
    float *t; int ldt, twidth; const float *targ_frames; const int *targ_frame;   // staged targets (t may be null)
    int yb_in;                                    // column blocks of the input part; blocks by >= yb_in sweep the target columns
    int nbx;                                      // row blocks (rows / 4, rounded up): block (bx, by) of the flat index e is bx = e % nbx, by = e / nbx
};
// The same for a STACKED chunk (win_start == null: the caller handed rows that are already stacked, BP_GPU.cu:127-130): rows
// r0..r0+3 of the bunch are copied as they lie, fea = first row of the bunch, fea_dim = its leading dimension (a multiple of 4
// floats, rows 16-byte aligned), with the visible-layer dropout of BP_GPU.cu:536-539 applied on the way instead of in place in
// the cached chunk.  One thread = 4 rows x 4 consecutive columns: four 16-byte loads, four Philox blocks (one per column, all
// four words used), four 16-byte stores.
__device__ __forceinline__ void stage_rows_block(const StageArgs &a, int bx, int by, int tx)
{
    const int r0 = bx * 4, c = (by * 256 + tx) * 4;
    if (c >= a.ld) return;
    float4 v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
        v[j] = *reinterpret_cast<const float4 *>(a.fea + (size_t)(r0 + j < a.rows ? r0 + j : a.rows - 1) * a.fea_dim + c);   // (clamped, unconditional: four loads in flight)
    if (a.thresh) {
        // one Philox block per column; the loop is NOT unrolled (four inlined copies of the ten rounds were 3 KB of a launch whose code
        // shares the instruction caches with the rest of the step): the decisions are collected as bits
        // (bit 4k + j: row j of column k) and applied with constant indices
        uint32_t drop = 0;
#pragma unroll 1
        for (int k = 0; k < 4; ++k) {
            if (c + k >= a.width) break;
            uint32_t w[4];
            drop_words4(w, r0, c + k, a.frame_off, (uint32_t)a.width, 0u, a.step, a.seed_lo, a.seed_hi);
            const uint32_t m = (w[0] < a.thresh ? 1u : 0u) | (w[1] < a.thresh ? 2u : 0u) | (w[2] < a.thresh ? 4u : 0u) | (w[3] < a.thresh ? 8u : 0u);
            drop |= m << (4 * k);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (drop & (1u << (0 + j))) v[j].x = 0.0f;
            if (drop & (1u << (4 + j))) v[j].y = 0.0f;
            if (drop & (1u << (8 + j))) v[j].z = 0.0f;
            if (drop & (1u << (12 + j))) v[j].w = 0.0f;
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) if (r0 + j < a.rows) *reinterpret_cast<float4 *>(a.x + (size_t)(r0 + j) * a.ld + c) = v[j];
}
__device__ __forceinline__ void stage_block(const StageArgs &a, int bx, int by, int tx)
{
    if (!a.win_start) { stage_rows_block(a, bx, by, tx); return; }
    const int r0 = bx * 4;
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    // The table entries of the four rows are block-uniform (scalar loads).  Rows past the bunch's end read the LAST row's entry and
    // data (unconditional, clamped) and are only kept from the stores: guarded per row, every row became s_load, s_waitcnt, load --
    // four dependent scalar round trips in front of the four row loads of a launch that is nothing but latency.
    int rr[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) rr[j] = r0 + j < a.rows ? r0 + j : a.rows - 1;
    if (by >= a.yb_in) {
        const int c = (by - a.yb_in) * 256 + tx;
        if (c >= a.ldt) return;
        if (c < a.twidth) {
            int tf[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) tf[j] = a.targ_frame[rr[j]];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = a.targ_frames[(size_t)tf[j] * a.twidth + c];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) if (r0 + j < a.rows) a.t[(size_t)(r0 + j) * a.ldt + c] = v[j];
        return;
    }
    const int c = by * 256 + tx;
    if (c >= a.ld) return;
    // all four rows' loads first (independent), the Philox block meanwhile, then the four stores
    if (c < a.win) {
        int ws[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) ws[j] = a.win_start[rr[j]];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = a.fea[(size_t)ws[j] * a.fea_dim + c];
    } else if (c < a.width) {
        int nr[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) nr[j] = a.nat_row[rr[j]];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = a.nat[(size_t)nr[j] * a.fea_dim + (c - a.win)];
    }
    uint32_t w[4] = {~0u, ~0u, ~0u, ~0u};
    if (a.thresh && c < a.width) drop_words4(w, r0, c, a.frame_off, (uint32_t)a.width, 0u, a.step, a.seed_lo, a.seed_hi);
#pragma unroll
    for (int j = 0; j < 4; ++j) if (r0 + j < a.rows) a.x[(size_t)(r0 + j) * a.ld + c] = w[j] < a.thresh ? 0.0f : v[j];
}
__global__ __launch_bounds__(256) void bp_stage_bunch(const StageArgs a)
{
    stage_block(a, blockIdx.x % a.nbx, blockIdx.x / a.nbx, threadIdx.x);
}

// Injected visible-layer mask (bp_train_resident_masked, parity tests): out[f][u] = mask[f][u] ? 0 : in[f][u]
__global__ void bp_apply_mask(const float *in, float *out, int ld, int width, const uint8_t *mask, int n_frames)
{
    const int u = blockIdx.x * blockDim.x + threadIdx.x, f = blockIdx.y;
    if (u >= ld || f >= n_frames) return;
    float v = in[(size_t)f * ld + u];
    if (u < width && mask[(size_t)f * width + u]) v = 0.0f;
    out[(size_t)f * ld + u] = v;
}

// Synthetic N(0,1) fill of a padded [rows][ld] buffer (cols >= width stay 0): Philox + Box-Muller.
__global__ void bp_fill_normal(float *buf, int ld, int width, int rows, uint32_t seed_lo, uint32_t seed_hi,
                               uint32_t stream)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;   // one thread = 4 elements
    const size_t per_row = (size_t)(ld / 4);
    if (i >= per_row * (size_t)rows) return;
    const size_t r = i / per_row; const int c = (int)(i % per_row) * 4;
    uint32_t w0 = (uint32_t)i, w1 = (uint32_t)(i >> 32), w2 = stream, w3 = 0x5EEDu;
    philox4x32_10(w0, w1, w2, w3, seed_lo, seed_hi);
    const float u0 = (w0 + 1.0f) * 2.3283064365386963e-10f, u1 = w1 * 2.3283064365386963e-10f;
    const float u2 = (w2 + 1.0f) * 2.3283064365386963e-10f, u3 = w3 * 2.3283064365386963e-10f;
    const float r0 = sqrtf(-2.0f * logf(fminf(u0, 1.0f))), r1 = sqrtf(-2.0f * logf(fminf(u2, 1.0f)));
    float v[4] = { r0 * cosf(6.283185307179586f * u1), r0 * sinf(6.283185307179586f * u1),
                   r1 * cosf(6.283185307179586f * u3), r1 * sinf(6.283185307179586f * u3) };
    float4 o;
    o.x = (c + 0 < width) ? v[0] : 0.f; o.y = (c + 1 < width) ? v[1] : 0.f;
    o.z = (c + 2 < width) ? v[2] : 0.f; o.w = (c + 3 < width) ? v[3] : 0.f;
    *reinterpret_cast<float4 *>(buf + r * ld + c) = o;
}

// The narrow output layer's forward, split over OUT_SPLITS k-slices (EPI_OUT_SPLIT; workgroup b < n_gemm: slice b / tiles of tile
// b % tiles) AND, in the same launch, the stacking of the NEXT bunch into the other staged tile (workgroups >= n_gemm; none if
// st.nbx == 0): the layer is 320 workgroups of launch latency on a chip that is otherwise idle at that point of the step, so the next
// bunch's bp_stage_bunch (5.1 us as its own launch in front of every bunch, round 3) rides along for free.  (Rounds 3-5 ran the layer
// as two launches -- partial sums, then a reduce launch that carried the staging: 7.9 + 5.2 us at configs[1].)
template <class K>
__global__ __launch_bounds__(256, K::MIN_WG) void bp_out_split_stage(const GemmArgs g, const EpiArgs e, int n_gemm, const StageArgs st)
{
    __shared__ __attribute__((aligned(16))) float smem[K::SMEM];
    const int b = blockIdx.x;
    // (the GEMM's operand fields ride in the batch that fetches n_gemm: one scalar round trip in front of a GEMM workgroup's first
    // operand load instead of two.  The staging workgroups branch away before any GEMM setup.)
    GemmArgs gg = g;
    int ng = n_gemm;
    BP_PIN_OPERANDS(gg, "+s"(ng), "+s"(gg.k_split));
    if (b < ng) { const int tiles = gg.tiles_m * gg.tiles_n; K::run(gg, e, b % tiles, b / tiles, smem); }
    else { const int i = b - ng; stage_block(st, i % st.nbx, i / st.nbx, threadIdx.x); }
}
