// bp_rbm.hip -- C-ABI implementation (include/bp_c_api.h): layer-wise pre-training of sigmoid nets, a stack of restricted Boltzmann machines
// trained with one-step contrastive divergence (the bp_rbm_* block of include/bp_c_api.h has the definition).  gfx950 only.
//
// One CD-1 bunch of RBM l is six launches on the stack's stream (layouts: bp_rbm.h):
//   bp_rbm_pad_rows the bunch's rows from the uploaded chunk into the padded image (Xs for l = 1, else T[0])
//   bp_rbm_gemm_up (l > 1: once per layer below, mean field)  -p0 into Ps, the sample into S0;  A k-contiguous, B = W as it lies
//   bp_rbm_gemm_down  v1 = S0 . W^T + a into Xs;  W read as [n = V][k = H], k-contiguous;  the tile's part of recon
//   bp_rbm_gemm_up    p1 into Ps
//   bp_rbm_colsum  column sums gc, ga (stored or applied) and the bunch's recon
//   bp_rbm_gemm_stats gW = Xs^T . Ps over K = 2 Bp, both operands as they lie;  the store, or update_delta on W, dW
// Every GEMM is the same loop (rbm_gemm): a workgroup of four waves owns a 64 x 64 tile, each wave one 32 x 32 block of
// v_mfma_f32_32x32x2_f32; both operands go global -> registers -> LDS as [k][m] images of RBM_KT k-rows, two images per operand,
// the loads of k-tile i + 1 in flight under the MFMAs of k-tile i, one barrier per k-tile.
//
// What the determinism rests on: an output element is one chain of MFMA accumulations in k order, fixed by the shapes; the column
// sums run over the rows in four interleaved chains combined as (0 + 1) + (2 + 3); recon is a per-lane chain in register order, a
// fixed tree over the workgroup and a serial sum over the tiles; the Philox words are keyed by (row, unit, layer, applied steps).
// No float atomics, no split-K.
#include "bp_rbm.h"

#include <cmath>

#include <new>
#include <string>

#include "bp_device.h"
#include "bp_handle.h"   // (exact_rdiv alone: no handle, no state)
#include "bp_mem.h"

namespace {
constexpr int LD_KC = 66;        // LDS row of an operand that arrives k-contiguous (scalar stores: 4 LD_KC = 8 banks apart)
constexpr int LD_MC = 68;        // LDS row of an operand that arrives m-contiguous (16-byte stores)
constexpr int IMG = RBM_KT * LD_MC;
typedef float f32x4 __attribute__((ext_vector_type(4)));   // (a native vector: HIP's float4 struct kept the staged tiles in scratch)

template <bool KC>
__device__ __forceinline__ void tile_load(f32x4 (&v)[2], const float *p, int ld, int k0, int t)
{
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int f = t + 256 * i;
        if constexpr (KC) v[i] = *reinterpret_cast<const f32x4 *>(p + (size_t)(f >> 3) * ld + k0 + 4 * (f & 7));
        else v[i] = *reinterpret_cast<const f32x4 *>(p + (size_t)(k0 + (f >> 4)) * ld + 4 * (f & 15));
    }
}

template <bool KC>
__device__ __forceinline__ void tile_store(const f32x4 (&v)[2], float *img, int t)
{
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int f = t + 256 * i;
        if constexpr (KC) {
            float *q = img + 4 * (f & 7) * LD_KC + (f >> 3);
            q[0] = v[i].x; q[LD_KC] = v[i].y; q[2 * LD_KC] = v[i].z; q[3 * LD_KC] = v[i].w;
        } else {
            *reinterpret_cast<f32x4 *>(img + (f >> 4) * LD_MC + 4 * (f & 15)) = v[i];
        }
    }
}

// acc += A[64][K] . B[K][64] for this wave's 32 x 32 block.  A, B: the tile's origin; KC: element (m, k) lies at p[m * ld + k],
// else at p[k * ld + m].  K % RBM_KT == 0 and whole tiles are readable.  lds: 4 * IMG floats.
template <bool A_KC, bool B_KC>
__device__ __forceinline__ void rbm_gemm(const float *A, int lda, const float *B, int ldb, int K, float *lds, f32x16 &acc)
{
    constexpr int LA = A_KC ? LD_KC : LD_MC, LB = B_KC ? LD_KC : LD_MC;
    const int t = threadIdx.x, lane = t & 63, c = lane & 31, h = lane >> 5, w = t >> 6;
    float *ia = lds, *ib = lds + 2 * IMG;
    f32x4 ra[2], rb[2];
    tile_load<A_KC>(ra, A, lda, 0, t);
    tile_load<B_KC>(rb, B, ldb, 0, t);
    tile_store<A_KC>(ra, ia, t);
    tile_store<B_KC>(rb, ib, t);
    __syncthreads();
    const int nk = K / RBM_KT;
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        const bool more = kt + 1 < nk;
        if (more) {
            tile_load<A_KC>(ra, A, lda, (kt + 1) * RBM_KT, t);
            tile_load<B_KC>(rb, B, ldb, (kt + 1) * RBM_KT, t);
        }
        const float *pa = ia + cur * IMG + h * LA + 32 * (w & 1) + c;
        const float *pb = ib + cur * IMG + h * LB + 32 * (w >> 1) + c;
#pragma unroll
        for (int kk = 0; kk < RBM_KT; kk += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[kk * LA], pb[kk * LB], acc, 0, 0, 0);
        if (more) {
            tile_store<A_KC>(ra, ia + (cur ^ 1) * IMG, t);
            tile_store<B_KC>(rb, ib + (cur ^ 1) * IMG, t);
        }
        __syncthreads();
    }
}

__device__ __forceinline__ void zero(f32x16 &acc)
{
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
}
}  // namespace

// The lane's elements of the wave's block: rows row0 + 8 g + rr (g, rr < 4; register 4 g + rr), column col.
#define RBM_LANE_TILE                                                                                       \
    __shared__ __attribute__((aligned(16))) float lds[4 * IMG];                                             \
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;                                               \
    const int m0 = (int)blockIdx.y * RBM_TILE, n0 = (int)blockIdx.x * RBM_TILE;                             \
    const int row0 = m0 + 32 * (wv & 1) + 4 * (lane >> 5), col = n0 + 32 * (wv >> 1) + (lane & 31);         \
    f32x16 acc;                                                                                             \
    zero(acc)

__global__ __launch_bounds__(256) void bp_rbm_pad_rows(float *dst, int ld, int rows_p, const float *src, int count, int width)
{
    const size_t n = (size_t)rows_p * ld;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int r = (int)(i / ld), k = (int)(i % ld);
        dst[i] = (r < count && k < width) ? src[(size_t)r * width + k] : 0.0f;
    }
}

__global__ __launch_bounds__(256) void bp_rbm_gemm_up(const RbmUpArgs a)
{
    RBM_LANE_TILE;
    rbm_gemm<true, false>(a.X + (size_t)m0 * a.ldx, a.ldx, a.W + n0, a.ldw, a.K, lds, acc);
    const bool col_ok = col < a.cols;
    const float bias = a.c[col];                               // (c is padded: a pad column reads 0)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int r0 = row0 + 8 * g;
        uint32_t wd[4] = {0u, 0u, 0u, 0u};
        if (a.mode == RBM_UP_P0 && a.sample && col_ok && r0 < a.rows)
            drop_words4(wd, r0, col, 0, (uint32_t)a.cols, a.layer, a.t, a.seed_lo, a.seed_hi);
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const bool live = col_ok && r0 + rr < a.rows;
            const float p = live ? act_fwd(1, acc[4 * g + rr] + bias) : 0.0f;
            const size_t o = (size_t)(r0 + rr) * a.ldy + col;
            if (a.mode == RBM_UP_P0) {
                const float u = (float)(wd[rr] >> 8) * 5.9604644775390625e-8f;          // 2^-24
                a.Y[o] = live ? -p : 0.0f;
                a.S[o] = (a.sample && live) ? (u < p ? 1.0f : 0.0f) : p;
            } else {
                a.Y[o] = p;
            }
        }
    }
}

__global__ __launch_bounds__(256) void bp_rbm_gemm_down(const RbmDownArgs a)
{
    RBM_LANE_TILE;
    __shared__ double red[256];
    rbm_gemm<true, true>(a.S0 + (size_t)m0 * a.lds0, a.lds0, a.W + (size_t)n0 * a.ldw, a.ldw, a.K, lds, acc);
    const bool col_ok = col < a.cols;
    const float bias = a.a[col];
    double part = 0.0;
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int row = row0 + 8 * g + rr;
            const bool live = col_ok && row < a.rows;
            const float x = acc[4 * g + rr] + bias;
            const float v1 = live ? (a.visible ? act_fwd(1, x) : x) : 0.0f;
            const size_t o = (size_t)row * a.ldx + col;
            a.X1[o] = v1;
            const float d = live ? a.X0[o] - v1 : 0.0f;
            part += (double)d * (double)d;
        }
    red[threadIdx.x] = part;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) a.part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = red[0];
}

__global__ __launch_bounds__(256) void bp_rbm_gemm_stats(const RbmStatsArgs a)
{
    RBM_LANE_TILE;
    rbm_gemm<false, false>(a.Xs + m0, a.ldx, a.Ps + n0, a.ldp, a.K, lds, acc);
    const bool col_ok = col < a.H;
    // (the tile's 16 values as a body per form of the update's quotient -- update_delta<RCP>, bp_device.h --, chosen once below)
    auto tile_out = [&](auto rcp_tag) __attribute__((always_inline)) {
    constexpr bool RCP = decltype(rcp_tag)::value;
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int row = row0 + 8 * g + rr;
            const bool live = col_ok && row < a.V;
            const size_t o = (size_t)row * a.ldp + col;
            const float gr = acc[4 * g + rr];
            if (!a.apply) {
                a.GW[o] = live ? gr : 0.0f;
            } else if (live) {
                const float wo = a.W[o];
                const float dn = update_delta<RCP>(a.mom, a.lrate, a.wc, a.ndiv, a.rdiv, a.dW[o], gr, wo);
                a.dW[o] = dn;
                a.W[o] = wo + dn;
            }
        }
    };
    if (a.rdiv != 0.0f) tile_out(std::true_type{}); else tile_out(std::false_type{});
}

// 64 columns per workgroup; thread (x = column, y) runs chain y of the column: the rows r with r % 4 == y, ascending.
__global__ __launch_bounds__(256) void bp_rbm_colsum(const RbmBiasArgs a)
{
    __shared__ float chain[4][64];
    const int x = threadIdx.x & 63, y = threadIdx.x >> 6;
    const int j = (int)blockIdx.x * 64 + x;
    const bool on = j < a.H + a.V, hid = j < a.H;
    const int k = hid ? j : j - a.H, ld = hid ? a.ldp : a.ldx;
    float s = 0.0f;
    if (on) {
        const float *lo = (hid ? a.Ps : a.Xs) + k, *hi = lo + (size_t)a.Bp * ld;
        for (int r = y; r < a.B; r += 4) {
            // hidden: p1 + (-p0); visible: v1 - v0 -- the same difference
            const float x1 = hi[(size_t)r * ld], x0 = lo[(size_t)r * ld];
            s += hid ? x1 + x0 : x1 - x0;
        }
    }
    chain[y][x] = s;
    __syncthreads();
    if (on && y == 0) {
        const float g = (chain[0][x] + chain[1][x]) + (chain[2][x] + chain[3][x]);
        float *b = hid ? a.c : a.a, *d = hid ? a.dc : a.da;
        if (!a.apply) {
            (hid ? a.gc : a.ga)[k] = g;
        } else {
            const float bo = b[k];
            float dn;                                 // (one value per thread: its whole update is the choice)
            if (a.rdiv != 0.0f) dn = update_delta<true>(a.mom, a.lrate, 0.0f, a.ndiv, a.rdiv, d[k], g, bo);
            else dn = update_delta<false>(a.mom, a.lrate, 0.0f, a.ndiv, a.rdiv, d[k], g, bo);
            d[k] = dn;
            b[k] = bo + dn;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && a.recon) {
        double t = 0.0;
        for (int i = 0; i < a.n_part; ++i) t += a.part[i];
        *a.recon += t;
    }
}

hipError_t rbm_rows_launch(float *dst, int ld, int rows_p, const float *src, int count, int width, hipStream_t st)
{
    const size_t n = (size_t)rows_p * ld;
    const unsigned blocks = (unsigned)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024);
    hipLaunchKernelGGL(bp_rbm_pad_rows, dim3(blocks), dim3(256), 0, st, dst, ld, rows_p, src, count, width);
    return hipGetLastError();
}
hipError_t rbm_up_launch(const RbmUpArgs &a, int rows_p, int cols_p, hipStream_t st)
{
    hipLaunchKernelGGL(bp_rbm_gemm_up, dim3(cols_p / RBM_TILE, rows_p / RBM_TILE), dim3(256), 0, st, a);
    return hipGetLastError();
}
hipError_t rbm_down_launch(const RbmDownArgs &a, int rows_p, int cols_p, hipStream_t st)
{
    hipLaunchKernelGGL(bp_rbm_gemm_down, dim3(cols_p / RBM_TILE, rows_p / RBM_TILE), dim3(256), 0, st, a);
    return hipGetLastError();
}
hipError_t rbm_stats_launch(const RbmStatsArgs &a, int v_p, int h_p, hipStream_t st)
{
    hipLaunchKernelGGL(bp_rbm_gemm_stats, dim3(h_p / RBM_TILE, v_p / RBM_TILE), dim3(256), 0, st, a);
    return hipGetLastError();
}
hipError_t rbm_bias_launch(const RbmBiasArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(bp_rbm_colsum, dim3((a.H + a.V + 63) / 64), dim3(256), 0, st, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------ the stack
struct bp_rbm {
    bp_rbm_config cfg;
    int L, B, Bp, cap, Pmax;
    int P[BP_MAXLAYER];
    bp_rbm_hyper hy[BP_MAXLAYER];
    unsigned applied[BP_MAXLAYER];
    Stream st;
    Buf dev, pin_out;                       // one device block and the pinned word recon comes back in, allocated at create
    float *W[BP_MAXLAYER], *dW[BP_MAXLAYER], *c[BP_MAXLAYER], *dc[BP_MAXLAYER], *a[BP_MAXLAYER], *da[BP_MAXLAYER];
    float *Xs, *Ps, *S0, *T[2], *GW, *gc, *ga, *chunk;
    double *part, *recon;
};

namespace {
int hyper_check(const char *who, const bp_rbm_hyper *p)
{
    if (!p) return fail(BP_ERR_ARG, std::string(who) + ": null hyper-parameters");
    if (!(p->lrate >= 0.0f) || !std::isfinite(p->lrate)) return fail(BP_ERR_ARG, std::string(who) + ": lrate must be finite and >= 0");
    if (!(p->weightcost >= 0.0f) || !std::isfinite(p->weightcost))
        return fail(BP_ERR_ARG, std::string(who) + ": weightcost must be finite and >= 0");
    if (!(p->momentum >= 0.0f && p->momentum < 1.0f)) return fail(BP_ERR_ARG, std::string(who) + ": momentum must lie in [0, 1)");
    if ((p->visible != 0 && p->visible != 1) || (p->sample != 0 && p->sample != 1))
        return fail(BP_ERR_ARG, std::string(who) + ": visible and sample must be 0 or 1");
    return BP_OK;
}

int layer_check(const char *who, const bp_rbm *s, int layer)
{
    if (!s) return fail(BP_ERR_ARG, std::string(who) + ": null stack");
    if (layer < 1 || layer > s->L - 1) return fail(BP_ERR_ARG, std::string(who) + ": layer must lie in [1, numlayers - 1]");
    return BP_OK;
}

int frames_check(const char *who, const bp_rbm *s, int n_frames, const void *in)
{
    if (n_frames < 0) return fail(BP_ERR_ARG, std::string(who) + ": n_frames is negative");
    if (n_frames > s->cap) return fail(BP_ERR_ARG, std::string(who) + ": n_frames is over the stack's capacity (max_chunk_frames)");
    if (n_frames > 0 && !in) return fail(BP_ERR_ARG, std::string(who) + ": null input rows");
    return BP_OK;
}

// mean field through RBMs 1 .. upto on the `count` rows at `rows` (device, [count][s_0]); where the result lies: *res, [Bp][P_upto]
// (upto == 0: the padded rows themselves).  into_xs: the result goes to Xs (the v0 of RBM upto + 1).
hipError_t propagate(bp_rbm *s, const float *rows, int count, int upto, bool into_xs, float **res)
{
    float *cur = (upto == 0 && into_xs) ? s->Xs : s->T[0];
    hipError_t e = rbm_rows_launch(cur, s->P[0], s->Bp, rows, count, s->cfg.layersizes[0], s->st);
    for (int j = 1; j <= upto && e == hipSuccess; ++j) {
        float *dst = (j == upto && into_xs) ? s->Xs : s->T[j & 1];
        RbmUpArgs u = {};
        u.X = cur; u.W = s->W[j]; u.c = s->c[j]; u.Y = dst; u.S = nullptr;
        u.ldx = s->P[j - 1]; u.ldw = s->P[j]; u.ldy = s->P[j]; u.K = s->P[j - 1];
        u.rows = count; u.cols = s->cfg.layersizes[j]; u.mode = RBM_UP_MF;
        e = rbm_up_launch(u, s->Bp, s->P[j], s->st);
        cur = dst;
    }
    *res = cur;
    return e;
}

// One CD-1 bunch of RBM l on the B rows at `rows`: store (gradients to GW / gc / ga), apply (the update), or both -- the store
// first, so that the stored gradients are those of the weights the bunch saw (a bunch that applies nothing stores: recon comes
// from the column-sum launch).  The bunch's recon is added onto *s->recon once.
hipError_t cd1_bunch(bp_rbm *s, int l, const float *rows, bool store, bool apply)
{
    if (!apply) store = true;
    const int V = s->cfg.layersizes[l - 1], H = s->cfg.layersizes[l], Vp = s->P[l - 1], Hp = s->P[l], B = s->B, Bp = s->Bp;
    const bp_rbm_hyper &hy = s->hy[l];
    float *v0;
    hipError_t e = propagate(s, rows, B, l - 1, true, &v0);
    if (e != hipSuccess) return e;
    RbmUpArgs u = {};
    u.X = s->Xs; u.W = s->W[l]; u.c = s->c[l]; u.Y = s->Ps; u.S = s->S0;
    u.ldx = Vp; u.ldw = Hp; u.ldy = Hp; u.K = Vp; u.rows = B; u.cols = H;
    u.mode = RBM_UP_P0; u.sample = hy.sample;
    u.layer = (uint32_t)l; u.t = s->applied[l]; u.seed_lo = (uint32_t)s->cfg.seed; u.seed_hi = (uint32_t)(s->cfg.seed >> 32);
    e = rbm_up_launch(u, Bp, Hp, s->st);
    if (e != hipSuccess) return e;
    RbmDownArgs d = {};
    d.S0 = s->S0; d.W = s->W[l]; d.a = s->a[l]; d.X0 = s->Xs; d.X1 = s->Xs + (size_t)Bp * Vp; d.part = s->part;
    d.lds0 = Hp; d.ldw = Hp; d.ldx = Vp; d.K = Hp; d.rows = B; d.cols = V; d.visible = hy.visible;
    e = rbm_down_launch(d, Bp, Vp, s->st);
    if (e != hipSuccess) return e;
    u.X = s->Xs + (size_t)Bp * Vp; u.Y = s->Ps + (size_t)Bp * Hp; u.S = nullptr; u.mode = RBM_UP_P1; u.sample = 0;
    e = rbm_up_launch(u, Bp, Hp, s->st);
    bool recon_due = true;
    for (int pass = 0; pass < 2 && e == hipSuccess; ++pass) {
        if (pass == 0 ? !store : !apply) continue;
        RbmBiasArgs b = {};
        b.Xs = s->Xs; b.Ps = s->Ps; b.c = s->c[l]; b.dc = s->dc[l]; b.a = s->a[l]; b.da = s->da[l]; b.gc = s->gc; b.ga = s->ga;
        b.part = s->part; b.recon = recon_due ? s->recon : nullptr;
        b.ldx = Vp; b.ldp = Hp; b.B = B; b.Bp = Bp; b.V = V; b.H = H; b.apply = pass; b.n_part = (Bp / RBM_TILE) * (Vp / RBM_TILE);
        b.mom = hy.momentum; b.lrate = hy.lrate; b.ndiv = (float)B; b.rdiv = exact_rdiv((float)B);
        e = rbm_bias_launch(b, s->st);
        recon_due = false;
        if (e != hipSuccess) break;
        RbmStatsArgs g = {};
        g.Xs = s->Xs; g.Ps = s->Ps; g.W = s->W[l]; g.dW = s->dW[l]; g.GW = s->GW;
        g.ldx = Vp; g.ldp = Hp; g.K = 2 * Bp; g.V = V; g.H = H; g.apply = pass;
        g.mom = hy.momentum; g.lrate = hy.lrate; g.wc = hy.weightcost; g.ndiv = (float)B; g.rdiv = exact_rdiv((float)B);
        e = rbm_stats_launch(g, Vp, Hp, s->st);
    }
    if (e == hipSuccess && apply) ++s->applied[l];
    return e;
}

int dev_error(const char *who, hipError_t e) { return fail(BP_ERR_DEVICE, std::string(who) + ": " + hipGetErrorString(e)); }

hipError_t copy2d(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t height, hipMemcpyKind kind, hipStream_t st)
{
    if (width == 0 || height == 0) return hipSuccess;
    return hipMemcpy2DAsync(dst, dpitch * 4, src, spitch * 4, width * 4, height, kind, st);
}
}  // namespace

extern "C" int bp_rbm_defaults(int layer, bp_rbm_hyper *out)
{
    if (!out || layer < 1) return fail(BP_ERR_ARG, "bp_rbm_defaults: null output or layer < 1");
    out->visible = layer == 1 ? 0 : 1;
    out->lrate = layer == 1 ? 0.0005f : 0.01f;
    out->momentum = 0.9f;
    out->weightcost = 1e-5f;
    out->sample = 1;
    return BP_OK;
}

extern "C" int bp_rbm_destroy(bp_rbm *s)
{
    if (!s) return BP_OK;
    (void)hipSetDevice(s->cfg.device);
    if (s->st.s) (void)hipStreamSynchronize(s->st);
    delete s;
    return BP_OK;
}

extern "C" int bp_rbm_create(const bp_rbm_config *cfg, const float *const *weights, const float *const *hbias, const float *const *vbias,
                             bp_rbm **out)
{
    const char *who = "bp_rbm_create";
    if (!cfg || !weights || !hbias || !out) return fail(BP_ERR_ARG, std::string(who) + ": null argument");
    if (cfg->numlayers < 2 || cfg->numlayers > BP_MAXLAYER) return fail(BP_ERR_ARG, std::string(who) + ": numlayers must lie in [2, BP_MAXLAYER]");
    for (int l = 0; l < cfg->numlayers; ++l)
        if (cfg->layersizes[l] < 1) return fail(BP_ERR_ARG, std::string(who) + ": a layer size is < 1");
    if (cfg->bunchsize < 1) return fail(BP_ERR_ARG, std::string(who) + ": bunchsize is < 1");
    if (cfg->max_chunk_frames < 0) return fail(BP_ERR_ARG, std::string(who) + ": max_chunk_frames is negative");
    if (cfg->device < 0) return fail(BP_ERR_ARG, std::string(who) + ": device ordinal is negative");
    for (int l = 1; l < cfg->numlayers; ++l)
        if (!weights[l] || !hbias[l]) return fail(BP_ERR_ARG, std::string(who) + ": null weights or hidden bias of a layer");
    {
        int ndev = 0;
        HIPCHK(hipGetDeviceCount(&ndev));
        if (cfg->device >= ndev) return fail(BP_ERR_ARG, std::string(who) + ": device ordinal out of range");
        HIPCHK(hipSetDevice(cfg->device));
    }
    bp_rbm *s = new (std::nothrow) bp_rbm();
    if (!s) return fail(BP_ERR_NOMEM, std::string(who) + ": out of host memory");
    s->cfg = *cfg;
    s->L = cfg->numlayers; s->B = cfg->bunchsize; s->Bp = rbm_pad(s->B);
    s->cap = cfg->max_chunk_frames ? cfg->max_chunk_frames : BP_MAXCACHEFRAME;
    s->Pmax = 0;
    for (int l = 0; l < s->L; ++l) { s->P[l] = rbm_pad(cfg->layersizes[l]); if (s->P[l] > s->Pmax) s->Pmax = s->P[l]; }
    for (int l = 1; l < s->L; ++l) { (void)bp_rbm_defaults(l, &s->hy[l]); s->applied[l] = 0; }

    Layout lay;
    size_t oW[BP_MAXLAYER], odW[BP_MAXLAYER], oc[BP_MAXLAYER], odc[BP_MAXLAYER], oa[BP_MAXLAYER], oda[BP_MAXLAYER];
    size_t gw_floats = 0;
    for (int l = 1; l < s->L; ++l) {
        const size_t wf = (size_t)s->P[l - 1] * s->P[l];
        if (wf > gw_floats) gw_floats = wf;
        oW[l] = lay.take(wf * 4); odW[l] = lay.take(wf * 4);
        oc[l] = lay.take((size_t)s->P[l] * 4); odc[l] = lay.take((size_t)s->P[l] * 4);
        oa[l] = lay.take((size_t)s->P[l - 1] * 4); oda[l] = lay.take((size_t)s->P[l - 1] * 4);
    }
    const size_t img = (size_t)s->Bp * s->Pmax * 4;
    const size_t oXs = lay.take(2 * img), oPs = lay.take(2 * img), oS0 = lay.take(img), oT0 = lay.take(img), oT1 = lay.take(img);
    const size_t oGW = lay.take(gw_floats * 4), ogc = lay.take((size_t)s->Pmax * 4), oga = lay.take((size_t)s->Pmax * 4);
    const size_t opart = lay.take((size_t)(s->Bp / RBM_TILE) * (s->Pmax / RBM_TILE) * 8), orecon = lay.take(8);
    const size_t zeroed = lay.size();
    const size_t ochunk = lay.take((size_t)s->cap * cfg->layersizes[0] * 4);

    hipError_t e = s->st.create(hipStreamNonBlocking);
    if (e != hipSuccess) { delete s; return dev_error(who, e); }
    e = s->dev.alloc(lay.size());
    if (e == hipSuccess) e = s->pin_out.alloc(256, true);
    if (e != hipSuccess) { (void)hipGetLastError(); delete s; return fail(BP_ERR_NOMEM, std::string(who) + ": " + hipGetErrorString(e)); }
    char *base = s->dev.as<char>();
    for (int l = 1; l < s->L; ++l) {
        s->W[l] = (float *)(base + oW[l]); s->dW[l] = (float *)(base + odW[l]); s->c[l] = (float *)(base + oc[l]);
        s->dc[l] = (float *)(base + odc[l]); s->a[l] = (float *)(base + oa[l]); s->da[l] = (float *)(base + oda[l]);
    }
    s->Xs = (float *)(base + oXs); s->Ps = (float *)(base + oPs); s->S0 = (float *)(base + oS0);
    s->T[0] = (float *)(base + oT0); s->T[1] = (float *)(base + oT1);
    s->GW = (float *)(base + oGW); s->gc = (float *)(base + ogc); s->ga = (float *)(base + oga);
    s->part = (double *)(base + opart); s->recon = (double *)(base + orecon); s->chunk = (float *)(base + ochunk);

    e = hipMemsetAsync(base, 0, zeroed, s->st);
    for (int l = 1; l < s->L && e == hipSuccess; ++l) {
        const int V = cfg->layersizes[l - 1], H = cfg->layersizes[l];
        e = copy2d(s->W[l], s->P[l], weights[l], H, H, V, hipMemcpyHostToDevice, s->st);
        if (e == hipSuccess) e = hipMemcpyAsync(s->c[l], hbias[l], (size_t)H * 4, hipMemcpyHostToDevice, s->st);
        if (e == hipSuccess && vbias && vbias[l]) e = hipMemcpyAsync(s->a[l], vbias[l], (size_t)V * 4, hipMemcpyHostToDevice, s->st);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s->st);
    if (e != hipSuccess) { delete s; return dev_error(who, e); }
    *out = s;
    return BP_OK;
}

extern "C" int bp_rbm_set_hyper(bp_rbm *s, int layer, const bp_rbm_hyper *p)
{
    { const int r = hyper_check("bp_rbm_set_hyper", p); if (r != BP_OK) return r; }
    { const int r = layer_check("bp_rbm_set_hyper", s, layer); if (r != BP_OK) return r; }
    s->hy[layer] = *p;
    return BP_OK;
}

extern "C" int bp_rbm_steps(bp_rbm *s, int layer, unsigned *applied)
{
    { const int r = layer_check("bp_rbm_steps", s, layer); if (r != BP_OK) return r; }
    if (!applied) return fail(BP_ERR_ARG, "bp_rbm_steps: null output");
    *applied = s->applied[layer];
    return BP_OK;
}

extern "C" int bp_rbm_train_chunk(bp_rbm *s, int layer, int n_frames, const float *in, double *recon_sq_sum)
{
    const char *who = "bp_rbm_train_chunk";
    { const int r = layer_check(who, s, layer); if (r != BP_OK) return r; }
    { const int r = frames_check(who, s, n_frames, in); if (r != BP_OK) return r; }
    const int nb = n_frames / s->B, s0 = s->cfg.layersizes[0];
    if (recon_sq_sum) *recon_sq_sum = 0.0;
    if (nb == 0) return BP_OK;                                  // (rows short of one bunch train nothing, as in BP_GPU::train)
    HIPCHK(hipSetDevice(s->cfg.device));
    hipError_t e = hipMemcpyAsync(s->chunk, in, (size_t)nb * s->B * s0 * 4, hipMemcpyHostToDevice, s->st);
    if (e == hipSuccess) e = hipMemsetAsync(s->recon, 0, 8, s->st);
    for (int b = 0; b < nb && e == hipSuccess; ++b) e = cd1_bunch(s, layer, s->chunk + (size_t)b * s->B * s0, false, true);
    if (e == hipSuccess) e = hipMemcpyAsync(s->pin_out.p, s->recon, 8, hipMemcpyDeviceToHost, s->st);
    if (e == hipSuccess) e = hipStreamSynchronize(s->st);
    if (e != hipSuccess) return dev_error(who, e);
    if (recon_sq_sum) *recon_sq_sum = *s->pin_out.as<double>();
    return BP_OK;
}

extern "C" int bp_rbm_up(bp_rbm *s, int layer, int n_frames, const float *in, float *out)
{
    const char *who = "bp_rbm_up";
    { const int r = layer_check(who, s, layer); if (r != BP_OK) return r; }
    { const int r = frames_check(who, s, n_frames, in); if (r != BP_OK) return r; }
    if (n_frames > 0 && !out) return fail(BP_ERR_ARG, std::string(who) + ": null output");
    if (n_frames == 0) return BP_OK;
    HIPCHK(hipSetDevice(s->cfg.device));
    const int s0 = s->cfg.layersizes[0], H = s->cfg.layersizes[layer];
    hipError_t e = hipMemcpyAsync(s->chunk, in, (size_t)n_frames * s0 * 4, hipMemcpyHostToDevice, s->st);
    for (int r0 = 0; r0 < n_frames && e == hipSuccess; r0 += s->B) {
        const int count = n_frames - r0 < s->B ? n_frames - r0 : s->B;
        float *res;
        e = propagate(s, s->chunk + (size_t)r0 * s0, count, layer, false, &res);
        if (e == hipSuccess) e = copy2d(out + (size_t)r0 * H, H, res, s->P[layer], H, count, hipMemcpyDeviceToHost, s->st);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s->st);
    return e == hipSuccess ? BP_OK : dev_error(who, e);
}

extern "C" int bp_rbm_step(bp_rbm *s, int layer, const float *in, int apply, const bp_rbm_trace *tr)
{
    const char *who = "bp_rbm_step";
    { const int r = layer_check(who, s, layer); if (r != BP_OK) return r; }
    if (!in) return fail(BP_ERR_ARG, std::string(who) + ": null input rows");
    if (apply != 0 && apply != 1) return fail(BP_ERR_ARG, std::string(who) + ": apply must be 0 or 1");
    if (s->B > s->cap) return fail(BP_ERR_ARG, std::string(who) + ": one bunch is over the stack's capacity (max_chunk_frames)");
    HIPCHK(hipSetDevice(s->cfg.device));
    const int V = s->cfg.layersizes[layer - 1], H = s->cfg.layersizes[layer], Vp = s->P[layer - 1], Hp = s->P[layer], B = s->B, Bp = s->Bp;
    const int s0 = s->cfg.layersizes[0];
    const bool store = tr && (tr->gw || tr->gc || tr->ga);
    const hipMemcpyKind D2H = hipMemcpyDeviceToHost;
    hipError_t e = hipMemcpyAsync(s->chunk, in, (size_t)B * s0 * 4, hipMemcpyHostToDevice, s->st);
    if (e == hipSuccess) e = hipMemsetAsync(s->recon, 0, 8, s->st);
    if (e == hipSuccess) e = cd1_bunch(s, layer, s->chunk, store, apply == 1);
    if (e == hipSuccess && tr) {
        // (the passes' images are not touched by the update: what comes back is what the bunch computed)
        if (tr->v0) e = copy2d(tr->v0, V, s->Xs, Vp, V, B, D2H, s->st);
        if (e == hipSuccess && tr->v1) e = copy2d(tr->v1, V, s->Xs + (size_t)Bp * Vp, Vp, V, B, D2H, s->st);
        if (e == hipSuccess && tr->p0) e = copy2d(tr->p0, H, s->Ps, Hp, H, B, D2H, s->st);
        if (e == hipSuccess && tr->p1) e = copy2d(tr->p1, H, s->Ps + (size_t)Bp * Hp, Hp, H, B, D2H, s->st);
        if (e == hipSuccess && tr->s0) e = copy2d(tr->s0, H, s->S0, Hp, H, B, D2H, s->st);
        if (e == hipSuccess && tr->gw) e = copy2d(tr->gw, H, s->GW, Hp, H, V, D2H, s->st);
        if (e == hipSuccess && tr->gc) e = hipMemcpyAsync(tr->gc, s->gc, (size_t)H * 4, D2H, s->st);
        if (e == hipSuccess && tr->ga) e = hipMemcpyAsync(tr->ga, s->ga, (size_t)V * 4, D2H, s->st);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(s->pin_out.p, s->recon, 8, D2H, s->st);
    if (e == hipSuccess) e = hipStreamSynchronize(s->st);
    if (e != hipSuccess) return dev_error(who, e);
    if (tr && tr->p0)
        for (size_t i = 0; i < (size_t)B * H; ++i) tr->p0[i] = -tr->p0[i];             // Ps holds -p0; the negation is exact
    if (tr && tr->recon) *tr->recon = *s->pin_out.as<double>();
    return BP_OK;
}

extern "C" int bp_rbm_get(bp_rbm *s, float *const *weights, float *const *hbias, float *const *vbias)
{
    const char *who = "bp_rbm_get";
    if (!s) return fail(BP_ERR_ARG, std::string(who) + ": null stack");
    HIPCHK(hipSetDevice(s->cfg.device));
    hipError_t e = hipSuccess;
    for (int l = 1; l < s->L && e == hipSuccess; ++l) {
        const int V = s->cfg.layersizes[l - 1], H = s->cfg.layersizes[l];
        if (weights && weights[l]) e = copy2d(weights[l], H, s->W[l], s->P[l], H, V, hipMemcpyDeviceToHost, s->st);
        if (e == hipSuccess && hbias && hbias[l]) e = hipMemcpyAsync(hbias[l], s->c[l], (size_t)H * 4, hipMemcpyDeviceToHost, s->st);
        if (e == hipSuccess && vbias && vbias[l]) e = hipMemcpyAsync(vbias[l], s->a[l], (size_t)V * 4, hipMemcpyDeviceToHost, s->st);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s->st);
    return e == hipSuccess ? BP_OK : dev_error(who, e);
}
