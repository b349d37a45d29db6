// bp_infer.hip -- the row-invariant inference forward (BP_FORWARD_ROWINV, include/bp_c_api.h).  gfx950 only.
//
// One launch per layer, Y[M][N] = act(alpha * X[M][K] . W[K][N] + b), fp32, for M from 1 to the bunch.  At the handful of rows a
// stream push has, the layer is a stream of W: every weight is read ONCE per tile of 32 rows, with 16-byte loads straight into
// registers, three units of 8 loads per wave in flight; X is read in 32-byte pieces per lane and stays in L1 / L2.
//
// Decomposition (infer_plan, bp_infer.h: a function of K and N alone):
//   workgroup  one tile of 32 rows x 128 columns, one of `splitk` k-slices; 4 waves, wave w holds partial sum p = 4 * slice + w
//   wave       units [p * per, (p + 1) * per) of 16 k-rows.  In a unit, lane (c = lane & 31, h = lane >> 5) loads X[row c][k0 .. k0 + 8)
//              and W[k0 + i][n0 + 4c .. n0 + 4c + 4) for i < 8, k0 = 16 u + 8 h, and step i runs four v_mfma_f32_32x32x2_f32:
//              block j (columns n0 + 4c + j) += X[.][16u + i] * W[16u + i][.] + X[.][16u + 8 + i] * W[16u + 8 + i][.]
//   workgroup  the four waves' partial sums are added through LDS as ((p0 + p1) + p2) + p3 -- wave o finishes rows 8o .. 8o + 8
//   splitk > 1 the sum goes to the slice's slab (write-through stores), the workgroup takes a ticket (last_arrival, bp_device.h),
//              and the LAST one reads every slice's slab back -- its own included -- and adds them in slice order 0, 1, ...
//   epilogue   act_fwd / the output arithmetic of the step's forward kernels (bp_kernels.h), float4 stores
//
// What the row invariance rests on: an output element's value is a chain of additions whose order is fixed by (K, N) alone.  Rows
// of a tile never meet: the MFMA's row i reads only A's row i, the LDS exchange and the slabs are per element, and a row past
// M computes on a copy of row M - 1 and is never stored.  Which slice arrives last decides who adds, not in which order.
// No float atomics.
#include "bp_infer.h"

#include "bp_device.h"

namespace {
constexpr int DEPTH = 3;                   // units of W in flight per wave
struct Unit { float4 w[8]; float4 x[2]; };

__device__ __forceinline__ void unit_load(Unit &q, const float *xrow, const float *wcol, int ldw, int u, int h)
{
    const int k0 = INFER_KU * u + 8 * h;
    q.x[0] = *reinterpret_cast<const float4 *>(xrow + k0);
    q.x[1] = *reinterpret_cast<const float4 *>(xrow + k0 + 4);
#pragma unroll
    for (int i = 0; i < 8; ++i) q.w[i] = *reinterpret_cast<const float4 *>(wcol + (size_t)(k0 + i) * ldw);
}

__device__ __forceinline__ void unit_mfma(const Unit &q, f32x16 (&acc)[4])
{
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float4 xv = q.x[i >> 2];
        const float a = (i & 3) == 0 ? xv.x : (i & 3) == 1 ? xv.y : (i & 3) == 2 ? xv.z : xv.w;
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, q.w[i].x, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, q.w[i].y, acc[1], 0, 0, 0);
        acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, q.w[i].z, acc[2], 0, 0, 0);
        acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, q.w[i].w, acc[3], 0, 0, 0);
    }
}

typedef unsigned long long u64;
__device__ __forceinline__ u64 pack2(float a, float b) { return (u64)__float_as_uint(a) | ((u64)__float_as_uint(b) << 32); }
}  // namespace

template <bool SPLIT>
__global__ __launch_bounds__(256) void bp_infer_layer(const InferArgs a)
{
    // red[o][w][j][rr][lane]: what wave w hands to wave o (registers 4o .. 4o + 4 of its four blocks)
    __shared__ float red[4 * 4 * 4 * 4 * 64];
    const int lane = threadIdx.x & 63, c = lane & 31, h = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int slice = SPLIT ? (int)blockIdx.x % a.splitk : 0, tn = SPLIT ? (int)blockIdx.x / a.splitk : (int)blockIdx.x;
    const int mb = (int)blockIdx.y * INFER_BM, n0 = tn * INFER_BN + 4 * c;
    const bool col_ok = n0 < a.N;                          // (N % 4 == 0: the lane's four columns are in or out together)
    const int mrow = mb + c < a.M ? mb + c : a.M - 1;
    const float *xrow = a.X + (size_t)mrow * a.ldx;
    const float *wcol = a.W + (col_ok ? n0 : 0);
    const int U = a.K / INFER_KU, p = 4 * slice + w;
    const int u0 = p * a.per < U ? p * a.per : U, u1 = u0 + a.per < U ? u0 + a.per : U;

    f32x16 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.0f;
    Unit q[DEPTH];
    static_for<0, DEPTH>([&](auto d) { if (u0 + d < u1) unit_load(q[d], xrow, wcol, a.ldw, u0 + d, h); });
    for (int u = u0; u < u1; u += DEPTH)
        static_for<0, DEPTH>([&](auto d) {
            if (u + d < u1) {
                unit_mfma(q[d], acc);
                if (u + d + DEPTH < u1) unit_load(q[d], xrow, wcol, a.ldw, u + d + DEPTH, h);
            }
        });

    // ---- the four partial sums of the workgroup, in wave order; wave o keeps registers [4o, 4o + 4): rows 8o + 4h + rr
#pragma unroll
    for (int o = 0; o < 4; ++o)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) red[(((o * 4 + w) * 4 + j) * 4 + rr) * 64 + lane] = acc[j][4 * o + rr];
    __syncthreads();
    float s[4][4];                                          // [rr][j]
#pragma unroll
    for (int rr = 0; rr < 4; ++rr)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float t = red[(((w * 4 + 0) * 4 + j) * 4 + rr) * 64 + lane];
#pragma unroll
            for (int v = 1; v < 4; ++v) t += red[(((w * 4 + v) * 4 + j) * 4 + rr) * 64 + lane];
            s[rr][j] = t;
        }
    const int m0 = mb + 8 * w + 4 * h;                      // the lane's rows m0 + rr, columns n0 + j

    if constexpr (SPLIT) {
        // ---- k-slices: partial tile to the slab, ticket, the last arriver adds all slices in slice order
        float *mine = a.slab + (size_t)slice * a.slab_stride;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr)
            if (col_ok && m0 + rr < a.M) {
                u64 *dst = reinterpret_cast<u64 *>(mine + (size_t)(m0 + rr) * a.N + n0);
                __hip_atomic_store(dst, pack2(s[rr][0], s[rr][1]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(dst + 1, pack2(s[rr][2], s[rr][3]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        // (the ticket's LDS word: red[0], free once every wave is past last_arrival's first barrier)
        if (!last_arrival(a.ticket + (size_t)blockIdx.y * a.tiles_n + tn, reinterpret_cast<unsigned *>(red), (unsigned)a.splitk)) return;
        u64 part[INFER_MAX_SPLITK][4][2];
#pragma unroll
        for (int z = 0; z < INFER_MAX_SPLITK; ++z)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const bool on = z < a.splitk && col_ok && m0 + rr < a.M;
                const u64 *src = reinterpret_cast<const u64 *>(a.slab + (size_t)z * a.slab_stride + (size_t)(m0 + rr) * a.N + n0);
                part[z][rr][0] = on ? __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
                part[z][rr][1] = on ? __hip_atomic_load(src + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
            }
#pragma unroll
        for (int rr = 0; rr < 4; ++rr)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float t = 0.0f;
#pragma unroll
                for (int z = 0; z < INFER_MAX_SPLITK; ++z) {
                    const u64 v = part[z][rr][j >> 1];
                    const float f = __uint_as_float((unsigned)((j & 1) ? v >> 32 : v));
                    if (z == 0) t = f; else if (z < a.splitk) t += f;
                }
                s[rr][j] = t;
            }
    }

    // ---- epilogue: the arithmetic of EPI_FWD_HIDDEN / EPI_FWD_OUT / EPI_FWD_OUT_LOGI (bp_kernels.h); pad columns are stored as 0
    if (!col_ok) return;
    float bn[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) bn[j] = a.bias[n0 + j];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        float y[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool live = n0 + j < a.n_true;
            if (!a.out) {
                const float v = act_fwd(a.act, a.alpha * s[rr][j] + bn[j]);
                y[j] = live ? v : 0.0f;
            } else {
                const float z = live ? a.alpha * s[rr][j] + bn[j] : 0.0f;
                y[j] = (a.logi && live && n0 + j >= a.lin_cols) ? 1.0f / (1.0f + expf(-z)) : z;
            }
        }
        if (m0 + rr < a.M) *reinterpret_cast<float4 *>(a.Y + (size_t)(m0 + rr) * a.ldy + n0) = make_float4(y[0], y[1], y[2], y[3]);
    }
}

hipError_t infer_layer_launch(InferArgs a, hipStream_t st)
{
    const dim3 grid((unsigned)(a.tiles_n * a.splitk), (unsigned)((a.M + INFER_BM - 1) / INFER_BM));
    if (a.splitk > 1) hipLaunchKernelGGL(bp_infer_layer<true>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(bp_infer_layer<false>, grid, dim3(256), 0, st, a);
    return hipGetLastError();
}
