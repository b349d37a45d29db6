// bp_device.h -- device helpers shared by the kernel headers (bp_kernels.h, bp_bf16.h, bp_wgrad_dma*.h, bp_dp.h): the
// numeric rules that more than one kernel family applies (activations, dropout words, momentum update) and the split-K
// ticket, each written once.  No __global__ function: bp_step.hip and bp_dp.hip both include this header and are linked
// into one library.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>
#include <utility>

typedef float f32x16 __attribute__((ext_vector_type(16)));

template <int B, int E, class F>
__device__ __forceinline__ void static_for(F &&f)
{
    if constexpr (B < E) {
        f(std::integral_constant<int, B>{});
        static_for<B + 1, E>(std::forward<F>(f));
    }
}

// ------------------------------------------------------------------ Philox4x32-10
__device__ __forceinline__ void philox4x32_10(uint32_t &c0, uint32_t &c1, uint32_t &c2, uint32_t &c3,
                                              uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        // (two multiplies per product, v_mul_hi_u32 + v_mul_lo_u32, on purpose: written as (uint64_t)c * x it is ONE v_mad_u64_u32,
        // which is faster with many waves per SIMD but 10 % slower as the chain of dependent products that a GEMM epilogue's single
        // wave per SIMD runs -- tools/philox_mul_probe.hip, profiles/r16_gemm_tail.txt section 3)
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        const uint32_t n0 = h1 ^ c1 ^ k0, n2 = h0 ^ c3 ^ k1;
        c0 = n0; c1 = l1; c2 = n2; c3 = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

// Dropout words of the 4 consecutive bunch rows r0..r0+3 (r0 % 4 == 0) of unit n: word (gf & 3) of the Philox block
// keyed by (gf >> 2, unit) with gf = global frame index = row + frame_off.  frame_off % 4 == 0 (the usual case) needs
// one block; otherwise the four rows straddle two (frame_off is a launch constant, so the branch is uniform).
__device__ __forceinline__ void drop_words4(uint32_t (&w)[4], int r0, int n, int frame_off, uint32_t n_true, uint32_t layer,
                                            uint32_t step, uint32_t seed_lo, uint32_t seed_hi)
{
    const uint64_t g0 = (uint64_t)(uint32_t)(r0 + frame_off);
    const uint64_t idx = (g0 >> 2) * (uint64_t)n_true + (uint32_t)n;
    uint32_t a[4] = {(uint32_t)idx, (uint32_t)(idx >> 32), layer, step};
    philox4x32_10(a[0], a[1], a[2], a[3], seed_lo, seed_hi);
    const int sh = frame_off & 3;
    if (sh == 0) { w[0] = a[0]; w[1] = a[1]; w[2] = a[2]; w[3] = a[3]; return; }
    const uint64_t idx2 = idx + (uint64_t)n_true;
    uint32_t b[4] = {(uint32_t)idx2, (uint32_t)(idx2 >> 32), layer, step};
    philox4x32_10(b[0], b[1], b[2], b[3], seed_lo, seed_hi);
    if (sh == 1) { w[0] = a[1]; w[1] = a[2]; w[2] = a[3]; w[3] = b[0]; }
    else if (sh == 2) { w[0] = a[2]; w[1] = a[3]; w[2] = b[0]; w[3] = b[1]; }
    else { w[0] = a[3]; w[1] = b[0]; w[2] = b[1]; w[3] = b[2]; }
}

__device__ __forceinline__ float act_fwd(int act, float x)
{
    // DevFunc.cu:67-79 (ReLU, strict > 0) | DevFunc.cu:47-54 (.bak: 1/(1+expf(-x)))
    return act == 0 ? (x > 0.0f ? x : 0.0f) : 1.0f / (1.0f + expf(-x));
}
__device__ __forceinline__ float act_bwd(int act, float y)
{
    // DevFunc.cu:81-97 (y>0 ? 1 : 0) | :56-64 (.bak: (1-y)*y), from the post-dropout output y
    return act == 0 ? (y > 0.0f ? 1.0f : 0.0f) : (1.0f - y) * y;
}

// ------------------------------------------------------------------ momentum update (DevFunc.cu:313-318 + 270-277)
// kernUpdatedelta: the new momentum state of one parameter from its old state d, its summed gradient g and its weight w;
// c1 = (1-m)*lr or lr (host: update_coef in bp_handle.h), ndiv = (float)n, wc = 0 for biases.  Every caller then stores
// d' and applies kernAccSum itself, w' = d' + 1.0f*w, reading w again where the delta store may alias it.
//
// RCP: the quotient as ONE multiply by rdiv = exact_rdiv(ndiv) (bp_handle.h), for the divisors where that is the division to the
// bit; the IEEE division is 11 dependent VALU instructions per value (v_div_scale x 2, v_rcp, 6 fma, v_div_fmas, v_div_fixup), and
// a wave that keeps the matrix pipe busy has no VALU slot to spare.  The caller chooses ONCE per tile (per thread in
// the element-wise kernels) on the uniform rdiv != 0, around its whole update: chosen per value hipcc keeps every division and
// adds a branch each.  The product is a rounding step of its own -- the empty asm keeps it out of a contraction: left alone hipcc
// forms fma(g, rdiv, fl(wc * w)), which rounds wc * w first and is other bits than the division side's fma(wc, w, fl(g / ndiv)).
template <bool RCP = false>
__device__ __forceinline__ float update_delta(float mom, float c1, float wc, float ndiv, float rdiv, float d, float g, float w)
{
    if constexpr (RCP) {
        float q = g * rdiv;
        asm("" : "+v"(q));
        return mom * d - c1 * (q + wc * w);
    } else {
        return mom * d - c1 * (g / ndiv + wc * w);
    }
}

// ------------------------------------------------------------------ split-K ticket
// The n k-slices of one output tile run as n workgroups of ONE launch.  Each writes its partial tile, then calls this; the call
// returns true (in every thread) in the workgroup that arrived last, which then reads all n partials back and runs the epilogue.
// Nobody waits for anybody.  The ticket words only grow: n arrivals per tile and launch, n a power of two (2^32 is a multiple).
// lds_word: a free LDS word of the workgroup.
//
// The memory orders are all RELAXED (no release/acquire pair: under the HIP/LLVM memory model this is a race), so correctness
// rests on the gfx950 instruction sequence, which is:
//   partials  global_store_dword ... sc1   (__hip_atomic_store relaxed, agent scope: written through, the line leaves L2)
//             s_waitcnt vmcnt(0)           (in EVERY wave: each of its partial stores has been acknowledged)
//             s_barrier                    (every wave of the workgroup is past its wait)
//   ticket    global_atomic_add ... sc0    (one lane, relaxed, agent scope; returns the old value)
//             s_barrier                    (the old value goes to the other waves through lds_word)
//   readback  global_load_dword ... sc1    (__hip_atomic_load relaxed, agent scope: misses the CU's L1, served by L2 / memory)
// What that relies on (gfx950, observed; not an architectural guarantee): an sc1 store counts down vmcnt only once every CU's sc1
// load sees it, on any XCD; so once a workgroup has taken its ticket, all of its partials are visible to the sc1 loads of the
// workgroup that takes the last one (tests/test_gpu_parity.py runs the slices of a tile on different XCDs for 60 steps).  The
// partials must be stored and read with exactly these accesses (no plain store, no plain or flat load), and every wave's drain
// must stay in front of the first barrier.
__device__ __forceinline__ bool last_arrival(unsigned *ticket, unsigned *lds_word, unsigned n)
{
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) *lds_word = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    return (*lds_word & (n - 1)) == n - 1;
}
