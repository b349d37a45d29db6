// tools/philox_mul_probe.hip -- development probe: the 32x32 -> 64-bit product of a Philox round as __umulhi(c, x) plus c * x
// (v_mul_hi_u32 + v_mul_lo_u32) against (uint64_t)c * x (one v_mad_u64_u32), as a chain of dependent products per lane, the way a
// GEMM epilogue's draw runs them: one wave per SIMD (256 workgroups of 256 threads) and, for the throughput side, eight.
// usage: philox_mul_probe [rounds]        (default 4096 Philox rounds per lane = 8192 dependent-pair products)
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); exit(1);} } while (0)

template <bool WIDE>
__device__ __forceinline__ void round1(uint32_t &c0, uint32_t &c1, uint32_t &c2, uint32_t &c3, uint32_t &k0, uint32_t &k1)
{
    uint32_t h0, l0, h1, l1;
    if constexpr (WIDE) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        h0 = (uint32_t)(p0 >> 32); l0 = (uint32_t)p0; h1 = (uint32_t)(p1 >> 32); l1 = (uint32_t)p1;
    } else {
        h0 = __umulhi(0xD2511F53u, c0); l0 = 0xD2511F53u * c0; h1 = __umulhi(0xCD9E8D57u, c2); l1 = 0xCD9E8D57u * c2;
    }
    const uint32_t n0 = h1 ^ c1 ^ k0, n2 = h0 ^ c3 ^ k1;
    c0 = n0; c1 = l1; c2 = n2; c3 = l0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
}
template <bool WIDE>
__global__ __launch_bounds__(256) void chain(uint32_t *out, int rounds, uint32_t seed)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t c0 = (uint32_t)i, c1 = seed, c2 = 3u, c3 = 7u, k0 = seed, k1 = ~seed;
#pragma unroll 10
    for (int r = 0; r < rounds; ++r) round1<WIDE>(c0, c1, c2, c3, k0, k1);
    out[i] = c0 ^ c1 ^ c2 ^ c3;
}

template <bool WIDE>
static double run(uint32_t *out, int blocks, int rounds, uint32_t *host)
{
    hipEvent_t a, b; CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
    float best = 1e30f;
    for (int rep = 0; rep < 6; ++rep) {
        CK(hipEventRecord(a));
        hipLaunchKernelGGL(chain<WIDE>, dim3(blocks), dim3(256), 0, 0, out, rounds, 0x9E3779B9u);
        CK(hipEventRecord(b)); CK(hipEventSynchronize(b));
        float ms; CK(hipEventElapsedTime(&ms, a, b));
        if (rep && ms < best) best = ms;
    }
    CK(hipMemcpy(host, out, 256 * 4, hipMemcpyDeviceToHost));
    return best * 1e3;   // us
}
int main(int argc, char **argv)
{
    const int rounds = argc > 1 ? atoi(argv[1]) : 4096;
    uint32_t *out; CK(hipMalloc(&out, (size_t)2048 * 256 * 4));
    uint32_t h0[256], h1[256];
    for (int blocks : {256, 2048}) {
        const double pair = run<false>(out, blocks, rounds, h0), wide = run<true>(out, blocks, rounds, h1);
        int diff = 0;
        for (int i = 0; i < 256; ++i) diff += h0[i] != h1[i];
        printf("%4d workgroups (%d wave(s) per SIMD), %d rounds per lane: mul_hi+mul_lo %.1f us = %.2f ns per round | mad_u64_u32 %.1f us = %.2f ns per round | words differ: %d\n",
               blocks, blocks / 256, rounds, pair, pair * 1e3 / rounds, wide, wide * 1e3 / rounds, diff);
    }
    return 0;
}
