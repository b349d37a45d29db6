// bp_philox_host.h -- Philox4x32-10 on the host, the same function as philox4x32_10 of bp_device.h: the counter-based draws of the
// host-side planners (bp_mix_plan and bp_mix_shuffle in bp_mix.hip, bp_mix_reverb_pairs and bp_rir_rooms in bp_room.hip).  Host
// only; internal: nothing in here is part of the C ABI.
#pragma once
#include <stdint.h>

inline void philox(uint32_t c[4], uint64_t seed)
{
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        c[0] = n0; c[1] = (uint32_t)p1; c[2] = n2; c[3] = (uint32_t)p0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}
inline uint32_t word0(uint64_t seed, uint32_t c0, uint32_t c1, uint32_t c2)
{
    uint32_t c[4] = {c0, c1, c2, 0};
    philox(c, seed);
    return c[0];
}
inline uint64_t scale(uint32_t u, uint64_t n) { return ((uint64_t)u * n) >> 32; }
