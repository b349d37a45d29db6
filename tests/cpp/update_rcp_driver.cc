// update_rcp_driver.cc -- the reciprocal the momentum update may multiply by, on the host: no GPU, nothing is launched.
// exact_rdiv (csrc/bp_handle.h, next to update_coef) returns 1/ndiv where g * (1/ndiv) is g / ndiv to the bit for every float g --
// ndiv a power of two whose reciprocal is a normal float -- and 0, "keep the division", for every other divisor.  This driver prints
// one line per divisor of its table, `ndiv <bits of ndiv> rdiv <bits of rdiv>`, and checks the rule itself: a power of two gives the
// float 1/ndiv exactly and multiplies as it divides on a set of edge words; everything else gives 0.  tests/test_update_rcp_host.py
// reads the lines and runs the large random check with numpy.  Built by that test with hipcc (the header needs the HIP headers to
// parse).
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <iterator>
#include <vector>

#include "bp_handle.h"

#define CHECK(c) do { if (!(c)) { printf("update_rcp_driver: line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

int main()
{
    std::vector<float> pow2, other;
    for (int k = 0; k <= 24; ++k) pow2.push_back(ldexpf(1.0f, k));
    for (float v : {3.0f, 96.0f, 100.0f, 384.0f, 768.0f, 16777218.0f /* 2^24 + 2 */, 0.0f, -256.0f, -3.0f}) other.push_back(v);
    // what a bunch size never is, but the helper must still answer: powers of two below 1 and at the ends of the exponent range,
    // infinities, NaN, a subnormal
    const float far_pow2[] = {0.5f, ldexpf(1.0f, -24), ldexpf(1.0f, 126), ldexpf(1.0f, -126), ldexpf(1.0f, -127) /* a subnormal: 1/ndiv = 2^127 */};
    const float far_other[] = {ldexpf(1.0f, 127) /* 1/ndiv is subnormal */, ldexpf(1.0f, -128), ldexpf(1.0f, -149) /* 1/ndiv is infinite */,
                               INFINITY, -INFINITY, NAN, 1.5f};
    // edge words for the product: zeros, the smallest and largest subnormals and normals, odd mantissas that a shift into the
    // subnormal range must round (to even), infinities
    const uint32_t edge[] = {0x00000000u, 0x80000000u, 0x00000001u, 0x80000001u, 0x00000003u, 0x007FFFFFu, 0x00800000u, 0x00800001u,
                             0x00800003u, 0x00FFFFFFu, 0x01000001u, 0x0B800001u, 0x0B800003u, 0x0C7FFFFFu, 0x3F800000u, 0x3FFFFFFFu,
                             0x7F7FFFFFu, 0xFF7FFFFFu, 0x7F800000u, 0xFF800000u};
    long products = 0;
    for (int far = 0; far < 2; ++far) {
        std::vector<float> p = far ? std::vector<float>(std::begin(far_pow2), std::end(far_pow2)) : pow2;
        for (float n : p) {
            const float r = exact_rdiv(n);
            CHECK(r != 0.0f && r == 1.0f / n && isnormal(r));
            CHECK(bits(r) == bits(1.0f / n) && (double)r * (double)n == 1.0);
            for (uint32_t w : edge) {
                volatile float g = from_bits(w);
                volatile float a = g * r, b = g / n;
                CHECK(bits(a) == bits(b));
                ++products;
            }
            if (!far) printf("ndiv %08x rdiv %08x\n", bits(n), bits(r));
        }
        std::vector<float> o = far ? std::vector<float>(std::begin(far_other), std::end(far_other)) : other;
        for (float n : o) {
            const float r = exact_rdiv(n);
            CHECK(bits(r) == 0u);
            if (!far) printf("ndiv %08x rdiv %08x\n", bits(n), bits(r));
        }
    }
    printf("update_rcp_driver: %zu powers of two multiply as they divide (%ld edge products), %zu other divisors keep the division\n",
           pow2.size() + std::size(far_pow2), products, other.size() + std::size(far_other));
    return 0;
}
