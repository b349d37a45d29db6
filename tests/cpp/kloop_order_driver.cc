// kloop_order_driver.cc -- the order in which a workgroup of the fp32 GEMM multiplies its k, on the host: no GPU, nothing is launched.
// GemmCfg::step (csrc/bp_kernels.h) addresses LDS and its accumulator chains through the constexpr index functions step_row and
// step_chain (NK steps per k-tile and wave).  Here the same functions enumerate, for nt = 1 .. 9 k-tiles and every wave group of
// every tile configuration the step dispatches, the (wave group, chain, k) triples in the order the MFMAs are issued; they must be,
// element for element, those of the plain loop written out below without them: wave group ks takes rows [ks * BK / KS,
// (ks + 1) * BK / KS) of every BK-deep tile, two rows per MFMA, step s of a tile into chain s % NCH.  Whatever reschedules the
// k-loop (more than one tile between two barriers, a split first tile) has to keep this sequence, and is to be enumerated here
// next to it; the two-tiles-per-barrier forward that was measured and not kept (profiles/r17_kloop_pairs.txt) is not in the tree.
// Built by tests/test_kloop_order.py with hipcc (the header needs the HIP headers to parse).
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "bp_kernels.h"

#define CHECK(c) do { if (!(c)) { printf("kloop_order_driver: line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

struct Triple {
    int ks, chain, k;
    bool operator==(const Triple &o) const { return ks == o.ks && chain == o.chain && k == o.k; }
};

// the reference: one k-tile after the other
static std::vector<Triple> plain_order(int nt, int ks, int BK, int KS, int NCH)
{
    std::vector<Triple> v;
    const int per = BK / KS;
    for (int t = 0; t < nt; ++t)
        for (int s = 0; s < per / 2; ++s)
            for (int kh = 0; kh < 2; ++kh) v.push_back({ks, s % NCH, t * BK + ks * per + 2 * s + kh});
    return v;
}

// GemmKernel::run: one GemmCfg::step per k-tile, in order (head, loop and tail steps differ in what they stage, not in what they multiply)
template <class Cfg>
static std::vector<Triple> kernel_order(int nt, int ks, int BK)
{
    std::vector<Triple> v;
    for (int t = 0; t < nt; ++t)
        for (int s = 0; s < Cfg::NK; ++s)
            for (int kh = 0; kh < 2; ++kh) v.push_back({ks, Cfg::step_chain(s), t * BK + Cfg::step_row(ks, s) + kh});
    return v;
}

template <class Cfg>
static long same_order(int BK, const char *what)
{
    long n = 0;
    CHECK(Cfg::NK * 2 * Cfg::KS == BK && Cfg::NK % Cfg::NCH == 0);        // chain parity continues from tile to tile
    for (int nt = 1; nt <= 9; ++nt)
        for (int ks = 0; ks < Cfg::KS; ++ks) {
            const std::vector<Triple> a = plain_order(nt, ks, BK, Cfg::KS, Cfg::NCH), b = kernel_order<Cfg>(nt, ks, BK);
            CHECK(a.size() == b.size() && a.size() == (size_t)nt * BK / Cfg::KS);
            for (size_t i = 0; i < a.size(); ++i)
                if (!(a[i] == b[i])) {
                    printf("kloop_order_driver: %s, nt %d, wave group %d, element %zu: (%d, %d, %d) for (%d, %d, %d)\n", what, nt, ks, i,
                           b[i].ks, b[i].chain, b[i].k, a[i].ks, a[i].chain, a[i].k);
                    exit(1);
                }
            n += (long)a.size();
        }
    return n;
}

int main()
{
    long n = 0;
    n += same_order<GemmCfg<32, 64, 64, 1, 2, true, false, EPI_FWD_HIDDEN> >(64, "wide forward");
    n += same_order<GemmCfg<32, 64, 64, 1, 2, true, false, EPI_FWD_OUT> >(64, "wide output forward");
    n += same_order<GemmCfg<32, 32, 64, 1, 1, true, false, EPI_FWD_HIDDEN> >(64, "narrow forward");
    n += same_order<GemmCfg<32, 32, 64, 1, 1, true, false, EPI_OUT_SPLIT> >(64, "split output forward");
    n += same_order<GemmCfg<32, 64, 128, 1, 2, true, true, EPI_DGRAD> >(128, "128-deep dgrad");
    n += same_order<GemmCfg<32, 64, 64, 1, 2, true, true, EPI_DGRAD> >(64, "64-deep dgrad");
    n += same_order<GemmCfg<32, 32, 64, 1, 1, true, true, EPI_DGRAD> >(64, "narrow dgrad");
    n += same_order<GemmCfg<64, 64, 32, 2, 2, false, false, EPI_WGRAD_UPDATE> >(32, "weight gradient, update");
    n += same_order<GemmCfg<128, 64, 16, 2, 2, false, false, EPI_WGRAD_STORE> >(16, "weight gradient, store");
    printf("kloop_order_driver: %ld triples in the order of the plain loop\n", n);
    return 0;
}
