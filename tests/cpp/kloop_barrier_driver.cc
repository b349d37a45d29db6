// kloop_barrier_driver.cc -- where the k-tile barrier of the fp32 GEMM stands among the tile's LDS traffic, on the host: no GPU, nothing
// is launched.  GemmCfg::step (csrc/bp_kernels.h) places its fragment reads, its ds_writes of the next tile, its global loads and the
// tile's barrier by the constexpr functions and constants NK, RD, LAST_READ, BAR, store_slot and load_slot.  From them this driver
// writes out, for every tile configuration the library instantiates and nt = 1 .. 9 k-tiles, what one wave does to the two LDS
// stages in program order -- the head of GemmKernel::run, one step per tile, the barrier behind MFMA BAR of every step but the last,
// the hand-over reads behind it -- and counts the barriers in front of every access (its epoch; every wave passes every barrier, so
// accesses of two waves in different epochs are ordered).  The two stages suffice when every ds_write of tile T has epoch T and
// every read of tile T epoch T + 1: the stage is then written (tile T), read (tile T), and written again (tile T + 2) in three
// different epochs by whichever waves.  Beside that: the slots are in range and in order, the barrier's wait has no young read to
// wait for (BAR > LAST_READ), the forwards have it in front of the last MFMA and every other configuration behind it, and the
// (row, chain) pairs a tile multiplies are those of the plain loop (the order itself: kloop_order_driver.cc).
// Built by tests/test_kloop_barrier_host.py with hipcc (the header needs the HIP headers to parse).
#include <stdio.h>
#include <stdlib.h>

#include <set>
#include <utility>
#include <vector>

#include "bp_kernels.h"

#define CHECK(c) do { if (!(c)) { printf("kloop_barrier_driver: %s: line %d: %s\n", g_what, __LINE__, #c); exit(1); } } while (0)
static const char *g_what = "";

struct Access {
    bool write;
    int tile, epoch;
};

// one wave, nt k-tiles: GemmKernel::run's head, then one GemmCfg::step per tile (the last one stages nothing and has no barrier)
template <class Cfg>
static std::vector<Access> wave_program(int nt)
{
    std::vector<Access> v;
    int epoch = 0;
    v.push_back({true, 0, epoch});                                        // Cfg::store(r0, stage 0)
    ++epoch;                                                              // __syncthreads()
    for (int s = 0; s < Cfg::RD; ++s) v.push_back({false, 0, epoch});     // Cfg::read_first
    for (int t = 0; t < nt; ++t) {
        const bool stage_next = t + 1 < nt;
        for (int s = 0; s < Cfg::NK; ++s) {                               // behind MFMA s:
            if (s + Cfg::RD < Cfg::NK) v.push_back({false, t, epoch});    //   the fragments of step s + RD
            if (stage_next) {
                for (int q = 0; q < Cfg::NP; ++q)
                    if (Cfg::store_slot(q) == s) v.push_back({true, t + 1, epoch});
                if (s == Cfg::BAR) {
                    ++epoch;                                              //   the k-tile's barrier
                    for (int r = 0; r < Cfg::RD; ++r) v.push_back({false, t + 1, epoch});
                }
            }
        }
    }
    return v;
}

template <class Cfg>
static long check(int BK, bool forward, const char *what)
{
    g_what = what;
    constexpr int NK = Cfg::NK, RD = Cfg::RD, BAR = Cfg::BAR, NP = Cfg::NP;
    CHECK(NK * 2 * Cfg::KS == BK && RD >= 1 && RD <= NK && Cfg::LAST_READ == NK - RD - 1);
    CHECK(BAR > Cfg::LAST_READ && BAR <= NK - 1);
    if (forward && NK > RD + 2) CHECK(BAR < NK - 1 && Cfg::EARLY_BAR);
    else CHECK(BAR == NK - 1);
    for (int q = 0; q < NP; ++q) {
        CHECK(Cfg::store_slot(q) >= 0 && Cfg::store_slot(q) <= BAR && Cfg::load_slot(q) >= 0 && Cfg::load_slot(q) < NK);
        if (q) CHECK(Cfg::store_slot(q) >= Cfg::store_slot(q - 1) && Cfg::load_slot(q) >= Cfg::load_slot(q - 1));
    }
    // every step's fragments are read once: handed over (s < RD) or issued behind MFMA s - RD <= LAST_READ < BAR
    for (int s = RD; s < NK; ++s) CHECK(s - RD <= Cfg::LAST_READ && s - RD < BAR);
    // the (row, chain) pairs of a tile: two rows per step from the wave group's first row on, chains in turn
    for (int ks = 0; ks < Cfg::KS; ++ks) {
        std::set<std::pair<int, int> > a, b;
        for (int s = 0; s < NK; ++s) {
            a.insert({Cfg::step_row(ks, s), Cfg::step_chain(s)});
            b.insert({ks * (BK / Cfg::KS) + 2 * s, s % Cfg::NCH});
        }
        CHECK(a == b && (int)a.size() == NK);
    }
    long n = 0;
    for (int nt = 1; nt <= 9; ++nt) {
        const std::vector<Access> v = wave_program<Cfg>(nt);
        std::vector<int> writes(nt, 0), reads(nt, 0);
        for (const Access &x : v) {
            CHECK(x.tile >= 0 && x.tile < nt);
            if (x.write) { CHECK(x.epoch == x.tile); ++writes[x.tile]; }
            else { CHECK(x.epoch == x.tile + 1); ++reads[x.tile]; }
        }
        for (int t = 0; t < nt; ++t) CHECK(writes[t] == (t ? NP : 1) && reads[t] == NK);
        n += (long)v.size();
    }
    return n;
}

int main()
{
    long n = 0;
    n += check<GemmCfg<32, 64, 64, 1, 2, true, false, EPI_FWD_HIDDEN> >(64, true, "wide forward");
    n += check<GemmCfg<32, 64, 64, 1, 2, true, false, EPI_FWD_OUT> >(64, true, "wide output forward");
    n += check<GemmCfg<32, 64, 64, 1, 2, true, false, EPI_FWD_OUT_LOGI> >(64, true, "wide logistic output forward");
    n += check<GemmCfg<32, 32, 64, 1, 1, true, false, EPI_FWD_HIDDEN> >(64, true, "narrow forward");
    n += check<GemmCfg<32, 32, 64, 1, 1, true, false, EPI_FWD_OUT> >(64, true, "narrow output forward");
    n += check<GemmCfg<32, 32, 64, 1, 1, true, false, EPI_FWD_OUT_LOGI> >(64, true, "narrow logistic output forward");
    n += check<GemmCfg<32, 32, 64, 1, 1, true, false, EPI_OUT_SPLIT> >(64, true, "split output forward");
    n += check<GemmCfg<32, 32, 64, 1, 1, true, false, EPI_OUT_SPLIT_LOGI> >(64, true, "split logistic output forward");
    n += check<GemmCfg<32, 64, 128, 1, 2, true, true, EPI_DGRAD> >(128, false, "128-deep dgrad");
    n += check<GemmCfg<32, 64, 64, 1, 2, true, true, EPI_DGRAD> >(64, false, "64-deep dgrad");
    n += check<GemmCfg<32, 32, 64, 1, 1, true, true, EPI_DGRAD> >(64, false, "narrow dgrad");
    n += check<GemmCfg<64, 64, 32, 2, 2, false, false, EPI_WGRAD_UPDATE> >(32, false, "weight gradient, update");
    n += check<GemmCfg<128, 64, 16, 2, 2, false, false, EPI_WGRAD_STORE> >(16, false, "weight gradient, store");
    printf("kloop_barrier_driver: %ld LDS accesses, every one in the epoch of its tile\n", n);
    return 0;
}
