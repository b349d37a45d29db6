// one_tile_driver.cc -- the host side of GemmKernel::run's one-tile-per-workgroup contract (csrc/bp_kernels.h: covers_tiles,
// multi_covers_tiles) on its own: no GPU, no library, nothing is launched.  The three launch sites of bp_step.hip return
// hipErrorInvalidConfiguration where these say no; here they are asked about launches that cover their tile lists and about ones whose
// stride is shorter.  Built by tests/test_gemm_tail_gpu.py with hipcc (the header needs the HIP headers to parse).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bp_kernels.h"

#define CHECK(c) do { if (!(c)) { printf("one_tile_driver: line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

// the tile list as bp_step.hip packs it: every problem starts on a multiple of 8 entries
static int pack(MultiArgs &a, const int (*tiles)[2], int n)
{
    int t = 0;
    memset(&a, 0, sizeof(a));
    for (int i = 0; i < n; ++i) {
        a.g[i].tiles_m = tiles[i][0]; a.g[i].tiles_n = tiles[i][1];
        a.first_tile[i] = t; t += (tiles[i][0] * tiles[i][1] + 7) & ~7;
    }
    a.first_tile[n] = t; a.n = n;
    return t;
}

int main()
{
    GemmArgs g; memset(&g, 0, sizeof(g));
    long checked = 0;
    // bp_gemm: the grid is the stride
    for (int tm = 1; tm <= 9; ++tm)
        for (int tn = 1; tn <= 33; tn += 4) {
            g.tiles_m = tm; g.tiles_n = tn;
            CHECK(covers_tiles(tm * tn, g));
            CHECK(covers_tiles(tm * tn + 5, g));
            CHECK(!covers_tiles(tm * tn - 1, g));
            CHECK(!covers_tiles(tm * tn / 2, g));             // (a walk of stride tiles / 2 would take two trips)
            // split output launch: OUT_SPLITS slices of every tile
            CHECK(covers_tiles(tm * tn * OUT_SPLITS, g, OUT_SPLITS));
            CHECK(!covers_tiles(tm * tn * OUT_SPLITS - 1, g, OUT_SPLITS));
            CHECK(!covers_tiles(tm * tn, g, OUT_SPLITS));
            checked += 7;
        }
    g.tiles_m = 8; g.tiles_n = 32;
    CHECK(!covers_tiles(0, g) && !covers_tiles(-1, g) && !covers_tiles(255, g) && covers_tiles(256, g));
    g.tiles_m = 1 << 16; g.tiles_n = 1 << 16;                 // the product does not wrap
    CHECK(!covers_tiles(0, g) && !covers_tiles(1 << 30, g));
    g.tiles_m = -1; g.tiles_n = 4;
    CHECK(!covers_tiles(100, g));

    // grouped launch: each problem's share of the list
    MultiArgs a;
    const int one[1][2] = {{8, 16}}, four[4][2] = {{3, 3}, {8, 16}, {1, 1}, {2, 37}};
    CHECK(pack(a, one, 1) == 128 && multi_covers_tiles(a));
    a.first_tile[1] = 127;                                    // one entry short
    CHECK(!multi_covers_tiles(a));
    CHECK(pack(a, four, 4) == 16 + 128 + 8 + 80 && multi_covers_tiles(a));
    for (int p = 0; p < 4; ++p) {                             // any one problem short, the others whole
        pack(a, four, 4);
        a.g[p].tiles_n += (a.first_tile[p + 1] - a.first_tile[p]) / a.g[p].tiles_m;      // (now more tiles than entries)
        CHECK(!multi_covers_tiles(a));
        ++checked;
    }
    pack(a, four, 4);
    a.n = 0; CHECK(!multi_covers_tiles(a));
    a.n = 5; CHECK(!multi_covers_tiles(a));
    printf("one_tile_driver: %ld launches asked, all answered as the contract says\n", checked);
    return 0;
}
