// bp_rbm.h -- what bp_rbm.hip's host code and its kernels agree on: the padded device layout of a stack of restricted Boltzmann
// machines and the argument records of its launches.  Internal: nothing in here is part of the C ABI (include/bp_c_api.h: the
// bp_rbm_* block has the definition of one CD-1 step).
//
// Device layout (fp32): every width s_l is padded to P_l = roundup(s_l, 64) and the bunch B to Bp = roundup(B, 64); pad rows and
// pad columns hold zeros and stay zero (the epilogues store zeros there, the update skips them), so the k-loops of the GEMMs load
// whole tiles without predicates and stay inside the block.
//   W_l, dW_l  [P_{l-1}][P_l]   the reference's [prev][cur] layout, rows padded
//   c_l, dc_l  [P_l]            hidden bias (the net's bias of layer l) and its momentum state
//   a_l, da_l  [P_{l-1}]        visible bias and its momentum state
//   Xs         [2 Bp][Vp]       rows [0, Bp): v0, rows [Bp, 2 Bp): v1               (the statistics GEMM's A, read as [m = v][k = row])
//   Ps         [2 Bp][Hp]       rows [0, Bp): -p0, rows [Bp, 2 Bp): p1              (its B)
//   S0         [Bp][Hp]         what the down pass reads: the sample, or p0
//   T[2]       [Bp][Pmax]       the mean-field outputs of the layers below, alternating
//   GW         [Vp][Hp]         the stored weight gradient (bp_rbm_step's trace)
//   chunk      [cap][s_0]       the caller's rows as uploaded, not padded
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bp_c_api.h"

constexpr int RBM_TILE = 64;     // a workgroup's output tile, rows and columns: four waves, one 32 x 32 MFMA block each
constexpr int RBM_KT = 32;       // k-rows per LDS image
static inline int rbm_pad(int x) { return (x + RBM_TILE - 1) / RBM_TILE * RBM_TILE; }

enum { RBM_UP_P0 = 0, RBM_UP_P1 = 1, RBM_UP_MF = 2 };

// Y[rows][cols] = sigma(X[.][K] . W[K][.] + c), pad rows and pad columns stored as 0.
//   RBM_UP_P0: Y = -p0 (into Ps) and S = sample ? (u < p0) : p0 (into S0);  RBM_UP_P1, RBM_UP_MF: Y = the probability.
struct RbmUpArgs {
    const float *X, *W, *c;
    float *Y, *S;
    int ldx, ldw, ldy, K;          // K = Vp
    int rows, cols;                // true sizes: the bunch's rows, H
    int mode, sample;
    uint32_t layer, t, seed_lo, seed_hi;
};
// v1[rows][cols] = visible ? sigma(S0 . W^T + a) : S0 . W^T + a into X1; part[tile] = sum (v0 - v1)^2 of the tile, in double.
struct RbmDownArgs {
    const float *S0, *W, *a, *X0;
    float *X1;
    double *part;
    int lds0, ldw, ldx, K;         // K = Hp
    int rows, cols;                // B, V
    int visible;
};
// g = Xs^T . Ps over K = 2 Bp rows; apply == 0: GW = g; apply == 1: dW' = update_delta(..., dW, g, W), W' = W + dW'.
struct RbmStatsArgs {
    const float *Xs, *Ps;
    float *W, *dW, *GW;
    int ldx, ldp, K;
    int V, H, apply;
    float mom, lrate, wc, ndiv, rdiv;      // rdiv = exact_rdiv(ndiv) (bp_handle.h), 0 = divide
};
// Column sums gc = sum_r (p1 - p0), ga = sum_r (v1 - v0) over the B rows, stored or applied (wc = 0), and the bunch's recon:
// the tiles' partial sums added in tile order, onto *recon.
struct RbmBiasArgs {
    const float *Xs, *Ps;
    float *c, *dc, *a, *da, *gc, *ga;
    const double *part;
    double *recon;
    int ldx, ldp, B, Bp, V, H, apply, n_part;
    float mom, lrate, ndiv, rdiv;
};

hipError_t rbm_rows_launch(float *dst, int ld, int rows_p, const float *src, int count, int width, hipStream_t st);
hipError_t rbm_up_launch(const RbmUpArgs &a, int rows_p, int cols_p, hipStream_t st);
hipError_t rbm_down_launch(const RbmDownArgs &a, int rows_p, int cols_p, hipStream_t st);
hipError_t rbm_stats_launch(const RbmStatsArgs &a, int v_p, int h_p, hipStream_t st);
hipError_t rbm_bias_launch(const RbmBiasArgs &a, hipStream_t st);
