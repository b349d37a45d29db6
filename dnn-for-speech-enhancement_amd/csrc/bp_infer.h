// bp_infer.h -- the row-invariant inference forward of bp_infer.hip (BP_FORWARD_ROWINV), launched by forward_bunch (bp_step.hip).
// Definition: include/bp_c_api.h (bp_set_forward), INTEGRATION.md 1i, DESIGN.md 16.  Internal: nothing in here is part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

// One layer, Y[M][N] = act(alpha * X[M][K] . W[K][N] + bias): rows in tiles of INFER_BM, columns in tiles of INFER_BN, the k
// range in splitk slices of 4 partial sums each (one per wave).  K and N are the padded widths (multiples of 64).
static const int INFER_BM = 32, INFER_BN = 128, INFER_KU = 16, INFER_MAX_SPLITK = 8;

// The decomposition of a layer: a function of its shape (K, N) alone -- never of M, of the bunch or of the handle.
//   tiles_n  column tiles
//   splitk   k-slices (workgroups per output tile): the largest power of two that keeps tiles_n * splitk <= 128 and leaves each
//            of the 4 * splitk partial sums at least 3 units of INFER_KU k-rows
//   per      units of INFER_KU k-rows per partial sum; partial p covers units [p * per, min(K / INFER_KU, (p + 1) * per))
struct InferPlan { int tiles_n, splitk, per; };
static inline InferPlan infer_plan(int K, int N)
{
    InferPlan p;
    const int U = K / INFER_KU;
    p.tiles_n = (N + INFER_BN - 1) / INFER_BN;
    p.splitk = 1;
    while (p.splitk < INFER_MAX_SPLITK && p.tiles_n * p.splitk * 2 <= 128 && U / (4 * p.splitk * 2) >= 3) p.splitk *= 2;
    p.per = (U + 4 * p.splitk - 1) / (4 * p.splitk);
    return p;
}

struct InferArgs {
    const float *X; int ldx;               // input rows [M][ldx]
    const float *W; int ldw;               // weights [K][ldw], N contiguous
    const float *bias;
    float *Y; int ldy;                     // output rows [M][ldy]
    int M, K, N, n_true;
    int splitk, per, tiles_n;
    float alpha;                           // x = alpha * acc + bias (the CV keep-scale)
    int out;                               // 0: hidden layer (act: 0 ReLU | 1 Sigmoid), 1: output layer
    int act, logi, lin_cols;               // output layer: logistic on the columns [lin_cols, n_true) (bp_set_output)
    float *slab; size_t slab_stride;       // splitk > 1: the slices' partial tiles [slice][rows][N], slab_stride = rows * N floats apart
                                           // (rows: the handle's bunch rounded up to INFER_BM; the slab holds splitk of them)
    unsigned *ticket;                      // ... and one ticket word per output tile of this layer (they only grow)
};

hipError_t infer_layer_launch(InferArgs a, hipStream_t st);
