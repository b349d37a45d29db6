// bp_wgrad_dma.h -- weight gradient + fused momentum update with LDS-DMA operand staging (static bunch sizes).
//
//   G = Y_prev^T . dEdX  (SgemmNT, DevFunc.h:57-67; BP_GPU.cu:642), then kernUpdatedelta + kernAccSum
//   (DevFunc.cu:313-318, 270-277) on the tile while it is still in registers, bias gradient by m-tile 0
//   (kernAccSumrow, DevFunc.cu:224-242).
//
// Both operands of this GEMM are k-major in memory ([frame][unit]: the reduction runs over the frames of the bunch),
// which is exactly the LDS image the MFMA fragment fetch wants ([k][m] / [k][n], conflict-free ds_read_b32).  So the
// tiles go global -> LDS by `global_load_lds_dwordx4` (1 KiB per wave instruction = 4 k-rows of a 64-wide tile): no
// register staging, no ds_write, 100 VGPRs (90 while the update had one body) => 4 workgroups per CU instead of 3.  64x64 tiles, 16-row k-tiles in a
// 4-stage LDS ring (32 KB), ONE raw s_barrier per k-tile with an exact, counted s_waitcnt vmcnt (a __syncthreads()
// would fence with vmcnt(0) and drain the DMA queue); the k-loop is fully unrolled for the bunch size, so every count is
// an immediate.  Results are bit-identical to the register-staged GemmKernel<64,64,32,...> it replaced (same k-order,
// same two accumulator chains).  Other shapes of this design that were measured and not adopted (128x64 tiles, dynamic
// k-loop, 3/6-stage rings) live in tools/wgrad_glds_probe.h.
//
// PERSISTENT GRID, RING CARRIED ACROSS TILES.  The launch has G = min(entries, 4 x CUs) workgroups (bp_handle::wgrad_slots);
// workgroup w walks the entries w, w + G, ... of the concatenated tile list of the grouped problems (every problem padded
// to a multiple of 8 entries and G a multiple of 8: w & 7, the XCD, stays the low bits of the problem-relative index the
// tile map wants; padding entries are skipped; consecutive tiles of a walk may belong to different problems).  Invariant
// at every barrier of the walk: the D = ST - 1 = 3 k-tiles that follow the one about to be multiplied are in flight, k-tile j
// of EVERY tile in ring stage j % ST (NT % ST == 0).  From iteration NT - D on, the k-tiles issued are those of the
// workgroup's NEXT tile, so only a workgroup's first tile waits a memory latency before its first MFMA; the tile boundary
// costs no wait and no barrier.  Behind the last tile of a walk the same loads are issued once more from that tile's
// panels and never read (unconditional loads: bp_kernels.h says what a conditional one costs), and drained before exit.
//
// THE vmcnt COUNTS (vmcnt retires in order; LDS-DMA loads, plain loads and stores all count).  A wave's queue, per tile:
//     k0 k1 k2 | S x the previous tile's epilogue stores | k3 ... k(NT-1) | 32 W/delta loads | n0 n1 n2 (next tile) | S stores
// Each k-tile is NDMA = 2 instructions per wave.  The wait in front of k-tile T leaves outstanding what was issued behind it:
// the two following k-tiles (4), plus the 32 W/delta loads for T > NT - D, plus -- for T < D of every tile but the
// workgroup's first -- the S = 32 (fused) / 16 (store form) stores of the previous epilogue, which must not be waited
// for: a store's acknowledgement is a memory latency of its own.  S is a LOWER bound of what lies there (bias lanes and
// the tile count add to it): more behind a k-tile than counted only makes its wait stricter.  It holds because no tile of
// a padded layer is partial; after an epilogue that stored nothing the wave drains instead.  The W / delta tile is fetched
// right behind the tile's LAST operand k-tile and has three k-tiles of MFMA work to land; the epilogue waits for it with
// vmcnt(D * NDMA), which leaves the next tile's head in flight.  Those loads are written out (wd_fetch): with LDS-DMA in
// flight the compiler turns every wait it places for a load of its own into vmcnt(0).
// THE UPDATE HAS TWO BODIES, chosen per tile on the uniform e.rdiv != 0 (update_delta<RCP>, bp_device.h): the quotient g / ndiv as one
// v_mul_f32 by the exact reciprocal of a power-of-two bunch -- per value v_mul, v_fmac, v_pk_mul, v_sub, v_add and two stores, no
// v_div_* / v_rcp between the tile's last MFMA and its stores -- or the IEEE division (11 dependent VALU instructions per value, 187
// of a tile's ~300; every bunch this launch is built for is a power of two, so that body is cold).  Both bodies store the same 32
// words per lane: the counts above hold for either.  (The bias lanes are the same choice; their bias_w / bias_d loads are the
// compiler's own and drain with vmcnt(0) as they did -- m-tile 0 only.)
// The bias reduction's scratch is ring stage ST - 1: it held the tile's last k-tile and is next written behind the barrier
// of the next tile's iter<0>.  Measured on C2 (grouped launch of all four layers, rocprofv3 average in the step): 74.5 us
// against 77.5 us for one tile per workgroup (profiles/r08_wgrad_cross_tile_prefetch.txt).
#pragma once
#include "bp_kernels.h"

// template <BK, ST, MINWG, K>: K = frames of the bunch (static).  Prefetch distance D = ST-1 k-tiles.
template <int N> struct VmWait { static __device__ __forceinline__ void go() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N < 63 ? N : 63) : "memory"); } };

template <int BKX, int STX, int MINWG, int KTOT, bool STORE = false>
struct WgradDma {
    // STORE: data-parallel form -- the gradient tile and the bias gradient go to the flat gradient buffer (e.C / e.bias_g),
    // no W / delta traffic; otherwise the fused momentum update
    static constexpr int EPI = STORE ? EPI_WGRAD_STORE : EPI_WGRAD_UPDATE;
    static constexpr int NWD = STORE ? 0 : 32;                    // plain loads of the W / delta tile per lane
    static constexpr int BM = 64, BN = 64, BK = BKX, ST = STX, NT = KTOT / BKX, D = STX - 1;
    static constexpr int A_STAGE = BK * BM, B_STAGE = BK * BN, STAGE = A_STAGE + B_STAGE;
    static constexpr int SMEM = ST * STAGE;
    static constexpr int MIN_WG = MINWG;
    static constexpr int NA = A_STAGE / 1024, NB = B_STAGE / 1024, NDMA = NA + NB;
    static_assert(NA >= 1 && NB >= 1 && NT > D, "shape");
    typedef __attribute__((address_space(3))) void *lds_ptr;
    typedef const __attribute__((address_space(1))) void *glb_ptr;

    // Stores of one wave's epilogue (no tile of a padded layer is partial, run() drains after one that were): what lies between
    // the carried k-tiles 0..D-1 of a tile and its k-tile D in the wave's queue.  A LOWER bound is what the waits need: more
    // operations behind a k-tile than counted only make its wait stricter (bias lanes, the tile count of the store form).
    static constexpr int NST = STORE ? 16 : 32;
    static_assert(NT % ST == 0, "k-tile j of EVERY tile lies in ring stage j % ST: the ring runs on across tiles");
    static_assert(NT >= 2 * D, "the carried head and the W/delta tail of a tile do not overlap");
    static_assert((D - 1) * NDMA + (NWD > NST ? NWD : NST) < 64, "vmcnt is 6 bits");

    struct Pos { int p, m0, n0; };                                // problem of the launch, origin of the tile
    struct Src { const float *a, *b; int lda, ldb; unsigned oa, ob; };       // operand panels of one tile (k-row 0); the lane's byte offsets (lane_off)

    // entry i of the concatenated tile list (every problem padded to a multiple of 8 entries): false for a padding entry.
    // t.p only grows along a workgroup's walk.
    static __device__ __forceinline__ bool decode(const MultiArgs &a, int i, Pos &t)
    {
        const int p = problem_of(a, i, t.p);
        const GemmArgs &g = a.g[p];
        const int b = i - a.first_tile[p];                        // (low 3 bits = the workgroup's XCD: G and first_tile are multiples of 8)
        if (b >= g.tiles_m * g.tiles_n) return false;
        int tile_m, tile_n;
        xcd_tile<true>(b, g.tiles_m, g.tiles_n, tile_m, tile_n);
        t.p = p; t.m0 = tile_m * BM; t.n0 = tile_n * BN;
        return true;
    }
    static __device__ __forceinline__ int seek(const MultiArgs &a, int i, int stride, int total, Pos &t)
    {
        while (i < total && !decode(a, i, t)) i += stride;
        return i;
    }
    static __device__ __forceinline__ Src src_of(const MultiArgs &a, const Pos &t, int wave, int lane)
    {
        const GemmArgs &g = a.g[t.p];
        return Src{g.A + t.m0, g.B + t.n0, g.lda, g.ldb, lane_off(g.lda, wave, lane), lane_off(g.ldb, wave, lane)};
    }

    // The W / delta tile of one wave's 32x32 block (the lane -> element map of epilogue_fetch, bp_kernels.h).  The loads are
    // written out: with LDS-DMA in flight hipcc turns every wait IT places for a load into vmcnt(0), which here would drain the
    // next tile's head in every epilogue (and, through the registers of a skipped epilogue, in every iter<0>).  So the compiler
    // never sees these registers pending; wd_landed() is the one wait, and hands the values on only behind it.
    struct WD { float w[16], d[16]; };
    static __device__ __forceinline__ void wd_fetch(const EpiArgs &e, int mb, int nb, int lane, WD &x)
    {
        const int mbc = mb < e.m_limit ? mb : 0;                  // (a block outside the matrix reads row 0 and is never stored)
        const float *cw = uniform_ptr(e.C + (size_t)mbc * e.ldc + nb);
        const float *cd = uniform_ptr(e.aux2 + (size_t)mbc * e.ldc + nb);
        const unsigned ldc = __builtin_amdgcn_readfirstlane(e.ldc);
        const unsigned lob = 4u * ((unsigned)(4 * (lane >> 5)) * (unsigned)e.ldc + (unsigned)(lane & 31));   // bytes
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const unsigned ro = (unsigned)((r & 3) + 8 * (r >> 2)) * ldc;
            // (r == 0: the hazard recogniser does not look into these, and a base that came straight from a v_readfirstlane must be 5
            // wait states old when a load reads it)
            if (r == 0) asm volatile("s_nop 4\n\tglobal_load_dword %0, %1, %2" : "=v"(x.w[r]) : "v"(lob), "s"(cw + ro) : "memory");
            else asm volatile("global_load_dword %0, %1, %2" : "=v"(x.w[r]) : "v"(lob), "s"(cw + ro) : "memory");
            asm volatile("global_load_dword %0, %1, %2" : "=v"(x.d[r]) : "v"(lob), "s"(cd + ro) : "memory");
        }
    }
    // behind the W/delta loads at the epilogue: the D k-tiles of the next tile's head, which stay in flight
    static __device__ __forceinline__ void wd_landed(WD &x, EpiPre &pre)
    {
        VmWait<D * NDMA>::go();
#pragma unroll
        for (int r = 0; r < 16; r += 8) {
            asm volatile("" : "+v"(x.w[r]), "+v"(x.w[r + 1]), "+v"(x.w[r + 2]), "+v"(x.w[r + 3]), "+v"(x.w[r + 4]), "+v"(x.w[r + 5]), "+v"(x.w[r + 6]), "+v"(x.w[r + 7]) :: "memory");
            asm volatile("" : "+v"(x.d[r]), "+v"(x.d[r + 1]), "+v"(x.d[r + 2]), "+v"(x.d[r + 3]), "+v"(x.d[r + 4]), "+v"(x.d[r + 5]), "+v"(x.d[r + 6]), "+v"(x.d[r + 7]) :: "memory");
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) { pre.p0[r] = x.w[r]; pre.p1[r] = x.d[r]; }
    }

    // One k-tile: uniform row base (SGPRs) + the lane's byte offset inside a k-tile of its panel (lane_off, formed once per tile in
    // src_of; NA = NB = 1: wave w moves k-rows 4w .. 4w+3 of either operand) -- one 32-bit address register per operand, and the
    // DMA is global_load_lds_dwordx4 v_off, s[base:base+1].  The offsets are made opaque in place in front of every DMA: their zero
    // extension then stays in the block of the DMA, where instruction selection folds it into the address.  (Left alone it is
    // hoisted in front of the tile, comes back as a 64-bit VGPR pair, and every DMA but the first of a tile pays a 64-bit VALU
    // add between the MFMAs.)  The empty asm issues nothing: the queue accounting below is what it was.
    static_assert(NA == 1 && NB == 1, "one LDS-DMA per wave, operand and k-tile");
    static __device__ __forceinline__ unsigned lane_off(int ld, int wave, int lane) { return 4u * ((unsigned)(wave * 4 + (lane >> 4)) * (unsigned)ld + (unsigned)(lane & 15) * 4u); }
    static __device__ __forceinline__ void issue_tile(Src &s, int k0, float *smem, int st, int wave, int lane)
    {
        const char *pa = reinterpret_cast<const char *>(sgpr_row_base(s.a + (size_t)k0 * s.lda));
        const char *pb = reinterpret_cast<const char *>(sgpr_row_base(s.b + (size_t)k0 * s.ldb));
        asm volatile("" : "+v"(s.oa), "+v"(s.ob));
        __builtin_amdgcn_global_load_lds((glb_ptr)(pa + s.oa), (lds_ptr)(smem + st * STAGE + wave * 256), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((glb_ptr)(pb + s.ob), (lds_ptr)(smem + st * STAGE + A_STAGE + wave * 256), 16, 0, 0);
    }
    static __device__ __forceinline__ void multiply(const float *smem, int st, int a_off, int b_off, int kh, f32x16 (&acc)[2])
    {
        constexpr int NK = BK / 2, RD = NK < 4 ? NK : 4;
        const float *ap = smem + st * STAGE + kh * BM + a_off, *bp = smem + st * STAGE + A_STAGE + kh * BN + b_off;
        float av[NK], bv[NK];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s = 0; s < RD; ++s) { av[s] = ap[2 * s * BM]; bv[s] = bp[2 * s * BN]; }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s = 0; s < NK; ++s) {
            acc[s & 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], bv[s], acc[s & 1], 0, 0, 0);
            if (s + RD < NK) { av[s + RD] = ap[2 * (s + RD) * BM]; bv[s + RD] = bp[2 * (s + RD) * BN]; }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    // k-tile T of the tile `cur`.  carried: this is not the workgroup's first tile, so the epilogue stores of the tile before lie in
    // the queue between k-tiles D-1 and D.
    template <int T>
    static __device__ __forceinline__ void iter(Src &cur, Src &nxt, const EpiArgs &e, bool carried, float *smem, int wave, int lane, int tid,
                                                int a_off, int b_off, int kh, int mb, int nb, bool do_bias, float &bsum, f32x16 (&acc)[2], WD &wd)
    {
        if constexpr (T < NT) {
            // behind k-tile T at this point: k-tiles T+1 .. T+D-1 (of the next tile from NT on), the W/delta loads once issued, and
            // the previous tile's stores while k-tile D has not been issued
            constexpr int behind = (D - 1) * NDMA + (T + D > NT ? NWD : 0);
            if constexpr (T < D) { if (carried) VmWait<behind + NST>::go(); else VmWait<behind>::go(); }
            else VmWait<behind>::go();
            __builtin_amdgcn_s_barrier();
            if constexpr (T + D < NT) issue_tile(cur, (T + D) * BK, smem, (T + D) % ST, wave, lane);
            if constexpr (T + D == NT && !STORE) wd_fetch(e, mb, nb, lane, wd);   // behind the last k-tile (issued at T-1)
            if constexpr (T + D >= NT) issue_tile(nxt, (T + D - NT) * BK, smem, (T + D) % ST, wave, lane);       // the next tile's head
            if (do_bias) {
                constexpr int RPT = BK / 4;
                const float *bs = smem + (T % ST) * STAGE + A_STAGE + (tid >> 6) * RPT * BN + (tid & 63);
#pragma unroll
                for (int k = 0; k < RPT; ++k) bsum += bs[k * BN];
            }
            multiply(smem, T % ST, a_off, b_off, kh, acc);
            iter<T + 1>(cur, nxt, e, carried, smem, wave, lane, tid, a_off, b_off, kh, mb, nb, do_bias, bsum, acc, wd);
        }
    }
    // Workgroup w of G walks the entries w, w + G, ... of the launch's tile list.
    static __device__ __forceinline__ void run(const MultiArgs &a, float *smem)
    {
        const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
        const int wm = wave >> 1, wn = wave & 1;
        const int stride = gridDim.x, total = a.first_tile[a.n];
        Pos t; t.p = 0;
        int i = seek(a, blockIdx.x, stride, total, t);
        if (i >= total) return;
        Src cur = src_of(a, t, wave, lane);
#pragma unroll
        for (int k = 0; k < D; ++k) issue_tile(cur, k * BK, smem, k, wave, lane);
        bool carried = false;
        for (;;) {
            // the tile after this one; none: the same loads again from this tile's panels, never read (a conditional load would
            // cost every wait its immediate)
            Pos tn = t;
            const int in = seek(a, i + stride, stride, total, tn);
            const bool more = in < total;
            Src nxt = more ? src_of(a, tn, wave, lane) : cur;
            const EpiArgs &e = a.e[t.p];
            const int mb = t.m0 + wm * 32, nb = t.n0 + wn * 32;
            const int a_off = wm * 32 + (lane & 31), b_off = wn * 32 + (lane & 31), kh = lane >> 5;
            f32x16 acc[2];
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc[0][r] = 0.f; acc[1][r] = 0.f; }
            const bool do_bias = t.m0 == 0;
            float bsum = 0.f;
            WD wd;
            iter<0>(cur, nxt, e, carried, smem, wave, lane, tid, a_off, b_off, kh, mb, nb, do_bias, bsum, acc, wd);
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[0][r] += acc[1][r];
            if (do_bias) {
                // scratch in stage ST-1: it held this tile's last k-tile and is next written by k-tile D of the next tile, behind the
                // barrier of its iter<0>; stages 0..D-1 are receiving the next tile.  Raw barriers: nothing is drained.
                float *red = smem + (ST - 1) * STAGE;
                __builtin_amdgcn_s_barrier();                     // every wave has multiplied the last k-tile
                red[(tid >> 6) * BN + (tid & 63)] = bsum;
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                if (tid < BN && t.n0 + tid < e.n_limit) {
                    const float s = (red[tid] + red[BN + tid]) + (red[2 * BN + tid] + red[3 * BN + tid]);
                    const int n = t.n0 + tid;
                    if constexpr (STORE) {
                        __hip_atomic_store(e.bias_g + n, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);     // (write-through, like the tile below)
                    } else {
                        if (e.rdiv != 0.0f) bias_update<true>(e, n, s); else bias_update<false>(e, n, s);
                    }
                }
            }
            EpiPre pre;
            if constexpr (!STORE) wd_landed(wd, pre);
            // the fused update as two bodies, chosen once per tile: the quotient g / ndiv as one multiply where that is the division
            // to the bit (e.rdiv != 0: a power-of-two bunch), the IEEE division otherwise (update_delta, bp_device.h)
            if constexpr (STORE) epilogue_block<EPI, 0, 16>(e, mb, nb, acc[0], lane, pre);
            else if (e.rdiv != 0.0f) epilogue_block<EPI, 0, 16, true>(e, mb, nb, acc[0], lane, pre);
            else epilogue_block<EPI, 0, 16, false>(e, mb, nb, acc[0], lane, pre);
            if (mb >= e.m_limit || nb >= e.n_limit) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // no stores: NST does not hold
            if constexpr (STORE) {
                // data-parallel step: tell the exchange stream that this tile of the layer's gradient segment is complete, WITHOUT a
                // kernel boundary (one grouped launch for all layers; the exchange of layer 1 starts while the other layers' tiles
                // still run).  The tile and the bias gradient were stored with system-scope write-through stores (sc0 sc1,
                // epilogue_block): every storing wave drains vmcnt -- an acknowledged write-through store is in memory --, the
                // workgroup meets at a barrier, one lane counts the tile (relaxed, system scope).  That is the store half of the memory
                // model's own code sequence for system-scope atomics; it needs no L2 write-back because nothing was left dirty.
                // Measured alternatives (C2 through the exchange path at world 1, profiles/r05_dp_world1.txt): a system-scope RELEASE on
                // the count (ADVICE r4's first proposal: one buffer_wbl2 per tile, 3648 per step) 0.3445 ms against 0.2533; one release
                // per layer on every XCD inside bp_dp_sync 0.2750 (16 waves) / 0.2640 (8) against 0.2551.
                // (The drain takes the next tile's head with it: it was issued before the stores.)
                if (e.done) {
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    __syncthreads();
                    if (tid == 0) __hip_atomic_fetch_add(e.done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                }
            }
            if (!more) break;
            t = tn; i = in; cur = nxt; carried = true;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // the unread head behind the last tile lands before the LDS is given back
    }
};

template <int BKX, int STX, int MINWG, int KTOT, bool STORE = false>
__global__ __launch_bounds__(256, MINWG) void bp_wgrad_dma(const MultiArgs a)
{
    using K = WgradDma<BKX, STX, MINWG, KTOT, STORE>;
    __shared__ __attribute__((aligned(16))) float smem[K::SMEM];
    K::run(a, smem);
}
