// bp_room.hip -- C-ABI implementation (include/bp_c_api.h): room acoustics.  Sentences convolved with room impulse responses
// (bp_reverb_waves; for the mixing corpus bp_set_mix_reverb of bp_mix.hip, through bp_room.h) and the responses themselves simulated
// with the image method (bp_rir_image).  Neither call has a handle: each runs in a OneShot of bp_handle.h.  gfx950 only.
//
// Kernels:
//   bp_mix_reverb_fir  clean sentences convolved with room impulse responses, once per call: the derived entries n_clean + k of the
//                    mixing corpus, or the sentences of bp_reverb_waves
//   bp_rir_image_taps  room impulse responses by the image method, one workgroup per 256 taps of a response:
//                    what bp_set_mix_reverb takes when there are no measured responses
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "bp_fft.h"
#include "bp_handle.h"
#include "bp_philox_host.h"
#include "bp_room.h"

// ------------------------------------------------------------------ reverberant entries
// bp_mix_reverb_fir: r[i] = fl32(sum_j (double)h[j] (double)s[i + d - j]), j ascending, one double accumulator per output sample (the
// order over j is the definition: no tap of a sample is ever added by another thread).  A workgroup owns RV_BLOCK consecutive
// outputs of one job, a thread RV_R consecutive ones.  Per tile of RV_TILE taps the workgroup stages, already converted to double,
// the taps and the RV_BLOCK + RV_TILE source samples the tile touches; a thread then walks the tile 8 taps at a time with the 15
// source samples those 8 taps x 8 outputs need held in registers (8 new ones per step, one aligned chunk of the segment).  The
// segment is stored with 2 doubles of padding after every 8, which makes the lanes' 64-byte chunks 80 bytes apart: every 16-lane
// group of a ds_read_b128 then covers all 64 banks once.  Taps are read as broadcasts.  Tiles whose samples all lie outside
// [0, n) add exact zeros and are skipped.  EARLY: the accumulators are also copied when tap je has been added.
namespace {
constexpr int RV_R = 8, RV_BLOCK = WAVE_THREADS * RV_R, RV_TILE = WAVE_THREADS;
static_assert(RV_R == 8 && RV_TILE % 8 == 0, "the inner step is 8 taps x 8 outputs");

__device__ __forceinline__ int rv_pad(int k) { return k + ((k >> 3) << 1); }

// taps hh[0..7] on outputs 0..7: tap u of output r reads sample 7 - u + r of cur (0..7) | prev (8..14); jl: the tap after which the
// accumulators are copied (SNAP), else unused
template <bool SNAP>
__device__ __forceinline__ void rv_step(double (&acc)[RV_R], double (&snap)[RV_R], const double (&hh)[8], const double (&cur)[8],
                                        const double (&prev)[8], int jl)
{
#pragma unroll
    for (int u = 0; u < 8; ++u) {
#pragma unroll
        for (int r = 0; r < RV_R; ++r) {
            const int k = 7 - u + r;
            acc[r] = fma(hh[u], k < 8 ? cur[k] : prev[k - 8], acc[r]);
        }
        if (SNAP && u == jl) {
#pragma unroll
            for (int r = 0; r < RV_R; ++r) snap[r] = acc[r];
        }
    }
}
}  // namespace

template <bool EARLY>
__global__ __launch_bounds__(WAVE_THREADS) void bp_mix_reverb_fir(const ReverbArgs a)
{
    __shared__ __attribute__((aligned(16))) double seg[(RV_BLOCK + RV_TILE) / 8 * 10];
    __shared__ __attribute__((aligned(16))) double tap[RV_TILE];
    const int q = blockIdx.x, tid = threadIdx.x, o0 = tid * RV_R;
    int lo = 0, hi = a.n_job - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (a.job[mid].blk0 <= q) lo = mid; else hi = mid - 1; }
    const ReverbJob J = a.job[lo];
    const float *s = a.src + J.src, *h = a.rir + J.rir;
    const int i0 = (q - J.blk0) * RV_BLOCK, i_last = min(i0 + RV_BLOCK, J.n) - 1;
    // tile t (taps [t RV_TILE, (t+1) RV_TILE)) reads samples [i0 + d - (t+1) RV_TILE + 1, i_last + d - t RV_TILE]: inside [0, n) for
    // a contiguous range of t only
    const int nt = (J.Lh + RV_TILE - 1) / RV_TILE, qlo = i0 + J.d - J.n - RV_TILE + 2;
    const int ta = qlo <= 0 ? 0 : (qlo + RV_TILE - 1) / RV_TILE, tb = min(nt, (i_last + J.d) / RV_TILE + 1);
    double acc[RV_R], snap[RV_R];
#pragma unroll
    for (int r = 0; r < RV_R; ++r) acc[r] = snap[r] = 0.0;
    for (int t = ta; t < tb; ++t) {
        const int j0 = t * RV_TILE, base = i0 + J.d - j0 - RV_TILE + 1;
        __syncthreads();                                         // (the previous tile is read)
        for (int k = tid; k < RV_BLOCK + RV_TILE; k += WAVE_THREADS) {
            const int p = base + k;
            seg[rv_pad(k)] = p >= 0 && p < J.n ? (double)s[p] : 0.0;
        }
        tap[tid] = j0 + tid < J.Lh ? (double)h[j0 + tid] : 0.0;
        __syncthreads();
        const int ng = (min(RV_TILE, J.Lh - j0) + 7) >> 3, jl = J.je - j0;
        double prev[8], cur[8], hh[8];
        {
            const double *c = seg + rv_pad(o0 + RV_TILE);
#pragma unroll
            for (int k = 0; k < 8; ++k) prev[k] = c[k];
        }
        for (int g = 0; g < ng; ++g) {
            const double *c = seg + rv_pad(o0 + RV_TILE - 8 - 8 * g);
#pragma unroll
            for (int k = 0; k < 8; ++k) { cur[k] = c[k]; hh[k] = tap[8 * g + k]; }
            if (EARLY && (jl >> 3) == g) rv_step<true>(acc, snap, hh, cur, prev, jl & 7);
            else rv_step<false>(acc, snap, hh, cur, prev, 0);
#pragma unroll
            for (int k = 0; k < 8; ++k) prev[k] = cur[k];
        }
    }
    if (EARLY && J.je >= tb * RV_TILE) {                         // (the rest of the early sum was skipped zeros)
#pragma unroll
        for (int r = 0; r < RV_R; ++r) snap[r] = acc[r];
    }
#pragma unroll
    for (int r = 0; r < RV_R; ++r) {
        const int i = i0 + o0 + r;
        if (i < J.n) {
            if (a.out_r) a.out_r[J.dst + i] = (float)acc[r];
            if (EARLY) a.out_e[J.dst + i] = (float)snap[r];
        }
    }
}

// ------------------------------------------------------------------ simulated responses
// bp_rir_image_taps: h[j] = fl32(sum over the images of a w(j - tau)), the images in the order of include/bp_c_api.h, one double
// accumulator per tap.  A workgroup owns RIR_BLOCK consecutive taps of one response, a thread one tap.  It walks the box plane by
// plane (axis 2), each plane in chunks of RIR_BLOCK images in image order: a thread computes dist, tau and a of one image, the
// images whose window misses the block's taps (or whose a is 0) are dropped, the others are appended IN IMAGE ORDER (ballot and
// prefix count within the wave, then wave order) to a list in LDS.  When the list may not take another chunk, every thread adds
// the listed images' terms to its tap, in list order.  Planes and chunks whose nearest image lies beyond the block's last tap
// are skipped without a distance evaluation: their terms are exact zeros.  Whether an image is listed depends on the block
// alone and never changes the order of the others.  sin and cos are called per image and per tap (the factored window of the
// header), the term itself is one division, two fmas, two multiplies and a select.
namespace {
constexpr int RIR_BLOCK = WAVE_THREADS, RIR_LIST = 2 * RIR_BLOCK, RIR_WAVES = WAVE_THREADS / 64;
constexpr double RIR_C = 343.0, RIR_PI = 3.14159265358979323846;
// response k: its room, orders N, taps; tab: first double of its tables B_0 | B_1 | B_2 (B_d[(n + N_d) 2 + p]); out: its first
// tap; blk0: its first workgroup
struct RirJob { double L[3], src[3], mic[3], d0; int64_t tab, out; int N[3], n_taps, blk0, pad; };
struct RirArgs { const RirJob *job; int n_job, Tw; double fs_c, inv_Tw; const double *tab; float *out; };
struct RirImage { double tau, a, s, cw, sw; };                   // s: -(-1)^m sin(pi f) a / (2 pi); cw, sw: cos, sin(2 pi tau / Tw)

// |x| of the images (n, 0) and (n, 1) of one axis, the smaller
__device__ __forceinline__ double rir_near(double src, double mic, double L, int n)
{
    const double t = 2.0 * (double)n * L - mic;
    return fmin(fabs(t + src), fabs(t - src));
}
}  // namespace

__global__ __launch_bounds__(WAVE_THREADS) void bp_rir_image_taps(const RirArgs a)
{
    __shared__ RirImage list[RIR_LIST];
    __shared__ int wcnt[2][RIR_WAVES];
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int lo = 0, hi = a.n_job - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (a.job[mid].blk0 <= q) lo = mid; else hi = mid - 1; }
    const RirJob &J = a.job[lo];
    const int j0 = (q - J.blk0) * RIR_BLOCK, j = j0 + tid, Tw = a.Tw;
    const double hw = 0.5 * (double)Tw, fs_c = a.fs_c, d0 = J.d0;
    const int N0 = J.N[0], N1 = J.N[1], N2 = J.N[2], R0 = 2 * (2 * N0 + 1), R1 = 2 * (2 * N1 + 1), R2 = 2 * (2 * N2 + 1);
    const double L0 = J.L[0], L1 = J.L[1], L2 = J.L[2], s0 = J.src[0], s1 = J.src[1], s2 = J.src[2];
    const double m0 = J.mic[0], m1 = J.mic[1], m2 = J.mic[2];
    const double *B0 = a.tab + J.tab, *B1 = B0 + R0, *B2 = B1 + R1;
    // the block's taps [j0, j0 + RIR_BLOCK): an image reaches one of them only if tau + hw >= j0 and tau - hw <= j0 + RIR_BLOCK - 1;
    // rmax: a distance beyond which tau - hw is certainly past the last tap (one tap of margin for the roundings)
    const double t_lo = (double)j0 - hw, t_hi = (double)(j0 + RIR_BLOCK - 1) + hw;
    const double rmax = (t_hi + 1.0) / fs_c, rmax2 = rmax * rmax;
    // this thread's tap: cos, sin(2 pi j / Tw) from j mod Tw, and (-1)^j
    const double tj = (double)j, pj = (2.0 * RIR_PI) * (double)(j % Tw) * a.inv_Tw;
    const double cj = cos(pj), sj = sin(pj), gj = (j & 1) ? -1.0 : 1.0;
    double acc = 0.0;
    int n_list = 0, par = 0;
    // every thread adds the listed images' terms to its tap, in list order
    auto add_list = [&]() {
        __syncthreads();
        for (int i = 0; i < n_list; ++i) {
            const RirImage im = list[i];
            const double u = tj - im.tau;
            const double t = (gj * im.s) / u * (1.0 + (cj * im.cw + sj * im.sw));
            acc += fabs(u) < hw ? (u == 0.0 ? im.a : t) : 0.0;
        }
        __syncthreads();
        n_list = 0;
    };
    const int64_t plane_n = (int64_t)R1 * R0;                    // (<= 2^26 / 2)
    for (int z = 0; z < R2; ++z) {
        const double x2 = ((z & 1) ? -s2 : s2) + 2.0 * (double)((z >> 1) - N2) * L2 - m2, x22 = x2 * x2;
        if (x22 > rmax2) continue;
        const double b2 = B2[z];
        for (int64_t c0 = 0; c0 < plane_n; c0 += RIR_BLOCK) {
            // rows (n1, p1) the chunk touches: ya .. yb; away from n1 in [-1, 1] the nearest of them is at one end
            const int ya = (int)(c0 / R0), yb = (int)((min(c0 + (int64_t)RIR_BLOCK, plane_n) - 1) / R0);
            const int na = (ya >> 1) - N1, nb = (yb >> 1) - N1;
            if (na > 1 || nb < -1) {
                const double y = fmin(rir_near(s1, m1, L1, na), rir_near(s1, m1, L1, nb));
                if (y * y + x22 > rmax2) continue;
            }
            const int64_t c = c0 + tid;
            bool keep = false;
            RirImage im = {0.0, 0.0, 0.0, 0.0, 0.0};
            if (c < plane_n) {
                const int y = (int)(c / R0), x = (int)(c - (int64_t)y * R0);
                const double x1 = ((y & 1) ? -s1 : s1) + 2.0 * (double)((y >> 1) - N1) * L1 - m1;
                const double x0 = ((x & 1) ? -s0 : s0) + 2.0 * (double)((x >> 1) - N0) * L0 - m0;
                const double dist = sqrt((x0 * x0 + x1 * x1) + x22), tau = dist * fs_c;
                const double amp = ((B0[x] * B1[y]) * b2) * (d0 / dist);
                keep = amp != 0.0 && tau >= t_lo && tau <= t_hi;
                if (keep) {
                    const double m = rint(tau), f = tau - m, tm = tau - (double)Tw * floor(tau * a.inv_Tw);
                    const double pw = (2.0 * RIR_PI) * tm * a.inv_Tw, sf = sin(RIR_PI * f);
                    im.tau = tau; im.a = amp;
                    im.s = (((int64_t)m & 1) ? sf : -sf) * amp * (0.5 / RIR_PI);
                    im.cw = cos(pw); im.sw = sin(pw);
                }
            }
            const unsigned long long mask = __ballot(keep);
            if (lane == 0) wcnt[par][wave] = __popcll(mask);
            __syncthreads();
            int at = n_list, tot = 0;
#pragma unroll
            for (int w = 0; w < RIR_WAVES; ++w) { const int k = wcnt[par][w]; if (w < wave) at += k; tot += k; }
            if (keep) list[at + __popcll(mask & ((1ull << lane) - 1ull))] = im;
            n_list += tot; par ^= 1;
            if (n_list > RIR_LIST - RIR_BLOCK) add_list();       // (the list may not take another chunk)
        }
    }
    add_list();
    if (j < J.n_taps) a.out[J.out + j] = (float)acc;
}

// ------------------------------------------------------------------ reverberant entries: host side
namespace {

int rir_delay(const float *h, int n)
{
    int d = 0;
    for (int j = 1; j < n; ++j)
        if (fabsf(h[j]) > fabsf(h[d])) d = j;
    return d;
}

}  // namespace

int check_rirs(const char *who, int n_rir, const int *rir_len, const float *rir_pcm, int early_taps, std::vector<int64_t> &off,
               std::vector<int> &delay)
{
    if (!rir_len || !rir_pcm) return fail(BP_ERR_ARG, std::string(who) + ": null pointer");
    if (n_rir < 1) return fail(BP_ERR_ARG, std::string(who) + ": need at least one impulse response");
    if (early_taps < 0) return fail(BP_ERR_ARG, std::string(who) + ": early_taps is negative");
    off.assign((size_t)n_rir + 1, 0); delay.assign(n_rir, 0);
    for (int k = 0; k < n_rir; ++k) {
        if (rir_len[k] < 1 || rir_len[k] > BP_MIX_RIR_MAX_TAPS)
            return fail(BP_ERR_ARG, std::string(who) + ": impulse response " + std::to_string(k) + ": length outside [1, " +
                                    std::to_string(BP_MIX_RIR_MAX_TAPS) + "]");
        off[k + 1] = off[k] + rir_len[k];
    }
    for (int k = 0; k < n_rir; ++k) {
        const float *hh = rir_pcm + off[k];
        for (int j = 0; j < rir_len[k]; ++j)
            if (!std::isfinite(hh[j])) return fail(BP_ERR_ARG, std::string(who) + ": impulse response " + std::to_string(k) + ": tap " +
                                                                   std::to_string(j) + " is not finite");
        delay[k] = rir_delay(hh, rir_len[k]);
    }
    return BP_OK;
}

int64_t fill_jobs(std::vector<ReverbJob> &job, const std::vector<int64_t> &off, const std::vector<int> &delay, const int *rir_len,
                  int early_taps)
{
    int64_t blk = 0, dst = 0;
    for (ReverbJob &j : job) {
        const int k = (int)j.rir;                                // (the caller left the response's index here)
        j.rir = off[k]; j.Lh = rir_len[k]; j.d = delay[k];
        j.je = (int)std::min<int64_t>((int64_t)j.Lh - 1, (int64_t)j.d + early_taps);
        j.dst = dst; j.blk0 = (int)blk; j.pad = 0;
        dst += j.n; blk += (j.n + RV_BLOCK - 1) / RV_BLOCK;
    }
    return blk;
}

hipError_t reverb_launch(const ReverbArgs &a, int64_t blocks, bool early, hipStream_t st)
{
    if (early) bp_mix_reverb_fir<true><<<dim3((unsigned)blocks), dim3(WAVE_THREADS), 0, st>>>(a);
    else bp_mix_reverb_fir<false><<<dim3((unsigned)blocks), dim3(WAVE_THREADS), 0, st>>>(a);
    return hipGetLastError();
}

extern "C" int bp_mix_rir_delay(const float *h, int n_taps, int *delay)
{
    if (!h || !delay) return fail(BP_ERR_ARG, "bp_mix_rir_delay: null pointer");
    if (n_taps < 1 || n_taps > BP_MIX_RIR_MAX_TAPS) return fail(BP_ERR_ARG, "bp_mix_rir_delay: length outside [1, " + std::to_string(BP_MIX_RIR_MAX_TAPS) + "]");
    for (int j = 0; j < n_taps; ++j)
        if (!std::isfinite(h[j])) return fail(BP_ERR_ARG, "bp_mix_rir_delay: tap " + std::to_string(j) + " is not finite");
    *delay = rir_delay(h, n_taps);
    return BP_OK;
}

extern "C" int bp_mix_reverb_pairs(uint64_t seed, int n_clean, int n_rir, int *pair_rir)
{
    if (n_clean < 1 || n_rir < 1 || !pair_rir) return fail(BP_ERR_ARG, "bp_mix_reverb_pairs: need n_clean, n_rir >= 1 and a non-null array");
    for (int c = 0; c < n_clean; ++c) pair_rir[c] = (int)scale(word0(seed, (uint32_t)c, 0, 3), (uint64_t)n_rir);
    return BP_OK;
}

extern "C" int bp_reverb_waves(int device, int n_sent, const int *sent_len, const float *pcm, const int *sent_rir, int n_rir, const int *rir_len,
                               const float *rir_pcm, int early_taps, float *out_rev, float *out_early)
{
    std::vector<int64_t> off;
    std::vector<int> delay;
    int rc;
    if ((rc = check_rirs("bp_reverb_waves", n_rir, rir_len, rir_pcm, early_taps, off, delay)) != BP_OK) return rc;
    if (n_sent < 1 || !sent_len || !pcm || !sent_rir) return fail(BP_ERR_ARG, "bp_reverb_waves: need at least one sentence and non-null arrays");
    if (!out_rev && !out_early) return fail(BP_ERR_ARG, "bp_reverb_waves: both outputs are null");
    std::vector<ReverbJob> job(n_sent);
    int64_t tot = 0;
    for (int k = 0; k < n_sent; ++k) {
        if (sent_len[k] < 1 || sent_len[k] > RV_MAX_LEN) return fail(BP_ERR_ARG, "bp_reverb_waves: sentence " + std::to_string(k) + ": length outside [1, 2^30]");
        if (sent_rir[k] < 0 || sent_rir[k] >= n_rir) return fail(BP_ERR_ARG, "bp_reverb_waves: sentence " + std::to_string(k) + ": response index out of range");
        job[k].src = tot; job[k].n = sent_len[k]; job[k].rir = sent_rir[k];
        tot += sent_len[k];
    }
    const int64_t blocks = fill_jobs(job, off, delay, rir_len, early_taps);
    if (blocks > INT32_MAX) return fail(BP_ERR_ARG, "bp_reverb_waves: too many samples for one call");
    // one input block: jobs | sentences | responses; one output block: r | e (whichever are asked for)
    const bool early = out_early != nullptr;
    Layout lay;
    lay.take(job.size() * sizeof(ReverbJob));
    const size_t o_pcm = lay.take((size_t)tot * 4), o_rir = lay.take((size_t)off[n_rir] * 4);
    const size_t in_b = lay.size(), sig_b = (size_t)tot * 4, out_b = sig_b * ((out_rev ? 1 : 0) + (early ? 1 : 0));
    OneShot os;
    if ((rc = os.open("bp_reverb_waves", device, in_b + out_b)) != BP_OK) return rc;
    std::vector<char> hb(in_b), ho(out_rev && early ? out_b : 0);
    memcpy(hb.data(), job.data(), job.size() * sizeof(ReverbJob));
    memcpy(hb.data() + o_pcm, pcm, sig_b);
    memcpy(hb.data() + o_rir, rir_pcm, (size_t)off[n_rir] * 4);
    hipError_t &e = os.e;
    char *d = os.d.as<char>();
    if (e == hipSuccess) e = hipMemcpyAsync(d, hb.data(), in_b, hipMemcpyHostToDevice, os.st);
    if (e == hipSuccess) {
        ReverbArgs a; memset(&a, 0, sizeof(a));
        a.job = (const ReverbJob *)d; a.n_job = n_sent; a.src = (const float *)(d + o_pcm); a.rir = (const float *)(d + o_rir);
        a.out_r = out_rev ? (float *)(d + in_b) : nullptr;
        a.out_e = early ? (float *)(d + in_b + (out_rev ? sig_b : 0)) : nullptr;
        e = reverb_launch(a, blocks, early, os.st);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(ho.empty() ? (char *)(out_rev ? out_rev : out_early) : ho.data(), d + in_b, out_b, hipMemcpyDeviceToHost, os.st);
    if ((rc = os.finish("bp_reverb_waves")) != BP_OK) return rc;
    if (!ho.empty()) { memcpy(out_rev, ho.data(), sig_b); memcpy(out_early, ho.data() + sig_b, sig_b); }
    return BP_OK;
}

// ------------------------------------------------------------------ simulated responses: host side
namespace {

bool rir_in(double v, double lo, double hi) { return std::isfinite(v) && v >= lo && v <= hi; }

// the checks of a room that do not depend on the response's length; d0 out
int rir_check_room(const std::string &who, const bp_rir_room &r, double &d0)
{
    for (int d = 0; d < 3; ++d) {
        if (!rir_in(r.L[d], 0.5, 100.0)) return fail(BP_ERR_ARG, who + ": L outside [0.5, 100] m");
        if (!(std::isfinite(r.src[d]) && r.src[d] > 0.0 && r.src[d] < r.L[d])) return fail(BP_ERR_ARG, who + ": the source is not strictly inside the box");
        if (!(std::isfinite(r.mic[d]) && r.mic[d] > 0.0 && r.mic[d] < r.L[d])) return fail(BP_ERR_ARG, who + ": the microphone is not strictly inside the box");
    }
    for (int w = 0; w < 6; ++w)
        if (!rir_in(r.beta[w], 0.0, 1.0)) return fail(BP_ERR_ARG, who + ": beta outside [0, 1]");
    const double dx = r.src[0] - r.mic[0], dy = r.src[1] - r.mic[1], dz = r.src[2] - r.mic[2];
    d0 = sqrt((dx * dx + dy * dy) + dz * dz);
    if (!(d0 >= 0.05)) return fail(BP_ERR_ARG, who + ": source and microphone are less than 0.05 m apart");
    return BP_OK;
}

int rir_check_rate(const char *who, int sample_rate, int window_taps)
{
    if (sample_rate < 1000 || sample_rate > 192000) return fail(BP_ERR_ARG, std::string(who) + ": sample_rate outside [1000, 192000]");
    if (window_taps < 2 || window_taps > 1024) return fail(BP_ERR_ARG, std::string(who) + ": window_taps outside [2, 1024]");
    return BP_OK;
}

// N_d = ceil(reach / (2 L_d)), reach = (n_taps + Tw/2) c / fs; returns the images of the box
int64_t rir_orders(const bp_rir_room &r, int sample_rate, int n_taps, int window_taps, int N[3])
{
    const double reach = (((double)n_taps + (double)window_taps / 2.0) * RIR_C) / (double)sample_rate;
    int64_t n = 8;
    for (int d = 0; d < 3; ++d) { N[d] = (int)ceil(reach / (2.0 * r.L[d])); n *= 2 * (int64_t)N[d] + 1; }
    return n;
}

// lo^|n-p| hi^|n| for n = -N .. N, p = 0, 1 at t[(n + N) 2 + p]: each power by repeated multiplication from 1.0
void rir_table(double lo, double hi, int N, double *t)
{
    std::vector<double> pl((size_t)N + 2), ph((size_t)N + 1);
    pl[0] = 1.0; ph[0] = 1.0;
    for (int k = 1; k <= N + 1; ++k) pl[k] = pl[k - 1] * lo;
    for (int k = 1; k <= N; ++k) ph[k] = ph[k - 1] * hi;
    for (int n = -N; n <= N; ++n)
        for (int p = 0; p < 2; ++p) t[(size_t)(n + N) * 2 + p] = pl[abs(n - p)] * ph[abs(n)];
}

}  // namespace

extern "C" int bp_rir_orders(const bp_rir_room *r, int sample_rate, int n_taps, int window_taps, int order[3], int64_t *n_images)
{
    if (!r || !order || !n_images) return fail(BP_ERR_ARG, "bp_rir_orders: null pointer");
    int rc;
    double d0;
    if ((rc = rir_check_rate("bp_rir_orders", sample_rate, window_taps)) != BP_OK) return rc;
    if (n_taps < 1 || n_taps > BP_MIX_RIR_MAX_TAPS) return fail(BP_ERR_ARG, "bp_rir_orders: length outside [1, " + std::to_string(BP_MIX_RIR_MAX_TAPS) + "]");
    if ((rc = rir_check_room("bp_rir_orders", *r, d0)) != BP_OK) return rc;
    *n_images = rir_orders(*r, sample_rate, n_taps, window_taps, order);
    return BP_OK;
}

extern "C" int bp_rir_beta(const double L[3], double t60, double beta[6])
{
    if (!L || !beta) return fail(BP_ERR_ARG, "bp_rir_beta: null pointer");
    for (int d = 0; d < 3; ++d)
        if (!rir_in(L[d], 0.5, 100.0)) return fail(BP_ERR_ARG, "bp_rir_beta: L outside [0.5, 100] m");
    if (!(std::isfinite(t60) && t60 > 0.0)) return fail(BP_ERR_ARG, "bp_rir_beta: t60 must be positive and finite");
    const double V = (L[0] * L[1]) * L[2], S = 2.0 * ((L[0] * L[1] + L[0] * L[2]) + L[1] * L[2]);
    const double k = (24.0 * log(10.0)) / RIR_C, alpha = 1.0 - exp(-((k * V) / (S * t60)));
    const double b = sqrt(1.0 - alpha);
    for (int w = 0; w < 6; ++w) beta[w] = b;
    return BP_OK;
}

extern "C" int bp_rir_rooms(uint64_t seed, int n, const bp_rir_range *g, bp_rir_room *out)
{
    if (!g || !out) return fail(BP_ERR_ARG, "bp_rir_rooms: null pointer");
    if (n < 1) return fail(BP_ERR_ARG, "bp_rir_rooms: need n >= 1");
    for (int d = 0; d < 3; ++d) {
        if (!(rir_in(g->L_lo[d], 0.5, 100.0) && rir_in(g->L_hi[d], 0.5, 100.0) && g->L_lo[d] <= g->L_hi[d]))
            return fail(BP_ERR_ARG, "bp_rir_rooms: need 0.5 <= L_lo <= L_hi <= 100 on every axis");
        if (!(std::isfinite(g->margin) && g->margin > 0.0 && 2.0 * g->margin < g->L_lo[d]))
            return fail(BP_ERR_ARG, "bp_rir_rooms: need margin > 0 and 2 margin < L_lo on every axis");
    }
    if (!(std::isfinite(g->t60_lo) && std::isfinite(g->t60_hi) && g->t60_lo > 0.0 && g->t60_lo <= g->t60_hi))
        return fail(BP_ERR_ARG, "bp_rir_rooms: need 0 < t60_lo <= t60_hi");
    if (!(std::isfinite(g->dist_lo) && std::isfinite(g->dist_hi) && g->dist_lo >= 0.05 && g->dist_lo <= g->dist_hi))
        return fail(BP_ERR_ARG, "bp_rir_rooms: need 0.05 <= dist_lo <= dist_hi");
    auto U = [seed](uint32_t r, uint32_t a, double u[4]) {
        uint32_t c[4] = {r, a, 4, 0};
        philox(c, seed);
        for (int i = 0; i < 4; ++i) u[i] = (double)c[i] / 4294967296.0;
    };
    for (int r = 0; r < n; ++r) {
        bp_rir_room &R = out[r];
        double u[4];
        U((uint32_t)r, 0, u);
        for (int d = 0; d < 3; ++d) R.L[d] = g->L_lo[d] + u[d] * (g->L_hi[d] - g->L_lo[d]);
        const double t60 = g->t60_lo + u[3] * (g->t60_hi - g->t60_lo);
        U((uint32_t)r, 1, u);
        for (int d = 0; d < 3; ++d) R.mic[d] = g->margin + u[d] * (R.L[d] - 2.0 * g->margin);
        bool found = false;
        for (uint32_t k = 0; k < 32 && !found; ++k) {
            U((uint32_t)r, 2 + k, u);
            for (int d = 0; d < 3; ++d) R.src[d] = g->margin + u[d] * (R.L[d] - 2.0 * g->margin);
            const double dx = R.src[0] - R.mic[0], dy = R.src[1] - R.mic[1], dz = R.src[2] - R.mic[2];
            const double dist = sqrt((dx * dx + dy * dy) + dz * dz);
            found = dist >= g->dist_lo && dist <= g->dist_hi;
        }
        if (!found) return fail(BP_ERR_ARG, "bp_rir_rooms: room " + std::to_string(r) + ": no source position in 32 attempts lies within [dist_lo, dist_hi] of the microphone");
        const int rc = bp_rir_beta(R.L, t60, R.beta);
        if (rc != BP_OK) return rc;
    }
    return BP_OK;
}

extern "C" int bp_rir_image(int device, int sample_rate, int window_taps, int n_rir, const bp_rir_room *rooms, const int *rir_len, float *out)
{
    if (!rooms || !rir_len || !out) return fail(BP_ERR_ARG, "bp_rir_image: null pointer");
    if (n_rir < 1) return fail(BP_ERR_ARG, "bp_rir_image: need at least one response");
    int rc;
    if ((rc = rir_check_rate("bp_rir_image", sample_rate, window_taps)) != BP_OK) return rc;
    std::vector<RirJob> job(n_rir);
    int64_t taps = 0, tab = 0, blk = 0;
    for (int k = 0; k < n_rir; ++k) {
        const std::string who = "bp_rir_image: response " + std::to_string(k);
        RirJob &j = job[k];
        memset(&j, 0, sizeof(j));
        if (rir_len[k] < 1 || rir_len[k] > BP_MIX_RIR_MAX_TAPS) return fail(BP_ERR_ARG, who + ": length outside [1, " + std::to_string(BP_MIX_RIR_MAX_TAPS) + "]");
        if ((rc = rir_check_room(who, rooms[k], j.d0)) != BP_OK) return rc;
        if (rir_orders(rooms[k], sample_rate, rir_len[k], window_taps, j.N) > BP_RIR_MAX_IMAGES)
            return fail(BP_ERR_ARG, who + ": more than " + std::to_string(BP_RIR_MAX_IMAGES) + " images (a shorter response or a larger room has fewer)");
        for (int d = 0; d < 3; ++d) { j.L[d] = rooms[k].L[d]; j.src[d] = rooms[k].src[d]; j.mic[d] = rooms[k].mic[d]; }
        j.tab = tab; j.out = taps; j.n_taps = rir_len[k]; j.blk0 = (int)blk;
        for (int d = 0; d < 3; ++d) tab += 2 * (2 * (int64_t)j.N[d] + 1);
        taps += rir_len[k]; blk += (rir_len[k] + RIR_BLOCK - 1) / RIR_BLOCK;
    }
    if (blk > INT32_MAX) return fail(BP_ERR_ARG, "bp_rir_image: too many taps for one call");
    // one input block: jobs | tables; one output block: the taps
    Layout lay;
    lay.take(job.size() * sizeof(RirJob));
    const size_t o_tab = lay.take((size_t)tab * 8), in_b = lay.size(), out_b = (size_t)taps * 4;
    std::vector<char> hb(in_b);
    memcpy(hb.data(), job.data(), job.size() * sizeof(RirJob));
    for (int k = 0; k < n_rir; ++k) {
        double *t = (double *)(hb.data() + o_tab) + job[k].tab;
        for (int d = 0; d < 3; ++d) { rir_table(rooms[k].beta[2 * d], rooms[k].beta[2 * d + 1], job[k].N[d], t); t += 2 * (2 * (size_t)job[k].N[d] + 1); }
    }
    OneShot os;
    if ((rc = os.open("bp_rir_image", device, in_b + out_b)) != BP_OK) return rc;
    hipError_t &e = os.e;
    char *d = os.d.as<char>();
    if (e == hipSuccess) e = hipMemcpyAsync(d, hb.data(), in_b, hipMemcpyHostToDevice, os.st);
    if (e == hipSuccess) {
        RirArgs a; memset(&a, 0, sizeof(a));
        a.job = (const RirJob *)d; a.n_job = n_rir; a.Tw = window_taps;
        a.fs_c = (double)sample_rate / RIR_C; a.inv_Tw = 1.0 / (double)window_taps;
        a.tab = (const double *)(d + o_tab); a.out = (float *)(d + in_b);
        bp_rir_image_taps<<<dim3((unsigned)blk), dim3(WAVE_THREADS), 0, os.st>>>(a);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, d + in_b, out_b, hipMemcpyDeviceToHost, os.st);
    return os.finish("bp_rir_image");
}
