// Verification statistics of generated fields against the truth, on the device.  Four HBM-bound reductions:
//   K41 error_stats     — one pass over gen [N][HW] and obs [No][HW]: per-pixel count / MAE / RMSE / bias over samples,
//                         per-sample count / MAE / RMSE over pixels, global count / means / bias / MAE / RMSE / min / max.
//   K42 histogram       — integer counts of x (or |x - ref|) in `bins` equal bins over [lo, hi] (floor rule, closed last bin).
//   K43 ensemble_scores — per-pixel ensemble mean, variance (ddof 1), fair CRPS and randomised rank of the truth among M
//                         members; rank histogram, mean fair / standard CRPS, skill, spread and spread/skill ratio.
//   K44 radial_spectrum — radially averaged power spectral density of |F|^2 fields (the FFT itself is torch.fft's).
// A pixel is valid when gen (every member, for K43) and obs are not NaN and the mask (uint8 != 0, or fp32 > 0.5) admits it.
// Reproducibility: float sums are fp64 per-wave partials that a finalize kernel adds in a fixed order (verify_common.h,
// block_sum_butterfly_waves); histograms are LDS-private integer bins flushed with one global integer atomic per non-empty
// bin per workgroup.  No float atomics.  The helpers shared with the other verify files are in verify_common.h.
// FP contraction is off in this file so that every statistic is the exact op sequence its numpy restatement performs.
#include <algorithm>
#include <cmath>

#include "kernels.h"
#include "philox.h"
#include "verify_common.h"

#pragma clang fp contract(off)

#define ST ((hipStream_t)stream)

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / SBGM_WAVE;
constexpr int kGlobFields = 9;               // per-wave error_stats partial: cnt, sum g, sum o, sum |d|, sum d^2, min/max g, min/max o
constexpr int kEnsFields = 5;                // per-wave ensemble partial: cnt, sum crps_fair, sum crps_std, sum (mean-y)^2, sum var
constexpr int kEnsChunk = 16;                // members held in registers per pass of the pairwise loop
constexpr int kMaxBins = 8192;               // LDS histogram: 32 KB of uint32
constexpr int kMaxSpectrumL = 2048;          // LDS: 4 wave rows of L/2+1 doubles

// 4 consecutive pixels [p0, p0+4) of one row of a [.][HW] array; out-of-range pixels read NaN.  VEC: HW % 4 == 0 and the
// base is 16-byte aligned, so one f32x4 load; otherwise scalar loads with the tail guarded.
template <bool VEC>
__device__ __forceinline__ f32x4 load_px4(const float* row, size_t p0, size_t HW) {
    if (VEC) return *reinterpret_cast<const f32x4*>(row + p0);
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (p0 + e < HW) ? row[p0 + e] : nan_f();
    return v;
}
template <bool VEC>
__device__ __forceinline__ void mask_px4(bool (&m)[4], const void* mask, int mask_u8, size_t off, size_t p0, size_t HW) {
    if (!mask) {
#pragma unroll
        for (int e = 0; e < 4; ++e) m[e] = p0 + e < HW;
        return;
    }
    if (VEC && mask_u8) {
        const uchar4 u = *reinterpret_cast<const uchar4*>(static_cast<const unsigned char*>(mask) + off + p0);
        m[0] = u.x != 0; m[1] = u.y != 0; m[2] = u.z != 0; m[3] = u.w != 0;
    } else if (VEC) {
        const f32x4 f = *reinterpret_cast<const f32x4*>(static_cast<const float*>(mask) + off + p0);
#pragma unroll
        for (int e = 0; e < 4; ++e) m[e] = f[e] > 0.5f;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) m[e] = (p0 + e < HW) && mask_at(mask, mask_u8, off + p0 + e);
    }
}

// ---- K41 error statistics ------------------------------------------------------------------------------------------------
// grid ceil(HW / 1024): one thread owns 4 consecutive pixels and walks the N samples; wave slot = blockIdx.x * 4 + wave.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void error_stats_kernel(const float* __restrict__ gen, const float* __restrict__ obs,
                                                               const void* __restrict__ mask, int mask_u8, int N, int obs_step,
                                                               int mask_step, size_t HW, int* __restrict__ pix_cnt,
                                                               float* __restrict__ pix_mae, float* __restrict__ pix_rmse,
                                                               float* __restrict__ pix_bias, double* __restrict__ smp_part,
                                                               double* __restrict__ glob_part) {
    const int lane = threadIdx.x & 63;
    const size_t slot = (size_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    const size_t p0 = ((size_t)blockIdx.x * kThreads + threadIdx.x) * 4;
    int cnt[4] = {0, 0, 0, 0};
    double sad[4] = {0, 0, 0, 0}, ssd[4] = {0, 0, 0, 0}, sg[4] = {0, 0, 0, 0}, so[4] = {0, 0, 0, 0};
    float gmin = INFINITY, gmax = -INFINITY, omin = INFINITY, omax = -INFINITY;
    for (int n = 0; n < N; ++n) {
        f32x4 g = {nan_f(), nan_f(), nan_f(), nan_f()}, o = g;
        bool m[4] = {false, false, false, false};
        if (p0 < HW) {
            g = load_px4<VEC>(gen + (size_t)n * HW, p0, HW);
            o = load_px4<VEC>(obs + (size_t)n * obs_step * HW, p0, HW);
            mask_px4<VEC>(m, mask, mask_u8, (size_t)n * mask_step * HW, p0, HW);
        }
        double c_n = 0.0, ad_n = 0.0, sd_n = 0.0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (!m[e] || is_nan(g[e]) || is_nan(o[e])) continue;
            const double d = (double)g[e] - (double)o[e];
            cnt[e] += 1;
            sad[e] += fabs(d);
            ssd[e] += d * d;
            sg[e] += (double)g[e];
            so[e] += (double)o[e];
            c_n += 1.0;
            ad_n += fabs(d);
            sd_n += d * d;
            gmin = fminf(gmin, g[e]); gmax = fmaxf(gmax, g[e]);
            omin = fminf(omin, o[e]); omax = fmaxf(omax, o[e]);
        }
        c_n = wave_sum_d(c_n);
        ad_n = wave_sum_d(ad_n);
        sd_n = wave_sum_d(sd_n);
        if (lane == 0) {
            double* q = smp_part + (slot * N + n) * 3;
            q[0] = c_n; q[1] = ad_n; q[2] = sd_n;
        }
    }
    double c = 0.0, a = 0.0, s = 0.0, gs = 0.0, os = 0.0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const size_t p = p0 + e;
        if (p < HW) {
            const int k = cnt[e];
            const double kd = (double)k;
            pix_cnt[p] = k;
            pix_mae[p] = k ? (float)(sad[e] / kd) : nan_f();
            pix_rmse[p] = k ? (float)sqrt(ssd[e] / kd) : nan_f();
            pix_bias[p] = k ? (float)(sg[e] / kd - so[e] / kd) : nan_f();
        }
        c += (double)cnt[e]; a += sad[e]; s += ssd[e]; gs += sg[e]; os += so[e];
    }
    c = wave_sum_d(c); a = wave_sum_d(a); s = wave_sum_d(s); gs = wave_sum_d(gs); os = wave_sum_d(os);
    gmin = wave_min(gmin); gmax = wave_max(gmax); omin = wave_min(omin); omax = wave_max(omax);
    if (lane == 0) {
        double* q = glob_part + slot * kGlobFields;
        q[0] = c; q[1] = gs; q[2] = os; q[3] = a; q[4] = s;
        q[5] = gmin; q[6] = gmax; q[7] = omin; q[8] = omax;
    }
}

// grid N + 1: block n < N adds sample n's wave partials in slot order; block N finishes the global statistics.
// sample_out [N][3] = (count, MAE, RMSE); global_out [10] = (count, mean gen, mean obs, bias, MAE, RMSE, min gen, max gen,
// min obs, max obs).  Empty sets give NaN.
__global__ __launch_bounds__(kThreads) void error_stats_finish_kernel(const double* __restrict__ smp_part,
                                                                      const double* __restrict__ glob_part, int N, int slots,
                                                                      double* __restrict__ sample_out, double* __restrict__ global_out) {
    __shared__ double sh[kWaves];
    const double nan = nan_d();
    if ((int)blockIdx.x < N) {
        const int n = blockIdx.x;
        double v[3] = {0, 0, 0};
        for (int s = threadIdx.x; s < slots; s += kThreads)
            for (int f = 0; f < 3; ++f) v[f] += smp_part[((size_t)s * N + n) * 3 + f];
        for (int f = 0; f < 3; ++f) v[f] = block_sum_butterfly_waves<kThreads>(v[f], sh);
        if (threadIdx.x == 0) {
            sample_out[n * 3 + 0] = v[0];
            sample_out[n * 3 + 1] = v[0] > 0 ? v[1] / v[0] : nan;
            sample_out[n * 3 + 2] = v[0] > 0 ? sqrt(v[2] / v[0]) : nan;
        }
        return;
    }
    double v[5] = {0, 0, 0, 0, 0};
    float mn[2] = {INFINITY, INFINITY}, mx[2] = {-INFINITY, -INFINITY};
    for (int s = threadIdx.x; s < slots; s += kThreads) {
        const double* q = glob_part + (size_t)s * kGlobFields;
        for (int f = 0; f < 5; ++f) v[f] += q[f];
        mn[0] = fminf(mn[0], (float)q[5]); mx[0] = fmaxf(mx[0], (float)q[6]);
        mn[1] = fminf(mn[1], (float)q[7]); mx[1] = fmaxf(mx[1], (float)q[8]);
    }
    for (int f = 0; f < 5; ++f) v[f] = block_sum_butterfly_waves<kThreads>(v[f], sh);
    __shared__ float shm[4][kWaves];
    const float r[4] = {wave_min(mn[0]), wave_max(mx[0]), wave_min(mn[1]), wave_max(mx[1])};
    if ((threadIdx.x & 63) == 0)
        for (int f = 0; f < 4; ++f) shm[f][threadIdx.x >> 6] = r[f];
    __syncthreads();
    if (threadIdx.x == 0) {
        float e[4] = {shm[0][0], shm[1][0], shm[2][0], shm[3][0]};
        for (int w = 1; w < kWaves; ++w) {
            e[0] = fminf(e[0], shm[0][w]); e[1] = fmaxf(e[1], shm[1][w]);
            e[2] = fminf(e[2], shm[2][w]); e[3] = fmaxf(e[3], shm[3][w]);
        }
        const bool any = v[0] > 0;
        const double mg = v[1] / v[0], mo = v[2] / v[0];
        global_out[0] = v[0];
        global_out[1] = any ? mg : nan;
        global_out[2] = any ? mo : nan;
        global_out[3] = any ? mg - mo : nan;
        global_out[4] = any ? v[3] / v[0] : nan;
        global_out[5] = any ? sqrt(v[4] / v[0]) : nan;
        for (int f = 0; f < 4; ++f) global_out[6 + f] = any ? (double)e[f] : nan;
    }
}

// ---- K42 histogram -------------------------------------------------------------------------------------------------------
// Bin rule (fp64, evaluated left to right): idx = floor(((double)v - lo) * bins / (hi - lo)); v is kept iff lo <= v <= hi,
// and idx is clamped to bins - 1 so that v == hi lands in the last bin.  This is numpy.histogram's range and closed-last-bin
// convention with the floor rule; numpy also corrects indices against its linspace edges, so for a value within rounding of
// an interior edge the two can differ by one bin (on exactly representable edges they agree).
__device__ __forceinline__ int hist_bin(float v, double lo, double hi, int bins) {
    const double x = (double)v;
    if (!(x >= lo && x <= hi)) return -1;                          // NaN fails both comparisons
    const int idx = (int)floor((x - lo) * (double)bins / (hi - lo));
    return idx < bins ? idx : bins - 1;
}

// grid (pixel blocks, N); dynamic LDS = bins * 4 bytes
__global__ __launch_bounds__(kThreads) void histogram_kernel(const float* __restrict__ x, const float* __restrict__ ref,
                                                             const void* __restrict__ mask, int mask_u8, int ref_step, int mask_step,
                                                             size_t HW, int absdiff, double lo, double hi, int bins,
                                                             unsigned long long* __restrict__ counts) {
    extern __shared__ unsigned int hbin[];
    for (int b = threadIdx.x; b < bins; b += kThreads) hbin[b] = 0;
    __syncthreads();
    const size_t n = blockIdx.y;
    const float* xr = x + n * HW;
    const float* rr = ref ? ref + n * ref_step * HW : nullptr;
    const size_t moff = n * mask_step * HW;
    for (size_t p = (size_t)blockIdx.x * kThreads + threadIdx.x; p < HW; p += (size_t)gridDim.x * kThreads) {
        float v = xr[p];
        if (rr) {
            const float r = rr[p];
            if (is_nan(r)) continue;
            if (absdiff) v = fabsf(v - r);
        }
        if (!mask_at(mask, mask_u8, moff + p)) continue;
        const int b = hist_bin(v, lo, hi, bins);
        if (b >= 0) atomicAdd(&hbin[b], 1u);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < bins; b += kThreads)
        if (hbin[b]) atomicAdd(&counts[b], (unsigned long long)hbin[b]);
}

// ---- K43 ensemble scores -------------------------------------------------------------------------------------------------
// grid ceil(HW / 256), one lane per pixel, members read coalesced ([M][HW] rows).  The pairwise CRPS term is the O(M^2) sum
// sum_ij |x_i - x_j| over all ordered pairs: kEnsChunk members of the lane's pixel sit in registers while all M members stream
// past (from L2 after the first pass), so HBM sees each member once and the cache M / kEnsChunk times.  The same loop gives
// sum_ij (x_i - x_j)^2 = 2 M sum_i (x_i - mean)^2, the variance without cancellation.  Differences of two fp32 values are
// exact in fp64, so only the fp64 accumulation rounds.  Dynamic LDS = (M + 1) * 4 bytes (rank histogram).
__global__ __launch_bounds__(kThreads) void ensemble_kernel(const float* __restrict__ ens, const float* __restrict__ obs,
                                                            const void* __restrict__ mask, int mask_u8, int M, size_t HW,
                                                            unsigned long long seed, float* __restrict__ mean_out,
                                                            float* __restrict__ var_out, float* __restrict__ crps_out,
                                                            int* __restrict__ rank_out, double* __restrict__ part,
                                                            unsigned long long* __restrict__ rank_hist) {
    extern __shared__ unsigned int rbin[];
    for (int b = threadIdx.x; b <= M; b += kThreads) rbin[b] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const size_t slot = (size_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    const size_t p = (size_t)blockIdx.x * kThreads + threadIdx.x;
    const bool inb = p < HW;
    const float y = inb ? obs[p] : nan_f();
    bool valid = inb && !is_nan(y) && mask_at(mask, mask_u8, p);
    const double yd = (double)y;
    double sx = 0.0, sad = 0.0, spair = 0.0, spair2 = 0.0;
    int lt = 0, le = 0;
    for (int i0 = 0; i0 < M && valid; i0 += kEnsChunk) {
        const int nk = min(kEnsChunk, M - i0);
        double xi[kEnsChunk];
#pragma unroll
        for (int k = 0; k < kEnsChunk; ++k) {
            xi[k] = 0.0;
            if (k < nk) {
                const float v = ens[(size_t)(i0 + k) * HW + p];
                valid = valid && !is_nan(v);
                xi[k] = (double)v;
                sx += (double)v;
                sad += fabs((double)v - yd);
                lt += v < y;
                le += v <= y;
            }
        }
        if (!valid) break;
        for (int j = 0; j < M; ++j) {
            const double xj = (double)ens[(size_t)j * HW + p];
#pragma unroll
            for (int k = 0; k < kEnsChunk; ++k) {
                if (k < nk) {
                    const double d = xi[k] - xj;
                    spair += fabs(d);
                    spair2 += d * d;
                }
            }
        }
    }
    const double Md = (double)M;
    double c = 0.0, cf = 0.0, cs = 0.0, se = 0.0, vv = 0.0;
    if (valid) {
        const double mean = sx / Md;
        const double var = spair2 / (2.0 * Md * (Md - 1.0));
        const double crps_fair = sad / Md - spair / (2.0 * Md * (Md - 1.0));
        const double crps_std = sad / Md - spair / (2.0 * Md * Md);
        // ties broken at random: rank ~ U{lt, ..., le}, one Philox draw keyed by (seed, pixel)
        const float u = philox_uniform4(seed, 0ull, (unsigned long long)p)[0];
        const int r = min(le, lt + (int)floorf(u * (float)(le - lt + 1)));
        mean_out[p] = (float)mean;
        var_out[p] = (float)var;
        crps_out[p] = (float)crps_fair;
        rank_out[p] = r;
        atomicAdd(&rbin[r], 1u);
        c = 1.0; cf = crps_fair; cs = crps_std; se = (mean - yd) * (mean - yd); vv = var;
    } else if (inb) {
        mean_out[p] = nan_f();
        var_out[p] = nan_f();
        crps_out[p] = nan_f();
        rank_out[p] = -1;
    }
    c = wave_sum_d(c); cf = wave_sum_d(cf); cs = wave_sum_d(cs); se = wave_sum_d(se); vv = wave_sum_d(vv);
    if (lane == 0) {
        double* q = part + slot * kEnsFields;
        q[0] = c; q[1] = cf; q[2] = cs; q[3] = se; q[4] = vv;
    }
    __syncthreads();
    for (int b = threadIdx.x; b <= M; b += kThreads)
        if (rbin[b]) atomicAdd(&rank_hist[b], (unsigned long long)rbin[b]);
}

// one block: scores [6] = (count, mean fair CRPS, mean standard CRPS, skill = RMSE of the ensemble mean,
// spread = sqrt(mean variance), spread/skill * sqrt((M+1)/M))
__global__ __launch_bounds__(kThreads) void ensemble_finish_kernel(const double* __restrict__ part, int slots, int M,
                                                                   double* __restrict__ scores) {
    __shared__ double sh[kWaves];
    double v[kEnsFields] = {0, 0, 0, 0, 0};
    for (int s = threadIdx.x; s < slots; s += kThreads)
        for (int f = 0; f < kEnsFields; ++f) v[f] += part[(size_t)s * kEnsFields + f];
    for (int f = 0; f < kEnsFields; ++f) v[f] = block_sum_butterfly_waves<kThreads>(v[f], sh);
    if (threadIdx.x == 0) {
        const double nan = nan_d();
        const bool any = v[0] > 0;
        const double skill = sqrt(v[3] / v[0]), spread = sqrt(v[4] / v[0]);
        scores[0] = v[0];
        scores[1] = any ? v[1] / v[0] : nan;
        scores[2] = any ? v[2] / v[0] : nan;
        scores[3] = any ? skill : nan;
        scores[4] = any ? spread : nan;
        scores[5] = any ? sqrt(((double)M + 1.0) / (double)M) * spread / skill : nan;
    }
}

// ---- K44 radial spectrum -------------------------------------------------------------------------------------------------
// wavenumber of pixel (iy, ix): k = rint(L * sqrt(fy^2 + fx^2)), f = numpy.fft.fftfreq (index * (1.0 / n)); -1 = corner (k > L/2)
__device__ __forceinline__ int spectrum_bin(int iy, int ix, int H, int W, int L) {
    const double fy = (double)(iy < (H + 1) / 2 ? iy : iy - H) * (1.0 / (double)H);
    const double fx = (double)(ix < (W + 1) / 2 ? ix : ix - W) * (1.0 / (double)W);
    const int k = (int)rint((double)L * sqrt(fy * fy + fx * fx));
    return k <= L / 2 ? k : -1;
}

// grid nblk (fixed for a shape); each lane sums its pixel's power over the valid fields in field order, then lane 0 of each
// wave adds the 64 lanes' sums, broadcast one by one, into the wave's private LDS bins (a fixed order, no float atomics); the 4 wave rows are added
// in order into the block's partial row.  Dynamic LDS = 4 * nb doubles + nb uint32 (pixel counts).
__global__ __launch_bounds__(kThreads) void spectrum_kernel(const float* __restrict__ power, const unsigned char* __restrict__ field_ok,
                                                            int F, int H, int W, int nb, double* __restrict__ part,
                                                            unsigned long long* __restrict__ bin_count) {
    extern __shared__ double wbins[];
    unsigned int* cbins = reinterpret_cast<unsigned int*>(wbins + (size_t)kWaves * nb);
    for (int b = threadIdx.x; b < kWaves * nb; b += kThreads) wbins[b] = 0.0;
    for (int b = threadIdx.x; b < nb; b += kThreads) cbins[b] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    double* mine = wbins + (size_t)(threadIdx.x >> 6) * nb;
    const size_t HW = (size_t)H * W;
    const int L = max(H, W);
    for (size_t base = (size_t)blockIdx.x * kThreads; base < HW; base += (size_t)gridDim.x * kThreads) {
        const size_t p = base + threadIdx.x;
        int k = -1;
        double acc = 0.0;
        if (p < HW) {
            k = spectrum_bin((int)(p / W), (int)(p % W), H, W, L);
            if (k >= 0) {
                for (int f = 0; f < F; ++f)
                    if (field_ok[f]) acc += (double)power[(size_t)f * HW + p];
                atomicAdd(&cbins[k], 1u);
            }
        }
        // lane 0 adds the wave's 64 (bin, power) pairs itself, in lane order.  These are one thread's sequential
        // read-modify-writes, so single-thread semantics fix their count and order; nothing depends on how the compiler
        // treats 64 divergent lanes each guarding its own update.
        for (int l = 0; l < 64; ++l) {
            const int kl = __shfl(k, l, 64);
            const double al = __shfl(acc, l, 64);
            if (lane == 0 && kl >= 0) mine[kl] += al;
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < nb; b += kThreads) {
        double s = 0.0;
        for (int w = 0; w < kWaves; ++w) s += wbins[(size_t)w * nb + b];
        part[(size_t)blockIdx.x * nb + b] = s;
        if (cbins[b]) atomicAdd(&bin_count[b], (unsigned long long)cbins[b]);
    }
}

// one block: psd[k] = (sum over blocks in order) / (pixels in bin k * valid fields); n_fields[0] = valid fields
__global__ __launch_bounds__(kThreads) void spectrum_finish_kernel(const double* __restrict__ part, const unsigned char* __restrict__ field_ok,
                                                                   int F, int nb, int nblk,
                                                                   const unsigned long long* __restrict__ bin_count,
                                                                   double* __restrict__ psd, long long* __restrict__ n_fields) {
    int nv = 0;
    for (int f = 0; f < F; ++f) nv += field_ok[f] != 0;
    for (int b = threadIdx.x; b < nb; b += kThreads) {
        double s = 0.0;
        for (int k = 0; k < nblk; ++k) s += part[(size_t)k * nb + b];
        const double denom = (double)bin_count[b] * (double)nv;
        psd[b] = denom > 0 ? s / denom : nan_d();
    }
    if (threadIdx.x == 0) n_fields[0] = nv;
}

inline int err_blocks(int64_t HW) { return (int)((HW + 4 * kThreads - 1) / (4 * kThreads)); }
inline int ens_blocks(int64_t HW) { return (int)((HW + kThreads - 1) / kThreads); }
inline int spec_blocks(int64_t HW) { return (int)std::min<int64_t>((HW + kThreads - 1) / kThreads, 256); }

bool aligned16(const void* p) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" {

int64_t sbgm_error_stats_workspace_bytes(int N, int64_t HW) {
    if (N < 1 || HW < 1) return 0;
    const int64_t slots = (int64_t)err_blocks(HW) * kWaves;
    return slots * ((int64_t)N * 3 + kGlobFields) * (int64_t)sizeof(double);
}

int sbgm_error_stats(const float* gen, const float* obs, const void* mask, int mask_is_u8, int N, int No, int Nm, int64_t HW,
                     int* pix_count, float* pix_mae, float* pix_rmse, float* pix_bias, double* sample_stats, double* global_stats,
                     void* workspace, void* stream) {
    SBGM_CHECK(gen && obs && pix_count && pix_mae && pix_rmse && pix_bias && sample_stats && global_stats && workspace,
               "error_stats: null argument");
    SBGM_CHECK(N >= 1 && HW >= 1 && HW < (1ll << 31), "error_stats: N=%d HW=%lld", N, (long long)HW);
    SBGM_CHECK(No == 1 || No == N, "error_stats: obs has %d samples; need 1 or N=%d", No, N);
    SBGM_CHECK(!mask || Nm == 1 || Nm == N, "error_stats: mask has %d samples; need 1 or N=%d", Nm, N);
    const int nblk = err_blocks(HW), slots = nblk * kWaves;
    double* smp_part = static_cast<double*>(workspace);
    double* glob_part = smp_part + (size_t)slots * N * 3;
    const bool vec = HW % 4 == 0 && aligned16(gen) && aligned16(obs) &&
                     (!mask || (mask_is_u8 ? (reinterpret_cast<uintptr_t>(mask) & 3) == 0 : aligned16(mask)));
    const int os = No == 1 ? 0 : 1, ms = Nm == 1 ? 0 : 1;
    if (vec)
        hipLaunchKernelGGL(error_stats_kernel<true>, dim3(nblk), dim3(kThreads), 0, ST, gen, obs, mask, mask_is_u8, N, os, ms,
                           (size_t)HW, pix_count, pix_mae, pix_rmse, pix_bias, smp_part, glob_part);
    else
        hipLaunchKernelGGL(error_stats_kernel<false>, dim3(nblk), dim3(kThreads), 0, ST, gen, obs, mask, mask_is_u8, N, os, ms,
                           (size_t)HW, pix_count, pix_mae, pix_rmse, pix_bias, smp_part, glob_part);
    SBGM_LAUNCH_CHECK();
    hipLaunchKernelGGL(error_stats_finish_kernel, dim3(N + 1), dim3(kThreads), 0, ST, smp_part, glob_part, N, slots, sample_stats,
                       global_stats);
    SBGM_LAUNCH_CHECK();
    return 0;
}

int sbgm_histogram(const float* x, const float* ref, const void* mask, int mask_is_u8, int N, int Nr, int Nm, int64_t HW,
                   int absdiff, double lo, double hi, int bins, int64_t* counts, void* stream) {
    SBGM_CHECK(x && counts, "histogram: null argument");
    SBGM_CHECK(N >= 1 && N <= 65535 && HW >= 1, "histogram: N=%d HW=%lld", N, (long long)HW);
    SBGM_CHECK(bins >= 1 && bins <= kMaxBins, "histogram: bins=%d (1..%d)", bins, kMaxBins);
    SBGM_CHECK(std::isfinite(lo) && std::isfinite(hi) && hi > lo, "histogram: range [%g, %g]", lo, hi);
    SBGM_CHECK(!ref || Nr == 1 || Nr == N, "histogram: ref has %d samples; need 1 or N=%d", Nr, N);
    SBGM_CHECK(!mask || Nm == 1 || Nm == N, "histogram: mask has %d samples; need 1 or N=%d", Nm, N);
    SBGM_CHECK(!absdiff || ref, "histogram: absdiff needs ref");
    if (int rc = sbgm_zero_async(counts, (size_t)bins * sizeof(int64_t), ST)) return rc;
    const int bx = (int)std::min<int64_t>((HW + 4 * kThreads - 1) / (4 * kThreads), 256);
    hipLaunchKernelGGL(histogram_kernel, dim3(bx, N), dim3(kThreads), (size_t)bins * sizeof(unsigned int), ST, x, ref, mask,
                       mask_is_u8, Nr == 1 ? 0 : 1, Nm == 1 ? 0 : 1, (size_t)HW, absdiff, lo, hi, bins,
                       reinterpret_cast<unsigned long long*>(counts));
    SBGM_LAUNCH_CHECK();
    return 0;
}

int64_t sbgm_ensemble_scores_workspace_bytes(int64_t HW) {
    return HW < 1 ? 0 : (int64_t)ens_blocks(HW) * kWaves * kEnsFields * (int64_t)sizeof(double);
}

int sbgm_ensemble_scores(const float* ens, const float* obs, const void* mask, int mask_is_u8, int M, int64_t HW,
                         uint64_t seed, float* mean, float* var, float* crps, int* rank, int64_t* rank_hist, double* scores,
                         void* workspace, void* stream) {
    SBGM_CHECK(ens && obs && mean && var && crps && rank && rank_hist && scores && workspace, "ensemble_scores: null argument");
    SBGM_CHECK(M >= 2 && M <= kMaxBins - 1, "ensemble_scores: M=%d members (2..%d)", M, kMaxBins - 1);
    SBGM_CHECK(HW >= 1 && HW < (1ll << 31), "ensemble_scores: HW=%lld", (long long)HW);
    if (int rc = sbgm_zero_async(rank_hist, (size_t)(M + 1) * sizeof(int64_t), ST)) return rc;
    const int nblk = ens_blocks(HW);
    double* part = static_cast<double*>(workspace);
    hipLaunchKernelGGL(ensemble_kernel, dim3(nblk), dim3(kThreads), (size_t)(M + 1) * sizeof(unsigned int), ST, ens, obs, mask,
                       mask_is_u8, M, (size_t)HW, (unsigned long long)seed, mean, var, crps, rank, part,
                       reinterpret_cast<unsigned long long*>(rank_hist));
    SBGM_LAUNCH_CHECK();
    hipLaunchKernelGGL(ensemble_finish_kernel, dim3(1), dim3(kThreads), 0, ST, part, nblk * kWaves, M, scores);
    SBGM_LAUNCH_CHECK();
    return 0;
}

int64_t sbgm_radial_spectrum_workspace_bytes(int H, int W) {
    if (H < 1 || W < 1) return 0;
    return (int64_t)spec_blocks((int64_t)H * W) * (std::max(H, W) / 2 + 1) * (int64_t)sizeof(double);
}

int sbgm_radial_spectrum(const float* power, const unsigned char* field_ok, int F, int H, int W, double* psd, int64_t* bin_count,
                         int64_t* n_fields, void* workspace, void* stream) {
    SBGM_CHECK(power && field_ok && psd && bin_count && n_fields && workspace, "radial_spectrum: null argument");
    SBGM_CHECK(F >= 1 && H >= 2 && W >= 2 && std::max(H, W) <= kMaxSpectrumL, "radial_spectrum: F=%d H=%d W=%d (sides 2..%d)", F, H,
               W, kMaxSpectrumL);
    const int nb = std::max(H, W) / 2 + 1, nblk = spec_blocks((int64_t)H * W);
    if (int rc = sbgm_zero_async(bin_count, (size_t)nb * sizeof(int64_t), ST)) return rc;
    double* part = static_cast<double*>(workspace);
    const size_t lds = (size_t)kWaves * nb * sizeof(double) + (size_t)nb * sizeof(unsigned int);
    hipLaunchKernelGGL(spectrum_kernel, dim3(nblk), dim3(kThreads), lds, ST, power, field_ok, F, H, W, nb, part,
                       reinterpret_cast<unsigned long long*>(bin_count));
    SBGM_LAUNCH_CHECK();
    hipLaunchKernelGGL(spectrum_finish_kernel, dim3(1), dim3(kThreads), 0, ST, part, field_ok, F, nb, nblk,
                       reinterpret_cast<const unsigned long long*>(bin_count), psd, reinterpret_cast<long long*>(n_fields));
    SBGM_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
