// Pooled ensemble verification of a series on the device: D days of M members E[d][m][p] against one truth
// Y[d][p] per day, pooled over days x pixels, for all days (row 0 of every [G+1] axis) and per group of days (row 1 + g).
//   K58 series_cells     — one lane per pixel walks the days of a chunk in day order.  Per valid cell K43's expressions (mean,
//                          var, fair and standard CRPS, squared error) in K43's op order; the per-pixel sums of crps_fair, var
//                          and se run in fp64 in that one thread, across chunks through the workspace, and become the four maps
//                          after the last day.  Per day it leaves per-wave partials of the five pooled sums, the validity bits
//                          (one uint32 per 32 days and pixel, as K55) and, for the climatology, the per-group sums of crps_fair.
//        series_daily    — adds a day's wave partials in slot order: `daily`, and the day's raw sums for `scores`.
//        series_rows     — a row's raw sums over its days: `scores`.
//   K59 series_counts    — the integer statistics: the randomised rank of the truth (K43's draw, keyed by (seed, day, pixel)) and
//                          K46's table, binned in LDS for one row at a time and flushed with 64-bit integer atomics when the
//                          row changes.  Integer sums do not depend on their order, so this kernel splits days, pixels and
//                          thresholds over the grid freely.  Validity comes from K58's bits.  With groups it fills the group rows
//                          and series_row0 adds them into row 0; K46's finish formulas then run per row.
//   K60 series_climatology — the leave-one-out climatological reference.  Per pixel and row S = sum over ordered pairs of valid
//                          days |y_i - y_j| by K43's form: 16 days in registers while the later days stream past (each unordered
//                          pair once, doubled at the end; differences of fp32 values are exact in fp64), O(n^2).  Then
//                          C = S / (2 (n - 1)), the maps and per-wave partials of (cells, F, C) over the pixels with n >= 3.
//        series_skill    — adds those partials in slot order: `skill_scores`.
// Lanes map to pixels, so every day row and member row is read coalesced.  Reproducibility: no float atomics; every fp64 sum
// has a fixed order that does not depend on how the days are chunked over the workspace.
// FP contraction is off in this file: the fp64 expressions are the op sequences of the numpy restatement
// (tests/series_scores_ref.py).
#include "philox.h"
#include "verify_common.h"

#pragma clang fp contract(off)

#define ST ((hipStream_t)stream)

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / SBGM_WAVE;
constexpr int kMaxDays = SBGM_TEMPORAL_MAX_DAYS;
constexpr int kMaxGroups = SBGM_SERIES_MAX_GROUPS;
constexpr int kSums = 5;                     // pooled sums of a set of cells: cnt, crps_fair, crps_std, (mean - y)^2, var
constexpr int kEnsChunk = 16;                // K43's: members held in registers per pass of the pairwise loop
constexpr int kDayChunk = 16;                // K60: days held in registers per pass of the pairwise loop
constexpr int kChunkDays = 32;               // the days of a workspace chunk are a multiple of this: a word of validity bits
constexpr int kCountDays = 64;               // K59: days per workgroup
constexpr int kCountMaxBlocks = 512;
constexpr int kCountLdsBytes = 49152;        // K59: (M + 1) * 4 bytes for the ranks and (M + 1) * 8 per threshold

// a group id as the kernels use it: ids outside 0..G-1 are the caller's error, but nothing is ever written out of bounds
__device__ __forceinline__ int group_at(const int* __restrict__ groups, int d, int G) { return min(max(groups[d], 0), G - 1); }

// scores [6] of ENSEMBLE_KEYS from the five pooled sums: K43's finish
__device__ __forceinline__ void scores_from_sums(const double* v, int M, double* scores) {
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

// ---- K58 ----------------------------------------------------------------------------------------------------------------------
// grid ceil(HW / 256); days [d0, d1) with d0 a multiple of 32.  state [3][HW] carries the per-pixel sums from chunk to chunk
// (and count the valid days); fgroup [G][HW] the per-group sums of crps_fair (group_sums != 0 only), which the lane keeps in a
// register while the group stays the same.  part [d1 - d0][slots][5], slots = 4 * gridDim.x.
__global__ __launch_bounds__(kThreads) void series_cells_kernel(
    const float* __restrict__ ens, long long day_stride, long long member_stride, const float* __restrict__ obs,
    const void* __restrict__ mask, int mask_u8, int mask_daily, const int* __restrict__ groups, int G, int group_sums, int D, int M,
    size_t HW, int d0, int d1, int* __restrict__ count, float* __restrict__ maps, double* __restrict__ state,
    double* __restrict__ fgroup, unsigned int* __restrict__ vbits, double* __restrict__ part) {
    const int lane = threadIdx.x & 63;
    const size_t slots = (size_t)gridDim.x * kWaves, slot = (size_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    const size_t p = (size_t)blockIdx.x * kThreads + threadIdx.x;
    const bool inb = p < HW;
    const bool admitted = inb && (mask_daily || mask_at(mask, mask_u8, p));
    int n = 0;
    double sum_crps = 0.0, sum_var = 0.0, sum_se = 0.0;
    if (inb && d0 > 0) {
        n = count[p];
        sum_crps = state[p];
        sum_var = state[HW + p];
        sum_se = state[2 * HW + p];
    }
    int cur = -1;
    double gacc = 0.0;
    unsigned int bits = 0u;
    const double Md = (double)M;
    for (int d = d0; d < d1; ++d) {
        const size_t i = (size_t)d * HW + p;
        const float y = admitted ? obs[i] : nan_f();
        bool valid = admitted && !is_nan(y) && (!mask_daily || mask_at(mask, mask_u8, i));
        const float* e = ens + (size_t)d * (size_t)day_stride + p;
        const double yd = (double)y;
        double sx = 0.0, sad = 0.0, spair = 0.0, spair2 = 0.0;
        for (int i0 = 0; i0 < M && valid; i0 += kEnsChunk) {
            const int nk = min(kEnsChunk, M - i0);
            double xi[kEnsChunk];
#pragma unroll
            for (int k = 0; k < kEnsChunk; ++k) {
                xi[k] = 0.0;
                if (k < nk) {
                    const float v = e[(size_t)(i0 + k) * (size_t)member_stride];
                    valid = valid && !is_nan(v);
                    xi[k] = (double)v;
                    sx += (double)v;
                    sad += fabs((double)v - yd);
                }
            }
            if (!valid) break;
            for (int j = 0; j < M; ++j) {
                const double xj = (double)e[(size_t)j * (size_t)member_stride];
#pragma unroll
                for (int k = 0; k < kEnsChunk; ++k) {
                    if (k < nk) {
                        const double dd = xi[k] - xj;
                        spair += fabs(dd);
                        spair2 += dd * dd;
                    }
                }
            }
        }
        double c = 0.0, cf = 0.0, cs = 0.0, se = 0.0, vv = 0.0;
        if (valid) {
            const double mean = sx / Md;
            const double var = spair2 / (2.0 * Md * (Md - 1.0));
            const double crps_fair = sad / Md - spair / (2.0 * Md * (Md - 1.0));
            const double crps_std = sad / Md - spair / (2.0 * Md * Md);
            c = 1.0; cf = crps_fair; cs = crps_std; se = (mean - yd) * (mean - yd); vv = var;
            ++n;
            sum_crps += cf;
            sum_var += vv;
            sum_se += se;
        }
        if (group_sums) {
            const int g = group_at(groups, d, G);
            if (g != cur) {                                               // the same in every lane: d is
                if (inb) {
                    if (cur >= 0) fgroup[(size_t)cur * HW + p] = gacc;
                    gacc = fgroup[(size_t)g * HW + p];
                }
                cur = g;
            }
            if (valid) gacc += cf;
        }
        bits |= (unsigned int)valid << (d & 31);
        if ((d & 31) == 31 || d == d1 - 1) {
            if (inb) vbits[(size_t)(d >> 5) * HW + p] = bits;
            bits = 0u;
        }
        c = wave_sum_d(c); cf = wave_sum_d(cf); cs = wave_sum_d(cs); se = wave_sum_d(se); vv = wave_sum_d(vv);
        if (lane == 0) {
            double* q = part + ((size_t)(d - d0) * slots + slot) * kSums;
            q[0] = c; q[1] = cf; q[2] = cs; q[3] = se; q[4] = vv;
        }
    }
    if (!inb) return;
    if (group_sums && cur >= 0) fgroup[(size_t)cur * HW + p] = gacc;
    count[p] = n;
    state[p] = sum_crps;
    state[HW + p] = sum_var;
    state[2 * HW + p] = sum_se;
    if (d1 == D) {
        const double nd = (double)n;
        const double spread = sqrt(sum_var / nd), skill = sqrt(sum_se / nd);
        maps[p] = n > 0 ? (float)(sum_crps / nd) : nan_f();
        maps[HW + p] = n > 0 ? (float)spread : nan_f();
        maps[2 * HW + p] = n > 0 ? (float)skill : nan_f();
        maps[3 * HW + p] = n > 0 ? (float)(sqrt((Md + 1.0) / Md) * spread / skill) : nan_f();
    }
}

// grid d1 - d0: block b adds the slots of day d0 + b in slot order ("butterfly, then wave partials in index order")
__global__ __launch_bounds__(kThreads) void series_daily_kernel(const double* __restrict__ part, int slots, int M, int d0,
                                                                double* __restrict__ day_sums, double* __restrict__ daily) {
    __shared__ double sh[kWaves];
    const int d = d0 + blockIdx.x;
    const double* q = part + (size_t)blockIdx.x * slots * kSums;
    double v[kSums] = {0, 0, 0, 0, 0};
    for (int s = threadIdx.x; s < slots; s += kThreads)
        for (int f = 0; f < kSums; ++f) v[f] += q[(size_t)s * kSums + f];
    for (int f = 0; f < kSums; ++f) v[f] = block_sum_butterfly_waves<kThreads>(v[f], sh);
    if (threadIdx.x == 0) {
        for (int f = 0; f < kSums; ++f) day_sums[(size_t)d * kSums + f] = v[f];
        scores_from_sums(v, M, daily + (size_t)d * 6);
    }
}

// grid G + 1: block r adds the day sums of row r's days, thread t taking the days t, t + 256, ... in day order
__global__ __launch_bounds__(kThreads) void series_rows_kernel(const double* __restrict__ day_sums, const int* __restrict__ groups,
                                                               int G, int D, int M, double* __restrict__ scores) {
    __shared__ double sh[kWaves];
    const int row = blockIdx.x;
    double v[kSums] = {0, 0, 0, 0, 0};
    for (int d = threadIdx.x; d < D; d += kThreads)
        if (row == 0 || group_at(groups, d, G) == row - 1)
            for (int f = 0; f < kSums; ++f) v[f] += day_sums[(size_t)d * kSums + f];
    for (int f = 0; f < kSums; ++f) v[f] = block_sum_butterfly_waves<kThreads>(v[f], sh);
    if (threadIdx.x == 0) scores_from_sums(v, M, scores + (size_t)row * 6);
}

// ---- K59 ----------------------------------------------------------------------------------------------------------------------
// grid (pixel blocks, threshold groups of tg, ceil(D / 64)); lane = pixel (grid-stride).  LDS: (M + 1) uint32 rank bins (used by
// threshold group 0), then tg tables [M + 1][2].  Every lane of the workgroup walks the same days, so the row of the bins is
// the same for all of them and the flush sits between two barriers.  Dynamic LDS = (M + 1) * (4 + 8 * tg) bytes.
__global__ __launch_bounds__(kThreads) void series_counts_kernel(
    const float* __restrict__ ens, long long day_stride, long long member_stride, const float* __restrict__ obs,
    const unsigned int* __restrict__ vbits, const int* __restrict__ groups, int G, int D, int M, size_t HW, int T, int tg,
    ThrList thr, unsigned long long seed, unsigned long long* __restrict__ rank_hist, unsigned long long* __restrict__ table) {
    extern __shared__ unsigned int bins[];
    const int t0 = blockIdx.y * tg, nt = T > 0 ? min(tg, T - t0) : 0;
    const bool ranks = blockIdx.y == 0;
    const int nb = (M + 1) * (1 + 2 * nt);
    unsigned int* tbins = bins + (M + 1);
    for (int b = threadIdx.x; b < nb; b += kThreads) bins[b] = 0;
    float th[kMaxThr];
#pragma unroll
    for (int t = 0; t < kMaxThr; ++t) th[t] = thr.v[min(t0 + t, max(T - 1, 0))];
    const int da = blockIdx.z * kCountDays, db = min(D, da + kCountDays);
    int cur = -1;                                                         // the row whose counts the bins hold
    for (size_t base = (size_t)blockIdx.x * kThreads; base < HW; base += (size_t)gridDim.x * kThreads) {
        const size_t p = base + threadIdx.x;
        const bool inb = p < HW;
        unsigned int word = 0u;
        for (int d = da; d < db; ++d) {
            const int row = G > 0 ? 1 + group_at(groups, d, G) : 0;
            if (row != cur) {
                __syncthreads();
                if (cur >= 0) {
                    unsigned long long* rh = rank_hist + (size_t)cur * (M + 1);
                    unsigned long long* tb = table + ((size_t)cur * T + t0) * (M + 1) * 2;
                    for (int b = threadIdx.x; b < nb; b += kThreads) {
                        if (bins[b]) atomicAdd(b <= M ? &rh[b] : &tb[b - (M + 1)], (unsigned long long)bins[b]);
                        bins[b] = 0;
                    }
                }
                __syncthreads();
                cur = row;
            }
            if (d == da || (d & 31) == 0) word = inb ? vbits[(size_t)(d >> 5) * HW + p] : 0u;
            if (!((word >> (d & 31)) & 1u)) continue;                     // no barrier below: the lanes meet again at the next day
            const float y = obs[(size_t)d * HW + p];
            const float* e = ens + (size_t)d * (size_t)day_stride + p;
            int k[kMaxThr];
#pragma unroll
            for (int t = 0; t < kMaxThr; ++t) k[t] = 0;
            int lt = 0, le = 0;
            for (int m = 0; m < M; ++m) {
                const float v = e[(size_t)m * (size_t)member_stride];
                lt += v < y;
                le += v <= y;
#pragma unroll
                for (int t = 0; t < kMaxThr; ++t) k[t] += v >= th[t];
            }
            if (ranks) {
                // ties broken at random: rank ~ U{lt, ..., le}, one Philox draw keyed by (seed, day, pixel)
                const float u = philox_uniform4(seed, (unsigned long long)d, (unsigned long long)p)[0];
                atomicAdd(&bins[min(le, lt + (int)floorf(u * (float)(le - lt + 1)))], 1u);
            }
#pragma unroll
            for (int t = 0; t < kMaxThr; ++t) {
                if (t < nt) {
                    unsigned int* bin = tbins + ((size_t)t * (M + 1) + k[t]) * 2;
                    atomicAdd(bin, 1u);
                    if (y >= th[t]) atomicAdd(bin + 1, 1u);
                }
            }
        }
    }
    __syncthreads();
    if (cur >= 0) {
        unsigned long long* rh = rank_hist + (size_t)cur * (M + 1);
        unsigned long long* tb = table + ((size_t)cur * T + t0) * (M + 1) * 2;
        for (int b = threadIdx.x; b < nb; b += kThreads)
            if (bins[b]) atomicAdd(b <= M ? &rh[b] : &tb[b - (M + 1)], (unsigned long long)bins[b]);
    }
}

// row 0 = the sum of the G group rows of x [G + 1][len] (every day is in exactly one group)
__global__ __launch_bounds__(kThreads) void series_row0_kernel(long long* __restrict__ x, int G, size_t len) {
    for (size_t b = (size_t)blockIdx.x * kThreads + threadIdx.x; b < len; b += (size_t)gridDim.x * kThreads) {
        long long s = 0;
        for (int g = 1; g <= G; ++g) s += x[(size_t)g * len + b];
        x[b] = s;
    }
}

// grid G + 1: K46's finish on each row's table; exceedance [G + 1][6][T]
__global__ __launch_bounds__(64) void series_exceedance_finish_kernel(const long long* __restrict__ table, int M, int T,
                                                                      double* __restrict__ exceedance) {
    const int t = threadIdx.x, row = blockIdx.x;
    if (t >= T) return;
    long long cells;
    exceedance_finish_row(table + ((size_t)row * T + t) * (M + 1) * 2, M, T, t, &cells, exceedance + (size_t)row * 6 * T);
}

// ---- K60 ----------------------------------------------------------------------------------------------------------------------
// the validity word of day j's block of 32 days, fetched when j enters a new block
struct DayBits {
    const unsigned int* vb;                                               // vbits + p
    size_t HW;
    bool inb;
    unsigned int word = 0u;
    int block = -1;
    __device__ __forceinline__ bool at(int j) {
        if ((j >> 5) != block) {
            block = j >> 5;
            word = inb ? vb[(size_t)block * HW] : 0u;
        }
        return (word >> (j & 31)) & 1u;
    }
};

// grid ceil(HW / 256), one lane per pixel.  half = sum over the unordered pairs i < j of valid days of |y_i - y_j| for row 0;
// sgroup [G][HW] (zeroed by the caller) gets the same over the pairs within each group.  The pixel's own 16 days i sit in
// registers with their partial sums; the days j > i stream past, first the 15 later days of the chunk, then the rest.  A day i
// that is not valid takes part in the arithmetic and its sums are dropped.  The ordered-pair sum is S = 2 * half, exactly.
template <bool GROUPS>
__global__ __launch_bounds__(kThreads) void series_climatology_kernel(
    const float* __restrict__ obs, const unsigned int* __restrict__ vbits, const int* __restrict__ groups, int G, int D, size_t HW,
    const int* __restrict__ count, const double* __restrict__ state, const double* __restrict__ fgroup, double* __restrict__ sgroup,
    float* __restrict__ clim_maps, double* __restrict__ part) {
    const int lane = threadIdx.x & 63;
    const size_t slots = (size_t)gridDim.x * kWaves, slot = (size_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    const size_t p = (size_t)blockIdx.x * kThreads + threadIdx.x;
    const bool inb = p < HW;
    const float* col = obs + p;
    double half = 0.0;
    for (int i0 = 0; i0 < D; i0 += kDayChunk) {
        double xi[kDayChunk], sa[kDayChunk], sg[kDayChunk];
        int gi[kDayChunk];
        bool vi[kDayChunk];
        DayBits own{vbits + p, HW, inb};
#pragma unroll
        for (int k = 0; k < kDayChunk; ++k) {
            const int i = i0 + k;
            vi[k] = i < D && own.at(i);
            xi[k] = vi[k] ? (double)col[(size_t)i * HW] : 0.0;
            gi[k] = GROUPS ? group_at(groups, min(i, D - 1), G) : 0;
            sa[k] = 0.0;
            sg[k] = 0.0;
        }
#pragma unroll
        for (int kk = 1; kk < kDayChunk; ++kk) {
            if (!vi[kk]) continue;
#pragma unroll
            for (int k = 0; k < kDayChunk; ++k) {
                if (k < kk) {
                    const double dd = fabs(xi[k] - xi[kk]);
                    sa[k] += dd;
                    if (GROUPS) sg[k] += gi[k] == gi[kk] ? dd : 0.0;
                }
            }
        }
        DayBits later{vbits + p, HW, inb};
        for (int j = i0 + kDayChunk; j < D; ++j) {
            if (!later.at(j)) continue;
            const double yj = (double)col[(size_t)j * HW];
            const int gj = GROUPS ? group_at(groups, j, G) : 0;
#pragma unroll
            for (int k = 0; k < kDayChunk; ++k) {
                const double dd = fabs(xi[k] - yj);
                sa[k] += dd;
                if (GROUPS) sg[k] += gi[k] == gj ? dd : 0.0;
            }
        }
#pragma unroll
        for (int k = 0; k < kDayChunk; ++k) {
            if (vi[k]) {
                half += sa[k];
                if (GROUPS) sgroup[(size_t)gi[k] * HW + p] += sg[k];     // this lane's own entry: no other thread touches it
            }
        }
    }
    // per row: n, F = sum of crps_fair, C = S / (2 (n - 1)); the maps are row 0's
    for (int row = 0; row <= (GROUPS ? G : 0); ++row) {
        int n = 0;
        double F = 0.0, S = 0.0;
        if (inb) {
            if (row == 0) {
                n = count[p];
                F = state[p];
                S = 2.0 * half;
            } else {
                DayBits b{vbits + p, HW, inb};
                for (int d = 0; d < D; ++d) n += (group_at(groups, d, G) == row - 1) && b.at(d);
                F = fgroup[(size_t)(row - 1) * HW + p];
                S = 2.0 * sgroup[(size_t)(row - 1) * HW + p];
            }
        }
        const bool scored = n >= 3;
        const double C = S / (2.0 * ((double)n - 1.0));
        if (row == 0 && inb) {
            clim_maps[p] = scored ? (float)(C / (double)n) : nan_f();
            clim_maps[HW + p] = (scored && C != 0.0) ? (float)(1.0 - F / C) : nan_f();
        }
        double c = scored ? (double)n : 0.0, f = scored ? F : 0.0, r = scored ? C : 0.0;
        c = wave_sum_d(c); f = wave_sum_d(f); r = wave_sum_d(r);
        if (lane == 0) {
            double* q = part + ((size_t)row * slots + slot) * 3;
            q[0] = c; q[1] = f; q[2] = r;
        }
    }
}

// grid G + 1: skill_scores [row][4] = (cells, mean forecast CRPS, mean reference CRPS, 1 - sum F / sum C)
__global__ __launch_bounds__(kThreads) void series_skill_kernel(const double* __restrict__ part, int slots, double* __restrict__ skill) {
    __shared__ double sh[kWaves];
    const double* q = part + (size_t)blockIdx.x * slots * 3;
    double v[3] = {0, 0, 0};
    for (int s = threadIdx.x; s < slots; s += kThreads)
        for (int f = 0; f < 3; ++f) v[f] += q[(size_t)s * 3 + f];
    for (int f = 0; f < 3; ++f) v[f] = block_sum_butterfly_waves<kThreads>(v[f], sh);
    if (threadIdx.x == 0) {
        double* out = skill + (size_t)blockIdx.x * 4;
        const bool any = v[0] > 0;
        out[0] = v[0];
        out[1] = any ? v[1] / v[0] : nan_d();
        out[2] = any ? v[2] / v[0] : nan_d();
        out[3] = (any && v[2] != 0.0) ? 1.0 - v[1] / v[2] : nan_d();
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
bool sizes_ok(int D, int M, int H, int W, int T, int G) {
    return D >= 1 && D <= kMaxDays && M >= 2 && M <= kMaxMembers && field_shape_ok(1, H, W) && T >= 0 && T <= kMaxThr && G >= 0 &&
           G <= kMaxGroups;
}

inline int pixel_blocks(int64_t HW) { return (int)((HW + kThreads - 1) / kThreads); }

// The workspace: the parts that every chunk of days shares, then the wave partials of one chunk, then the validity bits.
struct Layout {
    int64_t state, day_sums, fgroup, sgroup, skill_part, part;            // byte offsets, all multiples of 8
    int64_t fixed, day_bytes;                                             // bytes without `part`; bytes of `part` per day
    int64_t vbits(int days) const { return part + (int64_t)days * day_bytes; }
    int64_t bytes(int days) const { return fixed + (int64_t)days * day_bytes; }
};
Layout layout(int D, int H, int W, int G, int climatology) {
    const int64_t HW = (int64_t)H * W, slots = (int64_t)pixel_blocks(HW) * kWaves, f64 = (int64_t)sizeof(double);
    const int64_t per_group = (climatology && G > 0) ? (int64_t)G * HW * f64 : 0;
    Layout l{};
    l.state = 0;
    l.day_sums = l.state + 3 * HW * f64;
    l.fgroup = l.day_sums + (int64_t)D * kSums * f64;
    l.sgroup = l.fgroup + per_group;
    l.skill_part = l.sgroup + per_group;
    l.part = l.skill_part + (climatology ? (int64_t)(G + 1) * slots * 3 * f64 : 0);
    l.day_bytes = slots * kSums * f64;
    l.fixed = l.part + (int64_t)((D + 31) / 32) * HW * (int64_t)sizeof(unsigned int);
    return l;
}
// days of one chunk within `room` bytes of partials: all of them, else a multiple of 32, at least 32
int chunk_days(int D, int64_t room, int64_t day_bytes) {
    const int64_t fit = room > 0 ? room / day_bytes : 0;
    if (fit >= D) return D;
    return (int)std::min<int64_t>(D, std::max<int64_t>(kChunkDays, fit / kChunkDays * kChunkDays));
}

}  // namespace

extern "C" {

int64_t sbgm_series_scores_workspace_bytes(int D, int M, int H, int W, int T, int G, int climatology, int64_t max_bytes) {
    if (!sizes_ok(D, M, H, W, T, G)) return 0;
    const Layout l = layout(D, H, W, G, climatology);
    return l.bytes(chunk_days(D, max_bytes - l.fixed, l.day_bytes));
}

int sbgm_series_scores(const float* ens, int64_t day_stride, int64_t member_stride, const float* obs, const void* mask,
                       int mask_is_u8, int Nm, const int* groups, int G, int D, int M, int H, int W, const float* thresholds, int T,
                       uint64_t seed, int climatology, int* count, float* maps, double* daily, double* scores, int64_t* rank_hist,
                       int64_t* table, double* exceedance, float* clim_maps, double* skill_scores, void* workspace,
                       int64_t workspace_bytes, void* stream) {
    hipStream_t st = ST;
    SBGM_CHECK(ens && obs && count && maps && daily && scores && rank_hist && workspace, "series_scores: null argument");
    SBGM_CHECK(D >= 1 && D <= kMaxDays, "series_scores: D=%d days (1..%d)", D, kMaxDays);
    SBGM_CHECK(M >= 2 && M <= kMaxMembers, "series_scores: M=%d members (2..%d)", M, kMaxMembers);
    SBGM_CHECK(field_shape_ok(1, H, W), "series_scores: field size %dx%d (sides 2..%d, H*W <= 2^20)", H, W, kMaxSide);
    const int64_t HW = (int64_t)H * W;
    SBGM_CHECK(day_stride >= HW && member_stride >= HW, "series_scores: day_stride=%lld, member_stride=%lld elements (each >= H*W)",
               (long long)day_stride, (long long)member_stride);
    SBGM_CHECK(!mask || Nm == 1 || Nm == D, "series_scores: mask of %d fields (1 or %d)", Nm, D);
    SBGM_CHECK(G >= 0 && G <= kMaxGroups && (G == 0 || groups), "series_scores: G=%d groups (0..%d, with their ids)", G, kMaxGroups);
    SBGM_CHECK(T >= 0 && T <= kMaxThr && (T == 0 || (thresholds && table && exceedance)), "series_scores: T=%d thresholds (0..%d, "
               "with their values, table and exceedance)", T, kMaxThr);
    SBGM_CHECK(!climatology || (clim_maps && skill_scores), "series_scores: null clim_maps or skill_scores with climatology on");
    const Layout l = layout(D, H, W, G, climatology);
    SBGM_CHECK(workspace_bytes >= l.bytes(std::min(D, kChunkDays)), "series_scores: workspace of %lld bytes, %lld needed",
               (long long)workspace_bytes, (long long)l.bytes(std::min(D, kChunkDays)));
    ThrList thr;
    if (int rc = fill_thresholds("series_scores", thresholds, T, thr)) return rc;
    const int days = chunk_days(D, workspace_bytes - l.fixed, l.day_bytes);
    char* ws = static_cast<char*>(workspace);
    double* state = reinterpret_cast<double*>(ws + l.state);
    double* day_sums = reinterpret_cast<double*>(ws + l.day_sums);
    double* fgroup = reinterpret_cast<double*>(ws + l.fgroup);
    double* sgroup = reinterpret_cast<double*>(ws + l.sgroup);
    double* skill_part = reinterpret_cast<double*>(ws + l.skill_part);
    double* part = reinterpret_cast<double*>(ws + l.part);
    unsigned int* vbits = reinterpret_cast<unsigned int*>(ws + l.vbits(days));
    const int group_sums = climatology && G > 0;
    const int blocks = pixel_blocks(HW), slots = blocks * kWaves, rows = G + 1;
    const int mask_daily = mask && Nm == D && D > 1;
    if (group_sums)
        if (int rc = sbgm_zero_async(fgroup, (size_t)(2 * G) * HW * sizeof(double), st)) return rc;       // fgroup, then sgroup
    if (int rc = sbgm_zero_async(rank_hist, (size_t)rows * (M + 1) * sizeof(int64_t), st)) return rc;
    if (T > 0)
        if (int rc = sbgm_zero_async(table, (size_t)rows * T * (M + 1) * 2 * sizeof(int64_t), st)) return rc;
    for (int d0 = 0; d0 < D; d0 += days) {
        const int d1 = std::min(D, d0 + days);
        hipLaunchKernelGGL(series_cells_kernel, dim3(blocks), dim3(kThreads), 0, st, ens, (long long)day_stride,
                           (long long)member_stride, obs, mask, mask_is_u8, mask_daily, groups, G, group_sums, D, M, (size_t)HW, d0, d1,
                           count, maps, state, fgroup, vbits, part);
        SBGM_LAUNCH_CHECK();
        hipLaunchKernelGGL(series_daily_kernel, dim3(d1 - d0), dim3(kThreads), 0, st, part, slots, M, d0, day_sums, daily);
        SBGM_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(series_rows_kernel, dim3(rows), dim3(kThreads), 0, st, day_sums, groups, G, D, M, scores);
    SBGM_LAUNCH_CHECK();
    // thresholds per workgroup of K59: what the LDS budget holds beside the rank bins
    const int tg = T > 0 ? std::max(1, std::min(T, (kCountLdsBytes / ((M + 1) * 4) - 1) / 2)) : 0;
    const int bx = std::min(blocks, kCountMaxBlocks);
    hipLaunchKernelGGL(series_counts_kernel, dim3(bx, T > 0 ? (T + tg - 1) / tg : 1, (D + kCountDays - 1) / kCountDays), dim3(kThreads),
                       (size_t)(M + 1) * (4 + 8 * tg), st, ens, (long long)day_stride, (long long)member_stride, obs, vbits, groups, G, D, M,
                       (size_t)HW, T, tg, thr, (unsigned long long)seed, reinterpret_cast<unsigned long long*>(rank_hist),
                       reinterpret_cast<unsigned long long*>(table));
    SBGM_LAUNCH_CHECK();
    if (G > 0) {
        hipLaunchKernelGGL(series_row0_kernel, dim3(1), dim3(kThreads), 0, st, reinterpret_cast<long long*>(rank_hist), G, (size_t)(M + 1));
        SBGM_LAUNCH_CHECK();
        if (T > 0) {
            const size_t len = (size_t)T * (M + 1) * 2;
            hipLaunchKernelGGL(series_row0_kernel, dim3((unsigned)std::min<size_t>((len + kThreads - 1) / kThreads, 256)), dim3(kThreads), 0,
                               st, reinterpret_cast<long long*>(table), G, len);
            SBGM_LAUNCH_CHECK();
        }
    }
    if (T > 0) {
        hipLaunchKernelGGL(series_exceedance_finish_kernel, dim3(rows), dim3(64), 0, st, reinterpret_cast<const long long*>(table), M, T,
                           exceedance);
        SBGM_LAUNCH_CHECK();
    }
    if (climatology) {
        if (G > 0)
            hipLaunchKernelGGL(series_climatology_kernel<true>, dim3(blocks), dim3(kThreads), 0, st, obs, vbits, groups, G, D, (size_t)HW,
                               count, state, fgroup, sgroup, clim_maps, skill_part);
        else
            hipLaunchKernelGGL(series_climatology_kernel<false>, dim3(blocks), dim3(kThreads), 0, st, obs, vbits, groups, G, D, (size_t)HW,
                               count, state, fgroup, sgroup, clim_maps, skill_part);
        SBGM_LAUNCH_CHECK();
        hipLaunchKernelGGL(series_skill_kernel, dim3(rows), dim3(kThreads), 0, st, skill_part, slots, skill_scores);
        SBGM_LAUNCH_CHECK();
    }
    return 0;
}

}  // extern "C"
