// Neighbourhood and threshold verification scores on the device.  Both are integer statistics, so every count
// below is exact and independent of the order in which it was added:
//   K45 neighbourhood_scores — Fractions Skill Score (Roberts & Lean 2008) numerators and denominators over thresholds x
//                              window widths, in O(H*W) per (field, threshold, width) whatever the width.
//   K46 exceedance_scores    — per threshold the table (members above the threshold, truth above it) of an ensemble, and
//                              from the table alone the Brier score, Murphy's decomposition, the base rate and the ROC area.
// A pixel is valid when gen (every member, for K46) and obs are not NaN and the mask (uint8 != 0, or fp32 > 0.5) admits it;
// an event is `v >= thr` in fp32 at a valid pixel.
// Reproducibility: counts are integers (LDS-private bins and per-wave partials; the only global atomics are 64-bit integer
// adds), and the fp64 scores are computed by single threads of the finalize kernels in a fixed order.  No float atomics.
// FP contraction is off in this file, as in verify.hip.  The helpers shared with the other verify files (validity, ThrList,
// limits, the chunk planner) are in verify_common.h.
#include "verify_common.h"

#pragma clang fp contract(off)

#define ST ((hipStream_t)stream)

namespace {

constexpr int kMaxScales = SBGM_SPATIAL_MAX_SCALES;
constexpr int kRowThreads = 256;                          // K45 pass 1: one workgroup per row,
constexpr int kRowPer = kMaxSide / kRowThreads;           // each thread owns 8 consecutive columns
constexpr int kStrip = 256;                               // K45 pass 2: columns per workgroup, one per lane
constexpr int kStripWaves = kStrip / SBGM_WAVE;
constexpr int64_t kMaxChunkPairs = 65535;                 // gridDim.z of pass 2
constexpr int kExcThreads = 512;
constexpr int kExcMaxBlocks = 256;
constexpr int kExcLdsBytes = 32768;                       // LDS tables of one workgroup: (M + 1) * 8 bytes per threshold

struct ScaleList { int r[kMaxScales]; };                  // window radii, clamped to max(H, W)

// ---- K45 pass 1: row-wise inclusive prefix sums of the two indicator images ------------------------------------------------
// grid (H, nf): the workgroup reads row `blockIdx.x` of field f0 + blockIdx.y once and, for each of the nt thresholds from t0,
// writes P[fi][ti][row][col] = (prefix of I_g) | (prefix of I_o) << 16 — a row holds at most 2048 events, so each half is a
// uint16.  The two halves are scanned as one uint32 (neither can carry into the other).  The row totals are added to
// events_gen / events_obs with one 64-bit integer atomic per row; the chunk with t0 == 0 also scans the validity image for
// valid[f] (the pass ti == nt, which stores nothing).
__global__ __launch_bounds__(kRowThreads) void neighbourhood_prefix_kernel(
    const float* __restrict__ gen, const float* __restrict__ obs, const void* __restrict__ mask, int mask_u8, int obs_step,
    int mask_step, int H, int W, int f0, int T, int t0, int nt, ThrList thr, unsigned int* __restrict__ prefix,
    unsigned long long* __restrict__ events_gen, unsigned long long* __restrict__ events_obs, unsigned long long* __restrict__ valid) {
    __shared__ unsigned int wave_tot[2][kRowThreads / SBGM_WAVE];
    const int row = blockIdx.x, fi = blockIdx.y, f = f0 + fi;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t HW = (size_t)H * W;
    const int c0 = threadIdx.x * kRowPer;
    float g[kRowPer], o[kRowPer];
    bool ok[kRowPer];
#pragma unroll
    for (int e = 0; e < kRowPer; ++e) {
        const int c = c0 + e;
        g[e] = 0.f; o[e] = 0.f; ok[e] = false;
        if (c < W) {
            const size_t p = (size_t)row * W + c;
            g[e] = gen[(size_t)f * HW + p];
            o[e] = obs[(size_t)f * obs_step * HW + p];
            ok[e] = !is_nan(g[e]) && !is_nan(o[e]) && mask_at(mask, mask_u8, (size_t)f * mask_step * HW + p);
        }
    }
    const int passes = nt + (t0 == 0 ? 1 : 0);
    for (int ti = 0; ti < passes; ++ti) {
        const bool count_valid = ti == nt;
        const float th = thr.v[count_valid ? 0 : t0 + ti];
        unsigned int run[kRowPer], tot = 0;
#pragma unroll
        for (int e = 0; e < kRowPer; ++e) {
            const unsigned int ig = ok[e] && (count_valid || g[e] >= th), io = ok[e] && !count_valid && o[e] >= th;
            tot += ig | (io << 16);
            run[e] = tot;
        }
        unsigned int inc = tot;                                   // inclusive scan of the thread totals over the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned int up = __shfl_up(inc, d, 64);
            if (lane >= d) inc += up;
        }
        unsigned int* wt = wave_tot[ti & 1];                      // two buffers: one barrier per pass is enough
        if (lane == 63) wt[wave] = inc;
        __syncthreads();
        unsigned int before = inc - tot;
        for (int w = 0; w < wave; ++w) before += wt[w];
        if (!count_valid) {
            unsigned int* prow = prefix + ((size_t)fi * nt + ti) * HW + (size_t)row * W;
#pragma unroll
            for (int e = 0; e < kRowPer; ++e)
                if (c0 + e < W) prow[c0 + e] = before + run[e];
        }
        if (threadIdx.x == kRowThreads - 1) {
            const unsigned int all = before + tot;
            if (count_valid) {
                if (all) atomicAdd(&valid[f], (unsigned long long)all);
            } else {
                if (all & 0xFFFFu) atomicAdd(&events_gen[(size_t)f * T + t0 + ti], (unsigned long long)(all & 0xFFFFu));
                if (all >> 16) atomicAdd(&events_obs[(size_t)f * T + t0 + ti], (unsigned long long)(all >> 16));
            }
        }
    }
}

// ---- K45 pass 2: the vertical walk ------------------------------------------------------------------------------------------
// grid (strips, S, nf * nt).  Lane = one column j of the strip, so the 64 lanes of a wave read 256 consecutive bytes of a prefix
// row.  The horizontal window count of row i is h(i) = P[i][min(j + r, W - 1)] - P[i][j - r - 1] (both halves at once; the left
// term is 0 off the domain), and the lane keeps C = sum of h over rows i - r .. i + r inside the domain: it adds the row that
// enters the window and subtracts the row that leaves it, two loads each, whatever r is.  The rows before the first centre cost
// min(r, H) steps, so a (field, threshold, width) costs at most 2 H W steps.  (C_g - C_o)^2 and C_g^2 + C_o^2 accumulate in
// uint64 per lane (C <= 2^20, H <= 2^11: at most 2^52 per lane), a butterfly adds the lanes, and wave w of strip b writes slot
// 4 b + w of part[pair][scale][slot][2].
__global__ __launch_bounds__(kStrip) void neighbourhood_walk_kernel(const unsigned int* __restrict__ prefix, int H, int W,
                                                                    ScaleList sc, unsigned long long* __restrict__ part) {
    const int j = blockIdx.x * kStrip + threadIdx.x;
    const int s = blockIdx.y, S = gridDim.y, nslot = gridDim.x * kStripWaves;
    const size_t pair = blockIdx.z;
    const int r = sc.r[s];
    const unsigned int* P = prefix + pair * (size_t)H * W;
    unsigned long long num = 0, den = 0;
    if (j < W) {
        const int hi = min(j + r, W - 1), lo = j - r - 1;
        auto h = [&](int i) -> unsigned int {
            const unsigned int* prow = P + (size_t)i * W;
            return prow[hi] - (lo >= 0 ? prow[lo] : 0u);          // each half of [hi] >= that half of [lo]: no borrow
        };
        unsigned int cg = 0, co = 0;
        const int pre = min(r, H);
        for (int i = 0; i < pre; ++i) {
            const unsigned int v = h(i);
            cg += v & 0xFFFFu; co += v >> 16;
        }
        for (int i = 0; i < H; ++i) {
            if (i + r < H) {
                const unsigned int v = h(i + r);
                cg += v & 0xFFFFu; co += v >> 16;
            }
            if (i - r - 1 >= 0) {
                const unsigned int v = h(i - r - 1);
                cg -= v & 0xFFFFu; co -= v >> 16;
            }
            const unsigned long long a = cg, b = co, d = a > b ? a - b : b - a;
            num += d * d;
            den += a * a + b * b;
        }
    }
    num = wave_sum_u64(num);
    den = wave_sum_u64(den);
    if ((threadIdx.x & 63) == 0) {
        unsigned long long* q = part + ((pair * S + s) * nslot + (size_t)blockIdx.x * kStripWaves + (threadIdx.x >> 6)) * 2;
        q[0] = num; q[1] = den;
    }
}

// one thread per (pair, scale) of the chunk: the slots in index order -> num, den [N][T][S], fss_field = 1 - num / den
__global__ __launch_bounds__(256) void neighbourhood_collect_kernel(const unsigned long long* __restrict__ part, int nslot, int f0,
                                                                    int T, int t0, int nt, int S, int npairs,
                                                                    long long* __restrict__ num, long long* __restrict__ den,
                                                                    double* __restrict__ fss_field) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npairs * S) return;
    const int pair = i / S, s = i % S;
    const unsigned long long* q = part + (size_t)i * nslot * 2;
    unsigned long long n = 0, d = 0;
    for (int k = 0; k < nslot; ++k) { n += q[2 * k]; d += q[2 * k + 1]; }
    const size_t out = ((size_t)(f0 + pair / nt) * T + t0 + pair % nt) * S + s;
    num[out] = (long long)n;
    den[out] = (long long)d;
    fss_field[out] = d ? 1.0 - (double)n / (double)d : nan_d();
}

// one block, after the last chunk: thread i < T * S sums num and den over the fields in field order (fp64) for fss [T][S];
// thread t < T also gives freq_bias[t] = sum events_gen / sum events_obs and fss_useful[t] = 0.5 + (sum events_obs / sum valid) / 2
// (plain IEEE divisions of exactly representable totals: x / 0 is inf, 0 / 0 is NaN).
__global__ __launch_bounds__(256) void neighbourhood_finish_kernel(const long long* __restrict__ num, const long long* __restrict__ den,
                                                                   const long long* __restrict__ events_gen,
                                                                   const long long* __restrict__ events_obs,
                                                                   const long long* __restrict__ valid, int N, int T, int S,
                                                                   double* __restrict__ fss, double* __restrict__ freq_bias,
                                                                   double* __restrict__ fss_useful) {
    const int i = threadIdx.x;
    if (i < T * S) {
        double n = 0.0, d = 0.0;
        for (int f = 0; f < N; ++f) {
            n += (double)num[(size_t)f * T * S + i];
            d += (double)den[(size_t)f * T * S + i];
        }
        fss[i] = d > 0.0 ? 1.0 - n / d : nan_d();
    }
    if (i < T) {
        long long eg = 0, eo = 0, nv = 0;
        for (int f = 0; f < N; ++f) {
            eg += events_gen[(size_t)f * T + i];
            eo += events_obs[(size_t)f * T + i];
            nv += valid[f];
        }
        freq_bias[i] = (double)eg / (double)eo;
        fss_useful[i] = 0.5 + ((double)eo / (double)nv) / 2.0;
    }
}

// ---- K46 exceedance table ---------------------------------------------------------------------------------------------------
// grid (pixel blocks, threshold groups): lane = pixel (grid-stride), members read coalesced ([M][HW] rows) and streamed once,
// counting k for the group's up to 16 thresholds in registers.  The workgroup's LDS holds one uint32 table [M + 1][2] per
// threshold of its group: (pixels with that k, those of them with obs >= thr); every non-empty bin is flushed with one 64-bit
// integer atomic.  Dynamic LDS = tg * (M + 1) * 8 bytes.
__global__ __launch_bounds__(kExcThreads) void exceedance_kernel(const float* __restrict__ ens, const float* __restrict__ obs,
                                                                 const void* __restrict__ mask, int mask_u8, int M, size_t HW, int T,
                                                                 int tg, ThrList thr, unsigned long long* __restrict__ table) {
    extern __shared__ unsigned int bins[];
    const int t0 = blockIdx.y * tg, nt = min(tg, T - t0);
    const int nb = nt * (M + 1) * 2;
    for (int b = threadIdx.x; b < nb; b += kExcThreads) bins[b] = 0;
    __syncthreads();
    float th[kMaxThr];
#pragma unroll
    for (int t = 0; t < kMaxThr; ++t) th[t] = thr.v[min(t0 + t, T - 1)];
    for (size_t p = (size_t)blockIdx.x * kExcThreads + threadIdx.x; p < HW; p += (size_t)gridDim.x * kExcThreads) {
        const float y = obs[p];
        if (is_nan(y) || !mask_at(mask, mask_u8, p)) continue;
        int k[kMaxThr];
#pragma unroll
        for (int t = 0; t < kMaxThr; ++t) k[t] = 0;
        bool valid = true;
        for (int m = 0; m < M; ++m) {
            const float v = ens[(size_t)m * HW + p];
            valid = valid && !is_nan(v);
#pragma unroll
            for (int t = 0; t < kMaxThr; ++t) k[t] += v >= th[t];
        }
        if (!valid) continue;
#pragma unroll
        for (int t = 0; t < kMaxThr; ++t) {
            if (t < nt) {
                unsigned int* bin = bins + ((size_t)t * (M + 1) + k[t]) * 2;
                atomicAdd(bin, 1u);
                if (y >= th[t]) atomicAdd(bin + 1, 1u);
            }
        }
    }
    __syncthreads();
    unsigned long long* out = table + (size_t)t0 * (M + 1) * 2;
    for (int b = threadIdx.x; b < nb; b += kExcThreads)
        if (bins[b]) atomicAdd(&out[b], (unsigned long long)bins[b]);
}

// one block; thread t < T walks its threshold's table in bin order: exceedance_finish_row (verify_common.h), which
// verify_series.hip runs on each of its rows.  scores [6][T] = (brier, reliability, resolution, uncertainty, base_rate,
// roc_area); count[0] = N.  N == 0 gives NaN.
__global__ __launch_bounds__(64) void exceedance_finish_kernel(const long long* __restrict__ table, int M, int T,
                                                               long long* __restrict__ count, double* __restrict__ scores) {
    const int t = threadIdx.x;
    if (t >= T) return;
    long long cells;
    exceedance_finish_row(table + (size_t)t * (M + 1) * 2, M, T, t, &cells, scores);
    if (t == 0) count[0] = cells;
}

inline int strips(int W) { return (W + kStrip - 1) / kStrip; }
// workspace of one (field, threshold) pair: its prefix image and its S * slots partial pairs
inline int64_t pair_bytes(int H, int W, int S) {
    return (int64_t)H * W * (int64_t)sizeof(unsigned int) + (int64_t)S * strips(W) * kStripWaves * 2 * (int64_t)sizeof(unsigned long long);
}
inline ChunkPlan chunk_plan(int N, int H, int W, int T, int S, int64_t max_bytes) {
    return plan_chunks(N, T, max_bytes, pair_bytes(H, W, S), kMaxChunkPairs);
}
inline bool shape_ok(int N, int H, int W, int T, int S) {
    return field_shape_ok(N, H, W) && T >= 1 && T <= kMaxThr && S >= 1 && S <= kMaxScales;
}

}  // namespace

extern "C" {

int sbgm_neighbourhood_scores_strip_columns(void) { return kStrip; }

int64_t sbgm_neighbourhood_scores_workspace_bytes(int N, int H, int W, int T, int S, int64_t max_bytes) {
    if (!shape_ok(N, H, W, T, S)) return 0;
    return chunk_plan(N, H, W, T, S, max_bytes).pairs * pair_bytes(H, W, S);
}

int sbgm_neighbourhood_scores(const float* gen, const float* obs, const void* mask, int mask_is_u8, int N, int No, int Nm, int H, int W,
                              const float* thresholds, int T, const int* scales, int S, int64_t* num, int64_t* den,
                              int64_t* events_gen, int64_t* events_obs, int64_t* valid, double* fss, double* fss_field,
                              double* freq_bias, double* fss_useful, void* workspace, int64_t workspace_bytes, void* stream) {
    hipStream_t st = ST;
    SBGM_CHECK(gen && obs && thresholds && scales && num && den && events_gen && events_obs && valid && fss && fss_field && freq_bias &&
               fss_useful && workspace, "neighbourhood_scores: null argument");
    SBGM_CHECK(shape_ok(N, H, W, T, S), "neighbourhood_scores: N=%d H=%d W=%d T=%d S=%d (N 1..65535, sides 2..%d, H*W <= 2^20, "
               "1..%d thresholds, 1..%d widths)", N, H, W, T, S, kMaxSide, kMaxThr, kMaxScales);
    SBGM_CHECK(No == 1 || No == N, "neighbourhood_scores: obs has %d fields; need 1 or N=%d", No, N);
    SBGM_CHECK(!mask || Nm == 1 || Nm == N, "neighbourhood_scores: mask has %d fields; need 1 or N=%d", Nm, N);
    ThrList thr;
    ScaleList sc{};
    if (int rc = fill_thresholds("neighbourhood_scores", thresholds, T, thr)) return rc;
    for (int s = 0; s < S; ++s) {
        SBGM_CHECK(scales[s] >= 1 && scales[s] % 2 == 1, "neighbourhood_scores: width %d must be odd and >= 1", scales[s]);
        sc.r[s] = std::min((scales[s] - 1) / 2, std::max(H, W));       // a window past both sides covers the field either way
    }
    const int64_t pb = pair_bytes(H, W, S);
    SBGM_CHECK(workspace_bytes >= pb, "neighbourhood_scores: workspace of %lld bytes; one field x one threshold needs %lld",
               (long long)workspace_bytes, (long long)pb);
    const int nslot = strips(W) * kStripWaves;
    if (int rc = sbgm_zero_async(events_gen, (size_t)N * T * sizeof(int64_t), st)) return rc;
    if (int rc = sbgm_zero_async(events_obs, (size_t)N * T * sizeof(int64_t), st)) return rc;
    if (int rc = sbgm_zero_async(valid, (size_t)N * sizeof(int64_t), st)) return rc;
    const int rc = for_each_chunk(chunk_plan(N, H, W, T, S, workspace_bytes), N, T, [&](int f0, int nf, int t0, int nt) -> int {
        const int np = nf * nt;
        unsigned long long* part = static_cast<unsigned long long*>(workspace);              // 8-byte aligned: partials first
        unsigned int* prefix = reinterpret_cast<unsigned int*>(part + (size_t)np * S * nslot * 2);
        hipLaunchKernelGGL(neighbourhood_prefix_kernel, dim3(H, nf), dim3(kRowThreads), 0, st, gen, obs, mask, mask_is_u8,
                           No == 1 ? 0 : 1, Nm == 1 ? 0 : 1, H, W, f0, T, t0, nt, thr, prefix,
                           reinterpret_cast<unsigned long long*>(events_gen), reinterpret_cast<unsigned long long*>(events_obs),
                           reinterpret_cast<unsigned long long*>(valid));
        SBGM_LAUNCH_CHECK();
        hipLaunchKernelGGL(neighbourhood_walk_kernel, dim3(strips(W), S, np), dim3(kStrip), 0, st, prefix, H, W, sc, part);
        SBGM_LAUNCH_CHECK();
        hipLaunchKernelGGL(neighbourhood_collect_kernel, dim3((np * S + 255) / 256), dim3(256), 0, st, part, nslot, f0, T, t0, nt, S, np,
                           reinterpret_cast<long long*>(num), reinterpret_cast<long long*>(den), fss_field);
        SBGM_LAUNCH_CHECK();
        return 0;
    });
    if (rc) return rc;
    hipLaunchKernelGGL(neighbourhood_finish_kernel, dim3(1), dim3(256), 0, st, reinterpret_cast<const long long*>(num),
                       reinterpret_cast<const long long*>(den), reinterpret_cast<const long long*>(events_gen),
                       reinterpret_cast<const long long*>(events_obs), reinterpret_cast<const long long*>(valid), N, T, S, fss,
                       freq_bias, fss_useful);
    SBGM_LAUNCH_CHECK();
    return 0;
}

int64_t sbgm_exceedance_scores_workspace_bytes(int M, int64_t HW, int T) {
    (void)M; (void)HW; (void)T;
    return 0;                          // the table is accumulated in place; the query exists so callers size every score alike
}

int sbgm_exceedance_scores(const float* ens, const float* obs, const void* mask, int mask_is_u8, int M, int64_t HW,
                           const float* thresholds, int T, int64_t* table, int64_t* count, double* scores, void* workspace,
                           void* stream) {
    (void)workspace;
    hipStream_t st = ST;
    SBGM_CHECK(ens && obs && thresholds && table && count && scores, "exceedance_scores: null argument");
    SBGM_CHECK(M >= 2 && M <= kMaxMembers, "exceedance_scores: M=%d members (2..%d)", M, kMaxMembers);
    SBGM_CHECK(HW >= 1 && HW < (1ll << 31), "exceedance_scores: HW=%lld", (long long)HW);
    SBGM_CHECK(T >= 1 && T <= kMaxThr, "exceedance_scores: %d thresholds (1..%d)", T, kMaxThr);
    ThrList thr;
    if (int rc = fill_thresholds("exceedance_scores", thresholds, T, thr)) return rc;
    if (int rc = sbgm_zero_async(table, (size_t)T * (M + 1) * 2 * sizeof(int64_t), st)) return rc;
    const int tg = std::max(1, std::min(T, kExcLdsBytes / ((M + 1) * 8)));        // thresholds per workgroup: the LDS budget
    const int bx = (int)std::min<int64_t>((HW + kExcThreads - 1) / kExcThreads, kExcMaxBlocks);
    hipLaunchKernelGGL(exceedance_kernel, dim3(bx, (T + tg - 1) / tg), dim3(kExcThreads), (size_t)tg * (M + 1) * 8, st, ens, obs, mask,
                       mask_is_u8, M, (size_t)HW, T, tg, thr, reinterpret_cast<unsigned long long*>(table));
    SBGM_LAUNCH_CHECK();
    hipLaunchKernelGGL(exceedance_finish_kernel, dim3(1), dim3(64), 0, st, reinterpret_cast<const long long*>(table), M, T,
                       reinterpret_cast<long long*>(count), scores);
    SBGM_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
