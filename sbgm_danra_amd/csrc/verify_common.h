// Helpers shared by the verification kernels (verify.hip, verify_spatial.hip, verify_products.hip, verify_objects.hip,
// verify_multivariate.hip, verify_series.hip) and, for the order-preserving key, postproc.hip: the validity predicates, the NaN
// constants, the float <-> uint32 key, the threshold list and its host-side fill, the field / member limits, the block
// reductions and the host-side planner of (field, threshold) chunks.  Each is defined here once.
// Some of the including files compile with FP contraction off and some with it on.  The device helpers below contain only
// adds, comparisons and min / max, so nothing in them can contract and they mean the same in both; keep it that way: no
// multiply-add belongs in this header.  The one exception, exceedance_finish_row, turns contraction off inside its own body.
#pragma once
#include <algorithm>
#include <cmath>

#include "../../include/sbgm_hip.h"
#include "common.h"

static_assert(SBGM_SPATIAL_MAX_THRESHOLDS == SBGM_PRODUCTS_MAX_THRESHOLDS && SBGM_SPATIAL_MAX_THRESHOLDS == SBGM_OBJECTS_MAX_THRESHOLDS,
              "one ThrList serves the spatial, product and object scores: their threshold limits must be equal");

// ---- limits -----------------------------------------------------------------------------------------------------------------
constexpr int kMaxThr = SBGM_SPATIAL_MAX_THRESHOLDS;      // thresholds of one call (object_scores: fixed ones; the relative one is extra)
constexpr int kMaxFields = 65535;                         // fields of one call (a grid dimension)
constexpr int kMaxSide = 2048;                            // field sides of the neighbourhood and object scores
constexpr int64_t kMaxPixels = 1ll << 20;                 // H * W
constexpr int kMaxMembers = 4095;                         // exceedance scores, ensemble products, multivariate scores

inline bool field_shape_ok(int N, int H, int W) {
    return N >= 1 && N <= kMaxFields && H >= 2 && W >= 2 && H <= kMaxSide && W <= kMaxSide && (int64_t)H * W <= kMaxPixels;
}

// ---- thresholds: passed to the kernels by value -----------------------------------------------------------------------------
struct ThrList { float v[kMaxThr]; };

// thr = the T <= kMaxThr host values, each checked to be finite; entries past T stay 0
inline int fill_thresholds(const char* op, const float* thresholds, int T, ThrList& thr) {
    thr = ThrList{};
    for (int t = 0; t < T; ++t) {
        SBGM_CHECK(std::isfinite(thresholds[t]), "%s: threshold %d is not finite", op, t);
        thr.v[t] = thresholds[t];
    }
    return 0;
}

// ---- validity and NaN -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool is_nan(float v) { return v != v; }
__device__ __forceinline__ float nan_f() { return __uint_as_float(0x7FC00000u); }
__device__ __forceinline__ double nan_d() { return __longlong_as_double(0x7FF8000000000000ll); }
// the mask admits pixel i: uint8 != 0, or fp32 > 0.5; no mask admits everything
__device__ __forceinline__ bool mask_at(const void* mask, int mask_u8, size_t i) {
    if (!mask) return true;
    return mask_u8 ? static_cast<const unsigned char*>(mask)[i] != 0 : static_cast<const float*>(mask)[i] > 0.5f;
}

// ---- order-preserving key ---------------------------------------------------------------------------------------------------
// Monotone map of the fp32 values onto uint32 and back: all bits of a negative are flipped, and the sign bit of a
// non-negative.  -0 lands just below +0 (a caller that wants them equal folds -0 onto +0 first); no float maps to key 0;
// NaNs with the sign bit clear sort above +inf, as torch.sort places them.
// Written as one xor with the sign-derived pattern (0xFFFFFFFF for a negative, 0x80000000 otherwise): two instructions in the
// per-member loops of verify_products.hip.
__device__ __forceinline__ unsigned int float_key(float v) {
    const unsigned int b = __float_as_uint(v);
    return b ^ ((unsigned int)((int)b >> 31) | 0x80000000u);
}
__device__ __forceinline__ float key_float(unsigned int k) {
    return __uint_as_float(k ^ ((k & 0x80000000u) ? 0x80000000u : 0xFFFFFFFFu));
}

// ---- block reductions, named by the order in which they add -----------------------------------------------------------------
// Every thread of a workgroup of THREADS threads calls them, and every thread gets the result.  The two fp64 sums add in
// different orders and so round differently: they are NOT interchangeable.  Each output is specified bit for bit by the order
// its kernel uses, so a kernel must keep the one it has.

// fp64 sum, "butterfly, then wave partials in index order": xor butterfly over the 64 lanes of each wave, then the waves' sums
// added from wave 0 up.  `sh` holds THREADS / 64 doubles.
template <int THREADS>
__device__ __forceinline__ double block_sum_butterfly_waves(double v, double* sh) {
    v = wave_sum_d(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    for (int w = 0; w < THREADS / SBGM_WAVE; ++w) s += sh[w];
    return s;
}

// fp64 sum and minimum, "LDS halving tree": sh[t] op= sh[t + o] for o = THREADS / 2, THREADS / 4, ..., 1.  `sh` holds THREADS
// doubles and may be used again at once.
template <int THREADS>
__device__ __forceinline__ double block_sum_tree(double v, double* sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}
template <int THREADS>
__device__ __forceinline__ double block_min_tree(double v, double* sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] = fmin(sh[threadIdx.x], sh[threadIdx.x + o]);
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

// integer sum (exact in any order); `slot` holds THREADS / 64 entries
template <int THREADS>
__device__ __forceinline__ unsigned long long block_sum_u64(unsigned long long v, unsigned long long* slot) {
    v = wave_sum_u64(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long t = 0;
    for (int w = 0; w < THREADS / SBGM_WAVE; ++w) t += slot[w];
    return t;
}

// ---- the scores of one exceedance table -------------------------------------------------------------------------------------
// K46's finish, shared by exceedance_scores (one table per threshold) and series_scores (one per row and threshold).  `tab` is
// threshold t's table [M + 1][2].  With n_k, o_k the two columns, N = sum n_k, O = sum o_k, p_k = k / M, obar = O / N and
// obar_k = o_k / n_k:
//   brier = sum_k (n_k p_k^2 - 2 o_k p_k + o_k) / N        reliability = sum_k n_k (p_k - obar_k)^2 / N
//   resolution = sum_k n_k (obar_k - obar)^2 / N            uncertainty = obar (1 - obar)
//   roc_area: forecast "yes" when k >= c; the points (false-alarm rate, hit rate) for c = M + 1 (0, 0) down to c = 0 (1, 1)
//   joined by trapezoids; NaN when the event never or always occurs.
// scores [6][T]: entry t of (brier, reliability, resolution, uncertainty, base_rate, roc_area); *cells = N.  N == 0 gives NaN.
__device__ __forceinline__ void exceedance_finish_row(const long long* __restrict__ tab, int M, int T, int t, long long* cells,
                                                      double* __restrict__ scores) {
#pragma clang fp contract(off)
    long long Nn = 0, Oo = 0;
    for (int k = 0; k <= M; ++k) { Nn += tab[2 * k]; Oo += tab[2 * k + 1]; }
    *cells = Nn;
    const double N = (double)Nn, O = (double)Oo, Md = (double)M;
    double bs = 0.0, rel = 0.0, res = 0.0, area = 0.0;
    const double obar = O / N;
    long long hits = 0, fas = 0;
    for (int k = M; k >= 0; --k) {
        const double nk = (double)tab[2 * k], ok = (double)tab[2 * k + 1], pk = (double)k / Md;
        bs += nk * pk * pk - 2.0 * ok * pk + ok;
        if (tab[2 * k] > 0) {
            const double obk = ok / nk;
            rel += nk * (pk - obk) * (pk - obk);
            res += nk * (obk - obar) * (obk - obar);
        }
        const long long h1 = hits + tab[2 * k + 1], f1 = fas + tab[2 * k] - tab[2 * k + 1];
        area += ((double)(f1 - fas) / (N - O)) * (((double)h1 + (double)hits) / O) / 2.0;
        hits = h1; fas = f1;
    }
    const bool any = Nn > 0;
    scores[0 * T + t] = any ? bs / N : nan_d();
    scores[1 * T + t] = any ? rel / N : nan_d();
    scores[2 * T + t] = any ? res / N : nan_d();
    scores[3 * T + t] = any ? obar * (1.0 - obar) : nan_d();
    scores[4 * T + t] = any ? obar : nan_d();
    scores[5 * T + t] = (any && Oo > 0 && Oo < Nn) ? area : nan_d();
}

// ---- chunks of (field, threshold) pairs -------------------------------------------------------------------------------------
// A score whose workspace grows with the number of (field, threshold) pairs works through the N x T pairs in chunks: as many
// whole fields as fit into `room` bytes at `pair_bytes` a pair (and into `max_pairs`, a grid dimension), else some thresholds
// of one field; at least one pair, whatever the room.
struct ChunkPlan {
    int64_t pairs;                                        // pairs of a full chunk = fields * thresholds
    int fields, thresholds;
};
inline ChunkPlan plan_chunks(int N, int T, int64_t room, int64_t pair_bytes, int64_t max_pairs) {
    const int64_t fit = std::min(max_pairs, std::max<int64_t>(1, room / pair_bytes));
    if (fit >= T) {
        const int fields = (int)std::min<int64_t>(fit / T, N);
        return {(int64_t)fields * T, fields, T};
    }
    return {fit, 1, (int)fit};
}
// body(f0, nf, t0, nt) for every chunk, fields outermost; stops at the first non-zero return and returns it
template <class Body>
inline int for_each_chunk(const ChunkPlan& plan, int N, int T, Body body) {
    for (int f0 = 0; f0 < N; f0 += plan.fields)
        for (int t0 = 0; t0 < T; t0 += plan.thresholds)
            if (int rc = body(f0, std::min(plan.fields, N - f0), t0, std::min(plan.thresholds, T - t0))) return rc;
    return 0;
}
