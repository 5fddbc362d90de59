// Ensemble products on the device:
//   K47 ensemble_products — per pixel of an ensemble ens [M][HW]: mean, standard deviation (ddof 1), minimum, maximum, Q
//                           quantile maps (numpy's default, Hyndman-Fan type 7) and T exceedance-probability maps.
// A pixel is valid when no member is NaN and the mask (uint8 != 0, or fp32 > 0.5) admits it; every map is NaN elsewhere.
// Lanes map to pixels (grid-stride), so every member row is read coalesced, as K43 and K46 read it.  Two kernels:
//   moments   — sweep 1 over the members: NaN flag, fp64 sum, minimum and maximum, the T counters k = #{x >= thr}; sweep 2:
//               sum (x - mean)^2 in fp64 against the unrounded mean.  Both sums run in member order.
//   quantiles — exact selection by bitwise bisection on the order-preserving uint32 image of an fp32 value (-0 first mapped
//               to +0; then all bits of a negative are flipped, and the sign bit of a non-negative).  For a rank r the
//               candidate c = prefix | bit is kept iff #{keys < c} <= r, i.e. iff x_(r) >= c; after the 32 bits, top down,
//               the prefix is the key of x_(r).  One launch carries up to 8 quantiles = 16 ranks (lo and hi of each) through
//               the same 32 sweeps, one compare-and-add per member and rank; the kernel is instantiated per quantile count,
//               so no rank is carried in vain.  No LDS, no sort, one code path for every M.
// The minimum and the maximum are also taken on the keys, so a zero order statistic is +0 in every map and the q = 0 / q = 1
// maps are bit-equal to min / max.  Order statistics and counts do not depend on the member order.
// Reproducibility: no float atomics (the only atomic is the 64-bit integer add of the valid-pixel count).
// FP contraction is off in this file, as in verify.hip: the fp64 expressions are the op sequences of the numpy restatement.
// The helpers shared with the other verify files (validity, ThrList, limits, the key) are in verify_common.h.
#include "verify_common.h"

#pragma clang fp contract(off)

#define ST ((hipStream_t)stream)

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;
constexpr int kMaxQuant = SBGM_PRODUCTS_MAX_QUANTILES;
constexpr int kQuantPerLaunch = 8;           // 16 ranks: 16 prefixes, candidates and counters in registers (77 VGPRs)

// one launch's quantiles: x_(lo), x_(hi) and the weight g of x_(hi)
template <int NQ>
struct QuantGroup { int lo[NQ], hi[NQ]; double g[NQ]; };

// the key of a member: -0 is folded onto +0 before float_key, which alone would place it just below +0.  So the two zeros are
// one order statistic here, and a zero minimum, maximum or quantile is +0 in every map whichever zero the members held.
__device__ __forceinline__ unsigned int member_key(float v) {
    const unsigned int b = __float_as_uint(v);
    return float_key(__uint_as_float(b == 0x80000000u ? 0u : b));
}

__global__ __launch_bounds__(kThreads) void products_moments_kernel(const float* __restrict__ ens, const void* __restrict__ mask,
                                                                    int mask_u8, int M, size_t HW, int T, ThrList thr,
                                                                    float* __restrict__ mean, float* __restrict__ sdev,
                                                                    float* __restrict__ vmin, float* __restrict__ vmax,
                                                                    float* __restrict__ exceed, unsigned long long* __restrict__ count) {
    float th[kMaxThr];
#pragma unroll
    for (int t = 0; t < kMaxThr; ++t) th[t] = thr.v[t];                  // entries past T are 0: counted, never stored
    unsigned long long nvalid = 0;
    for (size_t p = (size_t)blockIdx.x * kThreads + threadIdx.x; p < HW; p += (size_t)gridDim.x * kThreads) {
        const float* col = ens + p;
        bool valid = mask_at(mask, mask_u8, p);
        double sum = 0.0, ss = 0.0;
        unsigned int kmin = 0xFFFFFFFFu, kmax = 0u;
        int k[kMaxThr];
#pragma unroll
        for (int t = 0; t < kMaxThr; ++t) k[t] = 0;
        if (valid) {
#pragma unroll 4
            for (int m = 0; m < M; ++m) {
                const float v = col[(size_t)m * HW];
                valid = valid && !is_nan(v);
                sum += (double)v;
                const unsigned int key = member_key(v);
                kmin = min(kmin, key);
                kmax = max(kmax, key);
#pragma unroll
                for (int t = 0; t < kMaxThr; ++t) k[t] += v >= th[t];
            }
        }
        const double mu = sum / (double)M;
        if (valid) {
#pragma unroll 4
            for (int m = 0; m < M; ++m) {
                const double d = (double)col[(size_t)m * HW] - mu;
                ss += d * d;
            }
        }
        nvalid += valid;
        mean[p] = valid ? (float)mu : nan_f();
        sdev[p] = valid ? (float)sqrt(ss / (double)(M - 1)) : nan_f();
        vmin[p] = valid ? key_float(kmin) : nan_f();
        vmax[p] = valid ? key_float(kmax) : nan_f();
#pragma unroll
        for (int t = 0; t < kMaxThr; ++t)
            if (t < T) exceed[(size_t)t * HW + p] = valid ? (float)((double)k[t] / (double)M) : nan_f();
    }
    nvalid = wave_sum_u64(nvalid);
    if ((threadIdx.x & 63) == 0 && nvalid) atomicAdd(count, nvalid);
}

// validity comes from the moments kernel, which ran before on the same stream: vmin is NaN exactly at the invalid pixels
template <int NQ>
__global__ __launch_bounds__(kThreads) void products_quantile_kernel(const float* __restrict__ ens, const float* __restrict__ vmin,
                                                                     int M, size_t HW, QuantGroup<NQ> qg,
                                                                     float* __restrict__ quant) {
    constexpr int S = 2 * NQ;
    for (size_t p = (size_t)blockIdx.x * kThreads + threadIdx.x; p < HW; p += (size_t)gridDim.x * kThreads) {
        if (is_nan(vmin[p])) {
#pragma unroll
            for (int j = 0; j < NQ; ++j) quant[(size_t)j * HW + p] = nan_f();
            continue;
        }
        const float* col = ens + p;
        unsigned int prefix[S];
#pragma unroll
        for (int s = 0; s < S; ++s) prefix[s] = 0u;
        for (int bit = 31; bit >= 0; --bit) {
            unsigned int cand[S], below[S];
#pragma unroll
            for (int s = 0; s < S; ++s) { cand[s] = prefix[s] | (1u << bit); below[s] = 0u; }
#pragma unroll 4
            for (int m = 0; m < M; ++m) {
                const unsigned int key = member_key(col[(size_t)m * HW]);
#pragma unroll
                for (int s = 0; s < S; ++s) below[s] += key < cand[s];
            }
#pragma unroll
            for (int j = 0; j < NQ; ++j) {
                prefix[2 * j] = below[2 * j] <= (unsigned int)qg.lo[j] ? cand[2 * j] : prefix[2 * j];
                prefix[2 * j + 1] = below[2 * j + 1] <= (unsigned int)qg.hi[j] ? cand[2 * j + 1] : prefix[2 * j + 1];
            }
        }
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            const float a = key_float(prefix[2 * j]), b = key_float(prefix[2 * j + 1]);
            const double g = qg.g[j];
            quant[(size_t)j * HW + p] = (g == 0.0 || a == b) ? a : (float)((double)a + g * ((double)b - (double)a));
        }
    }
}

template <int NQ>
int launch_quantiles(const float* ens, const float* vmin, int M, int64_t HW, const int* lo, const int* hi, const double* g,
                     float* quant, int blocks, hipStream_t st) {
    QuantGroup<NQ> qg;
    for (int j = 0; j < NQ; ++j) { qg.lo[j] = lo[j]; qg.hi[j] = hi[j]; qg.g[j] = g[j]; }
    hipLaunchKernelGGL(products_quantile_kernel<NQ>, dim3(blocks), dim3(kThreads), 0, st, ens, vmin, M, (size_t)HW, qg, quant);
    SBGM_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" {

int64_t sbgm_ensemble_products_workspace_bytes(int M, int64_t HW, int Q, int T) {
    (void)M; (void)HW; (void)Q; (void)T;
    return 0;                          // every statistic lives in registers; the query exists so callers size every score alike
}

int sbgm_ensemble_products(const float* ens, const void* mask, int mask_is_u8, int M, int64_t HW, const double* quantiles, int Q,
                           const float* thresholds, int T, float* mean, float* sdev, float* vmin, float* vmax, float* quant,
                           float* exceed, int64_t* count, void* workspace, void* stream) {
    (void)workspace;
    SBGM_CHECK(ens && mean && sdev && vmin && vmax && count, "ensemble_products: null argument");
    SBGM_CHECK(M >= 2 && M <= kMaxMembers, "ensemble_products: M=%d members (2..%d)", M, kMaxMembers);
    SBGM_CHECK(HW >= 1, "ensemble_products: HW=%lld", (long long)HW);
    SBGM_CHECK(Q >= 0 && Q <= kMaxQuant && (Q == 0 || (quantiles && quant)), "ensemble_products: %d quantiles (0..%d, with their "
               "levels and maps)", Q, kMaxQuant);
    SBGM_CHECK(T >= 0 && T <= kMaxThr && (T == 0 || (thresholds && exceed)), "ensemble_products: %d thresholds (0..%d, with their "
               "values and maps)", T, kMaxThr);
    ThrList thr;
    if (int rc = fill_thresholds("ensemble_products", thresholds, T, thr)) return rc;
    int lo[kMaxQuant], hi[kMaxQuant];
    double g[kMaxQuant];
    for (int q = 0; q < Q; ++q) {
        SBGM_CHECK(quantiles[q] >= 0.0 && quantiles[q] <= 1.0, "ensemble_products: quantile %d is outside [0, 1]", q);      // NaN fails
        const double h = quantiles[q] * (double)(M - 1), fl = std::floor(h);
        lo[q] = (int)fl;
        g[q] = h - fl;
        hi[q] = std::min(lo[q] + 1, M - 1);
    }
    if (int rc = sbgm_zero_async(count, sizeof(int64_t), ST)) return rc;
    const int blocks = (int)std::min<int64_t>((HW + kThreads - 1) / kThreads, kMaxBlocks);
    hipLaunchKernelGGL(products_moments_kernel, dim3(blocks), dim3(kThreads), 0, ST, ens, mask, mask_is_u8, M, (size_t)HW, T, thr, mean,
                       sdev, vmin, vmax, exceed, reinterpret_cast<unsigned long long*>(count));
    SBGM_LAUNCH_CHECK();
    const int launches = (Q + kQuantPerLaunch - 1) / kQuantPerLaunch;          // Q split evenly: 16 -> 8 + 8, 11 -> 6 + 5
    for (int q0 = 0, l = 0; l < launches; ++l) {
        const int nq = (Q - q0 + launches - l - 1) / (launches - l);
        float* out = quant + (size_t)q0 * HW;
        int rc = 1;
        switch (nq) {                                                         // one instance per count: no rank is carried in vain
#define SBGM_QUANT_CASE(NQ) case NQ: rc = launch_quantiles<NQ>(ens, vmin, M, HW, lo + q0, hi + q0, g + q0, out, blocks, ST); break;
            SBGM_QUANT_CASE(1) SBGM_QUANT_CASE(2) SBGM_QUANT_CASE(3) SBGM_QUANT_CASE(4)
            SBGM_QUANT_CASE(5) SBGM_QUANT_CASE(6) SBGM_QUANT_CASE(7) SBGM_QUANT_CASE(8)
#undef SBGM_QUANT_CASE
        }
        if (rc) return rc;
        q0 += nq;
    }
    return 0;
}

}  // extern "C"
