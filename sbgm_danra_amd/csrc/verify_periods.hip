// Period climate indices on the device: RxNday, RNNmm and PRCPTOT per pixel over the record and per period
// (year, season of a year, month of a year) of M member series gen [M][N][HW] and one truth series obs [N][HW].
//   K62 period_prepare — (a) one workgroup turns the day numbers and the period ids into one word per day, info[t] = id + 1
//                        (bits 0..8) | linked to day t - 1 (bit 9) | first day of its id (bit 10) | id differs from day t - 1's
//                        (bit 11), and used[P] (some day carries the id);  (b) the validity pass: day t is valid at pixel p when
//                        the mask admits it and obs and EVERY member are not NaN there, one bit per day and pixel in K55's
//                        layout (one uint32 per 32 days and pixel).  Validity is one map for all series, so every series sees the
//                        same days, the same run lengths and the same windows.
//   K63 period_sweep   — blockIdx.y = series (0..M-1 members, M = obs).  One pass in day order per pixel.  The run length
//                        r[t] = valid ? (linked ? r[t-1] : 0) + 1 : 0 is an integer; the last KMAX values (KMAX = 1, 8, 16 or 32,
//                        by the largest window) sit in a ring of registers whose slots are compile-time constants (the day loop is
//                        unrolled over the ring), so nothing is indexed dynamically and nothing goes to scratch.  A ring of up to 16
//                        slots holds the values widened to fp64 as they enter; the 32-slot ring holds them as fp32 and widens them
//                        where they are added.  Window K ending on day t exists iff r[t] >= K; its sum is formed from the ring,
//                        oldest day first, from +0.0, in fp64 — never by a sliding add and subtract, which is a different sum.
//                        The thread holds accumulators for the record and for the CURRENT period id only: where
//                        the id changes (uniform over the grid, ids are per day) it stores the current ones to slab [id] of the
//                        period outputs of its pixel and loads the new id's, or starts them fresh on the id's first day.  One
//                        thread owns the pixel, so the read-modify-write is race-free and costs a round trip per id change, not
//                        per day.  A window belongs to the period of its LAST day and may reach back into other ids.
//                        Between visits the window maxima rest in the fp32 output slab: rounding to fp32 is monotone, so
//                        round(max(round(a), b)) = max(round(a), round(b)) = round(max(a, b)) — the same value as keeping the
//                        fp64 maximum and rounding once at the end.  The wet-day sum is not a maximum: it rests as fp64 in the
//                        workspace.  NaN in a maximum means "no window yet".
//   K64 period_reduce  — per pixel and series: turns the resting wet-day sums into prcptot (NaN where the period has no valid
//                        day), fills the slabs of the ids no day carries (days 0, counts 0, NaN floats), then for every index the
//                        number n of counting periods (period_days >= min_days, value not NaN), their mean (fp64 sum of the fp32
//                        values in id order / n) and standard deviation sqrt(sum (v - mean)^2 / (n - 1)) against the unrounded mean.
// Lanes map to pixels (grid-stride), every day row is read coalesced, no atomics: two calls give bit-equal outputs.
// FP contraction is off: the fp64 expressions are the op sequences of the numpy restatement (tests/period_indices_ref.py).
#include <type_traits>

#include "verify_common.h"

#pragma clang fp contract(off)

#define ST ((hipStream_t)stream)

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;
constexpr int kMaxDays = SBGM_TEMPORAL_MAX_DAYS;
constexpr int kMaxWin = SBGM_PERIOD_MAX_WINDOWS;
constexpr int kMaxWindow = SBGM_PERIOD_MAX_WINDOW;
constexpr int kMaxThrP = SBGM_PERIOD_MAX_THRESHOLDS;
constexpr int kMaxPeriods = SBGM_PERIOD_MAX_PERIODS;
static_assert(kMaxPeriods <= kThreads, "K62 gives every period id a thread");

constexpr int kInfoIdMask = 0x1FF, kInfoLink = 1 << 9, kInfoFirst = 1 << 10, kInfoChange = 1 << 11;

struct WinList { int k[kMaxWin]; };
struct ThrListP { float v[kMaxThrP]; };

// K62 (a).  An id outside 0..P-1 counts as -1, so no slab index leaves [0, P).
__global__ __launch_bounds__(kThreads) void period_prepare_kernel(const int* __restrict__ day_numbers, const int* __restrict__ periods,
                                                                  int N, int P, int* __restrict__ info, int* __restrict__ used) {
    __shared__ int sid[kMaxDays];
    __shared__ int first_day[kMaxPeriods];
    const int tid = threadIdx.x;
    for (int t = tid; t < N; t += kThreads) {
        const int g = periods ? periods[t] : -1;
        sid[t] = (g >= 0 && g < P) ? g : -1;
    }
    __syncthreads();
    if (tid < P) {
        int f = -1;
        for (int t = 0; t < N; ++t)
            if (sid[t] == tid) { f = t; break; }
        first_day[tid] = f;
        used[tid] = f >= 0;
    }
    __syncthreads();
    for (int t = tid; t < N; t += kThreads) {
        const bool link = t > 0 && (!day_numbers || (long long)day_numbers[t] == (long long)day_numbers[t - 1] + 1);
        const int g = sid[t];
        const bool first = g >= 0 && first_day[g] == t;
        const bool change = t == 0 || g != sid[t - 1];
        info[t] = (g + 1) | (link ? kInfoLink : 0) | (first ? kInfoFirst : 0) | (change ? kInfoChange : 0);
    }
}

// K62 (b).  blockIdx.y = the word of 32 days; member m of day t is at gen + m * member_stride + t * day_stride.
__global__ __launch_bounds__(kThreads) void period_valid_kernel(const float* __restrict__ gen, size_t member_stride, size_t day_stride,
                                                                const float* __restrict__ obs, const void* __restrict__ mask,
                                                                int mask_u8, int mask_daily, int N, int M, size_t HW,
                                                                unsigned int* __restrict__ vbits) {
    const int word = blockIdx.y, t0 = word * 32, tn = min(32, N - t0);
    for (size_t p = (size_t)blockIdx.x * kThreads + threadIdx.x; p < HW; p += (size_t)gridDim.x * kThreads) {
        const bool admitted = mask_daily || mask_at(mask, mask_u8, p);
        unsigned int bits = 0u;
        for (int j = 0; j < tn; ++j) {
            const size_t t = (size_t)(t0 + j);
            bool valid = admitted && !is_nan(obs[t * HW + p]) && (!mask_daily || mask_at(mask, mask_u8, t * HW + p));
            const float* g = gen + t * day_stride + p;
#pragma unroll 4
            for (int m = 0; m < M; ++m) valid = valid && !is_nan(g[(size_t)m * member_stride]);
            bits |= (unsigned int)valid << j;
        }
        vbits[(size_t)word * HW + p] = bits;
    }
}

// the accumulators of the record, or of the current period
struct Acc {
    double best[kMaxWin];
    double sum;
    int cnt[kMaxThrP];
    int days;

    __device__ __forceinline__ void fresh() {
#pragma unroll
        for (int k = 0; k < kMaxWin; ++k) best[k] = nan_d();
#pragma unroll
        for (int j = 0; j < kMaxThrP; ++j) cnt[j] = 0;
        sum = 0.0;
        days = 0;
    }
    // the largest sum so far; NaN = none yet
    __device__ __forceinline__ void window(int k, double S) { best[k] = (best[k] != best[k] || S > best[k]) ? S : best[k]; }
};

struct SweepArgs {
    const float* gen;
    size_t member_stride, day_stride;
    const float* obs;
    const unsigned int* vbits;
    const int* info;
    int N, M, Kw, T, P;
    size_t HW;
    float wet;
    WinList win;
    ThrListP thr;
    int* days;              // [HW]
    float* rx;              // [M + 1][Kw][HW]
    int* count;             // [M + 1][T][HW]
    float* prcptot;         // [M + 1][HW]
    int* period_days;       // [P][HW]
    float* period_rx;       // [M + 1][P][Kw][HW]
    int* period_count;      // [M + 1][P][T][HW]
    double* period_sum;     // [M + 1][P][HW], workspace
};

// K63.  KMAX = the ring: the largest window rounded up to 1, 8, 16 or 32; CH = the days of one unrolled chunk, a multiple of
// KMAX that divides 32, so a chunk lies within one word of validity bits and day j of a chunk always owns ring slot j % KMAX.
template <int KMAX, bool PER>
__global__ __launch_bounds__(kThreads) void period_sweep_kernel(SweepArgs a) {
    constexpr int CH = KMAX < 16 ? 16 : KMAX;
    const int s = blockIdx.y;
    const bool is_obs = s == a.M;
    const float* x = is_obs ? a.obs : a.gen + (size_t)s * a.member_stride;
    const size_t dstride = is_obs ? a.HW : a.day_stride;
    const size_t HW = a.HW;
    const int N = a.N, Kw = a.Kw, T = a.T, P = a.P;
    for (size_t p = (size_t)blockIdx.x * kThreads + threadIdx.x; p < HW; p += (size_t)gridDim.x * kThreads) {
        const float* col = x + p;
        const unsigned int* vb = a.vbits + p;
        float* prx = PER ? a.period_rx + (size_t)s * P * Kw * HW + p : nullptr;
        int* pcnt = PER ? a.period_count + (size_t)s * P * T * HW + p : nullptr;
        double* psum = PER ? a.period_sum + (size_t)s * P * HW + p : nullptr;
        // up to 16 slots the ring holds the values widened once, on entry; the 32-slot ring stays fp32 and widens on use (64
        // more registers would halve the occupancy)
        using ring_t = typename std::conditional<KMAX <= 16, double, float>::type;
        ring_t ring[KMAX];
#pragma unroll
        for (int i = 0; i < KMAX; ++i) ring[i] = (ring_t)0;
        Acc rec, cur;
        rec.fresh();
        cur.fresh();
        int r = 0, cur_id = -1;

        auto store_cur = [&]() {                                               // cur_id is in [0, P)
            const size_t g = (size_t)cur_id;
#pragma unroll
            for (int k = 0; k < kMaxWin; ++k)
                if (k < Kw) prx[(g * Kw + k) * HW] = (float)cur.best[k];
#pragma unroll
            for (int j = 0; j < kMaxThrP; ++j)
                if (j < T) pcnt[(g * T + j) * HW] = cur.cnt[j];
            psum[g * HW] = cur.sum;
            if (is_obs) a.period_days[g * HW + p] = cur.days;
        };

        for (int t0 = 0; t0 < N; t0 += CH) {
            const unsigned int bits = vb[(size_t)(t0 >> 5) * HW] >> (t0 & 31);
            float v[CH];
#pragma unroll
            for (int j = 0; j < CH; ++j) v[j] = t0 + j < N ? col[(size_t)(t0 + j) * dstride] : 0.f;
#pragma unroll
            for (int j = 0; j < CH; ++j) {
                const int t = t0 + j;
                if (t >= N) continue;                                        // the tail of the last chunk
                const int info = a.info[t];
                if (PER && (info & kInfoChange)) {
                    if (cur_id >= 0) store_cur();
                    cur_id = (info & kInfoIdMask) - 1;
                    cur.fresh();
                    if (cur_id >= 0 && !(info & kInfoFirst)) {
                        const size_t g = (size_t)cur_id;
#pragma unroll
                        for (int k = 0; k < kMaxWin; ++k)
                            if (k < Kw) cur.best[k] = (double)prx[(g * Kw + k) * HW];
#pragma unroll
                        for (int jj = 0; jj < kMaxThrP; ++jj)
                            if (jj < T) cur.cnt[jj] = pcnt[(g * T + jj) * HW];
                        cur.sum = psum[g * HW];
                        if (is_obs) cur.days = a.period_days[g * HW + p];
                    }
                }
                const bool valid = (bits >> j) & 1u;
                const float xv = v[j];
                ring[j % KMAX] = (ring_t)xv;
                r = valid ? ((info & kInfoLink) ? r : 0) + 1 : 0;
                if (valid) {
                    ++rec.days;
                    if (PER) ++cur.days;
#pragma unroll
                    for (int jj = 0; jj < kMaxThrP; ++jj)
                        if (jj < T) {
                            const int c = xv >= a.thr.v[jj];
                            rec.cnt[jj] += c;
                            if (PER) cur.cnt[jj] += c;
                        }
                    if (xv >= a.wet) {
                        rec.sum += (double)xv;
                        if (PER) cur.sum += (double)xv;
                    }
                }
                // The window sums, for every lane alike (K is uniform; a lane without the window drops its sum below): one switch
                // into a chain of adds, day t - K + 1 first, so the adds are straight-line and every slot is a constant.
#pragma unroll
                for (int k = 0; k < kMaxWin; ++k)
                    if (k < Kw) {
                        const int K = a.win.k[k];
                        double S = 0.0;
#define SBGM_WINDOW_DAY(I) case (I) + 1: if ((I) < KMAX) S += (double)ring[(j - (I) + 2 * kMaxWindow) % KMAX]; [[fallthrough]];
                        if (KMAX > 16) {                                     // the chain of 32 is too long to enter by a switch
#pragma unroll
                            for (int i = KMAX - 1; i >= 0; --i)
                                if (i < K) S += (double)ring[(j - i + 2 * kMaxWindow) % KMAX];
                        } else
                        switch (K) {
                            SBGM_WINDOW_DAY(31) SBGM_WINDOW_DAY(30) SBGM_WINDOW_DAY(29) SBGM_WINDOW_DAY(28) SBGM_WINDOW_DAY(27)
                            SBGM_WINDOW_DAY(26) SBGM_WINDOW_DAY(25) SBGM_WINDOW_DAY(24) SBGM_WINDOW_DAY(23) SBGM_WINDOW_DAY(22)
                            SBGM_WINDOW_DAY(21) SBGM_WINDOW_DAY(20) SBGM_WINDOW_DAY(19) SBGM_WINDOW_DAY(18) SBGM_WINDOW_DAY(17)
                            SBGM_WINDOW_DAY(16) SBGM_WINDOW_DAY(15) SBGM_WINDOW_DAY(14) SBGM_WINDOW_DAY(13) SBGM_WINDOW_DAY(12)
                            SBGM_WINDOW_DAY(11) SBGM_WINDOW_DAY(10) SBGM_WINDOW_DAY(9) SBGM_WINDOW_DAY(8) SBGM_WINDOW_DAY(7)
                            SBGM_WINDOW_DAY(6) SBGM_WINDOW_DAY(5) SBGM_WINDOW_DAY(4) SBGM_WINDOW_DAY(3) SBGM_WINDOW_DAY(2)
                            SBGM_WINDOW_DAY(1) SBGM_WINDOW_DAY(0)
                            default: break;
                        }
#undef SBGM_WINDOW_DAY
                        if (r >= K) {                                        // r >= 1 only on a valid day
                            rec.window(k, S);
                            if (PER) cur.window(k, S);
                        }
                    }
            }
        }
        if (PER && cur_id >= 0) store_cur();
        if (is_obs) a.days[p] = rec.days;
#pragma unroll
        for (int k = 0; k < kMaxWin; ++k)
            if (k < Kw) a.rx[((size_t)s * Kw + k) * HW + p] = (float)rec.best[k];
#pragma unroll
        for (int j = 0; j < kMaxThrP; ++j)
            if (j < T) a.count[((size_t)s * T + j) * HW + p] = rec.cnt[j];
        a.prcptot[(size_t)s * HW + p] = rec.days > 0 ? (float)rec.sum : nan_f();
    }
}

struct ReduceArgs {
    const int* used;            // [P]
    int M, Kw, T, P, min_days;
    size_t HW;
    int* period_days;           // [P][HW]
    float* period_rx;           // [M + 1][P][Kw][HW]
    int* period_count;          // [M + 1][P][T][HW]
    float* period_prcptot;      // [M + 1][P][HW]
    const double* period_sum;   // [M + 1][P][HW]
    int* across_n;              // [M + 1][Kw + T + 1][HW]
    float* across_mean;
    float* across_std;
};

// K64.  blockIdx.y = series.  Index i of the across-period axis: the Kw windows, the T thresholds, prcptot.
__global__ __launch_bounds__(kThreads) void period_reduce_kernel(ReduceArgs a) {
    const int s = blockIdx.y, Kw = a.Kw, T = a.T, P = a.P, I = Kw + T + 1;
    const size_t HW = a.HW;
    const bool is_obs = s == a.M;
    for (size_t p = (size_t)blockIdx.x * kThreads + threadIdx.x; p < HW; p += (size_t)gridDim.x * kThreads) {
        float* prx = a.period_rx + (size_t)s * P * Kw * HW + p;
        int* pcnt = a.period_count + (size_t)s * P * T * HW + p;
        float* pprc = a.period_prcptot + (size_t)s * P * HW + p;
        const double* psum = a.period_sum + (size_t)s * P * HW + p;
        for (int g = 0; g < P; ++g) {
            if (a.used[g]) {
                pprc[(size_t)g * HW] = a.period_days[(size_t)g * HW + p] > 0 ? (float)psum[(size_t)g * HW] : nan_f();
            } else {                                                            // no day carries this id: nothing wrote its slabs
                if (is_obs) a.period_days[(size_t)g * HW + p] = 0;
                for (int k = 0; k < Kw; ++k) prx[((size_t)g * Kw + k) * HW] = nan_f();
                for (int j = 0; j < T; ++j) pcnt[((size_t)g * T + j) * HW] = 0;
                pprc[(size_t)g * HW] = nan_f();
            }
        }
        for (int i = 0; i < I; ++i) {
            // value of period g for index i, as the double that enters the sums; NaN = does not count
            auto value = [&](int g) -> double {
                if (!a.used[g] || a.period_days[(size_t)g * HW + p] < a.min_days) return nan_d();
                if (i < Kw) return (double)prx[((size_t)g * Kw + i) * HW];
                if (i < Kw + T) return (double)pcnt[((size_t)g * T + (i - Kw)) * HW];
                return (double)pprc[(size_t)g * HW];
            };
            int n = 0;
            double sum = 0.0;
            for (int g = 0; g < P; ++g) {
                const double v = value(g);
                if (v == v) { sum += v; ++n; }
            }
            const double mean = sum / (double)n;                                // n = 0: never used
            double ss = 0.0;
            for (int g = 0; g < P; ++g) {
                const double v = value(g);
                if (v == v) { const double d = v - mean; ss += d * d; }
            }
            const size_t o = ((size_t)s * I + i) * HW + p;
            a.across_n[o] = n;
            a.across_mean[o] = n > 0 ? (float)mean : nan_f();
            a.across_std[o] = n > 1 ? (float)sqrt(ss / (double)(n - 1)) : nan_f();
        }
    }
}

bool sizes_ok(int N, int M, int H, int W, int Kw, int T, int P) {
    return N >= 2 && N <= kMaxDays && M >= 1 && M <= SBGM_PERIOD_MAX_MEMBERS && field_shape_ok(N, H, W) && Kw >= 1 && Kw <= kMaxWin &&
           T >= 0 && T <= kMaxThrP && P >= 0 && P <= kMaxPeriods;
}

int64_t vbit_words(int N) { return (N + 31) / 32; }

template <int KMAX>
void launch_sweep(bool per, dim3 grid, hipStream_t st, const SweepArgs& a) {
    if (per) hipLaunchKernelGGL((period_sweep_kernel<KMAX, true>), grid, dim3(kThreads), 0, st, a);
    else hipLaunchKernelGGL((period_sweep_kernel<KMAX, false>), grid, dim3(kThreads), 0, st, a);
}

}  // namespace

extern "C" {

int64_t sbgm_period_indices_workspace_bytes(int N, int M, int H, int W, int Kw, int T, int P) {
    if (!sizes_ok(N, M, H, W, Kw, T, P)) return 0;
    const int64_t HW = (int64_t)H * W;
    // the resting wet-day sums [M + 1][P][HW] fp64, the validity bits, info[N] and used[P]
    return (int64_t)(M + 1) * P * HW * (int64_t)sizeof(double) + vbit_words(N) * HW * (int64_t)sizeof(unsigned int) +
           ((int64_t)N + P) * (int64_t)sizeof(int);
}

int sbgm_period_indices(const float* gen, int64_t member_stride, int64_t day_stride, const float* obs, const void* mask,
                        int mask_is_u8, int N, int Nm, int M, int H, int W, const int* windows, int Kw, const float* thresholds,
                        int T, float wet, int min_days, const int* day_numbers, const int* periods, int P, int* days, float* rx,
                        int* count, float* prcptot, int* period_days, float* period_rx, int* period_count, float* period_prcptot,
                        int* across_n, float* across_mean, float* across_std, void* workspace, int64_t workspace_bytes,
                        void* stream) {
    SBGM_CHECK(gen && obs && days && rx && prcptot && workspace, "period_indices: null argument");
    SBGM_CHECK(N >= 2 && N <= kMaxDays, "period_indices: N=%d days (2..%d)", N, kMaxDays);
    SBGM_CHECK(M >= 1 && M <= SBGM_PERIOD_MAX_MEMBERS, "period_indices: M=%d members (1..%d)", M, SBGM_PERIOD_MAX_MEMBERS);
    SBGM_CHECK(field_shape_ok(N, H, W), "period_indices: field size %dx%d (sides 2..%d, H*W <= 2^20)", H, W, kMaxSide);
    const int64_t HW = (int64_t)H * W;
    SBGM_CHECK(day_stride >= HW && (M == 1 || member_stride >= HW), "period_indices: strides %lld (member), %lld (day) are below "
               "H*W = %lld", (long long)member_stride, (long long)day_stride, (long long)HW);
    SBGM_CHECK(!mask || Nm == 1 || Nm == N, "period_indices: mask of %d fields (1 or %d)", Nm, N);
    SBGM_CHECK(Kw >= 1 && Kw <= kMaxWin && windows, "period_indices: %d windows (1..%d, with their lengths)", Kw, kMaxWin);
    WinList win{};
    for (int k = 0; k < Kw; ++k) {
        SBGM_CHECK(windows[k] >= 1 && windows[k] <= kMaxWindow, "period_indices: window %d is %d days (1..%d)", k, windows[k],
                   kMaxWindow);
        SBGM_CHECK(k == 0 || windows[k] > windows[k - 1], "period_indices: the windows must be distinct and ascending (window %d "
                   "is %d after %d)", k, windows[k], windows[k - 1]);
        win.k[k] = windows[k];
    }
    SBGM_CHECK(T >= 0 && T <= kMaxThrP && (T == 0 || (thresholds && count)), "period_indices: %d thresholds (0..%d, with their "
               "values and maps)", T, kMaxThrP);
    ThrListP thr{};
    for (int j = 0; j < T; ++j) {
        SBGM_CHECK(std::isfinite(thresholds[j]), "period_indices: threshold %d is not finite", j);
        thr.v[j] = thresholds[j];
    }
    SBGM_CHECK(std::isfinite(wet), "period_indices: the wet-day threshold is not finite");
    SBGM_CHECK(min_days >= 1, "period_indices: min_days=%d (>= 1)", min_days);
    SBGM_CHECK(P >= 0 && P <= kMaxPeriods && (P > 0) == (periods != nullptr), "period_indices: P=%d periods (0 without ids, else "
               "1..%d)", P, kMaxPeriods);
    SBGM_CHECK(P == 0 || (period_days && period_rx && period_prcptot && (T == 0 || period_count) && across_n && across_mean &&
                          across_std), "period_indices: null period output");
    const int64_t need = sbgm_period_indices_workspace_bytes(N, M, H, W, Kw, T, P);
    SBGM_CHECK(workspace_bytes >= need, "period_indices: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
               (long long)need);

    double* period_sum = static_cast<double*>(workspace);
    unsigned int* vbits = reinterpret_cast<unsigned int*>(period_sum + (size_t)(M + 1) * P * HW);
    int* info = reinterpret_cast<int*>(vbits + vbit_words(N) * HW);
    int* used = info + N;
    const int blocks = (int)std::min<int64_t>((HW + kThreads - 1) / kThreads, kMaxBlocks);

    hipLaunchKernelGGL(period_prepare_kernel, dim3(1), dim3(kThreads), 0, ST, day_numbers, periods, N, P, info, used);
    SBGM_LAUNCH_CHECK();
    hipLaunchKernelGGL(period_valid_kernel, dim3(blocks, (int)vbit_words(N)), dim3(kThreads), 0, ST, gen, (size_t)member_stride,
                       (size_t)day_stride, obs, mask, mask_is_u8, (int)(mask && Nm == N && N > 1), N, M, (size_t)HW, vbits);
    SBGM_LAUNCH_CHECK();

    SweepArgs a{};
    a.gen = gen; a.member_stride = (size_t)member_stride; a.day_stride = (size_t)day_stride; a.obs = obs; a.vbits = vbits;
    a.info = info; a.N = N; a.M = M; a.Kw = Kw; a.T = T; a.P = P; a.HW = (size_t)HW; a.wet = wet; a.win = win; a.thr = thr;
    a.days = days; a.rx = rx; a.count = count; a.prcptot = prcptot; a.period_days = period_days; a.period_rx = period_rx;
    a.period_count = period_count; a.period_sum = period_sum;
    const dim3 grid(blocks, M + 1);
    const int kmax = win.k[Kw - 1];
    if (kmax <= 1) launch_sweep<1>(P > 0, grid, ST, a);
    else if (kmax <= 8) launch_sweep<8>(P > 0, grid, ST, a);
    else if (kmax <= 16) launch_sweep<16>(P > 0, grid, ST, a);
    else launch_sweep<32>(P > 0, grid, ST, a);
    SBGM_LAUNCH_CHECK();

    if (P > 0) {
        ReduceArgs ra{used, M, Kw, T, P, min_days, (size_t)HW, period_days, period_rx, period_count, period_prcptot, period_sum,
                      across_n, across_mean, across_std};
        hipLaunchKernelGGL(period_reduce_kernel, grid, dim3(kThreads), 0, ST, ra);
        SBGM_LAUNCH_CHECK();
    }
    return 0;
}

}  // extern "C"
