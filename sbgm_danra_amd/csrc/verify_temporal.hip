// Climate indices over time on the device: per pixel of gen [N][HW] against obs [N][HW], along the day axis,
//   K55 climate_moments  — both sides in one kernel, because validity is paired (a day counts where gen AND obs are not NaN
//                          and the mask admits it).  Sweep 1 over the days: validity, n, n_wet, the fp64 sums (all valid days;
//                          wet days), the maximum key, the running and longest wet / dry spells, the four transition counts.
//                          Sweep 2: sum (x - mu)^2 and sum (x_t - mu)(x_t+1 - mu) in fp64 against the unrounded mean.  Sweep
//                          1 also leaves the validity bits (one uint32 per 32 days and pixel) and n_wet in the workspace.
//   K56 climate_select   — type-7 quantiles by K47's bitwise bisection on the order-preserving key.  Two differences from K47:
//                          the ranks lo, hi and the weight g are per pixel (n and n_wet vary), and a day that does not take
//                          part (invalid, or dry when the ranks are wet-day ranks) gets key 0xFFFFFFFF, so it is never counted
//                          below a candidate.  That key is a NaN's, no valid value owns it.  One launch covers both sides
//                          (blockIdx.y) and one level list; the all-day and the wet-day levels take a launch each.
//   K57 climate_heavy    — sum of x over the valid days with x > tau against the sum over the valid wet days, tau = the obs
//                          side's wet-day quantile map; it runs after K56 wrote that map.
// Lanes map to pixels (grid-stride), so every day row is read coalesced, as K43, K46 and K47 read theirs.  K56 and K57 read
// their own side only: validity comes from the bits, 1/32 of the traffic of a second row.
// Calendar and groups (sbgm_climate_indices_calendar): K61 climate_prepare, one workgroup, turns the day numbers and the group
// ids into three tables in the workspace: link[t] (day t is the calendar day after day t - 1), order (the days 0..N-1, then the
// days in a stable counting sort by group) and start[G+2] (slab s walks order[start[s]..start[s+1])).  K55 - K57 are templates
// on CAL: with it they take the slab from the grid (slab 0 = all days, slab 1 + g = group g) and walk their slab's list, so
// over all group slabs a sweep reads every day row once.  Position i is linked to i - 1 iff order[i] == order[i-1] + 1 and
// link[order[i]]; at a broken link prev_valid and both runs are reset before the day is taken, which is what one invalid day
// between the two does.  Only slab 0 writes the validity bits (keyed by day t); the group slabs of K55 run in the same
// launch and recompute validity; K56 and K57 read the bit of the day they visit (slab 0's list is the identity, so there they
// keep the plain loop over words of 32 days).  Without CAL the kernels are the code they were: no table is read.
// Reproducibility: no atomics at all; every sum runs in day order in one thread.
// FP contraction is off in this file, as in verify_products.hip: the fp64 expressions are the op sequences of the numpy
// restatement (tests/climate_ref.py).
#include "verify_common.h"

#pragma clang fp contract(off)

#define ST ((hipStream_t)stream)

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;
constexpr int kMaxDays = SBGM_TEMPORAL_MAX_DAYS;
constexpr int kMaxQuant = SBGM_TEMPORAL_MAX_QUANTILES;
constexpr int kStats = SBGM_TEMPORAL_STATS;
constexpr int kMaxGroups = SBGM_TEMPORAL_MAX_GROUPS;

struct Levels { double q[kMaxQuant]; };

// the key of a day's value: -0 folded onto +0 before float_key, as K47 folds its members
__device__ __forceinline__ unsigned int day_key(float v) {
    const unsigned int b = __float_as_uint(v);
    return float_key(__uint_as_float(b == 0x80000000u ? 0u : b));
}

__device__ __forceinline__ float ratio_f(double num, double den, bool defined) {
    return defined ? (float)(num / den) : nan_f();
}

// the running state of one side in sweep 1
struct SideSweep {
    double sum = 0.0, sum_wet = 0.0;
    unsigned int kmax = 0u;
    int n_wet = 0, run_wet = 0, run_dry = 0, cwd = 0, cdd = 0, ww = 0, wd = 0, dw = 0, dd = 0;
    bool prev_wet = false;

    __device__ __forceinline__ void end_runs() { run_wet = run_dry = 0; }

    __device__ __forceinline__ void day(float v, bool valid, bool pair, float wet_thr) {
        const bool wet = v >= wet_thr;
        if (valid) {
            sum += (double)v;
            kmax = max(kmax, day_key(v));
            if (wet) { sum_wet += (double)v; ++n_wet; }
        }
        run_wet = (valid && wet) ? run_wet + 1 : 0;
        run_dry = (valid && !wet) ? run_dry + 1 : 0;
        cwd = max(cwd, run_wet);
        cdd = max(cdd, run_dry);
        if (pair) {
            ww += prev_wet && wet;
            wd += prev_wet && !wet;
            dw += !prev_wet && wet;
            dd += !prev_wet && !wet;
        }
        prev_wet = wet;
    }
};

// the tables of K61 and the outputs of the group slabs ([G] leading axis on each)
struct Calendar {
    const int* order;        // [2N]
    const int* start;        // [G + 2]
    const int* link;         // [N]
    int* days;               // [G][HW]
    float* stats;            // [G][2][kStats][HW]
    int* spells;             // [G][2][2][HW]
    int* transitions;        // [G][2][4][HW]
};

// One workgroup.  A day whose id is outside 0..G-1 joins no group list (its LDS id is -1), so the lists hold at most N days
// in all and every write stays inside order[2N].
__global__ __launch_bounds__(kThreads) void climate_prepare_kernel(const int* __restrict__ day_numbers, const int* __restrict__ groups,
                                                                   int N, int G, int* __restrict__ order, int* __restrict__ start,
                                                                   int* __restrict__ link) {
    __shared__ int gid[kMaxDays];
    __shared__ int count[kMaxGroups];
    const int tid = threadIdx.x;
    for (int t = tid; t < N; t += kThreads) {
        link[t] = t > 0 && (!day_numbers || (long long)day_numbers[t] == (long long)day_numbers[t - 1] + 1);
        order[t] = t;
        const int g = groups ? groups[t] : -1;
        gid[t] = (g >= 0 && g < G) ? g : -1;
    }
    __syncthreads();
    if (tid < G) {
        int c = 0;
        for (int t = 0; t < N; ++t) c += gid[t] == tid;
        count[tid] = c;
    }
    __syncthreads();
    if (tid == 0) {
        start[0] = 0;
        int at = N;
        for (int g = 0; g < G; ++g) { start[1 + g] = at; at += count[g]; }
        start[1 + G] = at;
    }
    if (tid < G) {
        int at = N;
        for (int g = 0; g < tid; ++g) at += count[g];
        for (int t = 0; t < N; ++t)
            if (gid[t] == tid) order[at++] = t;
    }
}

template <bool CAL>
__global__ __launch_bounds__(kThreads) void climate_moments_kernel(const float* __restrict__ gen, const float* __restrict__ obs,
                                                                   const void* __restrict__ mask, int mask_u8, int mask_daily, int N,
                                                                   size_t HW, float wet, int* __restrict__ days,
                                                                   float* __restrict__ stats, int* __restrict__ spells,
                                                                   int* __restrict__ transitions, unsigned int* __restrict__ vbits,
                                                                   int* __restrict__ nwet, Calendar cal) {
    const int slab = CAL ? blockIdx.y : 0;
    const int lo = CAL ? cal.start[slab] : 0, hi = CAL ? cal.start[slab + 1] : N;
    if (CAL && slab > 0) {                                                    // group slab - 1: its own output maps
        const size_t g = (size_t)(slab - 1);
        days = cal.days + g * HW;
        stats = cal.stats + g * 2 * kStats * HW;
        spells = cal.spells + g * 4 * HW;
        transitions = cal.transitions + g * 8 * HW;
    }
    nwet += (size_t)slab * 2 * HW;
    for (size_t p = (size_t)blockIdx.x * kThreads + threadIdx.x; p < HW; p += (size_t)gridDim.x * kThreads) {
        const bool admitted = mask_daily || mask_at(mask, mask_u8, p);
        SideSweep s[2];
        int n = 0;
        bool prev_valid = false;
        unsigned int bits = 0u;
        int tprev = -2;
        for (int k = lo; k < hi; ++k) {
            const int t = CAL ? cal.order[k] : k;
            if (CAL && !(t == tprev + 1 && cal.link[t])) {                  // a broken link: as one invalid day in between
                prev_valid = false;
                s[0].end_runs();
                s[1].end_runs();
            }
            tprev = t;
            const size_t i = (size_t)t * HW + p;
            const float g = gen[i], o = obs[i];
            const bool valid = admitted && !is_nan(g) && !is_nan(o) && (!mask_daily || mask_at(mask, mask_u8, i));
            const bool pair = valid && prev_valid;
            n += valid;
            s[0].day(g, valid, pair, wet);
            s[1].day(o, valid, pair, wet);
            prev_valid = valid;
            if (!CAL || slab == 0) {                                          // slab 0 walks t = 0..N-1 in order
                bits |= (unsigned int)valid << (t & 31);
                if ((t & 31) == 31 || t == N - 1) {
                    vbits[(size_t)(t >> 5) * HW + p] = bits;
                    bits = 0u;
                }
            }
        }
        const double mu[2] = {s[0].sum / (double)n, s[1].sum / (double)n};          // n = 0: never used
        double c0[2] = {0.0, 0.0}, c1[2] = {0.0, 0.0}, dprev[2] = {0.0, 0.0};
        prev_valid = false;
        tprev = -2;
        for (int k = lo; k < hi; ++k) {
            const int t = CAL ? cal.order[k] : k;
            if (CAL && !(t == tprev + 1 && cal.link[t])) prev_valid = false;
            tprev = t;
            const size_t i = (size_t)t * HW + p;
            const float g = gen[i], o = obs[i];
            const bool valid = admitted && !is_nan(g) && !is_nan(o) && (!mask_daily || mask_at(mask, mask_u8, i));
            const double d[2] = {(double)g - mu[0], (double)o - mu[1]};
#pragma unroll
            for (int side = 0; side < 2; ++side) {
                if (valid) c0[side] += d[side] * d[side];
                if (valid && prev_valid) c1[side] += dprev[side] * d[side];
                dprev[side] = d[side];
            }
            prev_valid = valid;
        }
        days[p] = n;
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            const SideSweep& a = s[side];
            float* st = stats + (size_t)side * kStats * HW + p;
            const int n_pairs = a.ww + a.wd + a.dw + a.dd;
            const double var0 = c0[side] / (double)n, cov1 = c1[side] / (double)n_pairs;
            st[(size_t)SBGM_TEMPORAL_STAT_MEAN * HW] = n > 0 ? (float)mu[side] : nan_f();
            st[(size_t)SBGM_TEMPORAL_STAT_WET_FREQ * HW] = ratio_f((double)a.n_wet, (double)n, n > 0);
            st[(size_t)SBGM_TEMPORAL_STAT_SDII * HW] = ratio_f(a.sum_wet, (double)a.n_wet, a.n_wet > 0);
            st[(size_t)SBGM_TEMPORAL_STAT_MAX * HW] = n > 0 ? key_float(a.kmax) : nan_f();
            st[(size_t)SBGM_TEMPORAL_STAT_P_WW * HW] = ratio_f((double)a.ww, (double)(a.ww + a.wd), a.ww + a.wd > 0);
            st[(size_t)SBGM_TEMPORAL_STAT_P_DW * HW] = ratio_f((double)a.dw, (double)(a.dw + a.dd), a.dw + a.dd > 0);
            st[(size_t)SBGM_TEMPORAL_STAT_LAG1 * HW] = ratio_f(cov1, var0, n_pairs > 0 && var0 != 0.0);
            spells[((size_t)side * 2 + 0) * HW + p] = a.cwd;
            spells[((size_t)side * 2 + 1) * HW + p] = a.cdd;
            int* tr = transitions + (size_t)side * 4 * HW + p;
            tr[0] = a.ww;
            tr[HW] = a.wd;
            tr[2 * HW] = a.dw;
            tr[3 * HW] = a.dd;
            nwet[(size_t)side * HW + p] = a.n_wet;
        }
    }
}

// the validity bit of day t of one pixel (vb = vbits + p) on a walk over ascending days: the word is kept while it serves
struct ValidWord {
    int word = -1;
    unsigned int bits = 0u;

    __device__ __forceinline__ bool at(const unsigned int* __restrict__ vb, size_t HW, int t) {
        if ((t >> 5) != word) {
            word = t >> 5;
            bits = vb[(size_t)word * HW];
        }
        return (bits >> (t & 31)) & 1u;
    }
};

// blockIdx.y = side, with CAL blockIdx.z = slab (quant, days and nwet then hold the slabs one after the other).  `x` is gen
// (side 0) or obs (side 1); count = days (all-day ranks) or the side's n_wet (wet-day ranks)
template <int NQ, bool CAL>
__global__ __launch_bounds__(kThreads) void climate_select_kernel(const float* __restrict__ gen, const float* __restrict__ obs,
                                                                  const unsigned int* __restrict__ vbits,
                                                                  const int* __restrict__ days, const int* __restrict__ nwet,
                                                                  float* __restrict__ cal_quant, int wet_only, float wet, int N, size_t HW, Levels lv,
                                                                  float* __restrict__ quant, Calendar cal) {
    constexpr int S = 2 * NQ;
    const int side = blockIdx.y, slab = CAL ? blockIdx.z : 0;
    const int lo = CAL ? cal.start[slab] : 0, hi = CAL ? cal.start[slab + 1] : N;
    if (CAL && slab > 0) {
        days = cal.days + (size_t)(slab - 1) * HW;
        quant = cal_quant + (size_t)(slab - 1) * 2 * NQ * HW;
    }
    nwet += (size_t)slab * 2 * HW;
    const float* x = side ? obs : gen;
    const int* count = wet_only ? nwet + (size_t)side * HW : days;
    float* out = quant + (size_t)side * NQ * HW;
    const float wet_thr = wet_only ? wet : -INFINITY;                 // every valid value is >= -inf
    for (size_t p = (size_t)blockIdx.x * kThreads + threadIdx.x; p < HW; p += (size_t)gridDim.x * kThreads) {
        const int n = count[p];
        if (n <= 0) {
#pragma unroll
            for (int j = 0; j < NQ; ++j) out[(size_t)j * HW + p] = nan_f();
            continue;
        }
        unsigned int rank[S], prefix[S];
        double g[NQ];
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            const double h = lv.q[j] * (double)(n - 1), fl = floor(h);
            g[j] = h - fl;
            rank[2 * j] = (unsigned int)fl;
            rank[2 * j + 1] = (unsigned int)min((int)fl + 1, n - 1);
            prefix[2 * j] = prefix[2 * j + 1] = 0u;
        }
        const float* col = x + p;
        const unsigned int* vb = vbits + p;
        for (int bit = 31; bit >= 0; --bit) {
            unsigned int cand[S], below[S];
#pragma unroll
            for (int s = 0; s < S; ++s) { cand[s] = prefix[s] | (1u << bit); below[s] = 0u; }
            if (CAL && slab > 0) {                                            // a group's list; the word of day t is kept while it serves
                ValidWord vw;
#pragma unroll 4
                for (int k = lo; k < hi; ++k) {
                    const int t = cal.order[k];
                    const bool valid = vw.at(vb, HW, t);
                    const float v = col[(size_t)t * HW];
                    const unsigned int key = (valid && v >= wet_thr) ? day_key(v) : 0xFFFFFFFFu;
#pragma unroll
                    for (int s = 0; s < S; ++s) below[s] += key < cand[s];
                }
            } else
            for (int t0 = 0; t0 < N; t0 += 32) {
                const unsigned int bits = vb[(size_t)(t0 >> 5) * HW];
                const int tn = min(32, N - t0);
#pragma unroll 4
                for (int j = 0; j < tn; ++j) {
                    const float v = col[(size_t)(t0 + j) * HW];
                    const unsigned int key = (((bits >> j) & 1u) && v >= wet_thr) ? day_key(v) : 0xFFFFFFFFu;
#pragma unroll
                    for (int s = 0; s < S; ++s) below[s] += key < cand[s];
                }
            }
#pragma unroll
            for (int s = 0; s < S; ++s) prefix[s] = below[s] <= rank[s] ? cand[s] : prefix[s];
        }
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            const float a = key_float(prefix[2 * j]), b = key_float(prefix[2 * j + 1]);
            out[(size_t)j * HW + p] = (g[j] == 0.0 || a == b) ? a : (float)((double)a + g[j] * ((double)b - (double)a));
        }
    }
}

// blockIdx.y = side, with CAL blockIdx.z = slab; tau = the obs side's wet-day quantile maps [QW][HW] of the slab: wet_quant
// (slab 0) and cal_wet_quant (the groups) are the [2][QW][HW] maps K56 wrote
template <bool CAL>
__global__ __launch_bounds__(kThreads) void climate_heavy_kernel(const float* __restrict__ gen, const float* __restrict__ obs,
                                                                 const unsigned int* __restrict__ vbits,
                                                                 const float* __restrict__ wet_quant,
                                                                 const float* __restrict__ cal_wet_quant, float wet, int N, size_t HW,
                                                                 int QW, float* __restrict__ heavy, float* __restrict__ cal_heavy,
                                                                 Calendar cal) {
    const int side = blockIdx.y, slab = CAL ? blockIdx.z : 0;
    const int lo = CAL ? cal.start[slab] : 0, hi = CAL ? cal.start[slab + 1] : N;
    if (CAL && slab > 0) {
        wet_quant = cal_wet_quant + (size_t)(slab - 1) * 2 * QW * HW;
        heavy = cal_heavy + (size_t)(slab - 1) * 2 * QW * HW;
    }
    const float* tau = wet_quant + (size_t)QW * HW;
    const float* x = side ? obs : gen;
    float* out = heavy + (size_t)side * QW * HW;
    for (size_t p = (size_t)blockIdx.x * kThreads + threadIdx.x; p < HW; p += (size_t)gridDim.x * kThreads) {
        float th[kMaxQuant];
        double above[kMaxQuant], total = 0.0;
#pragma unroll
        for (int j = 0; j < kMaxQuant; ++j) {
            th[j] = j < QW ? tau[(size_t)j * HW + p] : nan_f();          // x > NaN is false: nothing is added
            above[j] = 0.0;
        }
        const float* col = x + p;
        const unsigned int* vb = vbits + p;
        if (CAL && slab > 0) {
            ValidWord vw;
#pragma unroll 4
            for (int k = lo; k < hi; ++k) {
                const int t = cal.order[k];
                const bool valid = vw.at(vb, HW, t);
                const float v = col[(size_t)t * HW];
                if (!valid) continue;
                const double d = (double)v;
                if (v >= wet) total += d;
#pragma unroll
                for (int j = 0; j < kMaxQuant; ++j)
                    if (v > th[j]) above[j] += d;
            }
        } else
        for (int t0 = 0; t0 < N; t0 += 32) {
            const unsigned int bits = vb[(size_t)(t0 >> 5) * HW];
            const int tn = min(32, N - t0);
#pragma unroll 4
            for (int j = 0; j < tn; ++j) {
                const float v = col[(size_t)(t0 + j) * HW];
                if (!((bits >> j) & 1u)) continue;
                const double d = (double)v;
                if (v >= wet) total += d;
#pragma unroll
                for (int k = 0; k < kMaxQuant; ++k)
                    if (v > th[k]) above[k] += d;
            }
        }
#pragma unroll
        for (int j = 0; j < kMaxQuant; ++j)
            if (j < QW) out[(size_t)j * HW + p] = ratio_f(above[j], total, !is_nan(th[j]) && total != 0.0);
    }
}

int check_levels(const char* what, const double* levels, int n, Levels& lv) {
    lv = Levels{};
    for (int j = 0; j < n; ++j) {
        SBGM_CHECK(levels[j] >= 0.0 && levels[j] <= 1.0, "climate_indices: %s level %d is outside [0, 1]", what, j);      // NaN fails
        lv.q[j] = levels[j];
    }
    return 0;
}

template <bool CAL>
int launch_select(int nq, const float* gen, const float* obs, const unsigned int* vbits, const int* days, const int* nwet,
                  float* cal_quant, int wet_only, float wet, int N, int64_t HW, const Levels& lv, float* quant, const Calendar& cal,
                  int slabs, int blocks, hipStream_t st) {
    switch (nq) {                                                             // one instance per count: no rank is carried in vain
#define SBGM_SELECT_CASE(NQ)                                                                                                    \
    case NQ:                                                                                                                   \
        hipLaunchKernelGGL((climate_select_kernel<NQ, CAL>), dim3(blocks, 2, slabs), dim3(kThreads), 0, st, gen, obs, vbits,    \
                           days, nwet, cal_quant, wet_only, wet, N, (size_t)HW, lv, quant, cal);                               \
        break;
        SBGM_SELECT_CASE(1) SBGM_SELECT_CASE(2) SBGM_SELECT_CASE(3) SBGM_SELECT_CASE(4)
        SBGM_SELECT_CASE(5) SBGM_SELECT_CASE(6) SBGM_SELECT_CASE(7) SBGM_SELECT_CASE(8)
#undef SBGM_SELECT_CASE
        default: SBGM_CHECK(false, "climate_indices: %d levels in one launch", nq);
    }
    SBGM_LAUNCH_CHECK();
    return 0;
}

bool sizes_ok(int N, int H, int W, int Q, int QW) {
    return N >= 2 && N <= kMaxDays && field_shape_ok(N, H, W) && Q >= 0 && Q <= kMaxQuant && QW >= 0 && QW <= kMaxQuant;
}

int64_t vbit_words(int N) { return (N + 31) / 32; }

// the words of K61's tables: order [2N], start [G + 2], link [N]
int64_t table_words(int N, int G) { return 3 * (int64_t)N + G + 2; }

struct GroupMaps { int* days; float* stats; int* spells; int* transitions; float* quant; float* wet_quant; float* heavy; };

// K55 - K57 on checked arguments; with CAL, K61 first and the slabs in the grid
template <bool CAL>
int run_indices(const float* gen, const float* obs, const void* mask, int mask_is_u8, int N, int Nm, int64_t HW, float wet,
                const Levels& lq, int Q, const Levels& lw, int QW, const int* day_numbers, const int* groups, int G, int* days,
                float* stats, int* spells, int* transitions, float* quant, float* wet_quant, float* heavy, const GroupMaps& gm,
                void* workspace, hipStream_t st) {
    const int slabs = CAL ? 1 + G : 1;
    unsigned int* vbits = static_cast<unsigned int*>(workspace);
    int* nwet = reinterpret_cast<int*>(vbits + vbit_words(N) * HW);               // [slabs][2][HW]
    Calendar cal{};
    if (CAL) {
        int* order = nwet + (size_t)slabs * 2 * HW;
        int* start = order + 2 * (size_t)N;
        int* link = start + G + 2;
        hipLaunchKernelGGL(climate_prepare_kernel, dim3(1), dim3(kThreads), 0, st, day_numbers, groups, N, G, order, start, link);
        SBGM_LAUNCH_CHECK();
        cal = Calendar{order, start, link, gm.days, gm.stats, gm.spells, gm.transitions};
    }
    const int blocks = (int)std::min<int64_t>((HW + kThreads - 1) / kThreads, kMaxBlocks);
    hipLaunchKernelGGL(climate_moments_kernel<CAL>, dim3(blocks, slabs), dim3(kThreads), 0, st, gen, obs, mask, mask_is_u8,
                       (int)(mask && Nm == N && N > 1), N, (size_t)HW, wet, days, stats, spells, transitions, vbits, nwet, cal);
    SBGM_LAUNCH_CHECK();
    if (Q > 0)
        if (int rc = launch_select<CAL>(Q, gen, obs, vbits, days, nwet, gm.quant, 0, wet, N, HW, lq, quant, cal, slabs, blocks, st))
            return rc;
    if (QW > 0) {
        if (int rc = launch_select<CAL>(QW, gen, obs, vbits, days, nwet, gm.wet_quant, 1, wet, N, HW, lw, wet_quant, cal, slabs,
                                        blocks, st))
            return rc;
        hipLaunchKernelGGL(climate_heavy_kernel<CAL>, dim3(blocks, 2, slabs), dim3(kThreads), 0, st, gen, obs, vbits, wet_quant,
                           gm.wet_quant, wet, N, (size_t)HW, QW, heavy, gm.heavy, cal);
        SBGM_LAUNCH_CHECK();
    }
    return 0;
}

}  // namespace

extern "C" {

int64_t sbgm_climate_indices_workspace_bytes(int N, int H, int W, int Q, int QW) {
    if (!sizes_ok(N, H, W, Q, QW)) return 0;
    return (vbit_words(N) + 2) * (int64_t)H * W * (int64_t)sizeof(unsigned int);      // validity bits, then n_wet of both sides
}

int64_t sbgm_climate_calendar_workspace_bytes(int N, int H, int W, int Q, int QW, int G) {
    if (!sizes_ok(N, H, W, Q, QW) || G < 0 || G > kMaxGroups) return 0;
    // validity bits, n_wet of both sides of every slab, K61's tables
    return ((vbit_words(N) + 2 * (1 + G)) * (int64_t)H * W + table_words(N, G)) * (int64_t)sizeof(unsigned int);
}

int sbgm_climate_indices_calendar(const float* gen, const float* obs, const void* mask, int mask_is_u8, int N, int Nm, int H, int W,
                                  float wet, const double* quantiles, int Q, const double* wet_quantiles, int QW,
                                  const int* day_numbers, const int* groups, int G, int* days, float* stats, int* spells,
                                  int* transitions, float* quant, float* wet_quant, float* heavy, int* group_days,
                                  float* group_stats, int* group_spells, int* group_transitions, float* group_quant,
                                  float* group_wet_quant, float* group_heavy, void* workspace, int64_t workspace_bytes,
                                  void* stream) {
    SBGM_CHECK(gen && obs && days && stats && spells && transitions && workspace, "climate_indices: null argument");
    SBGM_CHECK(N >= 2 && N <= kMaxDays, "climate_indices: N=%d days (2..%d)", N, kMaxDays);
    SBGM_CHECK(field_shape_ok(N, H, W), "climate_indices: field size %dx%d (sides 2..%d, H*W <= 2^20)", H, W, kMaxSide);
    SBGM_CHECK(!mask || Nm == 1 || Nm == N, "climate_indices: mask of %d fields (1 or %d)", Nm, N);
    SBGM_CHECK(std::isfinite(wet), "climate_indices: the wet-day threshold is not finite");
    SBGM_CHECK(Q >= 0 && Q <= kMaxQuant && (Q == 0 || (quantiles && quant)), "climate_indices: %d quantiles (0..%d, with their "
               "levels and maps)", Q, kMaxQuant);
    SBGM_CHECK(QW >= 0 && QW <= kMaxQuant && (QW == 0 || (wet_quantiles && wet_quant && heavy)), "climate_indices: %d wet-day "
               "quantiles (0..%d, with their levels and maps)", QW, kMaxQuant);
    SBGM_CHECK(G >= 0 && G <= kMaxGroups && (G > 0) == (groups != nullptr), "climate_indices: G=%d groups (0 without ids, else "
               "1..%d)", G, kMaxGroups);
    SBGM_CHECK(G == 0 || (group_days && group_stats && group_spells && group_transitions && (Q == 0 || group_quant) &&
                          (QW == 0 || (group_wet_quant && group_heavy))), "climate_indices: null group output");
    const bool cal = day_numbers || G > 0;
    // without a calendar and groups this is sbgm_climate_indices, its workspace included
    const int64_t need = cal ? sbgm_climate_calendar_workspace_bytes(N, H, W, Q, QW, G)
                             : sbgm_climate_indices_workspace_bytes(N, H, W, Q, QW);
    SBGM_CHECK(workspace_bytes >= need, "climate_indices: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
               (long long)need);
    Levels lq, lw;
    if (int rc = check_levels("quantile", quantiles, Q, lq)) return rc;
    if (int rc = check_levels("wet-day quantile", wet_quantiles, QW, lw)) return rc;
    const GroupMaps gm{group_days, group_stats, group_spells, group_transitions, group_quant, group_wet_quant, group_heavy};
    const int64_t HW = (int64_t)H * W;
    return cal ? run_indices<true>(gen, obs, mask, mask_is_u8, N, Nm, HW, wet, lq, Q, lw, QW, day_numbers, groups, G, days, stats,
                                   spells, transitions, quant, wet_quant, heavy, gm, workspace, ST)
               : run_indices<false>(gen, obs, mask, mask_is_u8, N, Nm, HW, wet, lq, Q, lw, QW, nullptr, nullptr, 0, days, stats,
                                    spells, transitions, quant, wet_quant, heavy, gm, workspace, ST);
}

int sbgm_climate_indices(const float* gen, const float* obs, const void* mask, int mask_is_u8, int N, int Nm, int H, int W,
                         float wet, const double* quantiles, int Q, const double* wet_quantiles, int QW, int* days, float* stats,
                         int* spells, int* transitions, float* quant, float* wet_quant, float* heavy, void* workspace,
                         int64_t workspace_bytes, void* stream) {
    return sbgm_climate_indices_calendar(gen, obs, mask, mask_is_u8, N, Nm, H, W, wet, quantiles, Q, wet_quantiles, QW, nullptr,
                                         nullptr, 0, days, stats, spells, transitions, quant, wet_quant, heavy, nullptr, nullptr,
                                         nullptr, nullptr, nullptr, nullptr, nullptr, workspace, workspace_bytes, stream);
}

}  // extern "C"
