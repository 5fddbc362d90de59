// Object-based verification on the device: connected objects of thresholded fields and the ingredients of the
// SAL score (structure, amplitude, location; Wernli et al. 2008).
//   K51 object_labels — connected-component labelling by union-find, 4- or 8-connected.  Canonical label = 1 + the smallest
//                       linear index row * W + col of the object; background 0.
//   K52 object_scores — per (side, field, threshold): object count, area, mass, V and r; per (side, field): domain mean and
//                       weighted centre; per field the scores S, A, L1, L2, L; the area histogram.
// A pixel is valid when gen and obs are not NaN and the mask (uint8 != 0, or fp32 > 0.5) admits it; an object pixel of a
// side is a valid pixel with `v >= thr` in fp32.
//
// Labelling, in launches (no workgroup ever waits for another; there is no spin-wait anywhere in this file):
//   runs     one workgroup per row: lab[p] = 1 + index of the first pixel of p's horizontal run (a max-scan, not a
//            propagation), 0 for background.  From here on lab[p] - 1 <= p always: lab is a forest whose edges point to
//            smaller indices, and a root x has lab[x] == x + 1.
//   merge    one thread per pixel unites its run with the runs it touches in the row above.  `unite` finds both roots and
//            links the larger to the smaller with atomicMin; when the atomic reports that the larger was no longer a root it
//            goes on with the parent it displaced, so no link is ever lost.
//   flatten  every run start is pointed at its root (only the run starts: the other pixels still point at their run start,
//            so the depth of the tree is paid once per run, not once per pixel); for object_labels a last launch copies the
//            root to the rest of each run.
// Termination: `find` only follows lab[x] - 1 < x and `unite` replaces the larger of its two indices by a smaller one in
// every round, so both end after at most 2 H W steps in total whatever any other thread does.  Each `unite` and each `find`
// also carries that number as an explicit budget; on reaching it the thread sets *status and gives up, so a bug shows as a
// non-zero status (and a failing test), never as a hung queue.
// Coherence: in the merge and flatten kernels other workgroups change lab while it is read.  Every read of lab there is an
// agent-scope relaxed atomic load and every link an agent-scope atomicMin.  The loads are NOT to be taken as fresh: they
// bypass the CU's L1 but are served by the reading XCD's L2, which does not see the other XCDs' atomics, so a load can
// return an old value.  Correctness rests on this argument alone: the algorithm needs each load to be only a value lab[x]
// held at some time.  Every value ever stored in lab[x] names a pixel that is, by the end of the launch, in x's set (the
// thread that displaces a parent goes on to unite the displaced parent with the new one), so a `find` over old values ends at
// an element of the right set, and whether that element is a root is decided by the atomicMin alone, which is performed at
// the memory side for all XCDs and whose return value is the truth at the moment of the link.  (In flatten the forest no
// longer changes except that run starts are re-pointed at their roots: an old value there is the former parent, also above.)
// Accumulation: a pixel contributes round(v * 2^(30 - e)) with 2^(e-1) <= max |v| < 2^e over the valid pixels of its field,
// a 31-bit signed integer; areas, masses and coordinate-weighted masses are 64-bit integer sums (exact whenever the values
// are multiples of 2^(e-30), e.g. multiples of 2^-8 below 256; within (vmax / thr) 2^-30 relative otherwise), added with
// 64-bit integer atomics after a wave has summed the pixels it holds of one object.  No floating-point atomics.  The fp64
// sums over objects are made per segment of 4096 slots by one workgroup: thread t adds the segment's slots t, t + 256, ...
// in ascending order, then a fixed tree over the 256 threads; one thread per problem then adds the segments in ascending
// order.  The scores are computed by single threads.  FP contraction is off in this file.  The helpers shared with the other
// verify files (validity, the key, ThrList, limits, block reductions, the chunk planner) are in verify_common.h; kMaxThr
// there bounds the fixed thresholds, the relative one is an extra index.
#include "verify_common.h"

#pragma clang fp contract(off)

#define ST ((hipStream_t)stream)

namespace {

constexpr int kRowThreads = 256;                          // runs: one workgroup per row,
constexpr int kRowPer = kMaxSide / kRowThreads;           // each thread owns 8 consecutive columns
constexpr int kPix = 256;                                 // merge / flatten: one pixel per thread
constexpr int kAccPer = 8;                                // accumulate: a wave owns 8 x 64 consecutive pixels
constexpr int kAccBlock = 256 * kAccPer;
constexpr int kPrepThreads = 512;
constexpr int kFinThreads = 256;
constexpr int kSegSlots = 4096;                           // sums: slots per workgroup
constexpr int kPartSums = 3;                              // its fp64 partial: sum R, sum R |x - x_n|, sum R (R / Rmax)
constexpr int kPartCounts = 2;                            // its int64 partial: objects, area
constexpr int kHistBins = SBGM_OBJECTS_AREA_BINS;
constexpr int64_t kMaxChunkProblems = 65534;              // gridDim.y
constexpr int64_t kProblemBytes = 36;                     // per pixel of one problem: 3 x int64, area, peak key, lab
constexpr int64_t kSegmentBytes = (kPartSums + kPartCounts) * 8;      // per segment of one problem: the two partials

// where the problems of a launch come from.  labels_mode: problem q is field q of `gen` at thr_host.  Otherwise problem q is
// side q & 1 of pair q >> 1, pair = (field f0 + pair / nt, threshold t0 + pair % nt), at threshold[side][f][t] on the device.
struct Src {
    const float* gen; const float* obs; const void* mask;
    int mask_u8, obs_step, mask_step, N, H, W, T, f0, t0, nt, labels_mode;
    const float* thr_dev; float thr_host;
};
struct Prob { int side, f, t; const float* v; float thr; };

__device__ __forceinline__ Prob problem(const Src& s, int q) {
    Prob p;
    const size_t HW = (size_t)s.H * s.W;
    if (s.labels_mode) {
        p.side = 0; p.f = q; p.t = 0; p.thr = s.thr_host;
    } else {
        const int pair = q >> 1;
        p.side = q & 1; p.f = s.f0 + pair / s.nt; p.t = s.t0 + pair % s.nt;
        p.thr = s.thr_dev[((size_t)p.side * s.N + p.f) * s.T + p.t];
    }
    p.v = p.side ? s.obs + (size_t)p.f * s.obs_step * HW : s.gen + (size_t)p.f * HW;
    return p;
}
__device__ __forceinline__ bool valid_at(const Src& s, int f, size_t i) {
    const size_t HW = (size_t)s.H * s.W;
    return !is_nan(s.gen[(size_t)f * HW + i]) && !is_nan(s.obs[(size_t)f * s.obs_step * HW + i]) &&
           mask_at(s.mask, s.mask_u8, (size_t)f * s.mask_step * HW + i);
}
__device__ __forceinline__ unsigned int lab_load(const unsigned int* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void lab_store(unsigned int* p, unsigned int v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// the root above object pixel x: follows lab[x] - 1 while it is smaller than x, at most `budget` steps
__device__ __forceinline__ unsigned int find_root(const unsigned int* lab, unsigned int x, int& budget) {
    while (budget > 0) {
        const unsigned int up = lab_load(lab + x) - 1u;
        if (up >= x) break;                                   // a root (up == x); up > x cannot be and would end the walk too
        x = up;
        --budget;
    }
    return x;
}
__device__ __forceinline__ void unite(unsigned int* lab, unsigned int a, unsigned int b, int budget, int* status) {
    for (;;) {
        a = find_root(lab, a, budget);
        b = find_root(lab, b, budget);
        if (budget <= 0) { atomicOr(status, SBGM_OBJECTS_STATUS_MERGE_CAP); return; }
        if (a == b) return;
        if (a < b) { const unsigned int s = a; a = b; b = s; }
        const unsigned int old = atomicMin(lab + a, b + 1u) - 1u;      // agent scope
        if (old == a) return;                                 // a was a root and now points at b
        a = old;                                              // a pointed at old < a: old and b remain to be united
        --budget;
    }
}

// ---- K51 runs: grid (H, problems) ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kRowThreads) void object_runs_kernel(Src s, unsigned int* __restrict__ lab) {
    __shared__ int wave_last[kRowThreads / SBGM_WAVE];
    const int row = blockIdx.x, q = blockIdx.y, W = s.W;
    const Prob pr = problem(s, q);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t r0 = (size_t)row * W;
    const int c0 = threadIdx.x * kRowPer;
    auto object_at = [&](int c) -> bool {
        if (c < 0 || c >= W) return false;
        return valid_at(s, pr.f, r0 + c) && pr.v[r0 + c] >= pr.thr;
    };
    bool prev = object_at(c0 - 1), obj[kRowPer];
    int start[kRowPer], last = -1;                            // the latest run start at or before each column
#pragma unroll
    for (int e = 0; e < kRowPer; ++e) {
        obj[e] = object_at(c0 + e);
        if (obj[e] && !prev) last = c0 + e;
        start[e] = last;
        prev = obj[e];
    }
    int inc = last;                                           // inclusive max-scan of the threads' last starts
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(inc, d, 64);
        if (lane >= d) inc = max(inc, up);
    }
    if (lane == 63) wave_last[wave] = inc;
    __syncthreads();
    int before = __shfl_up(inc, 1, 64);
    if (lane == 0) before = -1;
    for (int w = 0; w < wave; ++w) before = max(before, wave_last[w]);
    unsigned int* out = lab + (size_t)q * s.H * W + r0;
#pragma unroll
    for (int e = 0; e < kRowPer; ++e)
        if (c0 + e < W) out[c0 + e] = obj[e] ? (unsigned int)(r0 + max(start[e], before)) + 1u : 0u;
}

// ---- K51 merge: grid (ceil(HW / 256), problems) -------------------------------------------------------------------------------
// With U, UL, UR the pixels above and L the one to the left: a pixel unites with U unless L and UL are objects too (then
// the pixel to the left joins the same two runs); 8-connected and U background, it unites with UL unless L is an object (L
// has UL above it) and with UR.
__global__ __launch_bounds__(kPix) void object_merge_kernel(unsigned int* __restrict__ lab_all, int H, int W, int conn8,
                                                            int* __restrict__ status) {
    const int HW = H * W;
    const int p = blockIdx.x * kPix + threadIdx.x;
    if (p < W || p >= HW) return;
    unsigned int* lab = lab_all + (size_t)blockIdx.y * HW;
    if (!lab_load(lab + p)) return;
    const int c = p % W;
    const bool U = lab_load(lab + p - W) != 0;
    const bool L = c > 0 && lab_load(lab + p - 1) != 0;
    const bool UL = c > 0 && lab_load(lab + p - W - 1) != 0;
    const int budget = 2 * HW + 4;
    if (U) {
        if (!(L && UL)) unite(lab, p, p - W, budget, status);
    } else if (conn8) {
        if (UL && !L) unite(lab, p, p - W - 1, budget, status);
        if (c + 1 < W && lab_load(lab + p - W + 1) != 0) unite(lab, p, p - W + 1, budget, status);
    }
}

// ---- K51 flatten: run starts -> their root -------------------------------------------------------------------------------------
// Writers store roots over parents while others walk: a walker meets the old parent or the root, both above it in the (now
// fixed) forest.  The pixels that are not run starts are neither read nor written here.
__global__ __launch_bounds__(kPix) void object_flatten_kernel(unsigned int* __restrict__ lab_all, int H, int W, int* __restrict__ status) {
    const int HW = H * W;
    const int p = blockIdx.x * kPix + threadIdx.x;
    if (p >= HW) return;
    unsigned int* lab = lab_all + (size_t)blockIdx.y * HW;
    if (!lab_load(lab + p)) return;
    if (p % W > 0 && lab_load(lab + p - 1) != 0) return;     // not a run start
    int budget = HW + 1;
    const unsigned int root = find_root(lab, p, budget);
    if (budget <= 0) { atomicOr(status, SBGM_OBJECTS_STATUS_FIND_CAP); return; }
    if (root != (unsigned int)p) lab_store(lab + p, root + 1u);
}

// ---- K51 spread: the rest of each run takes the label of its run start (reads run starts only, writes the others only) ---
__global__ __launch_bounds__(kPix) void object_spread_kernel(unsigned int* __restrict__ lab_all, int H, int W) {
    const int HW = H * W;
    const int p = blockIdx.x * kPix + threadIdx.x;
    if (p >= HW) return;
    unsigned int* lab = lab_all + (size_t)blockIdx.y * HW;
    const unsigned int mine = lab[p];
    if (!mine || p % W == 0 || !lab[p - 1]) return;
    lab[p] = lab[mine - 1u];
}

// ---- K52 prepare: grid (N, 2), one workgroup per (field, side) ---------------------------------------------------------------
// Sweeps its field a few times: (1) valid count, max |v| and the count of values >= wet; (2) the fixed-point sums of v,
// v * row and v * col -> domain_mean, com; then, for the relative threshold, (3..6) a radix select of the order statistic
// x_(lo) among the valid values >= wet, 8 bits a sweep, and (7) x_(lo+1) as the smallest value above x_(lo) where x_(lo)
// is not repeated.  thr = (float)(factor * q), q the type-7 quantile: h = quantile (n - 1), lo = floor(h), g = h - lo,
// q = x_(lo) when g == 0 or x_(lo) == x_(lo+1), else (float)(x_(lo) + g (x_(lo+1) - x_(lo))) in fp64.
__global__ __launch_bounds__(kPrepThreads) void object_prepare_kernel(Src s, int Tfixed, ThrList thr, int has_rel, double factor,
                                                                      double quantile, float wet, float* __restrict__ threshold,
                                                                      long long* __restrict__ valid, double* __restrict__ domain_mean,
                                                                      double* __restrict__ com, int* __restrict__ fexp) {
    __shared__ unsigned long long slot[kPrepThreads / SBGM_WAVE];
    __shared__ unsigned int wmax[kPrepThreads / SBGM_WAVE];
    __shared__ unsigned int hist[256];
    __shared__ unsigned int sel_prefix, sel_rank, sel_eq, sel_less, sel_min;
    const int f = blockIdx.x, side = blockIdx.y, W = s.W;
    const int HW = s.H * W;
    const float* v = side ? s.obs + (size_t)f * s.obs_step * HW : s.gen + (size_t)f * HW;
    const int tid = threadIdx.x;
    const size_t sf = (size_t)side * s.N + f;

    unsigned long long cnt = 0, cntw = 0;
    unsigned int mx = 0;
    for (int p = tid; p < HW; p += kPrepThreads) {
        if (!valid_at(s, f, p)) continue;
        const float x = v[p];
        ++cnt;
        cntw += x >= wet;
        mx = max(mx, __float_as_uint(x) & 0x7FFFFFFFu);       // |x| as bits: integer order is magnitude order
    }
    const unsigned long long nvalid = block_sum_u64<kPrepThreads>(cnt, slot);
    const unsigned long long nwet = block_sum_u64<kPrepThreads>(cntw, slot);
    mx = wave_max_u32(mx);
    if ((tid & 63) == 0) wmax[tid >> 6] = mx;
    __syncthreads();
    mx = 0;
    for (int w = 0; w < kPrepThreads / SBGM_WAVE; ++w) mx = max(mx, wmax[w]);
    int e = 0;                                                // max |v| < 2^e (and >= 2^(e-1)); infinities count as 2^128
    if (mx) {
        const int be = (int)(mx >> 23);
        e = be ? be - 126 : -126 - __clz(mx << 9);            // normal : subnormal
    }
    const double up = ldexp(1.0, 30 - e);
    long long s0 = 0, s1 = 0, s2 = 0;
    for (int p = tid; p < HW; p += kPrepThreads) {
        if (!valid_at(s, f, p)) continue;
        const float x = v[p];
        const long long fx = fabsf(x) < __builtin_inff() ? __double2ll_rn((double)x * up) : 0;
        s0 += fx; s1 += fx * (p / W); s2 += fx * (p % W);
    }
    const long long t0 = (long long)block_sum_u64<kPrepThreads>((unsigned long long)s0, slot);
    const long long t1 = (long long)block_sum_u64<kPrepThreads>((unsigned long long)s1, slot);
    const long long t2 = (long long)block_sum_u64<kPrepThreads>((unsigned long long)s2, slot);
    if (tid == 0) {
        fexp[sf] = e;
        if (side == 0) valid[f] = (long long)nvalid;
        domain_mean[sf] = nvalid ? (double)t0 * ldexp(1.0, e - 30) / (double)nvalid : nan_d();
        com[sf * 2] = (nvalid && t0) ? (double)t1 / (double)t0 : nan_d();
        com[sf * 2 + 1] = (nvalid && t0) ? (double)t2 / (double)t0 : nan_d();
    }
    for (int t = tid; t < Tfixed; t += kPrepThreads) threshold[sf * s.T + t] = thr.v[t];
    if (!has_rel) return;
    float* out = threshold + sf * s.T + Tfixed;
    if (nwet == 0) {                                          // uniform over the workgroup
        if (tid == 0) *out = nan_f();
        return;
    }
    const double h = quantile * (double)(nwet - 1);
    const unsigned int lo = (unsigned int)floor(h);
    const double g = h - floor(h);
    if (tid == 0) { sel_prefix = 0; sel_rank = lo; sel_less = 0; sel_min = 0xFFFFFFFFu; }
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int b = tid; b < 256; b += kPrepThreads) hist[b] = 0;
        __syncthreads();
        const unsigned int prefix = sel_prefix, himask = shift == 24 ? 0u : 0xFFFFFFFFu << (shift + 8);
        for (int p = tid; p < HW; p += kPrepThreads) {
            if (!valid_at(s, f, p)) continue;
            const float x = v[p];
            if (!(x >= wet)) continue;
            const unsigned int k = float_key(x);
            if ((k & himask) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            unsigned int cum = 0, rank = sel_rank;
            int b = 0;
            for (; b < 255; ++b) {
                if (rank < cum + hist[b]) break;
                cum += hist[b];
            }
            sel_rank = rank - cum;
            sel_less += cum;
            sel_prefix = prefix | ((unsigned int)b << shift);
            sel_eq = hist[b];
        }
        __syncthreads();
    }
    const unsigned int klo = sel_prefix;
    const bool need_hi = g != 0.0 && sel_less + sel_eq < lo + 2u;        // x_(lo+1) is a larger value
    if (need_hi) {
        unsigned int mn = 0xFFFFFFFFu;
        for (int p = tid; p < HW; p += kPrepThreads) {
            if (!valid_at(s, f, p)) continue;
            const float x = v[p];
            if (!(x >= wet)) continue;
            const unsigned int k = float_key(x);
            if (k > klo) mn = min(mn, k);
        }
        mn = wave_min_u32(mn);
        if ((tid & 63) == 0) atomicMin(&sel_min, mn);
        __syncthreads();
    }
    if (tid == 0) {
        const float xlo = key_float(klo), xhi = need_hi ? key_float(sel_min) : xlo;
        const float qv = (g == 0.0 || xlo == xhi) ? xlo : (float)((double)xlo + g * ((double)xhi - (double)xlo));
        *out = (float)(factor * (double)qv);
    }
}

// ---- K52 accumulate: grid (ceil(HW / 2048), problems) ------------------------------------------------------------------------
// A wave walks 8 x 64 consecutive pixels.  While the object pixels it meets belong to one root the lanes add privately; when
// the root changes, the wave sums its lanes and lane 0 adds the totals to the root's slots with integer atomics.  A step
// whose lanes hold several roots is added lane by lane.
struct Slots { long long* acc; unsigned int* area; unsigned int* peak; };     // acc [3][HW]: mass, mass * row, mass * col
__device__ __forceinline__ void slot_add(const Slots& sl, int HW, unsigned int root, unsigned int n, long long m, long long mr,
                                         long long mc, unsigned int pk) {
    atomicAdd(sl.area + root, n);
    atomicAdd(reinterpret_cast<unsigned long long*>(sl.acc) + root, (unsigned long long)m);
    atomicAdd(reinterpret_cast<unsigned long long*>(sl.acc) + HW + root, (unsigned long long)mr);
    atomicAdd(reinterpret_cast<unsigned long long*>(sl.acc) + 2 * (size_t)HW + root, (unsigned long long)mc);
    atomicMax(sl.peak + root, pk);
}
__global__ __launch_bounds__(256) void object_accumulate_kernel(Src s, const unsigned int* __restrict__ lab_all, const int* __restrict__ fexp,
                                                                long long* __restrict__ acc_all, unsigned int* __restrict__ area_all,
                                                                unsigned int* __restrict__ peak_all) {
    const int q = blockIdx.y, W = s.W, HW = s.H * W;
    const Prob pr = problem(s, q);
    const unsigned int* lab = lab_all + (size_t)q * HW;
    const Slots sl{acc_all + (size_t)q * 3 * HW, area_all + (size_t)q * HW, peak_all + (size_t)q * HW};
    const double up = ldexp(1.0, 30 - fexp[(size_t)pr.side * s.N + pr.f]);
    const int lane = threadIdx.x & 63;
    const int base = blockIdx.x * kAccBlock + (threadIdx.x >> 6) * (64 * kAccPer);
    constexpr unsigned int kNone = 0xFFFFFFFFu;
    unsigned int cur = kNone, n = 0, pk = 0;                  // cur is uniform over the wave
    long long m = 0, mr = 0, mc = 0;
    auto flush = [&]() {
        if (cur != kNone) {
            const unsigned long long tn = wave_sum_u64(n), tm = wave_sum_u64((unsigned long long)m),
                                     tr = wave_sum_u64((unsigned long long)mr), tc = wave_sum_u64((unsigned long long)mc);
            const unsigned int tp = wave_max_u32(pk);
            if (lane == 0 && tn) slot_add(sl, HW, cur, (unsigned int)tn, (long long)tm, (long long)tr, (long long)tc, tp);
        }
        cur = kNone; n = 0; pk = 0; m = 0; mr = 0; mc = 0;
    };
    for (int it = 0; it < kAccPer; ++it) {
        const int p = base + it * 64 + lane;
        unsigned int root = kNone;
        long long fx = 0;
        unsigned int k = 0;
        if (p < HW) {
            const unsigned int l1 = lab[p];
            if (l1) {
                root = lab[l1 - 1u] - 1u;                     // run start -> root (a root points at itself)
                const float x = pr.v[p];
                fx = fabsf(x) < __builtin_inff() ? __double2ll_rn((double)x * up) : 0;
                k = float_key(x);
            }
        }
        const bool has = root != kNone;
        const unsigned long long who = __ballot(has);
        if (!who) continue;
        const unsigned int first = __shfl(root, __ffsll((long long)who) - 1, 64);
        if (__all(!has || root == first)) {
            if (first != cur) { flush(); cur = first; }
            if (has) { ++n; m += fx; mr += fx * (p / W); mc += fx * (p % W); pk = max(pk, k); }
        } else {
            flush();
            if (has) slot_add(sl, HW, root, 1u, fx, fx * (p / W), fx * (p % W), k);
        }
    }
    flush();
}

// ---- K52 sums: grid (segments of 4096 slots, problems) -----------------------------------------------------------------------
// Slot i with area > 0 is the object with label i + 1: R = mass, x_n = (mass * row, mass * col) / mass, Rmax from the peak key.
// Thread t adds the segment's slots t, t + 256, ... in ascending order; block_sum_tree then adds the 256 partial sums in a
// fixed order.  part_sums fp64 [problems][segments][3]; part_counts int64 [problems][segments][2] = (objects, area).
__global__ __launch_bounds__(kFinThreads) void object_sums_kernel(Src s, const int* __restrict__ fexp, const long long* __restrict__ acc_all,
                                                                  const unsigned int* __restrict__ area_all,
                                                                  const unsigned int* __restrict__ peak_all, const double* __restrict__ com,
                                                                  double* __restrict__ part_sums, long long* __restrict__ part_counts,
                                                                  unsigned long long* __restrict__ area_hist) {
    __shared__ double buf[kFinThreads];
    __shared__ unsigned int bins[kHistBins];
    __shared__ unsigned long long cnt[2];
    const int seg = blockIdx.x, q = blockIdx.y, HW = s.H * s.W;
    const Prob pr = problem(s, q);
    const size_t sf = (size_t)pr.side * s.N + pr.f;
    const long long* acc = acc_all + (size_t)q * 3 * HW;
    const unsigned int* ar = area_all + (size_t)q * HW;
    const unsigned int* pk = peak_all + (size_t)q * HW;
    const double down = ldexp(1.0, fexp[sf] - 30), cr = com[sf * 2], cc = com[sf * 2 + 1];
    if (threadIdx.x < kHistBins) bins[threadIdx.x] = 0;
    if (threadIdx.x < 2) cnt[threadIdx.x] = 0;
    __syncthreads();
    double sR = 0.0, sRd = 0.0, sRV = 0.0;
    unsigned long long nobj = 0, atot = 0;
    const int end = min(HW, (seg + 1) * kSegSlots);
    for (int i = seg * kSegSlots + threadIdx.x; i < end; i += kFinThreads) {
        const unsigned int a = ar[i];
        if (!a) continue;
        const double mi = (double)acc[i], R = mi * down;
        const double dr = cr - (double)acc[(size_t)HW + i] / mi, dc = cc - (double)acc[2 * (size_t)HW + i] / mi;
        sR += R;
        sRd += R * sqrt(dr * dr + dc * dc);
        sRV += R * (R / (double)key_float(pk[i]));
        ++nobj; atot += a;
        atomicAdd(&bins[31 - __clz(a)], 1u);
    }
    const double tR = block_sum_tree<kFinThreads>(sR, buf), tRd = block_sum_tree<kFinThreads>(sRd, buf),
                 tRV = block_sum_tree<kFinThreads>(sRV, buf);
    nobj = wave_sum_u64(nobj); atot = wave_sum_u64(atot);
    if ((threadIdx.x & 63) == 0) { atomicAdd(&cnt[0], nobj); atomicAdd(&cnt[1], atot); }
    __syncthreads();
    if (threadIdx.x < kHistBins && bins[threadIdx.x])
        atomicAdd(&area_hist[((size_t)pr.side * s.T + pr.t) * kHistBins + threadIdx.x], (unsigned long long)bins[threadIdx.x]);
    if (threadIdx.x == 0) {
        const size_t slot = (size_t)q * gridDim.x + seg;
        double* o = part_sums + slot * kPartSums;
        o[0] = tR; o[1] = tRd; o[2] = tRV;
        part_counts[slot * kPartCounts] = (long long)cnt[0];
        part_counts[slot * kPartCounts + 1] = (long long)cnt[1];
    }
}

// ---- K52 collect: one thread per problem adds its segments in ascending order -------------------------------------------------
__global__ __launch_bounds__(64) void object_collect_kernel(Src s, const double* __restrict__ part_sums,
                                                            const long long* __restrict__ part_counts, int nseg, int np,
                                                            long long* __restrict__ n_objects, long long* __restrict__ area,
                                                            double* __restrict__ mass, double* __restrict__ Vout, double* __restrict__ rout) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= np) return;
    const Prob pr = problem(s, q);
    const double* in = part_sums + (size_t)q * nseg * kPartSums;
    const long long* ic = part_counts + (size_t)q * nseg * kPartCounts;
    double tR = 0.0, tRd = 0.0, tRV = 0.0;
    long long n = 0, a = 0;
    for (int g = 0; g < nseg; ++g) {
        tR += in[g * kPartSums]; tRd += in[g * kPartSums + 1]; tRV += in[g * kPartSums + 2];
        n += ic[g * kPartCounts];
        a += ic[g * kPartCounts + 1];
    }
    const size_t o = ((size_t)pr.side * s.N + pr.f) * s.T + pr.t;
    n_objects[o] = n;
    area[o] = a;
    mass[o] = tR;
    Vout[o] = n ? tRV / tR : nan_d();
    rout[o] = n ? tRd / tR : nan_d();
}

// ---- K52 scores: one thread per (field, threshold) ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void object_scores_kernel(int N, int T, int H, int W, const long long* __restrict__ valid,
                                                            const double* __restrict__ domain_mean, const double* __restrict__ com,
                                                            const long long* __restrict__ n_objects, const double* __restrict__ V,
                                                            const double* __restrict__ r, double* __restrict__ S, double* __restrict__ L2,
                                                            double* __restrict__ A, double* __restrict__ L1, double* __restrict__ L) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * T) return;
    const int f = i / T, t = i % T;
    const double d = sqrt((double)(H - 1) * (double)(H - 1) + (double)(W - 1) * (double)(W - 1));
    const double Dg = domain_mean[f], Do = domain_mean[N + f];
    const double dr = com[(size_t)f * 2] - com[((size_t)N + f) * 2], dc = com[(size_t)f * 2 + 1] - com[((size_t)N + f) * 2 + 1];
    // a zero sum leaves com NaN and domain_mean 0; no valid pixel leaves both NaN
    const bool field_ok = valid[f] > 0 && Dg != 0.0 && Do != 0.0 && Dg + Do != 0.0;
    const double a = field_ok ? (Dg - Do) / (0.5 * (Dg + Do)) : nan_d();
    const double l1 = field_ok ? sqrt(dr * dr + dc * dc) / d : nan_d();
    const size_t g = (size_t)f * T + t, o = ((size_t)N + f) * T + t;
    const bool both = n_objects[g] > 0 && n_objects[o] > 0;
    const double Vg = V[g], Vo = V[o];
    const double sv = (both && Vg + Vo != 0.0) ? (Vg - Vo) / (0.5 * (Vg + Vo)) : nan_d();
    const double l2 = both ? 2.0 * fabs(r[g] - r[o]) / d : nan_d();
    S[i] = sv;
    L2[i] = l2;
    L[i] = l1 + l2;
    if (t == 0) { A[f] = a; L1[f] = l1; }
}

inline int64_t head_bytes(int N) { return ((int64_t)2 * N * (int64_t)sizeof(int) + 255) / 256 * 256; }
inline int segments(int HW) { return (HW + kSegSlots - 1) / kSegSlots; }
inline int64_t pair_bytes(int H, int W) {
    return 2 * (kProblemBytes * (int64_t)H * W + (int64_t)segments(H * W) * kSegmentBytes);
}
// a pair is two problems (gen and obs); the head (fexp) comes off the room first
inline ChunkPlan chunk_plan(int N, int H, int W, int T, int64_t max_bytes) {
    return plan_chunks(N, T, std::max<int64_t>(0, max_bytes - head_bytes(N)), pair_bytes(H, W), kMaxChunkProblems / 2);
}
inline int pix_blocks(int HW) { return (HW + kPix - 1) / kPix; }

int label_launches(const Src& src, unsigned int* lab, int nprob, int conn8, int* status, hipStream_t st) {
    const int H = src.H, W = src.W;
    hipLaunchKernelGGL(object_runs_kernel, dim3(H, nprob), dim3(kRowThreads), 0, st, src, lab);
    SBGM_LAUNCH_CHECK();
    hipLaunchKernelGGL(object_merge_kernel, dim3(pix_blocks(H * W), nprob), dim3(kPix), 0, st, lab, H, W, conn8, status);
    SBGM_LAUNCH_CHECK();
    hipLaunchKernelGGL(object_flatten_kernel, dim3(pix_blocks(H * W), nprob), dim3(kPix), 0, st, lab, H, W, status);
    SBGM_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" {

int sbgm_object_labels(const float* fields, const void* mask, int mask_is_u8, int N, int Nm, int H, int W, float threshold,
                       int connectivity, int* labels, int* status, void* stream) {
    hipStream_t st = ST;
    SBGM_CHECK(fields && labels && status, "object_labels: null argument");
    SBGM_CHECK(field_shape_ok(N, H, W), "object_labels: N=%d H=%d W=%d (N 1..65535, sides 2..%d, H*W <= 2^20)", N, H, W, kMaxSide);
    SBGM_CHECK(!mask || Nm == 1 || Nm == N, "object_labels: mask has %d fields; need 1 or N=%d", Nm, N);
    SBGM_CHECK(connectivity == 4 || connectivity == 8, "object_labels: connectivity %d; need 4 or 8", connectivity);
    SBGM_CHECK(std::isfinite(threshold), "object_labels: the threshold is not finite");
    Src src{fields, fields, mask, mask_is_u8, 1, Nm == 1 ? 0 : 1, N, H, W, 1, 0, 0, 1, 1, nullptr, threshold};
    if (int rc = sbgm_zero_async(status, sizeof(int), st)) return rc;
    unsigned int* lab = reinterpret_cast<unsigned int*>(labels);
    if (int rc = label_launches(src, lab, N, connectivity == 8, status, st)) return rc;
    hipLaunchKernelGGL(object_spread_kernel, dim3(pix_blocks(H * W), N), dim3(kPix), 0, st, lab, H, W);
    SBGM_LAUNCH_CHECK();
    return 0;
}

int64_t sbgm_object_scores_workspace_bytes(int N, int H, int W, int T, int64_t max_bytes) {
    if (!field_shape_ok(N, H, W) || T < 1 || T > kMaxThr + 1) return 0;
    return head_bytes(N) + chunk_plan(N, H, W, T, max_bytes).pairs * pair_bytes(H, W);
}

int sbgm_object_scores(const float* gen, const float* obs, const void* mask, int mask_is_u8, int N, int No, int Nm, int H, int W,
                       const float* thresholds, int n_fixed, int has_relative, double rel_factor, double rel_quantile, float rel_wet,
                       int connectivity, float* threshold, int64_t* n_objects, int64_t* area, double* mass, double* V, double* r,
                       double* domain_mean, double* com, int64_t* valid, double* S, double* L2, double* A, double* L1, double* L,
                       int64_t* area_hist, int* status, void* workspace, int64_t workspace_bytes, void* stream) {
    hipStream_t st = ST;
    SBGM_CHECK(gen && obs && threshold && n_objects && area && mass && V && r && domain_mean && com && valid && S && L2 && A && L1 && L &&
               area_hist && status && workspace, "object_scores: null argument");
    SBGM_CHECK(field_shape_ok(N, H, W), "object_scores: N=%d H=%d W=%d (N 1..65535, sides 2..%d, H*W <= 2^20)", N, H, W, kMaxSide);
    SBGM_CHECK(No == 1 || No == N, "object_scores: obs has %d fields; need 1 or N=%d", No, N);
    SBGM_CHECK(!mask || Nm == 1 || Nm == N, "object_scores: mask has %d fields; need 1 or N=%d", Nm, N);
    SBGM_CHECK(connectivity == 4 || connectivity == 8, "object_scores: connectivity %d; need 4 or 8", connectivity);
    SBGM_CHECK(n_fixed >= 0 && n_fixed <= kMaxThr && (n_fixed == 0 || thresholds), "object_scores: %d fixed thresholds (0..%d)", n_fixed,
               kMaxThr);
    const int T = n_fixed + (has_relative ? 1 : 0);
    SBGM_CHECK(T >= 1, "object_scores: no threshold given");
    ThrList thr;
    if (int rc = fill_thresholds("object_scores", thresholds, n_fixed, thr)) return rc;
    if (has_relative)
        SBGM_CHECK(std::isfinite(rel_factor) && rel_quantile >= 0.0 && rel_quantile <= 1.0 && std::isfinite(rel_wet),
                   "object_scores: relative threshold needs a finite factor, a quantile in [0, 1] and a finite wet value");
    const int64_t pb = pair_bytes(H, W), hb = head_bytes(N);
    SBGM_CHECK(workspace_bytes >= hb + pb, "object_scores: workspace of %lld bytes; one field x one threshold needs %lld",
               (long long)workspace_bytes, (long long)(hb + pb));
    const int HW = H * W, nseg = segments(HW);
    int* fexp = static_cast<int*>(workspace);
    char* chunk = static_cast<char*>(workspace) + hb;
    Src src{gen, obs, mask, mask_is_u8, No == 1 ? 0 : 1, Nm == 1 ? 0 : 1, N, H, W, T, 0, 0, T, 0, threshold, 0.f};
    if (int rc = sbgm_zero_async(status, sizeof(int), st)) return rc;
    if (int rc = sbgm_zero_async(area_hist, (size_t)2 * T * kHistBins * sizeof(int64_t), st)) return rc;
    hipLaunchKernelGGL(object_prepare_kernel, dim3(N, 2), dim3(kPrepThreads), 0, st, src, n_fixed, thr, has_relative, rel_factor,
                       rel_quantile, rel_wet, threshold, reinterpret_cast<long long*>(valid), domain_mean, com, fexp);
    SBGM_LAUNCH_CHECK();
    const int rc = for_each_chunk(chunk_plan(N, H, W, T, workspace_bytes), N, T, [&](int f0, int nf, int t0, int nt) -> int {
        const int np = 2 * nf * nt;
        // the chunk: part_sums fp64 [np][nseg][3], part_counts int64 [np][nseg][2], acc int64 [np][3][HW], area [np][HW],
        // peak [np][HW] (the last three zeroed together; np is even, so they start on a 16-byte boundary), then lab [np][HW]
        double* part_sums = reinterpret_cast<double*>(chunk);
        long long* part_counts = reinterpret_cast<long long*>(part_sums + (size_t)np * nseg * kPartSums);
        long long* acc = part_counts + (size_t)np * nseg * kPartCounts;
        unsigned int* ar = reinterpret_cast<unsigned int*>(acc + (size_t)np * 3 * HW);
        unsigned int* pk = ar + (size_t)np * HW;
        unsigned int* lab = pk + (size_t)np * HW;
        src.f0 = f0; src.t0 = t0; src.nt = nt;
        if (int rc = sbgm_zero_async(acc, (size_t)np * 32 * HW, st)) return rc;
        if (int rc = label_launches(src, lab, np, connectivity == 8, status, st)) return rc;
        hipLaunchKernelGGL(object_accumulate_kernel, dim3((HW + kAccBlock - 1) / kAccBlock, np), dim3(256), 0, st, src, lab, fexp, acc, ar,
                           pk);
        SBGM_LAUNCH_CHECK();
        hipLaunchKernelGGL(object_sums_kernel, dim3(nseg, np), dim3(kFinThreads), 0, st, src, fexp, acc, ar, pk, com, part_sums,
                           part_counts, reinterpret_cast<unsigned long long*>(area_hist));
        SBGM_LAUNCH_CHECK();
        hipLaunchKernelGGL(object_collect_kernel, dim3((np + 63) / 64), dim3(64), 0, st, src, part_sums, part_counts, nseg, np,
                           reinterpret_cast<long long*>(n_objects), reinterpret_cast<long long*>(area), mass, V, r);
        SBGM_LAUNCH_CHECK();
        return 0;
    });
    if (rc) return rc;
    hipLaunchKernelGGL(object_scores_kernel, dim3((N * T + 255) / 256), dim3(256), 0, st, N, T, H, W,
                       reinterpret_cast<const long long*>(valid), domain_mean, com, reinterpret_cast<const long long*>(n_objects), V, r, S,
                       L2, A, L1, L);
    SBGM_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
