// Multivariate ensemble scores on the device:
//   K53 energy_scores    — squared Euclidean distances over the valid pixels between all M members of ens [M][HW] and the
//                          truth obs [HW] (row / column M of D2 [M+1][M+1]), and from them the energy score.
//   K54 variogram_scores — variogram score of order p over the pixel pairs whose offset lies in the half-plane disc of a
//                          radius <= 8: per-pixel map, per-offset domain-mean variograms and pair counts, the score.
// A pixel is valid when every member and the truth are not NaN there and the mask (uint8 != 0, or fp32 > 0.5) admits it.  The
// flag is computed once into the workspace (valid_kernel); an invalid pixel enters every sum as an exact +0 or not at all.
//
// K53.  Difference form only: every loaded fp32 value is converted to fp64 once, d = a - b and acc = fma(d, d, acc) in fp64.
// (The Gram form ||a||^2 + ||b||^2 - 2<a, b> cancels for near-identical members and is not used.)  A workgroup of 256 threads
// owns a tile of 16 x 16 row pairs (i_tile <= j_tile; the result is mirrored) and one pixel segment; each of its 4 waves owns
// an 8 x 8 quarter of the tile and runs its 64 lanes over all pixels of the segment, each lane holding the 64 pair
// accumulators in registers: 16 loads for 64 updates, and the four waves read the same 32 rows, so half of those loads hit
// the CU's L1.  The loads of a lane's next pixel are issued before the updates of the current one.  The segments are a
// function of (M, HW) alone (energy_plan), never of a grid size chosen at launch: the grid IS tiles x segments.  Per
// accumulator the 64 lanes of a wave are summed by an xor butterfly, and the segments in segment order by energy_collect from
// the partials in the workspace.  No atomics on floating-point values.
//
// K54.  A workgroup owns a tile of 8 x 32 pixels and one group of <= 32 offsets; lane = pixel, one fp64 accumulator per offset
// of the group in registers (the groups split the <= 98 offsets of a disc evenly, so no accumulator ever leaves the register
// file).  Member by member the tile and its halo (radius to the left, right and below) are staged through LDS, double
// buffered: the loads of member m + 1 are in flight while member m is consumed.  |x_i - x_j|^p is formed in fp32 (p = 0.5:
// sqrtf, p = 1: identity, p = 2: square — three compiled paths, no powf), converted once and added in fp64 in member order.
// A pixel owns the pairs to its half-plane neighbours, so the map needs no atomics; per offset the block sums (butterfly, then
// waves in order) go to the workspace and variogram_collect adds the tiles in tile order.
// The helpers shared with the other verify files (validity, limits, block_sum_tree / block_min_tree) are in verify_common.h.
#include "verify_common.h"

#define ST ((hipStream_t)stream)

namespace {

constexpr int kThreads = 256;

// valid[p] and the number of valid pixels (a 64-bit integer atomic: exact in any order)
__global__ __launch_bounds__(kThreads) void valid_kernel(const float* __restrict__ ens, const float* __restrict__ obs,
                                                         const void* __restrict__ mask, int mask_u8, int M, size_t HW,
                                                         unsigned char* __restrict__ valid, unsigned long long* __restrict__ count) {
    const size_t p = (size_t)blockIdx.x * kThreads + threadIdx.x;
    bool v = false;
    if (p < HW) {
        v = mask_at(mask, mask_u8, p) && !is_nan(obs[p]);
        for (int m = 0; m < M && v; ++m) v = !is_nan(ens[(size_t)m * HW + p]);
        valid[p] = v;
    }
    const unsigned long long n = __popcll(__ballot(v));
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(count, n);
}

// ---- K53 ---------------------------------------------------------------------------------------------------------------------

constexpr int kTile = 8;                                  // 8 x 8 row pairs per wave: 64 fp64 accumulators per lane
constexpr int kBlockTile = 2 * kTile;                     // 16 x 16 row pairs per workgroup: its 4 waves as 2 x 2 such tiles
constexpr int kBlockPairs = kBlockTile * kBlockTile;
constexpr int64_t kEnergyPartialCap = 256LL << 20;        // bytes of per-segment partials the plan may ask for
constexpr int kEnergyBlocksWanted = 2048;                 // segments are added until the grid has this many workgroups
constexpr int64_t kEnergySegmentMax = 16384;              // pixels: all rows of one segment stay close to the caches

struct EnergyPlan {
    int N, T, ntiles, nseg;
    int64_t seg;                                          // pixels per segment, a multiple of kThreads
    int64_t off_count, off_part, off_rows, bytes;         // workspace layout
};

// the decomposition: a function of (M, HW) alone, so the order of every sum is too
EnergyPlan energy_plan(int M, int64_t HW) {
    EnergyPlan p{};
    p.N = M + 1;
    p.T = (p.N + kBlockTile - 1) / kBlockTile;
    p.ntiles = p.T * (p.T + 1) / 2;
    const int64_t max_seg = (HW + kThreads - 1) / kThreads;                              // a segment holds >= 256 pixels
    const int64_t by_blocks = (kEnergyBlocksWanted + p.ntiles - 1) / p.ntiles;
    const int64_t by_cache = (HW + kEnergySegmentMax - 1) / kEnergySegmentMax;
    const int64_t by_bytes = std::max<int64_t>(kEnergyPartialCap / ((int64_t)p.ntiles * kBlockPairs * 8), 1);
    int64_t nseg = std::max(by_blocks, std::min(by_cache, by_bytes));
    nseg = std::max<int64_t>(std::min(nseg, max_seg), 1);
    p.seg = ((HW + nseg - 1) / nseg + kThreads - 1) / kThreads * kThreads;
    p.nseg = (int)((HW + p.seg - 1) / p.seg);
    p.off_count = (HW + 255) / 256 * 256;
    p.off_part = p.off_count + 256;
    p.off_rows = p.off_part + (int64_t)p.nseg * p.ntiles * kBlockPairs * 8;
    p.bytes = p.off_rows + (int64_t)3 * p.N * 8;
    return p;
}

// row-major index of the upper triangle of a T x T tile grid -> (ti, tj), ti <= tj
__device__ __forceinline__ void tile_of(int t, int T, int& ti, int& tj) {
    const double b = 2.0 * T + 1.0;
    int i = (int)((b - sqrt(b * b - 8.0 * t)) * 0.5);
    i = max(0, min(i, T - 1));
    while (i > 0 && i * T - i * (i - 1) / 2 > t) --i;                                   // first index of row i
    while (i + 1 < T && (i + 1) * T - (i + 1) * i / 2 <= t) ++i;
    ti = i;
    tj = i + (t - (i * T - i * (i - 1) / 2));
}

__global__ __launch_bounds__(kThreads) void energy_pairs_kernel(const float* __restrict__ ens, const float* __restrict__ obs,
                                                                const unsigned char* __restrict__ valid, int M, size_t HW, int T,
                                                                int ntiles, size_t seg, double* __restrict__ partial) {
    const int tile = blockIdx.x % ntiles, s = blockIdx.x / ntiles;                      // segment-major: neighbours share pixels
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;     // scalar: row pointers stay in SGPRs
    const int wr = wave >> 1, wc = wave & 1;
    int ti, tj;
    tile_of(tile, T, ti, tj);
    if (ti == tj && wr > wc) return;                                                    // the mirror image of wave (0, 1): never read
    const float* ra[kTile];
    const float* rb[kTile];
#pragma unroll
    for (int r = 0; r < kTile; ++r) {                                                   // rows past M + 1 repeat the truth: never stored
        const int i = ti * kBlockTile + wr * kTile + r, j = tj * kBlockTile + wc * kTile + r;
        ra[r] = i < M ? ens + (size_t)i * HW : obs;
        rb[r] = j < M ? ens + (size_t)j * HW : obs;
    }
    double acc[kTile][kTile];
#pragma unroll
    for (int r = 0; r < kTile; ++r)
#pragma unroll
        for (int c = 0; c < kTile; ++c) acc[r][c] = 0.0;
    const size_t p0 = (size_t)s * seg, p1 = min(p0 + seg, HW);
    // the 16 loads of the next pixel are issued before the 64 updates of this one: with one wave a SIMD from each workgroup
    // there is little else to hide the latency of an ensemble that fits no cache (58.8 -> 32.0 ms at M = 1000, 589 x 789;
    // a ring of 2, 3 or 4 pixels in flight measured 31.4, 32.7 and 33.8 ms, so one is kept)
    float fa[kTile], fb[kTile];
    bool v = false;
    size_t p = p0 + lane;
    if (p < p1) {
        v = valid[p] != 0;
#pragma unroll
        for (int r = 0; r < kTile; ++r) { fa[r] = ra[r][p]; fb[r] = rb[r][p]; }
    }
    while (p < p1) {
        const size_t pn = p + 64;
        float na[kTile], nb[kTile];
        bool nv = false;
        if (pn < p1) {
            nv = valid[pn] != 0;
#pragma unroll
            for (int r = 0; r < kTile; ++r) { na[r] = ra[r][pn]; nb[r] = rb[r][pn]; }
        }
        double a[kTile], b[kTile];
#pragma unroll
        for (int r = 0; r < kTile; ++r) {
            a[r] = v ? (double)fa[r] : 0.0;                                             // an invalid pixel adds fma(0, 0, acc) = acc
            b[r] = v ? (double)fb[r] : 0.0;
        }
#pragma unroll
        for (int r = 0; r < kTile; ++r)
#pragma unroll
            for (int c = 0; c < kTile; ++c) {
                const double d = a[r] - b[c];
                acc[r][c] = __builtin_fma(d, d, acc[r][c]);
            }
        if (pn < p1) {
#pragma unroll
            for (int r = 0; r < kTile; ++r) { fa[r] = na[r]; fb[r] = nb[r]; }
        }
        v = nv;
        p = pn;
    }
    double* dst = partial + ((size_t)s * ntiles + tile) * kBlockPairs + wave * (kTile * kTile);
#pragma unroll
    for (int r = 0; r < kTile; ++r)
#pragma unroll
        for (int c = 0; c < kTile; ++c) {
            const double t = wave_sum_d(acc[r][c]);
            if (lane == 0) dst[r * kTile + c] = t;
        }
}

// D2 = sum of the segments' partials in segment order, mirrored
__global__ __launch_bounds__(kThreads) void energy_collect_kernel(const double* __restrict__ partial, int N, int T, int ntiles,
                                                                  int nseg, double* __restrict__ D2) {
    const int idx = blockIdx.x * kThreads + threadIdx.x;
    if (idx >= ntiles * kBlockPairs) return;
    const int tile = idx / kBlockPairs, e = idx % kBlockPairs, wave = e / (kTile * kTile), r = e / kTile % kTile, c = e % kTile;
    int ti, tj;
    tile_of(tile, T, ti, tj);
    const int i = ti * kBlockTile + (wave >> 1) * kTile + r, j = tj * kBlockTile + (wave & 1) * kTile + c;
    if (i >= N || j >= N || i > j) return;                                              // i > j only in diagonal tiles
    double v = 0.0;
    for (int s = 0; s < nseg; ++s) v += partial[((size_t)s * ntiles + tile) * kBlockPairs + e];
    D2[(size_t)i * N + j] = v;
    D2[(size_t)j * N + i] = v;
}

// member i: sum and minimum over the other members k of the RMS distance sqrt(D2[i][k] / count), and the distance to the truth
__global__ __launch_bounds__(kThreads) void energy_rows_kernel(const double* __restrict__ D2, const unsigned long long* __restrict__ count,
                                                               int M, double* __restrict__ rows) {
    __shared__ double sh[kThreads];
    const int i = blockIdx.x, N = M + 1;
    const double n = (double)*count;
    double sum = 0.0, mn = HUGE_VAL;
    for (int k = threadIdx.x; k < M; k += kThreads) {
        if (k == i) continue;
        const double d = sqrt(D2[(size_t)i * N + k] / n);
        sum += d;
        mn = fmin(mn, d);
    }
    sum = block_sum_tree<kThreads>(sum, sh);
    mn = block_min_tree<kThreads>(mn, sh);
    if (threadIdx.x == 0) {
        rows[i] = sum;
        rows[N + i] = mn;
        rows[2 * N + i] = sqrt(D2[(size_t)i * N + M] / n);
    }
}

__global__ __launch_bounds__(kThreads) void energy_scores_kernel(const double* __restrict__ rows, const unsigned long long* __restrict__ count,
                                                                 int M, double* __restrict__ scores) {
    __shared__ double sh[kThreads];
    const int N = M + 1;
    double pair = 0.0, obs = 0.0, mn = HUGE_VAL;
    for (int i = threadIdx.x; i < M; i += kThreads) {
        pair += rows[i];
        mn = fmin(mn, rows[N + i]);
        obs += rows[2 * N + i];
    }
    pair = block_sum_tree<kThreads>(pair, sh);
    obs = block_sum_tree<kThreads>(obs, sh);
    mn = block_min_tree<kThreads>(mn, sh);
    if (threadIdx.x == 0) {
        const double m = (double)M, n = (double)*count;
        const double mean_obs = obs / m;
        scores[0] = n;
        scores[1] = mean_obs - pair / (2.0 * m * (m - 1.0));
        scores[2] = mean_obs - pair / (2.0 * m * m);
        scores[3] = mean_obs;
        scores[4] = pair / (m * (m - 1.0));
        scores[5] = *count ? mn : nan_d();                                              // the sums are NaN by 0 / 0 already
    }
}

// ---- K54 ---------------------------------------------------------------------------------------------------------------------

constexpr int kMaxRadius = 8;
constexpr int kMaxOffsets = SBGM_VARIOGRAM_MAX_OFFSETS;
constexpr int kMaxGroup = 32;                             // offsets one workgroup carries: 32 fp64 accumulators per lane
constexpr int kTW = 32, kTH = 8;                          // pixels of a tile: a half-wave reads one LDS row, conflict-free
constexpr int kLW = kTW + 2 * kMaxRadius, kLH = kTH + kMaxRadius;
constexpr int kStage = (kLW * kLH + kThreads - 1) / kThreads;     // staged elements per thread and member

struct OffsetTable {
    int n;
    signed char dy[kMaxOffsets], dx[kMaxOffsets];
    float w[kMaxOffsets];                                 // 1 or 1 / distance
};

int build_offsets(int radius, int inverse_distance, OffsetTable& t) {
    t.n = 0;
    for (int dy = 0; dy <= radius; ++dy)
        for (int dx = -radius; dx <= radius; ++dx) {
            if (!(dy > 0 || dx > 0) || dy * dy + dx * dx > radius * radius) continue;
            t.dy[t.n] = (signed char)dy;
            t.dx[t.n] = (signed char)dx;
            t.w[t.n] = inverse_distance ? (float)(1.0 / std::sqrt((double)(dy * dy + dx * dx))) : 1.0f;
            ++t.n;
        }
    return t.n;
}

struct VarioPlan {
    int n_off, n_groups, group, tiles_x, tiles_y, ntiles;
    int64_t off_count, off_map, off_part, bytes;
};

VarioPlan vario_plan(int H, int W, int n_off) {
    VarioPlan p{};
    const int64_t HW = (int64_t)H * W;
    p.n_off = n_off;
    p.n_groups = (n_off + kMaxGroup - 1) / kMaxGroup;
    p.group = (n_off + p.n_groups - 1) / p.n_groups;
    p.tiles_x = (W + kTW - 1) / kTW;
    p.tiles_y = (H + kTH - 1) / kTH;
    p.ntiles = p.tiles_x * p.tiles_y;
    p.off_count = (HW + 255) / 256 * 256;
    p.off_map = p.off_count + 256;
    p.off_part = p.off_map + (int64_t)p.n_groups * HW * 8;
    p.bytes = p.off_part + (int64_t)p.ntiles * kMaxOffsets * 4 * 8;
    return p;
}

template <int ORDER2>                                     // twice the order: 1, 2 or 4
__device__ __forceinline__ float vario_pow(float d) {
    if (ORDER2 == 1) return sqrtf(fabsf(d));
    if (ORDER2 == 2) return fabsf(d);
    return d * d;
}

template <int G, int ORDER2>
__global__ __launch_bounds__(kThreads) void variogram_tiles_kernel(const float* __restrict__ ens, const float* __restrict__ obs,
                                                                   const unsigned char* __restrict__ valid, int M, int H, int W,
                                                                   int radius, OffsetTable tab, int group, int tiles_x,
                                                                   double* __restrict__ map_part, double* __restrict__ part) {
    __shared__ float buf[2][kLH * kLW];
    __shared__ unsigned char vld[kLH * kLW];
    __shared__ double wsum[kThreads / 64][3];
    __shared__ int wcnt[kThreads / 64];
    const int tile = blockIdx.x, g = blockIdx.y;
    const int ty0 = (tile / tiles_x) * kTH, tx0 = (tile % tiles_x) * kTW;
    const int o0 = g * group, ng = min(group, tab.n - o0);                              // this group: offsets o0 .. o0 + ng - 1
    const size_t HW = (size_t)H * W;
    // staged elements of this thread: LDS index and global pixel (-1 beyond the field: staged as 0 / invalid)
    int sidx[kStage];
    long long spix[kStage];
#pragma unroll
    for (int k = 0; k < kStage; ++k) {
        const int e = threadIdx.x + k * kThreads;
        const int ly = e / kLW, lx = e % kLW;
        const int y = ty0 + ly, x = tx0 + lx - kMaxRadius;
        const bool need = e < kLH * kLW && ly < kTH + radius && lx >= kMaxRadius - radius && lx < kMaxRadius + kTW + radius;
        sidx[k] = e < kLH * kLW ? e : -1;
        spix[k] = (need && y < H && x >= 0 && x < W) ? (long long)y * W + x : -1;
    }
#pragma unroll
    for (int k = 0; k < kStage; ++k)
        if (sidx[k] >= 0) vld[sidx[k]] = spix[k] >= 0 ? valid[spix[k]] : 0;
    // LDS displacement of every offset of the group (0 past the group's end: a pair with itself, dropped below)
    int disp[G];
#pragma unroll
    for (int k = 0; k < G; ++k) disp[k] = k < ng ? (int)tab.dy[o0 + k] * kLW + (int)tab.dx[o0 + k] : 0;
    const int row = threadIdx.x / kTW, col = threadIdx.x % kTW;
    const int centre = row * kLW + col + kMaxRadius;
    double acc[G];
#pragma unroll
    for (int k = 0; k < G; ++k) acc[k] = 0.0;
    float stage[kStage];
#pragma unroll
    for (int k = 0; k < kStage; ++k) stage[k] = spix[k] >= 0 ? ens[spix[k]] : 0.f;
    for (int m = 0; m < M; ++m) {
        float* cur = buf[m & 1];
#pragma unroll
        for (int k = 0; k < kStage; ++k)
            if (sidx[k] >= 0) cur[sidx[k]] = stage[k];
        __syncthreads();                                  // also orders this write after the reads of member m - 2
        if (m + 1 < M) {
            const float* next = ens + (size_t)(m + 1) * HW;
#pragma unroll
            for (int k = 0; k < kStage; ++k) stage[k] = spix[k] >= 0 ? next[spix[k]] : 0.f;
        }
        const float c = cur[centre];
#pragma unroll
        for (int k = 0; k < G; ++k) acc[k] += (double)vario_pow<ORDER2>(c - cur[centre + disp[k]]);
    }
    // the truth, staged the same way
    __syncthreads();
    float* cur = buf[0];
#pragma unroll
    for (int k = 0; k < kStage; ++k)
        if (sidx[k] >= 0) cur[sidx[k]] = spix[k] >= 0 ? obs[spix[k]] : 0.f;
    __syncthreads();
    const int y = ty0 + row, x = tx0 + col;
    const bool inside = y < H && x < W;
    const bool own = inside && vld[centre] != 0;
    const float c = cur[centre];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double map_sum = 0.0;
#pragma unroll
    for (int k = 0; k < G; ++k) {
        if (k < ng) {                                     // block-uniform
            const bool pv = own && vld[centre + disp[k]] != 0;
            const double go = (double)vario_pow<ORDER2>(c - cur[centre + disp[k]]);
            const double ge = acc[k] / (double)M;
            const double diff = go - ge;
            const double t = pv ? diff * diff : 0.0;
            map_sum += (double)tab.w[o0 + k] * t;
            const double s_ge = wave_sum_d(pv ? ge : 0.0), s_go = wave_sum_d(pv ? go : 0.0), s_t = wave_sum_d(t);
            const int n = __popcll(__ballot(pv));
            __syncthreads();
            if (lane == 0) {
                wsum[wave][0] = s_ge;
                wsum[wave][1] = s_go;
                wsum[wave][2] = s_t;
                wcnt[wave] = n;
            }
            __syncthreads();
            if (threadIdx.x < 4) {
                double* dst = part + ((size_t)tile * kMaxOffsets + (o0 + k)) * 4;
                if (threadIdx.x < 3) {
                    double v = wsum[0][threadIdx.x];
#pragma unroll
                    for (int w = 1; w < kThreads / 64; ++w) v += wsum[w][threadIdx.x];
                    dst[threadIdx.x] = v;
                } else {
                    int v = 0;
#pragma unroll
                    for (int w = 0; w < kThreads / 64; ++w) v += wcnt[w];
                    dst[3] = (double)v;                   // <= 256: exact
                }
            }
        }
    }
    if (inside) map_part[(size_t)g * HW + (size_t)y * W + x] = map_sum;
}

// vs_map = sum of the groups' partial maps in group order, NaN at an invalid pixel
__global__ __launch_bounds__(kThreads) void variogram_map_kernel(const double* __restrict__ map_part, const unsigned char* __restrict__ valid,
                                                                 size_t HW, int n_groups, float* __restrict__ vs_map) {
    const size_t p = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= HW) return;
    double v = 0.0;
    for (int g = 0; g < n_groups; ++g) v += map_part[(size_t)g * HW + p];
    vs_map[p] = valid[p] ? (float)v : nan_f();
}

// per offset the tiles in tile order; then the offsets in table order
__global__ __launch_bounds__(128) void variogram_collect_kernel(const double* __restrict__ part, int ntiles, OffsetTable tab,
                                                                double* __restrict__ gamma_ens, double* __restrict__ gamma_obs,
                                                                long long* __restrict__ pairs, double* __restrict__ scores) {
    __shared__ double st[kMaxOffsets], sn[kMaxOffsets];
    const int o = threadIdx.x;
    if (o < tab.n) {
        double ge = 0.0, go = 0.0, t = 0.0, n = 0.0;
        for (int b = 0; b < ntiles; ++b) {
            const double* src = part + ((size_t)b * kMaxOffsets + o) * 4;
            ge += src[0];
            go += src[1];
            t += src[2];
            n += src[3];                                  // integers below 2^53: exact
        }
        gamma_ens[o] = ge / n;
        gamma_obs[o] = go / n;
        pairs[o] = (long long)n;
        st[o] = t;
        sn[o] = n;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double num = 0.0, den = 0.0, unum = 0.0, n = 0.0;
        for (int k = 0; k < tab.n; ++k) {
            num += (double)tab.w[k] * st[k];
            den += (double)tab.w[k] * sn[k];
            unum += st[k];
            n += sn[k];
        }
        scores[0] = num / den;
        scores[1] = n;
        scores[2] = den;
        scores[3] = unum / n;
    }
}

template <int G>
int launch_variogram_tiles(int order2, dim3 grid, hipStream_t st, const float* ens, const float* obs, const unsigned char* valid, int M,
                           int H, int W, int radius, const OffsetTable& tab, int group, int tiles_x, double* map_part, double* part) {
    switch (order2) {
        case 1: hipLaunchKernelGGL((variogram_tiles_kernel<G, 1>), grid, dim3(kThreads), 0, st, ens, obs, valid, M, H, W, radius, tab,
                                   group, tiles_x, map_part, part); break;
        case 2: hipLaunchKernelGGL((variogram_tiles_kernel<G, 2>), grid, dim3(kThreads), 0, st, ens, obs, valid, M, H, W, radius, tab,
                                   group, tiles_x, map_part, part); break;
        default: hipLaunchKernelGGL((variogram_tiles_kernel<G, 4>), grid, dim3(kThreads), 0, st, ens, obs, valid, M, H, W, radius, tab,
                                    group, tiles_x, map_part, part); break;
    }
    SBGM_LAUNCH_CHECK();
    return 0;
}

int check_common(const char* op, const void* ens, const void* obs, int M, int64_t HW) {
    SBGM_CHECK(ens && obs, "%s: null argument", op);
    SBGM_CHECK(M >= 2 && M <= kMaxMembers, "%s: M=%d members (2..%d)", op, M, kMaxMembers);
    SBGM_CHECK(HW >= 1 && HW <= kMaxPixels, "%s: %lld pixels (1..2^20)", op, (long long)HW);
    return 0;
}

}  // namespace

extern "C" {

int64_t sbgm_energy_scores_workspace_bytes(int M, int64_t HW) {
    if (M < 2 || M > kMaxMembers || HW < 1 || HW > kMaxPixels) return 0;
    return energy_plan(M, HW).bytes;
}

int sbgm_energy_scores(const float* ens, const float* obs, const void* mask, int mask_is_u8, int M, int64_t HW, double* dist2,
                       double* scores, void* workspace, int64_t workspace_bytes, void* stream) {
    if (int rc = check_common("energy_scores", ens, obs, M, HW)) return rc;
    SBGM_CHECK(dist2 && scores && workspace, "energy_scores: null argument");
    const EnergyPlan pl = energy_plan(M, HW);
    SBGM_CHECK(workspace_bytes >= pl.bytes, "energy_scores: workspace of %lld bytes, need %lld", (long long)workspace_bytes,
               (long long)pl.bytes);
    char* ws = static_cast<char*>(workspace);
    unsigned char* valid = reinterpret_cast<unsigned char*>(ws);
    unsigned long long* count = reinterpret_cast<unsigned long long*>(ws + pl.off_count);
    double* partial = reinterpret_cast<double*>(ws + pl.off_part);
    double* rows = reinterpret_cast<double*>(ws + pl.off_rows);
    if (int rc = sbgm_zero_async(count, 8, ST)) return rc;
    hipLaunchKernelGGL(valid_kernel, dim3((unsigned)((HW + kThreads - 1) / kThreads)), dim3(kThreads), 0, ST, ens, obs, mask, mask_is_u8,
                       M, (size_t)HW, valid, count);
    SBGM_LAUNCH_CHECK();
    hipLaunchKernelGGL(energy_pairs_kernel, dim3((unsigned)pl.ntiles * (unsigned)pl.nseg), dim3(kThreads), 0, ST, ens, obs, valid, M,
                       (size_t)HW, pl.T, pl.ntiles, (size_t)pl.seg, partial);
    SBGM_LAUNCH_CHECK();
    const int entries = pl.ntiles * kBlockPairs;
    hipLaunchKernelGGL(energy_collect_kernel, dim3((entries + kThreads - 1) / kThreads), dim3(kThreads), 0, ST, partial, pl.N, pl.T,
                       pl.ntiles, pl.nseg, dist2);
    SBGM_LAUNCH_CHECK();
    hipLaunchKernelGGL(energy_rows_kernel, dim3(M), dim3(kThreads), 0, ST, dist2, count, M, rows);
    SBGM_LAUNCH_CHECK();
    hipLaunchKernelGGL(energy_scores_kernel, dim3(1), dim3(kThreads), 0, ST, rows, count, M, scores);
    SBGM_LAUNCH_CHECK();
    return 0;
}

int sbgm_variogram_offsets(int radius, int* n_offsets, int* dydx) {
    SBGM_CHECK(n_offsets && dydx, "variogram_offsets: null argument");
    SBGM_CHECK(radius >= 1 && radius <= kMaxRadius, "variogram_offsets: radius=%d (1..%d)", radius, kMaxRadius);
    OffsetTable t;
    *n_offsets = build_offsets(radius, 0, t);
    for (int k = 0; k < t.n; ++k) {
        dydx[2 * k] = t.dy[k];
        dydx[2 * k + 1] = t.dx[k];
    }
    return 0;
}

int64_t sbgm_variogram_scores_workspace_bytes(int M, int H, int W, int radius) {
    if (M < 2 || M > kMaxMembers || H < 1 || W < 1 || (int64_t)H * W > kMaxPixels || radius < 1 || radius > kMaxRadius) return 0;
    OffsetTable t;
    return vario_plan(H, W, build_offsets(radius, 0, t)).bytes;
}

int sbgm_variogram_scores(const float* ens, const float* obs, const void* mask, int mask_is_u8, int M, int H, int W, int radius,
                          double order, int inverse_distance, float* vs_map, double* gamma_ens, double* gamma_obs, int64_t* pairs,
                          double* scores, void* workspace, int64_t workspace_bytes, void* stream) {
    SBGM_CHECK(H >= 1 && W >= 1, "variogram_scores: field size %dx%d", H, W);
    const int64_t HW = (int64_t)H * W;
    if (int rc = check_common("variogram_scores", ens, obs, M, HW)) return rc;
    SBGM_CHECK(vs_map && gamma_ens && gamma_obs && pairs && scores && workspace, "variogram_scores: null argument");
    SBGM_CHECK(radius >= 1 && radius <= kMaxRadius, "variogram_scores: radius=%d (1..%d)", radius, kMaxRadius);
    SBGM_CHECK(order == 0.5 || order == 1.0 || order == 2.0, "variogram_scores: order=%g (0.5, 1 or 2)", order);
    OffsetTable tab{};
    build_offsets(radius, inverse_distance != 0, tab);
    const VarioPlan pl = vario_plan(H, W, tab.n);
    SBGM_CHECK(workspace_bytes >= pl.bytes, "variogram_scores: workspace of %lld bytes, need %lld", (long long)workspace_bytes,
               (long long)pl.bytes);
    char* ws = static_cast<char*>(workspace);
    unsigned char* valid = reinterpret_cast<unsigned char*>(ws);
    unsigned long long* count = reinterpret_cast<unsigned long long*>(ws + pl.off_count);
    double* map_part = reinterpret_cast<double*>(ws + pl.off_map);
    double* part = reinterpret_cast<double*>(ws + pl.off_part);
    if (int rc = sbgm_zero_async(count, 8, ST)) return rc;
    const unsigned pix_blocks = (unsigned)((HW + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(valid_kernel, dim3(pix_blocks), dim3(kThreads), 0, ST, ens, obs, mask, mask_is_u8, M, (size_t)HW, valid, count);
    SBGM_LAUNCH_CHECK();
    const int order2 = (int)(order * 2.0);
    const dim3 grid(pl.ntiles, pl.n_groups);
    int rc;
    if (pl.group <= 2) rc = launch_variogram_tiles<2>(order2, grid, ST, ens, obs, valid, M, H, W, radius, tab, pl.group, pl.tiles_x, map_part, part);
    else if (pl.group <= 8) rc = launch_variogram_tiles<8>(order2, grid, ST, ens, obs, valid, M, H, W, radius, tab, pl.group, pl.tiles_x, map_part, part);
    else if (pl.group <= 16) rc = launch_variogram_tiles<16>(order2, grid, ST, ens, obs, valid, M, H, W, radius, tab, pl.group, pl.tiles_x, map_part, part);
    else if (pl.group <= 25) rc = launch_variogram_tiles<25>(order2, grid, ST, ens, obs, valid, M, H, W, radius, tab, pl.group, pl.tiles_x, map_part, part);
    else rc = launch_variogram_tiles<32>(order2, grid, ST, ens, obs, valid, M, H, W, radius, tab, pl.group, pl.tiles_x, map_part, part);
    if (rc) return rc;
    hipLaunchKernelGGL(variogram_map_kernel, dim3(pix_blocks), dim3(kThreads), 0, ST, map_part, valid, (size_t)HW, pl.n_groups, vs_map);
    SBGM_LAUNCH_CHECK();
    hipLaunchKernelGGL(variogram_collect_kernel, dim3(1), dim3(128), 0, ST, part, pl.ntiles, tab, gamma_ens, gamma_obs,
                       reinterpret_cast<long long*>(pairs), scores);
    SBGM_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
