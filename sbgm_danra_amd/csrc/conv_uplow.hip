// A decoder block's conv_up(up(x)) on a small map, with the channels mixed at LOW resolution.
//
// `up` (bilinear x2, align_corners = False) acts per channel and a 3x3 tap's weight acts per pixel, so the two commute:
//   conv_up(up(x))[co][o] = b[co] + sum_{tap = (k, l), o + tap - 1 inside the HIGH-res map} up(Z_tap)[co][o + tap - 1]
//   Z_tap[co]             = sum_ci W[co][ci][k][l] x[ci]                       on the low-resolution map
// The 9 tap mixes are ONE 1x1 product with N = 9 C over a quarter of the pixels (2 C^2 9/4 flop per output pixel instead of 2 C^2 9),
// run by the ordinary implicit-GEMM convolution from the image sbgm_launch_up_lowres_pack builds; Z is [B h w][9 C], row n = tap C + co.
// The gather below finishes the block from Z rows staged in LDS: the 9 taps through the bilinear x2 as a horizontal and a vertical pass
// (`up` is a tensor product of its two axes), the bias, and, where a workgroup holds a whole (sample, GroupNorm group), norm1 itself.
// A tap whose intermediate pixel lies outside the high-res map is skipped: that is the zero padding of conv_up's input.
#include "common.h"
#include "kernels.h"

namespace {

// w1[(tap C + co) C + ci] = w[co][ci][k][l], tap = 3 k + l: the OIHW [9 C][C][1][1] weight of the mix, a copy of every element
__global__ void up_taps_kernel(const float* __restrict__ w, float* __restrict__ w1, int C) {
    const size_t total = (size_t)9 * C * C;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int ci = (int)(i % C);
        const size_t r = i / C;
        const int co = (int)(r % C), tap = (int)(r / C);
        w1[i] = w[((size_t)co * C + ci) * 9 + tap];
    }
}

// The high-res positions p = o + k - 1 (k = 0..2) a 3x3 tap reads on one axis, each through its two low-res neighbours: an even
// position 2j reads 0.25 Z[j-1] + 0.75 Z[j], an odd one 0.75 Z[j] + 0.25 Z[j+1], the neighbour clamped at the map edge
// (upsample2x_kernel, lr_axis of conv_final.hip).
struct UpAxis { int a[3], b[3]; float wa[3]; bool in[3]; };
__device__ __forceinline__ UpAxis up_axis(int o, int n_lo) {
    UpAxis r;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int p = o + k - 1, j = p >> 1;
        r.in[k] = (unsigned)p < (unsigned)(2 * n_lo);
        if (p & 1) { r.a[k] = j; r.b[k] = min(j + 1, n_lo - 1); r.wa[k] = 0.75f; }
        else { r.a[k] = max(j - 1, 0); r.b[k] = j; r.wa[k] = 0.25f; }
    }
    return r;
}
// first / last low-res row a high-res row p (inside the map) reads
__host__ __device__ inline int up_lo(int p) { return (p & 1) ? p >> 1 : ((p >> 1) > 0 ? (p >> 1) - 1 : 0); }
__host__ __device__ inline int up_hi(int p, int n_lo) { return (p & 1) ? ((p >> 1) + 1 < n_lo ? (p >> 1) + 1 : n_lo - 1) : p >> 1; }

enum { UP_RAW = 0, UP_PARTIALS = 1, UP_NORMED = 2 };
struct UpGatherArgs {
    const float* z;          // [B][h][w][9 C]
    const float* bias;       // [C]
    float* out;              // [B][2h][2w][C]
    const float *gamma, *beta;   // norm1's affine (UP_NORMED), may be null
    double* stats;           // UP_PARTIALS: [b][chunk][G][2], G = gridDim.x
    int h, w, C, CW;         // CW: channels of a workgroup's slice, a multiple of 4 (the GroupNorm group where statistics are formed)
    int rows;                // high-res rows per chunk (even; the whole map when gridDim.y == 1)
    int mode;
    float eps;
    int tps;                 // taps staged at a time: 9 (all of Z beside R) or 3 (one tap row ky at a time, three stagings)
    int rpp;                 // rows a sweep of the workgroup covers: blockDim / (2 w CW / 4), at least 1
    int sl, st, sq;          // blockDim as a step of the staging index: sl pixels + st taps + sq channel quads
};

constexpr int UP_MAX_THREADS = 1024;
constexpr int UP_MAX_ITEMS = 8;      // the largest register-resident instantiation (16 spills under the 128 VGPRs of 1024 threads)

// Grid (channel slices, row chunks, B).  The bilinear x2 is separable, so a workgroup works in two passes over the low-res rows its
// chunk reads.  Z rows are staged as z[pixel][tap][CW] (all 9 taps, or one tap row ky at a time where 9 do not fit beside R);
//   horizontal  R[ky][j][ox] = sum_kx in_x(kx) (wx Z[ky, kx][j][xa] + (1 - wx) Z[ky, kx][j][xb])       low-res row j, high-res column ox
//   vertical    out[oy][ox]  = b + sum_ky in_y(ky) (wy R[ky][ya][ox] + (1 - wy) R[ky][yb][ox])
// R lives in LDS behind Z.  A thread keeps one (column, channel quad) for both sweeps (lanes along the channels: 16-byte LDS accesses
// of consecutive addresses) and walks the rows r0, r0 + rpp, ..: the column's geometry is computed once, a row's from the loop counter.
// With statistics every thread adds its values in fp64 in row order, the waves combine by butterfly and the workgroup in wave order: no
// atomics, the same sum in every run.  UP_NORMED (one chunk: the workgroup holds the whole (sample, group)) with NI > 0: the thread's
// NI output values stay in registers across the statistics barrier and are stored once, normalised as groupnorm_apply_kernel does.
// NI == 0 is the general form (any number of columns and rows per thread): raw values are stored as they are formed, and UP_NORMED
// reads back what the thread itself stored.
template <int NI>
__global__ __launch_bounds__(UP_MAX_THREADS) void up_gather_kernel(UpGatherArgs a) {
    extern __shared__ __attribute__((aligned(16))) float s[];
    __shared__ double red[2 * UP_MAX_THREADS / 64];
    const int tid = threadIdx.x, nt = blockDim.x, slice = blockIdx.x, chunk = blockIdx.y, b = blockIdx.z;
    const int H = 2 * a.h, W = 2 * a.w, C = a.C, qs = a.CW >> 2, c0 = slice * a.CW, cq = C >> 2;
    const int y0 = chunk * a.rows, y1 = min(H, y0 + a.rows);
    const int ly0 = up_lo(max(y0 - 1, 0)), ly1 = up_hi(min(y1, H - 1), a.h), nl = ly1 - ly0 + 1;
    const int tps = a.tps, row_q = tps * qs, n_px = nl * a.w;
    f32x4* const z4 = reinterpret_cast<f32x4*>(s);
    f32x4* const r4 = z4 + n_px * row_q;                       // R[3][nl][W][qs]
    const int col = W * qs, r0 = tid / col, cid0 = tid - r0 * col;
    const bool active = r0 < a.rpp;                            // the threads past the last whole sweep row only stage
    // staging: item i = (pixel lp, tap, quad q) flattened, i = tid, tid + nt, ..; the step is applied with carries
    const int lp0 = tid / row_q, rem0 = tid - lp0 * row_q, tap0 = rem0 / qs, q0 = rem0 - tap0 * qs;
    for (int stage = 0; stage * tps < 9; ++stage) {
        if (stage) __syncthreads();                            // the horizontal pass of the tap row before is done with Z
        const f32x4* const zq = reinterpret_cast<const f32x4*>(a.z) + ((size_t)b * a.h + ly0) * a.w * (size_t)(9 * cq) + (c0 >> 2) + stage * tps * cq;
        int lp = lp0, tap = tap0, q = q0, i = tid;
        while (lp < n_px) {
            f32x4 v[4];
            int at[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {                      // four loads in flight
                at[u] = lp < n_px ? i : -1;
                if (lp < n_px) v[u] = zq[(size_t)lp * (9 * cq) + tap * cq + q];
                i += nt;
                q += a.sq;
                if (q >= qs) { q -= qs; ++tap; }
                tap += a.st;
                if (tap >= tps) { tap -= tps; ++lp; }
                lp += a.sl;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (at[u] >= 0) z4[at[u]] = v[u];
        }
        __syncthreads();
        for (int cid = cid0; cid < col && active; cid += nt) {
            const int ox = cid / qs, q = cid - ox * qs;
            const UpAxis rx = up_axis(ox, a.w);
            for (int j = r0; j < nl; j += a.rpp) {
                const f32x4* const zr = z4 + j * a.w * row_q + q;
#pragma unroll
                for (int kl = 0; kl < 3; ++kl) {
                    if (tps == 3 && kl) break;
                    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx) {
                        if (!rx.in[kx]) continue;
                        const f32x4* const t = zr + (kl * 3 + kx) * qs;
                        const float wx = rx.wa[kx];
                        acc += wx * t[rx.a[kx] * row_q] + (1.f - wx) * t[rx.b[kx] * row_q];
                    }
                    r4[(((stage + kl) * nl + j) * W + ox) * qs + q] = acc;
                }
            }
        }
    }
    __syncthreads();
    f32x4* const ob = reinterpret_cast<f32x4*>(a.out) + (size_t)b * H * W * cq + (c0 >> 2);
    double sm = 0.0, sq = 0.0;
    // one output element from the column's R entries (rq = r4 + ox qs + q)
    auto vertical = [&](const f32x4* rq, int oy, f32x4 v) {
        const UpAxis ry = up_axis(oy, a.h);
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            if (!ry.in[ky]) continue;
            const f32x4* const t = rq + ky * nl * col;
            const float wy = ry.wa[ky];
            v += wy * t[(ry.a[ky] - ly0) * col] + (1.f - wy) * t[(ry.b[ky] - ly0) * col];
        }
        return v;
    };
    f32x4 keep[NI > 0 ? NI : 1];
    if constexpr (NI > 0) {                                    // one column per thread, at most NI rows: the values stay in registers
        const int ox = cid0 / qs, q = cid0 - ox * qs;
        const f32x4 bq = *reinterpret_cast<const f32x4*>(a.bias + c0 + 4 * q);
#pragma unroll
        for (int k = 0; k < NI; ++k) {
            const int oy = r0 + k * a.rpp;
            if (!active || oy >= H) continue;
            const f32x4 v = vertical(r4 + cid0, oy, bq);
            keep[k] = v;
#pragma unroll
            for (int e = 0; e < 4; ++e) { sm += (double)v[e]; sq += (double)v[e] * (double)v[e]; }
        }
    } else {
        for (int cid = cid0; cid < col && active; cid += nt) {
            const int ox = cid / qs, q = cid - ox * qs;
            const f32x4 bq = *reinterpret_cast<const f32x4*>(a.bias + c0 + 4 * q);
            for (int oy = y0 + r0; oy < y1; oy += a.rpp) {
                const f32x4 v = vertical(r4 + cid, oy, bq);
                ob[((size_t)oy * W + ox) * cq + q] = v;
                if (a.mode != UP_RAW) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) { sm += (double)v[e]; sq += (double)v[e] * (double)v[e]; }
                }
            }
        }
        if (a.mode == UP_RAW) return;
    }
    sm = wave_sum_d(sm);
    sq = wave_sum_d(sq);
    if ((tid & 63) == 0) { red[2 * (tid >> 6)] = sm; red[2 * (tid >> 6) + 1] = sq; }
    __syncthreads();
    double tot = red[0], tot2 = red[1];
    for (int wv = 1; wv < (nt >> 6); ++wv) { tot += red[2 * wv]; tot2 += red[2 * wv + 1]; }
    if (a.mode == UP_PARTIALS) {
        if (tid == 0) {
            double* o = a.stats + (((size_t)b * gridDim.y + chunk) * gridDim.x + slice) * 2;
            o[0] = tot;
            o[1] = tot2;
        }
        return;
    }
    const double inv_n = 1.0 / ((double)H * W * a.CW);
    const double mean = tot * inv_n;
    const double var = fmax(tot2 * inv_n - mean * mean, 0.0);
    const float mu = (float)mean, rstd = (float)(1.0 / sqrt(var + (double)a.eps));
    for (int cid = cid0; cid < col && active; cid += nt) {
        const int ox = cid / qs, q = cid - ox * qs, c = c0 + 4 * q;
        f32x4 g = f32x4{rstd, rstd, rstd, rstd}, bt = f32x4{0.f, 0.f, 0.f, 0.f};
        if (a.gamma != nullptr) {
            g *= *reinterpret_cast<const f32x4*>(a.gamma + c);
            bt = *reinterpret_cast<const f32x4*>(a.beta + c);
        }
        f32x4* const o = ob + (size_t)ox * cq + q;
        if constexpr (NI > 0) {
#pragma unroll
            for (int k = 0; k < NI; ++k) {
                const int oy = r0 + k * a.rpp;
                if (oy < H) o[(size_t)oy * W * cq] = (keep[k] - mu) * g + bt;
            }
        } else {
            for (int oy = y0 + r0; oy < y1; oy += a.rpp) {
                f32x4* const e = o + (size_t)oy * W * cq;
                *e = (*e - mu) * g + bt;
            }
        }
    }
}

constexpr size_t UP_LDS_MAX = 160 * 1024 - 512;      // staged Z rows and R of one workgroup (the reduction scratch is static)
constexpr int UP_MAX_CHUNKS = 64;                    // as many chunk partials as groupnorm_apply reduces

// Threads per workgroup: the grid of the network's blocks is one workgroup per CU, so this is the occupancy (DESIGN.md 3.1 has the
// measurements).  SBGM_UP_GATHER_THREADS = 256 / 512 / 1024 overrides it for such a measurement.
int up_threads() {
    static const int v = [] {
        const char* e = getenv("SBGM_UP_GATHER_THREADS");
        const int n = e ? atoi(e) : 0;
        return n == 256 || n == 512 || n == 1024 ? n : 1024;
    }();
    return v;
}

template <int NI>
int up_gather_launch(const UpGatherArgs& a, dim3 grid, int threads, size_t lds, hipStream_t st) {
    static bool attr = false;
    if (lds > 64 * 1024 && !attr) {
        SBGM_HIP(hipFuncSetAttribute((const void*)up_gather_kernel<NI>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)UP_LDS_MAX));
        attr = true;
    }
    hipLaunchKernelGGL(up_gather_kernel<NI>, grid, dim3(threads), lds, st, a);
    SBGM_LAUNCH_CHECK();
    return 0;
}

}  // namespace

size_t sbgm_up_lowres_weight_floats(int C) { return (size_t)9 * C * C; }
size_t sbgm_up_lowres_ws_floats(int B, int h, int w, int C) { return (size_t)B * h * w * 9 * C; }

int sbgm_launch_up_lowres_pack(const float* w_oihw, float* w_taps, float* w_packed, int C, hipStream_t st) {
    SBGM_CHECK(w_oihw && w_taps && w_packed, "up_lowres_pack: null tensor");
    SBGM_CHECK(C >= 16 && C % 16 == 0 && C <= 4096, "up_lowres_pack: C=%d must be a multiple of 16, at most 4096", C);
    const size_t total = sbgm_up_lowres_weight_floats(C);
    hipLaunchKernelGGL(up_taps_kernel, dim3((unsigned)std::min<size_t>((total + 255) / 256, 65536)), dim3(256), 0, st, w_oihw, w_taps, C);
    SBGM_LAUNCH_CHECK();
    return sbgm_launch_pack_conv_weight(w_taps, w_packed, 9 * C, C, 1, 1, C, st);
}

int sbgm_launch_up_gather(const float* z, const float* bias, float* out, const float* gamma, const float* beta, double* stats, int G,
                          float eps, int B, int h, int w, int C, int* chunks_out, int* normed_out, hipStream_t st) {
    SBGM_CHECK(z && bias && out && chunks_out && normed_out, "up_gather: null tensor");
    SBGM_CHECK(B >= 1 && B <= 65535 && h >= 1 && w >= 1 && C >= 16 && C % 16 == 0, "up_gather: B=%d h=%d w=%d C=%d", B, h, w, C);
    SBGM_CHECK((long long)B * h * w * 4 * C < (1ll << 31), "up_gather: too many elements");
    SBGM_CHECK((gamma == nullptr) == (beta == nullptr), "up_gather: gamma and beta go together");
    // statistics are formed where a workgroup's channel slice can be a GroupNorm group (G = 0: none wanted)
    bool aware = G > 0 && stats != nullptr && C % G == 0 && (C / G) % 4 == 0;
    int CW = aware ? C / G : 16;
    const int H = 2 * h;
    int rows = H, chunks = 1, tps = 9;
    // The LDS plan, per low-res pixel of the slice: Z with all 9 taps beside R (36 + 24 bytes per channel); else Z one tap row at a time
    // beside R (12 + 24); else row chunks of the latter.  false: not even two output rows fit
    auto fit = [&]() {
        const size_t ch_bytes = (size_t)CW * 4;
        rows = H; chunks = 1; tps = 9;
        if ((size_t)h * w * 15 * ch_bytes <= UP_LDS_MAX) return true;
        tps = 3;
        if ((size_t)h * w * 9 * ch_bytes <= UP_LDS_MAX) return true;
        const size_t lo_rows = UP_LDS_MAX / ((size_t)w * 9 * ch_bytes);      // an even chunk of R rows reads R / 2 + 2 low-res rows
        if (lo_rows < 3) return false;
        rows = (int)std::min<size_t>(2 * (lo_rows - 2), (size_t)H);
        chunks = (H + rows - 1) / rows;
        return true;
    };
    bool ok = fit();
    if (aware && (!ok || chunks > UP_MAX_CHUNKS)) { aware = false; CW = 16; ok = fit(); }
    SBGM_CHECK(ok && chunks <= 65535, "up_gather: a low-res row of %d pixels does not fit the LDS", w);
    const int lo_rows = chunks == 1 ? h : std::min(h, rows / 2 + 2);
    const size_t lds = (size_t)lo_rows * w * (tps + 6) * CW * 4;
    const int threads = up_threads(), qs = CW / 4, col = 2 * w * qs, row_q = tps * qs;
    UpGatherArgs a{z, bias, out, gamma, beta, stats, h, w, C, CW, rows, aware ? (chunks == 1 ? UP_NORMED : UP_PARTIALS) : UP_RAW, eps};
    a.tps = tps;
    a.rpp = std::max(1, threads / col);
    a.sl = threads / row_q; a.st = threads % row_q / qs; a.sq = threads % qs;
    // register-resident norm1: one column per thread and at most UP_MAX_ITEMS rows of it
    const int items = col <= threads ? (H + a.rpp - 1) / a.rpp : UP_MAX_ITEMS + 1;
    const dim3 grid(C / CW, chunks, B);
    int rc;
    if (a.mode != UP_NORMED || items > UP_MAX_ITEMS) rc = up_gather_launch<0>(a, grid, threads, lds, st);
    else if (items <= 1) rc = up_gather_launch<1>(a, grid, threads, lds, st);
    else if (items <= 2) rc = up_gather_launch<2>(a, grid, threads, lds, st);
    else if (items <= 4) rc = up_gather_launch<4>(a, grid, threads, lds, st);
    else rc = up_gather_launch<8>(a, grid, threads, lds, st);
    if (rc) return 1;
    *chunks_out = a.mode == UP_PARTIALS ? chunks : 0;
    *normed_out = a.mode == UP_NORMED;
    return 0;
}
