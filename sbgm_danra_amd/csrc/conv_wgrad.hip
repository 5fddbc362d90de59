// Weight gradients of the training path's convolutions and linears (reference: the dW / db that `loss.backward()` leaves on every
// nn.Conv2d and nn.Linear of sbgm/score_unet.py): the kernel bodies, the host planner that picks one of them for a geometry
// (sbgm_wgrad_plan), the launcher (sbgm_launch_conv_wgrad) and the deferred, batched form of a backward sweep (sbgm_launch_wgrad_flush).
#include <cstdlib>
#include <vector>
#include "common.h"
#include "kernels.h"

namespace {

inline int stream_blocks(size_t n) { return (int)std::min<size_t>((n + 255) / 256, 2048); }

// =====================================================================================================================
// Convolution weight gradient:  dW[tap][co][ci] += sum_p dy[p][co] * x[p @ tap][ci]        (fp32 MFMA 16x16x4)
// GEMM roles: rows = output channels, cols = input channels, K = pixels.  A lane's 16-byte dy load holds 4 CHANNELS of
// one pixel, so MFMA i of a group uses element i and owns the rows {4r+i}: 4 accumulator sets cover 64 channels, the
// K index of the instruction is the pixel (lane>>4).  x is read one dword per lane (16 consecutive channels of the
// tap-shifted pixel).  Workgroups split the pixel range; partial sums are combined with fp32 atomics.
// =====================================================================================================================
template <int FCI>   // 16*FCI input channels per wave
__global__ __launch_bounds__(256) void conv_wgrad_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                         float* __restrict__ dwp, int B, int H, int W, int Cs, int OH,
                                                         int OW, int Cout, int KH, int KW, int S, int PAD, int px_per_split,
                                                         float* __restrict__ dbias) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r16 = lane & 15, kq = lane >> 4;
    const int n_ci_t = (Cs + 16 * FCI - 1) / (16 * FCI), n_co_t = Cout / 64;
    int tile = blockIdx.x * 4 + wave;
    if (tile >= KH * KW * n_co_t * n_ci_t) return;
    const int ci_t = tile % n_ci_t; tile /= n_ci_t;
    const int co_t = tile % n_co_t; tile /= n_co_t;
    const int tap = tile;
    const int kh = tap / KW, kw = tap - kh * KW;
    const int co0 = co_t * 64, ci0 = ci_t * 16 * FCI;
    const int M = B * OH * OW;
    const int p_begin = blockIdx.y * px_per_split;
    const int p_end = min(M, p_begin + px_per_split);

    f32x4 acc[4][FCI];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < FCI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // operands of the 4-pixel group starting at p0 (this lane's pixel p0 + kq is the MFMA k index); zeros past the range / image
    const int OHW = OH * OW;
    auto load = [&](int p0, f32x4& a, float (&bv)[FCI]) {
        const int p = p0 + kq;
        a = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < FCI; ++j) bv[j] = 0.f;
        if (p < p_end) {
            a = *reinterpret_cast<const f32x4*>(dy + (size_t)p * Cout + co0 + 4 * r16);
            const int b = p / OHW;
            const int rr = p - b * OHW;
            const int oy = rr / OW, ox = rr - oy * OW;
            const int iy = oy * S - PAD + kh, ix = ox * S - PAD + kw;
            if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W) {
                // (a 16-byte x load per lane was measured: the lane->channel map it forces makes the epilogue's atomics strided
                //  and the step 30 % slower; the dword loads keep every atomic instruction on 64 contiguous bytes per row)
                const float* xp = x + (((size_t)b * H + iy) * W + ix) * Cs + ci0 + r16;
#pragma unroll
                for (int j = 0; j < FCI; ++j)
                    if (ci0 + 16 * j + r16 < Cs) bv[j] = xp[16 * j];
            }
        }
    };
    // bias gradient db[co] = sum_p dy[p][co] as a by-product: the waves of tap 0 / input-channel tile 0 already stream every dy
    // row of their output-channel slice once (removes a separate column-sum launch and its memset per convolution)
    const bool do_bias = dbias != nullptr && tap == 0 && ci_t == 0;
    f32x4 bsum = {0.f, 0.f, 0.f, 0.f};
    auto mma = [&](const f32x4& a, const float (&bv)[FCI]) {
        if (do_bias) bsum += a;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < FCI; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], bv[j], acc[i][j], 0, 0, 0);
    };
    // two register sets: the loads of the next group are in flight while the matrix pipe works on the current one
    f32x4 a0, a1;
    float b0[FCI], b1[FCI];
    load(p_begin, a0, b0);
    for (int p0 = p_begin; p0 < p_end; p0 += 8) {
        load(p0 + 4, a1, b1);
        mma(a0, b0);
        load(p0 + 8, a0, b0);
        mma(a1, b1);
    }
    if (do_bias) {                                   // lanes kq = 0..3 hold the same channels 4*r16..+3 for different pixels
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            bsum[e] += __shfl_xor(bsum[e], 16, 64);
            bsum[e] += __shfl_xor(bsum[e], 32, 64);
        }
        if (kq == 0) {
#pragma unroll
            for (int e = 0; e < 4; ++e) atomicAdd(dbias + co0 + 4 * r16 + e, bsum[e]);
        }
    }
    // D_i[row][col]: row = 4*kq + reg -> channel co0 + 4*row + i ; col = r16 -> ci0 + 16j + r16
    float* base = dwp + ((size_t)tap * Cout) * Cs;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < FCI; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int co = co0 + 4 * (4 * kq + e) + i;
                if (ci0 + 16 * j + r16 < Cs) atomicAdd(base + (size_t)co * Cs + ci0 + 16 * j + r16, acc[i][j][e]);
            }
}

// What the two LDS-staged families below share of one launch's arguments.  gx x gy is the launch's grid: a workgroup of column bx owns
// one (co, ci) block and walks tiles_per_wg pixel tiles; dw_direct != null: it is the block's only writer and stores OIHW itself.
struct WgHead {
    const float *dy, *x;
    float *dwp, *dbias, *dw_direct;
    int Cs, Cout, Cin, tiles_per_wg, gx, gy;
    uint32_t dy_bytes, x_bytes;
};
// The batched form of a family (every weight gradient of a backward sweep in one launch): the descriptors travel by value in the kernel
// arguments (no device table to fill under stream capture), and workgroup blockIdx.x serves the slot k with start[k] <= blockIdx.x <
// start[k + 1].
template <class D, int MAX>
struct WgTable {
    static constexpr int CAP = MAX;
    D d[MAX];
    int start[MAX + 1];
    int n;
};
template <class Table>
__device__ __forceinline__ int table_slot(const Table& t) {
    int k = 0;
    while (k + 1 < t.n && (int)blockIdx.x >= t.start[k + 1]) ++k;
    return k;
}

// =====================================================================================================================
// Weight gradient of a 3x3 / stride 1 / pad 1 convolution on maps whose sides are multiples of 16 (or 8 x 8), LDS-staged (the layers
// that dominate the backward pass: K = B*H*W pixels is long, Cout x Cin is small).  A workgroup of 8 waves owns ONE
// 32 x 32 (co x ci) block of all 9 taps and walks over 16 x 16 pixel tiles of its share of the images: per tile it stages
// dy[256 px][32 co] and the halo patch x[18 x 18 px][32 ci] in LDS once (16-byte global loads, zero padding from the
// buffer bounds check), then wave w accumulates rows 2w, 2w+1 of the tile into its own copy of the block with fp32 MFMAs
// whose K index is the pixel: 2 + 18 LDS dword reads feed 36 MFMAs per 4-pixel step.  The wave-level kernel above re-reads
// dy 9x and x 9x from global memory and spends most of its time on per-pixel index arithmetic.
// The 8 copies are folded through LDS tap by tap, so one workgroup sends 36 KB of fp32 atomics into the pre-zeroed
// [tap][Cout][Cs] slab, from which unpack_wgrad_kernel writes OIHW (a layer without a pixel split stores OIHW directly and
// needs neither).  That volume is what the epilogue costs (the atomic units take ~1.5 TB/s for 64-byte runs and longer;
// 4-byte scatter straight into OIHW costs twice as much): with 64 x 64 blocks split over 4 quarter-waves it was 4x larger
// and cost more than the matrix work at training batch sizes.
// Pixel stride in LDS = 48 floats: lanes (r16, kq) of a ds_read_b32 then fall on 64 distinct banks.
// =====================================================================================================================
constexpr int WG_PS = 48;                          // LDS floats per pixel
constexpr int WG_THREADS = 512;                    // 8 waves = 8 pixel groups
constexpr int WG_DY_FLOATS = 256 * WG_PS;
// TW = 16: tiles are 16 x 16 pixels of one image.  TW = 8 (8 x 8 maps): a tile is 4 whole images stacked, each with its own
// zero halo in the patch (4 x 10 rows of 10 pixels).
template <int TW> struct WgTile {
    static constexpr int PW = TW + 2, PH = TW == 16 ? 18 : 40, X_FLOATS = PH * PW * WG_PS;
    static constexpr size_t LDS = (size_t)(WG_DY_FLOATS + X_FLOATS) * 4;      // dynamic LDS bytes of a launch
};
struct HaloDesc : WgHead {
    int B, H, W;
};

template <int TW>
__device__ __forceinline__ void halo_wgrad_body(const HaloDesc& a, const int bx, const int by) {
    const float* __restrict__ dy = a.dy;
    const float* __restrict__ x = a.x;
    float* __restrict__ dwp = a.dwp;
    float* __restrict__ dbias = a.dbias;
    float* __restrict__ dw_direct = a.dw_direct;
    const int B = a.B, H = a.H, W = a.W, Cs = a.Cs, Cout = a.Cout, tiles_per_wg = a.tiles_per_wg, Cin = a.Cin;
    const uint32_t dy_bytes = a.dy_bytes, x_bytes = a.x_bytes;
    constexpr int PW = WgTile<TW>::PW, PH = WgTile<TW>::PH;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* dys = reinterpret_cast<float*>(smem_raw);                   // [256 px][48]
    float* xs = dys + WG_DY_FLOATS;                                    // [PH][PW][48]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, kq = lane >> 4;
    const int n_ci = Cs / 32;
    const int co0 = (bx / n_ci) * 32, ci0 = (bx % n_ci) * 32;
    const int tiles_x = W / 16, tiles_img = tiles_x * (H / 16);        // TW = 16 only
    const int n_tiles = TW == 16 ? B * tiles_img : (B + 3) / 4;
    const int t_begin = by * tiles_per_wg, t_end = min(n_tiles, t_begin + tiles_per_wg);
    const __amdgpu_buffer_rsrc_t dr = make_rsrc(dy, dy_bytes);
    const __amdgpu_buffer_rsrc_t xr = make_rsrc(x, x_bytes);

    f32x4 acc[9][2][2];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[t][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const bool do_bias = dbias != nullptr && ci0 == 0;
    float bsum[2] = {0.f, 0.f};

    // register-staged double buffering: the global loads of tile t+1 are in flight while the matrix pipe works on tile t
    constexpr int DY_QUADS = 256 * 8, X_QUADS = PH * PW * 8;
    constexpr int DYQ = DY_QUADS / WG_THREADS;                          // 4 dy quads per thread
    constexpr int XQ = (X_QUADS + WG_THREADS - 1) / WG_THREADS;         // 6 (7) x quads per thread
    f32x4 rdy[DYQ], rx[XQ];
    auto tile_load = [&](int t) {
        int b0, y0 = 0, x0 = 0;
        if (TW == 16) {
            b0 = t / tiles_img;
            const int r = t - b0 * tiles_img;
            y0 = (r / tiles_x) * 16;
            x0 = (r % tiles_x) * 16;
        } else {
            b0 = t * 4;
        }
#pragma unroll
        for (int u = 0; u < DYQ; ++u) {
            const int q = tid + WG_THREADS * u;
            const int px = q >> 3, c4 = (q & 7) * 4;
            int b, oy, ox;
            if (TW == 16) { b = b0; oy = y0 + (px >> 4); ox = x0 + (px & 15); }
            else { b = b0 + (px >> 6); oy = (px >> 3) & 7; ox = px & 7; }
            rdy[u] = buf_load4(dr, b < B ? (uint32_t)(((b * H + oy) * W + ox) * Cout + co0 + c4) * 4u : 0x80000000u);
        }
#pragma unroll
        for (int u = 0; u < XQ; ++u) {
            const int q = tid + WG_THREADS * u;
            const int pp = q >> 3, c4 = (q & 7) * 4;
            const int py = pp / PW, pxx = pp - py * PW;
            int b, iy;
            if (TW == 16) { b = b0; iy = y0 - 1 + py; }
            else { const int img = py / 10; b = b0 + img; iy = py - img * 10 - 1; }
            const int ix = x0 - 1 + pxx;
            const bool ok = (q < X_QUADS) & (b < B) & ((unsigned)iy < (unsigned)H) & ((unsigned)ix < (unsigned)W);
            rx[u] = buf_load4(xr, ok ? (uint32_t)(((b * H + iy) * W + ix) * Cs + ci0 + c4) * 4u : 0x80000000u);
        }
    };
    auto tile_store = [&]() {
#pragma unroll
        for (int u = 0; u < DYQ; ++u) {
            const int q = tid + WG_THREADS * u;
            *reinterpret_cast<f32x4*>(dys + (q >> 3) * WG_PS + (q & 7) * 4) = rdy[u];
        }
#pragma unroll
        for (int u = 0; u < XQ; ++u) {
            const int q = tid + WG_THREADS * u;
            if (q < X_QUADS) *reinterpret_cast<f32x4*>(xs + (q >> 3) * WG_PS + (q & 7) * 4) = rx[u];
        }
    };
    if (t_begin < t_end) tile_load(t_begin);
    for (int t = t_begin; t < t_end; ++t) {
        __syncthreads();                                              // the previous tile's reads are done
        tile_store();
        __syncthreads();
        if (t + 1 < t_end) tile_load(t + 1);
#pragma unroll 2
        for (int s = 0; s < 8; ++s) {                                  // this wave's 32 pixels: 8 steps of 4 consecutive pixels
            // this lane's pixel = the MFMA k index; prow = its row in the halo patch for kh = 0
            const int row = TW == 16 ? 2 * wave + (s >> 2) : 4 * wave + (s >> 1);
            const int col = (TW == 16 ? (s & 3) : (s & 1)) * 4 + kq;
            const int prow = TW == 16 ? row : row + 2 * (row >> 3);
            float a[2], bv[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = dys[(row * TW + col) * WG_PS + 16 * i + r16];
            if (do_bias) { bsum[0] += a[0]; bsum[1] += a[1]; }
#pragma unroll
            for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) {
                    const float* xp = xs + ((prow + kh) * PW + col + kw) * WG_PS + r16;
                    bv[0] = xp[0];
                    bv[1] = xp[16];
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int j = 0; j < 2; ++j)
                            acc[kh * 3 + kw][i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], bv[j], acc[kh * 3 + kw][i][j], 0, 0, 0);
                }
        }
    }
    if (do_bias) {                                   // lane (r16, kq) summed channel 16i+r16 over its pixels: fold the 4 kq groups
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            bsum[i] += __shfl_xor(bsum[i], 16, 64);
            bsum[i] += __shfl_xor(bsum[i], 32, 64);
            if (kq == 0) atomicAdd(dbias + co0 + 16 * i + r16, bsum[i]);
        }
    }
    // Fold the 8 copies through LDS tap by tap (the staging area is free now; two alternating 32 KB regions, one barrier per
    // tap); wave t % 8 sums tap t and sends its atomics.  D[row][col]: row = 4*kq + reg -> co, col = r16 -> ci
    f32x4* red = reinterpret_cast<f32x4*>(smem_raw);                   // [2][8 waves][4 (i,j)][64 lanes] x f32x4
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        f32x4* region = red + (t & 1) * 8 * 4 * 64;
        if (wave != (t & 7)) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) region[(wave * 4 + i * 2 + j) * 64 + lane] = acc[t][i][j];
        }
        __syncthreads();
        if (wave == (t & 7)) {
            float* base = dwp + ((size_t)t * Cout) * Cs;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    f32x4 o = acc[t][i][j];
#pragma unroll
                    for (int w = 0; w < 8; ++w)
                        if (w != (t & 7)) {
                            const f32x4 v = region[(w * 4 + i * 2 + j) * 64 + lane];
                            o[0] += v[0]; o[1] += v[1]; o[2] += v[2]; o[3] += v[3];
                        }
                    if (dw_direct) {                  // this workgroup is the only writer of its block: straight into OIHW
                        const int ci = ci0 + 16 * j + r16;
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (ci < Cin) dw_direct[((size_t)(co0 + 16 * i + 4 * kq + e) * Cin + ci) * 9 + t] = o[e];
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            atomicAdd(base + (size_t)(co0 + 16 * i + 4 * kq + e) * Cs + ci0 + 16 * j + r16, o[e]);
                    }
                }
        }
    }
}

template <int TW>
__global__ __launch_bounds__(WG_THREADS) void conv3x3_wgrad_lds_kernel(const HaloDesc a) { halo_wgrad_body<TW>(a, blockIdx.x, blockIdx.y); }

// Batched form (see the per-tap kernel's batched form below for the rationale): at batch 8 most of a step's 19 3x3 layers own 2-8 tiles
// per workgroup before the 9-tap LDS fold and 36 KB of atomics; launched together they split their pixels over far fewer workgroups.
constexpr int HALO_MAX = 30;
using HaloTable = WgTable<HaloDesc, HALO_MAX>;
template <int TW>
__global__ __launch_bounds__(WG_THREADS) void conv3x3_wgrad_batched_kernel(const HaloTable t) {
    const int k = __builtin_amdgcn_readfirstlane(table_slot(t));
    const int rel = blockIdx.x - t.start[k];
    const int gx = t.d[k].gx;
    halo_wgrad_body<TW>(t.d[k], rel % gx, rel / gx);
}

// =====================================================================================================================
// Weight gradient as one split-K GEMM per kernel tap, LDS-staged: dW[tap][co][ci] = sum_m dy[m][co] * x[pixel(m, tap)][ci].
// Serves 1x1 convolutions and nn.Linear (one tap), and every other geometry the halo kernel above does not take (3x3
// stride 2, 3x3 on 4x4 maps, the 8x8 stride-2 stem convolutions): a tap only shifts the input pixel, out-of-range pixels
// load zeros.  A workgroup of 8 waves owns one (tap, 64 co, 64 ci) block; per tile of 128 output pixels it stages
// dy[128][64] and x[128][64] once, wave w takes pixels 16w..16w+15 (4 MFMA k-steps) and keeps its own 64 x 64 partial
// block (16 accumulator quads: 8 LDS dword reads feed 16 MFMAs, 128 staged bytes per MFMA).  The 8 partial blocks fold
// through LDS; one atomic (or, without a pixel split, one plain OIHW store) per element and workgroup.
// stem != 0 (padded Cin = 8, KW = 8): the 64 "channels" of a block are the (kw, ci) pairs of one kernel row kh, which are
// 64 contiguous floats of the NHWC input row, and the slab is [kh][Cout][kw][8].
// =====================================================================================================================
constexpr int W1_PX = 128, W1_PS = 80;             // pixels per tile, LDS floats per pixel (64 channels + pad: conflict-free)
constexpr size_t TAP_LDS = (size_t)2 * W1_PX * W1_PS * 4;      // dynamic LDS bytes of a launch (the 128 x 128 form below needs less)
struct TapGeom {
    int Mo, OH, OW, H, W, stride, pad, KW, taps, stem;
};
struct TapDesc : WgHead {
    TapGeom g;
    int big;               // 1: 128 x 128 blocks over 64-pixel tiles (tap_wgrad_body128), 0: 64 x 64 blocks over 128-pixel tiles
};

__device__ __forceinline__ void tap_wgrad_body(const TapDesc& a, const int bx, const int by) {
    const float* __restrict__ dy = a.dy;
    const float* __restrict__ x = a.x;
    float* __restrict__ dwp = a.dwp;
    float* __restrict__ dbias = a.dbias;
    float* __restrict__ dw_direct = a.dw_direct;
    const TapGeom g = a.g;
    const int Cs = a.Cs, Cout = a.Cout, tiles_per_wg = a.tiles_per_wg, Cin = a.Cin;
    const uint32_t dy_bytes = a.dy_bytes, x_bytes = a.x_bytes;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* dys = reinterpret_cast<float*>(smem_raw);                   // [128 px][80]
    float* xs = dys + W1_PX * W1_PS;                                   // [128 px][80]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, kq = lane >> 4;
    const int n_ci = g.stem ? 1 : Cs / 64, n_co = Cout / 64;
    int blk = bx;
    const int ci0 = (blk % n_ci) * 64; blk /= n_ci;
    const int co0 = (blk % n_co) * 64;
    const int tap = blk / n_co;
    const int kh = g.stem ? tap : tap / g.KW, kw0 = g.stem ? 0 : tap - kh * g.KW;
    const int slab_cs = g.stem ? 64 : Cs;                              // floats per (tap, co) row of the slab
    dwp += (size_t)tap * Cout * slab_cs;
    const int n_tiles = (g.Mo + W1_PX - 1) / W1_PX;
    const int t_begin = by * tiles_per_wg, t_end = min(n_tiles, t_begin + tiles_per_wg);
    const __amdgpu_buffer_rsrc_t dr = make_rsrc(dy, dy_bytes);
    const __amdgpu_buffer_rsrc_t xr = make_rsrc(x, x_bytes);
    const bool shifted = g.stride != 1 || g.taps != 1 || g.pad != 0;

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const bool do_bias = dbias != nullptr && ci0 == 0 && tap == 0;
    float bsum[4] = {0.f, 0.f, 0.f, 0.f};

    constexpr int QPT = W1_PX * 16 / WG_THREADS;                       // 4 quads of each operand per thread
    f32x4 rdy[QPT], rx[QPT];
    auto tile_load = [&](int t) {
#pragma unroll
        for (int u = 0; u < QPT; ++u) {
            const int q = tid + WG_THREADS * u;
            const int p = t * W1_PX + (q >> 4), c4 = (q & 15) * 4;
            bool ok = p < g.Mo;
            uint32_t xoff = (uint32_t)(p * Cs + ci0 + c4);
            if (shifted) {
                const int b = p / (g.OH * g.OW), r = p - b * (g.OH * g.OW);
                const int oy = r / g.OW, ox = r - oy * g.OW;
                const int iy = oy * g.stride - g.pad + kh;
                const int ix = ox * g.stride - g.pad + (g.stem ? (c4 >> 3) : kw0);
                xoff = (uint32_t)(((b * g.H + iy) * g.W + ix) * Cs + (g.stem ? (c4 & 7) : ci0 + c4));
                rdy[u] = buf_load4(dr, ok ? (uint32_t)(p * Cout + co0 + c4) * 4u : 0x80000000u);
                ok = ok & ((unsigned)iy < (unsigned)g.H) & ((unsigned)ix < (unsigned)g.W);
            } else {
                rdy[u] = buf_load4(dr, ok ? (uint32_t)(p * Cout + co0 + c4) * 4u : 0x80000000u);
            }
            rx[u] = buf_load4(xr, ok ? xoff * 4u : 0x80000000u);
        }
    };
    auto tile_store = [&]() {
#pragma unroll
        for (int u = 0; u < QPT; ++u) {
            const int q = tid + WG_THREADS * u;
            *reinterpret_cast<f32x4*>(dys + (q >> 4) * W1_PS + (q & 15) * 4) = rdy[u];
            *reinterpret_cast<f32x4*>(xs + (q >> 4) * W1_PS + (q & 15) * 4) = rx[u];
        }
    };
    if (t_begin < t_end) tile_load(t_begin);
    for (int t = t_begin; t < t_end; ++t) {
        __syncthreads();                                              // the previous tile's reads are done
        tile_store();
        __syncthreads();
        if (t + 1 < t_end) tile_load(t + 1);
#pragma unroll
        for (int s = 0; s < 4; ++s) {                                  // this wave's 16 pixels: 4 steps of 4 pixels
            const int px = 16 * wave + 4 * s + kq;                      // this lane's pixel = the MFMA k index
            float a[4], bv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                a[i] = dys[px * W1_PS + 16 * i + r16];
                bv[i] = xs[px * W1_PS + 16 * i + r16];
            }
            if (do_bias) {
#pragma unroll
                for (int i = 0; i < 4; ++i) bsum[i] += a[i];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], bv[j], acc[i][j], 0, 0, 0);
        }
    }
    if (do_bias) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            bsum[i] += __shfl_xor(bsum[i], 16, 64);
            bsum[i] += __shfl_xor(bsum[i], 32, 64);
            if (kq == 0) atomicAdd(dbias + co0 + 16 * i + r16, bsum[i]);
        }
    }
    // Fold the 8 partial blocks through LDS in two halves of 8 sub-blocks (64 KB each): every wave stores its copy of the
    // half, then wave w sums sub-block w of it over the 8 copies.  D[row][col]: row = 4*kq + reg -> co, col = r16 -> ci
    f32x4* red = reinterpret_cast<f32x4*>(smem_raw);                   // [8 waves][8 sub-blocks][64 lanes] x f32x4
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        __syncthreads();                                              // staging reads / the previous half's reads are done
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) red[(wave * 8 + i * 4 + j) * 64 + lane] = acc[2 * h + i][j];
        __syncthreads();
        f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int w = 0; w < 8; ++w) {
            const f32x4 v = red[(w * 8 + wave) * 64 + lane];
            o[0] += v[0]; o[1] += v[1]; o[2] += v[2]; o[3] += v[3];
        }
        const int i = 2 * h + (wave >> 2), j = wave & 3;
        const int ci = ci0 + 16 * j + r16;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int co = co0 + 16 * i + 4 * kq + e;
            if (dw_direct) { if (ci < Cin) dw_direct[((size_t)co * Cin + ci) * g.taps + tap] = o[e]; }
            else atomicAdd(dwp + (size_t)co * slab_cs + ci, o[e]);
        }
    }
}

// The same GEMM on 128 (co) x 128 (ci) blocks: wave w owns the 64 x 64 sub-block (w & 1, (w >> 1) & 1) over one half (w >> 2) of a
// 64-pixel tile, so a staged byte feeds twice the MFMAs of the 64 x 64 form (32 instead of 16 flop per byte: that form re-reads dy once
// per input-channel block and runs at the L2's rate) and only TWO partial copies fold through LDS.  Cs and Cout multiples of 128.
constexpr int W2_PX = 64, W2_PS = 144;
__device__ __forceinline__ void tap_wgrad_body128(const TapDesc& a, const int bx, const int by) {
    const TapGeom g = a.g;
    const int Cs = a.Cs, Cout = a.Cout;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* dys = reinterpret_cast<float*>(smem_raw);                   // [64 px][144]
    float* xs = dys + W2_PX * W2_PS;                                   // [64 px][144]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, kq = lane >> 4;
    const int wi = wave & 1, wj = (wave >> 1) & 1, ph = wave >> 2;
    const int n_ci = Cs / 128, n_co = Cout / 128;
    int blk = bx;
    const int ci0 = (blk % n_ci) * 128; blk /= n_ci;
    const int co0 = (blk % n_co) * 128;
    const int tap = blk / n_co;
    const int kh = tap / g.KW, kw0 = tap - kh * g.KW;
    float* dwp = a.dwp + (size_t)tap * Cout * Cs;
    const int n_tiles = (g.Mo + W2_PX - 1) / W2_PX;
    const int t_begin = by * a.tiles_per_wg, t_end = min(n_tiles, t_begin + a.tiles_per_wg);
    const __amdgpu_buffer_rsrc_t dr = make_rsrc(a.dy, a.dy_bytes);
    const __amdgpu_buffer_rsrc_t xr = make_rsrc(a.x, a.x_bytes);
    const bool shifted = g.stride != 1 || g.taps != 1 || g.pad != 0;

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const bool do_bias = a.dbias != nullptr && ci0 == 0 && tap == 0 && wj == 0;
    float bsum[4] = {0.f, 0.f, 0.f, 0.f};

    constexpr int QPT = W2_PX * 32 / WG_THREADS;                       // 4 quads of each operand per thread
    f32x4 rdy[QPT], rx[QPT];
    auto tile_load = [&](int t) {
#pragma unroll
        for (int u = 0; u < QPT; ++u) {
            const int q = tid + WG_THREADS * u;
            const int p = t * W2_PX + (q >> 5), c4 = (q & 31) * 4;
            bool ok = p < g.Mo;
            uint32_t xoff = (uint32_t)(p * Cs + ci0 + c4);
            rdy[u] = buf_load4(dr, ok ? (uint32_t)(p * Cout + co0 + c4) * 4u : 0x80000000u);
            if (shifted) {
                const int b = p / (g.OH * g.OW), r = p - b * (g.OH * g.OW);
                const int oy = r / g.OW, ox = r - oy * g.OW;
                const int iy = oy * g.stride - g.pad + kh, ix = ox * g.stride - g.pad + kw0;
                xoff = (uint32_t)(((b * g.H + iy) * g.W + ix) * Cs + ci0 + c4);
                ok = ok & ((unsigned)iy < (unsigned)g.H) & ((unsigned)ix < (unsigned)g.W);
            }
            rx[u] = buf_load4(xr, ok ? xoff * 4u : 0x80000000u);
        }
    };
    auto tile_store = [&]() {
#pragma unroll
        for (int u = 0; u < QPT; ++u) {
            const int q = tid + WG_THREADS * u;
            *reinterpret_cast<f32x4*>(dys + (q >> 5) * W2_PS + (q & 31) * 4) = rdy[u];
            *reinterpret_cast<f32x4*>(xs + (q >> 5) * W2_PS + (q & 31) * 4) = rx[u];
        }
    };
    if (t_begin < t_end) tile_load(t_begin);
    for (int t = t_begin; t < t_end; ++t) {
        __syncthreads();
        tile_store();
        __syncthreads();
        if (t + 1 < t_end) tile_load(t + 1);
#pragma unroll
        for (int s = 0; s < 8; ++s) {                                  // this wave's 32 pixels: 8 steps of 4 pixels
            const int px = 32 * ph + 4 * s + kq;
            float av[4], bv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                av[i] = dys[px * W2_PS + 64 * wi + 16 * i + r16];
                bv[i] = xs[px * W2_PS + 64 * wj + 16 * i + r16];
            }
            if (do_bias) {
#pragma unroll
                for (int i = 0; i < 4; ++i) bsum[i] += av[i];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[j], acc[i][j], 0, 0, 0);
        }
    }
    if (do_bias) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            bsum[i] += __shfl_xor(bsum[i], 16, 64);
            bsum[i] += __shfl_xor(bsum[i], 32, 64);
            if (kq == 0) atomicAdd(a.dbias + co0 + 64 * wi + 16 * i + r16, bsum[i]);
        }
    }
    // fold the two pixel halves: waves 4..7 hand their sub-block to waves 0..3 through LDS (16 KB each)
    f32x4* red = reinterpret_cast<f32x4*>(smem_raw);                   // [4 sub-blocks][16 fragments][64 lanes]
    __syncthreads();
    if (ph == 1) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) red[((wave & 3) * 16 + i * 4 + j) * 64 + lane] = acc[i][j];
    }
    __syncthreads();
    if (ph == 1) return;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const f32x4 o = acc[i][j] + red[(wave * 16 + i * 4 + j) * 64 + lane];
            const int ci = ci0 + 64 * wj + 16 * j + r16;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int co = co0 + 64 * wi + 16 * i + 4 * kq + e;
                if (a.dw_direct) { if (ci < a.Cin) a.dw_direct[((size_t)co * a.Cin + ci) * g.taps + tap] = o[e]; }
                else atomicAdd(dwp + (size_t)co * Cs + ci, o[e]);
            }
        }
}

__global__ __launch_bounds__(WG_THREADS) void conv_tap_wgrad_lds_kernel(const TapDesc a) {
    if (a.big) tap_wgrad_body128(a, blockIdx.x, blockIdx.y);
    else tap_wgrad_body(a, blockIdx.x, blockIdx.y);
}

// Batched form.  At training batch sizes a step has ~27 of these GEMMs (16 attention linears, the stride-2 and 1x1 shortcut convolutions,
// the 3x3 layers on 4x4 maps, the two stems), 0.1-4 GFLOP each: launched one by one each fills the chip with ~256 workgroups that own a
// tile or two and then pay the LDS fold and 4096 atomics, 13.8 us per launch on average.  Queued during the backward sweep and
// launched together, the layers fill the chip between them, so every layer splits its pixels over far fewer workgroups.
constexpr int TAP_MAX = 28;
using TapTable = WgTable<TapDesc, TAP_MAX>;
__global__ __launch_bounds__(WG_THREADS) void conv_tap_wgrad_batched_kernel(const TapTable t) {
    const int k = __builtin_amdgcn_readfirstlane(table_slot(t));
    const int rel = blockIdx.x - t.start[k];
    const int gx = t.d[k].gx;
    if (t.d[k].big) tap_wgrad_body128(t.d[k], rel % gx, rel / gx);
    else tap_wgrad_body(t.d[k], rel % gx, rel / gx);
}

// The layout pass behind a slab: dwp [tap][Cout][Cs] -> OIHW [Cout][Cin][KH][KW], or (taps < 0) the stem's slab [kh][Cout][kw][8] ->
// OIHW [Cout][Cin][KH][8] with KH = -taps.  Block blk of the nblk that share the slab.
struct UnpackDesc { const float* src; float* dst; int Cout, Cin, Cs, taps; };
__device__ __forceinline__ void unpack_wgrad_body(const UnpackDesc& d, const int blk, const int nblk) {
    if (d.taps < 0) {
        const int KH = -d.taps;
        const size_t total = (size_t)d.Cout * d.Cin * KH * 8;
        for (size_t i = (size_t)blk * blockDim.x + threadIdx.x; i < total; i += (size_t)nblk * blockDim.x) {
            const int kw = (int)(i & 7);
            const int kh = (int)((i >> 3) % KH);
            const int ci = (int)((i / ((size_t)8 * KH)) % d.Cin);
            const int co = (int)(i / ((size_t)8 * KH * d.Cin));
            d.dst[i] = d.src[(((size_t)kh * d.Cout + co) * 8 + kw) * 8 + ci];
        }
        return;
    }
    const size_t total = (size_t)d.Cout * d.Cin * d.taps;
    for (size_t i = (size_t)blk * blockDim.x + threadIdx.x; i < total; i += (size_t)nblk * blockDim.x) {
        const int tap = (int)(i % d.taps);
        const int ci = (int)((i / d.taps) % d.Cin);
        const int co = (int)(i / ((size_t)d.taps * d.Cin));
        d.dst[i] = d.src[((size_t)tap * d.Cout + co) * d.Cs + ci];
    }
}
__global__ __launch_bounds__(256) void unpack_wgrad_kernel(const UnpackDesc d) { unpack_wgrad_body(d, blockIdx.x, gridDim.x); }

// Deferred form: every slab -> OIHW pass of a backward sweep in ONE launch, each slab with its own range of blocks.
constexpr int UNPACK_MAX = 48;
using UnpackTable = WgTable<UnpackDesc, UNPACK_MAX>;
__global__ __launch_bounds__(256) void unpack_wgrad_batched_kernel(const UnpackTable t) {
    const int k = table_slot(t);
    unpack_wgrad_body(t.d[k], blockIdx.x - t.start[k], t.start[k + 1] - t.start[k]);
}

// the tables travel in the kernel arguments: none may outgrow what it was with a descriptor struct per family
static_assert(sizeof(HaloTable) <= 2768 && sizeof(TapTable) <= 3480 && sizeof(UnpackTable) <= 1736, "a weight-gradient table grew");

}  // namespace

// ---- launchers -----------------------------------------------------------------------------------------------------
// Deferred forms (sbgm_wgrad_defer / sbgm_wgrad_flush in the C ABI), process-wide like the prezeroed switch.
// sbgm_wgrad_deferred bit 0: sbgm_launch_conv_wgrad queues its slab -> OIHW layout pass instead of launching it, and the flush at the end
// of the backward sweep runs all of them as one kernel; the caller keeps every queued slab alive and untouched until the flush.
// Bit 1: the LDS-staged GEMMs themselves are queued, one queue per launch group, and the flush runs each group as ONE batched launch —
// the caller then also keeps dy and x of every queued call alive until the flush.
int sbgm_wgrad_deferred = 0;

// one call of an LDS-staged family, before it becomes a launch's or a table's descriptor
struct WgCall {
    WgHead h;
    int B;
    TapGeom g;
    int family;            // SBGM_WG_*
};
static HaloDesc halo_desc(const WgCall& c) { return HaloDesc{c.h, c.B, c.g.H, c.g.W}; }
static TapDesc tap_desc(const WgCall& c) { return TapDesc{c.h, c.g, c.family == SBGM_WG_TAP128 ? 1 : 0}; }
static void set_desc(HaloDesc& d, const WgCall& c) { d = halo_desc(c); }
static void set_desc(TapDesc& d, const WgCall& c) { d = tap_desc(c); }

struct WgQueued { WgCall c; int n_tiles; float* dw_oihw; int unpack_taps; bool aliased; };     // unpack_taps: as UnpackDesc.taps
// A launch group: the calls that share a kernel pair (immediate, batched) and so one batched launch per `cap` queued calls.
struct WgGroup {
    int cap;                                         // descriptors a table holds
    const char* knob;                                // environment variable (read once) that overrides ...
    int target;                                      // ... the workgroups a batched launch aims at, over all its GEMMs
    size_t lds;                                      // dynamic LDS bytes of either kernel
    const void* kernels[2];
    void (*launch)(const WgCall& c, dim3 grid, hipStream_t st);
    void (*launch_table)(const void* table, int blocks, hipStream_t st);
    bool target_read;
    std::vector<WgQueued> queue;                     // in the order of the calls
};
enum { G_HALO16 = 0, G_HALO8, G_TAP, N_GROUPS };     // the flush runs them in this order
template <int TW>
static WgGroup halo_group() {
    return WgGroup{HALO_MAX, "SBGM_HALO_BATCH_WGS", 768, WgTile<TW>::LDS,
                   {reinterpret_cast<const void*>(conv3x3_wgrad_lds_kernel<TW>), reinterpret_cast<const void*>(conv3x3_wgrad_batched_kernel<TW>)},
                   [](const WgCall& c, dim3 grid, hipStream_t st) {
                       hipLaunchKernelGGL(conv3x3_wgrad_lds_kernel<TW>, grid, dim3(WG_THREADS), WgTile<TW>::LDS, st, halo_desc(c));
                   },
                   [](const void* t, int blocks, hipStream_t st) {
                       hipLaunchKernelGGL(conv3x3_wgrad_batched_kernel<TW>, dim3(blocks), dim3(WG_THREADS), WgTile<TW>::LDS, st,
                                          *static_cast<const HaloTable*>(t));
                   }};
}
static WgGroup g_groups[N_GROUPS] = {
    halo_group<16>(), halo_group<8>(),
    WgGroup{TAP_MAX, "SBGM_TAP_BATCH_WGS", 1024, TAP_LDS,
            {reinterpret_cast<const void*>(conv_tap_wgrad_lds_kernel), reinterpret_cast<const void*>(conv_tap_wgrad_batched_kernel)},
            [](const WgCall& c, dim3 grid, hipStream_t st) {
                hipLaunchKernelGGL(conv_tap_wgrad_lds_kernel, grid, dim3(WG_THREADS), TAP_LDS, st, tap_desc(c));
            },
            [](const void* t, int blocks, hipStream_t st) {
                hipLaunchKernelGGL(conv_tap_wgrad_batched_kernel, dim3(blocks), dim3(WG_THREADS), TAP_LDS, st, *static_cast<const TapTable*>(t));
            }}};
static std::vector<UnpackDesc> g_unpack_queue;

static int wgrad_set_attr() {
    static bool done = false;
    if (!done) {
        for (const WgGroup& g : g_groups)
            for (const void* k : g.kernels) SBGM_HIP(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.lds));
        done = true;
    }
    return 0;
}

static size_t unpack_elems(const UnpackDesc& d) { return (size_t)d.Cout * d.Cin * (d.taps < 0 ? -d.taps * 8 : d.taps); }
static int unpack_or_queue(const UnpackDesc& d, hipStream_t st) {
    if (sbgm_wgrad_deferred & 1) {
        g_unpack_queue.push_back(d);
        return 0;
    }
    hipLaunchKernelGGL(unpack_wgrad_kernel, dim3(stream_blocks(unpack_elems(d))), dim3(256), 0, st, d);
    SBGM_LAUNCH_CHECK();
    return 0;
}

int sbgm_wgrad_pending() {
    size_t n = g_unpack_queue.size();
    for (const WgGroup& g : g_groups) n += g.queue.size();
    return (int)n;
}
// forget the queued work without running it (a backward pass that raised: the tensors it points at may be gone)
void sbgm_wgrad_discard_queue() {
    g_unpack_queue.clear();
    for (WgGroup& g : g_groups) g.queue.clear();
}

// ---- the flush's plan: which launch a queued GEMM rides in and how its pixels are split.  The flush below acts on these rows;
// sbgm_wgrad_flush_rows (the C ABI's sbgm_wgrad_flush_plan) reports the same rows without launching

// A group's rows, in queue order.  A layer's pixel split: its share of the group's work (gx * n_tiles; the 128 x 128 per-tap form does twice
// the MFMAs per tile step) times the group's workgroup target, in whole tiles.
static std::vector<WgradFlushRow> group_rows(WgGroup& g) {
    if (!g.target_read) {
        if (const char* e = getenv(g.knob)) g.target = atoi(e);
        g.target_read = true;
    }
    auto cost = [](const WgQueued& q) { return (double)q.c.h.gx * q.n_tiles * (q.c.family == SBGM_WG_TAP128 ? 2.0 : 1.0); };
    double work = 0.0;
    for (const WgQueued& q : g.queue) work += cost(q);
    std::vector<WgradFlushRow> rows;
    for (size_t i = 0; i < g.queue.size(); ++i) {
        const WgQueued& q = g.queue[i];
        const bool stem = q.c.family == SBGM_WG_STEM;
        WgradFlushRow r{q.c.family, (int)(i / g.cap), q.c.h.gx, 1, 1, q.n_tiles, 0, 0};
        int gy = (int)std::lround(g.target * (cost(q) / work) / r.gx);
        gy = std::max(1, std::min(gy, r.n_tiles));
        r.tiles_per_wg = (r.n_tiles + gy - 1) / gy;
        r.gy = (r.n_tiles + r.tiles_per_wg - 1) / r.tiles_per_wg;
        // no pixel split: plain OIHW stores, no slab, no layout pass (not for the stem's slab layout)
        r.direct = r.gy == 1 && !stem ? 1 : 0;
        r.unpack = stem || (!r.direct && !q.aliased) ? 1 : 0;
        rows.push_back(r);
    }
    return rows;
}
static int unpack_launch_of(size_t i) { return (int)(i / UNPACK_MAX); }

std::vector<WgradFlushRow> sbgm_wgrad_flush_rows(int* layout_passes, int* unpack_launches) {
    std::vector<WgradFlushRow> rows;
    size_t passes = g_unpack_queue.size();
    for (WgGroup& g : g_groups) {
        const std::vector<WgradFlushRow> r = group_rows(g);
        rows.insert(rows.end(), r.begin(), r.end());
    }
    for (auto& r : rows) passes += r.unpack;
    if (layout_passes) *layout_passes = (int)passes;
    if (unpack_launches) *unpack_launches = passes ? unpack_launch_of(passes - 1) + 1 : 0;
    return rows;
}

// A failed batched launch leaves nothing queued, in any group or in the layout stage: the tables point at the caller's tensors, and the
// caller keeps those alive only until the flush returns.
static int flush_failed() {
    sbgm_wgrad_discard_queue();
    sbgm_set_error("wgrad_flush: batched weight-gradient launch failed");
    return 1;
}

// The queued GEMMs of one group: every layer's pixels split by its row (all layers of a launch together make about `target` workgroups),
// one launch per table, the layout passes queued behind those already there.
template <class Table>
static int flush_group(WgGroup& g, hipStream_t st) {
    if (g.queue.empty()) return 0;
    SBGM_CHECK(g.cap == Table::CAP, "wgrad_flush: a group's rows are chunked by %d, its table holds %d", g.cap, Table::CAP);
    if (wgrad_set_attr()) return 1;
    const std::vector<WgradFlushRow> rows = group_rows(g);
    for (size_t i = 0; i < rows.size();) {
        Table t{};
        int nb = 0;
        for (const int launch = rows[i].launch; i < rows.size() && rows[i].launch == launch; ++i) {
            const WgQueued& q = g.queue[i];
            const WgradFlushRow& r = rows[i];
            WgCall c = q.c;
            c.h.tiles_per_wg = r.tiles_per_wg;
            c.h.gy = r.gy;
            c.h.dw_direct = r.direct ? q.dw_oihw : nullptr;
            if (r.unpack) g_unpack_queue.push_back(UnpackDesc{c.h.dwp, q.dw_oihw, c.h.Cout, c.h.Cin, c.h.Cs, q.unpack_taps});
            set_desc(t.d[t.n], c);
            t.start[t.n] = nb;
            nb += c.h.gx * c.h.gy;
            ++t.n;
        }
        t.start[t.n] = nb;
        g.launch_table(&t, nb, st);
        if (hipGetLastError() != hipSuccess) return flush_failed();
    }
    g.queue.clear();
    return 0;
}

int sbgm_launch_wgrad_flush(hipStream_t st) {
    if (flush_group<HaloTable>(g_groups[G_HALO16], st) || flush_group<HaloTable>(g_groups[G_HALO8], st) ||
        flush_group<TapTable>(g_groups[G_TAP], st))
        return 1;
    size_t i = 0;
    const size_t n = g_unpack_queue.size();
    while (i < n) {
        UnpackTable t{};
        int nb = 0;
        for (const int launch = unpack_launch_of(i); i < n && unpack_launch_of(i) == launch; ++i) {
            t.d[t.n] = g_unpack_queue[i];
            t.start[t.n] = nb;
            nb += (int)std::max<size_t>(1, std::min<size_t>((unpack_elems(t.d[t.n]) + 1023) / 1024, 256));          // >= 4 elements per thread
            ++t.n;
        }
        t.start[t.n] = nb;
        hipLaunchKernelGGL(unpack_wgrad_batched_kernel, dim3(nb), dim3(256), 0, st, t);
        if (hipGetLastError() != hipSuccess) return flush_failed();
    }
    g_unpack_queue.clear();
    return 0;
}

// Which kernel body and which pixel split a weight gradient of this geometry gets when launched at once: the launcher below acts on it, and
// sbgm_conv2d_wgrad_plan (capi.hip) reports it.  Under GEMM deferral the family and n_tiles hold; the split is decided at the flush (above).
int sbgm_wgrad_plan(WgradPlan* p, int B, int H, int W, int Cs, int Cin, int Cout, int KH, int KW, int S, int PAD) {
    SBGM_CHECK(Cout % 64 == 0, "wgrad: Cout=%d must be a multiple of 64", Cout);
    SBGM_CHECK((Cs == 4 || Cs == 8 || Cs % 16 == 0) && Cin <= Cs, "wgrad: padded Cin %d unsupported (Cin=%d)", Cs, Cin);
    const int OH = (H + 2 * PAD - KH) / S + 1, OW = (W + 2 * PAD - KW) / S + 1, M = B * OH * OW;
    p->M = M, p->OH = OH, p->OW = OW;
    p->dy_bytes = (size_t)M * Cout * 4, p->x_bytes = (size_t)B * H * W * Cs * 4;
    const bool small = p->dy_bytes < (1ull << 31) && p->x_bytes < (1ull << 31), lds_ok = getenv("SBGM_NO_LDS_WGRAD") == nullptr;
    const bool lds16 = W % 16 == 0 && H % 16 == 0, lds8 = W == 8 && H == 8;
    const bool stem = Cs == 8 && KW == 8;
    // the LDS-staged bodies: a workgroup owns a block of (co, ci) and walks tiles_per_wg pixel tiles; one 8-wave workgroup per CU
    auto tiled = [&](int family, int blocks_x, int n_tiles, bool may_direct) {
        const int wgs_y = std::max(1, std::min(n_tiles, (256 + blocks_x - 1) / blocks_x));
        p->family = family, p->gx = blocks_x, p->n_tiles = n_tiles;
        p->tiles_per_wg = (n_tiles + wgs_y - 1) / wgs_y;
        p->gy = (n_tiles + p->tiles_per_wg - 1) / p->tiles_per_wg;
        p->direct = p->gy == 1 && may_direct ? 1 : 0;         // no pixel split: no atomics, no slab, no unpack pass
    };
    if (KH == 3 && KW == 3 && S == 1 && PAD == 1 && Cs % 32 == 0 && (lds16 || lds8) && small && lds_ok) {
        tiled(lds16 ? SBGM_WG_HALO16 : SBGM_WG_HALO8, (Cout / 32) * (Cs / 32), lds16 ? B * (H / 16) * (W / 16) : (B + 3) / 4, true);
        return 0;
    }
    if ((Cs % 64 == 0 || stem) && small && lds_ok) {
        // one split-K GEMM per tap (1x1 / linear layers, and whatever the halo kernel above does not take)
        const int taps = stem ? KH : KH * KW;
        static const bool big_ok = getenv("SBGM_NO_TAP128") == nullptr;
        const bool big = big_ok && !stem && Cs % 128 == 0 && Cout % 128 == 0;
        tiled(stem ? SBGM_WG_STEM : big ? SBGM_WG_TAP128 : SBGM_WG_TAP64,
              big ? taps * (Cout / 128) * (Cs / 128) : taps * (Cout / 64) * (stem ? 1 : Cs / 64),
              big ? (M + W2_PX - 1) / W2_PX : (M + W1_PX - 1) / W1_PX, !stem);
        return 0;
    }
    const int fci = Cs % 64 == 0 ? 4 : (Cs % 32 == 0 ? 2 : 1);
    const int tiles = KH * KW * (Cout / 64) * ((Cs + 16 * fci - 1) / (16 * fci));
    static const int wtarget = getenv("SBGM_WG_TARGET") ? atoi(getenv("SBGM_WG_TARGET")) : 4096;
    int splits = std::max(1, std::min((M + 63) / 64, (wtarget + tiles - 1) / tiles));   // measured: 1024 target waves is 14 % slower per step
    const int pps = ((M + splits - 1) / splits + 3) / 4 * 4;
    splits = (M + pps - 1) / pps;
    p->family = fci == 4 ? SBGM_WG_GENERAL4 : fci == 2 ? SBGM_WG_GENERAL2 : SBGM_WG_GENERAL1;
    p->gx = (tiles + 3) / 4, p->gy = splits, p->tiles_per_wg = pps, p->n_tiles = M, p->direct = 0;
    return 0;
}

int sbgm_launch_conv_wgrad(const float* dy, const float* x, float* dw_oihw, float* dwp_ws, int B, int H, int W, int Cs, int Cin,
                           int Cout, int KH, int KW, int S, int PAD, hipStream_t st, float* dbias) {
    WgradPlan pl;
    if (sbgm_wgrad_plan(&pl, B, H, W, Cs, Cin, Cout, KH, KW, S, PAD)) return 1;
    const bool halo = pl.family == SBGM_WG_HALO16 || pl.family == SBGM_WG_HALO8, stem = pl.family == SBGM_WG_STEM;
    const bool tap = stem || pl.family == SBGM_WG_TAP64 || pl.family == SBGM_WG_TAP128;
    // ws == dw_oihw: for a 1x1 kernel without channel padding the per-tap kernel's slab IS the OIHW gradient, so the caller may hand in the
    // (zeroed) gradient tensor as workspace and no unpack pass is needed
    const bool aliased = tap && dwp_ws == dw_oihw;
    SBGM_CHECK(!aliased || (KH * KW == 1 && Cs == Cin), "wgrad: ws may alias dw only for 1x1 kernels with c_pad == Cin");
    const int OH = pl.OH, OW = pl.OW, M = pl.M;
    const size_t n = (size_t)KH * KW * Cout * Cs;
    if (!sbgm_scratch_prezeroed && dbias) { if (sbgm_zero_async(dbias, (size_t)Cout * 4, st)) return 1; }
    const dim3 grid(pl.gx, pl.gy);
    const UnpackDesc unpack{dwp_ws, dw_oihw, Cout, Cin, Cs, stem ? -KH : KH * KW};
    if (halo || tap) {
        WgGroup& g = g_groups[pl.family == SBGM_WG_HALO16 ? G_HALO16 : pl.family == SBGM_WG_HALO8 ? G_HALO8 : G_TAP];
        if (wgrad_set_attr()) return 1;
        WgCall c{WgHead{dy, x, dwp_ws, dbias, nullptr, Cs, Cout, Cin, pl.tiles_per_wg, pl.gx, pl.gy, (uint32_t)pl.dy_bytes, (uint32_t)pl.x_bytes},
                 B, TapGeom{M, OH, OW, H, W, S, PAD, KW, KH * KW, stem ? 1 : 0}, pl.family};
        // queued for the sweep's batched launch: the split, and with it whether the slab is needed, is decided at the flush, so the slab is
        // zeroed now; launched at once: a direct store needs no slab.  Either way not when it arrives zeroed.
        const bool queued = (sbgm_wgrad_deferred & 2) != 0;
        float* direct = pl.direct && !queued ? dw_oihw : nullptr;
        if (!direct && !sbgm_scratch_prezeroed) { if (sbgm_zero_async(dwp_ws, n * 4, st)) return 1; }
        if (queued) {
            g.queue.push_back(WgQueued{c, pl.n_tiles, dw_oihw, unpack.taps, aliased});
            return 0;
        }
        c.h.dw_direct = direct;
        g.launch(c, grid, st);
        SBGM_LAUNCH_CHECK();
        // exactly one store outcome: the kernel stored OIHW itself, its slab is the gradient tensor, or a layout pass (the stem: always)
        if (stem || (!direct && !aliased)) return unpack_or_queue(unpack, st);
        return 0;
    }
    if (!sbgm_scratch_prezeroed) { if (sbgm_zero_async(dwp_ws, n * 4, st)) return 1; }
    const int pps = pl.tiles_per_wg;
#define SBGM_WG(F) hipLaunchKernelGGL(conv_wgrad_kernel<F>, grid, dim3(256), 0, st, dy, x, dwp_ws, B, H, W, Cs, OH, OW, Cout, KH, KW, S, PAD, pps, dbias)
    if (pl.family == SBGM_WG_GENERAL4) SBGM_WG(4); else if (pl.family == SBGM_WG_GENERAL2) SBGM_WG(2); else SBGM_WG(1);
#undef SBGM_WG
    SBGM_LAUNCH_CHECK();
    return unpack_or_queue(unpack, st);
}
