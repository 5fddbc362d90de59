// 8x8 / stride 2 / pad 3 convolution (the stem's second convolution) as a 2-D Winograd F(2x2, 4x4) over the space-to-depth input,
// LDS-staged, on the fp32 MFMA pipe (gfx950).
//
// Space-to-depth.  Output row o reads input rows 2o - 3 + k, k = 0..7, and 2o - 3 + k = 2(o + u) - 3 + py with k = 2u + py.  So a
// "cell" c holds the input rows 2c - 3 (phase py = 0) and 2c - 2 (phase 1), zero outside the image, and the same for columns: the
// convolution is exactly a 4x4 stride-1 valid correlation over cells o..o+3 with Cin' = 4 * Cin channels (phase, channel) and the
// sub-filters g[u][v] = w[2u + py][2v + px].  The space-to-depth tensor is never materialised: a stage gathers its cells from the
// NHWC input through the buffer descriptor's bounds check (a pixel outside the image reads 0), so there are no zero taps and no
// padding logic.
//
// Winograd F(2x2, 4x4), alpha = 5, interpolation points {0, 1, -1, -2, inf} (the fourth point was chosen by the fp32-vs-fp64
// simulation of tools/wino_s2d_sim.py):
//     V = B^T d B   (5 x 5 cells d of a 2 x 2 output block)    U = G g G^T   (4 x 4 sub-filter g, packed once per upload, in fp64)
//     M[xi][eta] = sum_c U[xi][eta][co][c] * V[xi][eta][c]      Y = A^T M A   (2 x 2 outputs)
//     B^T = [-2 -1  2  1  0]   G = [-1/2    0    0    0]   A^T = [1  1  1  1  0]
//           [ 0  2  3  1  0]       [ 1/6  1/6  1/6  1/6]         [0  1 -1 -2  1]
//           [ 0 -2  1  1  0]       [ 1/2 -1/2  1/2 -1/2]
//           [ 0 -1  0  1  0]       [-1/6  1/3 -2/3  4/3]
//           [ 0 -2 -1  2  1]       [   0    0    0    1]
// 25 products per 2 x 2 outputs where the direct form needs 64: the executed MFMA work is 25/64 of the algorithmic FLOPs.
//
// Mapping (as conv_w2d.hip).  A workgroup (4 waves) owns a 16 x 16 output tile of ONE image and NCO = 16*FCO output channels; a wave
// owns 2 block rows x 8 block columns (fragment column r16 -> block (r16 >> 3, r16 & 7)) and keeps all 25 (xi, eta) accumulator sets
// of its blocks (25 * FCO f32x4).  One stage = 16 channels of the space-to-depth input = one phase (py, px) of 16 input channels:
// stage s = 4 * (channel block) + 2 * py + px.  Per stage the workgroup loads, once and cooperatively, the weight slab
// [25 (xi, eta)][NCO][16 ch] and the 19 x 19-cell halo patch into LDS; every wave then reads the 5 x 5 cells of its blocks, applies
// B^T . B in registers and issues 25 * FCO * 4 MFMAs.  The global loads of stage s + 1 are in flight during the sweep of stage s
// (register-staged).  Outputs outside the map (a map that is not a tile multiple) are computed but not stored.
//
// LDS layouts (conflict-free for every ds_read_b128 lane group, tools/lds_bank_check_s2w.py):
//   weight slab  [tap][co][4 quads], quad rotated by (co & 15) >> 1          (as conv_lds.hip / conv_w2d.hip)
//   patch        [cell row (stride 78 quads)][cell][4 quads], quad rotated by 2 * (cell >> 2)
#include "common.h"
#include "kernels.h"
#include "conv_common.h"

namespace {

constexpr int TW = 16, TH = 16;         // output tile = 8 x 8 blocks of 2 x 2 outputs
constexpr int PC = TW + 3;              // patch cells per row and per column
constexpr int SY = PC * 4 + 2;          // patch row stride in quads
constexpr int NT = 25;                  // (xi, eta) products of a block

__device__ __forceinline__ int pslot(int px, int quad) { return px * 4 + ((quad + 2 * (px >> 2)) & 3); }

// o = B^T d for one line of 5 cells
__device__ __forceinline__ void bt5(const f32x4 (&d)[5], f32x4 (&o)[5]) {
    const f32x4 s = d[3] - d[1];
    o[0] = 2.f * (d[2] - d[0]) + s;
    o[1] = 3.f * d[2] + 2.f * d[1] + d[3];
    o[2] = (d[2] - d[1]) + s;
    o[3] = s;
    o[4] = 2.f * s - d[2] + d[4];
}

// one workgroup per CU: at FCO = 2 the accumulators alone take 200 registers (AGPRs); a build held to two waves per SIMD spills
template <int FCO>
__global__ __launch_bounds__(256, 1) void conv8x8s2_s2w_kernel(const ConvParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    constexpr int NCO = 16 * FCO;
    constexpr int WQ = NT * NCO * 4;            // weight quads per stage
    constexpr int PQ = PC * PC * 4;             // patch quads loaded per stage
    f32x4* const wl = reinterpret_cast<f32x4*>(smem_raw);      // [tap][co][4 quads]
    f32x4* const pt = wl + WQ;                                  // [cell row][cell][4 quads]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, kq = lane >> 4;
    const int br = r16 >> 3, bc = r16 & 7;

    // block -> (image, tile row, tile col, co tile), co tile fastest (conv_w2d.hip)
    int t = xcd_contiguous_block(blockIdx.x, gridDim.x);
    const int tiles_x = (p.OW + TW - 1) / TW, tiles_y = (p.OH + TH - 1) / TH, n_co = p.Cout / NCO;
    const int co_tile = t % n_co; t /= n_co;
    const int tx = t % tiles_x; t /= tiles_x;
    const int ty = t % tiles_y;
    const int b = t / tiles_y;
    const int co0 = co_tile * NCO, x0 = tx * TW, y0 = ty * TH;

    const __amdgpu_buffer_rsrc_t xr = make_rsrc(p.x, p.x_bytes);
    const __amdgpu_buffer_rsrc_t wr = make_rsrc(p.wp, p.w_bytes);
    const int S = p.nsteps;

    f32x4 acc[NT][FCO];
#pragma unroll
    for (int tp = 0; tp < NT; ++tp)
#pragma unroll
        for (int i = 0; i < FCO; ++i) acc[tp][i] = f32x4{0.f, 0.f, 0.f, 0.f};

    // ---- staging ------------------------------------------------------------------------------------------------------------
    constexpr int WPT = (WQ + 255) / 256;       // weight quads per thread per stage
    constexpr int PPT = (PQ + 255) / 256;       // patch quads per thread per stage
    constexpr int RW = 256 / (NCO * 4);         // taps per 256-quad round
    static_assert(256 % (NCO * 4) == 0 && PPT * 4 <= 32, "staging rounds");
    constexpr uint32_t OOB = 0x80000000u;
    const int tl = tid / (NCO * 4), rem = tid - tl * (NCO * 4);
    const uint32_t wlane = (uint32_t)(tl * p.Cout * 16 + rem * 4) * 4u;
    // patch quad u of this thread: cell (py, px) of the tile, quad q & 3; offset of its phase-0 pixel (may lie outside the image)
    // and, per phase, whether the pixel is inside (bit 4u + phase)
    int pbase[PPT];
    uint32_t pok = 0;
#pragma unroll
    for (int u = 0; u < PPT; ++u) {
        const int q = tid + 256 * u;
        const int pix = q >> 2, py = pix / PC, px = pix - py * PC;
        const int iy = 2 * (y0 + py) - 3, ix = 2 * (x0 + px) - 3;
        pbase[u] = ((b * p.H + iy) * p.W + ix) * p.Cs + (q & 3) * 4;
#pragma unroll
        for (int ph = 0; ph < 4; ++ph) {
            const bool ok = (q < PQ) & ((unsigned)(iy + (ph >> 1)) < (unsigned)p.H) & ((unsigned)(ix + (ph & 1)) < (unsigned)p.W);
            pok |= (uint32_t)ok << (4 * u + ph);
        }
    }
    f32x4 rw[WPT], rp[PPT];
    auto stage_load = [&](int s) {
#pragma unroll
        for (int u = 0; u < WPT; ++u) {                      // [s][tap][Cout][16]: the round's first tap is wavefront-uniform
            const uint32_t su = (uint32_t)(((s * NT + u * RW) * p.Cout + co0) * 16) * 4u;
            rw[u] = (WQ % 256 == 0 || tl + u * RW < NT) ? buf_load4(wr, wlane + su) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
        const int ph = s & 3;
        const int delta = (ph >> 1) * p.W * p.Cs + (ph & 1) * p.Cs + (s >> 2) * 16;
#pragma unroll
        for (int u = 0; u < PPT; ++u)
            rp[u] = buf_load4(xr, (pok >> (4 * u + ph)) & 1 ? (uint32_t)(pbase[u] + delta) * 4u : OOB);
    };
    auto stage_store = [&]() {
#pragma unroll
        for (int u = 0; u < WPT; ++u) {
            const int q = tid + 256 * u;                       // [tap][co][quad]: rotate the quad by the fragment row (co & 15) >> 1
            if (WQ % 256 == 0 || q < WQ) wl[(q & ~3) + (((q & 3) + (((q >> 2) & 15) >> 1)) & 3)] = rw[u];
        }
#pragma unroll
        for (int u = 0; u < PPT; ++u) {
            const int q = tid + 256 * u;
            const int pix = q >> 2, py = pix / PC, px = pix - py * PC;
            if (q < PQ) pt[py * SY + pslot(px, q & 3)] = rp[u];
        }
    };

    // loop-invariant LDS read offsets of this lane (quads)
    const int aoff = r16 * 4 + ((kq + (r16 >> 1)) & 3);
    const int r0 = (wave * 4 + 2 * br) * SY;                  // first patch row of the lane's block
    int coff[5];
#pragma unroll
    for (int c = 0; c < 5; ++c) coff[c] = pslot(2 * bc + c, kq);

    stage_load(0);
    stage_store();
    for (int s = 0; s < S; ++s) {
        if (s + 1 < S) stage_load(s + 1);
        __syncthreads();                                       // stage s is in LDS

        // ---- sweep: V = B^T d B of the lane's block (rows, then columns), then 25 x FCO x 4 MFMAs ------------------------------
        f32x4 V[5][5];
#pragma unroll
        for (int r = 0; r < 5; ++r) {
            f32x4 d[5];
#pragma unroll
            for (int c = 0; c < 5; ++c) d[c] = pt[r0 + r * SY + coff[c]];
            bt5(d, V[r]);                                      // V[r][eta] = (d B)[r][eta]
        }
#pragma unroll
        for (int eta = 0; eta < 5; ++eta) {
            const f32x4 col[5] = {V[0][eta], V[1][eta], V[2][eta], V[3][eta], V[4][eta]};
            f32x4 o[5];
            bt5(col, o);
#pragma unroll
            for (int xi = 0; xi < 5; ++xi) V[xi][eta] = o[xi];
        }
#pragma unroll
        for (int xi = 0; xi < 5; ++xi) {
            f32x4 a[5][FCO];
#pragma unroll
            for (int eta = 0; eta < 5; ++eta)
#pragma unroll
                for (int i = 0; i < FCO; ++i) a[eta][i] = wl[((xi * 5 + eta) * NCO + 16 * i) * 4 + aoff];
            // k outermost: consecutive MFMAs go to 5 * FCO different accumulators
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int eta = 0; eta < 5; ++eta)
#pragma unroll
                    for (int i = 0; i < FCO; ++i)
                        acc[xi * 5 + eta][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[eta][i][k], V[xi][eta][k], acc[xi * 5 + eta][i], 0, 0, 0);
        }
        __syncthreads();                                       // every wave is done reading stage s
        if (s + 1 < S) stage_store();
    }

    // ---- epilogue: Y = A^T M A, then the shared convolution epilogue on the block's in-map pixels --------------------------------
    const int oy = y0 + wave * 4 + 2 * br, ox = x0 + 2 * bc;
#pragma unroll
    for (int i = 0; i < FCO; ++i) {
        f32x4 P0[5], P1[5];                                    // P_j[xi] = sum_eta M[xi][eta] A^T[j][eta]
#pragma unroll
        for (int xi = 0; xi < 5; ++xi) {
            const f32x4 m0 = acc[xi * 5][i], m1 = acc[xi * 5 + 1][i], m2 = acc[xi * 5 + 2][i], m3 = acc[xi * 5 + 3][i], m4 = acc[xi * 5 + 4][i];
            P0[xi] = (m0 + m1) + (m2 + m3);
            P1[xi] = (m1 - m2) + (m4 - 2.f * m3);
        }
        f32x4 y[4];                                            // [2 * row + col]
        y[0] = (P0[0] + P0[1]) + (P0[2] + P0[3]);
        y[1] = (P1[0] + P1[1]) + (P1[2] + P1[3]);
        y[2] = (P0[1] - P0[2]) + (P0[4] - 2.f * P0[3]);
        y[3] = (P1[1] - P1[2]) + (P1[4] - 2.f * P1[3]);
        const int co = co0 + 16 * i + 4 * kq;
#pragma unroll
        for (int px = 0; px < 4; ++px) {
            const int yy = oy + (px >> 1), xx = ox + (px & 1);
            if (yy < p.OH && xx < p.OW) {
                const size_t m = ((size_t)b * p.OH + yy) * p.OW + xx;
                *reinterpret_cast<f32x4*>(p.out + m * p.Cout + co) = conv_epilogue(y[px], p, co, m, b);
            }
        }
    }
}

// U = G g G^T of the 4 x 4 sub-filters, in fp64 (G of the header)
__constant__ double kG[5][4] = {{-0.5, 0.0, 0.0, 0.0},
                                {1.0 / 6.0, 1.0 / 6.0, 1.0 / 6.0, 1.0 / 6.0},
                                {0.5, -0.5, 0.5, -0.5},
                                {-1.0 / 6.0, 1.0 / 3.0, -2.0 / 3.0, 4.0 / 3.0},
                                {0.0, 0.0, 0.0, 1.0}};

// OIHW [Cout][Cin][8][8] -> U[s = 4 * cb + 2 * py + px][xi * 5 + eta][Cout][16], sub-filter g[u][v] = w[2u + py][2v + px] of the
// channel 16 * cb + (i & 15); channels >= Cin are zero
__global__ void pack_s2w_weight_kernel(const float* __restrict__ w, float* __restrict__ up, int Cout, int Cin, int cs) {
    const size_t total = (size_t)(cs / 16) * 4 * NT * Cout * 16;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c16 = (int)(i & 15);
        size_t r = i >> 4;
        const int co = (int)(r % Cout); r /= Cout;
        const int tap = (int)(r % NT);
        const int s = (int)(r / NT);
        const int xi = tap / 5, eta = tap - 5 * (tap / 5);
        const int py = (s >> 1) & 1, px = s & 1;
        const int c = (s >> 2) * 16 + c16;
        double v = 0.0;
        if (c < Cin) {
            const float* g = w + ((size_t)co * Cin + c) * 64;
            for (int u = 0; u < 4; ++u) {
                double rowv = 0.0;
                for (int vv = 0; vv < 4; ++vv) rowv += kG[eta][vv] * (double)g[(2 * u + py) * 8 + 2 * vv + px];
                v += kG[xi][u] * rowv;
            }
        }
        up[i] = (float)v;
    }
}

}  // namespace

size_t sbgm_s2w_packed_floats(int Cout, int cs) { return (size_t)(cs / 16) * 4 * NT * Cout * 16; }

int sbgm_launch_pack_s2w_weight(const float* w_oihw, float* up, int Cout, int Cin, int cs, hipStream_t st) {
    SBGM_CHECK(cs % 16 == 0 && Cin <= cs && Cout % 16 == 0, "pack_s2w: padded Cin %d must be a multiple of 16 (Cout %d of 16)", cs, Cout);
    const size_t total = sbgm_s2w_packed_floats(Cout, cs);
    hipLaunchKernelGGL(pack_s2w_weight_kernel, dim3((int)std::min<size_t>((total + 255) / 256, 4096)), dim3(256), 0, st, w_oihw, up,
                       Cout, Cin, cs);
    SBGM_LAUNCH_CHECK();
    return 0;
}

size_t sbgm_conv_s2w_bytes(const ConvTile& cfg) { return ((size_t)NT * 16 * cfg.fco * 4 + (size_t)PC * SY) * 16; }

// cfg.wino == 3; cfg.fco in {1, 2} (16 / 32 output channels per workgroup); p.wp = the F(2x2,4x4) space-to-depth weight image
// (sbgm_launch_pack_s2w_weight).
int sbgm_launch_conv_s2w(ConvParams p, const ConvTile& cfg, hipStream_t st) {
    SBGM_CHECK(p.wp != nullptr, "conv_s2w: no F(2x2,4x4) weight image for this convolution");
    SBGM_CHECK(p.Cs % 16 == 0 && p.H >= 2 && p.W >= 2, "conv_s2w: needs Cin padded to 16 and a map of at least 2 x 2 (Cs=%d H=%d W=%d)", p.Cs, p.H, p.W);
    SBGM_CHECK(p.Cout % (16 * cfg.fco) == 0, "conv_s2w: Cout=%d not a multiple of the %d-channel tile", p.Cout, 16 * cfg.fco);
    SBGM_CHECK(p.act == SBGM_ACT_NONE || p.act == SBGM_ACT_RELU || p.act == SBGM_ACT_GELU, "conv_s2w: act=%d does not fuse", p.act);
    SBGM_CHECK((size_t)p.B * p.H * p.W * p.Cs * 4 < (1ull << 31), "conv_s2w: input tensor exceeds 2 GiB buffer window");
    SBGM_CHECK(p.proj_w == nullptr && p.in_mode == 0 && p.c_real == 0 && p.in_dil <= 1,
               "conv_s2w: no tap projection, input mode, 2-channel stem or input dilation");
    const int OH = (p.H + 6 - 8) / 2 + 1, OW = (p.W + 6 - 8) / 2 + 1;
    SBGM_CHECK((p.out_h == 0 || p.out_h == OH) && (p.out_w == 0 || p.out_w == OW), "conv_s2w: explicit output size %dx%d", p.out_h, p.out_w);
    p.gn_stats = nullptr;
    p.OH = OH; p.OW = OW;
    p.M = p.B * OH * OW;
    p.cb_per_tap = p.Cs / 16;
    p.nsteps = 4 * p.cb_per_tap;
    p.x_bytes = (uint32_t)((size_t)p.B * p.H * p.W * p.Cs * 4);
    p.w_bytes = (uint32_t)(sbgm_s2w_packed_floats(p.Cout, p.Cs) * 4);
    const int tiles = ((OW + TW - 1) / TW) * ((OH + TH - 1) / TH) * p.B * (p.Cout / (16 * cfg.fco));
    const size_t lds = sbgm_conv_s2w_bytes(cfg);
    SBGM_CHECK(lds <= 160 * 1024, "conv_s2w: tile needs %zu bytes of LDS", lds);
    int rc = 1;
#define SBGM_S2W(FC)                                                                                          \
    if (cfg.fco == FC) {                                                                                      \
        if (lds > 64 * 1024)                                                                                  \
            SBGM_HIP(hipFuncSetAttribute((const void*)conv8x8s2_s2w_kernel<FC>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
        hipLaunchKernelGGL((conv8x8s2_s2w_kernel<FC>), dim3(tiles), dim3(256), lds, st, p);                 \
        rc = 0;                                                                                              \
    }
    SBGM_S2W(1) SBGM_S2W(2)
#undef SBGM_S2W
    SBGM_CHECK(rc == 0, "conv_s2w: no kernel for tile fco=%d", cfg.fco);
    SBGM_LAUNCH_CHECK();
    return 0;
}
