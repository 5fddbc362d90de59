// The decoder's final block as ONE 3x3 convolution to the 9 taps of its last layer.
//
// The reference builds the final DecoderBlock with identity norms, no skip, no time term and an identity activation
// (score_unet.py:713-730, :757), so the block is conv(conv_up(upsample(x))) with nothing non-linear in between:
//   d[tap][m] = sum_co w2[0][co][tap] * (sum_{ci,v,b} w1[co][ci][v][b] * up(x)[ci][m + (v,b)] + b1[co])
//             = sum_{ci,v,b} Wc[tap][ci][v][b] * up(x)[ci][m + (v,b)] + bc[tap]
//   out[o]    = b2 + sum_tap d[tap][o + tap - 1]          (d outside the image counts as 0: conv's zero padding of conv_up's output)
// Wc is an ordinary 3x3 weight from C to 9 channels (stored as 16, rows 9..15 zero), so every 16-channel kernel of the convolution
// families runs it; the gather below finishes the block from the pixel-major rows [M][16] those kernels write.
#include "common.h"
#include "kernels.h"

namespace {

// Wc[tap][ci][v][b] = sum_co w2[0][co][tap] * w1[co][ci][v][b],  bc[tap] = sum_co w2[0][co][tap] * b1[co]: fp64 sums, rounded once
__global__ void final_compose_kernel(const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w2,
                                     float* __restrict__ wc, float* __restrict__ bc, int C) {
    const int per = C * 9, total = 16 * per + 16;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const bool is_w = i < 16 * per;
        const int tap = is_w ? i / per : i - 16 * per;
        const int r = is_w ? i - tap * per : 0;              // (ci, v, b) of conv_up's weight
        double acc = 0.0;
        if (tap < 9)
            for (int co = 0; co < C; ++co) {
                const double a = (double)w2[co * 9 + tap];
                acc += a * (is_w ? (double)w1[(size_t)co * per + r] : (double)b1[co]);
            }
        if (is_w) wc[i] = (float)acc;
        else bc[tap] = (float)acc;
    }
}

// out[b, y, x] = (bias + sum_taps d[b, y + kh - 1, x + kw - 1][kh * 3 + kw]) / sigma(t_b) over pixel-major rows d [B][H][W][16].
// A workgroup stages the 9 used floats of its (16 + 2) x (32 + 2) pixel rows in LDS as tap planes (three 16-byte loads per row,
// neighbouring lanes on neighbouring quads), zeros where the row lies outside the image, and gathers from there: every row is
// fetched once per tile instead of once per tap.  Tile shape, measured at batch 32 x 128^2 (32 MiB of rows): 16 x 32 pixels 9.5 us
// and 38.9 MiB read; 8 x 64 pixels 8.8 us and 40.8 MiB; 16 x 64 pixels 12.9 us (half the workgroups) and 36.7 MiB.  The first keeps
// convolution + gather below the 72 MiB the projection path's two partial-plane sets move.
constexpr int GT_X = 32, GT_Y = 16, GT_PW = GT_X + 2, GT_PX = GT_PW * (GT_Y + 2), GT_LD = GT_PX + 1;
__global__ __launch_bounds__(256) void tap_gather_rows_kernel(const float* __restrict__ d, const float* __restrict__ bias,
                                                              const float* __restrict__ t, float sigma, float* __restrict__ out,
                                                              int B, int H, int W, int tiles_x, int tiles_y) {
    __shared__ float s[9 * GT_LD];
    const int tid = threadIdx.x;
    int blk = blockIdx.x;
    const int tx = blk % tiles_x; blk /= tiles_x;
    const int ty = blk % tiles_y;
    const int b = blk / tiles_y;
    const int x0 = tx * GT_X, y0 = ty * GT_Y;
    for (int i = tid; i < GT_PX * 3; i += 256) {
        const int px = i / 3, q = i - px * 3;
        const int ly = px / GT_PW, lx = px - ly * GT_PW;
        const int gy = y0 + ly - 1, gx = x0 + lx - 1;
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        if ((unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W)
            v = *reinterpret_cast<const f32x4*>(d + (((size_t)b * H + gy) * W + gx) * 16 + 4 * q);     // q = 2: floats 8..11 of the row
        s[(4 * q) * GT_LD + px] = v[0];
        if (q < 2) {
            s[(4 * q + 1) * GT_LD + px] = v[1];
            s[(4 * q + 2) * GT_LD + px] = v[2];
            s[(4 * q + 3) * GT_LD + px] = v[3];
        }
    }
    __syncthreads();
    float sd = 1.f;
    if (t != nullptr) {
        const float ls = logf(sigma);
        const float var = (expf((2.f * t[b]) * ls) - 1.f) / (2.f * ls);
        sd = fmaxf(sqrtf(var), 1e-5f);
    }
    for (int o = tid; o < GT_X * GT_Y; o += 256) {
        const int oy = o / GT_X, ox = o - oy * GT_X;
        const int gy = y0 + oy, gx = x0 + ox;
        if (gy >= H || gx >= W) continue;
        float v = 0.f;
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) v += s[(kh * 3 + kw) * GT_LD + (oy + kh) * GT_PW + ox + kw];
        v += bias[0];
        if (t != nullptr) v /= sd;
        out[((size_t)b * H + gy) * W + gx] = v;
    }
}

// ---- the same block mixed at LOW resolution ----------------------------------------------------------------------------------------
// `up` (bilinear x2) acts per channel, so the channel mix commutes with it, and the two 3x3 stencils compose into one 5x5 stencil:
//   Z[s]   = sum_ci Wz[s][ci] v[ci]                          low-res, s = (ty + vy, tx + vx) in 5x5: a 1x1 product with K = C
//   out[o] = beta + sum_{s, o + s - 2 inside} up(Z[s])[o + s - 2]
// `conv` zero-pads conv_up's OUTPUT: a tap whose intermediate pixel o + tap - 1 lies outside the image contributes nothing even where
// the input pixel is inside.  Per axis only o = 0 (tap 0 drops out) and o = O - 1 (tap 2 drops out) differ from the interior, where
// "input pixel inside" is the whole condition: 3 classes per axis, 9 sets (Wz, beta), class c = 3 cy + cx.  An output of a border class
// reads up(Z_c) on the two outermost low-res rows / columns only, so the 8 non-interior sets live on 2-pixel strips (lr_edge_index).
__host__ __device__ inline int lr_tap0(int cls) { return cls == 0 ? 1 : 0; }      // valid taps of `conv` on an axis: first {1,2},
__host__ __device__ inline int lr_tap1(int cls) { return cls == 2 ? 1 : 2; }      // interior {0,1,2}, last {0,1}
__host__ __device__ inline int lr_edge_pixels(int h, int w) { return 16 + 4 * w + 4 * h; }
__device__ __forceinline__ bool lr_in_strip(int cls, int l, int n) { return cls == 1 || (cls == 0 ? l < 2 : l >= n - 2); }
// pixel (ly, lx) of class c's strip within one image's edge block: corners 2x2, first / last rows 2 x w, first / last columns h x 2
__device__ __forceinline__ int lr_edge_base(int c, int h, int w) {
    return (c >= 1 ? 4 : 0) + (c >= 2 ? 2 * w : 0) + (c >= 3 ? 4 : 0) + (c >= 5 ? 2 * h : 0) + (c >= 6 ? 2 * h : 0) + (c >= 7 ? 4 : 0) +
           (c >= 8 ? 2 * w : 0);
}
__device__ __forceinline__ int lr_edge_index(int c, int ly, int lx, int h, int w) {
    const int cy = c / 3, cx = c - cy * 3;
    const int ry = cy == 2 ? ly - (h - 2) : ly, rx = cx == 2 ? lx - (w - 2) : lx;
    return lr_edge_base(c, h, w) + ry * (cx == 1 ? w : 2) + rx;
}

// Wz and beta of the 9 classes from the uploaded tensors: fp64 sums, rounded once.  wzp[c][ks][row][16] is the A operand of
// v_mfma_f32_16x16x4_f32 in the implicit-GEMM layout (32 rows: s = 0..24, then zeros); wz [9][25][C] (may be null) the plain copy.
__global__ void final_lowres_pack_kernel(const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w2,
                                         const float* __restrict__ b2, float* __restrict__ wz, float* __restrict__ beta,
                                         float* __restrict__ wzp, int C) {
    const int per = (C / 16) * 32 * 16, total = 9 * per + 9;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const bool is_w = i < 9 * per;
        const int c = is_w ? i / per : i - 9 * per;
        const int cy = c / 3, cx = c - cy * 3;
        double acc = 0.0;
        if (!is_w) {
            acc = (double)b2[0];
            for (int ty = lr_tap0(cy); ty <= lr_tap1(cy); ++ty)
                for (int tx = lr_tap0(cx); tx <= lr_tap1(cx); ++tx) {
                    double bc = 0.0;
                    for (int co = 0; co < C; ++co) bc += (double)w2[co * 9 + ty * 3 + tx] * (double)b1[co];
                    acc += bc;
                }
            beta[c] = (float)acc;
            continue;
        }
        const int r = i - c * per;
        const int ks = r / 512, row = (r >> 4) & 31, ci = ks * 16 + (r & 15);
        if (row < 25) {
            const int sy = row / 5, sx = row - sy * 5;
            for (int ty = lr_tap0(cy); ty <= lr_tap1(cy); ++ty) {
                const int vy = sy - ty;
                if (vy < 0 || vy > 2) continue;
                for (int tx = lr_tap0(cx); tx <= lr_tap1(cx); ++tx) {
                    const int vx = sx - tx;
                    if (vx < 0 || vx > 2) continue;
                    for (int co = 0; co < C; ++co)
                        acc += (double)w2[co * 9 + ty * 3 + tx] * (double)w1[(((size_t)co * C + ci) * 3 + vy) * 3 + vx];
                }
            }
            if (wz != nullptr) wz[((size_t)c * 25 + row) * C + ci] = (float)acc;
        }
        wzp[i] = (float)acc;
    }
}

// Z = Wz . act(x * scale + shift + skip) over the low-res pixels.  No LDS: a wave owns fragments of 16 pixels, a lane (pixel r16,
// k quarter kq) loads its B operand, the 4 channels 16 ks + 4 kq .. + 3 of its pixel, straight from the NHWC rows with 16-byte loads
// (all of a wave's loads are requested before the first product), and holds one class's A fragments for its lifetime.  The
// accumulator lane owns 4 consecutive positions s of its pixel: one 16-byte store per 16-row fragment into the row Z[pixel][28].
// The first n_main workgroups run the interior class over MIX_FPW fragments of consecutive pixels per wave; the workgroups after
// them form the 8 border classes on their strips, one strip fragment per wave (per image 4 corner fragments and ceil(2w / 16) /
// ceil(2h / 16) fragments per row / column strip: 13 % more pixels at 64 x 64), into the image's edge block.
constexpr int MIX_FPW = 2;
template <int NKS>
__device__ __forceinline__ void mix_operand(f32x4 (&v)[NKS], const f32x4 (&sk)[NKS], bool ok, int b, int kq, const float* aff,
                                            bool has_skip, int act) {
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
        f32x4 u = v[ks];
        if (aff != nullptr) {                                // [B][C/4][2][4]: scale quad, shift quad
            const f32x4* ap = reinterpret_cast<const f32x4*>(aff) + ((size_t)b * (NKS * 4) + ks * 4 + kq) * 2;
            u = u * ap[0] + ap[1];
        }
        if (has_skip) u += sk[ks];
        if (act == SBGM_ACT_SILU) {                          // hardware exp2 / rcp, as the in_mode-2 staging of conv_lds.hip / conv_w2d.hip
#pragma unroll
            for (int e = 0; e < 4; ++e) u[e] = u[e] * __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-1.4426950408889634f * u[e]));
        } else if (act != SBGM_ACT_NONE) {
#pragma unroll
            for (int e = 0; e < 4; ++e) u[e] = sbgm_act(u[e], act);
        }
        v[ks] = ok ? u : f32x4{0.f, 0.f, 0.f, 0.f};
    }
}
template <int NKS>
__device__ __forceinline__ void mix_product(const f32x4 (&a)[NKS][2], const f32x4 (&v)[NKS], f32x4* __restrict__ row, bool ok, int kq) {
    f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int i = 0; i < 2; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ks][i][k], v[ks][k], acc[i], 0, 0, 0);
    if (ok) {
        row[kq] = acc[0];
        if (kq < 3) row[4 + kq] = acc[1];
    }
}
// SKIPX (NKS = 4, the sampler route): the skip is not loaded but formed in place as the encoder's conv1 (8x8, stride 2, pad 3) at the
// pixel.  conv1 is linear: its share over the condition channels is the run's constant `skip` (Sc, null without such channels), its
// time bias the row tb0 [B][64], and its share over x, K = 64 taps, is 16 products per 16-channel fragment whose accumulator IS
// sk[ks]: the C/D layout of v_mfma_f32_16x16x4_f32 (column = lane & 15 = the pixel, rows 4 (lane >> 4) + reg = the channel quad) is
// the layout mix_operand reads.  k step s and lane quarter kq give tap 4 s + kq = 8 v + u.  The B values, x[b][2 ly + v - 3][2 lx + u - 3]
// of the planar input, are 4-byte global loads under a row and a column mask (a linear bounds check alone would wrap columns into the
// neighbouring row).  The A values are read per fragment from the workgroup's LDS copy of w1x [k step][64 co][4] (wl = the lane's own
// float of a 64-float row: conflict-free 4-byte reads at constant offsets).  Measured at batch 32 x 128^2 (the mix without the skip
// 27.4 us): every wave fetching its 64 A values from global memory 66 us (16 KB per wave, as many bytes again through the L2 as the
// kernel streams from HBM); the LDS copy with the values held in registers across the wave's fragments 51 us (188 VGPRs, 2 waves per
// SIMD); read per fragment 44 us (124 VGPRs, 3 waves per SIMD as without the skip).  Fewer, longer-lived workgroups striding over
// the fragments measured slower (70 us and more): the strip fragments then form a tail.
__device__ __forceinline__ void skip_from_x(f32x4 (&sk)[4], const float* __restrict__ wl, const float* __restrict__ xin,
                                            const float* __restrict__ tb0, const f32x4* __restrict__ sc4, bool ok, int pix, int b, int ly,
                                            int lx, int H, int W, int kq) {
    int off = 0;                                       // an offset the compiler cannot see through: the A values are read here, per
    asm volatile("" : "+v"(off));                      // fragment, instead of living in 64 registers across the wave's fragments
    wl += off;
    const float* const xb = xin + (size_t)b * H * W;
    const int ix0 = 2 * lx + kq - 3, ix1 = ix0 + 4;
    const bool cm0 = ok && (unsigned)ix0 < (unsigned)W, cm1 = ok && (unsigned)ix1 < (unsigned)W;
    float tap[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        const int iy = 2 * ly + (s >> 1) - 3;
        const bool in = (unsigned)iy < (unsigned)H && ((s & 1) ? cm1 : cm0);
        tap[s] = in ? xb[iy * W + ((s & 1) ? ix1 : ix0)] : 0.f;
    }
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        sk[ks] = reinterpret_cast<const f32x4*>(tb0)[b * 16 + ks * 4 + kq];
        if (sc4 != nullptr) sk[ks] += sc4[(size_t)pix * 16 + ks * 4 + kq];
    }
#pragma unroll
    for (int s = 0; s < 16; ++s)
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) sk[ks] = __builtin_amdgcn_mfma_f32_16x16x4f32(wl[(s * 64 + ks * 16) * 4], tap[s], sk[ks], 0, 0, 0);
}
template <int NKS, bool SKIPX>
__global__ __launch_bounds__(256) void final_mix_kernel(const float* __restrict__ x, const float* __restrict__ aff,
                                                        const float* __restrict__ skip, int act, const float* __restrict__ wzp,
                                                        float* __restrict__ z, float* __restrict__ edge, int h, int w, int M,
                                                        int n_main, int n_edge_frags, const float* __restrict__ xin,
                                                        const float* __restrict__ tb0, const float* __restrict__ w1x) {
    static_assert(!SKIPX || NKS == 4, "conv1 has 64 output channels");
    constexpr int QPP = NKS * 4;                       // quads per pixel
    constexpr int CLS_QUADS = NKS * 32 * 4;            // quads per class image
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, kq = lane >> 4;
    const f32x4* const wq = reinterpret_cast<const f32x4*>(wzp);
    const f32x4* const x4 = reinterpret_cast<const f32x4*>(x);
    const f32x4* const s4 = reinterpret_cast<const f32x4*>(skip);
    const int hw = h * w;
    f32x4 a[NKS][2];
    __shared__ float w1s[SKIPX ? SKIP_MIX_PACKED_FLOATS : 1];
    const float* const wl = w1s + (SKIPX ? r16 * 4 + kq : 0);
    if constexpr (SKIPX) {                             // before any wave leaves: every thread takes part in the copy and the barrier
        for (int i = threadIdx.x; i < SKIP_MIX_PACKED_FLOATS / 4; i += 256)
            reinterpret_cast<f32x4*>(w1s)[i] = reinterpret_cast<const f32x4*>(w1x)[i];
        __syncthreads();
    }
    if ((int)blockIdx.x >= n_main) {                   // ---- one strip fragment of a border class ----
        const int ef = ((int)blockIdx.x - n_main) * 4 + wave;
        if (ef >= n_edge_frags) return;
        const int fw = (2 * w + 15) >> 4, fh = (2 * h + 15) >> 4, per_image = 4 + 2 * fw + 2 * fh;
        const int b = ef / per_image;
        int r = ef - b * per_image, c = 0;             // class by class: corner, row strip, corner, column strips, corner, row strip, corner
        const int frags[9] = {1, fw, 1, fh, 0, fh, 1, fw, 1};
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (c == k && r >= frags[k]) { r -= frags[k]; c = k + 1; }
        const int cy = c / 3, cx = c - cy * 3;
        const int width = cx == 1 ? w : 2, size = width * (cy == 1 ? h : 2);
        const int j = r * 16 + r16;
        const bool ok = j < size;
        const int ry = j / width, rx = j - ry * width;
        const int ly = (cy == 2 ? h - 2 : 0) + ry, lx = (cx == 2 ? w - 2 : 0) + rx;
        const int pix = ok ? b * hw + ly * w + lx : 0;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
            for (int i = 0; i < 2; ++i) a[ks][i] = wq[c * CLS_QUADS + (ks * 32 + i * 16 + r16) * 4 + kq];
        f32x4 v[NKS], sk[NKS];
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            v[ks] = x4[(size_t)pix * QPP + ks * 4 + kq];
            if (!SKIPX) sk[ks] = skip != nullptr ? s4[(size_t)pix * QPP + ks * 4 + kq] : f32x4{0.f, 0.f, 0.f, 0.f};
        }
        if constexpr (SKIPX) skip_from_x(sk, wl, xin, tb0, skip != nullptr ? s4 : nullptr, ok, pix, b, ly, lx, 2 * h, 2 * w, kq);
        mix_operand<NKS>(v, sk, ok, b, kq, aff, SKIPX || skip != nullptr, act);
        const size_t ep = (size_t)b * lr_edge_pixels(h, w) + (ok ? lr_edge_index(c, ly, lx, h, w) : 0);
        mix_product<NKS>(a, v, reinterpret_cast<f32x4*>(edge) + ep * 7, ok, kq);
        return;
    }
    const int frag0 = (blockIdx.x * 4 + wave) * MIX_FPW;
    if (frag0 * 16 >= M) return;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
        for (int i = 0; i < 2; ++i) a[ks][i] = wq[4 * CLS_QUADS + (ks * 32 + i * 16 + r16) * 4 + kq];
    f32x4 v[MIX_FPW][NKS], sk[MIX_FPW][NKS];
#pragma unroll
    for (int f = 0; f < MIX_FPW; ++f) {
        const int pix = (frag0 + f) * 16 + r16;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            v[f][ks] = sk[f][ks] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (pix < M) {
                v[f][ks] = x4[(size_t)pix * QPP + ks * 4 + kq];
                if (!SKIPX && skip != nullptr) sk[f][ks] = s4[(size_t)pix * QPP + ks * 4 + kq];
            }
        }
        if constexpr (SKIPX) {
            const bool ok = pix < M;
            const int p = ok ? pix : 0, b = p / hw, r = p - b * hw, ly = r / w;
            skip_from_x(sk[f], wl, xin, tb0, skip != nullptr ? s4 : nullptr, ok, p, b, ly, r - ly * w, 2 * h, 2 * w, kq);
        }
    }
#pragma unroll
    for (int f = 0; f < MIX_FPW; ++f) {
        const int pix = (frag0 + f) * 16 + r16;
        const bool ok = pix < M;
        mix_operand<NKS>(v[f], sk[f], ok, ok ? pix / hw : 0, kq, aff, SKIPX || skip != nullptr, act);
        mix_product<NKS>(a, v[f], reinterpret_cast<f32x4*>(z) + (size_t)(ok ? pix : 0) * 7, ok, kq);
    }
}

// out[b, y, x] = (beta[c] + sum_{s, (y, x) + s - 2 inside} up(Z_c[s])[(y, x) + s - 2]) / sigma(t_b), c = the pixel's border class.
// A workgroup owns 16 x 32 outputs and stages the (8 + 4) x (16 + 4) low-res pixels they reach as 25 planes in LDS (seven 16-byte
// loads per pixel row of Z).  up = bilinear x2, align_corners = False: an even position 2k reads 0.25 Z[k-1] + 0.75 Z[k], an odd one
// 0.75 Z[k] + 0.25 Z[k+1], the neighbour clamped at the map edge (upsample2x_kernel).  Border-class outputs (first / last row and
// column of the image) read their class's strip from the edge block instead, in workgroups of their own after the n_main tiles (a
// tile that took them in line ran the 100 global reads on every wave that holds one ring pixel).  Fixed summation order: deterministic.
constexpr int LG_X = 32, LG_Y = 16, LG_PW = LG_X / 2 + 4, LG_PH = LG_Y / 2 + 4, LG_PX = LG_PW * LG_PH, LG_LD = LG_PX + 1;
struct LrAxis { int a[5], b[5]; float wa[5]; bool in[5]; };    // the two low-res neighbours (weights wa, 1 - wa) of o + s - 2, s = 0..4
__device__ __forceinline__ LrAxis lr_axis(int o, int n_lo) {
    LrAxis r;
#pragma unroll
    for (int s = 0; s < 5; ++s) {
        const int p = o + s - 2, k = p >> 1;
        r.in[s] = (unsigned)p < (unsigned)(2 * n_lo);
        if (p & 1) { r.a[s] = k; r.b[s] = min(k + 1, n_lo - 1); r.wa[s] = 0.75f; }
        else { r.a[s] = max(k - 1, 0); r.b[s] = k; r.wa[s] = 0.25f; }
    }
    return r;
}
template <typename Z>
__device__ __forceinline__ float lr_sum(const LrAxis& ry, const LrAxis& rx, Z zat) {      // zat(s, row, col) = Z[s] at a low-res pixel
    float v = 0.f;
#pragma unroll
    for (int sy = 0; sy < 5; ++sy)
#pragma unroll
        for (int sx = 0; sx < 5; ++sx) {
            if (!(ry.in[sy] && rx.in[sx])) continue;
            const int s = sy * 5 + sx;
            const float wx = rx.wa[sx], wy = ry.wa[sy];
            const float top = wx * zat(s, ry.a[sy], rx.a[sx]) + (1.f - wx) * zat(s, ry.a[sy], rx.b[sx]);
            const float bot = wx * zat(s, ry.b[sy], rx.a[sx]) + (1.f - wx) * zat(s, ry.b[sy], rx.b[sx]);
            v += wy * top + (1.f - wy) * bot;
        }
    return v;
}
__device__ __forceinline__ float sigma_of_t(float tb, float sigma) {      // the marginal std, as tap_gather_rows_kernel computes it
    const float ls = logf(sigma);
    const float var = (expf((2.f * tb) * ls) - 1.f) / (2.f * ls);
    return fmaxf(sqrtf(var), 1e-5f);
}
__global__ __launch_bounds__(256) void final_gather_kernel(const float* __restrict__ z, const float* __restrict__ edge,
                                                           const float* __restrict__ beta, const float* __restrict__ t, float sigma,
                                                           float* __restrict__ out, int h, int w, int tiles_x, int tiles_y,
                                                           int n_main, int border_blocks) {
    __shared__ float s[25 * LG_LD];
    const int tid = threadIdx.x;
    const int H = 2 * h, W = 2 * w;
    int blk = blockIdx.x;
    if (blk >= n_main) {                                     // ---- the image's border ring, one output per thread, from the edge block ----
        const int b = (blk - n_main) / border_blocks;
        const int idx = ((blk - n_main) - b * border_blocks) * 256 + tid;
        if (idx >= 2 * W + 2 * (H - 2)) return;
        const int k = idx - 2 * W;
        const int gy = idx < W ? 0 : idx < 2 * W ? H - 1 : 1 + (k >> 1);
        const int gx = idx < W ? idx : idx < 2 * W ? idx - W : (k & 1) ? W - 1 : 0;
        const int c = (gy == 0 ? 0 : gy == H - 1 ? 2 : 1) * 3 + (gx == 0 ? 0 : gx == W - 1 ? 2 : 1);
        // the thread's class is fixed: strip origin and row pitch once, a multiply-add and a subtraction per read
        const int cy = c / 3, cx = c - cy * 3, pitch = cx == 1 ? w : 2;
        const int org = (cy == 2 ? h - 2 : 0) * pitch + (cx == 2 ? w - 2 : 0);
        const float* const eb = edge + ((size_t)b * lr_edge_pixels(h, w) + lr_edge_base(c, h, w)) * FINAL_LOWRES_ZROW;
        const LrAxis ry = lr_axis(gy, h), rx = lr_axis(gx, w);
        float v = lr_sum(ry, rx, [&](int sp, int r, int cc) { return eb[(r * pitch + cc - org) * FINAL_LOWRES_ZROW + sp]; });
        v += beta[c];
        if (t != nullptr) v /= sigma_of_t(t[b], sigma);
        out[((size_t)b * H + gy) * W + gx] = v;
        return;
    }
    const int tx = blk % tiles_x; blk /= tiles_x;
    const int ty = blk % tiles_y;
    const int b = blk / tiles_y;
    const int x0 = tx * LG_X, y0 = ty * LG_Y;
    const int lx0 = (x0 >> 1) - 2, ly0 = (y0 >> 1) - 2;
    for (int i = tid; i < LG_PX * 7; i += 256) {
        const int px = i / 7, q = i - px * 7;
        const int pr = px / LG_PW, pc = px - pr * LG_PW;
        const int gy = ly0 + pr, gx = lx0 + pc;
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        if ((unsigned)gy < (unsigned)h && (unsigned)gx < (unsigned)w)
            v = reinterpret_cast<const f32x4*>(z)[(((size_t)b * h + gy) * w + gx) * 7 + q];
        s[(4 * q) * LG_LD + px] = v[0];
        if (q < 6) {                                             // q = 6: floats 24..27 of the row, position 24 and the padding
            s[(4 * q + 1) * LG_LD + px] = v[1];
            s[(4 * q + 2) * LG_LD + px] = v[2];
            s[(4 * q + 3) * LG_LD + px] = v[3];
        }
    }
    __syncthreads();
    const float sd = t != nullptr ? sigma_of_t(t[b], sigma) : 1.f;
    for (int o = tid; o < LG_X * LG_Y; o += 256) {
        const int oy = o / LG_X, ox = o - oy * LG_X;
        const int gy = y0 + oy, gx = x0 + ox;
        if (gy >= H || gx >= W) continue;
        if (gy == 0 || gy == H - 1 || gx == 0 || gx == W - 1) continue;          // the border ring has workgroups of its own
        const LrAxis ry = lr_axis(gy, h), rx = lr_axis(gx, w);
        float v = lr_sum(ry, rx, [&](int sp, int r, int cc) { return s[sp * LG_LD + (r - ly0) * LG_PW + (cc - lx0)]; });
        v += beta[4];
        if (t != nullptr) v /= sd;
        out[((size_t)b * H + gy) * W + gx] = v;
    }
}

// conv1's x-channel weights w1[co][0][v][u] (OIHW [64][cin][8][8]) as the A operand of skip_from_x: img[k step s][co][kq] = tap 4 s + kq
__global__ void skip_mix_pack_kernel(const float* __restrict__ w1, float* __restrict__ img, int cin) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= SKIP_MIX_PACKED_FLOATS) return;
    const int kq = i & 3, co = (i >> 2) & 63, s = i >> 8;
    img[i] = w1[(size_t)co * cin * 64 + 4 * s + kq];
}

}  // namespace

int sbgm_launch_final_compose(const float* w1_oihw, const float* b1, const float* w2_oihw, float* wc_oihw, float* bc, int C,
                              hipStream_t st) {
    SBGM_CHECK(w1_oihw && b1 && w2_oihw && wc_oihw && bc, "final_compose: null tensor");
    SBGM_CHECK(C >= 1 && C <= 4096, "final_compose: C=%d", C);
    const int total = 16 * C * 9 + 16;
    hipLaunchKernelGGL(final_compose_kernel, dim3((total + 255) / 256), dim3(256), 0, st, w1_oihw, b1, w2_oihw, wc_oihw, bc, C);
    SBGM_LAUNCH_CHECK();
    return 0;
}

int sbgm_launch_tap_gather_rows(const float* d, const float* bias, const float* t, float sigma, float* out, int B, int H, int W,
                                hipStream_t st) {
    SBGM_CHECK(d && bias && out && B >= 1 && H >= 1 && W >= 1, "tap_gather_rows: bad arguments");
    const int tiles_x = (W + GT_X - 1) / GT_X, tiles_y = (H + GT_Y - 1) / GT_Y;
    SBGM_CHECK((long long)B * tiles_x * tiles_y < (1ll << 31), "tap_gather_rows: too many tiles");
    hipLaunchKernelGGL(tap_gather_rows_kernel, dim3(B * tiles_x * tiles_y), dim3(256), 0, st, d, bias, t, sigma, out, B, H, W, tiles_x,
                       tiles_y);
    SBGM_LAUNCH_CHECK();
    return 0;
}

size_t sbgm_final_lowres_packed_floats(int C) { return (size_t)9 * (C / 16) * 32 * 16; }

size_t sbgm_final_lowres_ws_floats(int B, int h, int w) {
    return ((size_t)B * h * w + (size_t)B * lr_edge_pixels(h, w)) * FINAL_LOWRES_ZROW;
}

int sbgm_launch_final_lowres_pack(const float* w1_oihw, const float* b1, const float* w2_oihw, const float* b2, float* wz, float* beta,
                                  float* wz_packed, int C, hipStream_t st) {
    SBGM_CHECK(w1_oihw && b1 && w2_oihw && b2 && beta && wz_packed, "final_lowres_pack: null tensor");
    SBGM_CHECK(C >= 16 && C % 16 == 0 && C <= FINAL_LOWRES_MAX_C, "final_lowres_pack: C=%d must be a multiple of 16, at most %d", C,
               FINAL_LOWRES_MAX_C);
    const int total = (int)sbgm_final_lowres_packed_floats(C) + 9;
    hipLaunchKernelGGL(final_lowres_pack_kernel, dim3((total + 255) / 256), dim3(256), 0, st, w1_oihw, b1, w2_oihw, b2, wz, beta,
                       wz_packed, C);
    SBGM_LAUNCH_CHECK();
    return 0;
}

static int final_lowres_shape_ok(const char* who, int B, int h, int w) {
    SBGM_CHECK(B >= 1 && h >= 2 && w >= 2, "%s: needs a low-res map of at least 2 x 2 (B=%d h=%d w=%d)", who, B, h, w);
    SBGM_CHECK((long long)B * h * w < (1ll << 31) / 64, "%s: too many pixels", who);
    return 0;
}

int sbgm_launch_skip_mix_pack(const float* w1_oihw, float* w1x, int cin, hipStream_t st) {
    SBGM_CHECK(w1_oihw && w1x && cin >= 1, "skip_mix_pack: bad arguments");
    hipLaunchKernelGGL(skip_mix_pack_kernel, dim3(SKIP_MIX_PACKED_FLOATS / 256), dim3(256), 0, st, w1_oihw, w1x, cin);
    SBGM_LAUNCH_CHECK();
    return 0;
}

static int final_mix_launch(const float* x, const float* in_affine, const float* in_skip, int in_act, const float* wz_packed, float* zbuf,
                            int B, int h, int w, int C, const float* xin, const float* tb0, const float* w1x, hipStream_t st);

int sbgm_launch_final_mix(const float* x, const float* in_affine, const float* in_skip, int in_act, const float* wz_packed, float* zbuf,
                          int B, int h, int w, int C, hipStream_t st) {
    return final_mix_launch(x, in_affine, in_skip, in_act, wz_packed, zbuf, B, h, w, C, nullptr, nullptr, nullptr, st);
}

int sbgm_launch_final_mix_skipx(const float* x, const float* in_affine, int in_act, const float* wz_packed, const float* xin,
                                const float* sc, const float* tb0, const float* w1x, float* zbuf, int B, int h, int w, int C,
                                hipStream_t st) {
    SBGM_CHECK(xin && tb0 && w1x, "final_mix: the skip needs the planar input, the time row and conv1's x weights");
    SBGM_CHECK(C == 64, "final_mix: conv1's skip has 64 channels, the block %d", C);
    return final_mix_launch(x, in_affine, sc, in_act, wz_packed, zbuf, B, h, w, C, xin, tb0, w1x, st);
}

static int final_mix_launch(const float* x, const float* in_affine, const float* in_skip, int in_act, const float* wz_packed, float* zbuf,
                            int B, int h, int w, int C, const float* xin, const float* tb0, const float* w1x, hipStream_t st) {
    SBGM_CHECK(x && wz_packed && zbuf, "final_mix: null tensor");
    SBGM_CHECK(C >= 16 && C % 16 == 0 && C <= FINAL_LOWRES_MAX_C, "final_mix: C=%d must be a multiple of 16, at most %d", C, FINAL_LOWRES_MAX_C);
    if (final_lowres_shape_ok("final_mix", B, h, w)) return 1;
    const int M = B * h * w;
    float* edge = zbuf + (size_t)M * FINAL_LOWRES_ZROW;
    const int n_main = (M + 16 * 4 * MIX_FPW - 1) / (16 * 4 * MIX_FPW);
    const int n_edge_frags = B * (4 + 2 * ((2 * w + 15) / 16) + 2 * ((2 * h + 15) / 16));
    const dim3 grid(n_main + (n_edge_frags + 3) / 4);
#define SBGM_MIX(NKS)                                                                                                              \
    case NKS:                                                                                                                      \
        hipLaunchKernelGGL((final_mix_kernel<NKS, false>), grid, dim3(256), 0, st, x, in_affine, in_skip, in_act, wz_packed, zbuf, edge, h, \
                           w, M, n_main, n_edge_frags, xin, tb0, w1x);                                                             \
        break;
    if (xin != nullptr) {
        hipLaunchKernelGGL((final_mix_kernel<4, true>), grid, dim3(256), 0, st, x, in_affine, in_skip, in_act, wz_packed, zbuf, edge, h, w, M,
                           n_main, n_edge_frags, xin, tb0, w1x);
    } else switch (C / 16) {
        SBGM_MIX(1) SBGM_MIX(2) SBGM_MIX(3) SBGM_MIX(4) SBGM_MIX(5) SBGM_MIX(6) SBGM_MIX(7) SBGM_MIX(8)
    }
#undef SBGM_MIX
    SBGM_LAUNCH_CHECK();
    return 0;
}

int sbgm_launch_final_gather(const float* zbuf, const float* beta, const float* t, float sigma, float* out, int B, int h, int w,
                             hipStream_t st) {
    SBGM_CHECK(zbuf && beta && out, "final_gather: null tensor");
    if (final_lowres_shape_ok("final_gather", B, h, w)) return 1;
    const int tiles_x = (2 * w + LG_X - 1) / LG_X, tiles_y = (2 * h + LG_Y - 1) / LG_Y;
    SBGM_CHECK((long long)B * tiles_x * tiles_y < (1ll << 31), "final_gather: too many tiles");
    const float* edge = zbuf + (size_t)B * h * w * FINAL_LOWRES_ZROW;
    const int n_main = B * tiles_x * tiles_y, border_blocks = (4 * w + 4 * h - 4 + 255) / 256;
    hipLaunchKernelGGL(final_gather_kernel, dim3(n_main + B * border_blocks), dim3(256), 0, st, zbuf, edge, beta, t, sigma, out, h, w,
                       tiles_x, tiles_y, n_main, border_blocks);
    SBGM_LAUNCH_CHECK();
    return 0;
}
