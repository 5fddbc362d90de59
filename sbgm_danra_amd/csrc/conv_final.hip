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
