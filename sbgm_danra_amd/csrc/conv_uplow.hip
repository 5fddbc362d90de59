// A decoder block's conv_up(up(x)) on a small map, with the channels mixed at LOW resolution.
//
// `up` (bilinear x2, align_corners = False) acts per channel and a 3x3 tap's weight acts per pixel, so the two commute:
//   conv_up(up(x))[co][o] = b[co] + sum_{tap = (k, l), o + tap - 1 inside the HIGH-res map} up(Z_tap)[co][o + tap - 1]
//   Z_tap[co]             = sum_ci W[co][ci][k][l] x[ci]                       on the low-resolution map
// The 9 tap mixes are ONE 1x1 product with N = 9 C over a quarter of the pixels (2 C^2 9/4 flop per output pixel instead of 2 C^2 9),
// run by the ordinary implicit-GEMM convolution from the image sbgm_launch_up_lowres_pack builds; Z is [B h w][9 C], row n = tap C + co.
// The gather below finishes the block: 9 taps x 4 bilinear neighbours per output element from Z rows staged in LDS, the bias, and, where
// a workgroup holds a whole (sample, GroupNorm group), norm1 itself.  A tap whose intermediate pixel lies outside the high-res map is
// skipped: that is the zero padding of conv_up's input.
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
};

// Grid (channel slices, row chunks, B).  A workgroup stages the low-res rows its chunk reads, all 9 taps of its CW channels, as
// s[pixel][tap][CW]; a thread owns a channel quad of an output pixel (lanes along the channels: 16-byte LDS reads of consecutive
// addresses), sums the taps in a fixed order and stores the raw value.  With statistics every thread adds its values in fp64, the
// waves combine by butterfly and the workgroup in wave order: no atomics, the same sum in every run.  UP_NORMED (one chunk): the
// workgroup holds the whole (sample, group), so each thread reads back what it stored and applies norm1 as groupnorm_apply_kernel does.
__global__ __launch_bounds__(256) void up_gather_kernel(UpGatherArgs a) {
    extern __shared__ __attribute__((aligned(16))) float s[];
    __shared__ double red[8];
    const int tid = threadIdx.x, slice = blockIdx.x, chunk = blockIdx.y, b = blockIdx.z;
    const int H = 2 * a.h, W = 2 * a.w, C = a.C, qs = a.CW >> 2, c0 = slice * a.CW, cq = C >> 2;
    const int y0 = chunk * a.rows, y1 = min(H, y0 + a.rows);
    const int ly0 = up_lo(max(y0 - 1, 0)), ly1 = up_hi(min(y1, H - 1), a.h);
    const int row_q = 9 * qs, n_q = (ly1 - ly0 + 1) * a.w * row_q;
    const f32x4* const zq = reinterpret_cast<const f32x4*>(a.z) + ((size_t)b * a.h + ly0) * a.w * (size_t)(9 * cq) + (c0 >> 2);
    f32x4* const s4 = reinterpret_cast<f32x4*>(s);
    for (int i = tid; i < n_q; i += 256) {
        const int lp = i / row_q, r = i - lp * row_q, tap = r / qs, q = r - tap * qs;
        s4[i] = zq[(size_t)lp * (9 * cq) + tap * cq + q];
    }
    __syncthreads();
    const int items = (y1 - y0) * W * qs;
    f32x4* const ob = reinterpret_cast<f32x4*>(a.out) + (size_t)b * H * W * cq + (c0 >> 2);
    double sm = 0.0, sq = 0.0;
    for (int i = tid; i < items; i += 256) {
        const int px = i / qs, q = i - px * qs, py = px / W, ox = px - py * W, oy = y0 + py;
        const UpAxis ry = up_axis(oy, a.h), rx = up_axis(ox, a.w);
        f32x4 v = *reinterpret_cast<const f32x4*>(a.bias + c0 + 4 * q);
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            if (!ry.in[ky]) continue;
            const int ra = (ry.a[ky] - ly0) * a.w, rb = (ry.b[ky] - ly0) * a.w;
            const float wy = ry.wa[ky];
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                if (!rx.in[kx]) continue;
                const f32x4* const t = s4 + (ky * 3 + kx) * qs + q;
                const float wx = rx.wa[kx];
                const f32x4 top = wx * t[(ra + rx.a[kx]) * row_q] + (1.f - wx) * t[(ra + rx.b[kx]) * row_q];
                const f32x4 bot = wx * t[(rb + rx.a[kx]) * row_q] + (1.f - wx) * t[(rb + rx.b[kx]) * row_q];
                v += wy * top + (1.f - wy) * bot;
            }
        }
        ob[((size_t)oy * W + ox) * cq + q] = v;
        if (a.mode != UP_RAW) {
#pragma unroll
            for (int e = 0; e < 4; ++e) { sm += (double)v[e]; sq += (double)v[e] * (double)v[e]; }
        }
    }
    if (a.mode == UP_RAW) return;
    sm = wave_sum_d(sm);
    sq = wave_sum_d(sq);
    if ((tid & 63) == 0) { red[2 * (tid >> 6)] = sm; red[2 * (tid >> 6) + 1] = sq; }
    __syncthreads();
    const double tot = ((red[0] + red[2]) + red[4]) + red[6], tot2 = ((red[1] + red[3]) + red[5]) + red[7];
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
    for (int i = tid; i < items; i += 256) {
        const int px = i / qs, q = i - px * qs, py = px / W, ox = px - py * W, oy = y0 + py;
        const int c = c0 + 4 * q;
        f32x4 g = f32x4{rstd, rstd, rstd, rstd}, bt = f32x4{0.f, 0.f, 0.f, 0.f};
        if (a.gamma != nullptr) {
            g *= *reinterpret_cast<const f32x4*>(a.gamma + c);
            bt = *reinterpret_cast<const f32x4*>(a.beta + c);
        }
        f32x4* const o = ob + ((size_t)oy * W + ox) * cq + q;
        *o = (*o - mu) * g + bt;
    }
}

constexpr size_t UP_LDS_MAX = 160 * 1024 - 512;      // staged Z rows of one workgroup (the reduction scratch is static)
constexpr int UP_MAX_CHUNKS = 64;                    // as many chunk partials as groupnorm_apply reduces

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
    int rows = H, chunks = 1;
    auto fit = [&]() {      // the chunking at which a workgroup's Z rows fit the LDS; false: not even two output rows do
        const size_t px_bytes = (size_t)9 * CW * 4;
        rows = H; chunks = 1;
        if ((size_t)h * w * px_bytes <= UP_LDS_MAX) return true;
        const size_t lo_rows = UP_LDS_MAX / ((size_t)w * px_bytes);      // an even chunk of R rows reads R / 2 + 2 low-res rows
        if (lo_rows < 3) return false;
        rows = (int)std::min<size_t>(2 * (lo_rows - 2), (size_t)H);
        chunks = (H + rows - 1) / rows;
        return true;
    };
    bool ok = fit();
    if (aware && (!ok || chunks > UP_MAX_CHUNKS)) { aware = false; CW = 16; ok = fit(); }
    SBGM_CHECK(ok && chunks <= 65535, "up_gather: a low-res row of %d pixels does not fit the LDS", w);
    const int lo_rows = chunks == 1 ? h : std::min(h, rows / 2 + 2);
    const size_t lds = (size_t)lo_rows * w * 9 * CW * 4;
    static bool attr = false;
    if (lds > 64 * 1024 && !attr) {
        SBGM_HIP(hipFuncSetAttribute((const void*)up_gather_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)UP_LDS_MAX));
        attr = true;
    }
    UpGatherArgs a{z, bias, out, gamma, beta, stats, h, w, C, CW, rows, aware ? (chunks == 1 ? UP_NORMED : UP_PARTIALS) : UP_RAW, eps};
    hipLaunchKernelGGL(up_gather_kernel, dim3(C / CW, chunks, B), dim3(256), lds, st, a);
    SBGM_LAUNCH_CHECK();
    *chunks_out = a.mode == UP_PARTIALS ? chunks : 0;
    *normed_out = a.mode == UP_NORMED;
    return 0;
}
