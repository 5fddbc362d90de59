// The stem's two 8x8 / stride-2 / pad-3 convolutions composed into one 22x22 / stride-4 correlation (gfx950, fp32 MFMA).
//
// Encoder.forward has nothing non-linear between conv1 and conv2:  y2 = conv2(conv1(in) + tb0).  With conv2 tap (u, a) and conv1 tap
// (v, b) the input row of output row o is 2 (2o + u - 3) + v - 3 = 4o + r - 9, r = 2u + v in [0, 22), so
//     y2[b][co][oy][ox] = sum_cin sum_(ry, rx) Wc[class][cin][ry][rx][co] * in[b][cin][4 oy + ry - 9][4 ox + rx - 9]
//                       + sum_ci S[class][ci][co] * tb0[b][ci]
//     Wc[class][cin][ry][rx][co] = sum over valid (u, a) with 2u + v = ry, 2a + b = rx of sum_ci W2[co][ci][u][a] * W1[ci][cin][v][b]
//     S[class][ci][co]           = sum over valid (u, a) of W2[co][ci][u][a]
// conv2 zero-pads conv1's OUTPUT, so a conv2 tap u takes part only where the intermediate row 2o + u - 3 lies inside [0, 2 OH): per axis
// the outputs o = 0, 1, interior, OH - 2, OH - 1 have 5, 7, 8, 7, 5 valid taps (u in [3,7], [1,7], [0,7], [0,6], [0,4]): 5 x 5 = 25 classes
// of composed filter.  Input taps outside the image read zero (conv1's own padding).  The sums are formed in fp64 and rounded once.
//
// Kernel: implicit GEMM, M = pixels ordered (class, image, pixel of the class), N = 64, K = 528 per input channel (22 rows padded to
// 24 taps, zero weights in the padding) + 64 for the time-bias term, which rides along as 64 more K entries whose "input" is
// tb0[b][ci].  A 16-pixel fragment is class-homogeneous; a workgroup is 4 waves = 4 fragments of ONE class x all 64 channels, so its
// waves share the class's weight slab through LDS: a stage is 3 K-blocks of 16 (two filter rows) of one channel, 12 KB, loaded once per
// workgroup, register-staged one stage ahead.  The input is read straight from the planar [B][C][H][W] tensor: the K step (ry, rx0..+3)
// of the 16 pixels of a fragment in one row is one contiguous 256-byte segment.  Row / column validity is a per-lane bit mask; an
// invalid tap reads through the buffer descriptor's bounds check (0).
//
// Weight image: Wc[class][cin][kb = 33][co = 64][kq = 4][s = 4], k = 16 kb + 4 s + kq = 24 ry + rx: the lane (co, kq) of the A operand
// reads the four K steps of a K-block as one 16-byte quad, 64 lanes contiguous.  S has the same [class][kb = 4][co][kq][s] layout.
#include <type_traits>

#include "common.h"
#include "kernels.h"

namespace {

constexpr int KR = 22, KC = 24;             // filter rows, taps per row padded to a multiple of 4
constexpr int NKB = KR * KC / 16;           // 33 K-blocks of 16 per channel
constexpr int SKB = 3;                      // K-blocks per stage = two filter rows
constexpr int NST = NKB / SKB;              // 11 stages per channel
constexpr int TKB = 4;                      // K-blocks of the time-bias stage (64 intermediate channels)
constexpr int CO = 64, NCLS = 25;
constexpr int KBQ = CO * 4;                 // quads of one K-block

struct Stem22Params {
    const float* src;       // [B][nch][H][W]
    const float* wc;        // composed weights of all Cin channels
    const float* sb;        // S, or null with tb0
    const float* tb0;       // [B][64] or null
    const float* addend;    // [B][OH][OW][64] or null, added before scale / bias
    const float* scale;     // [64] or null
    const float* bias;      // [64] or null
    float* out;             // [B][OH][OW][64]
    int B, H, W, OH, OW, nch, c0, Cin, relu;
    uint32_t src_bytes, wc_bytes, tb_bytes;
    int wg_start[NCLS + 1];  // first workgroup of every class
};

__device__ __forceinline__ float buf_load1(__amdgpu_buffer_rsrc_t r, uint32_t byte_off) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (int)byte_off, 0, 0));
}

// first output and number of outputs of class c along an axis with O outputs
__host__ __device__ __forceinline__ int cls_first(int c, int O) { return c <= 2 ? c : O - 5 + c; }
__host__ __device__ __forceinline__ int cls_count(int c, int O) { return c == 2 ? O - 4 : 1; }

struct StageRegs { f32x4 w[TKB]; float x[4 * TKB]; };

template <bool TB>
__global__ __launch_bounds__(256, 2) void conv22s4_stem_kernel(const Stem22Params p) {
    __shared__ f32x4 wl[TKB * KBQ];             // [kb][co][kq] quads of (s)

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, kq = lane >> 4;

    int cls = 0, wg0 = 0;                       // class of this workgroup and the class's first workgroup
#pragma unroll
    for (int c = 1; c < NCLS; ++c) {
        const bool in = (int)blockIdx.x >= p.wg_start[c];
        cls = in ? c : cls;
        wg0 = in ? p.wg_start[c] : wg0;
    }
    const int cy = cls / 5, cx = cls - 5 * cy;
    const int nx = cls_count(cx, p.OW), npix = cls_count(cy, p.OH) * nx;

    // this lane's pixel (B operand column r16)
    const int q = (((int)blockIdx.x - wg0) * 4 + wave) * 16 + r16;
    const bool valid = q < p.B * npix;
    const int qq = valid ? q : 0;
    const int b = qq / npix, rr = qq - b * npix;
    const int py = rr / nx;
    const int oy = cls_first(cy, p.OH) + py, ox = cls_first(cx, p.OW) + (rr - py * nx);
    const int iy0 = 4 * oy - 9, ix0 = 4 * ox - 9;
    uint32_t rm = 0, cm = 0;                    // bit ry: the input row is inside; bit j: the column of tap rx = j + kq is a real, inside tap
#pragma unroll
    for (int r = 0; r < KR; ++r) {
        rm |= (uint32_t)(valid & ((unsigned)(iy0 + r) < (unsigned)p.H)) << r;
        cm |= (uint32_t)((unsigned)(ix0 + r) < (unsigned)p.W) << r;
    }
    cm >>= kq;
    const int HW = p.H * p.W;
    const int xbase = b * p.nch * HW + iy0 * p.W + ix0 + kq;

    const __amdgpu_buffer_rsrc_t xr = make_rsrc(p.src, p.src_bytes);
    const __amdgpu_buffer_rsrc_t wr = make_rsrc(p.wc, p.wc_bytes);
    const __amdgpu_buffer_rsrc_t sr = make_rsrc(p.sb, TB ? (uint32_t)(NCLS * TKB * KBQ * 16) : 0u);
    const __amdgpu_buffer_rsrc_t tr = make_rsrc(p.tb0, TB ? p.tb_bytes : 0u);
    constexpr uint32_t OOB = 0x80000000u;

    const int NS = p.nch * NST;                 // input stages

    auto stage_load = [&](int st, StageRegs& g) {
        const int ch = st / NST, rp = st - ch * NST;
        const uint32_t woff = (uint32_t)((((cls * p.Cin + p.c0 + ch) * NKB + rp * SKB) * KBQ + tid) * 16);
#pragma unroll
        for (int u = 0; u < SKB; ++u) g.w[u] = buf_load4(wr, woff + (uint32_t)(u * KBQ * 16));
        const int xo = xbase + ch * HW + 2 * rp * p.W;
        const uint32_t rms = rm >> (2 * rp);
#pragma unroll
        for (int t = 0; t < 4 * SKB; ++t) {
            const int ryl = t / 6, rx0 = 4 * (t % 6);
            const bool ok = ((rms >> ryl) & (cm >> rx0) & 1u) != 0;
            g.x[t] = buf_load1(xr, ok ? (uint32_t)(xo + ryl * p.W + rx0) * 4u : OOB);
        }
    };

    f32x4 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int aoff = r16 * 4 + kq;
    auto sweep = [&](auto nkb, const StageRegs& g) {
#pragma unroll
        for (int u = 0; u < decltype(nkb)::value; ++u) {
            f32x4 a[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = wl[u * KBQ + 64 * i + aoff];
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][s], g.x[4 * u + s], acc[i], 0, 0, 0);
        }
    };
    // stage st is in `cur` (its weights already in LDS); the loads of stage st + 1 go to `nxt` and are in flight during the sweep
    auto iter = [&](int st, StageRegs& cur, StageRegs& nxt) {
        if (st + 1 < NS) stage_load(st + 1, nxt);
        __syncthreads();
        sweep(std::integral_constant<int, SKB>{}, cur);
        __syncthreads();
        if (st + 1 < NS) {
#pragma unroll
            for (int u = 0; u < SKB; ++u) wl[u * KBQ + tid] = nxt.w[u];
        }
    };

    StageRegs ga, gb;
    if (TB) {                                   // the time-bias K entries first: S[class] and tb0[b] of the lane's image
        const uint32_t woff = (uint32_t)((cls * TKB * KBQ + tid) * 16);
#pragma unroll
        for (int u = 0; u < TKB; ++u) gb.w[u] = buf_load4(sr, woff + (uint32_t)(u * KBQ * 16));
#pragma unroll
        for (int t = 0; t < 4 * TKB; ++t) gb.x[t] = buf_load1(tr, valid ? (uint32_t)(b * CO + 4 * t + kq) * 4u : OOB);
    }
    stage_load(0, ga);
    if (TB) {
#pragma unroll
        for (int u = 0; u < TKB; ++u) wl[u * KBQ + tid] = gb.w[u];
        __syncthreads();
        sweep(std::integral_constant<int, TKB>{}, gb);
        __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < SKB; ++u) wl[u * KBQ + tid] = ga.w[u];
    for (int st = 0; st < NS; st += 2) {
        iter(st, ga, gb);
        if (st + 1 < NS) iter(st + 1, gb, ga);
    }

    // ---- epilogue: + addend, folded BatchNorm scale / shift, ReLU; NHWC store of 4 channels per lane and fragment -----------------------
    if (valid) {
        const size_t m = ((size_t)b * p.OH + oy) * p.OW + ox;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int co = 16 * i + 4 * kq;
            f32x4 v = acc[i];
            if (p.addend) v += *reinterpret_cast<const f32x4*>(p.addend + m * CO + co);
            if (p.scale) v *= *reinterpret_cast<const f32x4*>(p.scale + co);
            if (p.bias) v += *reinterpret_cast<const f32x4*>(p.bias + co);
            if (p.relu) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
            }
            *reinterpret_cast<f32x4*>(p.out + m * CO + co) = v;
        }
    }
}

// valid conv2 taps of class c along an axis: [lo, hi]
__device__ __forceinline__ int tap_lo(int c) { return c == 0 ? 3 : c == 1 ? 1 : 0; }
__device__ __forceinline__ int tap_hi(int c) { return c == 4 ? 4 : c == 3 ? 6 : 7; }

// OIHW conv1 [64][Cin][8][8], conv2 [64][64][8][8] -> Wc[25][Cin][33][64][4][4] and S[25][4][64][4][4] (header), fp64 sums rounded once
__global__ void pack_stem22_kernel(const float* __restrict__ w1, const float* __restrict__ w2, float* __restrict__ wc,
                                   float* __restrict__ sb, int Cin) {
    const size_t n_wc = (size_t)NCLS * Cin * NKB * KBQ * 4, n_sb = (size_t)NCLS * TKB * KBQ * 4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_wc + n_sb; i += (size_t)gridDim.x * blockDim.x) {
        const bool is_s = i >= n_wc;
        size_t r = is_s ? i - n_wc : i;
        const int s = (int)(r & 3), kq = (int)((r >> 2) & 3), co = (int)((r >> 4) & 63);
        r >>= 10;
        const int nkb = is_s ? TKB : NKB;
        const int kb = (int)(r % nkb); r /= nkb;
        const int cin = is_s ? 0 : (int)(r % Cin);
        const int cls = is_s ? (int)r : (int)(r / Cin);
        const int cy = cls / 5, cx = cls - 5 * cy;
        const int k = kb * 16 + 4 * s + kq;
        double v = 0.0;
        if (is_s) {
            const float* g2 = w2 + ((size_t)co * 64 + k) * 64;
            for (int u = tap_lo(cy); u <= tap_hi(cy); ++u)
                for (int a = tap_lo(cx); a <= tap_hi(cx); ++a) v += (double)g2[u * 8 + a];
            sb[i - n_wc] = (float)v;
            continue;
        }
        const int ry = k / KC, rx = k - ry * KC;
        if (rx < KR) {
            for (int u = tap_lo(cy); u <= tap_hi(cy); ++u) {
                const int vv = ry - 2 * u;
                if (vv < 0 || vv > 7) continue;
                for (int a = tap_lo(cx); a <= tap_hi(cx); ++a) {
                    const int bb = rx - 2 * a;
                    if (bb < 0 || bb > 7) continue;
                    const float* g2 = w2 + (size_t)co * 4096 + u * 8 + a;
                    const float* g1 = w1 + (size_t)cin * 64 + vv * 8 + bb;
                    for (int ci = 0; ci < 64; ++ci) v += (double)g2[ci * 64] * (double)g1[(size_t)ci * Cin * 64];
                }
            }
        }
        wc[i] = (float)v;
    }
}

}  // namespace

size_t sbgm_stem22_packed_floats(int Cin) { return (size_t)NCLS * Cin * NKB * KBQ * 4; }
size_t sbgm_stem22_bias_floats() { return (size_t)NCLS * TKB * KBQ * 4; }

int sbgm_launch_pack_stem22(const float* w1_oihw, const float* w2_oihw, float* wc, float* sb, int Cin, hipStream_t st) {
    SBGM_CHECK(Cin >= 1 && Cin <= 16, "pack_stem22: Cin=%d outside 1..16", Cin);
    const size_t total = sbgm_stem22_packed_floats(Cin) + sbgm_stem22_bias_floats();
    hipLaunchKernelGGL(pack_stem22_kernel, dim3((int)std::min<size_t>((total + 255) / 256, 16384)), dim3(256), 0, st, w1_oihw, w2_oihw,
                       wc, sb, Cin);
    SBGM_LAUNCH_CHECK();
    return 0;
}

// out[B][H/4][W/4][64] = act(scale * (sum over the channels c0 .. c0 + nch - 1 of the composed 22x22 / stride-4 correlation of
// src [B][nch][H][W] + S . tb0 + addend) + bias); tb0 / addend / scale / bias may be null.  Cin: channels of the weight image wc.
int sbgm_launch_conv_stem22(const float* src, int nch, int c0, int Cin, const float* wc, const float* sb, const float* tb0,
                            const float* addend, const float* scale, const float* bias, int relu, float* out, int B, int H, int W,
                            hipStream_t st) {
    SBGM_CHECK(src && wc && out, "conv_stem22: src, wc and out are required");
    SBGM_CHECK(B >= 1 && H >= 32 && W >= 32 && H % 4 == 0 && W % 4 == 0, "conv_stem22: needs H, W >= 32 and multiples of 4 (B=%d H=%d W=%d)", B, H, W);
    SBGM_CHECK(nch >= 1 && c0 >= 0 && c0 + nch <= Cin && Cin <= 16, "conv_stem22: channels %d..%d of %d", c0, c0 + nch - 1, Cin);
    SBGM_CHECK(tb0 == nullptr || sb != nullptr, "conv_stem22: tb0 needs the S image");
    SBGM_CHECK((size_t)B * nch * H * W * 4 < (1ull << 31), "conv_stem22: input tensor exceeds 2 GiB buffer window");
    Stem22Params p{};
    p.src = src; p.wc = wc; p.sb = sb; p.tb0 = tb0; p.addend = addend; p.scale = scale; p.bias = bias; p.out = out;
    p.B = B; p.H = H; p.W = W; p.OH = H / 4; p.OW = W / 4; p.nch = nch; p.c0 = c0; p.Cin = Cin; p.relu = relu;
    p.src_bytes = (uint32_t)((size_t)B * nch * H * W * 4);
    p.wc_bytes = (uint32_t)(sbgm_stem22_packed_floats(Cin) * 4);
    p.tb_bytes = (uint32_t)((size_t)B * CO * 4);
    int wgs = 0;
    for (int c = 0; c < NCLS; ++c) {
        p.wg_start[c] = wgs;
        const long long npix = (long long)B * cls_count(c / 5, p.OH) * cls_count(c % 5, p.OW);
        wgs += (int)((npix + 63) / 64);
    }
    p.wg_start[NCLS] = wgs;
    if (tb0) hipLaunchKernelGGL(conv22s4_stem_kernel<true>, dim3(wgs), dim3(256), 0, st, p);
    else hipLaunchKernelGGL(conv22s4_stem_kernel<false>, dim3(wgs), dim3(256), 0, st, p);
    SBGM_LAUNCH_CHECK();
    return 0;
}
