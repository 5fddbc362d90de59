// Device-resident cutout batches: what the reference's dataset does per sample on the host (data_modules.py:727-997) once the fields of a
// split sit in HBM as [N][Hd][Wd] stacks.
//
// K48 cutout_draw_kernel     — find_rand_points (data_modules.py:184-223) for a batch: sample b takes Philox block (seed, offset = draw,
//     idx = b) and y0 = r0 + min(max_off_y, (int)floorf(u_0 * (float)(max_off_y + 1))), x0 likewise from u_1, every step in fp32
//     (DESIGN.md 4.4).  u = 1 occurs (philox.h), hence the clamp.
// K49 cutout_gather_kernel   — one launch for every field of the batch: out[f][b][0][y][x] = program_f(src_f[item_b][y0_b + y][x0_b + x]),
//     item_b = 0 for the static planes; a field flagged "mask" is then binarised to v > 0.5 ? 1 : 0 (data_modules.py:874, :909).  x0 is
//     arbitrary, so a source row has no alignment: it is read as dwords (a wave's four loads cover the same cache lines), the output
//     row is written as f32x4 when w % 4 == 0.  A sample whose item or origin lies outside its stack gets NaN, never a wild read.
// K49b domain_gather_kernel  — the whole domain of a batch of days, right-padded for the tiler: out[f][b][0][y][x] =
//     program_f(src_f[item_b][y][min(x, Wd - 1)]), 0 <= x < Wp, Wp % 4 == 0.  The column is clamped BEFORE the program (the program is
//     pointwise, so this is the replicate pad of the transformed field).  A thread owns one output quad: four dword loads at clamped
//     columns (source rows of Wd floats have no alignment, and no load reaches past its row, let alone the plane), one f32x4 store.
// K50 sdf_* (three launches) — generate_sdf + normalize_sdf (data_modules.py:93-118) with an exact Euclidean distance transform:
//     columns:   g(y, x) = distance along the column to the nearest land pixel (two sweeps; SDF_FAR when the column has none)
//     rows:      D2(y, x) = min_x' (x - x')^2 + g(y, x')^2, the row of g held in LDS.  The search walks outwards from x and stops when
//                k^2 >= the best so far: every pixel it skips costs at least k^2, so the minimum is exact, never windowed.
//     normalise: raw = 10 land - sqrt(D2), sdf = (raw - min) / (max - min) per sample, in fp64, rounded once to fp32.  min and max
//                follow from the per-sample maximum of D2 and a has-land flag (integer atomics: order-independent).
//     Integer arithmetic up to D2; SDF_FAR^2 + (w - 1)^2 < 2^31 and SDF_FAR^2 exceeds every true D2 for sides <= 4096.
// All are latency- or HBM-bound at the loader's shapes (a batch of 128 x 128 crops is 64 KB per sample and field).
#include <algorithm>

#include "../../include/sbgm_hip.h"
#include "chain.h"
#include "common.h"
#include "kernels.h"
#include "philox.h"

namespace {

constexpr int SDF_FAR = 16384;
constexpr int SDF_MAX_SIDE = 4096;

__global__ __launch_bounds__(64) void cutout_draw_kernel(unsigned long long seed, unsigned long long draw, int B, int r0, int c0,
                                                         int max_off_y, int max_off_x, int* __restrict__ origins) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const f32x4 u = philox_uniform4(seed, draw, (unsigned long long)b);
    const int oy = (int)floorf(__fmul_rn(u[0], (float)(max_off_y + 1)));
    const int ox = (int)floorf(__fmul_rn(u[1], (float)(max_off_x + 1)));
    origins[2 * b] = r0 + (oy < max_off_y ? oy : max_off_y);
    origins[2 * b + 1] = c0 + (ox < max_off_x ? ox : max_off_x);
}

struct GatherArgs {
    const float* src[SBGM_CUTOUT_MAX_FIELDS];
    float* dst[SBGM_CUTOUT_MAX_FIELDS];
    int n_items[SBGM_CUTOUT_MAX_FIELDS];          // N of a stack, 0 for a static plane
    int Hd, Wd, h, w, vec4;
};

__device__ __forceinline__ float gather_value(float v, const ChainProgram& p, int is_mask) {
    v = chain_apply(v, p);
    return is_mask ? (v > 0.5f ? 1.f : 0.f) : v;
}

__global__ __launch_bounds__(256) void cutout_gather_kernel(GatherArgs a, const CutoutProgram* __restrict__ programs,
                                                            const int* __restrict__ items, const int* __restrict__ origins) {
    const int f = blockIdx.z, b = blockIdx.y;
    const int n_items = a.n_items[f];
    const int item = n_items > 0 ? items[b] : 0;
    const int y0 = origins[2 * b], x0 = origins[2 * b + 1];
    const bool inside = item >= 0 && (n_items == 0 || item < n_items) && y0 >= 0 && x0 >= 0 && y0 <= a.Hd - a.h && x0 <= a.Wd - a.w;
    const size_t per = (size_t)a.h * a.w;
    float* dst = a.dst[f] + (size_t)b * per;
    const float* src = a.src[f] + ((size_t)item * a.Hd + (inside ? y0 : 0)) * a.Wd + (inside ? x0 : 0);
    const CutoutProgram& pg = programs[f];
    ChainProgram p;
    p.n_ops = pg.n_ops < SBGM_CHAIN_MAX_OPS ? pg.n_ops : SBGM_CHAIN_MAX_OPS;
#pragma unroll
    for (int i = 0; i < SBGM_CHAIN_MAX_OPS; ++i) { p.op[i] = pg.ops[i]; p.c[i] = pg.consts[i]; }
    const int is_mask = pg.is_mask;
    const float nanv = __uint_as_float(0x7FC00000u);
    const size_t stride = (size_t)gridDim.x * blockDim.x, first = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (a.vec4) {
        const int wq = a.w >> 2;
        for (size_t q = first; q < per >> 2; q += stride) {
            const int y = (int)(q / wq), x = (int)(q % wq) << 2;
            f32x4 v = {nanv, nanv, nanv, nanv};
            if (inside) {
                const float* s = src + (size_t)y * a.Wd + x;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = gather_value(s[e], p, is_mask);
            }
            reinterpret_cast<f32x4*>(dst)[q] = v;
        }
    } else {
        for (size_t i = first; i < per; i += stride) {
            const int y = (int)(i / a.w), x = (int)(i % a.w);
            dst[i] = inside ? gather_value(src[(size_t)y * a.Wd + x], p, is_mask) : nanv;
        }
    }
}

struct DomainGatherArgs {
    const float* src[SBGM_CUTOUT_MAX_FIELDS];
    float* dst[SBGM_CUTOUT_MAX_FIELDS];
    int n_items[SBGM_CUTOUT_MAX_FIELDS];          // N of a stack, 0 for a static plane
    int Hd, Wd, Wp;
};

__global__ __launch_bounds__(256) void domain_gather_kernel(DomainGatherArgs a, const CutoutProgram* __restrict__ programs,
                                                            const int* __restrict__ items) {
    const int f = blockIdx.z, b = blockIdx.y;
    const int n_items = a.n_items[f];
    const int item = n_items > 0 ? items[b] : 0;
    const bool inside = item >= 0 && (n_items == 0 || item < n_items);
    const int wq = a.Wp >> 2, last = a.Wd - 1;
    const size_t quads = (size_t)a.Hd * wq;
    f32x4* dst = reinterpret_cast<f32x4*>(a.dst[f]) + (size_t)b * quads;
    const float* src = a.src[f] + (size_t)(inside ? item : 0) * a.Hd * a.Wd;
    const CutoutProgram& pg = programs[f];
    ChainProgram p;
    p.n_ops = pg.n_ops < SBGM_CHAIN_MAX_OPS ? pg.n_ops : SBGM_CHAIN_MAX_OPS;
#pragma unroll
    for (int i = 0; i < SBGM_CHAIN_MAX_OPS; ++i) { p.op[i] = pg.ops[i]; p.c[i] = pg.consts[i]; }
    const int is_mask = pg.is_mask;
    const float nanv = __uint_as_float(0x7FC00000u);
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += stride) {
        const int y = (int)(q / wq), x = (int)(q % wq) << 2;
        f32x4 v = {nanv, nanv, nanv, nanv};
        if (inside) {
            const float* s = src + (size_t)y * a.Wd;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = gather_value(s[x + e < last ? x + e : last], p, is_mask);
        }
        dst[q] = v;
    }
}

// stats: uint32 [B][2] = (max D2, has land), cleared here for the row pass that follows on the stream
__global__ __launch_bounds__(256) void sdf_columns_kernel(const float* __restrict__ mask, int* __restrict__ g, unsigned int* __restrict__ stats,
                                                          int B, int h, int w) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, total = (size_t)B * w;
    for (size_t i = t; i < 2 * (size_t)B; i += (size_t)gridDim.x * blockDim.x) stats[i] = 0u;
    if (t >= total) return;
    const int b = (int)(t / w), x = (int)(t % w);
    const float* m = mask + (size_t)b * h * w + x;
    int* gc = g + (size_t)b * h * w + x;
    int d = SDF_FAR;
    for (int y = 0; y < h; ++y) {
        d = m[(size_t)y * w] > 0.f ? 0 : (d < SDF_FAR ? d + 1 : SDF_FAR);
        gc[(size_t)y * w] = d;
    }
    d = SDF_FAR;
    for (int y = h - 1; y >= 0; --y) {
        const int down = gc[(size_t)y * w];
        d = down == 0 ? 0 : (d < SDF_FAR ? d + 1 : SDF_FAR);
        if (d < down) gc[(size_t)y * w] = d;
    }
}

// one workgroup per row (b, y); g is overwritten by D2 in place (the row is in LDS before its first pixel is written)
__global__ __launch_bounds__(256) void sdf_rows_kernel(int* __restrict__ g, unsigned int* __restrict__ stats, int h, int w) {
    __shared__ int row[SDF_MAX_SIDE];
    __shared__ unsigned int sh_max, sh_land;
    const int b = blockIdx.x / h;
    int* gr = g + (size_t)blockIdx.x * w;
    if (threadIdx.x == 0) { sh_max = 0u; sh_land = 0u; }
    for (int x = threadIdx.x; x < w; x += blockDim.x) row[x] = gr[x];
    __syncthreads();
    unsigned int local_max = 0u, local_land = 0u;
    for (int x = threadIdx.x; x < w; x += blockDim.x) {
        int best = row[x] * row[x];
        for (int k = 1; k < w && k * k < best; ++k) {
            if (x - k >= 0) { const int v = row[x - k]; best = min(best, k * k + v * v); }
            if (x + k < w) { const int v = row[x + k]; best = min(best, k * k + v * v); }
        }
        gr[x] = best;
        local_max = max(local_max, (unsigned int)best);
        local_land |= best == 0;
    }
    atomicMax(&sh_max, local_max);
    if (local_land) atomicOr(&sh_land, 1u);
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicMax(&stats[2 * b], sh_max);
        if (sh_land) atomicOr(&stats[2 * b + 1], 1u);
    }
}

__global__ __launch_bounds__(256) void sdf_normalise_kernel(const int* __restrict__ D2, const unsigned int* __restrict__ stats,
                                                            float* __restrict__ sdf, int* __restrict__ d2_out, size_t per, size_t total) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int b = (int)(i / per);
        const unsigned int mx = stats[2 * b], has_land = stats[2 * b + 1];
        const int d2 = D2[i];
        float v;
        if (!has_land) v = 0.f;                       // no land: nothing to measure a distance to
        else if (mx == 0u) v = 1.f;                   // no sea: the reference's 0 / 0
        else {
            const double lo = -sqrt((double)mx), raw = d2 == 0 ? 10.0 : -sqrt((double)d2);
            v = (float)((raw - lo) / (10.0 - lo));
        }
        sdf[i] = v;
        if (d2_out) d2_out[i] = has_land ? d2 : -1;
    }
}

size_t sdf_stats_bytes(int B) { return ((size_t)B * 8 + 15) / 16 * 16; }

}  // namespace

int sbgm_launch_cutout_draw(unsigned long long seed, unsigned long long draw, int B, const int* rect, int h, int w, int Hd, int Wd,
                            int* origins, hipStream_t st) {
    SBGM_CHECK(rect && origins && B >= 1 && h >= 1 && w >= 1, "cutout_draw: bad arguments (B=%d crop %dx%d)", B, h, w);
    const int r0 = rect[0], r1 = rect[1], c0 = rect[2], c1 = rect[3];
    SBGM_CHECK(r0 >= 0 && c0 >= 0 && r1 <= Hd && c1 <= Wd && r0 < r1 && c0 < c1,
               "cutout_draw: rectangle [%d, %d, %d, %d] lies outside the %dx%d domain", r0, r1, c0, c1, Hd, Wd);
    SBGM_CHECK(h <= r1 - r0 && w <= c1 - c0, "cutout_draw: crop size %dx%d is larger than the rectangle %dx%d", h, w, r1 - r0, c1 - c0);
    hipLaunchKernelGGL(cutout_draw_kernel, dim3((B + 63) / 64), dim3(64), 0, st, seed, draw, B, r0, c0, r1 - r0 - h, c1 - c0 - w, origins);
    SBGM_LAUNCH_CHECK();
    return 0;
}

static_assert(sizeof(CutoutProgram) == 4 * SBGM_CUTOUT_PROGRAM_WORDS && SBGM_CHAIN_MAX_OPS == 12, "program table row");

int sbgm_launch_cutout_gather(const float* const* srcs, float* const* dsts, const int* n_items, int n_fields, const CutoutProgram* programs,
                              const int* items, const int* origins, int B, int Hd, int Wd, int h, int w, hipStream_t st) {
    SBGM_CHECK(n_fields >= 1 && n_fields <= SBGM_CUTOUT_MAX_FIELDS, "cutout_gather: %d fields (1..%d)", n_fields, SBGM_CUTOUT_MAX_FIELDS);
    SBGM_CHECK(B >= 1 && B <= 65535 && h >= 1 && w >= 1 && h <= Hd && w <= Wd, "cutout_gather: B=%d crop %dx%d domain %dx%d", B, h, w, Hd, Wd);
    SBGM_CHECK(srcs && dsts && n_items && programs && items && origins, "cutout_gather: null argument");
    GatherArgs g{};
    int stacks = 0, planes = 0;
    bool vec4 = w % 4 == 0;
    for (int f = 0; f < n_fields; ++f) {
        SBGM_CHECK(srcs[f] && dsts[f] && n_items[f] >= 0, "cutout_gather: field %d is null or has a negative item count", f);
        (n_items[f] > 0 ? stacks : planes) += 1;
        g.src[f] = srcs[f];
        g.dst[f] = dsts[f];
        g.n_items[f] = n_items[f];
        vec4 = vec4 && ((uintptr_t)dsts[f] % 16) == 0;
    }
    SBGM_CHECK(stacks <= 1 + SBGM_ASSEMBLE_MAX_LR && planes <= 2, "cutout_gather: %d stacks (max %d), %d static planes (max 2)", stacks,
               1 + SBGM_ASSEMBLE_MAX_LR, planes);
    g.Hd = Hd; g.Wd = Wd; g.h = h; g.w = w; g.vec4 = vec4;
    const size_t work = vec4 ? (size_t)h * w / 4 : (size_t)h * w;
    const int bx = (int)std::min<size_t>((work + 255) / 256, 256);
    hipLaunchKernelGGL(cutout_gather_kernel, dim3(bx, B, n_fields), dim3(256), 0, st, g, programs, items, origins);
    SBGM_LAUNCH_CHECK();
    return 0;
}

int sbgm_launch_domain_gather(const float* const* srcs, float* const* dsts, const int* n_items, int n_fields, const CutoutProgram* programs,
                              const int* items, int B, int Hd, int Wd, int Wp, hipStream_t st) {
    SBGM_CHECK(n_fields >= 1 && n_fields <= SBGM_CUTOUT_MAX_FIELDS, "domain_gather: %d fields (1..%d)", n_fields, SBGM_CUTOUT_MAX_FIELDS);
    SBGM_CHECK(B >= 1 && B <= 65535 && Hd >= 1 && Wd >= 1, "domain_gather: B=%d domain %dx%d", B, Hd, Wd);
    SBGM_CHECK(Wp >= Wd && Wp % 4 == 0, "domain_gather: padded width %d (a multiple of 4, at least the domain width %d)", Wp, Wd);
    SBGM_CHECK(srcs && dsts && n_items && programs && items, "domain_gather: null argument");
    DomainGatherArgs g{};
    int stacks = 0, planes = 0;
    for (int f = 0; f < n_fields; ++f) {
        SBGM_CHECK(srcs[f] && dsts[f] && n_items[f] >= 0, "domain_gather: field %d is null or has a negative item count", f);
        SBGM_CHECK((uintptr_t)dsts[f] % 16 == 0, "domain_gather: dst of field %d is not 16-byte aligned", f);
        (n_items[f] > 0 ? stacks : planes) += 1;
        g.src[f] = srcs[f];
        g.dst[f] = dsts[f];
        g.n_items[f] = n_items[f];
    }
    SBGM_CHECK(stacks <= 1 + SBGM_ASSEMBLE_MAX_LR && planes <= 2, "domain_gather: %d stacks (max %d), %d static planes (max 2)", stacks,
               1 + SBGM_ASSEMBLE_MAX_LR, planes);
    g.Hd = Hd; g.Wd = Wd; g.Wp = Wp;
    const size_t quads = (size_t)Hd * (Wp / 4);
    const int bx = (int)std::min<size_t>((quads + 255) / 256, 256);
    hipLaunchKernelGGL(domain_gather_kernel, dim3(bx, B, n_fields), dim3(256), 0, st, g, programs, items);
    SBGM_LAUNCH_CHECK();
    return 0;
}

static int check_sdf(int B, int h, int w) {
    SBGM_CHECK(B >= 1 && h >= 1 && w >= 1 && h <= SDF_MAX_SIDE && w <= SDF_MAX_SIDE && (long long)B * h < (1ll << 31),
               "sdf_from_mask: B=%d, %dx%d (sides 1..%d)", B, h, w, SDF_MAX_SIDE);
    return 0;
}

long long sbgm_sdf_ws_bytes(int B, int h, int w) {
    if (check_sdf(B, h, w)) return -1;
    return (long long)(sdf_stats_bytes(B) + (size_t)B * h * w * 4);
}

int sbgm_launch_sdf_from_mask(const float* mask, float* sdf, int* d2, void* ws, int B, int h, int w, hipStream_t st) {
    if (check_sdf(B, h, w)) return 1;
    SBGM_CHECK(mask && sdf && ws, "sdf_from_mask: mask, sdf and workspace are required");
    unsigned int* stats = static_cast<unsigned int*>(ws);
    int* g = reinterpret_cast<int*>(static_cast<char*>(ws) + sdf_stats_bytes(B));
    const size_t cols = (size_t)B * w, total = (size_t)B * h * w;
    hipLaunchKernelGGL(sdf_columns_kernel, dim3((unsigned)((cols + 255) / 256)), dim3(256), 0, st, mask, g, stats, B, h, w);
    SBGM_LAUNCH_CHECK();
    const int threads = std::min(256, (w + 63) / 64 * 64);
    hipLaunchKernelGGL(sdf_rows_kernel, dim3((unsigned)(B * h)), dim3(threads), 0, st, g, stats, h, w);
    SBGM_LAUNCH_CHECK();
    hipLaunchKernelGGL(sdf_normalise_kernel, dim3((unsigned)std::min<size_t>((total + 255) / 256, 8192)), dim3(256), 0, st, g, stats, sdf, d2,
                       (size_t)h * w, total);
    SBGM_LAUNCH_CHECK();
    return 0;
}
