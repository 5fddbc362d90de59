// Adaptive probability-flow ODE solver of rk45_sampler: Dormand-Prince 5(4) with FSAL and the step controller of
// scipy.integrate.RK45 (restated in score_sampling.rk45_host_solve), everything but the network evaluations.
//
//   right-hand side  f(t, x) = c(t) * score(fp32(x), fp32(t)),  c(t) = fp32(-0.5 * fp32(g g)),  g = sigma^fp32(t) in fp32.
//   The seven stage derivatives stay as fp32 score slabs K[0..6] plus one float64 coefficient c[s] per stage (and per controller):
//   fp32 score x fp32 coefficient is an exact float64 product.  State y, y_new and every combination are float64.
//
// A controller ("group") is the whole batch (error_norm = batch, scipy's semantics) or one sample (error_norm = sample).  Its
// t, h, counters and status live in an OdeGroup in device memory, so one captured attempt replays for every attempt of every run.
// Grids are (blocks per sample, B): a block belongs to one sample, hence to one group, and reads that group's scalars once.
// Norms: per-block float64 partial sums in fixed slots, reduced by the one-block controller in a fixed order (no atomics on
// floating-point values), so a run is bitwise reproducible.
#include "common.h"
#include "kernels.h"

namespace {

typedef double f64x2 __attribute__((ext_vector_type(2)));

// Dormand-Prince 5(4) (the tableau of scipy.integrate.RK45)
__constant__ double RK_C[7] = {0.0, 1.0 / 5, 3.0 / 10, 4.0 / 5, 8.0 / 9, 1.0, 1.0};
__constant__ double RK_A[7][6] = {
    {0, 0, 0, 0, 0, 0},
    {1.0 / 5, 0, 0, 0, 0, 0},
    {3.0 / 40, 9.0 / 40, 0, 0, 0, 0},
    {44.0 / 45, -56.0 / 15, 32.0 / 9, 0, 0, 0},
    {19372.0 / 6561, -25360.0 / 2187, 64448.0 / 6561, -212.0 / 729, 0, 0},
    {9017.0 / 3168, -355.0 / 33, 46732.0 / 5247, 49.0 / 176, -5103.0 / 18656, 0},
    {35.0 / 384, 0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84}};          // row 6: B, the 5th-order weights
__constant__ double RK_E[7] = {-71.0 / 57600, 0, 71.0 / 16695, -71.0 / 1920, 17253.0 / 339200, -22.0 / 525, 1.0 / 40};

constexpr double SAFETY = 0.9, MIN_FACTOR = 0.2, MAX_FACTOR = 10.0;

__device__ __forceinline__ OdeGroup* groups_of(OdeHeader* h) { return reinterpret_cast<OdeGroup*>(h + 1); }
__device__ __forceinline__ const OdeGroup* groups_of(const OdeHeader* h) { return reinterpret_cast<const OdeGroup*>(h + 1); }

// c(t) in the reference's precision (score_sampling.py:296): everything in fp32, widened at the end.  The power is taken in float64 and
// rounded once, which gives the correctly rounded fp32 power that the host's powf returns (the device's powf may be an ulp off, and an
// ulp in c is the largest difference there is between this solver and scipy around the same network: enough to flip a step decision)
__device__ __forceinline__ double rhs_coef(float sigma, float tf) {
    const float g = (float)pow((double)sigma, (double)tf);
    const float g2 = g * g;
    return (double)(-0.5f * g2);
}

// Start of an attempt (scipy _step_impl up to rk_step): the minimal step at t, the lower clamp of a fresh step, TOO_SMALL_STEP
// after a rejection, the clip of t_new to t_bound.  Leaves the attempt's signed h and t_new in the group.
__device__ void prepare_attempt(const OdeHeader& hd, OdeGroup& g) {
    const double min_step = 10.0 * fabs(nextafter(g.t, hd.dir * (double)INFINITY) - g.t);
    if (!g.rejected) {
        if (g.h_abs < min_step) g.h_abs = min_step;
    } else if (g.h_abs < min_step) {
        g.status = SBGM_ODE_TOO_SMALL_STEP;
        return;
    }
    double h = g.h_abs * hd.dir;
    double t_new = g.t + h;
    if (hd.dir * (t_new - hd.t_bound) > 0) t_new = hd.t_bound;
    h = t_new - g.t;
    g.h = h;
    g.t_new = t_new;
    g.h_abs = fabs(h);
}

__global__ void ode_init_kernel(OdeHeader* hd, int groups, double t0, double t_bound, double rtol, double atol, float sigma,
                                long long max_steps) {
    OdeGroup* gs = groups_of(hd);
    for (int g = threadIdx.x; g < groups; g += blockDim.x) {
        OdeGroup v{};
        v.t = t0;
        gs[g] = v;
    }
    if (threadIdx.x == 0) {
        OdeHeader h{};
        h.t0 = t0; h.t_bound = t_bound; h.rtol = rtol; h.atol = atol; h.dir = t_bound >= t0 ? 1.0 : -1.0;
        h.sigma = sigma; h.groups = groups; h.max_steps = max_steps;
        *hd = h;
    }
}

__global__ __launch_bounds__(256) void ode_load_kernel(double* __restrict__ y, const float* __restrict__ x, size_t n4) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const f32x4 v = reinterpret_cast<const f32x4*>(x)[i];
        reinterpret_cast<f64x2*>(y)[2 * i] = f64x2{(double)v[0], (double)v[1]};
        reinterpret_cast<f64x2*>(y)[2 * i + 1] = f64x2{(double)v[2], (double)v[3]};
    }
}

__global__ __launch_bounds__(256) void ode_store_kernel(float* __restrict__ x, const double* __restrict__ y, size_t n4) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const f64x2 a = reinterpret_cast<const f64x2*>(y)[2 * i], b = reinterpret_cast<const f64x2*>(y)[2 * i + 1];
        reinterpret_cast<f32x4*>(x)[i] = f32x4{(float)a[0], (float)a[1], (float)b[0], (float)b[1]};
    }
}

// Network input of the next evaluation, the time it runs at and the coefficient its score will carry.
//   phase SBGM_ODE_PHASE_F0:  x = y                                    at t              -> K[0]   (first evaluation of a run)
//   phase SBGM_ODE_PHASE_F1:  x = y + (h0 dir) c0 K0                   at t + h0 dir     -> K[1]   (select_initial_step)
//   phase s = 1..5:           x = y + h sum_{j<s} a_sj c_j K_j         at t + C_s h      -> K[s]
//   phase 6:                  x = y_new = y + h sum_{j<6} b_j c_j K_j  at t + h          -> K[6]   (y_new is stored in float64 too)
// A group that has finished or failed is frozen: its rows are fed y at t again, nothing of it is written.
__global__ __launch_bounds__(256) void ode_stage_kernel(OdeHeader* __restrict__ hd, int phase, const double* __restrict__ y,
                                                        double* __restrict__ y_new, const float* __restrict__ K, size_t k_stride,
                                                        float* __restrict__ xs, float* __restrict__ t_dev, int t_copies,
                                                        int B, size_t per4, int per_sample) {
    const int b = blockIdx.y;
    const int gi = per_sample ? b : 0;
    OdeGroup& g = groups_of(hd)[gi];
    const bool live = g.status == SBGM_ODE_RUNNING;
    const bool f0 = phase == SBGM_ODE_PHASE_F0, f1 = phase == SBGM_ODE_PHASE_F1;
    const int slot = f0 ? 0 : f1 ? 1 : phase;
    const int terms = (!live || f0) ? 0 : f1 ? 1 : phase;
    const double h = f1 ? g.h0 * hd->dir : g.h;
    const double tt = (!live || f0) ? g.t : f1 ? g.t + h : g.t + RK_C[phase] * h;      // stage 6 runs at t + h, as scipy's rk_step
    const float tf = (float)tt;
    double a[6], c[6];                     // sum_j a_j (c_j K_j): c_j K_j is exact in float64, as the reference's float64 f is
#pragma unroll
    for (int j = 0; j < 6; ++j) { a[j] = j < terms ? (f1 ? 1.0 : RK_A[phase][j]) : 0.0; c[j] = j < terms ? g.c[j] : 0.0; }
    __syncthreads();                       // every thread has read the group before thread 0 publishes into it
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        for (int r = 0; r < t_copies; ++r) t_dev[(size_t)r * B + b] = tf;
        if (live && (per_sample || b == 0)) g.c[slot] = rhs_coef(hd->sigma, tf);
    }
    const size_t base = (size_t)b * per4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < per4; i += (size_t)gridDim.x * blockDim.x) {
        const size_t e = base + i;
        const f64x2 ya = reinterpret_cast<const f64x2*>(y)[2 * e], yb = reinterpret_cast<const f64x2*>(y)[2 * e + 1];
        double v[4] = {ya[0], ya[1], yb[0], yb[1]};
        if (terms > 0) {
            double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                if (j < terms) {
                    const f32x4 k = reinterpret_cast<const f32x4*>(K + (size_t)j * k_stride)[e];
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[q] += a[j] * (c[j] * (double)k[q]);
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] += acc[q] * h;
            if (phase == 6) {
                reinterpret_cast<f64x2*>(y_new)[2 * e] = f64x2{v[0], v[1]};
                reinterpret_cast<f64x2*>(y_new)[2 * e + 1] = f64x2{v[2], v[3]};
            }
        }
        reinterpret_cast<f32x4*>(xs)[e] = f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
    }
}

// sum of the block's values, the same order every time: wave butterfly, then the four wave sums in LDS
__device__ __forceinline__ double block_sum_256(double v, double* lds4) {
    const double w = wave_sum_d(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = w;
    __syncthreads();
    return (lds4[0] + lds4[1]) + (lds4[2] + lds4[3]);
}

// Norm partials.  what = 0: (y / scale)^2 and (f0 / scale)^2 with scale = atol + |y| rtol     (select_initial_step: d0, d1)
//                 what = 1: ((f1 - f0) / scale)^2                                                (d2)
//                 what = 2: (h K^T E / (atol + max(|y|, |y_new|) rtol))^2                        (the attempt's error norm)
// partials[2 * (b * gridDim.x + blockIdx.x) + {0, 1}]
__global__ __launch_bounds__(256) void ode_norm_kernel(const OdeHeader* __restrict__ hd, int what, const double* __restrict__ y,
                                                       const double* __restrict__ y_new, const float* __restrict__ K,
                                                       size_t k_stride, double* __restrict__ partials, size_t per4,
                                                       int per_sample) {
    __shared__ double lds4[4];
    const int b = blockIdx.y;
    const OdeGroup& g = groups_of(hd)[per_sample ? b : 0];
    const double rtol = hd->rtol, atol = hd->atol;
    double s0 = 0.0, s1 = 0.0;
    if (g.status == SBGM_ODE_RUNNING) {
        double w[7], c[7];
#pragma unroll
        for (int j = 0; j < 7; ++j) { w[j] = what == 2 ? RK_E[j] : 1.0; c[j] = g.c[j]; }
        const double h = g.h;
        const size_t base = (size_t)b * per4;
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < per4; i += (size_t)gridDim.x * blockDim.x) {
            const size_t e = base + i;
            const f64x2 ya = reinterpret_cast<const f64x2*>(y)[2 * e], yb = reinterpret_cast<const f64x2*>(y)[2 * e + 1];
            const double yv[4] = {ya[0], ya[1], yb[0], yb[1]};
            const f32x4 k0 = reinterpret_cast<const f32x4*>(K)[e];
            if (what == 2) {
                const f64x2 na = reinterpret_cast<const f64x2*>(y_new)[2 * e], nb = reinterpret_cast<const f64x2*>(y_new)[2 * e + 1];
                const double nv[4] = {na[0], na[1], nb[0], nb[1]};
                double acc[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[q] = w[0] * (c[0] * (double)k0[q]);
#pragma unroll
                for (int j = 2; j < 7; ++j) {                      // E[1] = 0
                    const f32x4 k = reinterpret_cast<const f32x4*>(K + (size_t)j * k_stride)[e];
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[q] += w[j] * (c[j] * (double)k[q]);
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const double r = acc[q] * h / (atol + fmax(fabs(yv[q]), fabs(nv[q])) * rtol);
                    s0 += r * r;
                }
            } else {
                const f32x4 k1 = what == 1 ? reinterpret_cast<const f32x4*>(K + k_stride)[e] : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const double sc = atol + fabs(yv[q]) * rtol;
                    const double f0 = c[0] * (double)k0[q];
                    if (what == 0) {
                        const double r0 = yv[q] / sc, r1 = f0 / sc;
                        s0 += r0 * r0;
                        s1 += r1 * r1;
                    } else {
                        const double r = (c[1] * (double)k1[q] - f0) / sc;
                        s0 += r * r;
                    }
                }
            }
        }
    }
    s0 = block_sum_256(s0, lds4);
    s1 = block_sum_256(s1, lds4);
    if (threadIdx.x == 0) {
        const size_t slot = 2 * ((size_t)b * gridDim.x + blockIdx.x);
        partials[slot] = s0;
        partials[slot + 1] = s1;
    }
}

// One block.  Reduces the partials of every group in a fixed order and takes the group's decision:
//   what = 0: h0 of select_initial_step;  what = 1: h1, the first step size, nfev = 2, first attempt prepared;
//   what = 2: accept / reject, step factor, counters, status, next attempt prepared; then the run's done word.
__global__ __launch_bounds__(256) void ode_control_kernel(OdeHeader* __restrict__ hd, int what, const double* __restrict__ partials,
                                                          int B, int blocks_per_sample, double values_per_sample, int per_sample) {
    __shared__ double red[2][256];
    __shared__ int running, was_live;
    OdeGroup* gs = groups_of(hd);
    const OdeHeader h = *hd;
    const int G = h.groups;
    if (threadIdx.x == 0) { running = 0; was_live = 0; }
    // batch mode: the block sums all B * blocks_per_sample slots together (thread-strided, then a fixed tree)
    double bsum[2] = {0.0, 0.0};
    if (!per_sample) {
        const int cnt = B * blocks_per_sample;
        double a0 = 0.0, a1 = 0.0;
        for (int i = threadIdx.x; i < cnt; i += 256) { a0 += partials[2 * i]; a1 += partials[2 * i + 1]; }
        red[0][threadIdx.x] = a0; red[1][threadIdx.x] = a1;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) { red[0][threadIdx.x] += red[0][threadIdx.x + o]; red[1][threadIdx.x] += red[1][threadIdx.x + o]; }
            __syncthreads();
        }
        bsum[0] = red[0][0]; bsum[1] = red[1][0];
    }
    __syncthreads();
    for (int gi = threadIdx.x; gi < G; gi += 256) {
        OdeGroup g = gs[gi];
        if (g.status != SBGM_ODE_RUNNING) {                 // frozen: a surplus attempt changes nothing
            if (g.accept) { g.accept = 0; gs[gi] = g; }
            continue;
        }
        atomicOr(&was_live, 1);
        double s0 = bsum[0], s1 = bsum[1], size = values_per_sample * (double)B;
        if (per_sample) {
            s0 = s1 = 0.0;
            for (int i = 0; i < blocks_per_sample; ++i) {
                s0 += partials[2 * ((size_t)gi * blocks_per_sample + i)];
                s1 += partials[2 * ((size_t)gi * blocks_per_sample + i) + 1];
            }
            size = values_per_sample;
        }
        const double n0 = sqrt(s0 / size), n1 = sqrt(s1 / size);
        if (what == 0) {
            const double interval = fabs(h.t_bound - g.t);
            double h0 = (n0 < 1e-5 || n1 < 1e-5) ? 1e-6 : 0.01 * n0 / n1;
            h0 = fmin(h0, interval);
            g.h0 = h0; g.d1 = n1;
            g.nfev = 1;
            if (!isfinite(n0) || !isfinite(n1)) g.status = SBGM_ODE_NONFINITE;
        } else if (what == 1) {
            const double interval = fabs(h.t_bound - g.t);
            const double d2 = n0 / g.h0;
            const double h1 = (g.d1 <= 1e-15 && d2 <= 1e-15) ? fmax(1e-6, g.h0 * 1e-3) : pow(0.01 / fmax(g.d1, d2), 1.0 / 5.0);
            g.h_abs = fmin(fmin(100.0 * g.h0, h1), interval);
            g.nfev = 2;
            if (!isfinite(d2)) g.status = SBGM_ODE_NONFINITE;
            else prepare_attempt(h, g);
        } else {
            const double err = n0;
            g.nfev += 6;
            g.accept = 0;
            if (!isfinite(err)) {
                g.status = SBGM_ODE_NONFINITE;
            } else if (err < 1.0) {
                double factor = err == 0.0 ? MAX_FACTOR : fmin(MAX_FACTOR, SAFETY * pow(err, -0.2));
                if (g.rejected) factor = fmin(1.0, factor);
                g.h_abs *= factor;
                g.t = g.t_new;
                g.c[0] = g.c[6];
                g.accept = 1;
                g.rejected = 0;
                g.n_accepted += 1;
                if (h.dir * (g.t - h.t_bound) >= 0) g.status = SBGM_ODE_FINISHED;
            } else {
                g.h_abs *= fmax(MIN_FACTOR, SAFETY * pow(err, -0.2));
                g.rejected = 1;
                g.n_rejected += 1;
            }
            if (g.status == SBGM_ODE_RUNNING) {
                if (g.n_accepted + g.n_rejected >= h.max_steps) g.status = SBGM_ODE_MAX_STEPS;
                else prepare_attempt(h, g);
            }
        }
        if (g.status == SBGM_ODE_RUNNING) atomicOr(&running, 1);
        gs[gi] = g;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        hd->done = running ? 0 : 1;
        if (what == 2 && was_live) hd->live_attempts = h.live_attempts + 1;
    }
}

// accept: y <- y_new, K[0] <- K[6] (first same as last; the controller moved c[6] to c[0])
__global__ __launch_bounds__(256) void ode_commit_kernel(const OdeHeader* __restrict__ hd, double* __restrict__ y,
                                                         const double* __restrict__ y_new, float* __restrict__ K, size_t k_stride,
                                                         size_t per4, int per_sample) {
    const int b = blockIdx.y;
    if (!groups_of(hd)[per_sample ? b : 0].accept) return;
    const size_t base = (size_t)b * per4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < per4; i += (size_t)gridDim.x * blockDim.x) {
        const size_t e = base + i;
        reinterpret_cast<f64x2*>(y)[2 * e] = reinterpret_cast<const f64x2*>(y_new)[2 * e];
        reinterpret_cast<f64x2*>(y)[2 * e + 1] = reinterpret_cast<const f64x2*>(y_new)[2 * e + 1];
        reinterpret_cast<f32x4*>(K)[e] = reinterpret_cast<const f32x4*>(K + 6 * k_stride)[e];
    }
}

inline int stream_blocks(size_t n) { return (int)std::min<size_t>((n + 255) / 256, 2048); }

int check_shape(const char* who, int B, size_t per) {
    SBGM_CHECK(B >= 1 && B <= 65535, "%s: batch %d out of range", who, B);
    SBGM_CHECK(per > 0 && per % 4 == 0, "%s: per-sample element count must be a positive multiple of 4", who);
    return 0;
}

}  // namespace

int sbgm_ode_blocks_per_sample(size_t per) { return (int)std::min<size_t>((per / 4 + 255) / 256, 16); }
size_t sbgm_ode_state_bytes(int groups) { return sizeof(OdeHeader) + sizeof(OdeGroup) * (size_t)groups; }
size_t sbgm_ode_partials_bytes(int B, size_t per) { return sizeof(double) * 2 * (size_t)B * sbgm_ode_blocks_per_sample(per); }

int sbgm_launch_ode_init(void* state, int groups, double t0, double t_bound, double rtol, double atol, float sigma,
                         long long max_steps, hipStream_t st) {
    SBGM_CHECK(groups >= 1, "ode_init: groups=%d", groups);
    SBGM_CHECK(rtol > 0 && atol >= 0 && t0 != t_bound && max_steps >= 1, "ode_init: need rtol > 0, atol >= 0, t0 != t_bound, max_steps >= 1");
    hipLaunchKernelGGL(ode_init_kernel, dim3(1), dim3(256), 0, st, static_cast<OdeHeader*>(state), groups, t0, t_bound, rtol, atol,
                       sigma, max_steps);
    SBGM_LAUNCH_CHECK();
    return 0;
}

int sbgm_launch_ode_load(double* y, const float* x, size_t n, hipStream_t st) {
    SBGM_CHECK(n % 4 == 0, "ode_load: element count must be a multiple of 4");
    hipLaunchKernelGGL(ode_load_kernel, dim3(stream_blocks(n / 4)), dim3(256), 0, st, y, x, n / 4);
    SBGM_LAUNCH_CHECK();
    return 0;
}

int sbgm_launch_ode_store(float* x, const double* y, size_t n, hipStream_t st) {
    SBGM_CHECK(n % 4 == 0, "ode_store: element count must be a multiple of 4");
    hipLaunchKernelGGL(ode_store_kernel, dim3(stream_blocks(n / 4)), dim3(256), 0, st, x, y, n / 4);
    SBGM_LAUNCH_CHECK();
    return 0;
}

int sbgm_launch_ode_stage(void* state, int phase, const double* y, double* y_new, const float* K, size_t k_stride, float* xs,
                          float* t_dev, int t_copies, int B, size_t per, int per_sample, hipStream_t st) {
    if (check_shape("ode_stage", B, per)) return 1;
    SBGM_CHECK((phase >= 1 && phase <= 6) || phase == SBGM_ODE_PHASE_F0 || phase == SBGM_ODE_PHASE_F1, "ode_stage: phase %d", phase);
    SBGM_CHECK(k_stride % 4 == 0 && k_stride >= (size_t)B * per, "ode_stage: stage stride %zu below B * per or not a multiple of 4", k_stride);
    SBGM_CHECK(t_copies == 1 || t_copies == 2, "ode_stage: t_copies=%d", t_copies);
    hipLaunchKernelGGL(ode_stage_kernel, dim3(sbgm_ode_blocks_per_sample(per), B), dim3(256), 0, st, static_cast<OdeHeader*>(state),
                       phase, y, y_new, K, k_stride, xs, t_dev, t_copies, B, per / 4, per_sample);
    SBGM_LAUNCH_CHECK();
    return 0;
}

int sbgm_launch_ode_control(void* state, int what, const double* y, const double* y_new, const float* K, size_t k_stride,
                            double* partials, int B, size_t per, int per_sample, hipStream_t st) {
    if (check_shape("ode_control", B, per)) return 1;
    SBGM_CHECK(what >= 0 && what <= 2, "ode_control: what=%d", what);
    const int bx = sbgm_ode_blocks_per_sample(per);
    hipLaunchKernelGGL(ode_norm_kernel, dim3(bx, B), dim3(256), 0, st, static_cast<const OdeHeader*>(state), what, y, y_new, K,
                       k_stride, partials, per / 4, per_sample);
    SBGM_LAUNCH_CHECK();
    hipLaunchKernelGGL(ode_control_kernel, dim3(1), dim3(256), 0, st, static_cast<OdeHeader*>(state), what, partials, B, bx,
                       (double)per, per_sample);
    SBGM_LAUNCH_CHECK();
    return 0;
}

int sbgm_launch_ode_commit(const void* state, double* y, const double* y_new, float* K, size_t k_stride, int B, size_t per,
                           int per_sample, hipStream_t st) {
    if (check_shape("ode_commit", B, per)) return 1;
    hipLaunchKernelGGL(ode_commit_kernel, dim3(sbgm_ode_blocks_per_sample(per), B), dim3(256), 0, st,
                       static_cast<const OdeHeader*>(state), y, y_new, K, k_stride, per / 4, per_sample);
    SBGM_LAUNCH_CHECK();
    return 0;
}

// Synchronous read-back: stats_i[4 g + {0,1,2,3}] = nfev, n_accepted, n_rejected, status of group g, then [4 G] = done word,
// [4 G + 1] = attempts in which any group was live; stats_d[g] = t of group g.
int sbgm_ode_read_state(const void* state, int groups, int64_t* stats_i, double* stats_d, hipStream_t st) {
    std::vector<char> buf(sbgm_ode_state_bytes(groups));
    SBGM_HIP(hipMemcpyAsync(buf.data(), state, buf.size(), hipMemcpyDeviceToHost, st));
    SBGM_HIP(hipStreamSynchronize(st));
    const OdeHeader* hd = reinterpret_cast<const OdeHeader*>(buf.data());
    const OdeGroup* gs = reinterpret_cast<const OdeGroup*>(hd + 1);
    SBGM_CHECK(hd->groups == groups, "ode_read_state: the state block holds %d groups, not %d", hd->groups, groups);
    for (int g = 0; g < groups; ++g) {
        stats_i[4 * g] = gs[g].nfev; stats_i[4 * g + 1] = gs[g].n_accepted; stats_i[4 * g + 2] = gs[g].n_rejected;
        stats_i[4 * g + 3] = gs[g].status;
        if (stats_d) stats_d[g] = gs[g].t;
    }
    stats_i[4 * groups] = hd->done;
    stats_i[4 * groups + 1] = hd->live_attempts;
    return 0;
}
