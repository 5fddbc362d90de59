// K25 / K26 / K27: per-step state updates of the reverse-SDE samplers, fused with the Gaussian draw.
// reference sbgm/score_sampling.py:124-125 (Euler-Maruyama), :200-204 (Langevin corrector), :224-227 (predictor),
// :55 (classifier-free-guidance combine).  Beyond the reference: the EDM Heun updates of edm_heun_sampler (churn / euler / heun) and the
// DPM-Solver++(2M) update of dpmpp_2m_sampler.
//
// Noise: when `z` is null the kernels draw N(0,1) themselves (Philox4x32-10 counter RNG + Box-Muller, keyed by
// (seed, running offset, element index)), so the sampler loop never round-trips noise through HBM; when `z`
// is given (parity mode) the host-generated draw is used verbatim.  With a noise plan (kernels.h: NoiseMap) the counter
// is keyed by the sample's noise row instead of its place in the batch and the draw is a moving average over the preceding rows.
// Joint tiled sampling: the JOINT instantiations of the five update kernels read the score through the partition-of-unity
// blend of all tiles' scores (tile_blend.h), so the T tiles of a domain are one diffusion and copies of a domain pixel stay bit-equal.
// All per-step scalars come from a device-resident table indexed by a device-side step counter, so one captured
// hipGraph replays for every step.
#include "common.h"
#include "kernels.h"
#include "philox.h"
#include "tile_blend.h"

namespace {

// Philox counter of quad i of a [B][H][W] batch.  Default: the quad index itself.  With a tile map (full-domain tiling,
// SURVEY.md 8f rank 3) the counter is the quad's position in the DOMAIN, so pixels that several overlapping tiles share
// receive the same draw in every tile and the tiles stay consistent where they are blended.
__device__ __forceinline__ unsigned long long noise_index(const NoiseMap& m, size_t i) {
    if (!m.origins) return i;
    const size_t per4 = (size_t)m.tile_h * m.tile_w4;
    const size_t b = i / per4, rem = i - b * per4;
    const size_t y = rem / m.tile_w4, x4 = rem - y * m.tile_w4;
    return ((unsigned long long)(m.origins[2 * b] + y)) * m.dom_w4 + (unsigned long long)(m.origins[2 * b + 1] >> 2) + x4;
}

// z + w x (lag 0: w x, the product itself and not 0 + product, which would lose the sign of a zero) with the product and the sum rounded
// separately: contraction is switched off for this body (HIP's __fmul_rn / __fadd_rn are plain operators and would be fused)
__device__ __forceinline__ float mix_lag(float z, float w, float x, bool first) {
#pragma clang fp contract(off)
    const float p = w * x;
    return first ? p : z + p;
}
// The draw of a noise plan at quad i (kernels.h: NoiseMap): with r the row of the quad's sample and q its place within the sample,
// z = w[0] xi_0, then z = z + w[k] xi_k in ascending k, xi_k = the white draw at counter (r - k stride) per4 + q in 64-bit unsigned
// arithmetic.  Each product and sum is an fp32 operation of its own (no contraction), so a float32 loop over the white draws gives the
// same bits.  The trip count is uniform over the launch and the loop stays a loop: one Philox state is live at a time.
// With origins (the domain plan) the ONE row rows[0] serves every tile, per4 is the domain's quad count and q the quad's domain position.
__device__ __forceinline__ f32x4 philox_rows_normal4(unsigned long long seed, unsigned long long off, const NoiseMap& m, size_t i) {
    unsigned long long r, q;
    if (m.origins) {
        r = (unsigned long long)m.rows[0];
        q = noise_index(m, i);
    } else {
        const unsigned long long b = i / m.per4;
        r = (unsigned long long)m.rows[b];
        q = i - b * m.per4;
    }
    unsigned long long c = r * m.per4 + q;
    const unsigned long long back = (unsigned long long)m.stride * m.per4;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int k = 0; k < m.lags; ++k, c -= back) {
        const f32x4 xk = philox_normal4(seed, off, c);
        const float wk = m.w[k];
        for (int l = 0; l < 4; ++l) acc[l] = mix_lag(acc[l], wk, xk[l], k == 0);
    }
    return acc;
}

// The N(0,1) quad an update kernel uses at quad i: the injected draw, the plan's mixed draw, or the plain / domain-keyed Philox draw
__device__ __forceinline__ f32x4 noise4(const float* __restrict__ z, unsigned long long seed, unsigned long long off, const NoiseMap& m,
                                        size_t i) {
    if (z) return reinterpret_cast<const f32x4*>(z)[i];
    if (m.rows) return philox_rows_normal4(seed, off, m, i);
    return philox_normal4(seed, off, noise_index(m, i));
}

// Constrained sampling: hold(v, target, m) is a select with a soft edge.  m <= 0 keeps v and m >= 1 takes target, both
// bit-exactly (the other operand is never combined arithmetically, so `known` may hold anything where the mask is 0); in between
// (1-m) v + m target.  The mask is clamped to [0,1] here; a NaN mask counts as 0.
__device__ __forceinline__ f32x4 clamp_mask(f32x4 m) {
    for (int k = 0; k < 4; ++k) m[k] = fminf(fmaxf(m[k], 0.f), 1.f);
    return m;
}
__device__ __forceinline__ f32x4 hold4(f32x4 v, f32x4 target, f32x4 m) {
    f32x4 r;
    for (int k = 0; k < 4; ++k) r[k] = m[k] <= 0.f ? v[k] : m[k] >= 1.f ? target[k] : (1.f - m[k]) * v[k] + m[k] * target[k];
    return r;
}
__device__ __forceinline__ f32x4 load_mask(const Hold& h, size_t i) { return clamp_mask(reinterpret_cast<const f32x4*>(h.mask)[i]); }
__device__ __forceinline__ f32x4 load_known(const Hold& h, size_t i) { return reinterpret_cast<const f32x4*>(h.known)[i]; }
// draw 0 of the run (the initial state's noise) at quad i: the injected one, or recomputed from (seed, offset 0, counter or plan)
__device__ __forceinline__ f32x4 draw0(const Hold& h, unsigned long long seed, size_t i) { return noise4(h.z0, seed, 0ull, h.nm, i); }

// the score an update kernel uses at quad i: as stored, or (JOINT) the blend of all tiles' scores at the quad's domain position
template <bool JOINT>
__device__ __forceinline__ f32x4 load_score(const float* __restrict__ score, size_t i, const JointMap& jm) {
    if (JOINT) return joint_score4(score, jm, i);
    return reinterpret_cast<const f32x4*>(score)[i];
}

// tbrun <- row `row` of the run's time rows, the same row for every sample.  A thread loads ONE quad of the row (its vector is found by
// comparing against the n starts, unrolled so that they stay in scalar registers) and then only stores: to that quad's place in the
// samples g, g + G, ... of tbrun [n][BE][ch_i], G = the groups of TB / 4 threads the workgroup holds.  The stores of a wave are
// consecutive quads of one sample's vector, and none waits for a load (a load - store pair per iteration made this 7 us at C2).
__device__ __forceinline__ void bcast_time_row(const TimeRows& tr, unsigned long long row, int tid, int nthreads) {
    const int tb4 = tr.off4[tr.n];
    const f32x4* __restrict__ src = reinterpret_cast<const f32x4*>(tr.rows) + (size_t)row * tb4;
    f32x4* __restrict__ dst = reinterpret_cast<f32x4*>(tr.tbrun);
    const int G = nthreads >= tb4 ? nthreads / tb4 : 1;
    const int g = tid / tb4;
    if (g >= G) return;
    for (int q = tid - g * tb4; q < tb4; q += nthreads) {        // one pass when the workgroup has at least TB / 4 threads
        int lo = 0, ch4 = tr.off4[1];
#pragma unroll
        for (int k = 1; k < 16; ++k)
            if (k < tr.n && q >= tr.off4[k]) { lo = tr.off4[k]; ch4 = tr.off4[k + 1] - tr.off4[k]; }
        const f32x4 v = src[q];
        f32x4* d = dst + (size_t)lo * tr.BE + (q - lo);
        for (int b = g; b < tr.BE; b += G) d[(size_t)b * ch4] = v;
    }
}
__global__ __launch_bounds__(1024) void time_rows_bcast_kernel(TimeRows tr, int row) { bcast_time_row(tr, row, threadIdx.x, blockDim.x); }

__global__ void fill_kernel(float* t, float v, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) t[i] = v;
}

// x = scale * N(0,1)   (sampler start: randn * marginal_prob_std(1), score_sampling.py:94-95, :168);  HELD: + m * known where m > 0
template <bool HELD>
__global__ __launch_bounds__(256) void init_noise_kernel(float* __restrict__ x, float scale, const float* __restrict__ z,
                                                         unsigned long long seed, const SamplerState* __restrict__ state,
                                                         unsigned long long off_val, size_t n4, NoiseMap nm, Hold hold) {
    const unsigned long long off = state ? state->rng_offset : off_val;
    if (state) seed = state->seed;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const f32x4 n = noise4(z, seed, off, nm, i);
        f32x4 v = n * scale;
        if (HELD) {
            const f32x4 m = load_mask(hold, i), kn = load_known(hold, i);
            for (int k = 0; k < 4; ++k) v[k] = m[k] <= 0.f ? v[k] : v[k] + m[k] * kn[k];
        }
        reinterpret_cast<f32x4*>(x)[i] = v;
    }
}

// x_mean = x + g^2 dt * score ;  x = x_mean + noise_coef * N(0,1);  HELD: x_mean = hold(., known), x = hold(., known + std(t_next) z)
// with the step's own draw z (the unheld branch discards it on a held pixel, so it is a fresh draw there);  JOINT (here and in the four
// kernels below): `score` is read through the tile blend, everything else is unchanged and the hold sees the blended update
template <bool HELD, bool JOINT>
__global__ __launch_bounds__(256) void em_update_kernel(float* __restrict__ x, float* __restrict__ x_mean,
                                                        const float* __restrict__ score, const float* __restrict__ z,
                                                        const StepScalars* __restrict__ table,
                                                        const SamplerState* __restrict__ state, StepScalars sc_val,
                                                        unsigned long long off_val, unsigned long long seed, size_t n4,
                                                        NoiseMap nm, Hold hold, JointMap jm) {
    const StepScalars sc = state ? table[state->step] : sc_val;
    const float s_next = !HELD ? 0.f : (state ? hold.levels[state->step] : hold.lv).next;
    const unsigned long long off = state ? state->rng_offset : off_val;
    if (state) seed = state->seed;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const f32x4 xv = reinterpret_cast<const f32x4*>(x)[i];
        const f32x4 sv = load_score<JOINT>(score, i, jm);
        const f32x4 n = noise4(z, seed, off, nm, i);
        const f32x4 mean = xv + (sc.g2 * sv) * sc.dt;   // association of score_sampling.py:124/:224
        if (HELD) {
            const f32x4 m = load_mask(hold, i), kn = load_known(hold, i);
            reinterpret_cast<f32x4*>(x_mean)[i] = hold4(mean, kn, m);
            reinterpret_cast<f32x4*>(x)[i] = hold4(mean + sc.noise * n, kn + s_next * n, m);
        } else {
            reinterpret_cast<f32x4*>(x_mean)[i] = mean;
            reinterpret_cast<f32x4*>(x)[i] = mean + sc.noise * n;
        }
    }
}

// runs after the update kernel of a step: advance the step counter / RNG offset, publish the next time
// and, for a run that keeps its time rows (tr.rows set), the next step's time biases: only the advance that moves the step publishes
// them (the corrector's does not), and the last step republishes its own row
__global__ void advance_kernel(SamplerState* state, const StepScalars* table, float* t_dev, int B, int advance_step,
                               int n_steps, TimeRows tr) {
    const unsigned long long s = state->step;
    const unsigned long long ns = state->n_steps ? state->n_steps : (unsigned long long)n_steps;
    const unsigned long long nxt = sampler_next_step(s, ns);
    const int i = threadIdx.x;
    if (advance_step && t_dev && i < B) t_dev[i] = table[s].t_next;
    if (advance_step && tr.rows) bcast_time_row(tr, nxt, i, blockDim.x);
    __syncthreads();
    if (i == 0) {
        state->rng_offset += 1;
        if (advance_step) state->step = nxt;
    }
}

// per-sample sum of squares of the score, fp64 atomics into sumsq[B] (zeroed by the launcher): ONE atomic per workgroup (the four
// wave sums meet in LDS first) and at most 16 workgroups per sample — same-address fp64 atomics retire at ~10 ns each, and one per wave
// of a 64 x B grid made this 4 MB reduction a 41 us kernel at B = 16, 256 x 256
__global__ __launch_bounds__(256) void sumsq_kernel(const float* __restrict__ score, double* __restrict__ sumsq,
                                                    size_t per_sample4) {
    __shared__ double part[4];
    const int b = blockIdx.y;
    const f32x4* s = reinterpret_cast<const f32x4*>(score) + (size_t)b * per_sample4;
    float acc = 0.f;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < per_sample4; i += (size_t)gridDim.x * blockDim.x) {
        const f32x4 v = s[i];
        acc += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
    }
    const double w = wave_sum_d((double)acc);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(&sumsq[b], (part[0] + part[1]) + (part[2] + part[3]));
}

// Langevin corrector: eps = 2 (snr*sqrt(CHW) / mean_b ||score_b||)^2 ;  x += eps*score + sqrt(2 eps) N(0,1)
// Tile mode (nm.origins set: the samples are tiles of one domain): the step size of a tile uses that tile's OWN score norm
// instead of the batch mean, so a tile's trajectory does not depend on which other tiles share its batch or its GPU
// (the reference has no tiler, its batch-mean rule :201 applies to batches of independent samples).
// HELD: x = hold(., known + std(t_i) z); the score norm stays over the whole sample.
// JOINT: all tiles of the domain are in the batch, so the reference's batch-mean rule over the RAW tile scores is well defined and gives
// ONE step size for the domain (copies of a pixel keep the same noise amplitude); the per-tile norm is not used.
template <bool HELD, bool JOINT>
__global__ __launch_bounds__(256) void langevin_kernel(float* __restrict__ x, const float* __restrict__ score,
                                                       const float* __restrict__ z, float snr_noise_norm,
                                                       const double* __restrict__ sumsq,
                                                       const SamplerState* __restrict__ state,
                                                       unsigned long long off_val, unsigned long long seed, int B,
                                                       size_t n4, NoiseMap nm, Hold hold, JointMap jm) {
    const float s_cur = !HELD ? 0.f : (state ? hold.levels[state->step] : hold.lv).cur;
    float gn = 0.f;
    for (int b = 0; b < B; ++b) gn += (float)sqrt(sumsq[b]);
    gn /= (float)B;
    const float r = snr_noise_norm / gn;
    float eps = 2.f * (r * r);
    float nz = sqrtf(2.f * eps);
    const bool per_tile = !JOINT && nm.origins != nullptr;
    const size_t per4 = n4 / (size_t)B;
    const unsigned long long off = state ? state->rng_offset : off_val;
    if (state) seed = state->seed;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        if (per_tile) {
            // a tile whose score is exactly zero (masked / constant tile) would get eps = inf and poison the stitched domain
            const float rt = snr_noise_norm / fmaxf((float)sqrt(sumsq[i / per4]), 1e-12f);
            eps = 2.f * (rt * rt);
            nz = sqrtf(2.f * eps);
        }
        const f32x4 xv = reinterpret_cast<const f32x4*>(x)[i];
        const f32x4 sv = load_score<JOINT>(score, i, jm);
        const f32x4 n = noise4(z, seed, off, nm, i);
        const f32x4 v = xv + eps * sv + nz * n;
        reinterpret_cast<f32x4*>(x)[i] = HELD ? hold4(v, load_known(hold, i) + s_cur * n, load_mask(hold, i)) : v;
    }
}

__global__ __launch_bounds__(256) void cfg_combine_kernel(float* __restrict__ out, const float* __restrict__ sc,
                                                          const float* __restrict__ su, float w, size_t n4) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const f32x4 a = reinterpret_cast<const f32x4*>(sc)[i], b = reinterpret_cast<const f32x4*>(su)[i];
        reinterpret_cast<f32x4*>(out)[i] = (1.0f + w) * a - w * b;
    }
}

// EDM Heun step, split around its two network evaluations (the step table row is picked by the device step counter when
// a state is given, so one captured graph serves every step; by value otherwise).
// churn: x_hat = x + churn_coef * z, written to x and to the network-input slab
__global__ __launch_bounds__(256) void edm_churn_kernel(float* __restrict__ x, float* __restrict__ x_copy,
                                                        const float* __restrict__ z, const EdmStep* __restrict__ table,
                                                        const SamplerState* __restrict__ state, EdmStep sc_val,
                                                        unsigned long long off_val, unsigned long long seed, size_t n4,
                                                        NoiseMap nm) {
    const float c = (state ? table[state->step] : sc_val).churn_coef;
    const unsigned long long off = state ? state->rng_offset : off_val;
    if (state) seed = state->seed;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const f32x4 n = noise4(z, seed, off, nm, i);
        const f32x4 v = reinterpret_cast<const f32x4*>(x)[i] + c * n;
        reinterpret_cast<f32x4*>(x)[i] = v;
        if (x_copy) reinterpret_cast<f32x4*>(x_copy)[i] = v;
    }
}

// Euler predictor: d = dx/dsigma = -sigma_hat * score ; x' = x_hat + (sigma_next - sigma_hat) * d.  The time vector of the
// second evaluation (t_next) is published by the same launch: nothing reads it until the next kernel.
// HELD (here and in the Heun corrector): a held pixel follows the probability-flow trajectory of a point mass, known + sigma z0 with
// the run's own draw 0, so the output is hold(., known + sigma_next z0): deterministic, and `known` itself after the last step.
template <bool HELD, bool JOINT>
__global__ __launch_bounds__(256) void edm_euler_kernel(const float* __restrict__ x_hat, const float* __restrict__ score,
                                                        float* __restrict__ d, float* __restrict__ x_next,
                                                        const EdmStep* __restrict__ table, const SamplerState* __restrict__ state,
                                                        EdmStep sc_val, float* __restrict__ t_dev, int t_entries, size_t n4,
                                                        Hold hold, JointMap jm) {
    const EdmStep sc = state ? table[state->step] : sc_val;
    const unsigned long long seed = state ? state->seed : hold.seed;
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    if (t_dev)
        for (size_t j = gid; j < (size_t)t_entries; j += stride) t_dev[j] = sc.t_next;
    const float h = sc.sigma_next - sc.sigma_hat;
    for (size_t i = gid; i < n4; i += stride) {
        const f32x4 dv = (-sc.sigma_hat) * load_score<JOINT>(score, i, jm);
        reinterpret_cast<f32x4*>(d)[i] = dv;
        const f32x4 v = reinterpret_cast<const f32x4*>(x_hat)[i] + h * dv;
        reinterpret_cast<f32x4*>(x_next)[i] =
            HELD ? hold4(v, load_known(hold, i) + sc.sigma_next * draw0(hold, seed, i), load_mask(hold, i)) : v;
    }
}

// Heun corrector: x = x_hat + (sigma_next - sigma_hat) * 0.5 (d + d'), d' = -sigma_next * score(x', sigma_next); in place over
// x_hat, mirrored into the network-input slab.  Publishes the first evaluation time of the next step (the advance follows).
template <bool HELD, bool JOINT>
__global__ __launch_bounds__(256) void edm_heun_kernel(float* __restrict__ x, float* __restrict__ x_copy,
                                                       const float* __restrict__ d, const float* __restrict__ score,
                                                       const EdmStep* __restrict__ table, const SamplerState* __restrict__ state,
                                                       EdmStep sc_val, float* __restrict__ t_dev, int t_entries, int n_steps,
                                                       size_t n4, Hold hold, JointMap jm) {
    const unsigned long long s = state ? state->step : 0ull;
    const unsigned long long seed = state ? state->seed : hold.seed;
    const EdmStep sc = state ? table[s] : sc_val;
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    if (state && t_dev) {
        const unsigned long long ns = state->n_steps ? state->n_steps : (unsigned long long)n_steps;
        const float tn = table[s + 1 < ns ? s + 1 : s].t_hat;
        for (size_t j = gid; j < (size_t)t_entries; j += stride) t_dev[j] = tn;
    }
    const float h = sc.sigma_next - sc.sigma_hat;
    for (size_t i = gid; i < n4; i += stride) {
        const f32x4 d2 = (-sc.sigma_next) * load_score<JOINT>(score, i, jm);
        f32x4 v = reinterpret_cast<const f32x4*>(x)[i] + (h * 0.5f) * (reinterpret_cast<const f32x4*>(d)[i] + d2);
        if (HELD) v = hold4(v, load_known(hold, i) + sc.sigma_next * draw0(hold, seed, i), load_mask(hold, i));
        reinterpret_cast<f32x4*>(x)[i] = v;
        if (x_copy) reinterpret_cast<f32x4*>(x_copy)[i] = v;
    }
}

// DPM-Solver++(2M) step (kernels.h: DpmStep): D = x + sigma^2 score; x = c_x x + c_0 D + c_1 hist + c_z z; hist = D.  One evaluation per
// step: the second-order term is the previous step's D, read and rewritten at the same index by the same thread.  The history is NOT read
// when c_1 == 0 (step 0 finds whatever the workspace held there, and 0 * NaN would poison the run); the draw is taken only in a
// stochastic run.  Publishes the time of the next step's evaluation (the advance follows).
// HELD: x = hold(., known + sigma_{i+1} z) with the step's own draw in a stochastic run (the EM / PC convention), else with the run's
// draw 0 (the point-mass trajectory, as in EDM Heun); sigma_N = 0, so the result is `known` itself.  The history is not held.
template <bool HELD, bool JOINT>
__global__ __launch_bounds__(256) void dpmpp_2m_kernel(float* __restrict__ x, float* __restrict__ x_copy, const float* __restrict__ score,
                                                       float* __restrict__ hist, const float* __restrict__ z,
                                                       const DpmStep* __restrict__ table, const SamplerState* __restrict__ state,
                                                       DpmStep sc_val, unsigned long long off_val, unsigned long long seed,
                                                       int stochastic, float* __restrict__ t_dev, int t_entries, size_t n4,
                                                       NoiseMap nm, Hold hold, JointMap jm) {
    const DpmStep sc = state ? table[state->step] : sc_val;
    const float s_next = !HELD ? 0.f : (state ? hold.levels[state->step] : hold.lv).next;
    const unsigned long long off = state ? state->rng_offset : off_val;
    if (state) seed = state->seed;
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    if (t_dev)
        for (size_t j = gid; j < (size_t)t_entries; j += stride) t_dev[j] = sc.t_next;
    const float sig2 = sc.sigma * sc.sigma;
    const bool second = sc.c_1 != 0.f;
    for (size_t i = gid; i < n4; i += stride) {
        const f32x4 xv = reinterpret_cast<const f32x4*>(x)[i];
        const f32x4 dv = xv + sig2 * load_score<JOINT>(score, i, jm);
        f32x4 v = sc.c_x * xv + sc.c_0 * dv;
        if (second) v = v + sc.c_1 * reinterpret_cast<const f32x4*>(hist)[i];
        f32x4 n = {0.f, 0.f, 0.f, 0.f};
        if (stochastic) {
            n = noise4(z, seed, off, nm, i);
            v = v + sc.c_z * n;
        }
        if (HELD) {
            if (!stochastic) n = draw0(hold, seed, i);
            v = hold4(v, load_known(hold, i) + s_next * n, load_mask(hold, i));
        }
        reinterpret_cast<f32x4*>(x)[i] = v;
        if (x_copy) reinterpret_cast<f32x4*>(x_copy)[i] = v;
        reinterpret_cast<f32x4*>(hist)[i] = dv;
    }
}

// The hold as an op of its own, for loops that run the network themselves: x = hold(x, known + level z, m) and, when given,
// x_mean = hold(x_mean, known, m); z null -> the Philox draw (seed, draw_index) the preceding step op consumed.
__global__ __launch_bounds__(256) void hold_known_kernel(float* __restrict__ x, float* __restrict__ x_mean, const float* __restrict__ z,
                                                         float level, unsigned long long seed, unsigned long long off, size_t n4,
                                                         Hold hold) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const f32x4 n = z ? reinterpret_cast<const f32x4*>(z)[i] : philox_normal4(seed, off, i);
        const f32x4 m = load_mask(hold, i), kn = load_known(hold, i);
        reinterpret_cast<f32x4*>(x)[i] = hold4(reinterpret_cast<const f32x4*>(x)[i], kn + level * n, m);
        if (x_mean) reinterpret_cast<f32x4*>(x_mean)[i] = hold4(reinterpret_cast<const f32x4*>(x_mean)[i], kn, m);
    }
}

// the held or the plain instantiation of a kernel template, by whether the call carries a constraint
#define SBGM_LAUNCH_HELD(kernel, held, grid, st, ...)                                                   \
    do {                                                                                                \
        if (held) hipLaunchKernelGGL((kernel<true>), grid, dim3(256), 0, st, __VA_ARGS__);              \
        else hipLaunchKernelGGL((kernel<false>), grid, dim3(256), 0, st, __VA_ARGS__);                  \
    } while (0)
// ... and of the five update kernels, which also come with and without the joint tile blend
#define SBGM_LAUNCH_STEP(kernel, held, joint, grid, st, ...)                                            \
    do {                                                                                                \
        if (joint) {                                                                                    \
            if (held) hipLaunchKernelGGL((kernel<true, true>), grid, dim3(256), 0, st, __VA_ARGS__);    \
            else hipLaunchKernelGGL((kernel<false, true>), grid, dim3(256), 0, st, __VA_ARGS__);        \
        } else {                                                                                        \
            if (held) hipLaunchKernelGGL((kernel<true, false>), grid, dim3(256), 0, st, __VA_ARGS__);   \
            else hipLaunchKernelGGL((kernel<false, false>), grid, dim3(256), 0, st, __VA_ARGS__);       \
        }                                                                                               \
    } while (0)
// a joint launch blends over the whole batch: its map must describe exactly the launch's [B][H][W]
inline int check_joint(const JointMap& jm, size_t n, const char* who) {
    if (!jm.origins) return 0;
    SBGM_CHECK(jm.T >= 1 && jm.tile_h >= 1 && jm.tile_w >= 4 && jm.tile_w % 4 == 0 && jm.R >= 1 &&
               (size_t)jm.T * jm.tile_h * jm.tile_w == n, "%s: the joint tile map (%d tiles of %d x %d, ramp %d) does not match %zu elements",
               who, jm.T, jm.tile_h, jm.tile_w, jm.R, n);
    return 0;
}
// a noise plan must describe exactly the launch's n elements (the kernel reads rows[quad / per4]); with a tile map it is the domain plan
// (the kernel reads rows[0] and origins[tile]): whole tiles, and a domain of whole quad rows that is at least a tile high;
// checked on the map a kernel reads: `nm` for its own draw, `hold.nm` where it recomputes the run's draw 0 (edm_euler, edm_heun, dpmpp_2m)
inline int check_noise(const NoiseMap& nm, size_t n, const char* who) {
    if (!nm.rows) return 0;
    SBGM_CHECK(nm.lags >= 1 && nm.lags <= SBGM_NOISE_MAX_LAGS && nm.stride >= 1, "%s: noise rows need 1 <= lags <= %d and stride >= 1 "
               "(lags=%d, stride=%d)", who, SBGM_NOISE_MAX_LAGS, nm.lags, nm.stride);
    if (nm.origins) {
        SBGM_CHECK(nm.tile_h >= 1 && nm.tile_w4 >= 1 && nm.dom_w4 >= nm.tile_w4 && (n / 4) % ((size_t)nm.tile_h * nm.tile_w4) == 0 &&
                   nm.per4 % (unsigned long long)nm.dom_w4 == 0 && nm.per4 >= (unsigned long long)nm.tile_h * nm.dom_w4,
                   "%s: a domain noise row over %llu quads does not fit tiles of %d x %d quads in rows of %d quads (%zu elements)", who,
                   nm.per4, nm.tile_h, nm.tile_w4, nm.dom_w4, n);
        return 0;
    }
    SBGM_CHECK(nm.per4 >= 1 && (n / 4) % nm.per4 == 0, "%s: noise rows over samples of %llu quads do not divide %zu elements", who, nm.per4, n);
    return 0;
}
inline int check_hold(const Hold& h, const char* who) {
    SBGM_CHECK((h.known == nullptr) == (h.mask == nullptr), "%s: known and known_mask must be given together", who);
    return 0;
}

// a usable time-row descriptor: 1..16 vectors of whole quads in increasing order, at least one sample
inline int check_time_rows(const TimeRows& tr) {
    if (!tr.rows || !tr.tbrun || tr.n < 1 || tr.n > 16 || tr.BE < 1 || tr.off4[0] != 0) return 1;
    for (int i = 0; i < tr.n; ++i) if (tr.off4[i + 1] <= tr.off4[i]) return 1;
    return 0;
}

inline int stream_blocks(size_t n) { return (int)std::min<size_t>((n + 255) / 256, 2048); }

}  // namespace

int sbgm_launch_time_rows_bcast(const TimeRows& tr, int row, hipStream_t st) {
    SBGM_CHECK(check_time_rows(tr) == 0 && row >= 0, "time_rows_bcast: bad time-row layout");
    hipLaunchKernelGGL(time_rows_bcast_kernel, dim3(1), dim3(1024), 0, st, tr, row);
    SBGM_LAUNCH_CHECK();
    return 0;
}

int sbgm_launch_fill_t(float* t, float value, int B, hipStream_t st) {
    hipLaunchKernelGGL(fill_kernel, dim3((B + 255) / 256), dim3(256), 0, st, t, value, B);
    SBGM_LAUNCH_CHECK();
    return 0;
}

int sbgm_launch_init_noise(float* x, float scale, const float* z, unsigned long long seed, SamplerState* state,
                           unsigned long long draw_index, size_t n, hipStream_t st, NoiseMap nm, const Hold& hold) {
    SBGM_CHECK(n % 4 == 0, "init_noise: element count must be a multiple of 4");
    if (check_hold(hold, "init_noise") || check_noise(nm, n, "init_noise")) return 1;
    SBGM_LAUNCH_HELD(init_noise_kernel, hold.known != nullptr, dim3(stream_blocks(n / 4)), st, x, scale, z, seed, state, draw_index,
                     n / 4, nm, hold);
    SBGM_LAUNCH_CHECK();
    if (state) {
        hipLaunchKernelGGL(advance_kernel, dim3(1), dim3(64), 0, st, state, (const StepScalars*)nullptr, (float*)nullptr, 0, 0, 0, TimeRows{});
        SBGM_LAUNCH_CHECK();
    }
    return 0;
}

int sbgm_launch_em_update(float* x, float* x_mean, const float* score, const float* z, const StepScalars* table,
                          SamplerState* state, const StepScalars* sc_val, unsigned long long draw_index, float* t_dev,
                          unsigned long long seed, int B, size_t per_sample, int n_steps, hipStream_t st, int t_entries,
                          NoiseMap nm, const Hold& hold, const JointMap& jm, const TimeRows& tr) {
    const size_t n = (size_t)B * per_sample;
    if (t_entries <= 0) t_entries = B;
    SBGM_CHECK(n % 4 == 0, "em_update: element count must be a multiple of 4");
    SBGM_CHECK(t_entries <= 1024, "em_update: %d time entries > 1024", t_entries);
    SBGM_CHECK(state != nullptr || sc_val != nullptr, "em_update: need a device table or explicit scalars");
    SBGM_CHECK(!(hold.known && state && !hold.levels), "em_update: a held run with a device state needs the hold-level table");
    SBGM_CHECK(!tr.rows || (state && check_time_rows(tr) == 0), "em_update: time rows need a device state and a valid layout");
    if (check_hold(hold, "em_update") || check_noise(nm, n, "em_update") || check_joint(jm, n, "em_update")) return 1;
    const StepScalars v = sc_val ? *sc_val : StepScalars{};
    SBGM_LAUNCH_STEP(em_update_kernel, hold.known != nullptr, jm.origins != nullptr, dim3(stream_blocks(n / 4)), st, x, x_mean, score, z,
                     table, state, v, draw_index, seed, n / 4, nm, hold, jm);
    SBGM_LAUNCH_CHECK();
    if (state) {
        hipLaunchKernelGGL(advance_kernel, dim3(1), dim3(1024), 0, st, state, table, t_dev, t_entries, 1, n_steps, tr);
        SBGM_LAUNCH_CHECK();
    }
    return 0;
}

int sbgm_launch_langevin(float* x, const float* score, const float* z, float snr_noise_norm, double* sumsq_ws,
                         SamplerState* state, unsigned long long draw_index, unsigned long long seed, int B,
                         size_t per_sample, hipStream_t st, NoiseMap nm, const Hold& hold, const JointMap& jm) {
    SBGM_CHECK(per_sample % 4 == 0, "langevin: per-sample element count must be a multiple of 4");
    SBGM_CHECK(!(hold.known && state && !hold.levels), "langevin: a held run with a device state needs the hold-level table");
    if (check_hold(hold, "langevin") || check_noise(nm, (size_t)B * per_sample, "langevin") ||
        check_joint(jm, (size_t)B * per_sample, "langevin")) return 1;
    { if (sbgm_zero_async(sumsq_ws, sizeof(double) * B, st)) return 1; }
    const int bx = (int)std::min<size_t>((per_sample / 4 + 255) / 256, B >= 64 ? 4 : 16);
    hipLaunchKernelGGL(sumsq_kernel, dim3(bx, B), dim3(256), 0, st, score, sumsq_ws, per_sample / 4);
    SBGM_LAUNCH_CHECK();
    const size_t n4 = (size_t)B * per_sample / 4;
    SBGM_LAUNCH_STEP(langevin_kernel, hold.known != nullptr, jm.origins != nullptr, dim3(stream_blocks(n4)), st, x, score, z,
                     snr_noise_norm, sumsq_ws, state, draw_index, seed, B, n4, nm, hold, jm);
    SBGM_LAUNCH_CHECK();
    if (state) {
        hipLaunchKernelGGL(advance_kernel, dim3(1), dim3(64), 0, st, state, (const StepScalars*)nullptr, (float*)nullptr, 0, 0, 0, TimeRows{});
        SBGM_LAUNCH_CHECK();
    }
    return 0;
}

int sbgm_launch_edm_churn(float* x, float* x_copy, const float* z, const EdmStep* table, const SamplerState* state,
                          const EdmStep* sc_val, unsigned long long draw_index, unsigned long long seed, size_t n, hipStream_t st,
                          NoiseMap nm) {
    SBGM_CHECK(n % 4 == 0, "edm_churn: element count must be a multiple of 4");
    SBGM_CHECK(state != nullptr || sc_val != nullptr, "edm_churn: need a device table or explicit scalars");
    if (check_noise(nm, n, "edm_churn")) return 1;
    const EdmStep v = sc_val ? *sc_val : EdmStep{};
    hipLaunchKernelGGL(edm_churn_kernel, dim3(stream_blocks(n / 4)), dim3(256), 0, st, x, x_copy, z, table, state, v, draw_index,
                       seed, n / 4, nm);
    SBGM_LAUNCH_CHECK();
    return 0;
}

int sbgm_launch_edm_euler(const float* x_hat, const float* score, float* d, float* x_next, const EdmStep* table,
                          const SamplerState* state, const EdmStep* sc_val, float* t_dev, int t_entries, size_t n, hipStream_t st,
                          const Hold& hold, const JointMap& jm) {
    SBGM_CHECK(n % 4 == 0, "edm_euler: element count must be a multiple of 4");
    if (check_hold(hold, "edm_euler") || check_noise(hold.nm, n, "edm_euler") || check_joint(jm, n, "edm_euler")) return 1;
    SBGM_CHECK(state != nullptr || sc_val != nullptr, "edm_euler: need a device table or explicit scalars");
    const EdmStep v = sc_val ? *sc_val : EdmStep{};
    SBGM_LAUNCH_STEP(edm_euler_kernel, hold.known != nullptr, jm.origins != nullptr, dim3(stream_blocks(n / 4)), st, x_hat, score, d,
                     x_next, table, state, v, t_dev, t_dev ? t_entries : 0, n / 4, hold, jm);
    SBGM_LAUNCH_CHECK();
    return 0;
}

int sbgm_launch_edm_heun(float* x, float* x_copy, const float* d, const float* score, const EdmStep* table, SamplerState* state,
                         const EdmStep* sc_val, float* t_dev, int t_entries, int n_steps, size_t n, hipStream_t st, const Hold& hold,
                         const JointMap& jm) {
    SBGM_CHECK(n % 4 == 0, "edm_heun: element count must be a multiple of 4");
    if (check_hold(hold, "edm_heun") || check_noise(hold.nm, n, "edm_heun") || check_joint(jm, n, "edm_heun")) return 1;
    SBGM_CHECK(state != nullptr || sc_val != nullptr, "edm_heun: need a device table or explicit scalars");
    const EdmStep v = sc_val ? *sc_val : EdmStep{};
    SBGM_LAUNCH_STEP(edm_heun_kernel, hold.known != nullptr, jm.origins != nullptr, dim3(stream_blocks(n / 4)), st, x, x_copy, d, score,
                     table, state, v, t_dev, t_dev ? t_entries : 0, n_steps, n / 4, hold, jm);
    SBGM_LAUNCH_CHECK();
    if (state) {                     // step counter and RNG offset: the EM mechanism, without its StepScalars time publish
        hipLaunchKernelGGL(advance_kernel, dim3(1), dim3(64), 0, st, state, (const StepScalars*)nullptr, (float*)nullptr, 0, 1, n_steps, TimeRows{});
        SBGM_LAUNCH_CHECK();
    }
    return 0;
}

int sbgm_launch_dpmpp_2m(float* x, float* x_copy, const float* score, float* hist, const float* z, const DpmStep* table,
                         SamplerState* state, const DpmStep* sc_val, unsigned long long draw_index, unsigned long long seed,
                         int stochastic, float* t_dev, int t_entries, int n_steps, size_t n, hipStream_t st, NoiseMap nm,
                         const Hold& hold, const JointMap& jm, const TimeRows& tr) {
    SBGM_CHECK(n % 4 == 0, "dpmpp_2m: element count must be a multiple of 4");
    SBGM_CHECK(x && score && hist, "dpmpp_2m: x, score and the history slab are required");
    SBGM_CHECK(state ? table != nullptr : sc_val != nullptr, "dpmpp_2m: need a device table with a state, or explicit scalars");
    SBGM_CHECK(!(z && !stochastic), "dpmpp_2m: a deterministic step takes no draw");
    SBGM_CHECK(!(hold.known && state && !hold.levels), "dpmpp_2m: a held run with a device state needs the hold-level table");
    SBGM_CHECK(!tr.rows || (state && check_time_rows(tr) == 0), "dpmpp_2m: time rows need a device state and a valid layout");
    if (check_hold(hold, "dpmpp_2m") || check_noise(nm, n, "dpmpp_2m") || check_noise(hold.nm, n, "dpmpp_2m") ||
        check_joint(jm, n, "dpmpp_2m")) return 1;
    const DpmStep v = sc_val ? *sc_val : DpmStep{};
    SBGM_LAUNCH_STEP(dpmpp_2m_kernel, hold.known != nullptr, jm.origins != nullptr, dim3(stream_blocks(n / 4)), st, x, x_copy, score,
                     hist, z, table, state, v, draw_index, seed, stochastic, t_dev, t_dev ? t_entries : 0, n / 4, nm, hold, jm);
    SBGM_LAUNCH_CHECK();
    if (state) {                     // step counter and RNG offset; a run that keeps its time rows publishes the next step's row here
        hipLaunchKernelGGL(advance_kernel, dim3(1), dim3(tr.rows ? 1024 : 64), 0, st, state, (const StepScalars*)nullptr, (float*)nullptr,
                           0, 1, n_steps, tr);
        SBGM_LAUNCH_CHECK();
    }
    return 0;
}

int sbgm_launch_hold_known(float* x, float* x_mean, const float* z, float level, unsigned long long seed, unsigned long long draw_index,
                           size_t n, hipStream_t st, const Hold& hold) {
    SBGM_CHECK(n % 4 == 0, "hold_known: element count must be a multiple of 4");
    SBGM_CHECK(x && hold.known && hold.mask, "hold_known: x, known and known_mask are required");
    hipLaunchKernelGGL(hold_known_kernel, dim3(stream_blocks(n / 4)), dim3(256), 0, st, x, x_mean, z, level, seed, draw_index, n / 4,
                       hold);
    SBGM_LAUNCH_CHECK();
    return 0;
}

int sbgm_launch_cfg_combine(float* out, const float* s_cond, const float* s_uncond, float scale, size_t n, hipStream_t st) {
    SBGM_CHECK(n % 4 == 0, "cfg_combine: element count must be a multiple of 4");
    hipLaunchKernelGGL(cfg_combine_kernel, dim3(stream_blocks(n / 4)), dim3(256), 0, st, out, s_cond, s_uncond, scale, n / 4);
    SBGM_LAUNCH_CHECK();
    return 0;
}
