/* sbgm_hip.h — C ABI of libsbgm_hip.so: the MI355X (gfx950) implementation of the SBGM_DANRA score-UNet forward
 * and reverse-SDE sampling hot path.
 *
 * Boundary: this library sits between the reference's Python layer L1 (sbgm/score_unet.py, sbgm/score_sampling.py)
 * and what used to be torch.nn ops.  Plain pointers and sizes only; every pointer is a DEVICE pointer unless said
 * otherwise; every call enqueues on `stream` (a hipStream_t passed as void*) and returns without synchronising (the exceptions —
 * the tuning / profiling calls, a sampler's first call of a shape — say so where they are declared).
 * Return value: 0 = ok, non-zero = error (text via sbgm_last_error()).  The Python mirror raises RuntimeError.
 *
 * Tensor conventions at the boundary are the reference's: NCHW contiguous fp32, t float [B], y int64 [B] with
 * 0 = null class (reference score_unet.py:224-226).  Internally everything is NHWC; the *_nhwc per-op entry
 * points below expose that layout for unit parity tests.
 */
#ifndef SBGM_HIP_H
#define SBGM_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct sbgm_model sbgm_model;

const char* sbgm_last_error(void);
int sbgm_abi_version(void);

enum { SBGM_NONE = 0, SBGM_RELU = 1, SBGM_SILU = 2, SBGM_GELU = 3 };   /* activation codes */
enum { SBGM_NORM_INSTANCE = 0, SBGM_NORM_GROUP = 1 };
enum { SBGM_SAMPLER_EM = 0, SBGM_SAMPLER_PC = 1, SBGM_SAMPLER_EDM_HEUN = 2, SBGM_SAMPLER_RK45 = 3, SBGM_SAMPLER_DPMPP_2M = 4 };

/* ------------------------------------------------------------------------------------------------------------
 * Model handle.  Replaces: training_utils.get_model -> Encoder/Decoder/ScoreNet construction
 * (reference training_utils.py:645-666) + ScoreNet.forward (score_unet.py:829-879).
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct sbgm_model_config {
    int struct_size;         /* = sizeof(sbgm_model_config) of the header the CALLER was compiled against; sbgm_model_create
                                rejects any other value (a binding generated from an older header would otherwise be read past
                                its end).  First member, so the check never reads beyond 4 bytes of a foreign struct. */
    int n_lsm_channels;      /* 0 or 2: lsm_cond value||mask          (cat order: x, lsm, topo, cond_img; :273-291) */
    int n_topo_channels;     /* 0 or 2 */
    int n_cond_channels;     /* LR condition channels */
    int time_embedding;      /* cfg.sampler.time_embedding */
    int block_layers[4];     /* cfg.sampler.block_layers */
    int n_heads;             /* cfg.sampler.num_heads */
    int num_classes;         /* 0 = no label embedding, else n_seasons (table has num_classes+1 rows) */
    int last_fmap_channels;  /* cfg.sampler.last_fmap_channels (512) */
    int decoder_norm;        /* SBGM_NORM_* (cfg.model.decoder_norm) */
    int gn_groups;           /* cfg.model.decoder_gn_groups */
    int decoder_activation;  /* SBGM_RELU / SBGM_SILU / SBGM_GELU (cfg.model.decoder_activation) */
    float sigma;             /* VE-SDE sigma (25.0, score_unet.py:932) */
    int decoder_transpose;   /* 0: bilinear x2 + conv_up (default); 1: ConvTranspose2d(k=2, s=2) upsampling, the reference's
                                ablation path (cfg.model.use_resize_conv = false, score_unet.py:470-475, :589) */
} sbgm_model_config;

/* Fails (non-zero, text in sbgm_last_error) when cfg->struct_size != sizeof(sbgm_model_config) of this library. */
int sbgm_model_create(const sbgm_model_config* cfg, sbgm_model** out);
/* sizeof(sbgm_model_config) as this library was compiled: lets a binding check its own struct before the first call. */
int sbgm_model_config_size(void);
void sbgm_model_destroy(sbgm_model* m);

/* Number of state_dict entries the model expects, and the i-th entry's name / element count (host strings). */
int sbgm_model_num_params(const sbgm_model* m);
const char* sbgm_model_param_name(const sbgm_model* m, int i);
int64_t sbgm_model_param_numel(const sbgm_model* m, int i);

/* Upload one state_dict tensor (device pointer, reference layout: OIHW convs, [out,in] linears, packed
 * mha.in_proj_weight [3C,C]).  The engine repacks into its own NHWC / K-major storage.  Replaces
 * nn.Module.load_state_dict for the path.  `num_batches_tracked` entries are accepted and ignored. */
int sbgm_model_set_param(sbgm_model* m, const char* name, const void* data, int64_t numel, void* stream);
/* Copy an engine-held tensor back in reference layout (used for BatchNorm running statistics after train-mode
 * forwards).  Only vector-shaped entries are supported. */
int sbgm_model_get_param(sbgm_model* m, const char* name, float* dst, int64_t numel, void* stream);
/* 0 when every expected entry has been uploaded; otherwise an error naming the first missing one. */
int sbgm_model_check_complete(const sbgm_model* m);
/* Bytes of activation workspace the handle currently owns.  The first evaluation of a shape runs on a generous bound; later calls
 * ask for the measured high-water mark and the surplus is returned (same addresses in the same order: bit-identical results). */
int64_t sbgm_model_workspace_bytes(const sbgm_model* m);

/* score = ScoreNet(x, t, y, cond_img, lsm_cond, topo_cond); out is NCHW [B,1,H,W].  Optional inputs may be NULL
 * when the model was configured with 0 channels for them.  bn_train != 0 uses batch statistics in the encoder's
 * BatchNorm layers and updates the engine-held running statistics (nn.Module.train() semantics).
 * fmaps (optional, may be NULL): 5 device pointers that receive the encoder feature maps in NHWC. */
int sbgm_model_forward(sbgm_model* m, const float* x, const float* t, const int64_t* y, const float* cond_img,
                       const float* lsm_cond, const float* topo_cond, float* out, float* const* fmaps, int B, int H,
                       int W, int bn_train, void* stream);

/* Whole reverse-SDE sampling loop on the device.  Replaces Euler_Maruyama_sampler / pc_sampler
 * (reference score_sampling.py:63-127, :136-230), including the classifier-free-guidance branch (guided_score_fn,
 * :10-56): with cfg_enabled the conditional and the unconditional evaluation of a step run as ONE batch of 2B samples
 * (rows B..2B-1: null class 0, zeroed cond_img, mask channel of the 2-channel geo fields zeroed) and are combined as
 * (1+w) s_c - w s_u.
 *   noise: NULL -> in-kernel Philox draws keyed by `seed`; else [n_draws][B][1][H][W] host-ordered N(0,1) draws
 *          consumed as the reference consumes torch.randn: init, then per step (corrector,) predictor.
 *   out:   x_mean after the last step, NCHW [B,1,H,W].
 *   use_graph: capture one SDE step into a hipGraph and replay it (ignored when noise != NULL). */
typedef struct sbgm_sampler_args {
    int kind;                /* SBGM_SAMPLER_* */
    int B, H, W;
    int num_steps;
    float eps;               /* smallest time (1e-3) */
    float snr;               /* PC only (0.16) */
    uint64_t seed;
    int use_graph;
    int bn_train;            /* literal reference launch_generation behaviour (generation.py:47) when != 0 */
    const int64_t* y;
    const float* cond_img;
    const float* lsm_cond;
    const float* topo_cond;
    const float* noise;
    float* out;
    int cfg_enabled;         /* classifier-free guidance on (cfg['classifier_free_guidance']['enabled']) */
    float cfg_scale;         /* guidance weight w of the predictor / Euler-Maruyama evaluation */
    float cfg_scale_corrector; /* w of the PC corrector evaluation (the reference clamps only this one to guidance_scale_max, :184-186) */
    /* Full-domain tiling (optional): the B samples are tiles of one domain.  tile_origins: device int32 [B][2] = (y0, x0),
     * x0 % 4 == 0; the in-kernel noise is then keyed by DOMAIN position, so overlapping tiles draw identical noise on the
     * pixels they share, and the Langevin step size of a tile uses that tile's own score norm (not the batch mean), so a tile's
     * result does not depend on which tiles share its batch or its GPU.  NULL = independent samples. */
    const int* tile_origins;
    int domain_w;
} sbgm_sampler_args;
/* Enqueues the whole reverse-SDE loop on `stream` and returns (with use_graph the step is captured once on a private stream and its
 * num_steps replays are launched on `stream`): the step table and the initial state are uploaded from pinned memory the handle owns,
 * so a steady-state call waits for nothing (two runs enqueued back to back simply execute in stream order).  It blocks the host only
 * in these cases: the first call of a (B, H, W) the handle has not seen (one measuring evaluation, then the workspace is sized), a call
 * that has to grow or trim the workspace or the step table (hipFree / hipMalloc), a change of the captured step's key while a replay of
 * the old graph is still executing, and guided runs (cfg_enabled), which free per-call condition copies at their end.  The handle's
 * workspace is the engine's: the caller passes no scratch memory. */
int sbgm_sampler_run(sbgm_model* m, const sbgm_sampler_args* a, void* stream);

/* Deterministic few-step sampler: second-order Heun solver of the probability-flow ODE on the Karras sigma ladder
 * (Karras et al. 2022, Alg. 2), for the same VE-SDE score network (no retraining).  a->kind must be SBGM_SAMPLER_EDM_HEUN;
 * a->snr and a->cfg_scale_corrector are ignored (with guidance both evaluations of a step use cfg_scale); a->bn_train must be 0.
 *   ladder: sigma_i = (smax^(1/rho) + i/(N-1) (smin^(1/rho) - smax^(1/rho)))^rho, i < N = num_steps, sigma_N = 0.
 *           sigma_min / sigma_max <= 0 mean the trained range [std(eps), std(1)] of the model's sigma; other values are clipped to it.
 *   step i: gamma_i = min(s_churn/N, sqrt2-1) if s_tmin <= sigma_i <= s_tmax else 0, capped so sigma_hat = sigma_i (1+gamma_i) <= sigma_0;
 *           x_hat = x + s_noise sqrt(sigma_hat^2 - sigma_i^2) z_i (only when s_churn > 0); d = -sigma_hat score(x_hat, t(sigma_hat));
 *           x' = x_hat + (sigma_{i+1} - sigma_hat) d; then for i < N-1 the Heun correction with score(x', t(sigma_{i+1})), and for
 *           i = N-1 x = x' (one evaluation).  2N-1 network evaluations; out = x after the last step, NCHW [B,1,H,W].
 *   noise:  init x = sigma_0 z_0, then z_{1+i} per step when s_churn > 0: 1 draw, or 1 + N.
 * With use_graph one full Heun step is captured and replayed N-1 times on `stream`; the final Euler-only step is enqueued
 * eagerly.  Blocking behaviour is that of sbgm_sampler_run. */
int sbgm_sampler_run_edm(sbgm_model* m, const sbgm_sampler_args* a, float sigma_min, float sigma_max, float rho, float s_churn,
                         float s_tmin, float s_tmax, float s_noise, void* stream);

/* Constrained sampling (imputation / inpainting, Song et al. 2021 App. I.2): sbgm_sampler_run and sbgm_sampler_run_edm with known pixels
 * held.  known, known_mask: device fp32 [B][1][H][W], both required, used in place (no copy: new contents at the same addresses are read
 * by a cached step graph's replays, as the conditions are); known_mask is clamped to [0,1] in the kernels, known may hold anything (NaN
 * included) where the mask is 0.  hold(v, target, m) = v if m == 0, target if m == 1 (both bit-exactly), else (1-m) v + m target; std =
 * marginal_prob_std in double at the step table's fp32 times, rounded to fp32.
 *   start:      x0 = scale z0 + m known (where m > 0), scale = std(1), or sigma_0 for EDM Heun.
 *   EM / PC predictor, step i, draw z:  x_mean = hold(mean, known, m); x = hold(mean + noise z, known + std(t_{i+1}) z, m), level 0 on
 *               the last step, so out equals known where the mask is 1.
 *   PC corrector, step i, draw z:       x = hold(x + eps score + sqrt(2 eps) z, known + std(t_i) z, m); the score norm is unchanged.
 *   EDM Heun:   both the Euler and the Heun output of step i are hold(., known + sigma_{i+1} z0, m) with the run's draw 0 (read from
 *               noise[0], or recomputed from the seed): the trajectory of a point mass, deterministic.  The churn is not constrained.
 * No extra noise draw is consumed (a held pixel reuses the draw of its update kernel), no launch is added, guidance acts on the
 * evaluations only, and the captured step's key holds the two pointers.  Everything else is as in the unconstrained entry points. */
int sbgm_sampler_run_held(sbgm_model* m, const sbgm_sampler_args* a, const float* known, const float* known_mask, void* stream);
int sbgm_sampler_run_edm_held(sbgm_model* m, const sbgm_sampler_args* a, float sigma_min, float sigma_max, float rho, float s_churn,
                              float s_tmin, float s_tmax, float s_noise, const float* known, const float* known_mask, void* stream);

/* Joint full-domain sampling (Mixture of Diffusers, Jimenez 2023 / MultiDiffusion, Bar-Tal et al. 2023): sbgm_sampler_run and
 * sbgm_sampler_run_edm as ONE diffusion over a domain of domain_h x a->domain_w pixels whose B samples are ALL its tiles (a->tile_origins,
 * in-kernel noise, one batch).  Wherever an update kernel (EM / PC predictor, Langevin corrector, EDM Euler, EDM Heun) reads the score of
 * tile b at domain pixel P it uses
 *     s*(P) = sum_t w_t(P) s_t(P) / sum_t w_t(P)
 * over all tiles t of the batch that cover P, in ascending tile index with the reading tile at its own place, w_t = ramp_y * ramp_x the
 * weight of sbgm_stitch_tiles (ramp length ramp_len = max(1, overlap), no ramp on a domain edge, taken against domain_h and a->domain_w,
 * the padded width), accumulated in fp32 as acc += w s, wsum += w, acc / wsum.  A pixel only one tile covers uses its score unchanged
 * (no arithmetic); any number of tiles may cover a pixel.  The initial state is equal across the copies of a domain pixel (domain-keyed
 * draw 0) and every copy then sees the same x, the same s* computed by the same instruction sequence and the same draw, so all copies of
 * a domain pixel are bit-equal after every kernel of every step (x_mean included) and sbgm_stitch_tiles of the result equals any copy.
 *   Langevin corrector: the step size follows the batch-mean rule eps = 2 (snr sqrt(HW) / mean_t ||s_t||)^2 over the RAW tile scores (one
 *               step size for the domain), not the per-tile norm of a non-joint tiled run.
 *   EDM Heun:   d = -sigma_hat s*, so the stored slope is the blended one too.
 *   known, known_mask: both NULL, or both given as in the _held entry points; the hold runs after the blend and sees equal inputs in
 *               every copy when the fields were cut from domain fields.
 *   guidance:   acts before the blend (the combined B-row score is what the update reads).
 * Refused: no tile_origins, injected noise, bn_train, ramp_len < 1, W not a multiple of 4, an origin that is negative, has x0 % 4 != 0 or
 * has y0 + H > domain_h or x0 + W > domain_w (the table is read back once per call, which waits for `stream`).  No launch is added to the
 * step and no domain-sized buffer exists; the captured step's key holds the joint flag, domain_h and ramp_len, so a joint and a non-joint
 * step never share a graph.  Everything else is as in the entry points above. */
int sbgm_sampler_run_joint(sbgm_model* m, const sbgm_sampler_args* a, int domain_h, int ramp_len, const float* known,
                           const float* known_mask, void* stream);
int sbgm_sampler_run_edm_joint(sbgm_model* m, const sbgm_sampler_args* a, float sigma_min, float sigma_max, float rho, float s_churn,
                               float s_tmin, float s_tmax, float s_noise, int domain_h, int ramp_len, const float* known,
                               const float* known_mask, void* stream);

/* Adaptive deterministic sampler: the probability-flow ODE dx/dt = -1/2 g(t)^2 score(x, t) integrated from t0 to t1 by
 * Dormand-Prince 5(4) with the step controller of scipy.integrate.RK45 (select_initial_step, FSAL, accept when the RMS error
 * norm is < 1, factor min(10, 0.9 err^-0.2), max(0.2, .) on rejection), entirely on the device.  a->kind must be
 * SBGM_SAMPLER_RK45; a->num_steps, a->snr, a->eps and a->cfg_scale_corrector are ignored (with guidance every evaluation uses
 * cfg_scale); a->bn_train must be 0.  t0 > t1 samples (1 -> eps), t0 < t1 encodes data into the latent; both in [0, 1].
 *   x0:         start state [B,1,H,W], or NULL: marginal_prob_std(t0) times draw 0 of the run's Philox stream (a->seed; a->noise, when
 *               given, holds that one draw; tile_origins key it by domain position).
 *   per_sample: 0 = one controller over all B*H*W values (scipy's semantics); 1 = B independent controllers, each with its own t, h,
 *               error norm over its H*W values, accept / reject and counters; a finished or failed sample is frozen.  Required with
 *               tile_origins.
 *   max_steps:  attempts (accepted + rejected) a controller may use.
 *   stats_i:    int64 [4 G + 2], G = per_sample ? B : 1: per controller nfev, n_accepted, n_rejected, status (1 finished, 2 step size
 *               below 10 ulp of t after a rejection, 3 non-finite error norm, 4 max_steps used up), then the surplus attempts (enqueued
 *               after the run was done; at most 1) and the attempts enqueued.  stats_d: double [G] final t (may be NULL).
 * A status other than 1 is not a failure of the call (it returns 0); out then holds the state where the controller stopped.
 * With use_graph one attempt (6 evaluations, their stage kernels, norm, controller, commit) is captured once and replayed on `stream`
 * until the device reports done; the host reads a 4-byte word in pinned memory and stays at most one attempt ahead of it.  Unlike the
 * other samplers the call returns only when the run is complete. */
int sbgm_sampler_run_ode(sbgm_model* m, const sbgm_sampler_args* a, double t0, double t1, double rtol, double atol, int per_sample,
                         int64_t max_steps, const float* x0, int64_t* stats_i, double* stats_d, void* stream);

/* Second-order multistep sampler at ONE evaluation per step: DPM-Solver++(2M) (Lu et al. 2022) on the Karras ladder of sbgm_sampler_run_edm
 * (same sigma_min / sigma_max / rho rules, sigma_N = 0, no churn), for the same VE-SDE score network; eta > 0 is its SDE variant ("2M SDE",
 * midpoint form).  a->kind must be SBGM_SAMPLER_DPMPP_2M; a->snr and a->cfg_scale_corrector are ignored; a->bn_train must be 0.
 *   step i: D_i = x_i + sigma_i^2 score(x_i, t(sigma_i));  x_{i+1} = c_x x_i + c_0 D_i + c_1 D_{i-1} + c_z z_i  with, for sigma_{i+1} > 0,
 *           h_i = ln(sigma_i / sigma_{i+1}), a_i = -expm1(-(1+eta) h_i), c_x = (sigma_{i+1} / sigma_i) exp(-eta h_i),
 *           c_0 = a_i, c_1 = 0 (i = 0);  c_0 = a_i (1 + 1/(2r)), c_1 = -a_i / (2r), r = h_{i-1} / h_i (i >= 1),
 *           c_z = s_noise sigma_{i+1} sqrt(-expm1(-2 eta h_i));  the last step is x_N = D_{N-1}.  The table is built in float64 and stored as
 *           fp32.  Exactly N = num_steps network evaluations; out = x_N, NCHW [B,1,H,W].
 *   noise:  init x = sigma_0 z_0; with eta > 0 also z_{1+i} for step i (the last step consumes its draw with c_z = 0): 1 draw, or 1 + N.
 *   known, known_mask: both NULL, or constrained sampling as in the _held entry points: x_{i+1} = hold(., known + sigma_{i+1} z, m) with
 *           z the run's draw 0 when eta = 0 (the point-mass trajectory, as EDM Heun) and the step's own draw when eta > 0 (as EM / PC);
 *           out equals known where the mask is 1.  The history D is not held.
 *   domain_h, ramp_len: both 0, or joint full-domain sampling as in the _joint entry points (the update reads the blended score).
 * With use_graph one step (evaluation + update) is captured and replayed N times; a deterministic and a stochastic step never share a graph.
 * A run without labels (a->y NULL) keeps its time rows like EM / PC.  Blocking behaviour is that of sbgm_sampler_run. */
int sbgm_sampler_run_dpmpp(sbgm_model* m, const sbgm_sampler_args* a, float sigma_min, float sigma_max, float rho, float eta, float s_noise,
                           const float* known, const float* known_mask, int domain_h, int ramp_len, void* stream);

/* Row-keyed, temporally correlated in-kernel noise for every sampler entry point above.  A noise plan gives sample b of
 * the runs to come a noise row r_b = rows[b] (device int32 [B], used in place: new contents at the same address are read by a cached step
 * graph's replays, as the conditions are) and makes each of its draws a moving average over `lags` = K white rows `stride` = s apart.
 * With P4 = H W / 4 quads per sample, the draw with stream offset `off` at quad q of sample b is
 *     xi_k = the four Philox normals of (seed, off, counter (r_b - k s) P4 + q),  k = 0 .. K-1     (64-bit unsigned counter arithmetic)
 *     z    = w_0 xi_0 ;  z = z + w_k xi_k  for k = 1 .. K-1 in ascending k,  every product and every sum rounded to fp32 on its own,
 * where xi_k is what sbgm_randn_scaled with (seed, off) writes at flat elements [(r_b - k s) H W, (r_b - k s + 1) H W).  So the noise of
 * a sample depends on its row, not on its place in the batch or on its batch-mates; rows 0 .. B-1 with K = 1, w = {1} draw bit for bit
 * what a run without a plan draws; with sum_k w_k^2 = 1 every draw of a sample is N(0,1), independent across pixels and steps, and
 * samples whose rows are j s apart are correlated with acf[j] = sum_k w_k w_{k+j}.
 *   weights: host fp32 [lags], copied into the handle (1 <= lags <= 32, stride >= 1).  The caller keeps every r_b >= (K-1) s; the counter
 *            is never an address, so a smaller row yields other counters, not an out-of-bounds access.
 *   The plan is held by the handle and used by sbgm_sampler_run, its _edm, _held, _joint and _dpmpp variants and the start draw of
 *   sbgm_sampler_run_ode until it is cleared with rows = NULL (stride, weights and lags <= 1 are then ignored; NULL rows with lags > 1
 *   are an error).  It serves the start, EM, PC, EDM Heun's churn and held pixels (the same mixed draw 0), and 2M SDE, each with and
 *   without known / known_mask and guidance; the captured step's key holds the rows pointer, stride, lags and the weights.
 * A run refuses a plan together with a->noise, a->tile_origins (tiled and joint runs) or a start state x0. */
int sbgm_sampler_set_noise_rows(sbgm_model* m, const int32_t* rows, int stride, const float* weights, int lags);

/* The same for tiled and joint runs (a->tile_origins): the domain noise plan.  All tiles of a batch are one field on one
 * day, so ONE row R = *row_dev (device int32, used in place: a new value at the same address is read by a cached step graph's replays)
 * serves the whole batch.  With dom_w4 = ceil(a->domain_w / 4) and Q = domain_h dom_w4 quads per domain, the draw with stream offset `off`
 * at domain row Y, quad column X4 is
 *     xi_k = the four Philox normals of (seed, off, counter (R - k s) Q + Y dom_w4 + X4),  k = 0 .. K-1     (64-bit unsigned arithmetic)
 *     z    = w_0 xi_0 ;  z = z + w_k xi_k  in ascending k,  every product and every sum rounded to fp32 on its own,
 * so R = 0 with K = 1, w = {1} is the tiled draw without a plan bit for bit, a single tile that covers the domain draws what
 * sbgm_sampler_set_noise_rows with rows = {R} draws, and the copies of a domain pixel in overlapping tiles still receive one draw.
 *   Held by the handle until cleared with row_dev = NULL; the two plans exclude each other (setting one while the other is held is an
 *   error; clearing either clears the handle's plan).  1 <= lags <= 32, stride >= 1, domain_h >= 1; weights: host fp32 [lags], copied.
 *   Used by sbgm_sampler_run, its _edm, _held, _joint and _dpmpp variants (a joint run's domain_h must equal the plan's).  A run reads the
 *   tile table and the row back once (this waits for `stream`) and refuses a tile that does not lie quad-aligned inside domain_h x
 *   a->domain_w (its counters would reach into another row's) or R < (K-1) s.  The captured step's key holds the row's address, domain_h,
 *   stride, lags and the weights, not the row's value: two days of one geometry replay one step.
 * Refused: no a->tile_origins, a->noise, sbgm_sampler_run_ode.  sbgm_randn_domain_rows is the draw as an op. */
int sbgm_sampler_set_noise_domain_row(sbgm_model* m, const int32_t* row_dev, int domain_h, int stride, const float* weights, int lags);

/* Conv autotuning: time the tile / split-K candidates of every convolution of the (B,H,W) plan once and keep the
 * fastest.  Synchronises the stream.  Optional; without it a static heuristic is used. */
int sbgm_model_autotune(sbgm_model* m, int B, int H, int W, void* stream);
/* Persist / restore the tuned tile table (text file) so a service tunes once per problem size, not once per process.
 * Load merges into the current table; malformed lines are an error and leave the table untouched. */
int sbgm_model_tune_save(sbgm_model* m, const char* path);
int sbgm_model_tune_load(sbgm_model* m, const char* path);
/* Eager forward with each convolution launch bracketed by HIP events on `stream` (synchronises).  csv_path (host
 * string, may be NULL) receives one line per convolution. */
typedef struct sbgm_profile {
    float ms_total_with_events;  /* whole evaluation, including the event records */
    float ms_conv;               /* sum over implicit-GEMM convolution launches (+ their split-K reduce) */
    float ms_conv_max;           /* slowest single convolution */
    double flops_conv;           /* algorithmic FLOPs of those launches (2*M*Cout*K, unpadded K) */
    double flops_conv_max;
    int n_conv;
} sbgm_profile;
int sbgm_model_profile_forward(sbgm_model* m, const float* x, const float* t, const int64_t* y, const float* cond_img,
                               const float* lsm_cond, const float* topo_cond, float* out, int B, int H, int W,
                               sbgm_profile* summary, const char* csv_path, void* stream);
/* Device time of the last N forwards is not tracked here; bench.py brackets calls with HIP events it gets from: */
int sbgm_event_create(void** ev);
int sbgm_event_record(void* ev, void* stream);
int sbgm_event_elapsed_ms(void* start, void* stop, float* ms);   /* synchronises on `stop` */
int sbgm_event_destroy(void* ev);

/* ------------------------------------------------------------------------------------------------------------
 * Per-op entry points (NHWC fp32).  Each names the torch op instance it replaces.
 * ---------------------------------------------------------------------------------------------------------- */
/* torch.cat + .contiguous(NHWC): up to 4 NCHW sources -> [B,H,W,Cpad] (zero padded).  score_unet.py:273-291 */
int sbgm_pack_input(const float* const* srcs, const int* src_channels, int n_src, float* dst_nhwc, int B, int H,
                    int W, int c_pad, void* stream);
int sbgm_nchw_to_nhwc(const float* src, float* dst, int B, int H, int W, int C, void* stream);
int sbgm_nhwc_to_nchw(const float* src, float* dst, int B, int H, int W, int C, void* stream);

/* nn.Conv2d / nn.Linear weight repack: OIHW -> [k_step][Cout][16].  Returns packed float count via
 * sbgm_conv_packed_numel.  c_pad: padded input channels (4, 8 or a multiple of 16). */
int64_t sbgm_conv_packed_numel(int Cout, int KH, int KW, int c_pad);
int sbgm_conv_pack_weight(const float* w_oihw, float* packed, int Cout, int Cin, int KH, int KW, int c_pad, void* stream);
/* nn.Conv2d (+ folded BatchNorm scale/bias, + time bias, + residual, + ReLU) on the fp32 MFMA implicit-GEMM
 * kernel.  score_unet.py:206-219, torchvision BasicBlock convs, :468, :489; nn.Linear as 1x1 (:127-134).
 * tile_co/tile_px/splits/waves_per_tile = 0 -> defaults.  ws: split-K scratch (>= splits*M*Cout floats) or NULL if splits<=1. */
typedef struct sbgm_conv_args {
    const float* x;          /* [B,H,W,c_pad] */
    const float* w_packed;
    float* out;              /* [B,OH,OW,Cout] */
    const float* scale;      /* [Cout] or NULL */
    const float* bias;       /* [Cout] or NULL */
    const float* tbias;      /* [B,Cout] or NULL */
    const float* residual;   /* [B,OH,OW,Cout] or NULL */
    int B, H, W, c_pad, Cout;
    int KH, KW, stride, pad;
    int act;                 /* SBGM_NONE, SBGM_RELU or SBGM_GELU (exact erf), fused into the epilogue */
    int tbias_after_act;
    int tile_co, tile_px;    /* wave tile in 16-element fragments: {2,4} x {1,2,4}; 0 = default */
    int splits;              /* split-K over the grid (needs ws); 0/1 = off */
    int waves_per_tile;      /* in-workgroup split-K: 1, 2 or 4 waves share one tile (8 with winograd bit 0 alone); 0 = 1 */
    int winograd;            /* bit 0: Winograd F(2,3) weights/kernel (3x3/s1/p1; w_packed from sbgm_conv_wino_pack_weight;
                                tile_px counts 32-pixel fragments: {4,1} {2,2} {2,1} {4,2});
                                bit 1: LDS-staged kernel (W %% 16 == 0; tile_px = tile rows per wave, 2x that with bit 0);
                                bit 2 (with bit 1): two LDS stage buffers, one barrier per stage;
                                bit 5 (32, alone): 8x8/s2/p3 as a space-to-depth Winograd F(2x2,4x4), LDS-staged (w_packed from
                                sbgm_conv8x8s2_wino_pack_weight; c_pad %% 16 == 0; tile_co in {1, 2} = 16 / 32 output channels per
                                workgroup, 0 = 2; tile_px / splits / waves_per_tile ignored; no in_mode, no in_dil) */
    int in_dil;              /* 0/1, or 2: read x through a zero-inserted grid (data gradient of a stride-2 conv) */
    int out_h, out_w;        /* explicit output size (required with in_dil = 2), else 0 */
    float* ws;
    int64_t ws_floats;
    /* LDS-staged kernel only (winograd bits 0+1): what happens to the input while the halo patch is staged, i.e. the
     * normalisation / resampling passes between the convolutions of a DecoderBlock (score_unet.py:583-615) without a pass of
     * their own.  0 = plain.  1 = affine on load: the convolution sees x*scale + shift per (sample, channel) (a GroupNorm of x,
     * in_affine from sbgm_groupnorm_finalize), zero padding kept.  2 = nn.Upsample(x2, bilinear, align_corners=False) on load:
     * x is the LOW-resolution map [B,H/2,W/2,c_pad] (H, W = the convolution's size), optionally act(x*scale + shift + in_skip)
     * first. */
    int in_mode;
    const float* in_affine;  /* [B][c_pad/4][2][4] scale quad, shift quad; required for mode 1, optional for mode 2 */
    const float* in_skip;    /* mode 2: [B,H/2,W/2,c_pad] or NULL */
    int in_act;              /* mode 2: SBGM_NONE / RELU / SILU / GELU applied to the low-resolution value */
    /* Optional second weight image in the Winograd layout (sbgm_conv_wino_pack_weight / a sbgm_pack_desc with transposed bit 1).
     * When given: sbgm_conv2d_tune also times the Winograd candidates, and sbgm_conv2d_fwd takes its weights from here when
     * winograd bit 0 is set (w_packed stays the implicit-GEMM image for every other kernel).  NULL: as before, a call with
     * winograd bit 0 reads the Winograd image from w_packed. */
    const float* w_wino;
    /* Optional third weight image for the 2-D Winograd F(2x2,3x3) LDS kernel (sbgm_conv_wino2d_pack_weight).  winograd bit 3 selects
     * that kernel: 16x16-pixel tiles, tile_co in {1, 2} (16 / 32 output channels per workgroup), tile_px / splits ignored,
     * waves_per_tile = 2 picks the build whose registers are held to two workgroups per CU, bit 2 = two LDS stage buffers, bit 4
     * (16) = the persistent form (two workgroups per CU walk over the tiles, weight slab by LDS-DMA); needs W %% 16 == 0 and an
     * even H; all three in_mode values.  Weights: w_wino2d when given, else w_packed must be that image.
     * When given, sbgm_conv2d_tune also times these candidates (tile[4] == 2 then means bit 3; tile[5] == 3 means bit 4). */
    const float* w_wino2d;
} sbgm_conv_args;
int sbgm_conv2d_fwd(const sbgm_conv_args* a, void* stream);
/* Two convolutions of ONE input (same x, B, H, W, c_pad), each with its explicit tile as in sbgm_conv2d_fwd: what the encoder does with a
 * BasicBlock's 3x3 / stride 2 / pad 1 convolution (main) and its 1x1 / stride 2 shortcut (aux).  Where the implicit-GEMM kernels serve the
 * pair of tiles (a small instantiated set, no grid split-K) both run in one launch, otherwise as two launches, main first; the outputs
 * are those of the two sbgm_conv2d_fwd calls bit for bit.  *paired (may be NULL): 1 when it was one launch.  SBGM_NO_CONV_PAIR=1 in the
 * environment: always two launches.  Both calls name the same split-K workspace `ws` (or none). */
int sbgm_conv2d_pair_fwd(const sbgm_conv_args* main_conv, const sbgm_conv_args* aux_conv, int* paired, void* stream);
/* Times the kernel / tile / split candidates for exactly this call (same operands; launches are idempotent; synchronises)
 * and writes the fastest as tile[6] = {tile_co, tile_px, splits, waves_per_tile, winograd bit 0, LDS kernel: 0 off / 1 on (bit 1) / 2 double-buffered (bits 1+2)}, the values
 * to put into sbgm_conv_args.  Winograd candidates are timed when a->w_wino is given (they need the transformed weights);
 * split-K candidates are considered when a->ws is given.  Used by the training path, whose convolutions run op by op. */
int sbgm_conv2d_tune(const sbgm_conv_args* a, int* tile, void* stream);
/* The candidates sbgm_conv2d_tune would time for exactly this call, without timing anything: host only, no device, no stream, no
 * launch, and no pointer of `a` is dereferenced (x, w_packed, out must be non-NULL; w_wino / w_wino2d / ws count as present or
 * absent).  Same checks as sbgm_conv2d_tune (winograd == 0, Cout %% 32 == 0).  Writes up to `cap` candidates, 6 ints each in the
 * tile[6] form above (tile[4] == 2: F(2x2,3x3), tile[5] == 3: its persistent form), in the order the tuner times them, and returns
 * their number, which may exceed `cap`; 0 for a call sbgm_conv2d_tune refuses.  Split-K candidates appear only with a->ws, and only
 * those whose partial sums (B*OH*OW*Cout*splits floats) fit ws_floats.  Every entry is a tile sbgm_conv2d_fwd runs for this call. */
int sbgm_conv2d_tiles(const sbgm_conv_args* a, int* tiles, int cap);
/* Pack many convolution weights in one launch.  desc: DEVICE array of n descriptors; block_begin = exclusive prefix of
 * sbgm_conv_pack_weights_batched_blocks(Cout, KH, KW, cs) over the descriptors (the workgroups each weight needs),
 * total_blocks = its total; nsteps = sbgm_conv_packed_numel / (Cout*16).
 * transposed bit 0 packs the data-gradient operator: then Cout/Cin are the TRANSPOSED sizes (Cout = forward Cin, Cin = forward
 * Cout) and cs is the padded forward Cout, exactly as sbgm_conv_pack_weight_dgrad does for one weight.
 * transposed bit 1 (3x3 kernels, cs %% 16 == 0, Cout %% 16 == 0): dst is the Winograd image U[kh][cs/16][xi][Cout][16] of
 * sbgm_conv_wino_pack_weight (sbgm_conv_wino_packed_numel floats) of that operator instead; nsteps is ignored.
 * transposed bit 2 (same conditions): dst is the F(2x2,3x3) image of sbgm_conv_wino2d_pack_weight (sbgm_conv_wino2d_packed_numel). */
typedef struct sbgm_pack_desc {
    const float* src;      /* OIHW */
    float* dst;            /* packed [nsteps][Cout][16] */
    int Cout, Cin, KH, KW, cs, nsteps, transposed, block_begin;
} sbgm_pack_desc;
int sbgm_conv_pack_weights_batched_blocks(int Cout, int KH, int KW, int c_pad);
int sbgm_conv_pack_weights_batched(const sbgm_pack_desc* desc_dev, int n, int total_blocks, void* stream);
/* Process-wide switch for the backward launchers (sbgm_conv2d_wgrad[_bias], sbgm_groupnorm_bwd, sbgm_batchnorm_bwd,
 * sbgm_layernorm_bwd's dgamma/dbeta, sbgm_samplesum's output, sbgm_mha_core_bwd's dqkv, sbgm_batchnorm_train_fwd's sums): 1 = the caller
 * hands in already-zeroed scratch and the launchers skip their own memsets.  Returns the previous value. */
int sbgm_set_scratch_prezeroed(int on);
/* Deferred weight-gradient layout passes.  sbgm_conv2d_wgrad[_bias] accumulates most gradients in a [tap][Cout][c_pad] slab (ws)
 * and converts it to OIHW with a small layout launch.  With sbgm_wgrad_defer(1) in force that launch is queued instead, and
 * sbgm_wgrad_flush runs every queued conversion as ONE launch (21 per training step of the default model): the caller keeps the
 * queued ws / dw_oihw buffers alive and untouched until the flush, after which dw_oihw holds the gradients.  Process-wide, returns
 * the previous value; sbgm_wgrad_flush_pending() = number of queued conversions.
 * `on` is a bit mask: bit 0 = the layout passes as above; bit 1 (2) = also queue the weight-gradient GEMMs of the layers the per-tap
 * split-K kernel serves (1x1 / linear, 3x3 stride 2, 3x3 on 4x4 maps, the 8x8 stems) and run them as ONE batched launch at the flush —
 * the caller then keeps dy, x, ws and dw_oihw (and dbias) of every call made under the flag alive and untouched until the flush. */
int sbgm_wgrad_defer(int on);
int sbgm_wgrad_flush(void* stream);
int sbgm_wgrad_flush_pending(void);
/* Forget the queued conversions without running them (returns how many): after a backward pass that raised, the queued dw_oihw
 * destinations may already be freed, and the next backward recomputes every gradient anyway. */
int sbgm_wgrad_discard(void);
/* Winograd F(2,3)-along-rows weight transform for 3x3 kernels: OIHW -> U[kh][c/16][xi][Cout][16] */
int64_t sbgm_conv_wino_packed_numel(int Cout, int c_pad);
int sbgm_conv_wino_pack_weight(const float* w_oihw, float* packed, int Cout, int Cin, int c_pad, void* stream);

/* Winograd F(2x2,3x3) weight transform for 3x3 kernels: OIHW -> U[c/16][xi*4+eta][Cout][16], U = G g G^T */
int64_t sbgm_conv_wino2d_packed_numel(int Cout, int c_pad);
int sbgm_conv_wino2d_pack_weight(const float* w_oihw, float* packed, int Cout, int Cin, int c_pad, void* stream);
/* 8x8 stride-2 pad-3 weight OIHW [Cout][Cin][8][8] -> the space-to-depth F(2x2,4x4) image that sbgm_conv2d_fwd reads with
 * winograd bit 5: U = G g G^T (in fp64) of every 4x4 phase sub-filter, [4 * c_pad / 16 stages][25][Cout][16].  c_pad %% 16 == 0,
 * Cout %% 16 == 0. */
int64_t sbgm_conv8x8s2_wino_packed_numel(int Cout, int c_pad);
int sbgm_conv8x8s2_wino_pack_weight(const float* w_oihw, float* packed, int Cout, int Cin, int c_pad, void* stream);

/* The stem's two 8x8 / stride-2 / pad-3 convolutions as ONE 22x22 / stride-4 correlation (samplers only; conv_stem22.hip):
 *   conv2(conv1(in) + tb0[:, :, None, None]) = sum_cin Wc[class] * in[cin] + S[class] . tb0,  64 -> 64 channels in between.
 * conv2 zero-pads conv1's output, so the composed filter depends on the output's border class (5 per axis: o = 0, 1, interior,
 * O - 2, O - 1).  pack: w1 OIHW [64][Cin][8][8], w2 OIHW [64][64][8][8] -> wc (sbgm_stem22_packed_numel(Cin) floats) and s
 * (sbgm_stem22_bias_numel() floats), summed in fp64, rounded once.
 * fwd: out [B][H/4][W/4][64] (NHWC) = act(scale * (sum over the weight channels first_channel .. first_channel + n_channels - 1 of
 * the composed correlation of src [B][n_channels][H][W] (NCHW) + S . tb0 + addend) + bias).  tb0 [B][64], addend (out's layout; may
 * be out itself), scale, bias [64] may be NULL; relu != 0 applies ReLU.  H, W >= 32 and multiples of 4; Cin <= 16. */
int64_t sbgm_stem22_packed_numel(int Cin);
int64_t sbgm_stem22_bias_numel(void);
int sbgm_stem22_pack_weight(const float* w1_oihw, const float* w2_oihw, float* wc, float* s, int Cin, void* stream);
int sbgm_stem22_fwd(const float* src, int n_channels, int first_channel, int Cin, const float* wc, const float* s, const float* tb0,
                    const float* addend, const float* scale, const float* bias, int relu, float* out, int B, int H, int W, void* stream);

/* The final DecoderBlock (identity norms, no skip, no time term, identity activation: score_unet.py:713-730, :757) as ONE 3x3
 * convolution (conv_final.hip): conv(conv_up(up(x))) = gather(Wc * up(x) + bc), Wc[tap][ci][v][b] = sum_co w2[0][co][tap] w1[co][ci][v][b],
 * bc[tap] = sum_co w2[0][co][tap] b1[co], out[o] = b2 + sum_tap d[tap][o + tap - 1] with d = 0 outside the image.
 * pack: w1 OIHW [C][C][3][3] and b1 [C] (conv_up), w2 OIHW [1][C][3][3] (conv) -> wc OIHW [16][C][3][3] (rows 9..15 zero) and bc [16],
 * summed in fp64 and rounded once; pack wc with sbgm_conv_pack_weight, sbgm_conv_wino_pack_weight, sbgm_conv_wino2d_pack_weight (Cout 16).
 * fwd: x = the LOW-resolution NHWC input [B,H/2,W/2,C], optionally act(x*scale + shift + in_skip) on load (in_affine / in_skip / in_act
 * as in sbgm_conv_args, fused route only); out [B,1,H,W] = the block's output, divided by sigma(t) when t [B] is given.  W >= 32 runs
 * the bilinear x2 inside the convolution (in_mode 2) as the decoder does, narrower maps upsample into ws first.  ws: 16*B*H*W floats
 * (+ C*B*H*W for the narrow route).  tile: NULL = the engine's static choice, else one of sbgm_final_block_tiles' candidates
 * {tile_co, tile_px, splits, waves_per_tile, winograd kind, LDS kind}; w_wino2d may be NULL when no such tile is used.
 * sbgm_final_block_tiles writes up to `cap` candidates (6 ints each), the ones the autotuner times for this op, and returns their number. */
int sbgm_final_compose_pack(const float* w1_oihw, const float* b1, const float* w2_oihw, float* wc_oihw, float* bc, int C, void* stream);
int sbgm_final_block_tiles(int B, int H, int W, int C, int* tiles, int cap);
int sbgm_final_block_fwd(const float* x, const float* in_affine, const float* in_skip, int in_act, const float* w_packed,
                         const float* w_wino, const float* w_wino2d, const float* bc, const float* b2, const float* t, float sigma,
                         float* out, float* ws, int64_t ws_floats, int B, int H, int W, int C, const int* tile, void* stream);

/* The same block with the channels mixed at LOW resolution (conv_final.hip, the route of the EM / PC / EDM Heun samplers): the channel
 * mix commutes with the per-channel bilinear x2 and the two 3x3 stencils compose into one 5x5 stencil, so
 *   Z[s] = sum_ci Wz[s][ci] v[ci] (low-res, s = (sy, sx) in 0..4 x 0..4),   out[o] = beta + sum_{s, o+s-2 inside the image} up(Z[s])[o + s - 2].
 * conv zero-pads conv_up's OUTPUT, so the first and the last output row / column drop the taps whose intermediate pixel lies outside:
 * 3 classes per axis (first, interior, last), 9 sets (Wz, beta), class index 3*cy + cx:
 *   Wz[c][sy][sx][ci] = sum over ty in valid(cy), tx in valid(cx), ty+vy = sy, tx+vx = sx of sum_co w2[0][co][ty][tx] w1[co][ci][vy][vx],
 *   beta[c] = b2 + sum over the valid taps of sum_co w2[0][co][tap] b1[co];   valid: first {1,2}, interior {0,1,2}, last {0,1}.
 * pack: -> wz_out [9][25][C] and beta_out [9] (fp64 sums rounded once; wz_out may be NULL) and wz_packed
 * (sbgm_final_lowres_packed_numel(C) floats: per class the MFMA A operand [C/16][32][16], rows 25..31 zero).
 * fwd: x = the low-resolution NHWC input [B,H/2,W/2,C], optionally act(x*scale + shift + in_skip) on load (any map size); out [B,1,H,W],
 * divided by sigma(t) when t [B] is given.  ws: sbgm_final_lowres_ws_numel(B, H, W) floats.  C % 16 == 0, C <= 128, H and W even, >= 4. */
int64_t sbgm_final_lowres_packed_numel(int C);
int64_t sbgm_final_lowres_ws_numel(int B, int H, int W);
int sbgm_final_lowres_pack(const float* w1_oihw, const float* b1, const float* w2_oihw, const float* b2, float* wz_out, float* beta_out,
                           float* wz_packed, int C, void* stream);
int sbgm_final_lowres_fwd(const float* x_lowres_nhwc, const float* in_affine, const float* in_skip, int in_act, const float* wz_packed,
                          const float* beta, const float* t, float sigma, float* out, float* ws, int64_t ws_floats, int B, int H, int W,
                          int C, void* stream);

/* The same block where the step samplers form the decoder's last skip inside the mix instead of reading the stem's map (C = 64):
 *   v = act(raw * scale + shift + skip),   skip = conv1(x || cond) + tb0 = sc + tb0 + conv1_x(x)
 * with conv1 the encoder's 8x8 / stride-2 / pad-3 convolution, conv1_x its share over input channel 0 and sc its share over the other
 * channels (constant during a run).  pack: w1 OIHW [64][Cin][8][8] -> w1x, sbgm_skip_mix_packed_numel() floats, the MFMA A operand
 * [16 k steps][64 co][4]: k step s, quarter kq = tap 4 s + kq = 8 v + u of channel 0.
 * fwd: raw = the low-resolution NHWC map [B,H/2,W/2,64] with in_affine / in_act as above; x_planar [B,1,H,W]; sc_nhwc [B,H/2,W/2,64] or
 * NULL (no condition channels); tb0 [B,64]; out, t, sigma and ws as in sbgm_final_lowres_fwd. */
int64_t sbgm_skip_mix_packed_numel(void);
int sbgm_skip_mix_pack(const float* w1_oihw, float* w1x, int Cin, void* stream);
int sbgm_final_lowres_skip_fwd(const float* raw_lowres_nhwc, const float* in_affine, int in_act, const float* wz_packed, const float* beta,
                               const float* x_planar, const float* sc_nhwc, const float* tb0, const float* w1x, const float* t, float sigma,
                               float* out, float* ws, int64_t ws_floats, int B, int H, int W, int C, void* stream);

/* A resize DecoderBlock's conv_up(up(x)) on a small map with the channels mixed at LOW resolution (conv_uplow.hip, the route the EM / PC /
 * EDM Heun samplers take for blocks whose output is narrower than 32 pixels): `up` acts per channel and a tap's weight per pixel, so
 *   Z_tap[co] = sum_ci W[co][ci][k][l] x[ci] (low-res, tap = 3k + l),   out[co][o] = b[co] + sum_{tap, o+tap-1 inside the 2x map} up(Z_tap)[co][o + tap - 1].
 * pack: w OIHW [C][C][3][3] -> w_taps, the OIHW [9C][C][1][1] weight of the mix (row tap*C + co), and w_packed, its implicit-GEMM image
 * (sbgm_up_lowres_weight_numel(C) floats each).
 * fwd: x = the low-resolution NHWC input [B,H/2,W/2,C] -> out NHWC [B,H,W,C]; groups > 0: followed by GroupNorm(groups) with eps and the
 * affine gamma / beta (both NULL: none), formed inside the gather where a (sample, group) fits one workgroup.  ws:
 * sbgm_up_lowres_ws_numel(B, H, W, C, groups) floats, 8-byte aligned.  C % 16 == 0, H and W even. */
int64_t sbgm_up_lowres_weight_numel(int C);
int64_t sbgm_up_lowres_ws_numel(int B, int H, int W, int C, int groups);
int sbgm_up_lowres_pack(const float* w_oihw, float* w_taps, float* w_packed, int C, void* stream);
int sbgm_up_lowres_fwd(const float* x_lowres_nhwc, const float* w_packed, const float* bias, const float* gamma, const float* beta,
                       int groups, float eps, float* out, float* ws, int64_t ws_floats, int B, int H, int W, int C, void* stream);

/* nn.LayerNorm(C, eps) followed by nn.Linear(C, Cout) without a normalisation pass (conv_igemm.hip; the route the EM / PC / EDM Heun
 * samplers take for the attention blocks that run separate GEMMs, score_unet.py:136-148): LN(x) = r diag(gamma) (I - 11^T/C) x + beta with
 * r = 1/sqrt(var(x) + eps), so
 *   linear(LN(x))[co] = r * sum_k W''[co][k] x[k] + h[co],   W'' = W diag(gamma) (I - 11^T/C),   h = b + W beta.
 * pack: w [Cout][C], b [Cout] or NULL, gamma / beta [C] -> w2_oihw [Cout][C] (W'') and h [Cout], summed in fp64 and rounded once, and
 * w2_packed, the implicit-GEMM image of W'' (sbgm_conv_packed_numel(Cout, 1, 1, C) floats).  C % 16 == 0.
 * fwd: x [M][C] raw rows -> out [M][Cout] = act(r * W'' x + h + res), res [M][Cout] or NULL, act as in sbgm_conv_args.  The product loads
 * every element of a row as its B operand and sums it and its square in fp64 on the way, so r is the two-pass fp64 value to fp32 rounding
 * for rows with |mean|/sigma up to 64 at least.  tile: NULL or six zeros = the static choice, else one of sbgm_ln_linear_tiles'
 * candidates {tile_co, tile_px, 1, waves_per_tile, 0, 0}, tile_co in {1, 2, 4}; Cout % (16 tile_co) == 0, no grid split-K.
 * sbgm_ln_linear_tiles writes up to `cap` candidates (6 ints each), the ones the autotuner times for this op, and returns their number. */
int sbgm_ln_fold_pack(const float* w, const float* b, const float* gamma, const float* beta, int C, int Cout, float* w2_oihw, float* w2_packed,
                      float* h, void* stream);
int sbgm_ln_linear_tiles(int M, int C, int Cout, int* tiles, int cap);
int sbgm_ln_linear_fwd(const float* x, const float* w2_packed, const float* h, const float* res, int act, float eps, float* out, int M, int C,
                       int Cout, const int* tile, void* stream);

/* Time rows of an Euler-Maruyama / predictor-corrector run without labels: the run computes the time-bias vectors of all
 * its steps once, row s = the vectors at the time of step s one after the other, and the end of a step publishes the row of the next.
 * Host-side statements of the two rules, usable without a device:
 * sbgm_time_row_layout: widths channels[n] (n in 1..16, positive multiples of 4) -> offsets[n + 1], the start of each vector in a row
 * in floats with offsets[n] = the row length; returns the row length, or -1 for widths a row cannot hold.
 * sbgm_time_row_index: the row a run of num_steps steps evaluates at after `advances` completed steps (the last step republishes its own). */
int sbgm_time_row_layout(const int* channels, int n, int* offsets);
int64_t sbgm_time_row_index(int64_t advances, int64_t num_steps);

/* ConvTranspose2d(k=2,s=2) = one 1x1 convolution to 4C channels (weights from sbgm_tconv_weight_to_oihw, bias repeated
 * 4x) followed by depth->space; its backward is space->depth followed by the 1x1 convolution's backward. */
int sbgm_depth_to_space2(const float* x /* [B,H,W,4C] */, float* y /* [B,2H,2W,C] */, int B, int H, int W, int C, void* stream);
int sbgm_space_to_depth2(const float* y /* [B,2H,2W,C] */, float* x /* [B,H,W,4C] */, int B, int H, int W, int C, void* stream);
/* The same permutation for any stride s in 1..16 (ConvTranspose2d(k = s, stride = s): DecoderBlock(upsample_scale = s, use_resize_conv =
 * False) called on its own): depth [B,H,W,s*s*C] with channels ordered (dy, dx, c) <-> space [B,s*H,s*W,C]. */
int sbgm_depth_to_space(const float* x, float* y, int B, int H, int W, int C, int s, void* stream);
int sbgm_space_to_depth(const float* y, float* x, int B, int H, int W, int C, int s, void* stream);
int sbgm_tconv_weight_to_oihw(const float* w /* [Cin,Cout,2,2] */, float* oihw /* [4*Cout,Cin,1,1] */, int Cin, int Cout,
                              void* stream);
/* nn.Upsample(scale_factor=2, mode="bilinear", align_corners=False).  score_unet.py:467 */
int sbgm_upsample2x_fwd(const float* x, float* y, int B, int H, int W, int C, void* stream);
/* nn.GroupNorm / nn.InstanceNorm2d (+ skip add, + time bias, + activation).  score_unet.py:480-483, :585-615.
 * gamma/beta NULL = no affine (InstanceNorm2d default).  stats_ws: >= 1024*B*G bytes. */
int sbgm_groupnorm_fwd(const float* x, float* y, const float* gamma, const float* beta, const float* skip,
                       const float* tbias, int act, int B, int HW, int C, int G, float eps, void* stats_ws,
                       float* mean_rstd_out /* [B,G,2] or NULL */, void* stream);
/* GroupNorm statistics only (the chunk partials sbgm_groupnorm_fwd computes first): stats_ws as above; *chunks receives the
 * number of partials per (sample, group).  Then sbgm_groupnorm_finalize turns them into the per-(sample, channel) affine a
 * consumer convolution applies on load (sbgm_conv_args.in_affine): out[b][c/4][0][c%4] = rstd*gamma,
 * out[b][c/4][1][c%4] = beta - mean*rstd*gamma (+ tbias[b][c]).  gamma/beta NULL = no affine. */
int sbgm_groupnorm_stats(const float* x, void* stats_ws, int B, int HW, int C, int G, int* chunks, void* stream);
int sbgm_groupnorm_finalize(const void* stats_ws, int chunks, const float* gamma, const float* beta, const float* tbias,
                            float* out /* [B][C][2] */, int B, int HW, int C, int G, float eps, void* stream);
/* nn.LayerNorm(C).  score_unet.py:128-129 */
int sbgm_layernorm_fwd(const float* x, float* y, const float* gamma, const float* beta, int M, int C, float eps, void* stream);
/* nn.BatchNorm2d in training mode (+ residual, ReLU, time bias).  stats_ws: >= 24*C bytes; its first 16*C bytes are the
 * fp64 sums and must arrive zeroed when sbgm_set_scratch_prezeroed(1) is in force.  mean_rstd_out [C,2] (for
 * sbgm_batchnorm_bwd) or NULL: the pairs are then left behind the sums, at stats_ws + 16*C bytes. */
int sbgm_batchnorm_train_fwd(const float* x, float* y, const float* gamma, const float* beta, float* running_mean,
                             float* running_var, const float* residual, const float* tbias_after, int relu, int B, int HW,
                             int C, float eps, float momentum, void* stats_ws, float* mean_rstd_out, void* stream);
/* SyncBatchNorm (new capability: the reference is single-device, so its BatchNorm sees the whole batch, score_unet.py:323; with
 * the batch sharded over ranks the statistics must be summed over the ranks to reproduce that step).  The forward above in two
 * halves: _stats leaves the per-channel fp64 sums (x, x^2) of the local batch in stats_ws[2*C]; the caller sums stats_ws over
 * the ranks (one RCCL all-reduce of 2*C doubles); _apply finalises with n_total = sum over ranks of B*HW. */
int sbgm_batchnorm_train_stats(const float* x, int B, int HW, int C, void* stats_ws, void* stream);
int sbgm_batchnorm_train_apply(const float* x, float* y, const float* gamma, const float* beta, float* running_mean,
                               float* running_var, const float* residual, const float* tbias_after, int relu, int B, int HW, int C,
                               float eps, float momentum, void* stats_ws, double n_total, float* mean_rstd_out, void* stream);
/* Core of nn.MultiheadAttention between in_proj and out_proj: qkv [B,S,3C] -> [B,S,C].  score_unet.py:142 */
int sbgm_mha_core_fwd(const float* qkv, float* out, int B, int S, int C, int heads, void* stream);
/* The same core with TRAIN-MODE DROPOUT on the softmax probabilities — nn.MultiheadAttention(dropout = p), the `dropout` argument of
 * ImageSelfAttention (score_unet.py:118-127): out = (softmax(q k^T / sqrt(d)) o D) v with D_ij = keep_ij / (1 - p), keep_ij drawn from a
 * Philox stream keyed by (seed, offset, ((b heads + h) S + i) S + j).  _bwd needs the same (p, seed, offset) and the forward's qkv; dqkv
 * [B,S,3C] is accumulated with atomics (zeroed by the call unless sbgm_set_scratch_prezeroed(1)).  sbgm_mha_dropout_mask writes D
 * [B,heads,S,S] (how the tests compare against an explicit-mask evaluation).  0 <= p < 1; 32 * S bytes of LDS per workgroup. */
int sbgm_mha_core_dropout_fwd(const float* qkv, float* out, int B, int S, int C, int heads, float p, uint64_t seed, uint64_t offset,
                              void* stream);
int sbgm_mha_core_dropout_bwd(const float* qkv, const float* dout, float* dqkv, int B, int S, int C, int heads, float p, uint64_t seed,
                              uint64_t offset, void* stream);
int sbgm_mha_dropout_mask(float* mask, int B, int S, int heads, float p, uint64_t seed, uint64_t offset, void* stream);
/* The per-token halves of ImageSelfAttention (score_unet.py:141-145) as single launches over token tiles, C in {64,128,256,512}:
 *   sbgm_attn_qkv_fwd : qkv[M][3C] = LayerNorm(x; ln_gamma, ln_beta) . in_proj_weight^T + in_proj_bias          (self.ln1 + mha in_proj)
 *   sbgm_attn_tail_fwd: h = x + att . out_proj^T + b_out;  out = h + ff[2](GELU(ff[0](LayerNorm(h))))           (:142-145)
 * Weights are sbgm_conv_pack_weight images of the [Cout][C][1][1] matrices; `out` may alias `x`, not `att`. */
int sbgm_attn_qkv_fwd(const float* x, const float* ln_gamma, const float* ln_beta, const float* w_in_packed, const float* b_in,
                      float* qkv, int M, int C, float eps, void* stream);
int sbgm_attn_tail_fwd(const float* att, const float* x, const float* w_out_packed, const float* b_out, const float* ln_gamma,
                       const float* ln_beta, const float* w_ff1_packed, const float* b_ff1, const float* w_ff2_packed,
                       const float* b_ff2, float* out, int M, int C, float eps, void* stream);
/* Which kernel instantiation ("variant") the attention launchers run for a shape.  Host-only: no device, no stream, no launch; the
 * launchers call the same functions, and the SBGM_NO_LDS_ATTENTION / SBGM_NO_MHA_BWD_MFMA / SBGM_MHA_BWD_G / SBGM_MHA_BWD_WIDE_S
 * environment switches act on both alike (each is read once per process).  A variant id indexes the complete list of instantiations
 * of its family, 0 .. _variant_count() - 1; _variant_name(id) is the kernel's name (NULL outside the list).  The return value is the
 * id, or -1 where the launcher refuses the shape (info is then unspecified).
 *   sbgm_mha_core_fwd_variant : info = { family SBGM_MHA_FWD_*, d16 = ceil(head dim / 16), KSPLIT (register) or NQ (LDS), qsplit }
 *   sbgm_mha_core_bwd_variant : info = { family SBGM_MHA_BWD_*, head dim, G (query blocks per workgroup; 1 outside mfma), workgroups }
 *                               (head dims that are no multiple of 4 are not refused: they take the scalar kernel)
 *   sbgm_attn_tokens_variant  : info = { C / 64, tokens per tile }; one id stands for that instantiation of BOTH token kernels */
enum { SBGM_MHA_FWD_REGISTER = 0, SBGM_MHA_FWD_LDS = 1 };
enum { SBGM_MHA_BWD_MFMA = 0, SBGM_MHA_BWD_LDS16 = 1, SBGM_MHA_BWD_LDS32 = 2, SBGM_MHA_BWD_SCALAR = 3 };
int sbgm_mha_core_fwd_variant(int B, int S, int C, int heads, int info[4]);
int sbgm_mha_core_fwd_variant_count(void);
const char* sbgm_mha_core_fwd_variant_name(int id);
int sbgm_mha_core_bwd_variant(int B, int S, int C, int heads, int info[4]);
int sbgm_mha_core_bwd_variant_count(void);
const char* sbgm_mha_core_bwd_variant_name(int id);
int sbgm_attn_tokens_variant(int M, int C, int info[2]);
int sbgm_attn_tokens_variant_count(void);
const char* sbgm_attn_tokens_variant_name(int id);
/* SinusoidalEmbedding (+ label embedding) -> SiLU -> Linear, for one projection.  score_unet.py:41-45, :377-381 */
int sbgm_time_proj_fwd(const float* t, const int64_t* y, const float* label_emb, const float* freqs, const float* weight,
                       const float* bias, float* out, float* emb_ws /* [B,D] silu(emb) */, float* emb_raw /* [B,D] or NULL */,
                       int B, int D, int ch, void* stream);
/* Several projections in one launch pair (embeddings | projections): n_emb embeddings (label_emb is added to embedding 0), n_proj
 * projections, projection i reads embedding emb_index[i] and writes outs[i] [B, chs[i]].  emb_ws / emb_raw: [n_emb][B][D]
 * (silu(emb) / emb; emb_raw may be NULL).  n_emb <= 8, n_proj <= 16.  The encoder's 5 projections share one embedding
 * (score_unet.py:301-308); each decoder block has its own (:606-609). */
int sbgm_time_proj_multi_fwd(const float* t, const int64_t* y, const float* label_emb, const float* const* freqs, int n_emb,
                             const float* const* weights, const float* const* biases, float* const* outs, const int* chs,
                             const int* emb_index, int n_proj, float* emb_ws, float* emb_raw, int B, int D, void* stream);
/* final_layer.conv (3x3, C->1) + division by marginal_prob_std(t).  score_unet.py:489, :876-877.
 * w_tap_c from sbgm_cout1_pack_weight; t NULL = no division. */
int sbgm_cout1_pack_weight(const float* w_oihw, float* w_tap_c, int C, void* stream);
int sbgm_conv3x3_cout1_fwd(const float* x, const float* w_tap_c, const float* bias, const float* t, float sigma, float* out,
                           int B, int H, int W, int C, void* stream);
/* Elementwise activation in place (GELU between the attention FF linears, score_unet.py:132). */
int sbgm_act_inplace(float* x, int64_t n, int act, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Training path: what `loss.backward()` (reference training.py:403-405) needs from each op above.
 * Data gradients of convolutions / linears run sbgm_conv2d_fwd on weights packed by sbgm_conv_pack_weight_dgrad
 * (stride-2 layers with in_dil = 2 and an explicit output size).
 * ---------------------------------------------------------------------------------------------------------- */
int sbgm_conv_pack_weight_dgrad(const float* w_oihw, float* packed, int Cout, int Cin, int KH, int KW, void* stream);
/* Data gradient of an 8x8 / stride-2 / pad-3 convolution (the encoder's conv2, score_unet.py:214-219) by output phase instead of
 * through a zero-inserted dy: builds the OIHW operator [4*Cin][Cout][5][5] whose 5x5 / stride-1 / pad-2 convolution over dy
 * [B,OH,OW,Cout] yields the 4 phases (py, px, ci) of dx; sbgm_depth_to_space2 interleaves them into dx [B,2*OH,2*OW,Cin].
 * 2.56x fewer MACs than the dilated form.  Pack the result with sbgm_conv_pack_weight(.., 4*Cin, Cout, 5, 5, Cout). */
int sbgm_conv8x8s2_dgrad_phase_weight(const float* w_oihw, float* out_oihw, int Cout, int Cin, void* stream);
/* dW (OIHW) = sum_p dy[p,:] (x) x[p@tap,:]; ws: >= KH*KW*Cout*c_pad floats.  For a 1x1 kernel with c_pad == Cin (and c_pad % 64
 * == 0) ws may be dw_oihw itself: the partial sums then meet directly in the gradient and the layout pass is skipped. */
int sbgm_conv2d_wgrad(const float* dy, const float* x, float* dw_oihw, float* ws, int B, int H, int W, int c_pad, int Cin,
                      int Cout, int KH, int KW, int stride, int pad, void* stream);
/* the same, plus the bias gradient db[Cout] = sum_p dy[p,:] produced by the waves that stream dy anyway */
int sbgm_conv2d_wgrad_bias(const float* dy, const float* x, float* dw_oihw, float* dbias, float* ws, int B, int H, int W, int c_pad,
                           int Cin, int Cout, int KH, int KW, int stride, int pad, void* stream);
/* What an immediate sbgm_conv2d_wgrad[_bias] call of this geometry launches; host arithmetic only (no device, no pointers), the
 * helper the launcher itself acts on.  out = {family, gx, gy, tiles_per_wg, n_tiles, direct, M = B*OH*OW, 0}:
 *   family: SBGM_WGRAD_GENERAL1/2/4 the wave-level kernel with 16 / 32 / 64 input channels per tile (any geometry),
 *           SBGM_WGRAD_HALO16 / _HALO8 the 3x3 stride-1 halo kernel on 16x16 tiles / on 8x8 maps (four images per tile),
 *           SBGM_WGRAD_TAP64 / _TAP128 the per-tap split-K GEMM on 64x64 blocks over 128-pixel tiles / 128x128 blocks over 64-pixel
 *           tiles, SBGM_WGRAD_STEM its form for 8x8 kernels on c_pad = 8;
 *   gx x gy workgroups, each walking tiles_per_wg of the n_tiles pixel tiles (general kernel: gy pixel splits of tiles_per_wg
 *   pixels, n_tiles = M);  direct = 1: gy == 1 and the kernel stores OIHW itself, ws is not touched and no layout pass runs.
 * Non-zero (text in sbgm_last_error) for a geometry sbgm_conv2d_wgrad refuses.  Reads SBGM_NO_LDS_WGRAD per call, SBGM_NO_TAP128 and
 * SBGM_WG_TARGET once per process, as the launcher does. */
enum { SBGM_WGRAD_GENERAL1 = 0, SBGM_WGRAD_GENERAL2 = 1, SBGM_WGRAD_GENERAL4 = 2, SBGM_WGRAD_HALO16 = 3, SBGM_WGRAD_HALO8 = 4,
       SBGM_WGRAD_TAP64 = 5, SBGM_WGRAD_TAP128 = 6, SBGM_WGRAD_STEM = 7 };
int sbgm_conv2d_wgrad_plan(int B, int H, int W, int c_pad, int Cin, int Cout, int KH, int KW, int stride, int pad, int out[8]);
/* What sbgm_wgrad_flush would launch for the work queued at this moment (sbgm_wgrad_defer bit 1); changes nothing.  Returns the number
 * of queued GEMMs n.  out (may be NULL; else 2 + 7 * cap ints): out[0] = layout passes the flush will run (those already queued and
 * those its GEMMs add), out[1] = layout launches, then min(n, cap) rows {family, launch, gx, gy, tiles_per_wg, n_tiles, direct} in
 * launch order (16x16 halo layers, 8x8 halo layers, per-tap layers); launch = index of the batched launch of its family the GEMM
 * rides in.  The split of a queued GEMM depends on everything queued with it, so the rows hold until the next call that queues. */
int sbgm_wgrad_flush_plan(int* out, int cap);
/* `optimizer.step()` of torch.optim.Adam (decoupled = 0: weight decay as an L2 term on the gradient) or AdamW (decoupled = 1)
 * over every parameter tensor in one launch (reference training.py:407, training_utils.py:50-59).  desc: DEVICE array of n
 * descriptors, block_begin = exclusive prefix of sbgm_adam_step_blocks(numel), total_blocks = its total.  step: DEVICE
 * scalar holding the step count t of THIS update (the caller increments it before the call), used for the bias corrections
 * 1 - beta^t.  Update: m += (1-b1)(g'-m); v = b2 v + (1-b2) g'^2; p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps). */
typedef struct sbgm_adam_desc {
    float* p;              /* parameter */
    const float* g;        /* gradient */
    float* m;              /* exp_avg */
    float* v;              /* exp_avg_sq */
    int64_t numel;
    int block_begin, reserved;
} sbgm_adam_desc;
int sbgm_adam_step_blocks(int64_t numel);
/* grad_scale multiplies every gradient as it is read (1, or 1/world when the gradients are the data-parallel SUM over the
 * replicas: the averaging of reference-style data parallelism without a pass of its own). */
int sbgm_adam_step_batched(const sbgm_adam_desc* desc_dev, int n, int total_blocks, const float* step, float lr, float beta1,
                           float beta2, float eps, float weight_decay, int decoupled, float grad_scale, void* stream);
/* The same step with an exponential moving average of the parameters in the same launch (training.with_ema).  ema: DEVICE array
 * of n shadow pointers, parallel to desc.  After the update each shadow moves towards its parameter, e += ema_rate * (p - e),
 * ema_rate = 1 - decay of this step; p, m and v come out bit-identical to the launch without the average.  A descriptor with
 * g == NULL takes no optimizer step (m, v unused): only its shadow moves towards p, or, with reserved == 1, receives a bit copy of
 * p, numel then counting 32-bit words (integer buffers such as num_batches_tracked).  Shadows follow the 16-byte alignment rule
 * of the other pointers (aligned tensors take the vector path, the rest the scalar one). */
int sbgm_adam_ema_step_batched(const sbgm_adam_desc* desc_dev, float* const* ema, int n, int total_blocks, const float* step, float lr,
                               float beta1, float beta2, float eps, float weight_decay, int decoupled, float grad_scale, float ema_rate,
                               void* stream);
/* EMA only, for optimizers whose step is not the launch above: every descriptor is treated as g == NULL (g, m, v are never read).
 * Blocks per descriptor: sbgm_adam_step_blocks(numel). */
int sbgm_ema_update_batched(const sbgm_adam_desc* desc_dev, float* const* ema, int n, int total_blocks, float ema_rate, void* stream);
int sbgm_colsum(const float* x, const float* y /* NULL or multiplied elementwise */, float* out, int M, int C, void* stream);
int sbgm_samplesum(const float* x, float* out /* [B,C] */, int B, int HW, int C, void* stream);
/* ws: >= 8*B*C bytes */
int sbgm_groupnorm_bwd(const float* x, const float* dy, const float* gamma, const float* beta, const float* skip,
                       const float* tbias, const float* mean_rstd, int act, float* dx, float* dskip, float* dgamma,
                       float* dbeta, float* dtbias, float* ws, int B, int HW, int C, int G, void* stream);
int sbgm_batchnorm_bwd(const float* x, const float* dy, const float* y, const float* gamma, const float* tbias_after,
                       const float* mean_rstd /* [C,2] */, int relu, float* dx, float* dres, float* dgamma, float* dbeta,
                       float* ws, int B, int HW, int C, void* stream);
/* SyncBatchNorm backward in two halves: _reduce leaves the local sums (g, g*xhat) per (sample, channel) in ws [B][C][2]; the caller
 * sums them over samples and ranks into sync_sums [C][2] (one all-reduce of 2*C floats); _apply uses sync_sums / n_total for the two
 * means (sync_sums NULL: the local ws and B*HW, i.e. exactly sbgm_batchnorm_bwd).  dgamma / dbeta stay LOCAL sums: they are
 * averaged over the ranks with every other parameter gradient. */
int sbgm_batchnorm_bwd_reduce(const float* x, const float* dy, const float* y, const float* tbias_after, const float* mean_rstd,
                              int relu, float* ws, int B, int HW, int C, void* stream);
int sbgm_batchnorm_bwd_apply(const float* x, const float* dy, const float* y, const float* gamma, const float* tbias_after,
                             const float* mean_rstd, int relu, float* dx, float* dres, float* dgamma, float* dbeta, const float* ws,
                             const float* sync_sums, double n_total, int B, int HW, int C, void* stream);
/* dx_add [M,C] or NULL: added to dx (the gradient reaching x along its other consumer, e.g. the residual around the block) */
int sbgm_layernorm_bwd(const float* x, const float* dy, const float* gamma, float* dx, float* dgamma, float* dbeta, int M,
                       int C, float eps, const float* dx_add, void* stream);
/* zero `bytes` (multiple of 4) of device memory with a kernel on `stream` (graph-capture safe; see common.h on hipMemsetAsync) */
int sbgm_fill_zero(void* p, int64_t bytes, void* stream);
int sbgm_mha_core_bwd(const float* qkv, const float* dout, float* dqkv, int B, int S, int C, int heads, void* stream);
int sbgm_upsample2x_bwd(const float* dy, float* dx, int B, int H, int W, int C, void* stream);
/* nn.Upsample(scale_factor = scale, mode="bilinear", align_corners=False) over NHWC for any integer scale in 1..16 — DecoderBlock's
 * `upsample_scale` argument (score_unet.py:420, :467; the Decoder only ever passes 2, which has the kernels above).  x [B,H,W,C] ->
 * y [B,scale*H,scale*W,C]; _bwd: dy [B,scale*H,scale*W,C] -> dx [B,H,W,C] (a gather: no atomics, no zeroing needed). */
int sbgm_upsample_bilinear_fwd(const float* x, float* y, int B, int H, int W, int C, int scale, void* stream);
int sbgm_upsample_bilinear_bwd(const float* dy, float* dx, int B, int H, int W, int C, int scale, void* stream);
int sbgm_conv3x3_cout1_bwd(const float* dout, const float* a, const float* w_tap_c, const float* t, float sigma, float* da,
                           float* dw_tap_c, float* dbias, int B, int H, int W, int C, void* stream);
int sbgm_time_proj_bwd(const float* dout, const float* weight, const float* semb, const float* emb_raw, float* dW,
                       float* dbias, float* demb_accum /* NULL or [B,D], accumulated */, int B, int D, int ch, void* stream);
/* dW / dbias of up to 16 projections in one launch (HOST arrays of device pointers; projection i: douts[i] [B, chs[i]], sembs[i] [B, D]
 * = silu(embedding) it read, dWs[i] [chs[i], D], dbiases[i] [chs[i]]).  The embedding gradient (label embedding only) stays with
 * sbgm_time_proj_bwd. */
int sbgm_time_proj_multi_bwd(const float* const* douts, const float* const* sembs, float* const* dWs, float* const* dbiases,
                             const int* chs, int n_proj, int B, int D, void* stream);
int sbgm_label_emb_bwd(const float* demb, const int64_t* y, float* dtable, int B, int D, void* stream);
int sbgm_act_fwd(const float* x, float* y, int64_t n, int act, void* stream);
int sbgm_act_bwd(const float* x, const float* dy, float* dx, int64_t n, int act, void* stream);

/* ---- the loss around the network: loss_fn (reference score_unet.py:936-985) --------------------------------------------
 * perturb: t_b = U(0,1)*(1-t_eps)+t_eps, z ~ N(0,1), std_b = marginal_prob_std(t_b), x_perturbed = x + std_b*z  (:957-963).
 *   z / t given (device tensors [B,1,H,W] / [B]): used verbatim (parity runs inject the reference's draws; z_out is then not
 *   written and may be NULL).  Either NULL: drawn in the kernel with Philox keyed by `seed` (rng_state NULL; eager calls pass a
 *   fresh seed per call) or by rng_state = device uint64[2] {seed, offset}; sbgm_dsm_loss_fwd advances that offset by one, so a
 *   captured (hipGraph) step replays with fresh noise.
 * loss_fwd: loss[0] = mean_b sum_{chw} w*(score*std_b + z)^2, w = sigmoid(sdf)*0.5+0.5 or 1 (sdf NULL)           (:974-984);
 *   partial_ws: >= 8 * B * sbgm_dsm_loss_blocks(per_sample) bytes (one fp64 partial per workgroup, summed in fixed order).
 * loss_bwd: dscore = dloss[0] * (2/B) * w * (score*std_b + z) * std_b   (dloss: DEVICE scalar, autograd's grad_output). */
/* perturb with another schedule (loss_fn takes any marginal_prob_std callable, :936-985): call once with per_sample = 0 (only t_out is
 * drawn / copied), evaluate the schedule on t_out into std_out, call again with t = t_out and sigma <= 0: std_out is then READ. */
int sbgm_dsm_loss_blocks(int64_t per_sample);
int sbgm_dsm_perturb(const float* x, const float* z, const float* t, const uint64_t* rng_state, uint64_t seed, float t_eps, float sigma,
                     float* x_perturbed, float* z_out, float* t_out /* [B] */, float* std_out /* [B] */, int B,
                     int64_t per_sample, void* stream);
int sbgm_dsm_loss_fwd(const float* score, const float* z, const float* std, const float* sdf, void* partial_ws, float* loss,
                      uint64_t* rng_state /* advanced; may be NULL */, int B, int64_t per_sample, void* stream);
int sbgm_dsm_loss_bwd(const float* score, const float* z, const float* std, const float* sdf, const float* dloss, float* dscore,
                      int B, int64_t per_sample, void* stream);

/* Sampler updates with explicit scalars (the fused loop above uses a device-side table instead).
 * z NULL -> Philox draw keyed by (seed, draw_index).
 *   em:       x_mean = x + (g2*score)*dt ; x = x_mean + noise_coef*z            score_sampling.py:124-125, :224-227
 *   langevin: eps = 2*(snr_noise_norm / mean_b||score_b||)^2 ; x += eps*score + sqrt(2 eps)*z      :200-204
 *   cfg:      out = (1+w)*s_cond - w*s_uncond                                                        :55
 *   edm churn: x += churn_coef*z                     (EDM Heun, sbgm_sampler_run_edm)
 *   edm euler: d = -sigma_hat*score ; x_next = x_hat + (sigma_next - sigma_hat)*d
 *   edm heun:  x = x + (sigma_next - sigma_hat)*0.5*(d - sigma_next*score)   (x holds x_hat on entry)
 *   dpmpp 2m:  D = x + sigma^2*score ; x = c_x*x + c_0*D + c_1*hist + c_z*z ; hist = D     (sbgm_sampler_run_dpmpp)
 *              hist is read only when c_1 != 0 (it may hold anything on the first step); a draw is taken only when z is given or
 *              c_z != 0.  A constrained loop follows it with sbgm_hold_known.                                          */
int sbgm_em_step(float* x, float* x_mean, const float* score, const float* z, float g2, float dt, float noise_coef,
                 uint64_t seed, uint64_t draw_index, int64_t n, void* stream);
int sbgm_langevin_step(float* x, const float* score, const float* z, float snr_noise_norm, void* sumsq_ws /* >= 8*B B */,
                       uint64_t seed, uint64_t draw_index, int B, int64_t per_sample, void* stream);
int sbgm_cfg_combine(float* out, const float* s_cond, const float* s_uncond, float scale, int64_t n, void* stream);
int sbgm_randn_scaled(float* x, float scale, uint64_t seed, uint64_t draw_index, int64_t n, void* stream);
/* sbgm_randn_scaled under a noise plan (see sbgm_sampler_set_noise_rows): x [B][per_sample] = scale * z, sample b drawn as noise row
 * rows[b] and mixed over `lags` rows `stride` apart with `weights` (host fp32 [lags]).  per_sample % 4 == 0, 1 <= lags <= 32. */
int sbgm_randn_rows(float* x, float scale, uint64_t seed, uint64_t draw_index, const int32_t* rows, int B, int64_t per_sample, int stride,
                    const float* weights, int lags, void* stream);
/* The tiled draw under a domain noise plan (see sbgm_sampler_set_noise_domain_row): tiles [T][th][tw] = scale * z, tile t cut at
 * origins[t] = (y0, x0) (device int32 [T][2], x0 % 4 == 0) out of the mixed draw of the domain row *row_dev (ONE device int32) over a
 * domain of domain_h x domain_w (the padded width) pixels.  tw % 4 == 0, 1 <= lags <= 32; the origins and the row are read back and
 * checked (every tile inside the domain, row >= (lags - 1) stride), which waits for `stream`. */
int sbgm_randn_domain_rows(float* tiles, float scale, uint64_t seed, uint64_t draw_index, const int32_t* row_dev, const int32_t* origins,
                           int T, int th, int tw, int domain_h, int domain_w, int stride, const float* weights, int lags, void* stream);
int sbgm_edm_churn(float* x, const float* z, float churn_coef, uint64_t seed, uint64_t draw_index, int64_t n, void* stream);
int sbgm_edm_euler(const float* x_hat, const float* score, float* d, float* x_next, float sigma_hat, float sigma_next, int64_t n,
                   void* stream);
int sbgm_edm_heun(float* x, const float* d, const float* score, float sigma_hat, float sigma_next, int64_t n, void* stream);
int sbgm_dpmpp_2m_step(float* x, const float* score, float* hist, const float* z, float sigma, float c_x, float c_0, float c_1, float c_z,
                       uint64_t seed, uint64_t draw_index, int64_t n, void* stream);
/* The hold of constrained sampling as an op of its own, called after a step op above by loops that run the network themselves:
 * x = hold(x, known + level*z, m) and, when x_mean is not NULL, x_mean = hold(x_mean, known, m).  z NULL -> the Philox draw
 * (seed, draw_index), i.e. the draw the step op just consumed. */
int sbgm_hold_known(float* x, float* x_mean, const float* known, const float* known_mask, const float* z, float level, uint64_t seed,
                    uint64_t draw_index, int64_t n, void* stream);

/* The pieces of the RK45 solver above, for callers that run the network evaluations themselves (rk45_sampler's Python loop).
 * `state` is an opaque device block of sbgm_rk45_state_bytes bytes for `groups` controllers (1, or B with per_sample); K holds the seven
 * fp32 stage scores, slab s at K + s * k_stride (k_stride >= B * per, a multiple of 4); y, y_new are float64 [B * per]; partials is
 * a float64 scratch of sbgm_rk45_partials_bytes bytes.
 *   init:    resets the block for a run from t0 to t_bound.     load / store: y = float64(x) / x = fp32(y).
 *   stage:   writes the network input xs (fp32) and the time vector t_dev[B] of the evaluation that `phase` leads to, whose score the
 *            caller then puts into slab: phase 7 -> slab 0 (f at t0), 8 -> slab 1 (the probe of the initial step), s = 1..5 -> slab s
 *            (Runge-Kutta stage s), 6 -> slab 6 (f at y_new, which it also stores).
 *   control: what = 0 after slab 0, 1 after slab 1 (the two halves of the initial step), 2 after slab 6: error norm and decision.
 *   commit:  after control 2: moves y_new and slab 6 into place if the attempt was accepted.
 *   read:    synchronises and returns stats_i [4 groups + 2] (per controller nfev, n_accepted, n_rejected, status; then the done word
 *            and the attempts that found a controller running) and stats_d [groups] (current t; may be NULL). */
int64_t sbgm_rk45_state_bytes(int groups);
int64_t sbgm_rk45_partials_bytes(int B, int64_t per);
int sbgm_rk45_init(void* state, int groups, double t0, double t_bound, double rtol, double atol, float sigma, int64_t max_steps,
                   void* stream);
int sbgm_rk45_load(double* y, const float* x, int64_t n, void* stream);
int sbgm_rk45_store(float* x, const double* y, int64_t n, void* stream);
int sbgm_rk45_stage(void* state, int phase, const double* y, double* y_new, const float* K, int64_t k_stride, float* xs, float* t_dev,
                    int B, int64_t per, int per_sample, void* stream);
int sbgm_rk45_control(void* state, int what, const double* y, const double* y_new, const float* K, int64_t k_stride, double* partials,
                      int B, int64_t per, int per_sample, void* stream);
int sbgm_rk45_commit(const void* state, double* y, const double* y_new, float* K, int64_t k_stride, int B, int64_t per, int per_sample,
                     void* stream);
int sbgm_rk45_read(const void* state, int groups, int64_t* stats_i, double* stats_d, void* stream);

/* ---- after the sampler -------------------------------------------------------------------------
 * sbgm_pointwise_chain: y[i] = program(x[i]); the program is at most SBGM_CHAIN_MAX_OPS scalar steps, each rounded to fp32
 * on its own exactly like the reference's tensor-scalar arithmetic.  Replaces the __call__ bodies of Scale /
 * ScaleBackTransform (special_transforms.py:87-100, :125-139), ZScoreTransform / ZScoreBackTransform (:159-184, :202-233),
 * PrcpLogTransform / PrcpLogBackTransform (:288-355, :418-462) and the generation clamp (training.py:744-748).
 * x == y (in place) is allowed. */
enum { SBGM_OP_ADD = 0, SBGM_OP_MUL = 1, SBGM_OP_DIV = 2, SBGM_OP_CLAMP_MIN = 3, SBGM_OP_CLAMP_MAX = 4, SBGM_OP_EXP = 5,
       SBGM_OP_LOG = 6 };
#define SBGM_CHAIN_MAX_OPS 12
int sbgm_pointwise_chain(const float* x, float* y, int64_t n, int n_ops, const int* ops, const float* consts, void* stream);
/* Per-sample maximum and q-quantile (torch.quantile "linear" interpolation, NaN-propagating) of x[B][per_sample]:
 * the two statistics report_precip_extremes needs (utils.py:1647-1649).  out_max, out_q: device [B]. */
int sbgm_sample_extremes(const float* x, int B, int64_t per_sample, float q, float* out_max, float* out_q, void* stream);

/* ---- verification statistics (verify.hip) -------------------------------------------------------------
 * Inputs are fp32 [rows][HW] on the device, HW = H*W of any size.  A pixel of row n is VALID when gen/x is not NaN, obs/ref is
 * not NaN and the mask admits it (mask_is_u8: uint8 != 0; else fp32 > 0.5); every statistic uses valid pixels only (nanmean).
 * obs / ref / mask rows are 1 (broadcast) or one per row.  Float sums are fp64 per-wave partials added in a fixed order and
 * histograms are integer, so every output is bitwise reproducible.  `workspace` holds the partials; size it with the
 * *_workspace_bytes query.  Empty sets give NaN statistics.
 *
 * sbgm_error_stats: gen [N][HW] against obs [No][HW], mask [Nm][HW] or NULL.  Per pixel over samples: pix_count int32 [HW],
 * pix_mae, pix_rmse, pix_bias = mean(gen) - mean(obs) fp32 [HW].  Per sample over pixels: sample_stats fp64 [N][3] =
 * (count, MAE, RMSE).  global_stats fp64 [10] = (count, mean gen, mean obs, bias, MAE, RMSE, min gen, max gen, min obs,
 * max obs). */
int64_t sbgm_error_stats_workspace_bytes(int N, int64_t HW);
int sbgm_error_stats(const float* gen, const float* obs, const void* mask, int mask_is_u8, int N, int No, int Nm, int64_t HW,
                     int* pix_count, float* pix_mae, float* pix_rmse, float* pix_bias, double* sample_stats, double* global_stats,
                     void* workspace, void* stream);
/* sbgm_histogram: counts int64 [bins] (overwritten) of v = x, or |x - ref| when absdiff, over the valid pixels of x [N][HW]
 * (ref [Nr][HW] or NULL, mask [Nm][HW] or NULL).  Equal bins on [lo, hi] with numpy.histogram's range and closed-last-bin
 * convention and the floor rule: v is kept iff lo <= v <= hi and idx = floor(((double)v - lo) * bins / (hi - lo)) in fp64,
 * clamped to bins - 1 (v == hi falls in the last bin).  numpy also corrects indices against its linspace edges, so a value
 * within rounding of an interior edge can land one bin away from numpy's choice.  1 <= bins <= 8192. */
int sbgm_histogram(const float* x, const float* ref, const void* mask, int mask_is_u8, int N, int Nr, int Nm, int64_t HW,
                   int absdiff, double lo, double hi, int bins, int64_t* counts, void* stream);
/* sbgm_ensemble_scores: members ens [M][HW] (2 <= M <= 8191), truth obs [HW], mask [HW] or NULL.  A pixel with any NaN member
 * is invalid: its maps are NaN and its rank -1.  Per pixel: mean, var (ddof 1), crps (fair: (1/M) sum|x_i - y| -
 * sum_ij|x_i - x_j| / (2M(M-1))) fp32 [HW]; rank int32 [HW] of obs among the members, uniform on [#{x_i < y}, #{x_i <= y}]
 * from a Philox draw keyed by (seed, pixel).  rank_hist int64 [M+1] (overwritten).  scores fp64 [6] = (count, mean fair
 * CRPS, mean standard CRPS (c = 1/(2M^2)), skill = RMSE of the ensemble mean, spread = sqrt(mean var),
 * spread / skill * sqrt((M+1)/M)). */
int64_t sbgm_ensemble_scores_workspace_bytes(int64_t HW);
int sbgm_ensemble_scores(const float* ens, const float* obs, const void* mask, int mask_is_u8, int M, int64_t HW,
                         uint64_t seed, float* mean, float* var, float* crps, int* rank, int64_t* rank_hist, double* scores,
                         void* workspace, void* stream);
/* sbgm_radial_spectrum: power [F][H][W] = |fft2|^2 of mean-removed fields; fields with field_ok[f] == 0 (uint8 [F]) are
 * skipped.  With L = max(H, W) and fy, fx = numpy.fft.fftfreq (cycles per pixel), pixel (iy, ix) is in bin
 * k = rint(L * sqrt(fy^2 + fx^2)); bins 0..L/2 are kept, the corners dropped.  psd fp64 [L/2+1] = mean power per bin over
 * the kept fields, bin_count int64 [L/2+1] = pixels per bin, n_fields int64 [1] = fields used.  2 <= H, W <= 2048. */
int64_t sbgm_radial_spectrum_workspace_bytes(int H, int W);
int sbgm_radial_spectrum(const float* power, const unsigned char* field_ok, int F, int H, int W, double* psd, int64_t* bin_count,
                         int64_t* n_fields, void* workspace, void* stream);

/* ---- neighbourhood and threshold scores (verify_spatial.hip) -----------------------------------
 * Validity and masks as above; an event is v >= thr in fp32 at a valid pixel.  `thresholds` (T finite values) and `scales`
 * (S odd window widths n >= 1, in pixels) are HOST arrays; every other pointer is device memory.  All counts are integers,
 * so the outputs are exact and bitwise reproducible; the only atomics are 64-bit integer adds.
 *
 * sbgm_neighbourhood_scores: gen [N][H][W] against obs [No][H][W], mask [Nm][H][W] or NULL.  With I_g, I_o the event
 * images of field f at threshold t and C_g, C_o their sums over the n x n window around each of the H*W centres (zero beyond
 * the domain, never renormalised), num [N][T][S] = sum (C_g - C_o)^2 and den [N][T][S] = sum (C_g^2 + C_o^2): the Fractions
 * Skill Score's numerator and denominator without their common factor n^-4.  events_gen, events_obs [N][T] = sum I;
 * valid [N] = valid pixels.  fss_field fp64 [N][T][S] = 1 - num / den; fss fp64 [T][S] = 1 - (sum_f num) / (sum_f den), the
 * sums in fp64 in field order; both NaN where den is 0.  freq_bias fp64 [T] = sum events_gen / sum events_obs; fss_useful
 * fp64 [T] = 0.5 + (sum events_obs / sum valid) / 2.  The cost per (field, threshold, width) is O(H*W) whatever the width.
 * Limits: sides 2..2048, H*W <= 2^20 (so den <= 2^61 and a window count fits 32 bits), N <= 65535.  The fields are
 * processed in chunks, stream-ordered, so that the workspace never exceeds `workspace_bytes`;
 * sbgm_neighbourhood_scores_workspace_bytes gives the size to allocate for a cap of max_bytes (at least one field x one
 * threshold, at most all of them).  sbgm_neighbourhood_scores_strip_columns: columns one workgroup of the window pass owns. */
#define SBGM_SPATIAL_MAX_THRESHOLDS 16
#define SBGM_SPATIAL_MAX_SCALES 16
int sbgm_neighbourhood_scores_strip_columns(void);
int64_t sbgm_neighbourhood_scores_workspace_bytes(int N, int H, int W, int T, int S, int64_t max_bytes);
int sbgm_neighbourhood_scores(const float* gen, const float* obs, const void* mask, int mask_is_u8, int N, int No, int Nm, int H, int W,
                              const float* thresholds, int T, const int* scales, int S, int64_t* num, int64_t* den,
                              int64_t* events_gen, int64_t* events_obs, int64_t* valid, double* fss, double* fss_field,
                              double* freq_bias, double* fss_useful, void* workspace, int64_t workspace_bytes, void* stream);
/* sbgm_exceedance_scores: members ens [M][HW] (2 <= M <= 4095), truth obs [HW], mask [HW] or NULL; a pixel with any NaN
 * member is invalid.  Per threshold t and valid pixel, k = #{members >= thr} and o = [obs >= thr]: table int64 [T][M+1][2]
 * (overwritten), table[t][k][0] = pixels with that k, table[t][k][1] = those of them with o = 1 (the reliability diagram).
 * count int64 [1] = valid pixels.  scores fp64 [6][T], from the table alone with p_k = k / M: Brier score, Murphy's
 * reliability, resolution and uncertainty over the M + 1 probability values (reliability - resolution + uncertainty = Brier),
 * base rate, and the ROC area (trapezoids over the M + 1 cut-offs; NaN when the event never or always occurs).  No valid
 * pixel gives NaN.  The table is accumulated in place, so the workspace query returns 0 and `workspace` may be NULL. */
int64_t sbgm_exceedance_scores_workspace_bytes(int M, int64_t HW, int T);
int sbgm_exceedance_scores(const float* ens, const float* obs, const void* mask, int mask_is_u8, int M, int64_t HW,
                           const float* thresholds, int T, int64_t* table, int64_t* count, double* scores, void* workspace,
                           void* stream);
/* sbgm_ensemble_products (verify_products.hip): per-pixel products of members ens [M][HW]
 * (2 <= M <= 4095), mask [HW] or NULL.  A pixel is valid when no member is NaN there and the mask admits it; every map is
 * NaN at an invalid pixel and count int64 [1] = valid pixels.  `quantiles` (Q levels in [0, 1], fp64) and `thresholds` (T
 * finite values) are HOST arrays, 0 <= Q, T <= 16; with Q (T) = 0 the levels and `quant` (the values and `exceed`) may be NULL.
 * With the members of a pixel ordered by value, x_(0) <= ... <= x_(M-1) (-0 and +0 compare equal; a zero order statistic is
 * +0): vmin = x_(0), vmax = x_(M-1), exact.  quant [Q][HW], numpy's default (Hyndman-Fan type 7): h = q (M - 1),
 * lo = floor(h), g = h - lo, hi = min(lo + 1, M - 1) in fp64 on the host; with a = x_(lo), b = x_(hi) the value is a when
 * g == 0 or a == b, else (float)(a + g (b - a)) evaluated in fp64 -- so q = 0 is vmin and q = 1 is vmax bit for bit, and the
 * value lies in [a, b].  exceed [T][HW] = (float)((double)k / M), k = #{x_i >= thr} in fp32.  mean = (float)(sum x_i / M)
 * and std = (float)sqrt(sum (x_i - mean64)^2 / (M - 1)), both sums in fp64 in member order, the second against the unrounded
 * fp64 mean.  The order statistics, quant and exceed do not depend on the order of the members; two calls give bit-equal
 * outputs (no float atomics).  Cost: 2 + 32 ceil(Q / 8) sweeps over the members, each read coalesced; every statistic
 * lives in registers, so the workspace query returns 0 and `workspace` may be NULL. */
#define SBGM_PRODUCTS_MAX_QUANTILES 16
#define SBGM_PRODUCTS_MAX_THRESHOLDS 16
int64_t sbgm_ensemble_products_workspace_bytes(int M, int64_t HW, int Q, int T);
int sbgm_ensemble_products(const float* ens, const void* mask, int mask_is_u8, int M, int64_t HW,
                           const double* quantiles, int Q, const float* thresholds, int T,      /* HOST arrays */
                           float* mean, float* std, float* vmin, float* vmax,                    /* [HW] */
                           float* quant /* [Q][HW] */, float* exceed /* [T][HW] */, int64_t* count /* [1] */,
                           void* workspace, void* stream);

/* ---- object-based verification (verify_objects.hip) ----------------------------------------------
 * Validity and masks as above.  For a side F in {gen, obs} an object pixel is a valid pixel with F >= thr in fp32; objects are
 * the 4- or 8-connected components (`connectivity`) of the object pixels.  Limits: sides 2..2048, H*W <= 2^20, N <= 65535.
 *
 * sbgm_object_labels: fields [N][H][W], mask [Nm][H][W] or NULL -> labels int32 [N][H][W]: 1 + the smallest linear index
 * row * W + col of the pixel's object, 0 for background.  The labels array is the only working memory.
 *
 * sbgm_object_scores: gen [N][H][W] against obs [No][H][W]; index 0 of every [2] axis is gen, 1 is obs.  `thresholds` is a
 * HOST array of n_fixed finite values (0..16), used on both sides; with has_relative, one more threshold index follows them:
 * thr = (float)(rel_factor * q) with q the type-7 quantile (level rel_quantile; exact order statistics, fp64 interpolation,
 * rounded to fp32 as sbgm_ensemble_products defines it) of that side's valid values >= rel_wet of that field, NaN (no
 * objects) when there is none.  T = n_fixed + has_relative >= 1.  Per object n: area a_n, mass R_n = sum F, peak Rmax_n,
 * centre x_n = sum F (row, col) / R_n.  Outputs: threshold fp32 [2][N][T]; n_objects, area int64 [2][N][T]; mass = sum_n R_n,
 * V = sum_n R_n (R_n / Rmax_n) / mass, r = sum_n R_n |x - x_n| / mass fp64 [2][N][T]; domain_mean fp64 [2][N] = mean of F
 * over the valid pixels; com fp64 [2][N][2] = x, the F-weighted centre of the valid pixels; valid int64 [N]; with
 * d = sqrt((H-1)^2 + (W-1)^2): S = (V_g - V_o) / (0.5 (V_g + V_o)), L2 = 2 |r_g - r_o| / d, L = L1 + L2 fp64 [N][T];
 * A = (D_g - D_o) / (0.5 (D_g + D_o)), L1 = |x_g - x_o| / d fp64 [N]; a score is NaN where a denominator is 0, S and L2 where
 * either side has no object, A and L1 where there is no valid pixel or a side sums to 0.  area_hist int64 [2][T][21]: objects
 * with floor(log2 a_n) = b, over all fields.  status int32 [1]: 0, or SBGM_OBJECTS_STATUS_* bits when a union-find walk hit
 * its step cap (a bug; the results are then not to be used).  Each pixel enters the sums as a 31-bit fixed-point integer
 * scaled to its field's largest magnitude: exact for values that are multiples of 2^-8 below 256, within (vmax / thr) 2^-30
 * relative otherwise; integer atomics only, fp64 sums in a fixed order, so two calls are bit-equal.  The (field, threshold)
 * pairs are processed in chunks, stream-ordered, within `workspace_bytes`; sbgm_object_scores_workspace_bytes gives the size
 * to allocate for a cap of max_bytes (at least one pair, at most all).  The result does not depend on the chunking. */
#define SBGM_OBJECTS_MAX_THRESHOLDS 16
#define SBGM_OBJECTS_AREA_BINS 21
#define SBGM_OBJECTS_STATUS_MERGE_CAP 1
#define SBGM_OBJECTS_STATUS_FIND_CAP 2
int sbgm_object_labels(const float* fields, const void* mask, int mask_is_u8, int N, int Nm, int H, int W, float threshold,
                       int connectivity, int* labels, int* status, void* stream);
int64_t sbgm_object_scores_workspace_bytes(int N, int H, int W, int T, int64_t max_bytes);
int sbgm_object_scores(const float* gen, const float* obs, const void* mask, int mask_is_u8, int N, int No, int Nm, int H, int W,
                       const float* thresholds, int n_fixed, int has_relative, double rel_factor, double rel_quantile, float rel_wet,
                       int connectivity, float* threshold, int64_t* n_objects, int64_t* area, double* mass, double* V, double* r,
                       double* domain_mean, double* com, int64_t* valid, double* S, double* L2, double* A, double* L1, double* L,
                       int64_t* area_hist, int* status, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- multivariate ensemble scores (verify_multivariate.hip) -----------------------------------------
 * Members ens [M][HW] (2 <= M <= 4095, HW <= 2^20) against the truth obs [HW], mask [HW] or NULL.  A pixel is valid when every
 * member and the truth are not NaN there and the mask admits it; an invalid pixel contributes nothing.  Both calls keep the
 * valid flags, the partial sums and nothing else in `workspace` (size from the _workspace_bytes query, which returns 0 for
 * arguments the call would reject), use no floating-point atomics and sum in an order that depends on the arguments alone:
 * two calls give bit-equal outputs.
 *
 * sbgm_energy_scores: dist2 fp64 [M+1][M+1], the squared Euclidean distances over the valid pixels between all members and
 * the truth (row / column M): every fp32 value converted to fp64 once, then d = a - b, sum = fma(d, d, sum) — the difference
 * form, so a duplicated member gives an exact 0.  Symmetric bit for bit with a zero diagonal.  scores fp64 [6]: count (valid
 * pixels); es_fair = (1/M) sum_m |x_m - y| - 1/(2 M (M-1)) sum_{m != k} |x_m - x_k|; es_standard, the same with 1/(2 M^2);
 * mean_dist_obs = (1/M) sum_m |x_m - y|; mean_dist_pair = 1/(M (M-1)) sum_{m != k} |x_m - x_k|; min_dist_pair = min_{m != k}
 * |x_m - x_k|.  Every norm is |a - b| = sqrt(dist2 / count), an RMS distance.  count = 0 gives dist2 = 0 and NaN scores.
 *
 * sbgm_variogram_scores (Scheuerer & Hamill 2015): the pixel pairs (i, j = i + (dy, dx)) with (dy, dx) in the half-plane
 * (dy > 0, or dy == 0 and dx > 0) and dy^2 + dx^2 <= radius^2, radius 1..8, in the order sbgm_variogram_offsets lists them
 * (dy ascending, then dx ascending; at most 98), both pixels valid and inside the field.  For such a pair g_ens = (1/M) sum_m
 * |x_i^m - x_j^m|^p and g_obs = |y_i - y_j|^p — the difference and its power (p = order: 0.5, 1 or 2, nothing else) in fp32,
 * the sum over the members and everything after it in fp64 — and term = (g_obs - g_ens)^2.  With w = 1, or 1 / sqrt(dy^2 +
 * dx^2) (rounded to fp32) when inverse_distance != 0: vs_map fp32 [H][W] = sum of w term over the pairs a pixel owns (its
 * half-plane neighbours), NaN at an invalid pixel; gamma_ens, gamma_obs fp64 [n_off] = mean of g_ens, g_obs over the pairs of
 * an offset (NaN without pairs); pairs int64 [n_off]; scores fp64 [4]: vs = sum w term / sum w, n_pairs, sum_w (both sums
 * over the counted pairs), vs_unweighted = sum term / n_pairs. */
#define SBGM_VARIOGRAM_MAX_OFFSETS 98
int64_t sbgm_energy_scores_workspace_bytes(int M, int64_t HW);
int sbgm_energy_scores(const float* ens, const float* obs, const void* mask, int mask_is_u8, int M, int64_t HW,
                       double* dist2 /* [M+1][M+1] */, double* scores /* [6] */, void* workspace, int64_t workspace_bytes,
                       void* stream);
/* HOST arrays: *n_offsets and dydx [n_offsets][2] (room for SBGM_VARIOGRAM_MAX_OFFSETS pairs) */
int sbgm_variogram_offsets(int radius, int* n_offsets, int* dydx);
int64_t sbgm_variogram_scores_workspace_bytes(int M, int H, int W, int radius);
int sbgm_variogram_scores(const float* ens, const float* obs, const void* mask, int mask_is_u8, int M, int H, int W, int radius,
                          double order, int inverse_distance, float* vs_map /* [H][W] */, double* gamma_ens, double* gamma_obs,
                          int64_t* pairs /* [n_off] each */, double* scores /* [4] */, void* workspace, int64_t workspace_bytes,
                          void* stream);

/* ---- climate indices over time (verify_temporal.hip) ------------------------------------------------
 * sbgm_climate_indices: per-pixel indices along the day axis of gen [N][H][W] against obs [N][H][W] (2 <= N <= 4095, the field
 * limits above), mask NULL, [H][W] (Nm = 1) or [N][H][W] (Nm = N).  Day t is valid at pixel p when gen and obs are both not NaN
 * there and the mask admits (t, p): validity is paired, both sides use the same days.  A valid day is wet on a side when its
 * value is >= wet (fp32), else dry.  Index 0 of every [2] axis is gen, 1 is obs; every float map is NaN where undefined.
 *   days int32 [HW]: n, the valid days.
 *   stats fp32 [2][7][HW], in the order of SBGM_TEMPORAL_STAT_*: mean = sum / n; wet_freq = n_wet / n; sdii = sum over the wet
 *     days / n_wet; max (on the order-preserving key, -0 folded onto +0); p_ww = n_ww / (n_ww + n_wd); p_dw = n_dw / (n_dw +
 *     n_dd); lag1 = c1 / c0 with c0 = sum (x - mu)^2 / n and c1 = sum over the valid adjacent pairs (x_t - mu)(x_t+1 - mu) /
 *     n_pairs against the unrounded fp64 mean mu (NaN when n_pairs = 0 or c0 = 0).  Every sum is fp64 in day order, a product
 *     is one multiply followed by one add, every quotient one fp64 division rounded to fp32 once.
 *   spells int32 [2][2][HW]: cwd, cdd, the longest run of consecutive valid wet (dry) days; an invalid day ends a run.
 *   transitions int32 [2][4][HW]: n_ww, n_wd, n_dw, n_dd over the pairs (t, t+1) with both days valid.
 *   quant fp32 [2][Q][HW]: numpy's default quantile (Hyndman-Fan type 7) over the n valid days of the pixel: h = q (n - 1),
 *     lo = floor(h), g = h - lo, hi = min(lo + 1, n - 1) in fp64; a = x_(lo), b = x_(hi); a when g == 0 or a == b, else
 *     (float)(a + g (b - a)) in fp64 -- sbgm_ensemble_products' expression with the pixel's own n.
 *   wet_quant fp32 [2][QW][HW]: the same over the n_wet valid wet days of the side (NaN when n_wet = 0).
 *   heavy fp32 [2][QW][HW] (ETCCDI R95pTOT family): sum over the valid days with x > tau of x / sum over the valid wet days of
 *     x, tau = the OBS side's wet_quant map at that pixel for both sides; NaN where tau is NaN or the side's wet total is 0.
 * `quantiles` and `wet_quantiles` are HOST arrays of Q, QW levels in [0, 1], 0 <= Q, QW <= 8; with a count of 0 the levels and
 * the maps may be NULL.  The workspace (size from the query, which returns 0 for arguments the call would reject) holds the
 * validity bits of every (day, pixel) and the wet-day counts.  No float atomics: two calls give bit-equal outputs.  Cost: 2
 * sweeps over both sides, 32 more over each side per non-empty level list, one more over each side when QW > 0. */
#define SBGM_TEMPORAL_MAX_DAYS 4095
#define SBGM_TEMPORAL_MAX_QUANTILES 8
enum { SBGM_TEMPORAL_STAT_MEAN = 0, SBGM_TEMPORAL_STAT_WET_FREQ, SBGM_TEMPORAL_STAT_SDII, SBGM_TEMPORAL_STAT_MAX,
       SBGM_TEMPORAL_STAT_P_WW, SBGM_TEMPORAL_STAT_P_DW, SBGM_TEMPORAL_STAT_LAG1, SBGM_TEMPORAL_STATS };
int64_t sbgm_climate_indices_workspace_bytes(int N, int H, int W, int Q, int QW);
int sbgm_climate_indices(const float* gen, const float* obs, const void* mask, int mask_is_u8, int N, int Nm, int H, int W,
                         float wet, const double* quantiles, int Q, const double* wet_quantiles, int QW,   /* HOST arrays */
                         int* days, float* stats, int* spells, int* transitions, float* quant, float* wet_quant, float* heavy,
                         void* workspace, int64_t workspace_bytes, void* stream);

/* sbgm_climate_indices_calendar: the same indices with a calendar and with groups of days (K61, then K55 - K57 over slabs).
 *   day_numbers: NULL, or a DEVICE int32 [N], strictly increasing (the caller checks that).  Day t is LINKED to day t - 1 iff
 *     day_numbers[t] == day_numbers[t-1] + 1; NULL links every adjacent pair.  A broken link between day t - 1 and day t acts
 *     exactly as one invalid day inserted between them: it ends a wet or dry run, and no transition and no lag-1 product spans
 *     it.  It counts nowhere else: not in n, the sums, the quantiles or heavy.
 *   groups: NULL (G = 0), or a DEVICE int32 [N] of ids in 0..G-1, 1 <= G <= 16.  The indices of group g are the calendar-aware
 *     indices of the subsequence of the days with id g, which keeps its own day numbers (positions when day_numbers is NULL):
 *     a link is also broken where consecutive days of the group are not consecutive days of the record.  The group has its own
 *     mean in lag1 and its own obs wet_quant map as tau of heavy.  A day whose id lies outside 0..G-1 joins no group; a group
 *     of 0 or 1 days follows the rules for n = 0 or n = 1.
 * The group outputs carry a leading [G] axis on the layout of the ungrouped ones (group_days [G][HW], group_stats
 * [G][2][7][HW], ...); they may be NULL when G = 0, the quantile ones also when their count is 0.  With day_numbers and groups
 * NULL this is sbgm_climate_indices, bit for bit, on that function's workspace size.  The fp64 operations and their order are
 * those of sbgm_climate_indices on the subsequence with an all-NaN day inserted at every broken link.  Cost: every group slab
 * walks only its own days, so a grouped call sweeps the record twice where the ungrouped call sweeps it once, whatever G is
 * (measured at 589 x 789 with four seasons: 1.45 - 1.58 times the ungrouped call). */
#define SBGM_TEMPORAL_MAX_GROUPS 16
int64_t sbgm_climate_calendar_workspace_bytes(int N, int H, int W, int Q, int QW, int G);
int sbgm_climate_indices_calendar(const float* gen, const float* obs, const void* mask, int mask_is_u8, int N, int Nm, int H, int W,
                                  float wet, const double* quantiles, int Q, const double* wet_quantiles, int QW, /* HOST arrays */
                                  const int* day_numbers, const int* groups, int G,                      /* DEVICE int32 [N] or NULL */
                                  int* days, float* stats, int* spells, int* transitions, float* quant, float* wet_quant,
                                  float* heavy, int* group_days, float* group_stats, int* group_spells, int* group_transitions,
                                  float* group_quant, float* group_wet_quant, float* group_heavy, void* workspace,
                                  int64_t workspace_bytes, void* stream);

/* ---- period climate indices (verify_periods.hip) ------------------------------------------------------
 * sbgm_period_indices: RxNday, RNNmm and PRCPTOT per pixel along the day axis, over the record and per period (a year, a season
 * of a year, a month of a year), for M member series and one truth series.  Member m of day t is read at gen + m * member_stride
 * + t * day_stride (strides in elements, day_stride >= H*W, member_stride >= H*W when M > 1; the H*W pixels of a field are
 * dense), obs is [N][H][W]; 2 <= N <= 4095, 1 <= M <= 4095, the field limits above; mask NULL, [H][W] (Nm = 1) or [N][H][W]
 * (Nm = N).  Series s = 0..M-1 are the members, s = M is obs: every [M+1] axis below is in that order.
 *   Validity is paired over everything: day t is valid at pixel p when the mask admits it, obs[t][p] is not NaN and gen[m][t][p]
 *     is not NaN for EVERY member m, so days, the period day counts and which windows exist are one map for all series.
 *   Run length r[t] = valid[t] ? (linked[t] ? r[t-1] : 0) + 1 : 0, r[-1] = 0; linked[t] iff day_numbers[t] == day_numbers[t-1]
 *     + 1 (DEVICE int32 [N], strictly increasing, the caller checks that; NULL: true for t > 0).  A broken link acts as one
 *     invalid day in between, the rule of sbgm_climate_indices_calendar.
 *   Window K ending on day t exists iff r[t] >= K.  Its sum is S = ((((+0.0 + x[t-K+1]) + x[t-K+2]) + ...) + x[t]) in fp64,
 *     oldest day first, each fp32 value widened first, FP contraction off; starting from +0.0 makes -0 impossible.
 *   windows: HOST int [Kw], 1 <= Kw <= 4 distinct ascending lengths in 1..32.  thresholds: HOST float [T], 0 <= T <= 8, finite.
 *   days int32 [HW]: the valid days.
 *   rx fp32 [M+1][Kw][HW]: the largest S over the windows that exist (best = S where best is NaN or S > best, in day order),
 *     rounded to fp32 once; NaN where none exists.  K = 1 is Rx1day, K = 5 Rx5day.
 *   count int32 [M+1][T][HW]: the valid days with x >= threshold_j, compared in fp32 (R10mm at 10).
 *   prcptot fp32 [M+1][HW]: the fp64 sum in day order over the valid days with x >= wet, rounded once; 0 where there is a valid
 *     day and no wet one, NaN where days = 0.
 * periods: NULL (P = 0), or a DEVICE int32 [N] of ids in -1..P-1, 1 <= P <= 256, in any order; ids may recur or stay unused; -1
 * (or any id outside 0..P-1) belongs to no period.  For period g: period_days [P][HW] counts the valid days with id g; count and
 * prcptot run over those days; rx runs over the windows whose LAST day has id g -- a window may reach back into days of another id
 * or of id -1 as long as its K days are linked and valid (a running sum over the record, then a maximum per year, as climdex
 * does).  This differs from the subsequence rule of the groups of sbgm_climate_indices_calendar.  period_rx [M+1][P][Kw][HW],
 * period_count [M+1][P][T][HW], period_prcptot [M+1][P][HW].  An id no day carries gets period_days 0, count 0 and NaN floats.
 * Across the periods, for each index i (the Kw windows, then the T thresholds, then prcptot; I = Kw + T + 1): period g counts
 * when period_days[g] >= min_days (>= 1) and its value is not NaN.  across_n int32 [M+1][I][HW]: the counting periods;
 * across_mean fp32: the fp64 sum of the fp32 values (counts as exact doubles) in id order / n, rounded once, NaN for n = 0;
 * across_std fp32: sqrt(sum (v - mean)^2 / (n - 1)) against the unrounded mean, NaN for n < 2.
 * Every element of every output is written.  With P = 0 the period and across outputs may be NULL, with T = 0 the count maps.
 * The workspace (size from the query, which returns 0 for arguments the call would reject) holds the validity bits, one word
 * per day and the wet-day sums of every (series, period, pixel) in fp64: (M + 1) * P * H*W * 8 bytes of it grow with P.  No
 * atomics: two calls give bit-equal outputs.  Cost: one pass over all series for validity, one for the sweep. */
#define SBGM_PERIOD_MAX_WINDOWS 4
#define SBGM_PERIOD_MAX_WINDOW 32
#define SBGM_PERIOD_MAX_THRESHOLDS 8
#define SBGM_PERIOD_MAX_PERIODS 256
#define SBGM_PERIOD_MAX_MEMBERS 4095
int64_t sbgm_period_indices_workspace_bytes(int N, int M, int H, int W, int Kw, int T, int P);
int sbgm_period_indices(const float* gen, int64_t member_stride, int64_t day_stride, const float* obs, const void* mask,
                        int mask_is_u8, int N, int Nm, int M, int H, int W, const int* windows /* HOST */, int Kw,
                        const float* thresholds /* HOST */, int T, float wet, int min_days,
                        const int* day_numbers, const int* periods, int P,                        /* DEVICE int32 [N] or NULL */
                        int* days, float* rx, int* count, float* prcptot, int* period_days, float* period_rx, int* period_count,
                        float* period_prcptot, int* across_n, float* across_mean, float* across_std, void* workspace,
                        int64_t workspace_bytes, void* stream);

/* ---- pooled ensemble verification of a series (verify_series.hip) --------------------------------------
 * sbgm_series_scores: D days (1 <= D <= 4095) of M members (2 <= M <= 4095) E[d][m][p] against one truth Y[d][p] per day, pooled
 * over days x pixels.  Member (d, m) is read at ens + d * day_stride + m * member_stride (strides in elements, each >= H*W; the H*W
 * pixels of a field are dense), so [D][M][H][W] and [M][D][H][W] both work without a copy.  obs [D][H][W]; mask NULL, [H][W]
 * (Nm = 1) or [D][H][W] (Nm = D); the field limits above.  groups: NULL (G = 0) or a DEVICE int32 [D] of ids in 0..G-1,
 * G <= 16 (an id outside is the caller's error; the kernels clamp it, so nothing is written out of bounds).  thresholds: a HOST
 * array of 0 <= T <= 16 finite values.  A cell (d, p) is valid when Y and every member are not NaN there and the mask admits it;
 * n_p = the valid days of pixel p.  Per valid cell, in fp64 and in sbgm_ensemble_scores' op order: mean, var (ddof 1),
 * crps_fair, crps_std, se = (mean - y)^2 and the randomised rank r in {lt..le}, its draw keyed by (seed, d, p), so day 0 draws
 * what sbgm_ensemble_scores draws.  Row 0 of every [G+1] axis is all days, row 1 + g is group g.
 *   count int32 [HW]: n_p.
 *   maps fp32 [4][HW], NaN where n_p = 0: crps = sum_d crps_fair / n_p; spread = sqrt(sum var / n_p); skill = sqrt(sum se / n_p);
 *     ssr = sqrt((M+1)/M) spread / skill.  Each sum is fp64 in day order in one thread, rounded to fp32 once.
 *   daily fp64 [D][6]: sbgm_ensemble_scores' scores over the valid pixels of each day.
 *   scores fp64 [G+1][6]: the same over the valid cells of the row's days.
 *   rank_hist int64 [G+1][M+1]; table int64 [G+1][T][M+1][2], sbgm_exceedance_scores' table over the row's cells; both exact.
 *   exceedance fp64 [G+1][6][T]: sbgm_exceedance_scores' scores of each row's table.
 * With climatology != 0 the reference forecast for day d at pixel p is the leave-one-out ensemble of the truth on the other valid
 * days of the same row at p (row 0: all days; a group row: the group's days).  With S the sum over the ordered pairs of those n
 * days of |y_i - y_j|, the reference's fair CRPS summed over the days is C = S / (2 (n - 1)); it needs n >= 3.
 *   clim_maps fp32 [2][HW]: clim_crps = C_p / n_p; crpss = (float)(1 - F_p / C_p), F_p = sum_d crps_fair.  NaN where n_p < 3;
 *     crpss also where C_p = 0.
 *   skill_scores fp64 [G+1][4]: (cells, mean forecast fair CRPS, mean reference CRPS, 1 - sum F / sum C) over the cells of the
 *     pixels with n >= 3 in that row; the means NaN without cells, the last also when sum C = 0.
 * With T = 0 thresholds, table and exceedance may be NULL; with climatology = 0, clim_maps and skill_scores.  The workspace
 * (size from the query, which returns 0 for arguments the call would reject) holds the per-pixel sums, the validity bits, the
 * per-group per-pixel sums and the per-wave partials of one chunk of days: the days are worked through in chunks that keep it
 * within max_bytes (at least 32 days a chunk), and no output depends on the chunking.  No float atomics: two calls give
 * bit-equal outputs.  Cost: M / 16 + 2 sweeps over the members; the climatology is O(n_p^2 / 2) per pixel. */
#define SBGM_SERIES_MAX_GROUPS 16
int64_t sbgm_series_scores_workspace_bytes(int D, int M, int H, int W, int T, int G, int climatology, int64_t max_bytes);
int sbgm_series_scores(const float* ens, int64_t day_stride, int64_t member_stride, const float* obs, const void* mask,
                       int mask_is_u8, int Nm, const int* groups /* DEVICE */, int G, int D, int M, int H, int W,
                       const float* thresholds /* HOST */, int T, uint64_t seed, int climatology, int* count, float* maps,
                       double* daily, double* scores, int64_t* rank_hist, int64_t* table, double* exceedance, float* clim_maps,
                       double* skill_scores, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- before the network ------------------------------------------------------------------------
 * Batch-level condition assembly: channel concatenation of the sorted *_lr fields (utils.py:441-447), classifier-free-
 * guidance condition dropout (data_modules.py:957-983: LR fields -> 0, class label -> NULL token 0) and the value||mask
 * layout of the geo fields (data_modules.py:971-993: mask 0 when dropped, 1 otherwise), one launch group per batch.
 * All tensors NCHW fp32 on the device; dropped: uint8 [B] (NULL = nothing dropped); any input group may be NULL/absent. */
#define SBGM_ASSEMBLE_MAX_LR 16
typedef struct sbgm_assemble_args {
    int B;
    int64_t HW;                               /* H*W, a multiple of 4 */
    int n_lr;                                 /* number of LR fields, already in sorted-key order */
    const float* lr[SBGM_ASSEMBLE_MAX_LR];    /* each [B][lr_channels[k]][H][W] */
    int lr_channels[SBGM_ASSEMBLE_MAX_LR];
    const float* lsm;  int lsm_channels;      /* [B][1 or 2][H][W] */
    const float* topo; int topo_channels;
    const int64_t* y;                         /* [B] class labels */
    const unsigned char* dropped;             /* [B] */
    float* lr_out;                            /* [B][sum lr_channels][H][W] */
    float* lsm_out;                           /* [B][2][H][W] */
    float* topo_out;                          /* [B][2][H][W] */
    int64_t* y_out;                           /* [B] */
} sbgm_assemble_args;
int sbgm_assemble_conditions(const sbgm_assemble_args* a, void* stream);

/* ---- device-resident cutout batches (cutout.hip) ------------------------------------------------
 * The per-sample host work of the reference's dataset (data_modules.py:727-997) for fields that live on the device as stacks
 * [N][Hd][Wd] (one plane per day) and static planes [Hd][Wd].  Every op is stream-ordered without a host synchronisation.
 *
 * sbgm_cutout_draw: find_rand_points (data_modules.py:184-223) for B samples.  rect: HOST int [4] = [r0, r1, c0, c1], rows first,
 * end-exclusive, inside the Hd x Wd domain; crop h x w no larger than it (both checked on the host).  origins: device int32 [B][2] =
 * (y0, x0).  Sample b takes the uniforms of Philox block (seed, offset = draw, idx = b): y0 = r0 + min(max_off_y, (int)floorf(u_0 *
 * (float)(max_off_y + 1))), x0 likewise from u_1 with c0, max_off = extent - crop; every step in fp32.
 *
 * sbgm_cutout_gather: dst[f][b][0][y][x] = program_f(src[f][item][y0_b + y][x0_b + x]) for every field f in ONE launch, item = items[b]
 * for a stack (n_items[f] = N > 0) and 0 for a static plane (n_items[f] = 0).  At most 1 + SBGM_ASSEMBLE_MAX_LR stacks and 2 planes.
 * srcs, dsts (each dst [B][1][h][w]) and n_items are HOST arrays of n_fields entries.  programs: DEVICE int32
 * [n_fields][SBGM_CUTOUT_PROGRAM_WORDS], per field the steps and per-step fp32 rounding of sbgm_pointwise_chain (fill a host copy
 * with sbgm_cutout_program_init, which validates it, and upload it once); a field with is_mask set is binarised after its program
 * to v > 0.5 ? 1 : 0 (data_modules.py:874, :909).  items: device int32 [B]; origins: device int32 [B][2].  Any h, w >= 1; dst rows are
 * written as 16-byte vectors when w % 4 == 0 and every dst is 16-byte aligned.  A sample whose item or origin lies outside its stack
 * is filled with NaN.
 *
 * sbgm_domain_gather: the whole Hd x Wd domain of B days, right-padded to Wp columns for the full-domain tiler:
 * dst[f][b][0][y][x] = program_f(src[f][item][y][min(x, Wd - 1)]) for 0 <= y < Hd, 0 <= x < Wp, every field in ONE launch.  srcs, dsts,
 * n_items, programs (with is_mask) and items are those of sbgm_cutout_gather; each dst is [B][1][Hd][Wp].  The column is clamped before
 * the program runs; the program is pointwise, so the result is the replicate pad of the transformed field.  Wp >= Wd and Wp % 4 == 0
 * (any pad width, Wp - Wd >= 4 included) and every dst 16-byte aligned: dst rows are written as 16-byte vectors throughout.  Source
 * rows are Wd floats of any alignment, read as dwords at clamped columns, so no load reaches past its row.  A sample whose item lies
 * outside its stack is filled with NaN.
 *
 * sbgm_sdf_from_mask: generate_sdf + normalize_sdf (data_modules.py:93-118) of mask [B][h][w] (land = mask > 0), per sample:
 * D2 = the EXACT squared Euclidean distance in pixels to the nearest land pixel (0 on land; integer arithmetic, no search window),
 * raw = 10 land - sqrt(D2), sdf = (raw - min raw) / (max raw - min raw), sqrt and normalisation in fp64 per pixel, rounded once to fp32.
 * Two deliberate differences from the reference, on crops without a coastline: a sample with no sea gives sdf = 1 everywhere (reference:
 * 0 / 0 = NaN); a sample with no land gives sdf = 0 everywhere (reference: scipy's transform of an input without background, which is
 * not a distance to anything).  sdf: fp32 [B][h][w]; d2: int32 [B][h][w] or NULL (-1 throughout a sample with no land).  Sides <= 4096.
 * ws: sbgm_sdf_workspace_bytes(B, h, w) bytes (-1: bad shape), cleared by the op itself.  Three launches; the only atomics are integer
 * max / or, so two calls give bit-equal outputs. */
#define SBGM_CUTOUT_MAX_FIELDS (1 + SBGM_ASSEMBLE_MAX_LR + 2)
#define SBGM_CUTOUT_PROGRAM_WORDS (2 + 2 * SBGM_CHAIN_MAX_OPS)   /* n_ops, is_mask, ops[12] (int32), consts[12] (fp32) */
int sbgm_cutout_draw(uint64_t seed, uint64_t draw, int B, const int* rect, int h, int w, int Hd, int Wd, int* origins, void* stream);
int sbgm_cutout_program_init(int32_t* words_host, int n_ops, const int* ops, const float* consts, int is_mask);
int sbgm_cutout_gather(const float* const* srcs, float* const* dsts, const int* n_items, int n_fields, const int32_t* programs,
                       const int* items, const int* origins, int B, int Hd, int Wd, int h, int w, void* stream);
int sbgm_domain_gather(const float* const* srcs, float* const* dsts, const int* n_items, int n_fields, const int32_t* programs,
                       const int* items, int B, int Hd, int Wd, int Wp, void* stream);
int64_t sbgm_sdf_workspace_bytes(int B, int h, int w);
int sbgm_sdf_from_mask(const float* mask, float* sdf, int* d2, void* ws, int B, int h, int w, void* stream);

/* ---- full-domain tiling (no reference counterpart, specification in DESIGN.md) -----------------
 * origins: device int32 [T][2] = (y0, x0) of every tile; the host validates that each tile lies inside the domain.
 * extract: tiles[T][C][th][tw] <- domain[C][Hd][Wd].   stitch: domain <- normalised blend of the covering tiles with
 * linear ramps of `ramp_len` pixels on tile edges that are not domain edges. */
int sbgm_extract_tiles(const float* domain, const int* origins, float* tiles, int T, int C, int Hd, int Wd, int th, int tw,
                       void* stream);
int sbgm_stitch_tiles(const float* tiles, const int* origins, float* domain, int T, int C, int Hd, int Wd, int th, int tw,
                      int ramp_len, void* stream);
/* The score blend of a joint run (sbgm_sampler_run_joint) as an op of its own, out of place: out[t] at tile pixel p = the blend, at p's
 * domain position, of scores[t'] over every tile t' that covers it (the same device function the fused update kernels call); a pixel
 * only its own tile covers is copied.  scores, out: device fp32 [T][1][H][W], W % 4 == 0, x origins multiples of 4, out != scores. */
int sbgm_blend_tile_scores(const float* scores, const int* origins, float* out, int T, int H, int W, int domain_h, int domain_w,
                           int ramp_len, void* stream);

#ifdef __cplusplus
}
#endif
#endif
