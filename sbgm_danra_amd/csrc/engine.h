// Host-side engine: owns the repacked weights and the activation workspace, builds the launch sequence of one
// ScoreNet evaluation for a given (B, H, W) and runs the reverse-SDE sampler loops (optionally as a replayed
// hipGraph).  Mirrors, at the launch-sequence level, reference sbgm/score_unet.py:247-364 (Encoder.forward),
// :559-627 (DecoderBlock.forward), :733-758 (Decoder.forward), :829-879 (ScoreNet.forward) and
// sbgm/score_sampling.py:63-127 / :136-230.
//
// This header declares what the engine's three files share; each body of substance has one owner:
//   model.hip        the parameter table, the weights derived from it, the workspace rule, autotune, the profiled forward
//   forward.hip      conv / conv_pair / attention and the network evaluation, stage by stage
//   sampler_run.hip  the step tables, the run context, the step samplers, the RK45 driver and SamplerStore's bodies
#pragma once
#include <algorithm>
#include <array>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/sbgm_hip.h"
#include "common.h"
#include "kernels.h"

constexpr float BN_EPS = 1e-5f, BN_MOMENTUM = 0.1f, GN_EPS = 1e-5f, LN_EPS = 1e-5f;
const int FMAP_CH[5] = {64, 64, 128, 256, 512};   // score_unet.py:198

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
inline int pad_channels(int c) { return c <= 4 ? 4 : c <= 8 ? 8 : (int)align_up(c, 16); }

// ---- parameters ------------------------------------------------------------------------------------------------
enum ParamKind { P_VEC, P_CONV, P_COUT1, P_IGNORE, P_TCONV, P_VEC4 };   // TCONV: ConvTranspose2d(2,2) weight; VEC4: vector stored 4x
struct Param {
    std::string name;
    ParamKind kind = P_VEC;
    int64_t numel = 0;          // element count in reference layout
    int cout = 0, cin = 0, kh = 1, kw = 1, cs = 0;   // P_CONV geometry (cs = padded Cin)
    bool want_wino = false;     // P_CONV: keep the Winograd images the geometry has as well (sbgm_conv_image_floats)
    float* img[CONV_IMAGES] = {};      // engine storage: the packed images of a convolution weight; index 0 alone for every other kind
    size_t floats[CONV_IMAGES] = {};
    bool filled = false;
    struct Derived* feeds = nullptr;   // the derived image this tensor is a source of (set in build()), told of every upload
    bool keep_oihw = false; float* oihw = nullptr;   // ... which then keeps the tensor as uploaded (OIHW) to rebuild from
    float* dev() const { return img[IMG_IGEMM]; }
    ConvImages images() const { ConvImages w; std::copy(img, img + CONV_IMAGES, w.img); return w; }
    size_t storage_floats() const {
        size_t n = 0;
        for (size_t f : floats) n += align_up(f, 64);
        return n;
    }
    float* place(float* at) {   // lays the images out from `at`, returns the end
        for (int i = 0; i < CONV_IMAGES; ++i)
            if (floats[i]) { img[i] = at; at += align_up(floats[i], 64); }
        return at;
    }
};

struct ConvW { Param* w = nullptr; Param* b = nullptr; };          // weight (+ optional bias)
struct BNW { Param *g, *b, *rm, *rv; float *scale, *bias; };       // + folded eval scale/bias
struct LnFold;
struct AttnW {
    Param *ln1g, *ln1b, *ln2g, *ln2b, *inw, *inb, *outw, *outb, *f1w, *f1b, *f2w, *f2b; int C;
    LnFold *fold1 = nullptr, *fold2 = nullptr;      // ln1 -> in_proj and ln2 -> ff[0] as folded operands (owned by sbgm_model::ln_folds)
};
struct BlockW { ConvW c1, c2, ds; BNW bn1, bn2, dsbn; bool has_ds; int cin, cout, stride; };
struct DecW { ConvW up, conv; Param *n1g, *n1b, *n2g, *n2b, *freq, *tpw, *tpb; AttnW attn; bool has_attn; int cin, cout; };

// ---- weights derived from uploaded weights (bodies: model.hip) ---------------------------------------------------
// Several images are computed from uploaded tensors, lazily and outside any captured step (who rebuilds which: refresh_derived).  The
// folded BatchNorm (sbgm_model::bn_dirty) is raised by EVERY upload of any tensor.  The composed stem and the composed final block each
// decide once whether they are active (`on`), are raised by an upload of one of their sources (Param::feeds, all the upload path knows
// of them) and own every allocation behind them.
struct Derived {
    bool on = false, dirty = true;
    std::vector<float*> owned;              // the image's own buffers and the OIHW copies of its sources
    ~Derived() { for (float* q : owned) (void)hipFree(q); }
    int alloc(float*& q, size_t floats) {
        if (!q) { SBGM_HIP(hipMalloc(&q, floats * 4)); owned.push_back(q); }
        return 0;
    }
    int source_uploaded(Param* p, const float* src, hipStream_t st);
};

// Composed stem of the samplers (conv_stem22.hip): conv2(conv1(.) + tb0) as one 22x22 / stride-4 kernel, built before an EM / PC / EDM
// Heun run, never by a training upload or a plain forward.
// With it, and rebuilt with it (conv1.weight feeds both): w1x, conv1's x-channel weights as the final mix reads them where the run forms
// the decoder's last skip there instead of launching conv1 (conv_final.hip, skip_from_x; sbgm_model::skip_mix_route).
struct Stem : Derived {
    float *wc = nullptr, *sb = nullptr;                    // composed weights and time-bias sums of the 25 border classes
    float* w1x = nullptr;
    static bool env_on() { static const bool v = getenv("SBGM_NO_STEM_COMPOSE") == nullptr; return v; }
    static bool env_skip_mix() { static const bool v = getenv("SBGM_NO_SKIP_MIX") == nullptr; return v; }
    void build(Param* w1, Param* w2);                      // encoder.conv1 / conv2 weights
    int prepare(const Param& w1, const Param& w2, int cin_total, hipStream_t st);
};

// Composed final block (conv_final.hip): final_layer.conv(final_layer.conv_up(.)) as one 3x3 convolution to 16 channels, the 9 taps
// of `conv` first.  cw / cb are no Params of the model (not in the state_dict, the gradient arena or Adam): their images live in one
// allocation at fixed addresses (Wc OIHW [16][ci][3][3], bc [16], then the three packed images), so a cached step graph stays valid.
// The low-resolution form of the same block (`lowres`: Wz of the 9 border classes as MFMA A operands, beta [9]) follows them in that
// allocation and is rebuilt with them; it also reads conv's bias, which therefore feeds this image too.
struct FinalBlock : Derived {                                  // up: final_layer.conv_up.weight / .bias, conv: final_layer.conv.weight / .bias
    float* wc = nullptr;
    Param cw, cb;                                              // the composed weight and bias
    bool lowres = false;
    float *wz = nullptr, *beta = nullptr;
    static bool env_on() { static const bool v = getenv("SBGM_NO_FINAL_COMPOSE") == nullptr; return v; }
    static bool env_lowres() { static const bool v = getenv("SBGM_NO_FINAL_LOWRES") == nullptr; return v; }
    int build(const ConvW& up, const ConvW& conv, int ci, bool resize_conv);
    int prepare(const ConvW& up, const ConvW& conv, hipStream_t st);
};

// A resize decoder block whose conv_up runs on a small map (conv_uplow.hip): the 1x1 weight [9 ci][ci] of the low-resolution tap mix.
// w1 is no Param of the model; its OIHW form and its implicit-GEMM image live in one allocation made by the first prepare() (so a
// training upload pays a copy of the source and nothing else) and kept at fixed addresses after it: a cached step graph stays valid.
// Which blocks take the route is decided in sbgm_model::up_lowres_block, from `on` (the configuration) and up_lowres_shape (the size);
// only those are ever packed.
struct UpLowres : Derived {                                    // up: residual_layers.<i>.conv_up.weight
    float* taps = nullptr;
    Param w1;                                                  // the mix as an ordinary 1x1 convolution weight
    static bool env_on() { static const bool v = getenv("SBGM_NO_UP_LOWRES") == nullptr; return v; }
    void build(const ConvW& up, int ci, bool resize_conv);
    int prepare(const ConvW& up, hipStream_t st);
};
// A LayerNorm followed by a linear of an attention block on the separate-GEMM path (conv_igemm.hip, in_mode 3): the linear's weight with the
// LayerNorm's fixed map folded in, W'' = W diag(gamma) (I - 11^T/C) as an ordinary 1x1 weight, and h = b + W beta.  Neither is a Param of the
// model; W'' in OIHW, its implicit-GEMM image and h live in one allocation made by the first prepare() and kept at fixed addresses after it:
// a cached step graph stays valid.  Raised by an upload of any of the four sources; rebuilt only by refresh_derived for a caller on the
// route (Routes::ln_fold) and a block that runs the separate GEMMs at that size, so a training step never builds it.  SBGM_NO_LN_FOLD=1:
// never.
struct LnFold : Derived {
    Param *g = nullptr, *b = nullptr, *w = nullptr, *bias = nullptr;
    float* buf = nullptr;
    Param w2;                                                  // W'' as a 1x1 convolution weight
    float* h = nullptr;
    static bool env_on() { static const bool v = getenv("SBGM_NO_LN_FOLD") == nullptr; return v; }
    void build(Param* gamma, Param* beta, Param* weight, Param* wbias);
    int prepare(hipStream_t st);
};

// The static rule: the block sizes at which mix + gather measured faster than upsample2x + conv_up + the norm1 passes (DESIGN.md 3.1,
// profiles/r10_block_sums.txt): low-res maps of 2x2 to 8x8 with 128 to 512 channels, 2 Ki to 32 Ki low-res elements per sample, at
// batch 2, 16 and 32.  Nothing outside that range has been measured inside the network, so nothing outside it takes the route (the next
// blocks up, 16x16 and 32x32 low-res maps, were timed as mix + gather alone with the two-pass gather: profiles/r11_block_sums.txt).
inline bool up_lowres_shape(int ci, int h, int w) {
    const long long n = (long long)ci * h * w;
    return h >= 2 && w >= 2 && h <= 8 && w <= 8 && ci >= 128 && ci <= 512 && n >= 2048 && n <= 32768;
}

// Which evaluations take the composed stem (+ the run's condition term, null without condition channels) and the composed final block
// (fin_lowres: as the low-resolution mix + gather instead of the composed 3x3 convolution) and the low-resolution conv_up of the
// small-map decoder blocks (up_lowres) and the folded LayerNorms of the attention blocks on the separate-GEMM path (ln_fold)
// tbrun (EM and PC runs without labels): the run's time biases [9][run_B][ch_i], kept current by the step's advance, so
// the evaluation launches neither the time embedding nor the time projections
// skip_mix (the step samplers only): the evaluation launches neither pack_input nor conv1; the final mix forms the decoder's last skip
// from x, the time row and the run's condition share skip_Sc of conv1 (null without condition channels)
struct Routes {
    bool stem = false, fin = false, fin_lowres = false, up_lowres = false;
    const float* stem_T = nullptr;
    float* tbrun = nullptr;
    int run_B = 0;
    bool skip_mix = false;
    const float* skip_Sc = nullptr;
    bool ln_fold = false;
};
enum Caller { CALL_PLAIN, CALL_SDE_RUN, CALL_MEASURE };

// A device allocation the model handle owns and a run uses: grown roomily (a changed address invalidates the cached step graph)
struct RunBuf {
    void* p = nullptr;
    size_t cap = 0;
    int need(size_t bytes, size_t roomy) {
        if (bytes <= cap) return 0;
        if (p) SBGM_HIP(hipFree(p));
        p = nullptr; cap = 0;
        SBGM_HIP(hipMalloc(&p, std::max(bytes, roomy)));
        cap = std::max(bytes, roomy);
        return 0;
    }
    float* f() const { return static_cast<float*>(p); }
};

// ---- the sampler state that outlives a call (bodies: sampler_run.hip) --------------------------------------------
// The captured SDE step is kept across sampler calls: capture + instantiation of its ~75 kernel nodes cost ~3 ms, as much as
// two steps.  Everything a step bakes in is in the key (shapes, sampler kind, caller tensors, scalar arguments, workspace,
// tile-table generation); what changes between runs lives in device memory (step table, step counter, RNG offset AND seed).
struct StepGraphKey {
    int B, H, W, kind, guided, bn_train, domain_w, churn, ode_norm;
    const void *y, *cond, *lsm, *topo, *origins, *ws, *table;
    const void *known, *known_mask, *levels;   // constrained runs (null otherwise): a held and an unheld step never share a graph
    int joint, domain_h, ramp_len;             // joint tiled runs (0 otherwise): a joint and a non-joint step never share a graph
    const void *rows, *tbrun;                  // EM / PC runs that keep their time rows (null otherwise)
    const void* noise_rows;                    // runs with a noise plan (null otherwise): the launches hold the plan by value, so a run
    int noise_stride, noise_lags;              // with a plan and one without never share a graph, nor do two plans that differ in more
    int noise_domain_h;                        // than the contents of the rows table; > 0: the domain plan (the ONE row's value is read
    float noise_w[SBGM_NOISE_MAX_LAGS];        // by every replay, so two days of one geometry replay the same step)
    size_t ws_bytes;
    float cfg, cfg_corr, snr_nn;
    unsigned long long plan_gen;
};
struct StepKind;                            // one step-sampler kind as data (sampler_run.hip)
struct StepStage;                           // what a call asks SamplerStore::stage for, and what it gets back (sampler_run.hip)
struct SamplerStore {
    SamplerState* d_state = nullptr;        // allocated with the model (sbgm_model::build)
    void* d_table = nullptr;                // step table of the current run: StepScalars rows (EM, PC), EdmStep rows (EDM Heun) or DpmStep rows (2M)
    size_t table_bytes = 0;                 // its capacity
    HoldLevels* d_levels = nullptr;         // hold levels of a constrained EM / PC run, one row per step (allocated by the first such run)
    size_t levels_rows = 0;                 // its capacity
    // pinned host staging of a run's step table + initial state: the upload is a true asynchronous copy, so sbgm_sampler_run does not
    // have to wait for it (or for anything enqueued before it); ev_stage guards the buffer against the next call's rewrite
    char* h_stage = nullptr;
    size_t h_stage_bytes = 0;
    hipEvent_t ev_stage = nullptr;
    bool stage_pending = false;
    RunBuf d_times, d_rows, d_tbrun;        // the run-owned buffers of the time rows (sbgm_model::time_row_layout)
    hipStream_t graph_stream = nullptr;     // private capture stream (the caller's may be the legacy default stream)
    hipEvent_t ev_replayed = nullptr;       // recorded on the caller's stream after a run's last replay of step_exec
    int* h_done = nullptr;                  // pinned copy of an RK45 run's done word, written by a copy node after each controller
    hipEvent_t ev_poll[2] = {nullptr, nullptr};   // recorded after attempt k (slot k & 1): the host reads h_done behind them
    StepGraphKey step_key{};
    hipGraph_t step_graph = nullptr;
    hipGraphExec_t step_exec = nullptr;
    unsigned long long plan_gen = 0;         // bumped whenever the tile table changes (the captured launches embed tile choices)
    SamplerStore() = default;
    SamplerStore(const SamplerStore&) = delete;
    ~SamplerStore();
    void drop_step_graph();
    // Makes step_exec the captured form of `body` under `key`: reused when the cached graph has that key (and `recapture` is not set),
    // else `body`, which enqueues on `st`, is recorded on the private stream (`st` points there meanwhile; capture runs nothing).
    int ensure_step_graph(const StepGraphKey& key, bool recapture, hipStream_t& st, const std::function<int()>& body);
    // A run's step table, initial state, hold levels and time rows: built in the pinned buffer and uploaded on `st` without a host wait
    int stage(const struct sbgm_model& m, const StepKind& kind, StepStage& s, hipStream_t st);
};

struct sbgm_model {
    sbgm_model_config cfg;
    int cin_total = 0, cs_in = 0, D = 0;
    std::vector<std::unique_ptr<Param>> params;
    std::map<std::string, Param*> by_name;
    float* arena = nullptr;
    size_t arena_floats = 0;
    // structure
    ConvW conv1, conv2;
    BNW bn1;
    std::vector<BlockW> layers[4];
    Param *enc_freq = nullptr, *label_emb = nullptr;
    Param *enc_tpw[5], *enc_tpb[5];
    AttnW enc_attn[5];
    bool enc_has_attn[5];
    DecW dec[4];
    ConvW fin_up, fin_conv;
    bool bn_dirty = true;                    // folded BatchNorm (see Derived)
    Stem stem; FinalBlock fin; UpLowres uplow[4];
    std::vector<std::unique_ptr<LnFold>> ln_folds;       // two per attention block (AttnW::fold1 / fold2)
    // What every evaluation reads besides the uploaded parameters: the BatchNorm fold and the final block, refreshed from the evaluation
    // for eager calls and from SamplerRun, prepare_ws and autotune ahead of a capture.  The composed stem is NOT refreshed here but only
    // where an EM / PC / EDM Heun run begins: a plain forward or a training-time evaluation must not start packing a 22x22 image.
    // A decoder block's low-resolution image is built only for a caller that takes that route (`up_route`) at an input size H x W at
    // which the block is eligible: a plain forward, a training-time evaluation or a network whose blocks never qualify packs nothing.
    // The same rule for the folded LayerNorms (`ln_route`): only the attention blocks that run the separate GEMMs at batch B.
    int refresh_derived(hipStream_t st, bool up_route = false, int H = 0, int W = 0, bool ln_route = false, int B = 0);
    // The one place that decides which form of an attention block M tokens take: the token-tile kernels when there are enough 16-token
    // tiles to give every CU one (3 launches: LN1 + in_proj | core | out_proj + residual + LN2 + FF + residual).  Deep levels (few
    // tokens, 256-512 channels) are bound by streaming 1-6 MB of weights: there the separate GEMMs, which split the OUTPUT CHANNELS over
    // the chip, stay faster (measured: 512 tokens x 512 channels 90 us per fused kernel on 32 workgroups vs ~8 us per GEMM).
    static bool attn_token_tiles(int C, int M) {
        static const bool no_fused = getenv("SBGM_NO_FUSED_ATTENTION") != nullptr;
        static const int fused_min_m = getenv("SBGM_ATTN_FUSED_MIN_M") ? atoi(getenv("SBGM_ATTN_FUSED_MIN_M")) : 256 * 16;
        return !no_fused && sbgm_attn_tokens_supported(C) && M >= fused_min_m;
    }
    // ... and whether a block on the separate GEMMs has its two LayerNorms folded into the linears after them
    static bool ln_fold_block(const AttnW& a, int M) { return M >= 1 && a.fold1->on && a.fold2->on && !attn_token_tiles(a.C, M); }
    // Whether a 3x3 convolution of the decoder takes its input through the fused load path (forward.hip, "Fused path")
    bool can_fuse(const ConvW& cw, int c_in, int w_out) const {
        static const bool fused_ok = getenv("SBGM_NO_FUSED_DECODER") == nullptr && !sbgm_conv_switches().no_lds && !sbgm_conv_switches().no_wino;
        return fused_ok && !cfg.decoder_transpose && w_out >= 32 && w_out % 16 == 0 && c_in % 16 == 0 && cw.w->img[IMG_WINO] != nullptr;
    }
    // The one place that decides which blocks run conv_up at low resolution, from block i's low-res map h x w: the configuration
    // (UpLowres::on), a block that is on the unfused path today, and the static rule on its size
    bool up_lowres_block(int i, int h, int w) const {
        return uplow[i].on && h >= 1 && w >= 1 && !can_fuse(dec[i].up, dec[i].cin, 2 * w) && up_lowres_shape(dec[i].cin, h, w);
    }
    // The one place that decides who evaluates through which form of the network, from the kind of caller:
    //   the EM / PC / EDM Heun driver: composed stem and composed final block, for the duration of a run (~SamplerRun ends them);
    //   profile_forward and a tuning evaluation: the final block only (the roofline and the tile table describe the two-convolution stem);
    //   the same callers as the final block: the attention blocks' LayerNorms folded into the linears after them (ln_fold);
    //   the plain forward and the RK45 driver: neither.  rk45_sampler's Python loop and SciPy's solver behind ode_sampler evaluate the
    //   network through the plain forward, and at rtol 1e-4 their accept / reject decisions are within rounding of the native loop's: with
    //   the composed block's rounding one run of tests/test_gpu_rk45_sampler.py took 452 evaluations under SciPy against 464 natively
    //   (bound 9), where the projection path gives 464 / 464; a stem that rounds differently flips such decisions too.
    //   an EM / PC run without a label vector additionally: its own time biases, see sampler().
    Routes routes;
    void set_routes(Caller c, const float* stem_T = nullptr, float* tbrun = nullptr, int run_B = 0, bool skip_mix = false,
                    const float* skip_Sc = nullptr) {
        const bool run = c == CALL_SDE_RUN;
        routes = Routes{run && stem.on, c != CALL_PLAIN && fin.on, c != CALL_PLAIN && fin.on && fin.lowres, c != CALL_PLAIN,
                        run ? stem_T : nullptr, run ? tbrun : nullptr, run ? run_B : 0, run && skip_mix, run && skip_mix ? skip_Sc : nullptr,
                        c != CALL_PLAIN && LnFold::env_on()};
    }
    // Whether a step sampler's evaluations at width W form the decoder's last skip inside the final mix (Routes::skip_mix): the composed
    // stem (so nothing else reads conv1's output in the encoder), the low-resolution final block, and a last decoder block that leaves
    // its normalisation pending with fm[0] as the skip (no attention, fused conv_up of the final layer).  SBGM_NO_SKIP_MIX=1: never.
    bool skip_mix_route(int W) const {
        return Stem::env_skip_mix() && stem.on && fin.on && fin.lowres && dec[3].cout == 64 && !dec[3].has_attn &&
               can_fuse(fin_up, dec[3].cout, W);
    }
    // the run's condition share of conv1, NHWC [B][H/2][W/2][64], after the composed stem's term at the top of the workspace
    size_t skip_sc_bytes(int B, int H, int W) const {
        return skip_mix_route(W) && cin_total > 1 ? align_up((size_t)B * (H / 2) * (W / 2) * 64 * 4, 256) : 0;
    }
    // The layout of a time row of the tbrun route (its run-owned buffers: SamplerStore): the nine time-bias vectors in the order of the
    // evaluation's tb[0..8] (five encoder maps, four decoder blocks); off4 in 16-byte quads, off4[9] = TB / 4
    static bool env_time_rows() { static const bool v = getenv("SBGM_NO_TIME_ROWS") == nullptr; return v; }
    int time_row_layout(int off4[10]) const {
        int ch[9], off[10];
        for (int i = 0; i < 9; ++i) ch[i] = i < 5 ? FMAP_CH[i] : dec[i - 5].cout;
        const int TB = sbgm_time_row_layout(ch, 9, off);
        for (int i = 0; i < 10 && TB > 0; ++i) off4[i] = off[i] / 4;
        return TB;
    }
    // what computes the time biases of B samples at times t into out[i] (rows `stride` floats apart; 0: packed)
    int time_biases(const float* t, const int64_t* y, int B, float* emb_ws, float* const out[9], int stride, hipStream_t st) const;
    size_t stem_t_bytes(int B, int H, int W) const { return stem.on && cin_total > 1 ? align_up((size_t)B * H * W * 4 * 4, 256) : 0; }
    // workspace
    char* ws = nullptr;
    size_t ws_bytes = 0, ws_used = 0;
    SamplerStore store;
    // The noise plan of the sampler runs to come (sbgm_sampler_set_noise_rows; kernels.h: NoiseMap): held until cleared, read by every
    // sampler entry point.  rows == null: none.  domain_h > 0: the domain plan of tiled runs (sbgm_sampler_set_noise_domain_row): rows
    // points to ONE row that serves all tiles of a domain of domain_h rows.  The handle holds one of the two plans or none.
    struct NoiseRows { const int* rows = nullptr; int stride = 1, lags = 1, domain_h = 0; float w[SBGM_NOISE_MAX_LAGS] = {}; } noise_rows;
    ConvTileTable tuned;
    ConvTile last_tile{};                   // tile of the most recent conv() (tells the caller whether GroupNorm statistics were fused)
    bool tuning = false;
    struct ConvRec { ConvGeom g; int B, H, W, Cs, Cout, M, nsteps; ConvTile t; double flops; hipEvent_t e0, e1; float ms; int c_real; int in_mode; int proj; };
    std::vector<ConvRec>* prof = nullptr;   // when set, conv() brackets every launch with events
    static constexpr int PROF_REPS = 4;

    ~sbgm_model() {
        store.drop_step_graph();             // a replay may still be executing in the workspace: waited for before it is freed
        if (arena) (void)hipFree(arena);
        if (ws) (void)hipFree(ws);
    }

    // parameter registration (model.hip)
    Param* add(const std::string& name, ParamKind kind, int64_t numel);
    Param* vec(const std::string& n, int64_t numel) { return add(n, P_VEC, numel); }
    Param* convw(const std::string& n, int cout, int cin, int kh, int kw, int cs = 0, bool wino = false);
    BNW bn(const std::string& pre, int c);
    AttnW attn(const std::string& pre, int C);

    int build(const sbgm_model_config& c);
    int ensure_ws(size_t bytes);
    int dummy_forward(int B, int H, int W, bool tune, hipStream_t st);
    int prepare_ws(int B, int H, int W, int bn_train, hipStream_t st, int slabs, size_t run_extra = 0);
    float* wsalloc(size_t floats) {     // bump allocator over the activation workspace; nullptr (+ error text) when full
        const size_t bytes = align_up(floats * 4, 256);
        if (ws_used + bytes > ws_bytes) {
            sbgm_set_error("workspace exhausted: need %zu more bytes at offset %zu of %zu", bytes, ws_used, ws_bytes);
            return nullptr;
        }
        float* p = reinterpret_cast<float*>(ws + ws_used);
        ws_used += bytes;
        return p;
    }
    float* partial = nullptr;           // split-K scratch shared by every convolution of a forward (stream-ordered reuse)
    static constexpr size_t PARTIAL_FLOATS = 16u << 20;   // 64 MiB
    // Workspace sizing.  The first evaluation of a (B, H, W, BatchNorm mode) runs on a generous bound (1 Ki floats per input pixel);
    // its bump-allocator high-water mark is recorded and every later call asks for exactly that (+ 8 MiB), and ensure_ws gives the
    // surplus back once every shape seen so far is measured (C2: 2.2 GB -> ~0.45 GB).  Addresses are assigned in the same order
    // either way, so results are bit-identical.
    std::map<std::array<int, 4>, size_t> ws_peak;
    size_t ws_target = 0;                   // largest measured total need (forward + sampler slabs) of any shape seen so far
    size_t fwd_need(int B, int H, int W, int bn_train = 0) const;
    // persistent sampler slabs: x, score, x_mean (+ the Heun derivative d for SBGM_SAMPLER_EDM_HEUN; SBGM_SAMPLER_DPMPP_2M keeps its
    // history D in the x_mean slab), then time vector, norm partials.
    // Evaluations and autotuning reserve the three slabs of EM / PC, so that such a sampler finds its workspace settled.
    // SBGM_SAMPLER_RK45: network input, the 2B score of a guided evaluation, seven stage scores, y and y_new in float64 (two slabs
    // each), one slab for the state block and the norm partials.
    static constexpr int ODE_SLABS = 14;
    static int sampler_slabs(int kind) { return kind == SBGM_SAMPLER_RK45 ? ODE_SLABS : kind == SBGM_SAMPLER_EDM_HEUN ? 4 : 3; }
    // After them (run-persistent as well): the composed stem's condition term T [B][H/4][W/4][64].
    size_t slabs_keep(int B, int H, int W, int slabs) const {
        const size_t n = (size_t)B * H * W;
        return align_up(n * 4, 256) * slabs + align_up((size_t)B * 4, 256) + align_up((size_t)B * 8, 256);
    }
    size_t sampler_keep(int B, int H, int W, int slabs) const { return slabs_keep(B, H, W, slabs) + stem_t_bytes(B, H, W); }
    size_t ws_need(int B, int H, int W, int bn_train = 0, int slabs = 3) const {
        return fwd_need(B, H, W, bn_train) + sampler_keep(B, H, W, slabs);
    }
    int fold_bn(hipStream_t st);
    // forward.hip
    ConvTile pick_tile(const ConvGeom& g, const ConvParams& p, const ConvImages& im) const {      // the tuned tile, else the static choice
        const auto it = tuned.find(sbgm_conv_op_key(g, p));
        return it != tuned.end() ? it->second : sbgm_static_tile(g, p, im);
    }
    ConvTile settled_tile(const ConvGeom& g, const ConvParams& p, const ConvImages& im) const;
    int conv(const ConvGeom& g, ConvParams p, const Param& w, hipStream_t st);
    int conv_pair(const ConvGeom& gm, const ConvParams& pm, const Param& wm, const ConvGeom& ga, const ConvParams& pa, const Param& wa,
                  hipStream_t st);
    int attention(const AttnW& a, float* x, int B, int S, hipStream_t st);
    int forward(const float* x, const float* t, const int64_t* y, const float* cond, const float* lsm, const float* topo,
                float* out, float* const* fmaps_out, int B, int H, int W, int bn_train, hipStream_t st);
    // sampler_run.hip
    struct EdmArgs; struct HeldArgs; struct JointArgs; struct DpmArgs; struct OdeArgs;
    int sampler(const sbgm_sampler_args& a, hipStream_t st, const EdmArgs* edm = nullptr, const HeldArgs* held = nullptr,
                const JointArgs* joint = nullptr, const DpmArgs* dpm = nullptr, const NoiseRows* plan = nullptr);
    int sampler_ode(const sbgm_sampler_args& a, hipStream_t st, const OdeArgs& o, const NoiseRows* plan = nullptr);
};
