// Host-side engine: owns the repacked weights and the activation workspace, builds the launch sequence of one
// ScoreNet evaluation for a given (B, H, W) and runs the reverse-SDE sampler loops (optionally as a replayed
// hipGraph).  Mirrors, at the launch-sequence level, reference sbgm/score_unet.py:247-364 (Encoder.forward),
// :559-627 (DecoderBlock.forward), :733-758 (Decoder.forward), :829-879 (ScoreNet.forward) and
// sbgm/score_sampling.py:63-127 / :136-230.
#include <array>
#include <cmath>
#include <cstdio>
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

namespace {

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

// ---- weights derived from uploaded weights ---------------------------------------------------------------------
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
    int source_uploaded(Param* p, const float* src, hipStream_t st) {
        if (!on) return 0;
        if (p->keep_oihw) {
            if (alloc(p->oihw, (size_t)p->numel)) return 1;
            SBGM_HIP(hipMemcpyAsync(p->oihw, src, (size_t)p->numel * 4, hipMemcpyDeviceToDevice, st));
        }
        dirty = true;
        return 0;
    }
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
    void build(Param* w1, Param* w2) {                     // encoder.conv1 / conv2 weights
        on = env_on();
        w1->feeds = w2->feeds = this; w1->keep_oihw = w2->keep_oihw = true;
    }
    int prepare(const Param& w1, const Param& w2, int cin_total, hipStream_t st) {
        if (!on || !dirty) return 0;
        SBGM_CHECK(w1.oihw && w2.oihw, "sampler: encoder.conv1 / conv2 weights were never uploaded");
        if (alloc(wc, sbgm_stem22_packed_floats(cin_total)) || alloc(sb, sbgm_stem22_bias_floats())) return 1;
        if (alloc(w1x, SKIP_MIX_PACKED_FLOATS)) return 1;
        if (sbgm_launch_pack_stem22(w1.oihw, w2.oihw, wc, sb, cin_total, st)) return 1;
        if (sbgm_launch_skip_mix_pack(w1.oihw, w1x, cin_total, st)) return 1;
        dirty = false;
        return 0;
    }
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
    int build(const ConvW& up, const ConvW& conv, int ci, bool resize_conv) {
        Param* const w2 = conv.w;
        // the 16-channel op runs on the LDS-staged Winograd kernels only, so the switches that take those away keep the projection path
        on = env_on() && resize_conv && ci % 16 == 0 && up.w->img[IMG_WINO] != nullptr && !sbgm_conv_switches().no_lds &&
             !sbgm_conv_switches().round1;
        if (!on) return 0;
        up.w->feeds = up.b->feeds = w2->feeds = this; up.w->keep_oihw = w2->keep_oihw = true;
        cw.name = "final_layer.composed.weight"; cw.kind = P_CONV; cw.numel = (int64_t)16 * ci * 9;
        cw.cout = 16; cw.cin = ci; cw.kh = cw.kw = 3; cw.cs = ci; cw.want_wino = true;
        sbgm_conv_image_floats(3, 3, ci, 16, true, cw.floats);
        cb.name = "final_layer.composed.bias"; cb.numel = cb.floats[0] = 16;
        lowres = env_lowres() && ci <= FINAL_LOWRES_MAX_C;
        if (lowres) conv.b->feeds = this;
        const size_t wz_floats = lowres ? align_up(sbgm_final_lowres_packed_floats(ci), 64) : 0;
        const size_t wc_floats = align_up((size_t)cw.numel, 64), images = wc_floats + cb.storage_floats() + cw.storage_floats();
        const size_t total = images + wz_floats + (lowres ? 64 : 0);
        if (alloc(wc, total)) return 1;
        SBGM_HIP(hipMemset(wc, 0, total * 4));
        cw.place(cb.place(wc + wc_floats));
        cw.filled = cb.filled = true;
        if (lowres) { wz = wc + images; beta = wz + wz_floats; }
        return 0;
    }
    int prepare(const ConvW& up, const ConvW& conv, hipStream_t st) {
        if (!on || !dirty) return 0;
        const Param& w2 = *conv.w;
        SBGM_CHECK(up.w->oihw && w2.oihw && up.b->filled, "final block: final_layer.conv_up / conv weights were never uploaded");
        if (sbgm_launch_final_compose(up.w->oihw, up.b->dev(), w2.oihw, wc, cb.dev(), cw.cin, st)) return 1;
        if (sbgm_pack_conv_images(wc, cw.img, 16, cw.cin, 3, 3, cw.cin, st)) return 1;
        if (lowres) {
            SBGM_CHECK(conv.b->filled, "final block: final_layer.conv.bias was never uploaded");
            if (sbgm_launch_final_lowres_pack(up.w->oihw, up.b->dev(), w2.oihw, conv.b->dev(), nullptr, beta, wz, cw.cin, st)) return 1;
        }
        dirty = false;
        return 0;
    }
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
    void build(const ConvW& up, int ci, bool resize_conv) {
        on = env_on() && resize_conv && ci % 16 == 0;
        if (!on) return;
        up.w->feeds = this; up.w->keep_oihw = true;             // the bias is read from its Param at launch: no part of the image
        w1.name = "conv_up.taps.weight"; w1.kind = P_CONV; w1.numel = (int64_t)sbgm_up_lowres_weight_floats(ci);
        w1.cout = 9 * ci; w1.cin = ci; w1.kh = w1.kw = 1; w1.cs = ci;
        w1.floats[IMG_IGEMM] = sbgm_up_lowres_weight_floats(ci);
    }
    int prepare(const ConvW& up, hipStream_t st) {
        if (!on || !dirty) return 0;
        SBGM_CHECK(up.w->oihw, "decoder: a conv_up weight was never uploaded");
        const size_t n = align_up((size_t)w1.numel, 64);
        if (alloc(taps, 2 * n)) return 1;
        w1.img[IMG_IGEMM] = taps + n;
        if (sbgm_launch_up_lowres_pack(up.w->oihw, taps, taps + n, w1.cin, st)) return 1;
        w1.filled = true;
        dirty = false;
        return 0;
    }
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
    void build(Param* gamma, Param* beta, Param* weight, Param* wbias) {
        g = gamma; b = beta; w = weight; bias = wbias;
        on = env_on() && w->cin % 16 == 0 && w->cs == w->cin;
        if (!on) return;
        g->feeds = b->feeds = w->feeds = bias->feeds = this; w->keep_oihw = true;
        w2.name = w->name + ".ln_folded"; w2.kind = P_CONV; w2.numel = w->numel;
        w2.cout = w->cout; w2.cin = w2.cs = w->cin; w2.kh = w2.kw = 1;
        w2.floats[IMG_IGEMM] = (size_t)w->numel;
    }
    int prepare(hipStream_t st) {
        if (!on || !dirty) return 0;
        SBGM_CHECK(w->oihw && g->filled && b->filled && bias->filled, "attention: '%s' or its LayerNorm was never uploaded", w->name.c_str());
        const size_t n = align_up((size_t)w2.numel, 64);
        if (alloc(buf, 2 * n + align_up((size_t)w2.cout, 64))) return 1;
        w2.img[IMG_IGEMM] = buf + n;
        h = buf + 2 * n;
        if (sbgm_launch_ln_fold(w->oihw, bias->dev(), g->dev(), b->dev(), buf, h, w2.cin, w2.cout, st)) return 1;
        if (sbgm_pack_conv_images(buf, w2.img, w2.cout, w2.cin, 1, 1, w2.cs, st)) return 1;
        w2.filled = true;
        dirty = false;
        return 0;
    }
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

}  // namespace

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
    // What every evaluation reads besides the uploaded parameters: the BatchNorm fold and the final block, refreshed from forward_impl
    // for eager calls and from SamplerRun, prepare_ws and autotune ahead of a capture.  The composed stem is NOT refreshed here but only
    // where an EM / PC / EDM Heun run begins: a plain forward or a training-time evaluation must not start packing a 22x22 image.
    // A decoder block's low-resolution image is built only for a caller that takes that route (`up_route`) at an input size H x W at
    // which the block is eligible: a plain forward, a training-time evaluation or a network whose blocks never qualify packs nothing.
    // The same rule for the folded LayerNorms (`ln_route`): only the attention blocks that run the separate GEMMs at batch B.
    int refresh_derived(hipStream_t st, bool up_route = false, int H = 0, int W = 0, bool ln_route = false, int B = 0) {
        if (bn_dirty && fold_bn(st)) return 1;
        for (int i = 0; i < 4 && up_route; ++i)
            if (up_lowres_block(i, (H / 32) << i, (W / 32) << i) && uplow[i].prepare(dec[i].up, st)) return 1;
        auto folds = [&](const AttnW& a, int h, int w) {
            return ln_fold_block(a, B * h * w) && (a.fold1->prepare(st) || a.fold2->prepare(st));
        };
        for (int i = 0; i < 5 && ln_route; ++i)                     // encoder map 0 is H / 2 high, map i >= 1 H / 2^(i+1)
            if (enc_has_attn[i] && folds(enc_attn[i], H >> (i ? i + 1 : 1), W >> (i ? i + 1 : 1))) return 1;
        for (int i = 0; i < 4 && ln_route; ++i)
            if (dec[i].has_attn && folds(dec[i].attn, (H / 32) << (i + 1), (W / 32) << (i + 1))) return 1;
        return fin.prepare(fin_up, fin_conv, st);
    }
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
    // Whether a 3x3 convolution of the decoder takes its input through the fused load path (forward_impl, "Fused path")
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
    // The run-owned buffers of that route and the layout of a time row: the nine time-bias vectors in the order of forward_impl's
    // tb[0..8] (five encoder maps, four decoder blocks); off4 in 16-byte quads, off4[9] = TB / 4
    static bool env_time_rows() { static const bool v = getenv("SBGM_NO_TIME_ROWS") == nullptr; return v; }
    RunBuf d_times, d_rows, d_tbrun;
    int time_row_layout(int off4[10]) const {
        int ch[9], off[10];
        for (int i = 0; i < 9; ++i) ch[i] = i < 5 ? FMAP_CH[i] : dec[i - 5].cout;
        const int TB = sbgm_time_row_layout(ch, 9, off);
        for (int i = 0; i < 10 && TB > 0; ++i) off4[i] = off[i] / 4;
        return TB;
    }
    // what computes the time biases of B samples at times t into out[i] (rows `stride` floats apart; 0: packed)
    int time_biases(const float* t, const int64_t* y, int B, float* emb_ws, float* const out[9], int stride, hipStream_t st) const {
        TimeEmbedArgs te{};
        te.t = t; te.y = y; te.label_emb = (y && label_emb) ? label_emb->dev() : nullptr;
        te.B = B; te.D = D;
        te.n_emb = 5;
        te.freqs[0] = enc_freq->dev();
        for (int i = 0; i < 4; ++i) te.freqs[1 + i] = dec[i].freq->dev();
        te.emb_ws = emb_ws;
        te.n_proj = 9;
        for (int i = 0; i < 5; ++i) te.proj[i] = TimeProj{enc_tpw[i]->dev(), enc_tpb[i]->dev(), out[i], FMAP_CH[i], 0, stride};
        for (int i = 0; i < 4; ++i) te.proj[5 + i] = TimeProj{dec[i].tpw->dev(), dec[i].tpb->dev(), out[5 + i], dec[i].cout, 1 + i, stride};
        return sbgm_launch_time_embed(te, st);
    }
    size_t stem_t_bytes(int B, int H, int W) const { return stem.on && cin_total > 1 ? align_up((size_t)B * H * W * 4 * 4, 256) : 0; }
    // workspace
    char* ws = nullptr;
    size_t ws_bytes = 0, ws_used = 0;
    // sampler state
    SamplerState* d_state = nullptr;
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
    ConvTileTable tuned;
    ConvTile last_tile{};                   // tile of the most recent conv() (tells the caller whether GroupNorm statistics were fused)
    bool tuning = false;
    struct ConvRec { ConvGeom g; int B, H, W, Cs, Cout, M, nsteps; ConvTile t; double flops; hipEvent_t e0, e1; float ms; int c_real; int in_mode; int proj; };
    std::vector<ConvRec>* prof = nullptr;   // when set, conv() brackets every launch with events
    static constexpr int PROF_REPS = 4;
    hipStream_t graph_stream = nullptr;     // private capture stream (the caller's may be the legacy default stream)
    hipEvent_t ev_replayed = nullptr;       // recorded on the caller's stream after a run's last replay of step_exec
    int* h_done = nullptr;                  // pinned copy of an RK45 run's done word, written by a copy node after each controller
    hipEvent_t ev_poll[2] = {nullptr, nullptr};   // recorded after attempt k (slot k & 1): the host reads h_done behind them
    // The captured SDE step is kept across sampler calls: capture + instantiation of its ~75 kernel nodes cost ~3 ms, as much as
    // two steps.  Everything a step bakes in is in the key (shapes, sampler kind, caller tensors, scalar arguments, workspace,
    // tile-table generation); what changes between runs lives in device memory (step table, step counter, RNG offset AND seed).
    struct StepGraphKey {
        int B, H, W, kind, guided, bn_train, domain_w, churn, ode_norm;
        const void *y, *cond, *lsm, *topo, *origins, *ws, *table;
        const void *known, *known_mask, *levels;   // constrained runs (null otherwise): a held and an unheld step never share a graph
        int joint, domain_h, ramp_len;             // joint tiled runs (0 otherwise): a joint and a non-joint step never share a graph
        const void *rows, *tbrun;                  // EM / PC runs that keep their time rows (null otherwise)
        size_t ws_bytes;
        float cfg, cfg_corr, snr_nn;
        unsigned long long plan_gen;
    };
    StepGraphKey step_key{};
    hipGraph_t step_graph = nullptr;
    hipGraphExec_t step_exec = nullptr;
    unsigned long long plan_gen = 0;         // bumped whenever the tile table changes (the captured launches embed tile choices)
    void drop_step_graph() {
        if (step_exec && ev_replayed) (void)hipEventSynchronize(ev_replayed);        // a replay of it may still be executing
        if (step_exec) (void)hipGraphExecDestroy(step_exec);
        if (step_graph) (void)hipGraphDestroy(step_graph);
        step_exec = nullptr;
        step_graph = nullptr;
    }
    // Makes step_exec the captured form of `body` under `key`: reused when the cached graph has that key (and `recapture` is not set),
    // else `body`, which enqueues on `st`, is recorded on the private stream (`st` points there meanwhile; capture runs nothing).
    int ensure_step_graph(const StepGraphKey& key, bool recapture, hipStream_t& st, const std::function<int()>& body) {
        if (step_exec != nullptr && !recapture && std::memcmp(&key, &step_key, sizeof key) == 0) return 0;
        drop_step_graph();
        const hipStream_t caller = st;
        st = graph_stream;
        int rc = 0;
        hipError_t e = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal);
        if (e != hipSuccess) { sbgm_set_error("hipStreamBeginCapture failed: %s", hipGetErrorString(e)); rc = 2; }
        if (rc == 0) {
            rc = body();
            e = hipStreamEndCapture(st, &step_graph);
            if (rc == 0 && (e != hipSuccess || hipGraphInstantiate(&step_exec, step_graph, nullptr, nullptr, 0) != hipSuccess)) {
                sbgm_set_error("hipGraph capture/instantiate failed: %s", hipGetErrorString(e));
                rc = 2;
            }
            if (rc) drop_step_graph();
            else step_key = key;
        }
        st = caller;
        return rc;
    }

    ~sbgm_model() {
        drop_step_graph();
        if (arena) (void)hipFree(arena);
        if (ws) (void)hipFree(ws);
        if (d_state) (void)hipFree(d_state);
        if (d_table) (void)hipFree(d_table);
        if (d_levels) (void)hipFree(d_levels);
        for (RunBuf* b : {&d_times, &d_rows, &d_tbrun}) if (b->p) (void)hipFree(b->p);
        if (h_stage) (void)hipHostFree(h_stage);
        if (ev_stage) (void)hipEventDestroy(ev_stage);
        if (graph_stream) (void)hipStreamDestroy(graph_stream);
        if (ev_replayed) (void)hipEventDestroy(ev_replayed);
        if (h_done) (void)hipHostFree(h_done);
        for (hipEvent_t e : ev_poll) if (e) (void)hipEventDestroy(e);
    }

    Param* add(const std::string& name, ParamKind kind, int64_t numel) {
        params.emplace_back(new Param());
        Param* p = params.back().get();
        p->name = name; p->kind = kind; p->numel = numel;
        by_name[name] = p;
        return p;
    }
    Param* vec(const std::string& n, int64_t numel) { return add(n, P_VEC, numel); }
    Param* convw(const std::string& n, int cout, int cin, int kh, int kw, int cs = 0, bool wino = false) {
        Param* p = add(n, P_CONV, (int64_t)cout * cin * kh * kw);
        p->cout = cout; p->cin = cin; p->kh = kh; p->kw = kw;
        p->cs = cs ? cs : (int)align_up(cin, 16);
        p->want_wino = wino;
        return p;
    }
    BNW bn(const std::string& pre, int c) {
        BNW b;
        b.g = vec(pre + ".weight", c); b.b = vec(pre + ".bias", c);
        b.rm = vec(pre + ".running_mean", c); b.rv = vec(pre + ".running_var", c);
        add(pre + ".num_batches_tracked", P_IGNORE, 1);
        b.scale = b.bias = nullptr;
        return b;
    }
    AttnW attn(const std::string& pre, int C) {
        AttnW a; a.C = C;
        a.inw = convw(pre + ".mha.in_proj_weight", 3 * C, C, 1, 1);
        a.inb = vec(pre + ".mha.in_proj_bias", 3 * C);
        a.outw = convw(pre + ".mha.out_proj.weight", C, C, 1, 1);
        a.outb = vec(pre + ".mha.out_proj.bias", C);
        a.ln1g = vec(pre + ".ln1.weight", C); a.ln1b = vec(pre + ".ln1.bias", C);
        a.ln2g = vec(pre + ".ln2.weight", C); a.ln2b = vec(pre + ".ln2.bias", C);
        a.f1w = convw(pre + ".ff.0.weight", C, C, 1, 1); a.f1b = vec(pre + ".ff.0.bias", C);
        a.f2w = convw(pre + ".ff.2.weight", C, C, 1, 1); a.f2b = vec(pre + ".ff.2.bias", C);
        for (LnFold** f : {&a.fold1, &a.fold2}) {
            ln_folds.emplace_back(new LnFold());
            *f = ln_folds.back().get();
        }
        a.fold1->build(a.ln1g, a.ln1b, a.inw, a.inb);
        a.fold2->build(a.ln2g, a.ln2b, a.f1w, a.f1b);
        return a;
    }

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
    ConvTile pick_tile(const ConvGeom& g, const ConvParams& p, const ConvImages& im) const {      // the tuned tile, else the static choice
        const auto it = tuned.find(sbgm_conv_op_key(g, p));
        return it != tuned.end() ? it->second : sbgm_static_tile(g, p, im);
    }
    int conv(const ConvGeom& g, ConvParams p, const Param& w, hipStream_t st);
    int conv_pair(const ConvGeom& gm, const ConvParams& pm, const Param& wm, const ConvGeom& ga, const ConvParams& pa, const Param& wa,
                  hipStream_t st);
    int attention(const AttnW& a, float* x, int B, int S, hipStream_t st);
    int forward_impl(const float* x, const float* t, const int64_t* y, const float* cond, const float* lsm, const float* topo,
                     float* out, float* const* fmaps_out, int B, int H, int W, int bn_train, hipStream_t st);
    int forward(const float* x, const float* t, const int64_t* y, const float* cond, const float* lsm, const float* topo,
                float* out, float* const* fmaps_out, int B, int H, int W, int bn_train, hipStream_t st) {
        const int rc = forward_impl(x, t, y, cond, lsm, topo, out, fmaps_out, B, H, W, bn_train, st);
        if (!rc && !tuning) {                                // the evaluation's high-water mark sizes every later call of this shape
            size_t& pk = ws_peak[std::array<int, 4>{B, H, W, bn_train != 0}];
            pk = std::max(pk, ws_used);
            // (with a step sampler's condition share of conv1: a plain call between two runs must not trim what the next run asks back)
            ws_target = std::max(ws_target, pk + ((size_t)8 << 20) + sampler_keep(B, H, W, 3) + skip_sc_bytes(B, H, W));
        }
        return rc;
    }
    struct EdmArgs { float sigma_min, sigma_max, rho, s_churn, s_tmin, s_tmax, s_noise; };
    struct HeldArgs { const float *known, *mask; };        // constrained sampling: both device [B][1][H][W], used in place
    struct JointArgs { int domain_h, ramp_len; };          // joint tiled sampling: the B tiles are one domain of domain_h x a.domain_w
    struct DpmArgs { float sigma_min, sigma_max, rho, eta, s_noise; };     // DPM-Solver++(2M): eta > 0 is the SDE variant
    int sampler(const sbgm_sampler_args& a, hipStream_t st, const EdmArgs* edm = nullptr, const HeldArgs* held = nullptr,
                const JointArgs* joint = nullptr, const DpmArgs* dpm = nullptr);
    struct OdeArgs { double t0, t1, rtol, atol; int per_sample; long long max_steps; const float* x0; int64_t* stats_i; double* stats_d; };
    int sampler_ode(const sbgm_sampler_args& a, hipStream_t st, const OdeArgs& o);
};

int sbgm_model::build(const sbgm_model_config& c) {
    cfg = c;
    SBGM_CHECK(c.time_embedding > 0 && c.time_embedding % 2 == 0, "time_embedding=%d must be even", c.time_embedding);
    SBGM_CHECK(c.last_fmap_channels == 512, "last_fmap_channels=%d: the encoder always emits 512 (score_unet.py:198)",
               c.last_fmap_channels);
    SBGM_CHECK(c.n_heads > 0, "n_heads must be positive");
    D = c.time_embedding;
    cin_total = 1 + c.n_lsm_channels + c.n_topo_channels + c.n_cond_channels;
    cs_in = pad_channels(cin_total);
    SBGM_CHECK(cs_in <= 16, "input channels %d > 16 unsupported", cin_total);
    // ---- encoder (registration mirrors the reference state_dict names) ------------------------------------------
    // 2 input channels (x + one condition, BASELINE config 2): pixels keep 4 slots but the weights are packed 8 taps x 2 channels
    // per K step, so no MFMA work is spent on the two padding slots
    conv1.w = convw("encoder.conv1.weight", 64, cin_total, 8, 8, cin_total == 2 ? 2 : cs_in);
    bn1 = bn("encoder.bn1", 64);
    int cin = 64;
    for (int li = 0; li < 4; ++li) {
        const int w = FMAP_CH[li + 1];
        SBGM_CHECK(c.block_layers[li] >= 1, "block_layers[%d] must be >= 1", li);
        for (int bi = 0; bi < c.block_layers[li]; ++bi) {
            const std::string pre = "encoder.layer" + std::to_string(li + 1) + "." + std::to_string(bi);
            BlockW b;
            b.cin = cin; b.cout = w; b.stride = (bi == 0 && li > 0) ? 2 : 1;
            b.c1.w = convw(pre + ".conv1.weight", w, cin, 3, 3, 0, b.stride == 1);
            b.bn1 = bn(pre + ".bn1", w);
            b.c2.w = convw(pre + ".conv2.weight", w, w, 3, 3, 0, true);
            b.bn2 = bn(pre + ".bn2", w);
            b.has_ds = (bi == 0) && (b.stride != 1 || cin != w);
            if (b.has_ds) {
                b.ds.w = convw(pre + ".downsample.0.weight", w, cin, 1, 1);
                b.dsbn = bn(pre + ".downsample.1", w);
            }
            layers[li].push_back(b);
            cin = w;
        }
    }
    enc_freq = vec("encoder.sinusoidal_embedding.W", D / 2);
    for (int i = 0; i < 5; ++i) {
        enc_tpw[i] = vec("encoder.time_projection_layers." + std::to_string(i) + ".1.weight", (int64_t)FMAP_CH[i] * D);
        enc_tpb[i] = vec("encoder.time_projection_layers." + std::to_string(i) + ".1.bias", FMAP_CH[i]);
    }
    for (int i = 0; i < 5; ++i) {
        enc_has_attn[i] = i >= 3;                                                   // score_unet.py:396
        if (enc_has_attn[i]) {
            SBGM_CHECK(FMAP_CH[i] % c.n_heads == 0, "channels %d not divisible by heads %d", FMAP_CH[i], c.n_heads);
            enc_attn[i] = attn("encoder.attention_layers." + std::to_string(i), FMAP_CH[i]);
        }
    }
    conv2.w = convw("encoder.conv2.weight", 64, 64, 8, 8, 0, true);       // conv1 keeps the implicit-GEMM kernels alone
    if (c.num_classes > 0) label_emb = vec("encoder.label_emb.weight", (int64_t)(c.num_classes + 1) * D);
    // ---- decoder ---------------------------------------------------------------------------------------------------
    int dc = c.last_fmap_channels;
    auto dec_block = [&](const std::string& pre, DecW& d, int ci, int co, bool with_norm, bool with_attn) {
        d.cin = ci; d.cout = co; d.has_attn = with_attn;
        if (c.decoder_transpose) {       // ablation path: ConvTranspose2d(ci, ci, 2, 2) as a 1x1 conv to 4*ci phase-major channels
            d.up.w = add(pre + ".transpose.weight", P_TCONV, (int64_t)ci * ci * 4);
            d.up.w->cout = 4 * ci; d.up.w->cin = ci; d.up.w->kh = d.up.w->kw = 1; d.up.w->cs = (int)align_up(ci, 16);
            d.up.b = add(pre + ".transpose.bias", P_VEC4, ci);
        } else {
            d.up.w = convw(pre + ".conv_up.weight", ci, ci, 3, 3, 0, true);
            d.up.b = vec(pre + ".conv_up.bias", ci);
        }
        const bool affine = with_norm && c.decoder_norm == SBGM_NORM_GROUP;
        d.n1g = affine ? vec(pre + ".norm1.weight", ci) : nullptr;
        d.n1b = affine ? vec(pre + ".norm1.bias", ci) : nullptr;
        if (co == 1) {
            d.conv.w = add(pre + ".conv.weight", P_COUT1, (int64_t)ci * 9);
            d.conv.w->cin = ci;
        } else {
            d.conv.w = convw(pre + ".conv.weight", co, ci, 3, 3, 0, true);
        }
        d.conv.b = vec(pre + ".conv.bias", co);
        d.n2g = affine ? vec(pre + ".norm2.weight", co) : nullptr;
        d.n2b = affine ? vec(pre + ".norm2.bias", co) : nullptr;
        d.freq = vec(pre + ".sinusoidal_embedding.W", D / 2);
        d.tpw = vec(pre + ".time_projection_layer.1.weight", (int64_t)co * D);
        d.tpb = vec(pre + ".time_projection_layer.1.bias", co);
        if (with_attn) {
            SBGM_CHECK(co % c.n_heads == 0, "channels %d not divisible by heads %d", co, c.n_heads);
            d.attn = attn(pre + ".attention", co);
        }
        return 0;
    };
    for (int i = 0; i < 4; ++i) {
        const int co = i != 3 ? dc / 2 : 64;
        if (dec_block("decoder.residual_layers." + std::to_string(i), dec[i], dc, co, true, i < 2)) return 1;
        dc = co;
    }
    DecW fl;
    if (dec_block("decoder.final_layer", fl, dec[3].cin, 1, false, false)) return 1;
    // final layer: its time-embedding tensors exist in the state_dict but are never used (score_unet.py:757)
    fl.freq->kind = fl.tpw->kind = fl.tpb->kind = P_IGNORE;
    fin_up = fl.up; fin_conv = fl.conv;

    // ---- storage ----------------------------------------------------------------------------------------------------
    size_t total = 0;
    for (auto& up : params) {
        Param* p = up.get();
        if (p->kind == P_CONV || p->kind == P_TCONV) sbgm_conv_image_floats(p->kh, p->kw, p->cs, p->cout, p->want_wino, p->floats);
        else if (p->kind == P_VEC4) p->floats[0] = (size_t)p->numel * 4;
        else if (p->kind == P_IGNORE) p->floats[0] = 0;
        else p->floats[0] = (size_t)p->numel;
        total += p->storage_floats();
    }
    // folded BN scale/bias
    size_t bn_floats = 0;
    auto count_bn = [&](BNW& b, int c_) { bn_floats += 2 * align_up((size_t)c_, 64); (void)b; };
    count_bn(bn1, 64);
    for (int li = 0; li < 4; ++li)
        for (auto& b : layers[li]) { count_bn(b.bn1, b.cout); count_bn(b.bn2, b.cout); if (b.has_ds) count_bn(b.dsbn, b.cout); }
    arena_floats = total + bn_floats + 64;
    SBGM_HIP(hipMalloc(&arena, arena_floats * 4));
    SBGM_HIP(hipMemset(arena, 0, arena_floats * 4));
    size_t off = 0;
    for (auto& up : params) {
        Param* p = up.get();
        off = p->place(arena + off) - arena;
        if (p->kind == P_IGNORE) p->filled = true;
    }
    auto place_bn = [&](BNW& b, int c_) {
        b.scale = arena + off; off += align_up((size_t)c_, 64);
        b.bias = arena + off; off += align_up((size_t)c_, 64);
    };
    place_bn(bn1, 64);
    for (int li = 0; li < 4; ++li)
        for (auto& b : layers[li]) { place_bn(b.bn1, b.cout); place_bn(b.bn2, b.cout); if (b.has_ds) place_bn(b.dsbn, b.cout); }
    SBGM_HIP(hipMalloc(&d_state, sizeof(SamplerState)));
    stem.build(conv1.w, conv2.w);
    for (int i = 0; i < 4; ++i) uplow[i].build(dec[i].up, dec[i].cin, !c.decoder_transpose);
    return fin.build(fin_up, fin_conv, dec[3].cout, !c.decoder_transpose);   // after place(): the route needs conv_up's Winograd image
}

int sbgm_model::ensure_ws(size_t bytes) {
    // enough, and not grossly oversized now that every shape in use has a measured need: keep it
    const bool trim = ws != nullptr && ws_target > 0 && bytes <= ws_bytes &&
                      ws_bytes > std::max(bytes, ws_target) + ((size_t)256 << 20);
    if (bytes <= ws_bytes && !trim) return 0;
    if (trim) bytes = std::max(bytes, ws_target);
    drop_step_graph();                       // its nodes point into the old workspace
    if (ws) SBGM_HIP(hipFree(ws));
    ws = nullptr; ws_bytes = 0;
    SBGM_HIP(hipMalloc(&ws, bytes));
    ws_bytes = bytes;
    return 0;
}

// measured high-water mark of this shape when there is one, else a generous upper bound
size_t sbgm_model::fwd_need(int B, int H, int W, int bn_train) const {
    auto it = ws_peak.find(std::array<int, 4>{B, H, W, bn_train != 0});
    if (it != ws_peak.end()) return it->second + ((size_t)8 << 20);
    const size_t px = (size_t)B * H * W;
    // NHWC floats per input pixel summed over all intermediates (encoder ~ 64/4*3 + ..., decoder dominated by the
    // final block's 3 x 64 channels at full resolution); 1024 floats/pixel is > 2x the true footprint.
    return px * 1024 * 4 + PARTIAL_FLOATS * 4 + (64u << 20);
}

int sbgm_model::fold_bn(hipStream_t st) {
    auto f = [&](BNW& b, int c) {
        return sbgm_launch_bn_fold(b.g->dev(), b.b->dev(), b.rm->dev(), b.rv->dev(), BN_EPS, b.scale, b.bias, c, st);
    };
    if (f(bn1, 64)) return 1;
    for (int li = 0; li < 4; ++li)
        for (auto& b : layers[li]) {
            if (f(b.bn1, b.cout) || f(b.bn2, b.cout)) return 1;
            if (b.has_ds && f(b.dsbn, b.cout)) return 1;
        }
    bn_dirty = false;
    return 0;
}

int sbgm_model::conv(const ConvGeom& g, ConvParams p, const Param& w, hipStream_t st) {
    const ConvImages im = w.images();
    const int OH = (p.H + 2 * g.pad - g.kh) / g.stride + 1, OW = (p.W + 2 * g.pad - g.kw) / g.stride + 1;
    const size_t mc = (size_t)p.B * OH * OW * p.Cout;
    if (tuning) {
        // time every candidate on this op, keep the fastest
        const ConvOpKey key = sbgm_conv_op_key(g, p);
        if (tuned.find(key) == tuned.end()) {
            ConvTile best_t = pick_tile(g, p, im);
            if (sbgm_tune_conv(g, p, im, partial, PARTIAL_FLOATS, st, &best_t)) return 1;
            tuned[key] = best_t;
            ++plan_gen;
        }
    }
    ConvTile ct = pick_tile(g, p, im);
    if (ct.splits > 1 && mc * ct.splits > PARTIAL_FLOATS) ct.splits = (int)std::max<size_t>(1, PARTIAL_FLOATS / mc);
    last_tile = ct;
    if (!prof) return sbgm_launch_tile(g, p, im, ct, partial, st);
    ConvRec r{g, p.B, p.H, p.W, p.Cs, p.Cout, p.B * OH * OW, sbgm_conv_nsteps(g.kh, g.kw, p.c_real == 2 ? 2 : p.Cs), ct, 0.0, nullptr, nullptr, 0.f, p.c_real, p.in_mode, p.proj_w != nullptr};
    // algorithmic FLOPs: 2 * M * Cout * (KH*KW*Cin_real); Cs may be padded (only the stem conv), count real K there
    const int cin_real = (g.kh == 8 && p.Cs <= 16) ? cin_total : p.Cs;
    r.flops = 2.0 * r.M * p.Cout * (double)(g.kh * g.kw * cin_real);
    SBGM_HIP(hipEventCreate(&r.e0));
    SBGM_HIP(hipEventCreate(&r.e1));
    // PROF_REPS back-to-back launches per event pair (a launch is idempotent: it never reads what it writes), so the interval is
    // dominated by execution time rather than by the event packets and the host's launch gaps
    SBGM_HIP(hipEventRecord(r.e0, st));
    int rc = 0;
    for (int rep = 0; rep < PROF_REPS && !rc; ++rep) rc = sbgm_launch_tile(g, p, im, ct, partial, st);
    SBGM_HIP(hipEventRecord(r.e1, st));
    prof->push_back(r);
    return rc;
}

// A BasicBlock's strided 3x3 convolution (main) and its 1x1 shortcut (aux), both of one input: one launch where the planner serves the
// pair of tiles, for every caller (the bodies and tiles are the ones the two launches use, so the bits are the same).  A tuning
// evaluation and the profiled forward keep the two launches: the tile table and the roofline CSV have one row per convolution.
int sbgm_model::conv_pair(const ConvGeom& gm, const ConvParams& pm, const Param& wm, const ConvGeom& ga, const ConvParams& pa, const Param& wa,
                          hipStream_t st) {
    if (tuning || prof) return conv(gm, pm, wm, st) || conv(ga, pa, wa, st);
    const ConvImages im = wm.images(), ia = wa.images();
    auto tile = [&](const ConvGeom& g, const ConvParams& p, const ConvImages& i) {       // as conv() settles it
        const int OH = (p.H + 2 * g.pad - g.kh) / g.stride + 1, OW = (p.W + 2 * g.pad - g.kw) / g.stride + 1;
        const size_t mc = (size_t)p.B * OH * OW * p.Cout;
        ConvTile ct = pick_tile(g, p, i);
        if (ct.splits > 1 && mc * ct.splits > PARTIAL_FLOATS) ct.splits = (int)std::max<size_t>(1, PARTIAL_FLOATS / mc);
        return ct;
    };
    const ConvTile tm = tile(gm, pm, im), ta = tile(ga, pa, ia);
    last_tile = ta;
    return sbgm_launch_tile_pair(gm, pm, im, tm, ga, pa, ia, ta, partial, st);
}

// y = h + FF(LN2(h)),  h = x + MHA(LN1(x))   over tokens [B*S, C]  (score_unet.py:136-148); in place on x
int sbgm_model::attention(const AttnW& a, float* x, int B, int S, hipStream_t st) {
    const int C = a.C, M = B * S;
    if (attn_token_tiles(C, M)) {
        float* qkv = wsalloc((size_t)M * 3 * C);
        if (!qkv) return 1;
        float* att = wsalloc((size_t)M * C);
        if (!att) return 1;
        if (sbgm_launch_attn_in(x, a.ln1g->dev(), a.ln1b->dev(), a.inw->dev(), a.inb->dev(), qkv, M, C, LN_EPS, st)) return 1;
        if (sbgm_launch_mha_core(qkv, att, B, S, C, cfg.n_heads, st)) return 1;
        return sbgm_launch_attn_out(att, x, a.outw->dev(), a.outb->dev(), a.ln2g->dev(), a.ln2b->dev(), a.f1w->dev(), a.f1b->dev(), a.f2w->dev(),
                                    a.f2b->dev(), x, M, C, LN_EPS, st);
    }
    float* n1 = wsalloc((size_t)M * C);
    if (!n1) return 1;
    float* qkv = wsalloc((size_t)M * 3 * C);
    if (!qkv) return 1;
    float* att = wsalloc((size_t)M * C);
    if (!att) return 1;
    float* h = wsalloc((size_t)M * C);
    if (!h) return 1;
    float* f1 = wsalloc((size_t)M * C);
    if (!f1) return 1;
    const ConvGeom lin{1, 1, 1, 0};
    // With the route's fold (Routes::ln_fold) neither LayerNorm is launched: in_proj reads x and ff[0] reads h through the folded operands
    // (in_mode 3).  n1 is carved all the same, so every later buffer keeps its address and the measured high-water mark serves both forms.
    // A tuning evaluation runs both forms, so both keys of the tile table are tuned whichever a later caller takes.
    const bool fold = routes.ln_fold && ln_fold_block(a, M);
    SBGM_CHECK(!fold || (!a.fold1->dirty && !a.fold2->dirty), "attention: the folded LayerNorm operands of %d tokens x %d channels are stale", M, C);
    ConvParams p{};
    p.B = 1; p.H = 1; p.W = M; p.Cs = C;
    p.out = qkv; p.Cout = 3 * C;
    auto folded = [&](const float* rows, const LnFold& f) {
        ConvParams q = p;
        q.x = rows; q.bias = f.h; q.in_mode = 3; q.ln_eps = LN_EPS;
        return conv(lin, q, f.w2, st);
    };
    if (!fold || tuning) {
        if (sbgm_launch_layernorm(x, n1, a.ln1g->dev(), a.ln1b->dev(), M, C, LN_EPS, st)) return 1;
        p.x = n1; p.bias = a.inb->dev();
        if (conv(lin, p, *a.inw, st)) return 1;
    }
    if (fold && folded(x, *a.fold1)) return 1;
    if (sbgm_launch_mha_core(qkv, att, B, S, C, cfg.n_heads, st)) return 1;
    p.x = att; p.out = h; p.bias = a.outb->dev(); p.Cout = C; p.res = x;
    if (conv(lin, p, *a.outw, st)) return 1;
    p.out = f1; p.res = nullptr; p.act = SBGM_ACT_GELU;   // :131-132
    if (!fold || tuning) {
        if (sbgm_launch_layernorm(h, n1, a.ln2g->dev(), a.ln2b->dev(), M, C, LN_EPS, st)) return 1;
        p.x = n1; p.bias = a.f1b->dev();
        if (conv(lin, p, *a.f1w, st)) return 1;
    }
    if (fold && folded(h, *a.fold2)) return 1;
    p.x = f1; p.out = x; p.bias = a.f2b->dev(); p.res = h; p.act = SBGM_ACT_NONE;
    return conv(lin, p, *a.f2w, st);
}

int sbgm_model::forward_impl(const float* x, const float* t, const int64_t* y, const float* cond, const float* lsm,
                             const float* topo, float* out, float* const* fmaps_out, int B, int H, int W, int bn_train,
                             hipStream_t st) {
    SBGM_CHECK(B >= 1 && H >= 32 && W >= 32 && H % 32 == 0 && W % 32 == 0,
               "forward: H,W must be positive multiples of 32 (five stride-2 stages), got B=%d H=%d W=%d", B, H, W);
    SBGM_CHECK(x && t && out, "forward: x, t and out are required");
    SBGM_CHECK((cfg.n_cond_channels > 0) == (cond != nullptr), "forward: cond_img presence does not match the model (%d channels)", cfg.n_cond_channels);
    SBGM_CHECK((cfg.n_lsm_channels > 0) == (lsm != nullptr), "forward: lsm_cond presence does not match the model");
    SBGM_CHECK((cfg.n_topo_channels > 0) == (topo != nullptr), "forward: topo_cond presence does not match the model");
    SBGM_CHECK(!(y && !label_emb), "forward: y given but the model has no label embedding");
    if (sbgm_model_check_complete(this)) return 1;
    if (!tuning) {
        SBGM_CHECK(fwd_need(B, H, W, bn_train) <= ws_bytes, "forward: workspace not prepared for B=%d H=%d W=%d", B, H, W);
        ws_used = 0;
    }
    if (refresh_derived(st, routes.up_lowres, H, W, routes.ln_fold, B)) return 1;
    partial = wsalloc(PARTIAL_FLOATS);
    if (!partial) return 1;

    // ---- pack inputs, time embedding -------------------------------------------------------------------------------
    PackSrc src{};
    auto push = [&](const float* p, int c) { if (p && c) { src.ptr[src.n] = p; src.ch[src.n] = c; ++src.n; } };
    push(x, 1); push(lsm, cfg.n_lsm_channels); push(topo, cfg.n_topo_channels); push(cond, cfg.n_cond_channels);
    float* x0 = wsalloc((size_t)B * H * W * cs_in);
    if (!x0) return 1;
    // A step sampler's evaluation whose final mix forms the decoder's last skip itself (Routes::skip_mix) launches neither this packing
    // nor conv1 below: the composed stem reads x, and nothing else reads fm[0].  x0 and fm[0] are carved all the same, so every later
    // buffer keeps its address and the measured high-water mark covers the route.
    const bool skip_mix = routes.skip_mix && routes.stem && routes.fin_lowres && !tuning && !prof && fmaps_out == nullptr;
    if (!skip_mix && sbgm_launch_pack_input(src, x0, B, H, W, cs_in, st)) return 1;

    // An EM / PC run without labels keeps its time biases itself (routes.tbrun); the workspace is carved the same either
    // way, so every later buffer keeps its address and the measured high-water mark serves both
    SBGM_CHECK(!routes.tbrun || routes.run_B == B, "forward: the run's time biases hold %d samples, not %d", routes.run_B, B);
    float* emb_ws = wsalloc((size_t)5 * B * D);
    if (!emb_ws) return 1;
    float* tb[9];
    for (int i = 0; i < 9; ++i) {
        tb[i] = wsalloc((size_t)B * (i < 5 ? FMAP_CH[i] : dec[i - 5].cout));
        if (!tb[i]) return 1;
    }
    if (routes.tbrun) {
        int off4[10];
        time_row_layout(off4);
        for (int i = 0; i < 9; ++i) tb[i] = routes.tbrun + (size_t)B * off4[i] * 4;
    } else if (time_biases(t, y, B, emb_ws, tb, 0, st)) return 1;

    // GroupNorm: 64 chunks x B x G x 2 doubles (G = C <= 512 for InstanceNorm); BatchNorm: 24 B x C
    const size_t n_groups = (size_t)B * (cfg.decoder_norm == SBGM_NORM_GROUP ? std::min(cfg.gn_groups, 512) : 512);
    double* stats = reinterpret_cast<double*>(wsalloc(std::max<size_t>(6 * 512, n_groups * 64 * 4)));
    if (!stats) return 1;

    // conv + BatchNorm (+res, relu, late time bias): eval folds BN into the conv epilogue, train runs it after
    auto conv_bn = [&](const ConvGeom& g, const float* in, int h, int w, int cs, const ConvW& cw, BNW& bnw, int cout,
                       const float* res, bool relu, const float* tb_after, float* o) -> int {
        ConvParams p{};
        p.x = in; p.B = B; p.H = h; p.W = w; p.Cs = cs; p.Cout = cout;
        if (!bn_train) {
            p.out = o; p.scale = bnw.scale; p.bias = bnw.bias; p.res = res; p.act = relu ? SBGM_ACT_RELU : SBGM_ACT_NONE;
            p.tbias = tb_after; p.tbias_after_act = 1;
            return conv(g, p, *cw.w, st);
        }
        const int oh = (h + 2 * g.pad - g.kh) / g.stride + 1, ow = (w + 2 * g.pad - g.kw) / g.stride + 1;
        float* raw = wsalloc((size_t)B * oh * ow * cout);
        if (!raw) return 1;
        p.out = raw;
        if (conv(g, p, *cw.w, st)) return 1;
        return sbgm_launch_batchnorm_train(raw, o, bnw.g->dev(), bnw.b->dev(), bnw.rm->dev(), bnw.rv->dev(), res, tb_after, relu, B,
                                           oh * ow, cout, BN_EPS, BN_MOMENTUM, stats, st);
    };

    // ---- encoder ------------------------------------------------------------------------------------------------------
    float* fm[5];
    int fh[5], fw[5];
    fh[0] = H / 2; fw[0] = W / 2;
    fm[0] = wsalloc((size_t)B * fh[0] * fw[0] * 64);
    if (!fm[0]) return 1;
    if (!skip_mix) {
        ConvParams p{};
        p.x = x0; p.out = fm[0]; p.tbias = tb[0]; p.B = B; p.H = H; p.W = W; p.Cs = cs_in; p.Cout = 64;
        p.c_real = cin_total == 2 ? 2 : 0;
        if (conv(ConvGeom{8, 8, 2, 3}, p, *conv1.w, st)) return 1;                                        // score_unet.py:312-316
    }
    int ch = H / 4, cw_ = W / 4;
    float* cur = wsalloc((size_t)B * ch * cw_ * 64);
    if (!cur) return 1;
    if (routes.stem) {
        // sampler runs: conv2(fm[0]) + bn1 + ReLU straight from x, the run's condition term and tb[0] (conv_stem22.hip); conv1 above
        // still writes fm[0], the decoder's last skip, unless the final mix forms it (skip_mix)
        float* o = cur;
        if (bn_train) {
            o = wsalloc((size_t)B * ch * cw_ * 64);
            if (!o) return 1;
        }
        if (sbgm_launch_conv_stem22(x, 1, 0, cin_total, stem.wc, stem.sb, tb[0], routes.stem_T, bn_train ? nullptr : bn1.scale,
                                    bn_train ? nullptr : bn1.bias, bn_train ? 0 : 1, o, B, H, W, st)) return 1;
        if (bn_train && sbgm_launch_batchnorm_train(o, cur, bn1.g->dev(), bn1.b->dev(), bn1.rm->dev(), bn1.rv->dev(), nullptr, nullptr, true, B,
                                                    ch * cw_, 64, BN_EPS, BN_MOMENTUM, stats, st)) return 1;
    } else if (conv_bn(ConvGeom{8, 8, 2, 3}, fm[0], fh[0], fw[0], 64, conv2, bn1, 64, nullptr, true, nullptr, cur)) return 1;   // :321-325
    int cc = 64;
    for (int li = 0; li < 4; ++li) {
        const int nb = (int)layers[li].size();
        for (int bi = 0; bi < nb; ++bi) {
            BlockW& b = layers[li][bi];
            const int oh = ch / b.stride, ow = cw_ / b.stride;
            float* y1 = wsalloc((size_t)B * oh * ow * b.cout);
            if (!y1) return 1;
            const float* idn = cur;
            if (b.has_ds && !bn_train) {
                // conv1 + bn1 + ReLU and the shortcut's 1x1 + BatchNorm read the same input and do not depend on each other: one launch
                float* d = wsalloc((size_t)B * oh * ow * b.cout);
                if (!d) return 1;
                ConvParams pm{}, pa{};
                pm.x = cur; pm.B = B; pm.H = ch; pm.W = cw_; pm.Cs = cc; pm.Cout = b.cout;
                pm.tbias_after_act = 1;
                pa = pm;
                pm.out = y1; pm.scale = b.bn1.scale; pm.bias = b.bn1.bias; pm.act = SBGM_ACT_RELU;
                pa.out = d; pa.scale = b.dsbn.scale; pa.bias = b.dsbn.bias; pa.act = SBGM_ACT_NONE;
                if (conv_pair(ConvGeom{3, 3, b.stride, 1}, pm, *b.c1.w, ConvGeom{1, 1, b.stride, 0}, pa, *b.ds.w, st)) return 1;
                idn = d;
            } else {
                if (conv_bn(ConvGeom{3, 3, b.stride, 1}, cur, ch, cw_, cc, b.c1, b.bn1, b.cout, nullptr, true, nullptr, y1)) return 1;
                if (b.has_ds) {
                    float* d = wsalloc((size_t)B * oh * ow * b.cout);
                    if (!d) return 1;
                    if (conv_bn(ConvGeom{1, 1, b.stride, 0}, cur, ch, cw_, cc, b.ds, b.dsbn, b.cout, nullptr, false, nullptr, d)) return 1;
                    idn = d;
                }
            }
            float* y2 = wsalloc((size_t)B * oh * ow * b.cout);
            if (!y2) return 1;
            const float* tba = (bi == nb - 1) ? tb[li + 1] : nullptr;                        // fmap + t_emb (:332,341,350,359)
            if (conv_bn(ConvGeom{3, 3, 1, 1}, y1, oh, ow, b.cout, b.c2, b.bn2, b.cout, idn, true, tba, y2)) return 1;
            cur = y2; ch = oh; cw_ = ow; cc = b.cout;
        }
        if (enc_has_attn[li + 1] && attention(enc_attn[li + 1], cur, B, ch * cw_, st)) return 1;
        fm[li + 1] = cur; fh[li + 1] = ch; fw[li + 1] = cw_;
    }
    if (fmaps_out) {
        for (int i = 0; i < 5; ++i)
            if (fmaps_out[i])
                SBGM_HIP(hipMemcpyAsync(fmaps_out[i], fm[i], (size_t)B * fh[i] * fw[i] * FMAP_CH[i] * 4, hipMemcpyDeviceToDevice, st));
    }

    // ---- decoder ------------------------------------------------------------------------------------------------------
    // Fused path (default): no GroupNorm-apply or upsample pass between the convolutions of a block.  conv_up reads the
    // low-resolution map and interpolates while staging (in_mode 2, with the PREVIOUS block's pending GroupNorm + skip + time
    // bias + activation applied to the low-res pixels), `conv` reads conv_up's raw output through norm1's affine (in_mode 1);
    // the statistics come out of the producing convolution's epilogue and one tiny finalize launch turns them into the
    // per-(sample, channel) scale / shift.  A block whose output feeds attention keeps the separate apply pass, and so do maps
    // narrower than 32 pixels: the fused staging costs the (compute-bound) convolution 2-4 us more than the plain one (measured,
    // tools/bench_fused_conv.py), which only pays where the pass it replaces streams more than ~8 MB (64 / 128 channels at
    // 32x32 and up; at 16x16 x 256 channels the separate 4 us pass is cheaper).  SBGM_NO_FUSED_DECODER=1 forces the separate
    // passes everywhere.
    const int G_of = cfg.gn_groups;
    auto groups = [&](int c) { return cfg.decoder_norm == SBGM_NORM_GROUP ? std::max(1, std::min(G_of, c)) : c; };
    struct Pending { const float* raw; const float* affine; const float* skip; int act; bool live; } pend{nullptr, nullptr, nullptr, SBGM_ACT_NONE, false};
    // statistics of `t` [B][hw][c] for its GroupNorm: from the convolution epilogue (chunks > 0) or a separate partial pass
    auto ensure_stats = [&](const float* t, int hw, int c, int& chunks) -> int {
        if (chunks > 0) return 0;
        return sbgm_launch_gn_partial(t, stats, B, hw, c, groups(c), &chunks, st);
    };
    // conv_up of a block: input `in` [B][ch][cw_][ci] (or the pending raw map), output raw [B][2ch][2cw_][ci] (+ bias)
    auto conv_up = [&](const ConvW& cw, const float* in, int ci, int oh, int ow, ConvParams& p, float* out_raw) -> int {
        p = ConvParams{};
        p.out = out_raw; p.bias = cw.b->dev(); p.B = B; p.H = oh; p.W = ow; p.Cs = ci; p.Cout = ci;
        if (can_fuse(cw, ci, ow)) {
            p.in_mode = 2;
            p.x = pend.live ? pend.raw : in;
            if (pend.live) { p.in_affine = pend.affine; p.in_skip = pend.skip; p.in_act = pend.act; }
            pend.live = false;
            return 0;
        }
        SBGM_CHECK(!pend.live, "decoder: a pending normalisation reached an unfused convolution");
        float* up = wsalloc((size_t)B * oh * ow * ci);
        if (!up) return 1;
        if (sbgm_launch_upsample2x(in, up, B, oh / 2, ow / 2, ci, st)) return 1;
        p.x = up;
        return 0;
    };
    cur = fm[4]; ch = fh[4]; cw_ = fw[4];
    for (int i = 0; i < 4; ++i) {
        DecW& d = dec[i];
        const int oh = 2 * ch, ow = 2 * cw_;
        SBGM_CHECK(oh == fh[3 - i] && ow == fw[3 - i] && d.cout == FMAP_CH[3 - i], "decoder/skip shape mismatch at block %d", i);
        float* a = wsalloc((size_t)B * oh * ow * d.cin);
        if (!a) return 1;
        ConvParams p{};
        int gn1_chunks = 0, normed1 = 0;
        // A small-map block (up_lowres): conv_up(up(cur)) as the 1x1 tap mix on the low-res map and the gather, which also forms norm1
        // where a workgroup holds a whole group.  Z is reserved on every route, so the workspace's high-water mark, measured by a plain
        // evaluation, covers the route as well; a tuning evaluation runs both forms, so the mix and the parent convolution are both tuned.
        const bool lowres = up_lowres_block(i, ch, cw_);
        float* zb = lowres ? wsalloc(sbgm_up_lowres_ws_floats(B, ch, cw_, d.cin)) : nullptr;
        if (lowres && !zb) return 1;
        const bool take_lowres = lowres && routes.up_lowres;
        if (take_lowres) {
            SBGM_CHECK(!pend.live, "decoder: a pending normalisation reached a low-resolution conv_up");
            p.x = cur; p.out = zb; p.B = B; p.H = ch; p.W = cw_; p.Cs = d.cin; p.Cout = 9 * d.cin;
            if (conv(ConvGeom{1, 1, 1, 0}, p, uplow[i].w1, st)) return 1;
            const bool gn = cfg.decoder_norm == SBGM_NORM_GROUP;
            if (sbgm_launch_up_gather(zb, d.up.b->dev(), a, d.n1g ? d.n1g->dev() : nullptr, d.n1b ? d.n1b->dev() : nullptr, stats,
                                      gn ? groups(d.cin) : 0, GN_EPS, B, ch, cw_, d.cin, &gn1_chunks, &normed1, st)) return 1;
        }
        if (take_lowres && !tuning) {                // `a` (and what the gather did of norm1) stands
        } else if (cfg.decoder_transpose) {          // ConvTranspose2d: 1x1 conv to 4*cin phase-major channels, then depth -> space
            float* up = wsalloc((size_t)B * oh * ow * d.cin);
            if (!up) return 1;
            p.x = cur; p.out = up; p.bias = d.up.b->dev(); p.B = B; p.H = ch; p.W = cw_; p.Cs = d.cin; p.Cout = 4 * d.cin;
            if (conv(ConvGeom{1, 1, 1, 0}, p, *d.up.w, st)) return 1;
            if (sbgm_launch_depth_space2(up, a, B, ch, cw_, d.cin, 1, st)) return 1;
        } else {
            if (conv_up(d.up, cur, d.cin, oh, ow, p, a)) return 1;
            p.gn_stats = stats; p.gn_groups = groups(d.cin);        // GroupNorm statistics in the epilogue when the LDS kernel runs
            if (conv(ConvGeom{3, 3, 1, 1}, p, *d.up.w, st)) return 1;
            gn1_chunks = sbgm_tile_gn_chunks(p, last_tile);
            normed1 = 0;
        }
        float* c2 = wsalloc((size_t)B * oh * ow * d.cout);
        if (!c2) return 1;
        if (!normed1 && ensure_stats(a, oh * ow, d.cin, gn1_chunks)) return 1;
        p = ConvParams{};
        p.B = B; p.H = oh; p.W = ow; p.Cs = d.cin;
        p.x = a; p.out = c2; p.bias = d.conv.b->dev(); p.Cout = d.cout;
        if (normed1) {                               // the gather stored norm1's output
        } else if (can_fuse(d.conv, d.cin, ow)) {    // norm1 applied while `conv` stages its patch
            float* aff1 = wsalloc((size_t)B * d.cin * 2);
            if (!aff1) return 1;
            if (sbgm_launch_gn_finalize(stats, gn1_chunks, d.n1g ? d.n1g->dev() : nullptr, d.n1b ? d.n1b->dev() : nullptr, nullptr, aff1, B, oh * ow,
                                        d.cin, groups(d.cin), GN_EPS, st)) return 1;
            p.in_mode = 1; p.in_affine = aff1;
        } else if (sbgm_launch_groupnorm_apply(a, a, d.n1g ? d.n1g->dev() : nullptr, d.n1b ? d.n1b->dev() : nullptr, nullptr, nullptr,
                                               SBGM_ACT_NONE, B, oh * ow, d.cin, groups(d.cin), GN_EPS, stats, gn1_chunks, st)) return 1;
        p.gn_stats = stats; p.gn_groups = groups(d.cout);
        if (conv(ConvGeom{3, 3, 1, 1}, p, *d.conv.w, st)) return 1;
        int gn2_chunks = sbgm_tile_gn_chunks(p, last_tile);
        if (ensure_stats(c2, oh * ow, d.cout, gn2_chunks)) return 1;
        const ConvW& next_up = i < 3 ? dec[i + 1].up : fin_up;
        if (!d.has_attn && can_fuse(next_up, d.cout, 2 * ow)) {
            // norm2 + skip + time bias + activation stay pending: the next conv_up applies them to the low-res pixels it loads
            float* aff2 = wsalloc((size_t)B * d.cout * 2);
            if (!aff2) return 1;
            if (sbgm_launch_gn_finalize(stats, gn2_chunks, d.n2g ? d.n2g->dev() : nullptr, d.n2b ? d.n2b->dev() : nullptr, tb[5 + i], aff2, B, oh * ow,
                                        d.cout, groups(d.cout), GN_EPS, st)) return 1;
            pend = Pending{c2, aff2, fm[3 - i], cfg.decoder_activation, true};
        } else {
            if (sbgm_launch_groupnorm_apply(c2, c2, d.n2g ? d.n2g->dev() : nullptr, d.n2b ? d.n2b->dev() : nullptr, fm[3 - i], tb[5 + i],
                                            cfg.decoder_activation, B, oh * ow, d.cout, groups(d.cout), GN_EPS, stats, gn2_chunks, st)) return 1;
            if (d.has_attn && attention(d.attn, c2, B, oh * ow, st)) return 1;
        }
        cur = c2; ch = oh; cw_ = ow;
    }
    {   // final block: no norms, no skip, no time, identity activation (score_unet.py:726-730, :757)
        const int ci = dec[3].cout;
        ConvParams p{};
        if (cfg.decoder_transpose) {
            float* up = wsalloc((size_t)B * H * W * ci);
            if (!up) return 1;
            float* a = wsalloc((size_t)B * H * W * ci);
            if (!a) return 1;
            p.x = cur; p.out = up; p.bias = fin_up.b->dev(); p.B = B; p.H = ch; p.W = cw_; p.Cs = ci; p.Cout = 4 * ci;
            if (conv(ConvGeom{1, 1, 1, 0}, p, *fin_up.w, st)) return 1;
            if (sbgm_launch_depth_space2(up, a, B, ch, cw_, ci, 1, st)) return 1;
            return sbgm_launch_conv3x3_cout1(a, fin_conv.w->dev(), fin_conv.b->dev(), t, cfg.sigma, out, B, H, W, ci, st);
        }
        if (routes.fin_lowres && !tuning) {
            // conv(conv_up(up(.))) with the channels mixed at low resolution: Z = Wz . v on the low-res map (the pending normalisation
            // applied on load, or the finished map where nothing is pending), then the 5x5 gather through the bilinear x2.  A tuning
            // evaluation keeps timing the composed 3x3 convolution below: SBGM_NO_FINAL_LOWRES=1 still runs it.
            float* zb = wsalloc(sbgm_final_lowres_ws_floats(B, ch, cw_));
            if (!zb) return 1;
            const bool live = pend.live;
            pend.live = false;
            if (skip_mix) {
                // the pending skip is fm[0], which nothing wrote: conv1(x || cond) + tb[0] inside the mix, from x, the run's Sc and tb[0]
                SBGM_CHECK(live && pend.skip == fm[0] && ci == 64, "forward: the final mix cannot form a skip that is not the stem's map");
                if (sbgm_launch_final_mix_skipx(pend.raw, pend.affine, pend.act, fin.wz, x, routes.skip_Sc, tb[0], stem.w1x, zb, B, ch, cw_, ci,
                                                st)) return 1;
                return sbgm_launch_final_gather(zb, fin.beta, t, cfg.sigma, out, B, ch, cw_, st);
            }
            if (sbgm_launch_final_mix(live ? pend.raw : cur, live ? pend.affine : nullptr, live ? pend.skip : nullptr,
                                      live ? pend.act : SBGM_ACT_NONE, fin.wz, zb, B, ch, cw_, ci, st)) return 1;
            return sbgm_launch_final_gather(zb, fin.beta, t, cfg.sigma, out, B, ch, cw_, st);
        }
        if (routes.fin) {
            // conv(conv_up(.)) composed: one 3x3 convolution from ci to the 9 taps (16 channels stored), rows [M][16], then the gather
            const Pending pend0 = pend;
            if (conv_up(ConvW{&fin.cw, &fin.cb}, cur, ci, H, W, p, nullptr)) return 1;
            float* d = wsalloc((size_t)16 * B * H * W);
            if (!d) return 1;
            p.Cout = 16; p.out = d;
            if (conv(ConvGeom{3, 3, 1, 1}, p, fin.cw, st)) return 1;
            if (sbgm_launch_tap_gather_rows(d, fin_conv.b->dev(), t, cfg.sigma, out, B, H, W, st)) return 1;
            if (!tuning) return 0;
            pend = pend0;                        // a tuning evaluation also times the projection form below (plain forward, RK45)
        }
        if (conv_up(fin_up, cur, ci, H, W, p, nullptr)) return 1;
        if (ci == 64) {
            // conv_up's 64-channel output feeds only the linear 3x3 Cout=1 conv: project onto its 9 taps in the epilogue
            // (9 floats per pixel instead of 64) and finish with a 9-point gather.
            p.proj_w = fin_conv.w->dev();
            float* d = wsalloc((size_t)9 * B * H * W * 4);      // up to 4 partial planes (2-D Winograd tiles of 16 channels)
            if (!d) return 1;
            p.out = d; p.proj_out = d;
            if (conv(ConvGeom{3, 3, 1, 1}, p, *fin_up.w, st)) return 1;
            if (sbgm_launch_tap_stencil(d, fin_conv.b->dev(), t, cfg.sigma, out, B, H, W, st, sbgm_tile_proj_parts(p, last_tile))) return 1;
        } else {
            float* a = wsalloc((size_t)B * H * W * ci);
            if (!a) return 1;
            p.out = a;
            if (conv(ConvGeom{3, 3, 1, 1}, p, *fin_up.w, st)) return 1;
            if (sbgm_launch_conv3x3_cout1(a, fin_conv.w->dev(), fin_conv.b->dev(), t, cfg.sigma, out, B, H, W, ci, st)) return 1;
        }
    }
    return 0;
}

// torch.linspace(start, end, n) in fp32, as ATen fills it (symmetric about the midpoint)
static std::vector<float> linspace_f32(float start, float end, int n) {
    std::vector<float> v(n);
    if (n == 1) { v[0] = start; return v; }
    const float step = (end - start) / (float)(n - 1);
    const int half = n / 2;
    for (int i = 0; i < n; ++i) v[i] = i < half ? start + step * (float)i : end - step * (float)(n - 1 - i);
    return v;
}

// Step tables, in the reference's precision.  Each builder writes the N rows of its kind into the staging buffer and returns the row
// size and the time of the run's first evaluation.
struct StepTable { size_t row_bytes; float t_first; };

// Euler-Maruyama: torch.linspace times in fp32 (score_sampling.py:96-97, :102-103, :124-125)
static StepTable em_table(void* stage, int N, float sig, float eps) {
    StepScalars* tab = static_cast<StepScalars*>(stage);
    const std::vector<float> ts = linspace_f32(1.0f, eps, N);
    const float dt = ts[0] - ts[1];
    for (int i = 0; i < N; ++i) {
        const float g = powf(sig, ts[i]);
        tab[i] = StepScalars{ts[i], g * g, dt, sqrtf(dt) * g, ts[std::min(i + 1, N - 1)]};
    }
    return {sizeof(StepScalars), tab[0].t};
}

// predictor-corrector: np.linspace times in float64, stored as fp32 (score_sampling.py:169-170, :176, :207, :224-227)
static StepTable pc_table(void* stage, int N, float sig, float eps) {
    StepScalars* tab = static_cast<StepScalars*>(stage);
    std::vector<double> ts(N);
    const double step = ((double)eps - 1.0) / (double)(N - 1);
    for (int i = 0; i < N; ++i) ts[i] = 1.0 + (double)i * step;
    ts[N - 1] = (double)eps;
    const float dt = (float)(ts[0] - ts[1]);
    for (int i = 0; i < N; ++i) {
        const float tf = (float)ts[i];
        const float g = powf(sig, tf);
        tab[i] = StepScalars{tf, g * g, dt, sqrtf((g * g) * dt), (float)ts[std::min(i + 1, N - 1)]};
    }
    return {sizeof(StepScalars), tab[0].t};
}

// The Karras ladder of the few-step samplers for the VE SDE std(t) = sqrt((sigma^2t - 1) / (2 ln sigma)): sigma_0 .. sigma_{N-1} between
// sigma_min and sigma_max (<= 0: the trained range [std(eps), std(1)]; other values are clipped to it), sigma_N = 0, and t(sigma) =
// log1p(2 ln sigma * s^2) / (2 ln sigma) clamped to [eps, 1].  float64 throughout.
struct KarrasLadder {
    double ls, lo, hi, eps;
    std::vector<double> sg;                                // [N + 1]
    KarrasLadder(int N, double sig, double eps_, float sigma_min, float sigma_max, float rho_) : ls(std::log(sig)), eps(eps_), sg(N + 1) {
        auto std_of = [&](double t) { return std::sqrt(std::expm1(2.0 * t * ls) / (2.0 * ls)); };
        lo = std_of(eps); hi = std_of(1.0);
        const double smin = sigma_min > 0 ? std::min(hi, std::max(lo, (double)sigma_min)) : lo;
        const double smax = sigma_max > 0 ? std::min(hi, std::max(lo, (double)sigma_max)) : hi;
        const double rho = rho_, a0 = std::pow(smax, 1.0 / rho), a1 = std::pow(smin, 1.0 / rho);
        for (int i = 0; i < N; ++i) sg[i] = std::pow(a0 + (double)i / (double)(N - 1) * (a1 - a0), rho);
        sg[0] = smax; sg[N - 1] = smin; sg[N] = 0.0;       // the ends exactly (the power round trip is off by an ulp)
    }
    double t_of(double s) const {                          // clamped in sigma too: sigma >= std(1) is t = 1 exactly
        return s >= hi ? 1.0 : s <= lo ? eps : std::min(1.0, std::max(eps, std::log1p(2.0 * ls * s * s) / (2.0 * ls)));
    }
};

// EDM Heun step table (Karras et al. 2022, Alg. 2): the ladder with the churn gamma_i.  Stored as fp32: score_sampling.edm_heun_schedule.
static StepTable edm_table(void* stage, int N, double sig, double eps, const sbgm_model::EdmArgs& e) {
    EdmStep* tab = static_cast<EdmStep*>(stage);
    const KarrasLadder k(N, sig, eps, e.sigma_min, e.sigma_max, e.rho);
    const std::vector<double>& sg = k.sg;
    const double gmax = std::min((double)e.s_churn / (double)N, std::sqrt(2.0) - 1.0);
    for (int i = 0; i < N; ++i) {
        double g = (e.s_tmin <= sg[i] && sg[i] <= e.s_tmax) ? gmax : 0.0;
        g = std::min(g, sg[0] / sg[i] - 1.0);
        const double sh = sg[i] * (1.0 + g);
        tab[i] = EdmStep{(float)sg[i], (float)sh, (float)sg[i + 1], (float)k.t_of(sh), (float)k.t_of(sg[i + 1]),
                         (float)((double)e.s_noise * std::sqrt(std::max(0.0, sh * sh - sg[i] * sg[i])))};
    }
    return {sizeof(EdmStep), tab[0].t_hat};
}

// DPM-Solver++(2M) step table (Lu et al. 2022; eta > 0: 2M SDE, midpoint form) on the same ladder, alpha = 1: the coefficients of
// x_{i+1} = c_x x_i + c_0 D_i + c_1 D_{i-1} + c_z z_i (kernels.h: DpmStep).  Stored as fp32: score_sampling.dpmpp_2m_schedule.
static StepTable dpm_table(void* stage, int N, double sig, double eps, const sbgm_model::DpmArgs& d) {
    DpmStep* tab = static_cast<DpmStep*>(stage);
    const KarrasLadder k(N, sig, eps, d.sigma_min, d.sigma_max, d.rho);
    const std::vector<double>& sg = k.sg;
    const double eta = d.eta;
    double h_prev = 0.0;
    for (int i = 0; i < N; ++i) {
        double c_x = 0.0, c_0 = 1.0, c_1 = 0.0, c_z = 0.0;   // the last step: x_N = D_{N-1}
        if (i + 1 < N) {
            const double h = std::log(sg[i] / sg[i + 1]), a = -std::expm1(-(1.0 + eta) * h);
            c_x = sg[i + 1] / sg[i] * std::exp(-eta * h);
            c_0 = a;
            if (i >= 1) {
                const double r = h_prev / h;
                c_0 = a * (1.0 + 1.0 / (2.0 * r));
                c_1 = -a / (2.0 * r);
            }
            c_z = (double)d.s_noise * sg[i + 1] * std::sqrt(std::max(0.0, -std::expm1(-2.0 * eta * h)));
            h_prev = h;
        }
        tab[i] = DpmStep{(float)sg[i], (float)k.t_of(sg[i]), (float)k.t_of(sg[i + 1]), (float)c_x, (float)c_0, (float)c_1, (float)c_z};
    }
    return {sizeof(DpmStep), tab[0].t};
}

// Condition tensors of a run's network evaluations: the caller's, or with guidance (guided_score_fn :27-43) per-call copies of 2B rows
// whose second half is the unconditional input (null class 0, zero cond_img, geo fields with their mask channel zeroed).  The copies
// are freed on every exit path, after the stream has drained.
struct SamplerConds {
    const int64_t* y;
    const float *cond, *lsm, *topo;
    hipStream_t st;
    std::vector<void*> bufs;
    SamplerConds(const sbgm_sampler_args& a, hipStream_t s) : y(a.y), cond(a.cond_img), lsm(a.lsm_cond), topo(a.topo_cond), st(s) {}
    SamplerConds(const SamplerConds&) = delete;
    ~SamplerConds() {
        if (bufs.empty()) return;
        (void)hipStreamSynchronize(st);
        for (void* p : bufs) (void)hipFree(p);
    }
    int add_unconditional(const sbgm_sampler_args& a, const sbgm_model_config& c) {
        const size_t per = (size_t)a.H * a.W, n = (size_t)a.B * per;
        // p -> [p; unconditional half]: zeros, or for a geo field with geo_ch channels a copy, with channel 1 (the mask) zeroed if 2
        auto dup = [&](auto& p, size_t bytes_half, int geo_ch) -> bool {
            void* d = nullptr;
            if (p == nullptr) return true;
            if (hipMalloc(&d, 2 * bytes_half) != hipSuccess) return false;
            bufs.push_back(d);
            (void)hipMemcpyAsync(d, p, bytes_half, hipMemcpyDeviceToDevice, st);
            char* lo = static_cast<char*>(d) + bytes_half;
            if (geo_ch == 0) (void)hipMemsetAsync(lo, 0, bytes_half, st);
            else (void)hipMemcpyAsync(lo, p, bytes_half, hipMemcpyDeviceToDevice, st);
            if (geo_ch == 2) (void)hipMemset2DAsync(lo + per * 4, 2 * per * 4, 0, per * 4, a.B, st);   // NCHW [B][2][H][W]
            p = static_cast<std::remove_reference_t<decltype(p)>>(d);
            return true;
        };
        SBGM_CHECK(dup(y, (size_t)a.B * 8, 0) && dup(cond, n * 4 * c.n_cond_channels, 0) &&
                   dup(lsm, n * 4 * c.n_lsm_channels, c.n_lsm_channels) && dup(topo, n * 4 * c.n_topo_channels, c.n_topo_channels) &&
                   hipGetLastError() == hipSuccess, "sampler: could not allocate the unconditional condition tensors");
        return 0;
    }
};

// What the drivers below share, done once: one sampler call's hold on the model.  open() validates the call and settles the workspace;
// begin() carves the run's persistent buffers off its top (the forward uses the rest), refreshes the derived weights ahead of any
// capture, builds the conditions, the routes and the tiled noise map and takes the buffers out of the forward's reach.  The destructor
// gives the workspace back and ends the routes on every exit path.  Layout from `top` (BE = B, or 2B with guidance): `lead` slabs of
// BE*per floats (slab 0: the network input, rows B.. mirror rows 0..B-1), the time vector [BE], double partials [BE], the kind's
// further slabs, the composed stem's condition term, conv1's condition share for the skip the final mix forms (skip_Sc).
struct SamplerRun {
    sbgm_model* m;
    const sbgm_sampler_args& a;
    hipStream_t st;                  // the caller's stream (ensure_step_graph points it at the capture stream meanwhile)
    const char* who;                 // the driver's name in error texts
    const bool graphed;
    const int B = a.B, H = a.H, W = a.W, slabs = sbgm_model::sampler_slabs(a.kind), lead = a.kind == SBGM_SAMPLER_RK45 ? slabs : 3;
    const bool guided = a.cfg_enabled != 0;
    const int BE = guided ? 2 * B : B;                     // samples per network evaluation
    const size_t per = (size_t)H * W, n = (size_t)B * per, slab = align_up((size_t)BE * per * 4, 256);
    char* top = nullptr;
    size_t saved_ws = 0;             // the model's ws_bytes while the run holds its slabs (0: not held)
    SamplerConds conds{a, st};       // guidance: the unconditional half is built once per run
    NoiseMap nm{};
    float* tbrun = nullptr;          // set by an EM / PC driver before begin(): the run keeps its time biases
    ~SamplerRun() { if (saved_ws) m->ws_bytes = saved_ws; m->set_routes(CALL_PLAIN); }
    size_t sc_bytes() const { return a.kind != SBGM_SAMPLER_RK45 ? m->skip_sc_bytes(BE, H, W) : 0; }
    size_t keep() const { return m->sampler_keep(BE, H, W, slabs) + sc_bytes(); }
    float* slab_at(int i) const { return reinterpret_cast<float*>(top + (i < lead ? i * slab : m->slabs_keep(BE, H, W, lead) + (i - lead) * slab)); }
    float* t_vec() const { return reinterpret_cast<float*>(top + lead * slab); }
    double* partials() const { return reinterpret_cast<double*>(top + lead * slab + align_up((size_t)BE * 4, 256)); }
    float* stem_T() const { return reinterpret_cast<float*>(top + m->slabs_keep(BE, H, W, slabs)); }
    float* skip_Sc() const { return reinterpret_cast<float*>(top + m->sampler_keep(BE, H, W, slabs)); }
    int open() {
        SBGM_CHECK(B >= 1 && H >= 32 && W >= 32, "%s: needs B >= 1 and H, W >= 32, got B=%d H=%d W=%d", who, B, H, W);
        SBGM_CHECK(!(guided && a.bn_train), "%s: guidance with train-mode BatchNorm would couple the two halves of the batch", who);
        return m->prepare_ws(BE, H, W, a.bn_train, st, slabs, sc_bytes());
    }
    int begin(bool draws_noise = true) {
        // Graph CAPTURE is illegal on the legacy default stream, so the step is captured on a private stream (capture records, it runs
        // nothing); the replays, the uploads and the final copy go to the caller's stream: ordinary stream-ordered work of the caller.
        if (graphed && !m->graph_stream) {
            SBGM_HIP(hipStreamCreateWithFlags(&m->graph_stream, hipStreamNonBlocking));
            SBGM_HIP(hipEventCreateWithFlags(&m->ev_replayed, hipEventDisableTiming));
        }
        top = m->ws + m->ws_bytes - keep();
        if (m->refresh_derived(st, a.kind != SBGM_SAMPLER_RK45, H, W, a.kind != SBGM_SAMPLER_RK45, BE)) return 1;
        if (guided && conds.add_unconditional(a, m->cfg)) return 1;
        if (a.kind != SBGM_SAMPLER_RK45) {
            // The run's condition term T: the composed filter over the channels that do not change from step to step (lsm, topo, cond_img,
            // in conv1's order after x).  On every call, outside the captured step: a cached step graph is replayed on new condition
            // contents at the same addresses.
            if (m->stem.prepare(*m->conv1.w, *m->conv2.w, m->cin_total, st)) return 1;
            const float *srcs[3] = {conds.lsm, conds.topo, conds.cond}, *term = nullptr;
            const int chs[3] = {m->cfg.n_lsm_channels, m->cfg.n_topo_channels, m->cfg.n_cond_channels};
            for (int i = 0, c0 = 1; i < 3 && m->stem.on; c0 += chs[i++]) {
                if (!chs[i]) continue;
                if (sbgm_launch_conv_stem22(srcs[i], chs[i], c0, m->cin_total, m->stem.wc, nullptr, nullptr, term, nullptr, nullptr, 0, stem_T(), BE, H, W, st)) return 1;
                term = stem_T();
            }
            // The same for the decoder's last skip where the final mix forms it (skip_mix_route): conv1 is linear, so its share over those
            // channels, Sc, is one pack_input with the x slot left zero and one conv1 launch without time bias into the run's buffer,
            // staged through the forward's part of the workspace, which nothing uses between evaluations.
            const bool skip_mix = m->skip_mix_route(W);
            const float* sc = nullptr;
            if (skip_mix && m->cin_total > 1) {
                PackSrc src{};
                src.c0 = 1;
                for (int i = 0; i < 3; ++i)
                    if (chs[i]) { src.ptr[src.n] = srcs[i]; src.ch[src.n] = chs[i]; ++src.n; }
                m->ws_used = 0;
                m->partial = m->wsalloc(sbgm_model::PARTIAL_FLOATS);
                float* x0 = m->partial ? m->wsalloc((size_t)BE * H * W * m->cs_in) : nullptr;
                if (!x0) return 1;
                if (sbgm_launch_pack_input(src, x0, BE, H, W, m->cs_in, st)) return 1;
                ConvParams p{};
                p.x = x0; p.out = skip_Sc(); p.B = BE; p.H = H; p.W = W; p.Cs = m->cs_in; p.Cout = 64;
                p.c_real = m->cin_total == 2 ? 2 : 0;
                if (m->conv(ConvGeom{8, 8, 2, 3}, p, *m->conv1.w, st)) return 1;
                sc = skip_Sc();
            }
            m->set_routes(CALL_SDE_RUN, term, tbrun, BE, skip_mix, sc);
        }
        if (a.tile_origins && draws_noise) {
            SBGM_CHECK(W % 4 == 0 && a.domain_w >= W, "%s: tiled noise needs W %% 4 == 0 and domain_w >= W (W=%d, domain_w=%d)", who, W, a.domain_w);
            nm = NoiseMap{a.tile_origins, H, W / 4, (a.domain_w + 3) / 4};
        }
        saved_ws = m->ws_bytes;
        m->ws_bytes -= keep();       // forward() must not touch the run's slabs
        return 0;
    }
    // One (possibly guided) score evaluation of slab 0 at t_vec() into dst[0 .. n), with guidance through scratch[0 .. 2n): in place for
    // the SDE steps (dst = scratch = the score slab), from a scratch slab into the stage's own for the ODE.
    int evaluate(float* dst, float* scratch, float w) {
        float* xs = slab_at(0);
        if (guided) SBGM_HIP(hipMemcpyAsync(xs + n, xs, n * 4, hipMemcpyDeviceToDevice, st));
        if (m->forward(xs, t_vec(), conds.y, conds.cond, conds.lsm, conds.topo, guided ? scratch : dst, nullptr, BE, H, W, a.bn_train, st)) return 1;
        return guided ? sbgm_launch_cfg_combine(dst, scratch, scratch + n, w, n, st) : 0;
    }
    // ensure_step_graph under k = value-initialised (the padding bytes compare equal) + the kind's own fields + what every kind bakes in
    int capture(sbgm_model::StepGraphKey& k, const std::function<int()>& body) {
        k.B = B; k.H = H; k.W = W; k.kind = a.kind; k.guided = guided; k.bn_train = a.bn_train;
        k.y = conds.y; k.cond = conds.cond; k.lsm = conds.lsm; k.topo = conds.topo;
        k.ws = m->ws; k.ws_bytes = saved_ws; k.cfg = a.cfg_scale; k.plan_gen = m->plan_gen;
        return m->ensure_step_graph(k, guided, st, body);
    }
    int replay_done(int rc) {        // after the last replay; a guided graph goes: its condition copies are freed when the call returns
        if (graphed && m->step_exec && hipEventRecord(m->ev_replayed, st) != hipSuccess && !rc) { sbgm_set_error("hipEventRecord failed"); rc = 2; }
        if (graphed && guided) m->drop_step_graph();
        return rc;
    }
};

int sbgm_model::sampler(const sbgm_sampler_args& a, hipStream_t caller, const EdmArgs* edm, const HeldArgs* held,
                        const JointArgs* joint, const DpmArgs* dpm) {
    const bool heun = edm != nullptr;                      // only sbgm_sampler_run_edm passes EDM arguments
    const bool dpm2m = dpm != nullptr;                     // only sbgm_sampler_run_dpmpp passes 2M arguments
    const bool dpm_sde = dpm2m && dpm->eta > 0.f;          // 2M SDE: every step takes a draw
    SBGM_CHECK(!held || (held->known && held->mask), "sampler: a constrained run needs both known and known_mask");
    if (joint) {
        SBGM_CHECK(a.tile_origins != nullptr, "sampler: a joint run needs tile_origins (its samples are the tiles of one domain)");
        SBGM_CHECK(a.noise == nullptr, "sampler: a joint run draws domain-keyed in-kernel noise; it cannot take injected noise");
        SBGM_CHECK(!a.bn_train, "sampler: a joint run serves eval-mode BatchNorm only (bn_train must be 0)");
        SBGM_CHECK(joint->ramp_len >= 1, "sampler: joint ramp length %d must be >= 1", joint->ramp_len);
        SBGM_CHECK(a.B >= 1 && a.W >= 4 && a.W % 4 == 0, "sampler: a joint run needs B >= 1 and W %% 4 == 0 (B=%d, W=%d)", a.B, a.W);
        // the tile table is read back once per call (a few bytes; this waits for the stream): the blend trusts it for the ramps
        std::vector<int> org(2 * (size_t)a.B);
        SBGM_HIP(hipMemcpyAsync(org.data(), a.tile_origins, org.size() * sizeof(int), hipMemcpyDeviceToHost, caller));
        SBGM_HIP(hipStreamSynchronize(caller));
        for (int t = 0; t < a.B; ++t) {
            const int y0 = org[2 * t], x0 = org[2 * t + 1];
            SBGM_CHECK(y0 >= 0 && x0 >= 0 && x0 % 4 == 0 && y0 + a.H <= joint->domain_h && x0 + a.W <= a.domain_w,
                       "sampler: joint tile %d at (%d, %d) of %d x %d does not lie quad-aligned inside the %d x %d domain", t, y0, x0, a.H,
                       a.W, joint->domain_h, a.domain_w);
        }
    }
    SBGM_CHECK(!(heun && dpm2m), "sampler: EDM Heun and 2M arguments exclude each other");
    SBGM_CHECK(heun ? a.kind == SBGM_SAMPLER_EDM_HEUN : dpm2m ? a.kind == SBGM_SAMPLER_DPMPP_2M
                    : (a.kind == SBGM_SAMPLER_EM || a.kind == SBGM_SAMPLER_PC), "sampler: unknown kind %d", a.kind);
    SBGM_CHECK(a.num_steps >= 2, "sampler: num_steps=%d must be >= 2 (step size = t0 - t1)", a.num_steps);
    SBGM_CHECK(a.out != nullptr, "sampler: out is required");
    SamplerRun run{this, a, caller, "sampler", a.use_graph && !a.noise};
    if (run.open()) return 1;
    const int B = a.B, N = a.num_steps, BE = run.BE;
    const size_t per = run.per, n = run.n;
    hipStream_t& st = run.st;

    // ---- step table and initial state, written into the pinned staging buffer and uploaded from there --------------------------
    static_assert(sizeof(DpmStep) >= sizeof(EdmStep) && sizeof(EdmStep) >= sizeof(StepScalars), "the staging buffer is sized for the largest row");
    const size_t stage_need = (sizeof(DpmStep) + sizeof(HoldLevels) + sizeof(float)) * (size_t)N + sizeof(SamplerState);
    if (stage_pending) {                                   // the previous call's upload still reads the buffer (normally long done)
        SBGM_HIP(hipEventSynchronize(ev_stage));
        stage_pending = false;
    }
    if (h_stage_bytes < stage_need) {
        if (h_stage) SBGM_HIP(hipHostFree(h_stage));
        h_stage = nullptr;
        h_stage_bytes = std::max(stage_need, (sizeof(DpmStep) + sizeof(HoldLevels) + sizeof(float)) * (size_t)4096 + sizeof(SamplerState));
        SBGM_HIP(hipHostMalloc(reinterpret_cast<void**>(&h_stage), h_stage_bytes, hipHostMallocDefault));
    }
    if (!ev_stage) SBGM_HIP(hipEventCreateWithFlags(&ev_stage, hipEventDisableTiming));
    const float sig = cfg.sigma;
    const StepTable tab = heun ? edm_table(h_stage, N, (double)sig, (double)a.eps, *edm)
                        : dpm2m ? dpm_table(h_stage, N, (double)sig, (double)a.eps, *dpm)
                        : a.kind == SBGM_SAMPLER_EM ? em_table(h_stage, N, sig, a.eps) : pc_table(h_stage, N, sig, a.eps);
    const size_t tab_bytes = tab.row_bytes * (size_t)N;
    if (table_bytes < tab_bytes) {                         // roomy: a new table address invalidates the cached step graph
        if (d_table) SBGM_HIP(hipFree(d_table));
        d_table = nullptr;
        const size_t cap = std::max(tab_bytes, sizeof(StepScalars) * 4096);
        SBGM_HIP(hipMalloc(&d_table, cap));
        table_bytes = cap;
    }
    SamplerState* state0 = reinterpret_cast<SamplerState*>(h_stage + tab_bytes);
    *state0 = SamplerState{0ull, 0ull, (unsigned long long)a.seed, (unsigned long long)N};
    SBGM_HIP(hipMemcpyAsync(d_table, h_stage, tab_bytes, hipMemcpyHostToDevice, st));
    SBGM_HIP(hipMemcpyAsync(d_state, state0, sizeof(SamplerState), hipMemcpyHostToDevice, st));
    // Constrained EM / PC run: the levels its held pixels are re-noised to, std(t_i) and std(t_{i+1}) (0 after the last step) with std =
    // marginal_prob_std in double at the table's fp32 times, as a table parallel to the step table (EDM Heun: EdmStep has sigma_next).
    // 2M: the ladder itself, sigma_i and sigma_{i+1} as the table stores them.
    Hold hold{};
    if (held) {
        hold.known = held->known;
        hold.mask = held->mask;
        hold.z0 = heun || (dpm2m && !dpm_sde) ? a.noise : nullptr;     // the deterministic kinds hold with the run's draw 0
        hold.seed = a.seed;
    }
    if (held && !heun) {
        if (levels_rows < (size_t)N) {
            if (d_levels) SBGM_HIP(hipFree(d_levels));
            d_levels = nullptr;
            levels_rows = std::max<size_t>(N, 4096);
            SBGM_HIP(hipMalloc(reinterpret_cast<void**>(&d_levels), levels_rows * sizeof(HoldLevels)));
        }
        HoldLevels* lv = reinterpret_cast<HoldLevels*>(h_stage + tab_bytes + sizeof(SamplerState));
        const StepScalars* rows = reinterpret_cast<const StepScalars*>(h_stage);
        const double lsd = std::log((double)sig);
        for (int i = 0; i < N; ++i)
            lv[i].cur = dpm2m ? reinterpret_cast<const DpmStep*>(h_stage)[i].sigma
                              : (float)std::max(std::sqrt(std::expm1(2.0 * (double)rows[i].t * lsd) / (2.0 * lsd)), 1e-5);
        for (int i = 0; i < N; ++i) lv[i].next = i + 1 < N ? lv[i + 1].cur : 0.f;
        SBGM_HIP(hipMemcpyAsync(d_levels, lv, sizeof(HoldLevels) * (size_t)N, hipMemcpyHostToDevice, st));
        hold.levels = d_levels;
    }
    // Time rows: an EM / PC run without labels evaluates every sample at the table's time of the step, so the nine
    // time-bias vectors of all N steps are computed here, once per call and outside the captured step, by the forward's own two kernels
    // with the N table times as their "samples" (a row does not depend on the other rows: bit-equal to what the step would compute);
    // the step's advance then copies row step + 1 into tbrun.  EDM Heun evaluates at two times per step and keeps its launches; a 2M
    // step evaluates once, at its table's time, and keeps its rows like EM / PC.
    TimeRows trows{};
    const bool keep_rows = !heun && a.y == nullptr && env_time_rows();
    if (keep_rows) {
        int off4[10];
        const int TB = time_row_layout(off4);
        SBGM_CHECK(TB > 0, "sampler: time-bias widths must be multiples of 4");
        constexpr int CHUNK = 512;                         // rows per launch: bounds the embedding scratch, taken from the idle workspace
        const size_t scratch = (size_t)5 * std::min(N, CHUNK) * D * 4;
        SBGM_CHECK(scratch <= ws_bytes, "sampler: workspace too small for the time-row scratch");
        if (d_times.need((size_t)N * 4, (size_t)4096 * 4) || d_rows.need((size_t)N * TB * 4, (size_t)1024 * TB * 4) ||
            d_tbrun.need((size_t)BE * TB * 4, (size_t)64 * TB * 4)) return 1;
        float* h_times = reinterpret_cast<float*>(h_stage + tab_bytes + sizeof(SamplerState) + sizeof(HoldLevels) * (size_t)N);
        for (int i = 0; i < N; ++i) h_times[i] = dpm2m ? reinterpret_cast<const DpmStep*>(h_stage)[i].t : reinterpret_cast<const StepScalars*>(h_stage)[i].t;
        SBGM_HIP(hipMemcpyAsync(d_times.p, h_times, (size_t)N * 4, hipMemcpyHostToDevice, st));
        for (int r0 = 0; r0 < N; r0 += CHUNK) {
            float* out[9];
            for (int i = 0; i < 9; ++i) out[i] = d_rows.f() + (size_t)r0 * TB + off4[i] * 4;
            if (time_biases(d_times.f() + r0, nullptr, std::min(CHUNK, N - r0), reinterpret_cast<float*>(ws), out, TB, st)) return 1;
        }
        trows.rows = d_rows.f(); trows.tbrun = d_tbrun.f(); trows.n = 9; trows.BE = BE;
        for (int i = 0; i <= 9; ++i) trows.off4[i] = off4[i];
        if (sbgm_launch_time_rows_bcast(trows, 0, st)) return 1;
        run.tbrun = d_tbrun.f();
    }
    SBGM_HIP(hipEventRecord(ev_stage, st));               // no host wait: the copies read pinned memory this handle owns
    stage_pending = true;
    const StepScalars* sde_tab = static_cast<const StepScalars*>(d_table);
    const EdmStep* edm_tab = static_cast<const EdmStep*>(d_table);
    const DpmStep* dpm_tab = static_cast<const DpmStep*>(d_table);

    if (run.begin()) return 1;
    hold.nm = run.nm;
    const JointMap jm = joint ? JointMap{a.tile_origins, B, a.H, a.W, joint->domain_h, a.domain_w, joint->ramp_len} : JointMap{};
    // slabs: x (the network input), score, x_mean, and for EDM Heun the derivative d; EDM Heun keeps its state x / x_hat in x_mean;
    // 2M keeps its state in the network input and its history D_{i-1} in x_mean
    float *xs = run.slab_at(0), *score = run.slab_at(1), *xmean = run.slab_at(2), *dheun = heun ? run.slab_at(3) : nullptr;
    float* t_dev = run.t_vec();
    double* sumsq = run.partials();                          // the Langevin corrector's norm partials

    // x0 = randn * marginal_prob_std(1); EDM Heun: sigma_0 z into its state slab, copied to the network input
    const float ls = logf(sig);
    const float std1 = fmaxf(sqrtf((expf((2.f * 1.0f) * ls) - 1.f) / (2.f * ls)), 1e-5f);
    const float* z = a.noise;
    size_t draw = 0;
    auto next_z = [&]() -> const float* { const float* p = z ? z + draw * n : nullptr; ++draw; return p; };
    const float x0_scale = heun ? reinterpret_cast<const EdmStep*>(h_stage)->sigma : dpm2m ? reinterpret_cast<const DpmStep*>(h_stage)->sigma : std1;
    if (sbgm_launch_init_noise(heun ? xmean : xs, x0_scale, next_z(), a.seed, d_state, 0, n, st, run.nm, hold)) return 1;
    if (heun) SBGM_HIP(hipMemcpyAsync(xs, xmean, n * 4, hipMemcpyDeviceToDevice, st));
    if (sbgm_launch_fill_t(t_dev, tab.t_first, BE, st)) return 1;
    const float snr_nn = (float)((double)a.snr * std::sqrt((double)per));     // snr * sqrt(prod(x.shape[1:])) (:202-203)

    auto evaluate = [&](float w) { return run.evaluate(score, score, w); };
    const bool churn = heun && edm->s_churn > 0.f;
    // One step of the run's kind; z_ptrs: read the caller's noise draws (eager runs).
    //   EM:  eval -> predictor + advance          PC: eval -> Langevin corrector -> eval -> predictor + advance
    //   EDM: (churn) -> eval -> euler -> eval -> heun + advance; `last` (sigma_N = 0) is Euler only, into `out`
    //   2M:  eval -> update + advance, all N steps alike (the last row of the table makes x_N = D_{N-1})
    auto step = [&](bool z_ptrs, bool last) -> int {
        if (dpm2m) {
            if (evaluate(a.cfg_scale)) return 1;
            return sbgm_launch_dpmpp_2m(xs, nullptr, score, xmean, z_ptrs && dpm_sde ? next_z() : nullptr, dpm_tab, d_state, nullptr, 0, a.seed,
                                        dpm_sde, t_dev, BE, N, n, st, run.nm, hold, jm, trows);
        }
        if (heun) {
            if (churn && sbgm_launch_edm_churn(xmean, xs, z_ptrs ? next_z() : nullptr, edm_tab, d_state, nullptr, 0, a.seed, n, st, run.nm))
                return 1;
            if (evaluate(a.cfg_scale)) return 1;
            if (sbgm_launch_edm_euler(xmean, score, dheun, last ? a.out : xs, edm_tab, d_state, nullptr, t_dev, BE, n, st, hold, jm)) return 1;
            if (last) return 0;
            if (evaluate(a.cfg_scale)) return 1;
            return sbgm_launch_edm_heun(xmean, xs, dheun, score, edm_tab, d_state, nullptr, t_dev, BE, N, n, st, hold, jm);
        }
        if (a.kind == SBGM_SAMPLER_PC) {
            if (evaluate(a.cfg_scale_corrector)) return 1;
            if (sbgm_launch_langevin(xs, score, z_ptrs ? next_z() : nullptr, snr_nn, sumsq, d_state, 0, a.seed, B, per, st, run.nm, hold, jm)) return 1;
        }
        if (evaluate(a.cfg_scale)) return 1;
        return sbgm_launch_em_update(xs, xmean, score, z_ptrs ? next_z() : nullptr, sde_tab, d_state, nullptr, 0, t_dev, a.seed, B,
                                     per, N, st, BE, run.nm, hold, jm, trows);
    };
    // The run: N - tail steps (replays of the captured step, or eager launches), then `tail` eager last steps.  EM / PC: no tail,
    // the result is the x_mean slab, copied to `out`; EDM Heun: the tail is its Euler-only last step, which writes `out` itself; 2M: no
    // tail, the result is its state, the network-input slab.
    const int tail = heun ? 1 : 0;
    int rc = 0;
    if (run.graphed) {
        StepGraphKey key{};
        key.churn = churn || dpm_sde; key.domain_w = a.domain_w; key.origins = a.tile_origins; key.table = d_table;
        key.cfg_corr = heun || dpm2m ? 0.f : a.cfg_scale_corrector; key.snr_nn = heun || dpm2m ? 0.f : snr_nn;
        key.known = hold.known; key.known_mask = hold.mask; key.levels = hold.levels;
        if (joint) { key.joint = 1; key.domain_h = joint->domain_h; key.ramp_len = joint->ramp_len; }
        key.rows = trows.rows; key.tbrun = trows.tbrun;
        rc = run.capture(key, [&] { return step(false, false); });
        for (int i = 0; i < N - tail && rc == 0; ++i)
            if (hipGraphLaunch(step_exec, st) != hipSuccess) { sbgm_set_error("hipGraphLaunch failed at step %d", i); rc = 2; }
    } else {
        for (int i = 0; i < N - tail && rc == 0; ++i) rc = step(z != nullptr, false);
    }
    if (tail && rc == 0) rc = step(z != nullptr, true);
    if ((rc = run.replay_done(rc))) return rc;
    if (!tail) SBGM_HIP(hipMemcpyAsync(a.out, dpm2m ? xs : xmean, n * 4, hipMemcpyDeviceToDevice, st));
    return 0;
}

// rk45_sampler: the adaptive probability-flow ODE solver (ode.hip).  The fourth kind shares the run context above (workspace rule,
// condition handling, cached step graph); what differs is the loop: its length is decided on the device.  One ATTEMPT is
// captured (six stage kernels with their evaluations, the norm, the controller, a 4-byte copy of the done word to pinned memory, the
// commit): a linear chain that depends on nothing that changes between attempts or runs, because t, h, tolerances, flags and counters
// live in the device state block.  The host replays it on the caller's stream and stays at most one attempt ahead of the done word it
// waits for, so the device does not idle on the poll; an attempt that runs after done finds every controller frozen and changes
// nothing.  It sets no route (set_routes).
int sbgm_model::sampler_ode(const sbgm_sampler_args& a, hipStream_t caller, const OdeArgs& o) {
    SBGM_CHECK(a.kind == SBGM_SAMPLER_RK45, "sampler_ode: kind %d is not SBGM_SAMPLER_RK45", a.kind);
    SBGM_CHECK(a.out != nullptr && o.stats_i != nullptr, "sampler_ode: out and stats_i are required");
    SBGM_CHECK(!a.bn_train, "sampler_ode: serves eval-mode BatchNorm only (bn_train must be 0)");
    SBGM_CHECK(o.rtol > 0 && o.atol >= 0 && o.max_steps >= 1, "sampler_ode: need rtol > 0, atol >= 0, max_steps >= 1");
    SBGM_CHECK(o.t0 != o.t1 && std::min(o.t0, o.t1) >= 0.0 && std::max(o.t0, o.t1) <= 1.0, "sampler_ode: t_span (%g, %g) must be two "
               "different times in [0, 1]", o.t0, o.t1);
    SBGM_CHECK(!(a.tile_origins && !o.per_sample), "sampler_ode: tiles need one controller per sample (a shared step would couple them)");
    SamplerRun run{this, a, caller, "sampler_ode", a.use_graph != 0};
    if (run.open()) return 1;
    const int B = a.B, G = o.per_sample ? B : 1;
    const size_t per = run.per, n = run.n;
    hipStream_t& st = run.st;
    if (!h_done) {
        SBGM_HIP(hipHostMalloc(reinterpret_cast<void**>(&h_done), 64, hipHostMallocDefault));
        for (hipEvent_t& e : ev_poll) SBGM_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }

    if (run.begin(o.x0 == nullptr)) return 1;
    // the 14 slabs: xs | score2 | K[0..6] | y, y | y_new, y_new | state + partials
    float *xs = run.slab_at(0), *score2 = run.slab_at(1), *K = run.slab_at(2), *t_dev = run.t_vec();
    const size_t ks = run.slab / 4;
    double *y = reinterpret_cast<double*>(run.slab_at(9)), *y_new = reinterpret_cast<double*>(run.slab_at(11));
    char* state = reinterpret_cast<char*>(run.slab_at(13));
    const size_t state_bytes = align_up(sbgm_ode_state_bytes(G), 256);
    double* partials = reinterpret_cast<double*>(state + state_bytes);
    SBGM_CHECK(state_bytes + sbgm_ode_partials_bytes(B, per) <= run.slab, "sampler_ode: %d x %d samples are too small for the solver's state slab", a.H, a.W);

    // start: the caller's state, or marginal_prob_std(t0) * draw 0 of the run's Philox stream (domain-keyed on tiles)
    if (sbgm_launch_ode_init(state, G, o.t0, o.t1, o.rtol, o.atol, cfg.sigma, o.max_steps, st)) return 1;
    if (o.x0) {
        if (sbgm_launch_ode_load(y, o.x0, n, st)) return 1;
    } else {
        const float ls = logf(cfg.sigma), t0f = (float)o.t0;
        const float std0 = fmaxf(sqrtf((expf((2.f * t0f) * ls) - 1.f) / (2.f * ls)), 1e-5f);
        if (sbgm_launch_init_noise(xs, std0, a.noise, a.seed, nullptr, 0, n, st, run.nm)) return 1;
        if (sbgm_launch_ode_load(y, xs, n, st)) return 1;
    }

    auto evaluate = [&](float* dst) { return run.evaluate(dst, score2, a.cfg_scale); };
    auto stage = [&](int phase) -> int {
        return sbgm_launch_ode_stage(state, phase, y, y_new, K, ks, xs, t_dev, run.guided ? 2 : 1, B, per, o.per_sample, st);
    };
    auto control = [&](int what) -> int {
        if (sbgm_launch_ode_control(state, what, y, y_new, K, ks, partials, B, per, o.per_sample, st)) return 1;
        SBGM_HIP(hipMemcpyAsync(h_done, state + offsetof(OdeHeader, done), 4, hipMemcpyDeviceToHost, st));
        return 0;
    };
    auto attempt = [&]() -> int {
        for (int s = 1; s <= 6; ++s)
            if (stage(s) || evaluate(K + (size_t)s * ks)) return 1;
        if (control(2)) return 1;
        return sbgm_launch_ode_commit(state, y, y_new, K, ks, B, per, o.per_sample, st);
    };

    long long enqueued = 0;
    // select_initial_step: f0, the two norms, f1 at t0 + h0, the third norm; then the first attempt is prepared
    int rc = stage(SBGM_ODE_PHASE_F0) || evaluate(K) || control(0) || stage(SBGM_ODE_PHASE_F1) || evaluate(K + ks) || control(1);
    if (rc == 0 && (hipEventRecord(ev_poll[0], st) != hipSuccess || hipEventSynchronize(ev_poll[0]) != hipSuccess)) {
        sbgm_set_error("sampler_ode: waiting for the initial step failed: %s", hipGetErrorString(hipGetLastError()));
        rc = 2;
    }
    volatile int* done = h_done;
    if (rc == 0 && !*done) {
        if (run.graphed) {
            StepGraphKey key{};
            key.ode_norm = o.per_sample;
            rc = run.capture(key, attempt);
        }
        auto launch = [&]() -> int {
            if (run.graphed) {
                if (hipGraphLaunch(step_exec, st) != hipSuccess) { sbgm_set_error("hipGraphLaunch failed at attempt %lld", enqueued); return 2; }
            } else if (attempt()) {
                return 1;
            }
            if (hipEventRecord(ev_poll[enqueued & 1], st) != hipSuccess) { sbgm_set_error("hipEventRecord failed"); return 2; }
            ++enqueued;
            return 0;
        };
        // every controller stops within max_steps attempts, so max_steps + 1 enqueued attempts always reach done
        const long long cap = o.max_steps + 1;
        for (long long k = 0; rc == 0; ++k) {                    // k: the attempt whose done word the host waits for
            while (rc == 0 && enqueued <= k + 1 && enqueued < cap) rc = launch();     // at most one attempt ahead of it
            if (rc) break;
            if (hipEventSynchronize(ev_poll[k & 1]) != hipSuccess) { sbgm_set_error("sampler_ode: waiting for attempt %lld failed", k); rc = 2; }
            if (rc || *done) break;
            if (k + 1 >= cap) { sbgm_set_error("sampler_ode: %lld attempts did not finish the run", cap); rc = 2; }
        }
    }
    if ((rc = run.replay_done(rc))) return rc;
    if (sbgm_launch_ode_store(a.out, y, n, st)) return 1;
    if (sbgm_ode_read_state(state, G, o.stats_i, o.stats_d, st)) return 1;       // synchronises: the run is complete on return
    o.stats_i[4 * G] = enqueued - o.stats_i[4 * G + 1];                            // surplus attempts: enqueued, found nothing to do
    o.stats_i[4 * G + 1] = enqueued;
    return 0;
}

// =====================================================================================================================
// C ABI
// =====================================================================================================================
const char* sbgm_get_error();
extern "C" {

const char* sbgm_last_error(void) { return sbgm_get_error(); }
int sbgm_abi_version(void) { return 13; }
int sbgm_model_config_size(void) { return (int)sizeof(sbgm_model_config); }

int sbgm_model_create(const sbgm_model_config* cfg, sbgm_model** out) {
    SBGM_CHECK(cfg && out, "model_create: null argument");
    SBGM_CHECK(cfg->struct_size == (int)sizeof(sbgm_model_config),
               "model_create: sbgm_model_config.struct_size = %d but this library's struct has %d bytes (ABI version %d): the caller "
               "was built against a different include/sbgm_hip.h", cfg->struct_size, (int)sizeof(sbgm_model_config), sbgm_abi_version());
    std::unique_ptr<sbgm_model> m(new sbgm_model());
    if (m->build(*cfg)) return 1;
    *out = m.release();
    return 0;
}
void sbgm_model_destroy(sbgm_model* m) { delete m; }
int sbgm_model_num_params(const sbgm_model* m) { return (int)m->params.size(); }
const char* sbgm_model_param_name(const sbgm_model* m, int i) {
    return (i >= 0 && i < (int)m->params.size()) ? m->params[i]->name.c_str() : nullptr;
}
int64_t sbgm_model_param_numel(const sbgm_model* m, int i) {
    return (i >= 0 && i < (int)m->params.size()) ? m->params[i]->numel : -1;
}

int sbgm_model_set_param(sbgm_model* m, const char* name, const void* data, int64_t numel, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    auto it = m->by_name.find(name);
    SBGM_CHECK(it != m->by_name.end(), "set_param: unexpected key '%s'", name);
    Param* p = it->second;
    if (p->kind == P_IGNORE) return 0;
    SBGM_CHECK(numel == p->numel, "set_param: '%s' has %lld elements, expected %lld", name, (long long)numel, (long long)p->numel);
    const float* src = static_cast<const float*>(data);
    if (p->kind == P_VEC) {
        SBGM_HIP(hipMemcpyAsync(p->dev(), src, (size_t)numel * 4, hipMemcpyDeviceToDevice, st));
    } else if (p->kind == P_CONV) {
        if (sbgm_pack_conv_images(src, p->img, p->cout, p->cin, p->kh, p->kw, p->cs, st)) return 1;
    } else if (p->kind == P_TCONV) {             // [Cin][Cout][2][2] -> OIHW [4*Cout][Cin][1][1] (scratch) -> packed
        float* tmp = nullptr;
        SBGM_HIP(hipMalloc(&tmp, (size_t)numel * 4));
        int rc = sbgm_launch_tconv_weight(src, tmp, p->cin, p->cout / 4, st);
        if (!rc) rc = sbgm_launch_pack_conv_weight(tmp, p->dev(), p->cout, p->cin, 1, 1, p->cs, st);
        (void)hipStreamSynchronize(st);
        (void)hipFree(tmp);
        if (rc) return rc;
    } else if (p->kind == P_VEC4) {
        for (int r = 0; r < 4; ++r)
            SBGM_HIP(hipMemcpyAsync(p->dev() + (size_t)r * numel, src, (size_t)numel * 4, hipMemcpyDeviceToDevice, st));
    } else {
        if (sbgm_launch_pack_cout1_weight(src, p->dev(), p->cin, st)) return 1;
    }
    if (p->feeds && p->feeds->source_uploaded(p, src, st)) return 1;
    p->filled = true;
    m->bn_dirty = true;
    return 0;
}

int sbgm_model_get_param(sbgm_model* m, const char* name, float* dst, int64_t numel, void* stream) {
    auto it = m->by_name.find(name);
    SBGM_CHECK(it != m->by_name.end(), "get_param: unknown key '%s'", name);
    Param* p = it->second;
    SBGM_CHECK(p->kind == P_VEC && numel == p->numel, "get_param: '%s' is not a plain vector of %lld elements", name, (long long)numel);
    SBGM_HIP(hipMemcpyAsync(dst, p->dev(), (size_t)numel * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

int64_t sbgm_model_workspace_bytes(const sbgm_model* m) { return (int64_t)m->ws_bytes; }

int sbgm_model_check_complete(const sbgm_model* m) {
    for (auto& p : m->params) SBGM_CHECK(p->filled, "model: state_dict entry '%s' was never uploaded", p->name.c_str());
    return 0;
}

int sbgm_model_forward(sbgm_model* m, const float* x, const float* t, const int64_t* y, const float* cond_img,
                       const float* lsm_cond, const float* topo_cond, float* out, float* const* fmaps, int B, int H, int W,
                       int bn_train, void* stream) {
    if (m->ensure_ws(m->ws_need(B, H, W, bn_train))) return 1;
    return m->forward(x, t, y, cond_img, lsm_cond, topo_cond, out, fmaps, B, H, W, bn_train, (hipStream_t)stream);
}

int sbgm_sampler_run(sbgm_model* m, const sbgm_sampler_args* a, void* stream) {
    SBGM_CHECK(a, "sampler_run: null args");
    return m->sampler(*a, (hipStream_t)stream);
}

static int edm_args_check(const sbgm_sampler_args* a, float rho, float s_churn, float s_noise, float sigma_min, float sigma_max) {
    SBGM_CHECK(a->kind == SBGM_SAMPLER_EDM_HEUN, "sampler_run_edm: kind %d is not SBGM_SAMPLER_EDM_HEUN", a->kind);
    SBGM_CHECK(!a->bn_train, "sampler_run_edm: serves eval-mode BatchNorm only (bn_train must be 0)");
    SBGM_CHECK(rho > 0.f && s_churn >= 0.f && s_noise >= 0.f, "sampler_run_edm: need rho > 0, s_churn >= 0, s_noise >= 0");
    SBGM_CHECK(!(sigma_min > 0.f && sigma_max > 0.f && sigma_min >= sigma_max), "sampler_run_edm: sigma_min %g >= sigma_max %g",
               sigma_min, sigma_max);
    return 0;
}

int sbgm_sampler_run_edm(sbgm_model* m, const sbgm_sampler_args* a, float sigma_min, float sigma_max, float rho, float s_churn,
                         float s_tmin, float s_tmax, float s_noise, void* stream) {
    SBGM_CHECK(a, "sampler_run_edm: null args");
    if (edm_args_check(a, rho, s_churn, s_noise, sigma_min, sigma_max)) return 1;
    const sbgm_model::EdmArgs e{sigma_min, sigma_max, rho, s_churn, s_tmin, s_tmax, s_noise};
    return m->sampler(*a, (hipStream_t)stream, &e);
}

// The two drivers above with a constraint (constrained sampling): the same sbgm_model::sampler, the held kernels.
int sbgm_sampler_run_held(sbgm_model* m, const sbgm_sampler_args* a, const float* known, const float* known_mask, void* stream) {
    SBGM_CHECK(a, "sampler_run_held: null args");
    SBGM_CHECK(known && known_mask, "sampler_run_held: known and known_mask are required");
    const sbgm_model::HeldArgs h{known, known_mask};
    return m->sampler(*a, (hipStream_t)stream, nullptr, &h);
}

int sbgm_sampler_run_edm_held(sbgm_model* m, const sbgm_sampler_args* a, float sigma_min, float sigma_max, float rho, float s_churn,
                              float s_tmin, float s_tmax, float s_noise, const float* known, const float* known_mask, void* stream) {
    SBGM_CHECK(a, "sampler_run_edm_held: null args");
    SBGM_CHECK(known && known_mask, "sampler_run_edm_held: known and known_mask are required");
    if (edm_args_check(a, rho, s_churn, s_noise, sigma_min, sigma_max)) return 1;
    const sbgm_model::EdmArgs e{sigma_min, sigma_max, rho, s_churn, s_tmin, s_tmax, s_noise};
    const sbgm_model::HeldArgs h{known, known_mask};
    return m->sampler(*a, (hipStream_t)stream, &e, &h);
}

// The drivers above as ONE diffusion over the domain (joint tiled sampling): the same sbgm_model::sampler, the joint kernels;
// known / known_mask may both be NULL.
int sbgm_sampler_run_joint(sbgm_model* m, const sbgm_sampler_args* a, int domain_h, int ramp_len, const float* known,
                           const float* known_mask, void* stream) {
    SBGM_CHECK(a, "sampler_run_joint: null args");
    SBGM_CHECK((known == nullptr) == (known_mask == nullptr), "sampler_run_joint: known and known_mask must be given together");
    const sbgm_model::HeldArgs h{known, known_mask};
    const sbgm_model::JointArgs j{domain_h, ramp_len};
    return m->sampler(*a, (hipStream_t)stream, nullptr, known ? &h : nullptr, &j);
}

int sbgm_sampler_run_edm_joint(sbgm_model* m, const sbgm_sampler_args* a, float sigma_min, float sigma_max, float rho, float s_churn,
                               float s_tmin, float s_tmax, float s_noise, int domain_h, int ramp_len, const float* known,
                               const float* known_mask, void* stream) {
    SBGM_CHECK(a, "sampler_run_edm_joint: null args");
    SBGM_CHECK((known == nullptr) == (known_mask == nullptr), "sampler_run_edm_joint: known and known_mask must be given together");
    if (edm_args_check(a, rho, s_churn, s_noise, sigma_min, sigma_max)) return 1;
    const sbgm_model::EdmArgs e{sigma_min, sigma_max, rho, s_churn, s_tmin, s_tmax, s_noise};
    const sbgm_model::HeldArgs h{known, known_mask};
    const sbgm_model::JointArgs j{domain_h, ramp_len};
    return m->sampler(*a, (hipStream_t)stream, &e, known ? &h : nullptr, &j);
}

// DPM-Solver++(2M) / 2M SDE with its optional parts as arguments: the same sbgm_model::sampler, the dpmpp_2m kernels.
int sbgm_sampler_run_dpmpp(sbgm_model* m, const sbgm_sampler_args* a, float sigma_min, float sigma_max, float rho, float eta, float s_noise,
                           const float* known, const float* known_mask, int domain_h, int ramp_len, void* stream) {
    SBGM_CHECK(a, "sampler_run_dpmpp: null args");
    SBGM_CHECK(a->kind == SBGM_SAMPLER_DPMPP_2M, "sampler_run_dpmpp: kind %d is not SBGM_SAMPLER_DPMPP_2M", a->kind);
    SBGM_CHECK(!a->bn_train, "sampler_run_dpmpp: serves eval-mode BatchNorm only (bn_train must be 0)");
    SBGM_CHECK(rho > 0.f && eta >= 0.f && s_noise >= 0.f, "sampler_run_dpmpp: need rho > 0, eta >= 0, s_noise >= 0");
    SBGM_CHECK(!(sigma_min > 0.f && sigma_max > 0.f && sigma_min >= sigma_max), "sampler_run_dpmpp: sigma_min %g >= sigma_max %g",
               sigma_min, sigma_max);
    SBGM_CHECK((known == nullptr) == (known_mask == nullptr), "sampler_run_dpmpp: known and known_mask must be given together");
    const sbgm_model::DpmArgs d{sigma_min, sigma_max, rho, eta, s_noise};
    const sbgm_model::HeldArgs h{known, known_mask};
    const sbgm_model::JointArgs j{domain_h, ramp_len};
    return m->sampler(*a, (hipStream_t)stream, nullptr, known ? &h : nullptr, domain_h || ramp_len ? &j : nullptr, &d);
}

int sbgm_sampler_run_ode(sbgm_model* m, const sbgm_sampler_args* a, double t0, double t1, double rtol, double atol, int per_sample,
                         int64_t max_steps, const float* x0, int64_t* stats_i, double* stats_d, void* stream) {
    SBGM_CHECK(a, "sampler_run_ode: null args");
    const sbgm_model::OdeArgs o{t0, t1, rtol, atol, per_sample != 0, (long long)max_steps, x0, stats_i, stats_d};
    return m->sampler_ode(*a, (hipStream_t)stream, o);
}

// One evaluation of the (B, H, W) plan on zero inputs placed at the top of the workspace.  tune = true: every convolution times its tile
// candidates; tune = false: a plain evaluation whose only purpose is the bump allocator's high-water mark (ws_peak).
int sbgm_model::dummy_forward(int B, int H, int W, bool tune, hipStream_t st) {
    const size_t px = (size_t)B * H * W;
    const size_t in_floats = px * 16 + 1024;
    float* inp = reinterpret_cast<float*>(ws + ws_bytes - align_up(in_floats * 4, 256));
    SBGM_HIP(hipMemsetAsync(inp, 0, in_floats * 4, st));
    float* x = inp; float* t = inp + px; float* cond = t + 1024; float* lsm = cond + px * 8; float* topo = lsm + px * 2;
    float* out = topo + px * 2;
    if (sbgm_launch_fill_t(t, 0.5f, B, st)) return 1;
    const size_t saved = ws_bytes;
    ws_bytes -= align_up(in_floats * 4, 256);
    tuning = tune; set_routes(tune ? CALL_MEASURE : CALL_PLAIN);
    ws_used = 0;
    const int rc = forward(x, t, nullptr, cfg.n_cond_channels ? cond : nullptr, cfg.n_lsm_channels ? lsm : nullptr,
                           cfg.n_topo_channels ? topo : nullptr, out, nullptr, B, H, W, 0, st);
    tuning = false; set_routes(CALL_PLAIN);
    ws_bytes = saved;
    SBGM_HIP(hipStreamSynchronize(st));
    return rc;
}

// Workspace for an eval-mode call of this shape.  A shape seen for the first time is measured by one extra evaluation on zero inputs
// BEFORE the caller's work, so the slab has its final size (and address) from the first real call on: a sampler's captured step graph
// is then captured once, not again after a later call has trimmed the slab.  Train-mode BatchNorm shapes are not pre-measured (an
// evaluation would move the running statistics): they run on the generous bound first and are trimmed by a later call.
int sbgm_model::prepare_ws(int B, int H, int W, int bn_train, hipStream_t st, int slabs, size_t run_extra) {
    if (!bn_train && ws_peak.find(std::array<int, 4>{B, H, W, 0}) == ws_peak.end() && sbgm_model_check_complete(this) == 0) {
        if (ensure_ws(ws_need(B, H, W, 0, slabs) + run_extra + ((size_t)B * H * W * 16 + 1024) * 4 + 4096)) return 1;
        if (refresh_derived(st)) return 1;
        if (dummy_forward(B, H, W, false, st)) return 1;
    }
    return ensure_ws(ws_need(B, H, W, bn_train, slabs) + run_extra);     // run_extra: what a step sampler keeps beyond sampler_keep
}

int sbgm_model_autotune(sbgm_model* m, int B, int H, int W, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (m->ensure_ws(2 * m->ws_need(B, H, W))) return 1;
    if (m->refresh_derived(st, true, H, W, true, B)) return 1;
    if (m->dummy_forward(B, H, W, true, st)) return 1;
    // the tuned plan's high-water mark, then the slab at its final size: what runs next (a sampler capturing its step) finds both settled
    if (m->dummy_forward(B, H, W, false, st)) return 1;
    return m->ensure_ws(m->ws_need(B, H, W));
}

// Tile table <-> text file (conv_plan.hip: one line per tuned convolution)
int sbgm_model_tune_save(sbgm_model* m, const char* path) { return sbgm_tile_table_save(m->tuned, path); }

int sbgm_model_tune_load(sbgm_model* m, const char* path) {
    if (sbgm_tile_table_load(&m->tuned, path)) return 1;
    ++m->plan_gen;
    return 0;
}

// Eager forward with every convolution launch bracketed by HIP events on `stream`.  Fills the summary and, when
// csv_path is non-null, writes one line per convolution (geometry, tile, split-K, ms, TFLOP/s).
int sbgm_model_profile_forward(sbgm_model* m, const float* x, const float* t, const int64_t* y, const float* cond_img,
                               const float* lsm_cond, const float* topo_cond, float* out, int B, int H, int W,
                               sbgm_profile* summary, const char* csv_path, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (m->ensure_ws(m->ws_need(B, H, W))) return 1;
    std::vector<sbgm_model::ConvRec> recs;
    hipEvent_t t0, t1;
    SBGM_HIP(hipEventCreate(&t0));
    SBGM_HIP(hipEventCreate(&t1));
    m->prof = &recs;
    SBGM_HIP(hipEventRecord(t0, st));
    m->set_routes(CALL_MEASURE);
    const int rc = m->forward(x, t, y, cond_img, lsm_cond, topo_cond, out, nullptr, B, H, W, 0, st);
    m->set_routes(CALL_PLAIN);
    SBGM_HIP(hipEventRecord(t1, st));
    m->prof = nullptr;
    if (rc) return rc;
    SBGM_HIP(hipEventSynchronize(t1));
    sbgm_profile s{};
    SBGM_HIP(hipEventElapsedTime(&s.ms_total_with_events, t0, t1));
    FILE* f = csv_path ? fopen(csv_path, "w") : nullptr;
    if (f) fprintf(f, "idx,kh,kw,stride,B,H,W,Cin_pad,Cout,M,ksteps,tile_co,tile_px,splits,ws,gflop,ms,tflops,kernel\n");
    int i = 0;
    for (auto& r : recs) {
        SBGM_HIP(hipEventElapsedTime(&r.ms, r.e0, r.e1));
        r.ms /= sbgm_model::PROF_REPS;
        (void)hipEventDestroy(r.e0);
        (void)hipEventDestroy(r.e1);
        s.ms_conv += r.ms;
        s.flops_conv += r.flops;
        s.n_conv += 1;
        if (r.ms > s.ms_conv_max) { s.ms_conv_max = r.ms; s.flops_conv_max = r.flops; }
        if (f) fprintf(f, "%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%.4f,%.4f,%.2f,%s\n", i, r.g.kh, r.g.kw, r.g.stride, r.B, r.H, r.W,
                       r.Cs, r.Cout, r.M, r.nsteps, 16 * r.t.fco, sbgm_tile_csv_px(r.t), r.t.splits, sbgm_tile_csv_ws(r.t), r.flops * 1e-9, r.ms,
                       r.flops / (r.ms * 1e-3) * 1e-12, sbgm_tile_kernel_name(r.g, r.t, r.Cs, r.c_real, r.in_mode, r.proj != 0).c_str());
        ++i;
    }
    if (f) fclose(f);
    (void)hipEventDestroy(t0);
    (void)hipEventDestroy(t1);
    if (summary) *summary = s;
    return 0;
}

// ---- the composed final block on its own (conv_final.hip; the engine's route in forward_impl, without a network) -------------------
int sbgm_final_compose_pack(const float* w1_oihw, const float* b1, const float* w2_oihw, float* wc_oihw, float* bc, int C, void* stream) {
    return sbgm_launch_final_compose(w1_oihw, b1, w2_oihw, wc_oihw, bc, C, (hipStream_t)stream);
}

extern "C++" {
// the block's convolution: bilinear x2 on load where the decoder fuses it (width >= 32), else a plain one on an upsampled copy
static bool final_block_fused(int W) { return W >= 32; }
static ConvParams final_block_conv(int B, int H, int W, int C) {
    ConvParams p{};
    p.B = B; p.H = H; p.W = W; p.Cs = C; p.Cout = 16;
    p.in_mode = final_block_fused(W) ? 2 : 0;
    return p;
}
}  // extern "C++"

int sbgm_final_block_tiles(int B, int H, int W, int C, int* tiles, int cap) {
    static const float present = 0.f;                 // the candidate list only asks which weight images exist
    const ConvImages im{{&present, &present, &present, nullptr}};
    const std::vector<ConvTile> c = sbgm_conv_candidates(ConvGeom{3, 3, 1, 1}, final_block_conv(B, H, W, C), im, false);
    for (int i = 0; i < (int)c.size() && i < cap; ++i) c[i].to_ints(tiles + 6 * i);
    return (int)c.size();
}

int sbgm_final_block_fwd(const float* x, const float* in_affine, const float* in_skip, int in_act, const float* w_packed,
                         const float* w_wino, const float* w_wino2d, const float* bc, const float* b2, const float* t, float sigma,
                         float* out, float* ws, int64_t ws_floats, int B, int H, int W, int C, const int* tile, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SBGM_CHECK(x && w_packed && w_wino && bc && b2 && out && ws, "final_block_fwd: null tensor");
    SBGM_CHECK(B >= 1 && H >= 2 && H % 2 == 0 && W >= 16 && W % 16 == 0 && C >= 16 && C % 16 == 0,
               "final_block_fwd: needs an even H, W %% 16 == 0 and C %% 16 == 0 (B=%d H=%d W=%d C=%d)", B, H, W, C);
    const size_t M = (size_t)B * H * W;
    const bool fused = final_block_fused(W);
    SBGM_CHECK(fused || (!in_affine && !in_skip && in_act == SBGM_ACT_NONE), "final_block_fwd: affine / skip / activation on load need the fused route (W >= 32)");
    SBGM_CHECK((size_t)ws_floats >= M * (fused ? 16 : 16 + (size_t)C), "final_block_fwd: workspace of %lld floats is too small", (long long)ws_floats);
    ConvParams p = final_block_conv(B, H, W, C);
    const ConvImages im{{w_packed, w_wino, w_wino2d, nullptr}};
    p.bias = bc; p.out = ws;
    if (fused) {
        p.x = x; p.in_affine = in_affine; p.in_skip = in_skip; p.in_act = in_act;
    } else {
        float* up = ws + M * 16;
        if (sbgm_launch_upsample2x(x, up, B, H / 2, W / 2, C, st)) return 1;
        p.x = up;
    }
    const ConvTile ct = tile ? ConvTile::from_ints(tile) : sbgm_cout16_tile(p, im);
    const ConvFamily fam = ct.well_formed() ? ct.family() : FAM_IGEMM;
    int v[6];
    ct.to_ints(v);
    SBGM_CHECK(ct.fco == 1 && ct.splits == 1 && (fam == FAM_LDS_WINO || ((fam == FAM_W2D || fam == FAM_W2DP) && w_wino2d)),
               "final_block_fwd: tile {%d,%d,%d,%d,%d,%d} is no 16-channel LDS-staged Winograd kernel", v[0], v[1], v[2], v[3], v[4], v[5]);
    if (sbgm_launch_tile(ConvGeom{3, 3, 1, 1}, p, im, ct, nullptr, st)) return 1;
    return sbgm_launch_tap_gather_rows(ws, b2, t, sigma, out, B, H, W, st);
}

// ---- the same block mixed at low resolution (conv_final.hip, second half; the engine's fin_lowres route) ----------------------------
int64_t sbgm_final_lowres_packed_numel(int C) { return C >= 16 && C % 16 == 0 ? (int64_t)sbgm_final_lowres_packed_floats(C) : 0; }
int64_t sbgm_final_lowres_ws_numel(int B, int H, int W) {
    return B >= 1 && H >= 2 && W >= 2 ? (int64_t)sbgm_final_lowres_ws_floats(B, H / 2, W / 2) : 0;
}

int sbgm_final_lowres_pack(const float* w1_oihw, const float* b1, const float* w2_oihw, const float* b2, float* wz_out, float* beta_out,
                           float* wz_packed, int C, void* stream) {
    return sbgm_launch_final_lowres_pack(w1_oihw, b1, w2_oihw, b2, wz_out, beta_out, wz_packed, C, (hipStream_t)stream);
}

int sbgm_final_lowres_fwd(const float* x_lowres_nhwc, const float* in_affine, const float* in_skip, int in_act, const float* wz_packed,
                          const float* beta, const float* t, float sigma, float* out, float* ws, int64_t ws_floats, int B, int H, int W,
                          int C, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SBGM_CHECK(x_lowres_nhwc && wz_packed && beta && out && ws, "final_lowres_fwd: null tensor");
    SBGM_CHECK(B >= 1 && H >= 4 && H % 2 == 0 && W >= 4 && W % 2 == 0, "final_lowres_fwd: needs even H, W >= 4 (B=%d H=%d W=%d)", B, H, W);
    SBGM_CHECK(ws_floats >= sbgm_final_lowres_ws_numel(B, H, W), "final_lowres_fwd: workspace of %lld floats is too small", (long long)ws_floats);
    if (sbgm_launch_final_mix(x_lowres_nhwc, in_affine, in_skip, in_act, wz_packed, ws, B, H / 2, W / 2, C, st)) return 1;
    return sbgm_launch_final_gather(ws, beta, t, sigma, out, B, H / 2, W / 2, st);
}

// ---- the same with the decoder's last skip formed inside the mix (the step samplers' skip_mix route) --------------------------------
int64_t sbgm_skip_mix_packed_numel(void) { return SKIP_MIX_PACKED_FLOATS; }

int sbgm_skip_mix_pack(const float* w1_oihw, float* w1x, int Cin, void* stream) {
    return sbgm_launch_skip_mix_pack(w1_oihw, w1x, Cin, (hipStream_t)stream);
}

int sbgm_final_lowres_skip_fwd(const float* raw_lowres_nhwc, const float* in_affine, int in_act, const float* wz_packed, const float* beta,
                               const float* x_planar, const float* sc_nhwc, const float* tb0, const float* w1x, const float* t, float sigma,
                               float* out, float* ws, int64_t ws_floats, int B, int H, int W, int C, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SBGM_CHECK(raw_lowres_nhwc && wz_packed && beta && out && ws, "final_lowres_skip_fwd: null tensor");
    SBGM_CHECK(B >= 1 && H >= 4 && H % 2 == 0 && W >= 4 && W % 2 == 0, "final_lowres_skip_fwd: needs even H, W >= 4 (B=%d H=%d W=%d)", B, H, W);
    SBGM_CHECK(ws_floats >= sbgm_final_lowres_ws_numel(B, H, W), "final_lowres_skip_fwd: workspace of %lld floats is too small", (long long)ws_floats);
    if (sbgm_launch_final_mix_skipx(raw_lowres_nhwc, in_affine, in_act, wz_packed, x_planar, sc_nhwc, tb0, w1x, ws, B, H / 2, W / 2, C, st))
        return 1;
    return sbgm_launch_final_gather(ws, beta, t, sigma, out, B, H / 2, W / 2, st);
}

// ---- a small-map decoder block's conv_up at low resolution (conv_uplow.hip; the engine's up_lowres route) ----------------------------
int64_t sbgm_up_lowres_weight_numel(int C) { return C >= 16 && C % 16 == 0 ? (int64_t)sbgm_up_lowres_weight_floats(C) : 0; }
// Z, then the chunk partials of the GroupNorm fallback ([B][64][G][2] doubles)
int64_t sbgm_up_lowres_ws_numel(int B, int H, int W, int C, int groups) {
    if (B < 1 || H < 2 || W < 2 || C < 16) return 0;
    return (int64_t)sbgm_up_lowres_ws_floats(B, H / 2, W / 2, C) + (int64_t)B * 64 * std::max(groups, 0) * 4;
}

int sbgm_up_lowres_pack(const float* w_oihw, float* w_taps, float* w_packed, int C, void* stream) {
    return sbgm_launch_up_lowres_pack(w_oihw, w_taps, w_packed, C, (hipStream_t)stream);
}

int sbgm_up_lowres_fwd(const float* x_lowres_nhwc, const float* w_packed, const float* bias, const float* gamma, const float* beta,
                       int groups, float eps, float* out, float* ws, int64_t ws_floats, int B, int H, int W, int C, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SBGM_CHECK(x_lowres_nhwc && w_packed && bias && out && ws, "up_lowres_fwd: null tensor");
    SBGM_CHECK(B >= 1 && H >= 2 && H % 2 == 0 && W >= 2 && W % 2 == 0 && C >= 16 && C % 16 == 0 && groups >= 0,
               "up_lowres_fwd: needs even H, W >= 2 and C %% 16 == 0 (B=%d H=%d W=%d C=%d)", B, H, W, C);
    SBGM_CHECK(ws_floats >= sbgm_up_lowres_ws_numel(B, H, W, C, groups), "up_lowres_fwd: workspace of %lld floats is too small", (long long)ws_floats);
    const int h = H / 2, w = W / 2;
    const ConvGeom lin{1, 1, 1, 0};
    ConvParams p{};
    p.x = x_lowres_nhwc; p.out = ws; p.B = B; p.H = h; p.W = w; p.Cs = C; p.Cout = 9 * C;
    const ConvImages im{{w_packed, nullptr, nullptr, nullptr}};
    ConvTile ct = sbgm_static_tile(lin, p, im);
    ct.splits = 1;                                   // no split-K scratch here
    if (sbgm_launch_tile(lin, p, im, ct, nullptr, st)) return 1;
    double* stats = reinterpret_cast<double*>(ws + sbgm_up_lowres_ws_floats(B, h, w, C));
    int chunks = 0, normed = 0;
    if (sbgm_launch_up_gather(ws, bias, out, gamma, beta, groups > 0 ? stats : nullptr, groups, eps, B, h, w, C, &chunks, &normed, st)) return 1;
    if (groups == 0 || normed) return 0;
    if (chunks == 0 && sbgm_launch_gn_partial(out, stats, B, H * W, C, groups, &chunks, st)) return 1;
    return sbgm_launch_groupnorm_apply(out, out, gamma, beta, nullptr, nullptr, SBGM_ACT_NONE, B, H * W, C, groups, eps, stats, chunks, st);
}

// ---- a LayerNorm folded into the linear after it (conv_igemm.hip, in_mode 3; the engine's ln_fold route, without a network) ----------
extern "C++" {
static ConvParams ln_linear_conv(int M, int C, int Cout, float eps) {
    ConvParams p{};
    p.B = 1; p.H = 1; p.W = M; p.Cs = C; p.Cout = Cout;
    p.in_mode = 3; p.ln_eps = eps;
    return p;
}
}  // extern "C++"

int sbgm_ln_fold_pack(const float* w, const float* b, const float* gamma, const float* beta, int C, int Cout, float* w2_oihw, float* w2_packed,
                      float* h, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SBGM_CHECK(w2_packed, "ln_fold_pack: null tensor");
    if (sbgm_launch_ln_fold(w, b, gamma, beta, w2_oihw, h, C, Cout, st)) return 1;
    return sbgm_launch_pack_conv_weight(w2_oihw, w2_packed, Cout, C, 1, 1, C, st);
}

int sbgm_ln_linear_tiles(int M, int C, int Cout, int* tiles, int cap) {
    if (M < 1 || C < 16 || C % 16 || Cout < 16 || Cout % 16 || !tiles) return 0;
    static const float present = 0.f;
    const ConvImages im{{&present, nullptr, nullptr, nullptr}};
    const std::vector<ConvTile> c = sbgm_conv_candidates(ConvGeom{1, 1, 1, 0}, ln_linear_conv(M, C, Cout, LN_EPS), im, false);
    for (int i = 0; i < (int)c.size() && i < cap; ++i) c[i].to_ints(tiles + 6 * i);
    return (int)c.size();
}

int sbgm_ln_linear_fwd(const float* x, const float* w2_packed, const float* h, const float* res, int act, float eps, float* out, int M, int C,
                       int Cout, const int* tile, void* stream) {
    SBGM_CHECK(x && w2_packed && h && out, "ln_linear_fwd: null tensor");
    SBGM_CHECK(M >= 1 && C >= 16 && C % 16 == 0 && Cout >= 16 && Cout % 16 == 0 && eps > 0.f,
               "ln_linear_fwd: needs C %% 16 == 0, Cout %% 16 == 0 and eps > 0 (M=%d C=%d Cout=%d)", M, C, Cout);
    SBGM_CHECK(act == SBGM_NONE || act == SBGM_RELU || act == SBGM_GELU, "ln_linear_fwd: act must be none, relu or gelu");
    const ConvGeom lin{1, 1, 1, 0};
    ConvParams p = ln_linear_conv(M, C, Cout, eps);
    p.x = x; p.out = out; p.bias = h; p.res = res; p.act = act;
    const ConvImages im{{w2_packed, nullptr, nullptr, nullptr}};
    const bool given = tile && (tile[0] | tile[1] | tile[2] | tile[3] | tile[4] | tile[5]) != 0;      // all zeros: the static tile
    const ConvTile ct = given ? ConvTile::from_ints(tile) : sbgm_static_tile(lin, p, im);
    return sbgm_launch_tile(lin, p, im, ct, nullptr, (hipStream_t)stream);
}

int sbgm_time_row_layout(const int* channels, int n, int* offsets) {
    if (!channels || !offsets || n < 1 || n > 16) return -1;
    offsets[0] = 0;
    for (int i = 0; i < n; ++i) {
        if (channels[i] < 4 || channels[i] % 4) return -1;
        offsets[i + 1] = offsets[i] + channels[i];
    }
    return offsets[n];
}
int64_t sbgm_time_row_index(int64_t advances, int64_t num_steps) {
    unsigned long long s = 0;
    for (int64_t k = 0; k < advances; ++k) s = sampler_next_step(s, (unsigned long long)num_steps);
    return (int64_t)s;
}

int sbgm_event_create(void** ev) { hipEvent_t e; SBGM_HIP(hipEventCreate(&e)); *ev = e; return 0; }
int sbgm_event_record(void* ev, void* stream) { SBGM_HIP(hipEventRecord((hipEvent_t)ev, (hipStream_t)stream)); return 0; }
int sbgm_event_elapsed_ms(void* start, void* stop, float* ms) {
    SBGM_HIP(hipEventSynchronize((hipEvent_t)stop));
    SBGM_HIP(hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop));
    return 0;
}
int sbgm_event_destroy(void* ev) { SBGM_HIP(hipEventDestroy((hipEvent_t)ev)); return 0; }

}  // extern "C"
