// Per-op C-ABI entry points declared in include/sbgm_hip.h (the model entry points live in model.hip and forward.hip, the sampler
// entry points in sampler_run.hip).
#include <string.h>
#include <algorithm>
#include <vector>

#include "../../include/sbgm_hip.h"
#include "common.h"
#include "kernels.h"

#define ST ((hipStream_t)stream)

// ---- helpers of the stand-alone operators at the end of this file ------------------------------------------------------------
constexpr float LN_EPS = 1e-5f;      // the attention blocks' LayerNorm (engine.h); sbgm_ln_linear_tiles lists candidates for it
// the block's convolution: bilinear x2 on load where the decoder fuses it (width >= 32), else a plain one on an upsampled copy
static bool final_block_fused(int W) { return W >= 32; }
static ConvParams final_block_conv(int B, int H, int W, int C) {
    ConvParams p{};
    p.B = B; p.H = H; p.W = W; p.Cs = C; p.Cout = 16;
    p.in_mode = final_block_fused(W) ? 2 : 0;
    return p;
}
// a LayerNorm folded into the linear after it, as the convolution it runs as
static ConvParams ln_linear_conv(int M, int C, int Cout, float eps) {
    ConvParams p{};
    p.B = 1; p.H = 1; p.W = M; p.Cs = C; p.Cout = Cout;
    p.in_mode = 3; p.ln_eps = eps;
    return p;
}

const char* sbgm_get_error();

extern "C" {

const char* sbgm_last_error(void) { return sbgm_get_error(); }
int sbgm_abi_version(void) { return 20; }
int sbgm_model_config_size(void) { return (int)sizeof(sbgm_model_config); }

int sbgm_pack_input(const float* const* srcs, const int* src_channels, int n_src, float* dst_nhwc, int B, int H, int W,
                    int c_pad, void* stream) {
    SBGM_CHECK(n_src >= 1 && n_src <= 4, "pack_input: n_src=%d (1..4)", n_src);
    PackSrc s{};
    s.n = n_src;
    for (int i = 0; i < n_src; ++i) { s.ptr[i] = srcs[i]; s.ch[i] = src_channels[i]; }
    return sbgm_launch_pack_input(s, dst_nhwc, B, H, W, c_pad, ST);
}
int sbgm_nchw_to_nhwc(const float* src, float* dst, int B, int H, int W, int C, void* stream) {
    return sbgm_launch_nchw_to_nhwc(src, dst, B, H, W, C, ST);
}
int sbgm_nhwc_to_nchw(const float* src, float* dst, int B, int H, int W, int C, void* stream) {
    return sbgm_launch_nhwc_to_nchw(src, dst, B, H, W, C, ST);
}

int64_t sbgm_conv_packed_numel(int Cout, int KH, int KW, int c_pad) {
    return (int64_t)sbgm_conv_nsteps(KH, KW, c_pad) * Cout * 16;
}
int64_t sbgm_conv_wino_packed_numel(int Cout, int c_pad) { return (int64_t)sbgm_wino_packed_floats(Cout, c_pad); }
int sbgm_conv_wino_pack_weight(const float* w_oihw, float* packed, int Cout, int Cin, int c_pad, void* stream) {
    return sbgm_launch_pack_wino_weight(w_oihw, packed, Cout, Cin, c_pad, ST);
}
int64_t sbgm_conv_wino2d_packed_numel(int Cout, int c_pad) { return (int64_t)sbgm_w2d_packed_floats(Cout, c_pad); }
int sbgm_conv_wino2d_pack_weight(const float* w_oihw, float* packed, int Cout, int Cin, int c_pad, void* stream) {
    return sbgm_launch_pack_w2d_weight(w_oihw, packed, Cout, Cin, c_pad, ST);
}
int64_t sbgm_conv8x8s2_wino_packed_numel(int Cout, int c_pad) { return (int64_t)sbgm_s2w_packed_floats(Cout, c_pad); }
int sbgm_conv8x8s2_wino_pack_weight(const float* w_oihw, float* packed, int Cout, int Cin, int c_pad, void* stream) {
    return sbgm_launch_pack_s2w_weight(w_oihw, packed, Cout, Cin, c_pad, ST);
}
int64_t sbgm_stem22_packed_numel(int Cin) { return (int64_t)sbgm_stem22_packed_floats(Cin); }
int64_t sbgm_stem22_bias_numel(void) { return (int64_t)sbgm_stem22_bias_floats(); }
int sbgm_stem22_pack_weight(const float* w1_oihw, const float* w2_oihw, float* wc, float* s, int Cin, void* stream) {
    SBGM_CHECK(w1_oihw && w2_oihw && wc && s, "stem22_pack_weight: null tensor");
    return sbgm_launch_pack_stem22(w1_oihw, w2_oihw, wc, s, Cin, ST);
}
int sbgm_stem22_fwd(const float* src, int n_channels, int first_channel, int Cin, const float* wc, const float* s, const float* tb0,
                    const float* addend, const float* scale, const float* bias, int relu, float* out, int B, int H, int W, void* stream) {
    return sbgm_launch_conv_stem22(src, n_channels, first_channel, Cin, wc, s, tb0, addend, scale, bias, relu, out, B, H, W, ST);
}
int sbgm_conv_pack_weight(const float* w_oihw, float* packed, int Cout, int Cin, int KH, int KW, int c_pad, void* stream) {
    return sbgm_launch_pack_conv_weight(w_oihw, packed, Cout, Cin, KH, KW, c_pad, ST);
}

int sbgm_conv2d_fwd(const sbgm_conv_args* a, void* stream) {
    ConvGeom g;
    ConvParams p;
    ConvImages w;
    ConvTile t;
    if (sbgm_conv_from_args(a, &g, &p, &w, &t)) return 1;
    return sbgm_launch_tile(g, p, w, t, a->ws, ST);
}

int sbgm_conv2d_pair_fwd(const sbgm_conv_args* main_conv, const sbgm_conv_args* aux_conv, int* paired, void* stream) {
    ConvGeom gm, ga;
    ConvParams pm, pa;
    ConvImages wm, wa;
    ConvTile tm, ta;
    if (sbgm_conv_from_args(main_conv, &gm, &pm, &wm, &tm) || sbgm_conv_from_args(aux_conv, &ga, &pa, &wa, &ta)) return 1;
    SBGM_CHECK(pm.x == pa.x && pm.B == pa.B && pm.H == pa.H && pm.W == pa.W && pm.Cs == pa.Cs, "conv2d_pair: the two convolutions must read one input");
    SBGM_CHECK(main_conv->ws == aux_conv->ws, "conv2d_pair: the two convolutions share one split-K workspace");
    return sbgm_launch_tile_pair(gm, pm, wm, tm, ga, pa, wa, ta, main_conv->ws, ST, paired);
}

int sbgm_conv_pack_weights_batched_blocks(int Cout, int KH, int KW, int c_pad) { return sbgm_conv_pack_blocks(Cout, KH, KW, c_pad); }
int sbgm_conv_pack_weights_batched(const sbgm_pack_desc* desc_dev, int n, int total_blocks, void* stream) {
    return sbgm_launch_pack_conv_weights_batched(desc_dev, n, total_blocks, ST);   // descriptors live on the device: the caller
}                                                                                    // guarantees bit 1 only on 3x3, cs%16, Cout%16
int sbgm_adam_step_blocks(int64_t numel) { return sbgm_adam_blocks(numel); }
int sbgm_adam_step_batched(const sbgm_adam_desc* desc_dev, int n, int total_blocks, const float* step, float lr, float beta1,
                           float beta2, float eps, float weight_decay, int decoupled, float grad_scale, void* stream) {
    return sbgm_launch_adam_batched(desc_dev, n, total_blocks, step, lr, beta1, beta2, eps, weight_decay, decoupled, grad_scale, ST);
}
int sbgm_adam_ema_step_batched(const sbgm_adam_desc* desc_dev, float* const* ema, int n, int total_blocks, const float* step, float lr,
                               float beta1, float beta2, float eps, float weight_decay, int decoupled, float grad_scale, float ema_rate,
                               void* stream) {
    return sbgm_launch_adam_ema_batched(desc_dev, ema, n, total_blocks, step, lr, beta1, beta2, eps, weight_decay, decoupled, grad_scale,
                                        ema_rate, ST);
}
int sbgm_ema_update_batched(const sbgm_adam_desc* desc_dev, float* const* ema, int n, int total_blocks, float ema_rate, void* stream) {
    return sbgm_launch_ema_batched(desc_dev, ema, n, total_blocks, ema_rate, ST);
}
int sbgm_batchnorm_train_stats(const float* x, int B, int HW, int C, void* stats_ws, void* stream) {
    return sbgm_launch_batchnorm_stats(x, B, HW, C, static_cast<double*>(stats_ws), ST);
}
int sbgm_batchnorm_train_apply(const float* x, float* y, const float* gamma, const float* beta, float* running_mean,
                               float* running_var, const float* residual, const float* tbias_after, int relu, int B, int HW, int C,
                               float eps, float momentum, void* stats_ws, double n_total, float* mean_rstd_out, void* stream) {
    return sbgm_launch_batchnorm_apply(x, y, gamma, beta, running_mean, running_var, residual, tbias_after, relu, B, HW, C, eps, momentum,
                                       static_cast<double*>(stats_ws), n_total, ST, mean_rstd_out);
}
int sbgm_batchnorm_bwd_reduce(const float* x, const float* dy, const float* y, const float* tbias_after, const float* mean_rstd,
                              int relu, float* ws, int B, int HW, int C, void* stream) {
    return sbgm_launch_batchnorm_bwd_reduce(x, dy, y, tbias_after, mean_rstd, relu, ws, B, HW, C, ST);
}
int sbgm_batchnorm_bwd_apply(const float* x, const float* dy, const float* y, const float* gamma, const float* tbias_after,
                             const float* mean_rstd, int relu, float* dx, float* dres, float* dgamma, float* dbeta, const float* ws,
                             const float* sync_sums, double n_total, int B, int HW, int C, void* stream) {
    return sbgm_launch_batchnorm_bwd_apply(x, dy, y, gamma, tbias_after, mean_rstd, relu, dx, dres, dgamma, dbeta, ws, sync_sums, n_total,
                                           B, HW, C, ST);
}
int sbgm_conv8x8s2_dgrad_phase_weight(const float* w_oihw, float* out_oihw, int Cout, int Cin, void* stream) {
    return sbgm_launch_dgrad_phase_weight(w_oihw, out_oihw, Cout, Cin, ST);
}
int sbgm_groupnorm_stats(const float* x, void* stats_ws, int B, int HW, int C, int G, int* chunks, void* stream) {
    SBGM_CHECK(chunks != nullptr, "groupnorm_stats: chunks is required");
    return sbgm_launch_gn_partial(x, static_cast<double*>(stats_ws), B, HW, C, G, chunks, ST);
}
int sbgm_groupnorm_finalize(const void* stats_ws, int chunks, const float* gamma, const float* beta, const float* tbias, float* out, int B,
                            int HW, int C, int G, float eps, void* stream) {
    return sbgm_launch_gn_finalize(static_cast<const double*>(stats_ws), chunks, gamma, beta, tbias, out, B, HW, C, G, eps, ST);
}
int sbgm_dsm_loss_blocks(int64_t per_sample) { return sbgm_dsm_nblk(per_sample); }
int sbgm_dsm_perturb(const float* x, const float* z, const float* t, const uint64_t* rng_state, uint64_t seed, float t_eps, float sigma,
                     float* x_perturbed, float* z_out, float* t_out, float* std_out, int B, int64_t per_sample, void* stream) {
    return sbgm_launch_dsm_perturb(x, z, t, reinterpret_cast<const unsigned long long*>(rng_state), (unsigned long long)seed, t_eps, sigma,
                                   x_perturbed, z_out,
                                   t_out, std_out, B, (size_t)per_sample, ST);
}
int sbgm_dsm_loss_fwd(const float* score, const float* z, const float* std, const float* sdf, void* partial_ws, float* loss,
                      uint64_t* rng_state, int B, int64_t per_sample, void* stream) {
    return sbgm_launch_dsm_loss_fwd(score, z, std, sdf, static_cast<double*>(partial_ws), loss,
                                    reinterpret_cast<unsigned long long*>(rng_state), B, (size_t)per_sample, ST);
}
int sbgm_dsm_loss_bwd(const float* score, const float* z, const float* std, const float* sdf, const float* dloss, float* dscore,
                      int B, int64_t per_sample, void* stream) {
    return sbgm_launch_dsm_loss_bwd(score, z, std, sdf, dloss, dscore, B, (size_t)per_sample, ST);
}
int sbgm_set_scratch_prezeroed(int on) {
    const int prev = sbgm_scratch_prezeroed;
    sbgm_scratch_prezeroed = on ? 1 : 0;
    return prev;
}
int sbgm_wgrad_defer(int on) {
    const int prev = sbgm_wgrad_deferred;
    sbgm_wgrad_deferred = on & 3;
    return prev;
}
int sbgm_wgrad_flush(void* stream) { return sbgm_launch_wgrad_flush(ST); }
int sbgm_wgrad_flush_pending(void) { return sbgm_wgrad_pending(); }
int sbgm_wgrad_discard(void) { const int n = sbgm_wgrad_pending(); sbgm_wgrad_discard_queue(); return n; }

// the checks sbgm_conv2d_tune and sbgm_conv2d_tiles share, and the call in the planner's terms; *own: the call's own tile
static int tune_call_from_args(const char* who, const sbgm_conv_args* a, ConvGeom* g, ConvParams* p, ConvImages* w, ConvTile* own) {
    SBGM_CHECK(a->winograd == 0, "%s: winograd must be 0 (the search decides the kernel; w_wino / w_wino2d say which images exist)", who);
    SBGM_CHECK(a->Cout % 32 == 0, "%s: Cout=%d must be a multiple of 32", who, a->Cout);
    return sbgm_conv_from_args(a, g, p, w, own);
}

int sbgm_conv2d_tune(const sbgm_conv_args* a, int* tile, void* stream) {
    SBGM_CHECK(a && tile, "conv2d_tune: null argument");
    ConvGeom g;
    ConvParams p;
    ConvImages w;
    ConvTile best;                      // the call's own tile (the default one when its tile fields are zero) is the fallback
    if (tune_call_from_args("conv2d_tune", a, &g, &p, &w, &best)) return 1;
    if (sbgm_tune_conv(g, p, w, a->ws, a->ws ? (size_t)a->ws_floats : 0, ST, &best)) return 1;
    best.to_ints(tile);
    return 0;
}

int sbgm_conv2d_tiles(const sbgm_conv_args* a, int* tiles, int cap) {
    if (!a || (!tiles && cap > 0) || cap < 0) return 0;
    ConvGeom g;
    ConvParams p;
    ConvImages w;
    ConvTile own;
    if (tune_call_from_args("conv2d_tiles", a, &g, &p, &w, &own)) return 0;
    const std::vector<ConvTile> c = sbgm_conv_tune_list(g, p, w, a->ws != nullptr, a->ws ? (size_t)a->ws_floats : 0);
    for (int i = 0; i < (int)c.size() && i < cap; ++i) c[i].to_ints(tiles + 6 * i);
    return (int)c.size();
}

int sbgm_upsample2x_fwd(const float* x, float* y, int B, int H, int W, int C, void* stream) {
    return sbgm_launch_upsample2x(x, y, B, H, W, C, ST);
}
int sbgm_groupnorm_fwd(const float* x, float* y, const float* gamma, const float* beta, const float* skip, const float* tbias,
                       int act, int B, int HW, int C, int G, float eps, void* stats_ws, float* mean_rstd_out, void* stream) {
    return sbgm_launch_groupnorm(x, y, gamma, beta, skip, tbias, act, B, HW, C, G, eps, (double*)stats_ws, ST, mean_rstd_out);
}
int sbgm_layernorm_fwd(const float* x, float* y, const float* gamma, const float* beta, int M, int C, float eps, void* stream) {
    return sbgm_launch_layernorm(x, y, gamma, beta, M, C, eps, ST);
}
int sbgm_batchnorm_train_fwd(const float* x, float* y, const float* gamma, const float* beta, float* running_mean,
                             float* running_var, const float* residual, const float* tbias_after, int relu, int B, int HW,
                             int C, float eps, float momentum, void* stats_ws, float* mean_rstd_out, void* stream) {
    return sbgm_launch_batchnorm_train(x, y, gamma, beta, running_mean, running_var, residual, tbias_after, relu, B, HW, C, eps,
                                       momentum, (double*)stats_ws, ST, mean_rstd_out);
}
int sbgm_mha_core_fwd(const float* qkv, float* out, int B, int S, int C, int heads, void* stream) {
    return sbgm_launch_mha_core(qkv, out, B, S, C, heads, ST);
}
int sbgm_mha_core_dropout_fwd(const float* qkv, float* out, int B, int S, int C, int heads, float p, uint64_t seed, uint64_t offset, void* stream) {
    return sbgm_launch_mha_core_dropout(qkv, nullptr, out, B, S, C, heads, p, seed, offset, 0, ST);
}
int sbgm_mha_core_dropout_bwd(const float* qkv, const float* dout, float* dqkv, int B, int S, int C, int heads, float p, uint64_t seed,
                              uint64_t offset, void* stream) {
    return sbgm_launch_mha_core_dropout(qkv, dout, dqkv, B, S, C, heads, p, seed, offset, 1, ST);
}
int sbgm_mha_dropout_mask(float* mask, int B, int S, int heads, float p, uint64_t seed, uint64_t offset, void* stream) {
    return sbgm_launch_mha_dropout_mask(mask, B, S, heads, p, seed, offset, ST);
}
int sbgm_attn_qkv_fwd(const float* x, const float* ln_gamma, const float* ln_beta, const float* w_in_packed, const float* b_in,
                      float* qkv, int M, int C, float eps, void* stream) {
    return sbgm_launch_attn_in(x, ln_gamma, ln_beta, w_in_packed, b_in, qkv, M, C, eps, ST);
}
int sbgm_attn_tail_fwd(const float* att, const float* x, const float* w_out_packed, const float* b_out, const float* ln_gamma,
                       const float* ln_beta, const float* w_ff1_packed, const float* b_ff1, const float* w_ff2_packed,
                       const float* b_ff2, float* out, int M, int C, float eps, void* stream) {
    return sbgm_launch_attn_out(att, x, w_out_packed, b_out, ln_gamma, ln_beta, w_ff1_packed, b_ff1, w_ff2_packed, b_ff2, out, M, C, eps, ST);
}
static_assert(SBGM_MHA_FWD_REGISTER == MHA_FWD_REGISTER && SBGM_MHA_FWD_LDS == MHA_FWD_LDS, "family codes of the header");
static_assert(SBGM_MHA_BWD_MFMA == MHA_BWD_MFMA && SBGM_MHA_BWD_LDS16 == MHA_BWD_LDS16 && SBGM_MHA_BWD_LDS32 == MHA_BWD_LDS32 &&
              SBGM_MHA_BWD_SCALAR == MHA_BWD_SCALAR, "family codes of the header");
int sbgm_mha_core_fwd_variant(int B, int S, int C, int heads, int info[4]) {
    MhaFwdPlan p;
    const int id = sbgm_mha_fwd_plan(B, S, C, heads, &p);
    if (info) { info[0] = p.family; info[1] = p.d16; info[2] = p.kn; info[3] = p.qsplit; }
    return id;
}
int sbgm_mha_core_fwd_variant_count(void) { return sbgm_mha_fwd_variant_count(); }
const char* sbgm_mha_core_fwd_variant_name(int id) { return sbgm_mha_fwd_variant_name(id); }
int sbgm_mha_core_bwd_variant(int B, int S, int C, int heads, int info[4]) {
    MhaBwdPlan p;
    const int id = sbgm_mha_bwd_plan(B, S, C, heads, &p);
    if (info) { info[0] = p.family; info[1] = p.d; info[2] = p.G; info[3] = p.grid; }
    return id;
}
int sbgm_mha_core_bwd_variant_count(void) { return sbgm_mha_bwd_variant_count(); }
const char* sbgm_mha_core_bwd_variant_name(int id) { return sbgm_mha_bwd_variant_name(id); }
int sbgm_attn_tokens_variant(int M, int C, int info[2]) {
    AttnTokensPlan p;
    const int id = sbgm_attn_tokens_plan(M, C, &p);
    if (info) { info[0] = p.fco; info[1] = p.tok; }
    return id;
}
int sbgm_attn_tokens_variant_count(void) { return sbgm_attn_tok_variant_count(); }
const char* sbgm_attn_tokens_variant_name(int id) { return sbgm_attn_tok_variant_name(id); }
int sbgm_time_proj_fwd(const float* t, const int64_t* y, const float* label_emb, const float* freqs, const float* weight,
                       const float* bias, float* out, float* emb_ws, float* emb_raw, int B, int D, int ch, void* stream) {
    TimeEmbedArgs a{};
    a.emb_raw = emb_raw;
    a.t = t; a.y = y; a.label_emb = label_emb; a.freqs[0] = freqs; a.n_emb = 1; a.n_proj = 1;
    a.proj[0] = TimeProj{weight, bias, out, ch, 0};
    a.emb_ws = emb_ws; a.B = B; a.D = D;
    return sbgm_launch_time_embed(a, ST);
}
int sbgm_time_proj_multi_fwd(const float* t, const int64_t* y, const float* label_emb, const float* const* freqs, int n_emb,
                             const float* const* weights, const float* const* biases, float* const* outs, const int* chs,
                             const int* emb_index, int n_proj, float* emb_ws, float* emb_raw, int B, int D, void* stream) {
    SBGM_CHECK(t && freqs && weights && biases && outs && chs && emb_index && emb_ws, "time_proj_multi: null argument");
    SBGM_CHECK(n_emb >= 1 && n_emb <= 8 && n_proj >= 1 && n_proj <= 16, "time_proj_multi: n_emb=%d (1..8), n_proj=%d (1..16)", n_emb, n_proj);
    TimeEmbedArgs a{};
    a.t = t; a.y = y; a.label_emb = label_emb; a.n_emb = n_emb; a.n_proj = n_proj;
    for (int i = 0; i < n_emb; ++i) a.freqs[i] = freqs[i];
    for (int i = 0; i < n_proj; ++i) {
        SBGM_CHECK(emb_index[i] >= 0 && emb_index[i] < n_emb, "time_proj_multi: emb_index[%d]=%d", i, emb_index[i]);
        a.proj[i] = TimeProj{weights[i], biases[i], outs[i], chs[i], emb_index[i]};
    }
    a.emb_ws = emb_ws; a.emb_raw = emb_raw; a.B = B; a.D = D;
    return sbgm_launch_time_embed(a, ST);
}
int sbgm_cout1_pack_weight(const float* w_oihw, float* w_tap_c, int C, void* stream) {
    return sbgm_launch_pack_cout1_weight(w_oihw, w_tap_c, C, ST);
}
int sbgm_conv3x3_cout1_fwd(const float* x, const float* w_tap_c, const float* bias, const float* t, float sigma, float* out,
                           int B, int H, int W, int C, void* stream) {
    return sbgm_launch_conv3x3_cout1(x, w_tap_c, bias, t, sigma, out, B, H, W, C, ST);
}
int sbgm_act_inplace(float* x, int64_t n, int act, void* stream) { return sbgm_launch_act(x, (size_t)n, act, ST); }

int sbgm_pointwise_chain(const float* x, float* y, int64_t n, int n_ops, const int* ops, const float* consts, void* stream) {
    SBGM_CHECK(n >= 0 && (n_ops == 0 || (ops && consts)), "pointwise_chain: bad arguments");
    return sbgm_launch_pointwise_chain(x, y, (size_t)n, n_ops, ops, consts, ST);
}
int sbgm_sample_extremes(const float* x, int B, int64_t per_sample, float q, float* out_max, float* out_q, void* stream) {
    SBGM_CHECK(x && out_max && out_q && per_sample > 0, "sample_extremes: bad arguments");
    return sbgm_launch_sample_extremes(x, B, (size_t)per_sample, q, out_max, out_q, ST);
}

// ---- device-resident cutout batches (cutout.hip) ----------------------------------------------------------------------
int sbgm_cutout_draw(uint64_t seed, uint64_t draw, int B, const int* rect, int h, int w, int Hd, int Wd, int* origins, void* stream) {
    return sbgm_launch_cutout_draw((unsigned long long)seed, (unsigned long long)draw, B, rect, h, w, Hd, Wd, origins, ST);
}
int sbgm_cutout_program_init(int32_t* words_host, int n_ops, const int* ops, const float* consts, int is_mask) {
    SBGM_CHECK(words_host && (n_ops == 0 || (ops && consts)), "cutout_program_init: null argument");
    SBGM_CHECK(n_ops >= 0 && n_ops <= SBGM_CHAIN_MAX_OPS, "cutout_program_init: %d ops (max %d)", n_ops, SBGM_CHAIN_MAX_OPS);
    CutoutProgram p{};
    p.n_ops = n_ops;
    p.is_mask = is_mask ? 1 : 0;
    for (int i = 0; i < n_ops; ++i) {
        SBGM_CHECK(ops[i] >= SBGM_OP_ADD && ops[i] <= SBGM_OP_LOG, "cutout_program_init: unknown op code %d", ops[i]);
        p.ops[i] = ops[i];
        p.consts[i] = consts[i];
    }
    memcpy(words_host, &p, sizeof(p));
    return 0;
}
int sbgm_cutout_gather(const float* const* srcs, float* const* dsts, const int* n_items, int n_fields, const int32_t* programs,
                       const int* items, const int* origins, int B, int Hd, int Wd, int h, int w, void* stream) {
    return sbgm_launch_cutout_gather(srcs, dsts, n_items, n_fields, reinterpret_cast<const CutoutProgram*>(programs), items, origins, B, Hd,
                                     Wd, h, w, ST);
}
int sbgm_domain_gather(const float* const* srcs, float* const* dsts, const int* n_items, int n_fields, const int32_t* programs,
                       const int* items, int B, int Hd, int Wd, int Wp, void* stream) {
    return sbgm_launch_domain_gather(srcs, dsts, n_items, n_fields, reinterpret_cast<const CutoutProgram*>(programs), items, B, Hd, Wd, Wp,
                                     ST);
}
int64_t sbgm_sdf_workspace_bytes(int B, int h, int w) { return (int64_t)sbgm_sdf_ws_bytes(B, h, w); }
int sbgm_sdf_from_mask(const float* mask, float* sdf, int* d2, void* ws, int B, int h, int w, void* stream) {
    return sbgm_launch_sdf_from_mask(mask, sdf, d2, ws, B, h, w, ST);
}

int sbgm_assemble_conditions(const sbgm_assemble_args* a, void* stream) {
    SBGM_CHECK(a, "assemble_conditions: null args");
    return sbgm_launch_assemble_conditions(*a, ST);
}

int sbgm_extract_tiles(const float* domain, const int* origins, float* tiles, int T, int C, int Hd, int Wd, int th, int tw,
                       void* stream) {
    SBGM_CHECK(domain && origins && tiles, "extract_tiles: null pointer");
    return sbgm_launch_extract_tiles(domain, origins, tiles, T, C, Hd, Wd, th, tw, ST);
}
int sbgm_stitch_tiles(const float* tiles, const int* origins, float* domain, int T, int C, int Hd, int Wd, int th, int tw,
                      int ramp_len, void* stream) {
    SBGM_CHECK(domain && origins && tiles, "stitch_tiles: null pointer");
    return sbgm_launch_stitch_tiles(tiles, origins, domain, T, C, Hd, Wd, th, tw, ramp_len, ST);
}

int sbgm_blend_tile_scores(const float* scores, const int* origins, float* out, int T, int H, int W, int domain_h, int domain_w,
                           int ramp_len, void* stream) {
    return sbgm_launch_blend_tile_scores(scores, out, JointMap{origins, T, H, W, domain_h, domain_w, ramp_len}, ST);
}

int sbgm_depth_to_space2(const float* x, float* y, int B, int H, int W, int C, void* stream) {
    return sbgm_launch_depth_space2(x, y, B, H, W, C, 1, ST);
}
int sbgm_space_to_depth2(const float* y, float* x, int B, int H, int W, int C, void* stream) {
    return sbgm_launch_depth_space2(y, x, B, H, W, C, 0, ST);
}
int sbgm_depth_to_space(const float* x, float* y, int B, int H, int W, int C, int s, void* stream) {
    return sbgm_launch_depth_space(x, y, B, H, W, C, s, 1, ST);
}
int sbgm_space_to_depth(const float* y, float* x, int B, int H, int W, int C, int s, void* stream) {
    return sbgm_launch_depth_space(y, x, B, H, W, C, s, 0, ST);
}
int sbgm_tconv_weight_to_oihw(const float* w, float* oihw, int Cin, int Cout, void* stream) {
    return sbgm_launch_tconv_weight(w, oihw, Cin, Cout, ST);
}

// ---- training path: backward entry points ---------------------------------------------------------------------------
int sbgm_conv_pack_weight_dgrad(const float* w_oihw, float* packed, int Cout, int Cin, int KH, int KW, void* stream) {
    // operator of the data gradient: Cout' = Cin, Cin' = Cout (padded to 16), taps flipped
    return sbgm_launch_pack_conv_weight(w_oihw, packed, Cin, Cout, KH, KW, (Cout + 15) / 16 * 16, ST, 1);
}
int sbgm_conv2d_wgrad(const float* dy, const float* x, float* dw_oihw, float* ws, int B, int H, int W, int c_pad, int Cin, int Cout,
                      int KH, int KW, int stride, int pad, void* stream) {
    return sbgm_launch_conv_wgrad(dy, x, dw_oihw, ws, B, H, W, c_pad, Cin, Cout, KH, KW, stride, pad, ST);
}
int sbgm_conv2d_wgrad_bias(const float* dy, const float* x, float* dw_oihw, float* dbias, float* ws, int B, int H, int W, int c_pad, int Cin,
                           int Cout, int KH, int KW, int stride, int pad, void* stream) {
    SBGM_CHECK(dbias != nullptr, "conv2d_wgrad_bias: dbias is required");
    return sbgm_launch_conv_wgrad(dy, x, dw_oihw, ws, B, H, W, c_pad, Cin, Cout, KH, KW, stride, pad, ST, dbias);
}
static_assert(SBGM_WG_GENERAL1 == SBGM_WGRAD_GENERAL1 && SBGM_WG_GENERAL4 == SBGM_WGRAD_GENERAL4 && SBGM_WG_HALO16 == SBGM_WGRAD_HALO16 &&
                  SBGM_WG_HALO8 == SBGM_WGRAD_HALO8 && SBGM_WG_TAP64 == SBGM_WGRAD_TAP64 && SBGM_WG_TAP128 == SBGM_WGRAD_TAP128 &&
                  SBGM_WG_STEM == SBGM_WGRAD_STEM, "kernels.h and include/sbgm_hip.h number the weight-gradient families alike");
int sbgm_conv2d_wgrad_plan(int B, int H, int W, int c_pad, int Cin, int Cout, int KH, int KW, int stride, int pad, int out[8]) {
    SBGM_CHECK(out != nullptr, "conv2d_wgrad_plan: out is required");
    WgradPlan p;
    if (sbgm_wgrad_plan(&p, B, H, W, c_pad, Cin, Cout, KH, KW, stride, pad)) return 1;
    const int v[8] = {p.family, p.gx, p.gy, p.tiles_per_wg, p.n_tiles, p.direct, p.M, 0};
    std::copy(v, v + 8, out);
    return 0;
}
int sbgm_wgrad_flush_plan(int* out, int cap) {
    int passes = 0, launches = 0;
    const std::vector<WgradFlushRow> rows = sbgm_wgrad_flush_rows(&passes, &launches);
    if (out) {
        out[0] = passes, out[1] = launches;
        for (int i = 0; i < (int)rows.size() && i < cap; ++i) {
            const WgradFlushRow& r = rows[i];
            const int v[7] = {r.family, r.launch, r.gx, r.gy, r.tiles_per_wg, r.n_tiles, r.direct};
            std::copy(v, v + 7, out + 2 + 7 * i);
        }
    }
    return (int)rows.size();
}
int sbgm_colsum(const float* x, const float* y, float* out, int M, int C, void* stream) { return sbgm_launch_colsum(x, y, out, M, C, ST); }
int sbgm_samplesum(const float* x, float* out, int B, int HW, int C, void* stream) { return sbgm_launch_samplesum(x, out, B, HW, C, ST); }
int sbgm_groupnorm_bwd(const float* x, const float* dy, const float* gamma, const float* beta, const float* skip, const float* tbias,
                       const float* mean_rstd, int act, float* dx, float* dskip, float* dgamma, float* dbeta, float* dtbias, float* ws,
                       int B, int HW, int C, int G, void* stream) {
    return sbgm_launch_groupnorm_bwd(x, dy, gamma, beta, skip, tbias, mean_rstd, act, dx, dskip, dgamma, dbeta, dtbias, ws, B, HW, C, G, ST);
}
int sbgm_batchnorm_bwd(const float* x, const float* dy, const float* y, const float* gamma, const float* tbias_after,
                       const float* mean_rstd, int relu, float* dx, float* dres, float* dgamma, float* dbeta, float* ws, int B, int HW,
                       int C, void* stream) {
    return sbgm_launch_batchnorm_bwd(x, dy, y, gamma, tbias_after, mean_rstd, relu, dx, dres, dgamma, dbeta, ws, B, HW, C, ST);
}
int sbgm_layernorm_bwd(const float* x, const float* dy, const float* gamma, float* dx, float* dgamma, float* dbeta, int M, int C,
                       float eps, const float* dx_add, void* stream) {
    return sbgm_launch_layernorm_bwd(x, dy, gamma, dx, dgamma, dbeta, M, C, eps, ST, dx_add);
}
int sbgm_fill_zero(void* p, int64_t bytes, void* stream) {
    SBGM_CHECK(p && bytes >= 0 && bytes % 4 == 0, "fill_zero: bytes=%lld must be a non-negative multiple of 4", (long long)bytes);
    return bytes ? sbgm_zero_async(p, (size_t)bytes, ST) : 0;
}
int sbgm_mha_core_bwd(const float* qkv, const float* dout, float* dqkv, int B, int S, int C, int heads, void* stream) {
    return sbgm_launch_mha_core_bwd(qkv, dout, dqkv, B, S, C, heads, ST);
}
int sbgm_upsample_bilinear_fwd(const float* x, float* y, int B, int H, int W, int C, int scale, void* stream) {
    return sbgm_launch_upsample_bilinear(x, y, B, H, W, C, scale, 0, ST);
}
int sbgm_upsample_bilinear_bwd(const float* dy, float* dx, int B, int H, int W, int C, int scale, void* stream) {
    return sbgm_launch_upsample_bilinear(dy, dx, B, H, W, C, scale, 1, ST);
}
int sbgm_upsample2x_bwd(const float* dy, float* dx, int B, int H, int W, int C, void* stream) {
    return sbgm_launch_upsample2x_bwd(dy, dx, B, H, W, C, ST);
}
int sbgm_conv3x3_cout1_bwd(const float* dout, const float* a, const float* w_tap_c, const float* t, float sigma, float* da,
                           float* dw_tap_c, float* dbias, int B, int H, int W, int C, void* stream) {
    return sbgm_launch_cout1_bwd(dout, a, w_tap_c, t, sigma, da, dw_tap_c, dbias, B, H, W, C, ST);
}
int sbgm_time_proj_bwd(const float* dout, const float* weight, const float* semb, const float* emb_raw, float* dW, float* dbias,
                       float* demb_accum, int B, int D, int ch, void* stream) {
    return sbgm_launch_time_proj_bwd(dout, weight, semb, emb_raw, dW, dbias, demb_accum, B, D, ch, ST);
}
int sbgm_time_proj_multi_bwd(const float* const* douts, const float* const* sembs, float* const* dWs, float* const* dbiases, const int* chs,
                             int n_proj, int B, int D, void* stream) {
    SBGM_CHECK(douts && sembs && dWs && dbiases && chs, "time_proj_multi_bwd: null argument");
    return sbgm_launch_time_proj_multi_bwd(douts, sembs, dWs, dbiases, chs, n_proj, B, D, ST);
}
int sbgm_label_emb_bwd(const float* demb, const int64_t* y, float* dtable, int B, int D, void* stream) {
    return sbgm_launch_label_emb_bwd(demb, y, dtable, B, D, ST);
}
int sbgm_act_fwd(const float* x, float* y, int64_t n, int act, void* stream) { return sbgm_launch_act_fwd(x, y, (size_t)n, act, ST); }
int sbgm_act_bwd(const float* x, const float* dy, float* dx, int64_t n, int act, void* stream) {
    return sbgm_launch_act_bwd(x, dy, dx, (size_t)n, act, ST);
}

int sbgm_em_step(float* x, float* x_mean, const float* score, const float* z, float g2, float dt, float noise_coef,
                 uint64_t seed, uint64_t draw_index, int64_t n, void* stream) {
    const StepScalars sc{0.f, g2, dt, noise_coef, 0.f};
    return sbgm_launch_em_update(x, x_mean, score, z, nullptr, nullptr, &sc, draw_index, nullptr, seed, 1, (size_t)n, 1, ST);
}
int sbgm_langevin_step(float* x, const float* score, const float* z, float snr_noise_norm, void* sumsq_ws, uint64_t seed,
                       uint64_t draw_index, int B, int64_t per_sample, void* stream) {
    return sbgm_launch_langevin(x, score, z, snr_noise_norm, (double*)sumsq_ws, nullptr, draw_index, seed, B, (size_t)per_sample, ST);
}
int sbgm_hold_known(float* x, float* x_mean, const float* known, const float* known_mask, const float* z, float level, uint64_t seed,
                    uint64_t draw_index, int64_t n, void* stream) {
    Hold h{};
    h.known = known;
    h.mask = known_mask;
    return sbgm_launch_hold_known(x, x_mean, z, level, seed, draw_index, (size_t)n, ST, h);
}
int sbgm_cfg_combine(float* out, const float* s_cond, const float* s_uncond, float scale, int64_t n, void* stream) {
    return sbgm_launch_cfg_combine(out, s_cond, s_uncond, scale, (size_t)n, ST);
}
int sbgm_randn_scaled(float* x, float scale, uint64_t seed, uint64_t draw_index, int64_t n, void* stream) {
    return sbgm_launch_init_noise(x, scale, nullptr, seed, nullptr, draw_index, (size_t)n, ST);
}
int sbgm_randn_rows(float* x, float scale, uint64_t seed, uint64_t draw_index, const int32_t* rows, int B, int64_t per_sample, int stride,
                    const float* weights, int lags, void* stream) {
    SBGM_CHECK(x && rows && weights, "randn_rows: x, rows and weights are required");
    SBGM_CHECK(B >= 1 && per_sample >= 4 && per_sample % 4 == 0, "randn_rows: need B >= 1 and per_sample a positive multiple of 4 (B=%d, "
               "per_sample=%lld)", B, (long long)per_sample);
    SBGM_CHECK(lags >= 1 && lags <= SBGM_NOISE_MAX_LAGS && stride >= 1, "randn_rows: need 1 <= lags <= %d and stride >= 1 (lags=%d, stride=%d)",
               SBGM_NOISE_MAX_LAGS, lags, stride);
    return sbgm_launch_init_noise(x, scale, nullptr, seed, nullptr, draw_index, (size_t)B * (size_t)per_sample, ST,
                                  sbgm_noise_rows_map(rows, stride, lags, weights, (size_t)per_sample));
}
int sbgm_randn_domain_rows(float* tiles, float scale, uint64_t seed, uint64_t draw_index, const int32_t* row_dev, const int32_t* origins,
                           int T, int th, int tw, int domain_h, int domain_w, int stride, const float* weights, int lags, void* stream) {
    SBGM_CHECK(tiles && row_dev && origins && weights, "randn_domain_rows: tiles, row_dev, origins and weights are required");
    SBGM_CHECK(T >= 1 && th >= 1 && tw >= 4 && tw % 4 == 0, "randn_domain_rows: need T >= 1, th >= 1 and tw a positive multiple of 4 (T=%d, "
               "th=%d, tw=%d)", T, th, tw);
    SBGM_CHECK(domain_h >= th && domain_w >= tw, "randn_domain_rows: the %d x %d domain is smaller than a %d x %d tile", domain_h, domain_w,
               th, tw);
    SBGM_CHECK(lags >= 1 && lags <= SBGM_NOISE_MAX_LAGS && stride >= 1, "randn_domain_rows: need 1 <= lags <= %d and stride >= 1 (lags=%d, "
               "stride=%d)", SBGM_NOISE_MAX_LAGS, lags, stride);
    // the tile table and the row are read back (this waits for the stream): a tile outside the domain would reach into another row's counters
    std::vector<int> org(2 * (size_t)T);
    int r = 0;
    SBGM_HIP(hipMemcpyAsync(org.data(), origins, org.size() * sizeof(int), hipMemcpyDeviceToHost, ST));
    SBGM_HIP(hipMemcpyAsync(&r, row_dev, sizeof(int), hipMemcpyDeviceToHost, ST));
    SBGM_HIP(hipStreamSynchronize(ST));
    for (int t = 0; t < T; ++t)
        SBGM_CHECK(org[2 * t] >= 0 && org[2 * t + 1] >= 0 && org[2 * t + 1] % 4 == 0 && org[2 * t] + th <= domain_h &&
                   org[2 * t + 1] + tw <= domain_w, "randn_domain_rows: tile %d at (%d, %d) of %d x %d does not lie quad-aligned inside the "
                   "%d x %d domain", t, org[2 * t], org[2 * t + 1], th, tw, domain_h, domain_w);
    SBGM_CHECK((long long)r >= (long long)(lags - 1) * stride, "randn_domain_rows: the row %d must be >= (lags - 1) * stride = %lld", r,
               (long long)(lags - 1) * stride);
    const NoiseMap tiled{origins, th, tw / 4, (domain_w + 3) / 4};
    return sbgm_launch_init_noise(tiles, scale, nullptr, seed, nullptr, draw_index, (size_t)T * th * tw, ST,
                                  sbgm_noise_domain_map(tiled, row_dev, domain_h, stride, lags, weights));
}
int sbgm_edm_churn(float* x, const float* z, float churn_coef, uint64_t seed, uint64_t draw_index, int64_t n, void* stream) {
    const EdmStep sc{0.f, 0.f, 0.f, 0.f, 0.f, churn_coef};
    return sbgm_launch_edm_churn(x, nullptr, z, nullptr, nullptr, &sc, draw_index, seed, (size_t)n, ST);
}
int sbgm_edm_euler(const float* x_hat, const float* score, float* d, float* x_next, float sigma_hat, float sigma_next, int64_t n,
                   void* stream) {
    const EdmStep sc{0.f, sigma_hat, sigma_next, 0.f, 0.f, 0.f};
    return sbgm_launch_edm_euler(x_hat, score, d, x_next, nullptr, nullptr, &sc, nullptr, 0, (size_t)n, ST);
}
int sbgm_edm_heun(float* x, const float* d, const float* score, float sigma_hat, float sigma_next, int64_t n, void* stream) {
    const EdmStep sc{0.f, sigma_hat, sigma_next, 0.f, 0.f, 0.f};
    return sbgm_launch_edm_heun(x, nullptr, d, score, nullptr, nullptr, &sc, nullptr, 0, 1, (size_t)n, ST);
}
int sbgm_dpmpp_2m_step(float* x, const float* score, float* hist, const float* z, float sigma, float c_x, float c_0, float c_1, float c_z,
                       uint64_t seed, uint64_t draw_index, int64_t n, void* stream) {
    const DpmStep sc{sigma, 0.f, 0.f, c_x, c_0, c_1, c_z};
    return sbgm_launch_dpmpp_2m(x, nullptr, score, hist, z, nullptr, nullptr, &sc, draw_index, seed, z != nullptr || c_z != 0.f, nullptr, 0,
                                1, (size_t)n, ST);
}

int64_t sbgm_rk45_state_bytes(int groups) { return (int64_t)sbgm_ode_state_bytes(groups); }
int64_t sbgm_rk45_partials_bytes(int B, int64_t per) { return (int64_t)sbgm_ode_partials_bytes(B, (size_t)per); }
int sbgm_rk45_init(void* state, int groups, double t0, double t_bound, double rtol, double atol, float sigma, int64_t max_steps,
                   void* stream) {
    return sbgm_launch_ode_init(state, groups, t0, t_bound, rtol, atol, sigma, (long long)max_steps, ST);
}
int sbgm_rk45_load(double* y, const float* x, int64_t n, void* stream) { return sbgm_launch_ode_load(y, x, (size_t)n, ST); }
int sbgm_rk45_store(float* x, const double* y, int64_t n, void* stream) { return sbgm_launch_ode_store(x, y, (size_t)n, ST); }
int sbgm_rk45_stage(void* state, int phase, const double* y, double* y_new, const float* K, int64_t k_stride, float* xs, float* t_dev,
                    int B, int64_t per, int per_sample, void* stream) {
    return sbgm_launch_ode_stage(state, phase, y, y_new, K, (size_t)k_stride, xs, t_dev, 1, B, (size_t)per, per_sample, ST);
}
int sbgm_rk45_control(void* state, int what, const double* y, const double* y_new, const float* K, int64_t k_stride, double* partials,
                      int B, int64_t per, int per_sample, void* stream) {
    return sbgm_launch_ode_control(state, what, y, y_new, K, (size_t)k_stride, partials, B, (size_t)per, per_sample, ST);
}
int sbgm_rk45_commit(const void* state, double* y, const double* y_new, float* K, int64_t k_stride, int B, int64_t per, int per_sample,
                     void* stream) {
    return sbgm_launch_ode_commit(state, y, y_new, K, (size_t)k_stride, B, (size_t)per, per_sample, ST);
}
int sbgm_rk45_read(const void* state, int groups, int64_t* stats_i, double* stats_d, void* stream) {
    return sbgm_ode_read_state(state, groups, stats_i, stats_d, ST);
}

// ---- the composed final block on its own (conv_final.hip; the engine's route in forward.hip, without a network) -------------------
int sbgm_final_compose_pack(const float* w1_oihw, const float* b1, const float* w2_oihw, float* wc_oihw, float* bc, int C, void* stream) {
    return sbgm_launch_final_compose(w1_oihw, b1, w2_oihw, wc_oihw, bc, C, (hipStream_t)stream);
}

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
