// Internal launcher interface between the kernel translation units and the engine / C-ABI layer.
// Every launcher enqueues on `st`, never synchronises and never allocates (graph-capture safe).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "conv_plan.h"   // ConvGeom, ConvTile, ConvParams, the weight images and the planner

int sbgm_conv_nsteps(int KH, int KW, int cs);
int sbgm_conv_pack_blocks(int Cout, int KH, int KW, int cs);   // workgroups one weight takes in the batched pack launch
// transposed != 0 packs the data-gradient operator (swap Cout/Cin, flip taps); then Cout/Cin are the transposed sizes
int sbgm_launch_pack_conv_weight(const float* w_oihw, float* wp, int Cout, int Cin, int KH, int KW, int cs, hipStream_t st,
                                 int transposed = 0);
struct sbgm_pack_desc;
struct sbgm_adam_desc;
int sbgm_adam_blocks(int64_t numel);
int sbgm_launch_adam_batched(const sbgm_adam_desc* desc_dev, int n, int total_blocks, const float* step_dev, float lr, float beta1,
                             float beta2, float eps, float weight_decay, int decoupled, float grad_scale, hipStream_t st);
int sbgm_launch_adam_ema_batched(const sbgm_adam_desc* desc_dev, float* const* ema_dev, int n, int total_blocks, const float* step_dev, float lr,
                                 float beta1, float beta2, float eps, float weight_decay, int decoupled, float grad_scale, float ema_rate,
                                 hipStream_t st);
int sbgm_launch_ema_batched(const sbgm_adam_desc* desc_dev, float* const* ema_dev, int n, int total_blocks, float ema_rate, hipStream_t st);
int sbgm_launch_pack_conv_weights_batched(const sbgm_pack_desc* desc_dev, int n, int total_blocks, hipStream_t st);
int sbgm_launch_conv(const ConvGeom& g, ConvParams p, const ConvTile& cfg, float* partial_ws, hipStream_t st);
// LayerNorm (gamma, beta) followed by a linear (w [Cout][C], b or null) as operands of the in_mode 3 launch: w2_oihw [Cout][C] =
// W diag(gamma) (I - 11^T/C) and h [Cout] = b + W beta, fp64 sums rounded once; pack w2_oihw as an ordinary 1x1 weight
int sbgm_launch_ln_fold(const float* w, const float* b, const float* gamma, const float* beta, float* w2_oihw, float* h, int C, int Cout,
                        hipStream_t st);
// A BasicBlock's 3x3 / stride 2 / pad 1 convolution (main) and its 1x1 / stride 2 shortcut (aux), both of one input, in ONE launch of
// the implicit-GEMM kernels (conv_igemm.hip): served for a small set of tile combinations without grid split-K; the launch computes what
// the two launches of the same tiles compute, bit for bit
bool sbgm_conv_pair_served(const ConvGeom& gm, const ConvParams& pm, const ConvTile& tm, const ConvGeom& ga, const ConvParams& pa,
                           const ConvTile& ta);
int sbgm_launch_conv_pair(ConvParams pm, const ConvTile& tm, ConvParams pa, const ConvTile& ta, hipStream_t st);
// When set, the launchers below trust that their atomically accumulated scratch (weight-gradient slab, norm-backward sums)
// arrives zeroed and skip their own memsets (the training path zeroes one pooled buffer per step instead of ~75 small ones).
extern int sbgm_scratch_prezeroed;
extern int sbgm_wgrad_deferred;                 // conv_wgrad.hip: bit 0 queues the slab -> OIHW passes, bit 1 the GEMMs, for sbgm_launch_wgrad_flush
int sbgm_wgrad_pending();
void sbgm_wgrad_discard_queue();
int sbgm_launch_wgrad_flush(hipStream_t st);
// What sbgm_launch_conv_wgrad launches for a geometry, and what sbgm_launch_wgrad_flush will launch for a queued GEMM: the launcher and
// the flush act on these, and the C ABI's plan queries report them.  Host arithmetic only.
enum { SBGM_WG_GENERAL1 = 0, SBGM_WG_GENERAL2, SBGM_WG_GENERAL4, SBGM_WG_HALO16, SBGM_WG_HALO8, SBGM_WG_TAP64, SBGM_WG_TAP128, SBGM_WG_STEM };
struct WgradPlan {
    int family;            // SBGM_WG_*
    int gx, gy;            // grid; general kernel: gy = pixel splits
    int tiles_per_wg;      // pixel tiles a workgroup walks; general kernel: pixels per split
    int n_tiles;           // pixel tiles of the call; general kernel: output pixels M
    int direct;            // 1: one workgroup owns a block and stores OIHW, no slab, no layout pass
    int M, OH, OW;
    size_t dy_bytes, x_bytes;
};
int sbgm_wgrad_plan(WgradPlan* p, int B, int H, int W, int Cs, int Cin, int Cout, int KH, int KW, int S, int PAD);
struct WgradFlushRow {
    int family, launch;    // launch: index of the batched launch (table) of its family the GEMM rides in
    int gx, gy, tiles_per_wg, n_tiles, direct;
    int unpack;            // 1: the flush queues a layout pass behind it
};
// rows of the queued GEMMs in launch order; *layout_passes / *unpack_launches: what the flush's layout stage will run
std::vector<WgradFlushRow> sbgm_wgrad_flush_rows(int* layout_passes, int* unpack_launches);

// ---- conv_wino.hip: 3x3 stride-1 pad-1 convolution, 1-D Winograd F(2,3) along rows ------------------------------------
size_t sbgm_wino_packed_floats(int Cout, int cs);
int sbgm_launch_pack_wino_weight(const float* w_oihw, float* up, int Cout, int Cin, int cs, hipStream_t st);
int sbgm_launch_conv_wino(ConvParams p, const ConvTile& cfg, hipStream_t st);   // p.wp = Winograd-packed weights

// ---- conv_lds.hip: 3x3 stride-1 pad-1 convolution with LDS-staged halo patch + weight slab (direct or Winograd) -----------
int sbgm_launch_conv_lds(ConvParams p, const ConvTile& cfg, hipStream_t st);
size_t sbgm_conv_lds_bytes(const ConvTile& cfg, int in_mode);
// chunks per sample the launch above writes into p.gn_stats for this tile, or 0 if that tile cannot produce them
int sbgm_conv_lds_gn_chunks(const ConvParams& p, const ConvTile& cfg);

// ---- conv_w2d.hip: the same convolution as a 2-D Winograd F(2x2,3x3), LDS-staged (FAM_W2D, FAM_W2DP) -----------------------
size_t sbgm_w2d_packed_floats(int Cout, int cs);
int sbgm_launch_pack_w2d_weight(const float* w_oihw, float* up, int Cout, int Cin, int cs, hipStream_t st);
int sbgm_launch_conv_w2d(ConvParams p, const ConvTile& cfg, hipStream_t st);    // p.wp = F(2x2,3x3)-packed weights
size_t sbgm_conv_w2d_bytes(const ConvTile& cfg, int in_mode);
int sbgm_conv_w2d_gn_chunks(const ConvParams& p, const ConvTile& cfg);
// co tiles of a tap-projection launch: each writes its own partial plane [tile][9][M], sbgm_launch_tap_stencil sums `parts` planes
int sbgm_conv_w2d_proj_parts(const ConvParams& p, const ConvTile& cfg);

// ---- conv_s2w.hip: 8x8 stride-2 pad-3 convolution as a space-to-depth Winograd F(2x2,4x4), LDS-staged (FAM_S2W) -----
size_t sbgm_s2w_packed_floats(int Cout, int cs);
int sbgm_launch_pack_s2w_weight(const float* w_oihw, float* up, int Cout, int Cin, int cs, hipStream_t st);
int sbgm_launch_conv_s2w(ConvParams p, const ConvTile& cfg, hipStream_t st);    // p.wp = F(2x2,4x4) space-to-depth weights
size_t sbgm_conv_s2w_bytes(const ConvTile& cfg);

// ---- conv_stem22.hip: the stem's conv2(conv1(.) + tb0) composed into one 22x22 stride-4 correlation (samplers only) --------------
size_t sbgm_stem22_packed_floats(int Cin);      // Wc[25 classes][Cin][33][64][4][4]
size_t sbgm_stem22_bias_floats();               // S[25 classes][4][64][4][4]
int sbgm_launch_pack_stem22(const float* w1_oihw, const float* w2_oihw, float* wc, float* sb, int Cin, hipStream_t st);
// channels c0 .. c0 + nch - 1 of the composed filter over src [B][nch][H][W] (+ S . tb0, + addend, folded BN, ReLU) -> out NHWC
int sbgm_launch_conv_stem22(const float* src, int nch, int c0, int Cin, const float* wc, const float* sb, const float* tb0,
                            const float* addend, const float* scale, const float* bias, int relu, float* out, int B, int H, int W,
                            hipStream_t st);

// ---- conv_final.hip: the final DecoderBlock's conv(conv_up(.)) composed into one 3x3 convolution to the 9 taps of `conv` -------------
// w1 OIHW [C][C][3][3], b1 [C] (conv_up), w2 OIHW [1][C][3][3] (conv) -> wc OIHW [16][C][3][3] (rows 9..15 zero), bc [16]
int sbgm_launch_final_compose(const float* w1_oihw, const float* b1, const float* w2_oihw, float* wc_oihw, float* bc, int C,
                              hipStream_t st);
// sbgm_launch_tap_stencil over the pixel-major rows d [B][H][W][16] a 16-channel convolution writes (floats 0..8 of a row = the taps)
int sbgm_launch_tap_gather_rows(const float* d, const float* bias, const float* t, float sigma, float* out, int B, int H, int W,
                                hipStream_t st);
// The same block as a low-resolution 1x1 product to the 25 positions of the composed 5x5 stencil and a gather through the bilinear x2
// (conv_final.hip, second half).  wz_packed: 9 border classes x [C/16][32][16] A-operand images; beta [9]; wz [9][25][C] may be null.
constexpr int FINAL_LOWRES_ZROW = 28;           // floats per low-res pixel of Z: 25 used + 3 zeros (seven 16-byte stores)
constexpr int FINAL_LOWRES_MAX_C = 128;
size_t sbgm_final_lowres_packed_floats(int C);
size_t sbgm_final_lowres_ws_floats(int B, int h, int w);      // Z [B*h*w][28] + the border strips of the 8 non-interior classes
int sbgm_launch_final_lowres_pack(const float* w1_oihw, const float* b1, const float* w2_oihw, const float* b2, float* wz, float* beta,
                                  float* wz_packed, int C, hipStream_t st);
// x: low-res NHWC [B][h][w][C] (+ affine [B][C/4][2][4], skip, activation on load) -> zbuf (sbgm_final_lowres_ws_floats)
int sbgm_launch_final_mix(const float* x, const float* in_affine, const float* in_skip, int in_act, const float* wz_packed, float* zbuf,
                          int B, int h, int w, int C, hipStream_t st);
// The mix with the skip formed in place (C = 64, the sampler route): skip = conv1(x || cond) + tb0 of the encoder's 8x8 / stride-2 stem as
// sc + tb0 + conv1_x(xin): xin planar [B][2h][2w], sc NHWC [B][h][w][64] = conv1 over the condition channels (null: none), tb0 [B][64],
// w1x = conv1's x-channel weights packed by sbgm_launch_skip_mix_pack ([16 k steps][64 co][4], tap 4 s + kq = 8 v + u)
constexpr int SKIP_MIX_PACKED_FLOATS = 64 * 64;
int sbgm_launch_skip_mix_pack(const float* w1_oihw, float* w1x, int cin, hipStream_t st);
int sbgm_launch_final_mix_skipx(const float* x, const float* in_affine, int in_act, const float* wz_packed, const float* xin,
                                const float* sc, const float* tb0, const float* w1x, float* zbuf, int B, int h, int w, int C,
                                hipStream_t st);
// zbuf -> out [B][1][2h][2w] (/ sigma(t_b) when t is given)
int sbgm_launch_final_gather(const float* zbuf, const float* beta, const float* t, float sigma, float* out, int B, int h, int w,
                             hipStream_t st);

// ---- conv_uplow.hip: a small-map decoder block's conv_up(up(x)) as a low-resolution 1x1 product to the 9 taps and a gather ----------
size_t sbgm_up_lowres_weight_floats(int C);                  // 9 C^2: the OIHW [9C][C][1][1] weight and its implicit-GEMM image alike
size_t sbgm_up_lowres_ws_floats(int B, int h, int w, int C);  // Z [B*h*w][9C]
// w OIHW [C][C][3][3] -> w_taps [9C][C] (row tap * C + co) -> w_packed, the image a 1x1 convolution from C to 9C channels reads
int sbgm_launch_up_lowres_pack(const float* w_oihw, float* w_taps, float* w_packed, int C, hipStream_t st);
// Z -> out [B][2h][2w][C] = conv_up(up(x)) + bias.  G > 0 with stats: the GroupNorm of G groups that follows.  *normed_out = 1: out
// is already normalised (gamma / beta applied, either may be null together); else *chunks_out > 0: raw map + that many chunk partials
// in stats ([b][chunk][G][2], what sbgm_launch_groupnorm_apply reduces); else the raw map alone.
int sbgm_launch_up_gather(const float* z, const float* bias, float* out, const float* gamma, const float* beta, double* stats, int G,
                          float eps, int B, int h, int w, int C, int* chunks_out, int* normed_out, hipStream_t st);

// ---- pointwise.hip ---------------------------------------------------------------------------------
struct PackSrc {
    const float* ptr[4];   // NCHW sources, concatenated along C in this order
    int ch[4];
    int n;
    int c0;                // channel of dst the first source lands on (the channels below it are written as zeros)
};
int sbgm_launch_pack_input(const PackSrc& src, float* dst_nhwc, int B, int H, int W, int Cs, hipStream_t st);
int sbgm_launch_nhwc_to_nchw(const float* src, float* dst, int B, int H, int W, int C, hipStream_t st);
int sbgm_launch_nchw_to_nhwc(const float* src, float* dst, int B, int H, int W, int C, hipStream_t st);
int sbgm_launch_upsample2x(const float* x, float* y, int B, int H, int W, int C, hipStream_t st);
// nn.Upsample(scale_factor = scale, bilinear, align_corners=False), integer scale 1..16; backward != 0: x = dy (upsampled size), y = dx
int sbgm_launch_upsample_bilinear(const float* x, float* y, int B, int H, int W, int C, int scale, int backward, hipStream_t st);
// [B][H][W][4C] (phase-major channels) <-> [B][2H][2W][C]; to_space = 1: depth -> space
int sbgm_launch_depth_space2(const float* in, float* out, int B, int H, int W, int C, int to_space, hipStream_t st);
int sbgm_launch_depth_space(const float* in, float* out, int B, int H, int W, int C, int s, int to_space, hipStream_t st);   // any stride s
int sbgm_launch_tconv_weight(const float* w_cin_cout_2_2, float* oihw_4cout_cin, int Cin, int Cout, hipStream_t st);
int sbgm_launch_act(float* x, size_t n, int act, hipStream_t st);
int sbgm_launch_bn_fold(const float* gamma, const float* beta, const float* mean, const float* var, float eps,
                        float* scale, float* bias, int C, hipStream_t st);

struct TimeProj {          // out[b][c] = bias[c] + sum_d W[c][d] * silu(emb_g[b][d])
    const float* weight;   // [ch][D] (nn.Linear layout)
    const float* bias;     // [ch]
    float* out;            // [B][ch]
    int ch;
    int emb;               // which embedding (index into freqs[])
    int out_stride = 0;    // floats between the rows of `out` (0: ch, rows packed); a run's time-row table uses its row length
};
struct TimeEmbedArgs {
    const float* t;             // [B]
    const int64_t* y;           // [B] or null
    const float* label_emb;     // [ncls+1][D] or null (added to embedding 0 only)
    const float* freqs[8];      // Gaussian-Fourier W vectors [D/2]
    int n_emb;
    TimeProj proj[16];
    int n_proj;
    float* emb_ws;              // workspace [n_emb][B][D]: silu(embedding)
    float* emb_raw;             // optional [n_emb][B][D]: embedding before the SiLU (training)
    int B, D;
};
int sbgm_launch_time_embed(const TimeEmbedArgs& a, hipStream_t st);

// final 3x3 conv with a single output channel, fused with the division by sigma(t): out NCHW [B,1,H,W]
int sbgm_launch_conv3x3_cout1(const float* x, const float* w_tap_c, const float* bias, const float* t, float sigma,
                              float* out, int B, int H, int W, int C, hipStream_t st);
// out[b,y,x] = (bias + sum_taps d[tap][b, y+kh-1, x+kw-1]) / sigma(t_b): finishes the fused final conv
int sbgm_launch_tap_stencil(const float* d, const float* bias, const float* t, float sigma, float* out, int B, int H, int W,
                            hipStream_t st, int parts = 1);   // parts: partial planes [parts][9][M] summed on the way
int sbgm_launch_pack_cout1_weight(const float* w_oihw, float* w_tap_c, int C, hipStream_t st);

// ---- norm.hip ------------------------------------------------------------------------------------------
// GroupNorm / InstanceNorm over NHWC.  stats_ws: groupnorm needs 16*64*B*G bytes (partial sums per pixel chunk);
// batchnorm needs 24*C bytes (zeroed by the launcher).
// second half of sbgm_launch_groupnorm only: the statistics were already written (by a convolution epilogue) as `chunks` partials
int sbgm_launch_groupnorm_apply(const float* x, float* y, const float* gamma, const float* beta, const float* skip, const float* tbias,
                                int act, int B, int HW, int C, int G, float eps, const double* stats, int chunks, hipStream_t st,
                                float* mr_out = nullptr);
int sbgm_launch_groupnorm(const float* x, float* y, const float* gamma, const float* beta, const float* skip,
                          const float* tbias, int act, int B, int HW, int C, int G, float eps, double* stats_ws,
                          hipStream_t st, float* mr_out = nullptr);   // mr_out: [B][G][2] (mean, rstd) kept for backward
// GroupNorm statistics (chunk partials as written by gn_partial / the conv_lds epilogue) -> per-(sample, channel) affine
// out[b][c/4][0][4] = rstd*gamma, out[b][c/4][1][4] = beta - mean*rstd*gamma (+ tbias[b][c]): what conv_lds applies on load
int sbgm_launch_gn_finalize(const double* stats, int chunks, const float* gamma, const float* beta, const float* tbias, float* out,
                            int B, int HW, int C, int G, float eps, hipStream_t st);
// first half of sbgm_launch_groupnorm only: the chunk partials; returns the chunk count through *chunks
int sbgm_launch_gn_partial(const float* x, double* stats_ws, int B, int HW, int C, int G, int* chunks, hipStream_t st);
int sbgm_launch_layernorm(const float* x, float* y, const float* gamma, const float* beta, int M, int C, float eps,
                          hipStream_t st);
// train-mode BatchNorm2d: batch statistics over (B,H,W), running-stat update, optional residual + ReLU
int sbgm_launch_batchnorm_train(const float* x, float* y, const float* gamma, const float* beta, float* running_mean,
                                float* running_var, const float* res, const float* tbias_after, int relu, int B,
                                int HW, int C, float eps, float momentum, double* stats_ws, hipStream_t st,
                                float* mr_out = nullptr);

// SyncBatchNorm halves (the caller all-reduces stats_ws / the s12 channel sums over the ranks in between)
int sbgm_launch_batchnorm_stats(const float* x, int B, int HW, int C, double* stats_ws, hipStream_t st);
int sbgm_launch_batchnorm_apply(const float* x, float* y, const float* gamma, const float* beta, float* running_mean,
                                float* running_var, const float* res, const float* tbias_after, int relu, int B, int HW, int C,
                                float eps, float momentum, double* stats_ws, double n_total, hipStream_t st, float* mr_out = nullptr);
int sbgm_launch_batchnorm_bwd_reduce(const float* x, const float* dy, const float* y, const float* tbias_after, const float* mr,
                                     int relu, float* s12_ws, int B, int HW, int C, hipStream_t st);
int sbgm_launch_batchnorm_bwd_apply(const float* x, const float* dy, const float* y, const float* gamma, const float* tbias_after,
                                    const float* mr, int relu, float* dx, float* dres, float* dgamma, float* dbeta, const float* s12_ws,
                                    const float* sync_sums, double n_total, int B, int HW, int C, hipStream_t st);

// ---- attention.hip -------------------------------------------------------------------------------------
int sbgm_launch_mha_core(const float* qkv, float* out, int B, int S, int C, int heads, hipStream_t st);
// Which kernel instantiation a shape takes, decided on the host without a device call.  The launchers run exactly what these
// return; the C ABI exposes them (sbgm_*_variant, include/sbgm_hip.h) so that tests can prove they reach every instantiation.
// family codes = the SBGM_MHA_FWD_* / SBGM_MHA_BWD_* enums of the public header.
constexpr int MHA_FWD_REGISTER = 0, MHA_FWD_LDS = 1;
struct MhaFwdPlan {
    int id;            // index into the variant table, -1 = refused
    int family, d16;
    int kn;            // KSPLIT of the register kernel, NQ of the LDS kernel
    int qsplit;        // workgroups per (sample, head) of the LDS kernel (1 for the register kernel)
    float scale;
    int grid;
    size_t lds;
};
int sbgm_mha_fwd_plan(int B, int S, int C, int heads, MhaFwdPlan* p);      // returns p->id
int sbgm_mha_fwd_variant_count();
const char* sbgm_mha_fwd_variant_name(int id);
// attn_tokens.hip: the per-token halves of an attention block, one launch each (C in {64, 128, 256, 512})
int sbgm_attn_tokens_supported(int C);
struct AttnTokensPlan { int id, fco, tok, grid; size_t lds; };               // id: (C/64, tile tokens) of attn_in_kernel and attn_out_kernel
int sbgm_attn_tokens_plan(int M, int C, AttnTokensPlan* p);                 // returns p->id, -1 = refused
int sbgm_attn_tok_variant_count();
const char* sbgm_attn_tok_variant_name(int id);
// ---- attention_dropout.hip: the attention core with train-mode dropout on the softmax probabilities (Philox mask keyed by seed / offset)
// forward: out_or_dqkv = out [B,S,C], dout unused;  backward != 0: out_or_dqkv = dqkv [B,S,3C] (zeroed unless sbgm_scratch_prezeroed)
int sbgm_launch_mha_core_dropout(const float* qkv, const float* dout, float* out_or_dqkv, int B, int S, int C, int heads, float p,
                                 unsigned long long seed, unsigned long long offset, int backward, hipStream_t st);
int sbgm_launch_mha_dropout_mask(float* mask, int B, int S, int heads, float p, unsigned long long seed, unsigned long long offset,
                                 hipStream_t st);
int sbgm_launch_attn_in(const float* x, const float* ln_g, const float* ln_b, const float* w_packed, const float* bias, float* qkv,
                        int M, int C, float eps, hipStream_t st);
int sbgm_launch_attn_out(const float* att, const float* x, const float* wo, const float* bo, const float* ln_g, const float* ln_b,
                         const float* w1, const float* b1, const float* w2, const float* b2, float* out, int M, int C, float eps,
                         hipStream_t st);

// ---- sampler.hip ---------------------------------------------------------------------------------------
struct StepScalars {       // one row of the device-side step table
    float t;               // time fed to the network at this step
    float g2;              // g(t)^2
    float dt;              // step size
    float noise;           // coefficient of the fresh N(0,1) draw in the predictor
    float t_next;          // time of the next step (written to the device time vector after the update)
};
struct SamplerState {      // device-resident, lets one captured graph serve every step
    unsigned long long step;        // advanced by the predictor kernel
    unsigned long long rng_offset;  // Philox counter base, advanced by every noise-drawing kernel
    unsigned long long seed;        // Philox key of the run: read from here when a state is given, so that a captured step is
                                    // reusable across runs with different seeds (the by-value seed argument serves eager calls)
    unsigned long long n_steps;     // length of the run (0: use the launch argument): the last step does not advance past it
};
// the step after step s of a run of ns steps: the last step stays where it is
__host__ __device__ inline unsigned long long sampler_next_step(unsigned long long s, unsigned long long ns) { return s + 1 < ns ? s + 1 : s; }
// optional map from tile-local quads to domain-global Philox counters (null origins = plain element order)
// ... and the optional noise plan ("row-keyed noise"): sample b draws as noise row r_b = rows[b] instead of as its
// position in the batch, and its draw is the moving average z = sum_k w[k] xi(r_b - k stride) over `lags` white rows, every product and
// sum rounded to fp32 on its own.  rows == null (the default) is the plain counter.
// A plan WITH origins is the domain noise plan ("domain rows"): all tiles of the batch are one field on one day, so
// `rows` points to ONE row R that serves every tile, per4 holds Q = domain_height * dom_w4, and the white draw of lag k at domain row Y,
// quad column X4 has the counter (R - k stride) Q + Y dom_w4 + X4.  R = 0 with one lag of weight 1 is the tiled draw without a plan.
constexpr int SBGM_NOISE_MAX_LAGS = 32;
struct NoiseMap {
    const int* origins;   // device [B][2] = (y0, x0) of each tile in the domain, x0 % 4 == 0
    int tile_h, tile_w4;  // tile rows, tile width / 4
    int dom_w4;           // ceil(domain width / 4)
    const int* rows;      // device [B]: the noise row of each sample, every one >= (lags - 1) * stride; with origins: ONE row for all tiles
    int stride, lags;     // rows between two lags (>= 1), number of lags (1 .. SBGM_NOISE_MAX_LAGS)
    unsigned long long per4;            // quads per sample, H W / 4; with origins: quads per domain, domain_height * dom_w4
    float w[SBGM_NOISE_MAX_LAGS];       // the weights, by value
};
// nm with the plan (rows, stride, lags, weights) over samples of per_sample elements
inline NoiseMap sbgm_noise_rows_map(const int* rows, int stride, int lags, const float* w, size_t per_sample) {
    NoiseMap nm{};
    nm.rows = rows; nm.stride = stride; nm.lags = lags; nm.per4 = per_sample / 4;
    for (int k = 0; k < lags && k < SBGM_NOISE_MAX_LAGS; ++k) nm.w[k] = w[k];
    return nm;
}
// the tile map `tiled` with the domain plan (one device row, stride, lags, weights) over a domain of domain_h rows
inline NoiseMap sbgm_noise_domain_map(NoiseMap tiled, const int* row, int domain_h, int stride, int lags, const float* w) {
    tiled.rows = row; tiled.stride = stride; tiled.lags = lags;
    tiled.per4 = (unsigned long long)domain_h * (unsigned long long)tiled.dom_w4;
    for (int k = 0; k < lags && k < SBGM_NOISE_MAX_LAGS; ++k) tiled.w[k] = w[k];
    return tiled;
}
// Joint tiled sampling: the B samples are ALL T tiles of one domain, and every update kernel reads the score through the
// partition-of-unity blend of the tiles' scores (tile_blend.h).  origins == null (the default) is the kernel without the blend.
struct JointMap {
    const int* origins;   // device [T][2] = (y0, x0), x0 % 4 == 0: the run's tile_origins
    int T;                // tiles in the batch
    int tile_h, tile_w;   // tile_w % 4 == 0
    int dom_h, dom_w;     // the domain the ramps are taken against (dom_w: the padded width, a multiple of 4)
    int R;                // ramp length, max(1, overlap)
};
// Constrained sampling: pixels with mask > 0 are held at known + level * z after each state update, in the update
// kernel's own epilogue.  known == null (the default) is the unconstrained kernel.
struct HoldLevels {        // noise levels a held pixel is re-noised to in an SDE step: one row per step, parallel to the step table
    float cur;             // std(t_i): the Langevin corrector's output
    float next;            // std(t_{i+1}), 0 after the last step: the predictor's output
};
struct Hold {
    const float* known;        // [B][H][W] model-space values (anything, NaN included, where mask == 0)
    const float* mask;         // [B][H][W], clamped to [0,1] in the kernel
    const HoldLevels* levels;  // device table indexed by the step counter (with a state), else `lv` by value
    HoldLevels lv;
    // EDM Heun only: its held pixels carry the run's draw 0, read from z0 or (null) recomputed from (seed, offset 0, nm)
    const float* z0;
    unsigned long long seed;   // used without a state (the state's seed otherwise)
    NoiseMap nm;
};
// Time rows of an EM / PC run without labels: every sample of such a run has the same time and all N times are known
// when the run starts, so the n time-bias vectors of every step are computed once per run (rows) and the advance at the end of a step
// copies the next step's row to where the forward reads its time biases (tbrun), the same row for each of the BE samples.
// rows == null (the default): the forward computes its own embedding and projections.
struct TimeRows {
    const float* rows;     // [N][TB]: row s = the n vectors at time table[s].t, concatenated
    float* tbrun;          // [n][BE][ch_i], contiguous: vector i of sample b at tbrun + BE * off_i + b * ch_i
    int n, BE;
    int off4[17];          // start of vector i within a row, in 16-byte quads; off4[n] = TB / 4
};
int sbgm_launch_time_rows_bcast(const TimeRows& tr, int row, hipStream_t st);   // tbrun <- row `row` (the run's first evaluation)
int sbgm_launch_fill_t(float* t, float value, int B, hipStream_t st);
// `state` != null: scalars / RNG offset come from device memory (graph-replayable) and the state is advanced after
// the update; `state` == null: explicit by-value scalars and draw index.
int sbgm_launch_init_noise(float* x, float scale, const float* z, unsigned long long seed, SamplerState* state,
                           unsigned long long draw_index, size_t n, hipStream_t st, NoiseMap nm = NoiseMap{},
                           const Hold& hold = Hold{});       // held: x = scale z + m known
int sbgm_launch_em_update(float* x, float* x_mean, const float* score, const float* z, const StepScalars* table,
                          SamplerState* state, const StepScalars* sc_val, unsigned long long draw_index, float* t_dev,
                          unsigned long long seed, int B, size_t per_sample, int n_steps, hipStream_t st,
                          int t_entries = 0,    // entries of t_dev to refresh (0 -> B; 2B for the batched guidance pass)
                          NoiseMap nm = NoiseMap{}, const Hold& hold = Hold{}, const JointMap& jm = JointMap{},
                          const TimeRows& tr = TimeRows{});    // tr.rows set: the advance also publishes the next step's time row
// jm set: the step size is the batch-mean rule over the raw tile scores (one step size for the domain), not tile mode's per-tile norm
int sbgm_launch_langevin(float* x, const float* score, const float* z, float snr_noise_norm, double* sumsq_ws,
                         SamplerState* state, unsigned long long draw_index, unsigned long long seed, int B,
                         size_t per_sample, hipStream_t st, NoiseMap nm = NoiseMap{}, const Hold& hold = Hold{},
                         const JointMap& jm = JointMap{});
// x = hold(x, known + level z, m), x_mean (may be null) = hold(x_mean, known, m); z null: the Philox draw (seed, draw_index)
int sbgm_launch_hold_known(float* x, float* x_mean, const float* z, float level, unsigned long long seed, unsigned long long draw_index,
                           size_t n, hipStream_t st, const Hold& hold);
int sbgm_launch_cfg_combine(float* out, const float* s_cond, const float* s_uncond, float scale, size_t n, hipStream_t st);

// EDM Heun sampler (Karras et al. 2022, Alg. 2) on the probability-flow ODE of the VE SDE: one row per step i of the
// Karras sigma ladder, built in float64 on the host and stored as fp32 (score_sampling.edm_heun_schedule is the same table)
struct EdmStep {
    float sigma;           // sigma_i
    float sigma_hat;       // sigma_i (1 + gamma_i): the noise level the step starts from after churn
    float sigma_next;      // sigma_{i+1} (0 after the last step)
    float t_hat;           // t(sigma_hat), the time of the step's first evaluation
    float t_next;          // t(sigma_{i+1}), the time of its second evaluation (unused on the last step)
    float churn_coef;      // s_noise * sqrt(sigma_hat^2 - sigma_i^2)
};
// churn: x += churn_coef * z (z null: Philox draw at the run's RNG offset / draw_index); x_copy (may be null) receives x too
int sbgm_launch_edm_churn(float* x, float* x_copy, const float* z, const EdmStep* table, const SamplerState* state,
                          const EdmStep* sc_val, unsigned long long draw_index, unsigned long long seed, size_t n, hipStream_t st,
                          NoiseMap nm = NoiseMap{});
// euler: d = -sigma_hat * score ; x_next = x_hat + (sigma_next - sigma_hat) * d ; t_dev[0 .. t_entries) = t_next
int sbgm_launch_edm_euler(const float* x_hat, const float* score, float* d, float* x_next, const EdmStep* table,
                          const SamplerState* state, const EdmStep* sc_val, float* t_dev, int t_entries, size_t n, hipStream_t st,
                          const Hold& hold = Hold{}, const JointMap& jm = JointMap{});
// heun: x = x_hat + (sigma_next - sigma_hat) * 0.5 (d - sigma_next * score), in place over x_hat (x_copy may be null);
// with a state: t_dev = t_hat of the next step, then the step counter / RNG offset advance
int sbgm_launch_edm_heun(float* x, float* x_copy, const float* d, const float* score, const EdmStep* table, SamplerState* state,
                         const EdmStep* sc_val, float* t_dev, int t_entries, int n_steps, size_t n, hipStream_t st,
                         const Hold& hold = Hold{}, const JointMap& jm = JointMap{});

// DPM-Solver++(2M) sampler (Lu et al. 2022; eta > 0: its SDE variant in midpoint form) on the same Karras ladder: one row per step i,
// built in float64 on the host and stored as fp32 (score_sampling.dpmpp_2m_schedule is the same table).  With D_i = x_i + sigma_i^2 s_i
// the step is x_{i+1} = c_x x_i + c_0 D_i + c_1 D_{i-1} + c_z z_i; row 0 has c_1 = 0 and the last row is (0, 1, 0, 0): x_N = D_{N-1}.
struct DpmStep {
    float sigma;           // sigma_i
    float t;               // t(sigma_i), the time of the step's evaluation
    float t_next;          // t(sigma_{i+1}), the time of the next step's evaluation (unused after the last step)
    float c_x, c_0, c_1;   // coefficients of x_i, D_i and the history D_{i-1}
    float c_z;             // coefficient of the step's draw (0 in a deterministic run and on the last step)
};
// one 2M step: x (in place; x_copy, may be null, receives it too) and hist <- D_i (read only when c_1 != 0); t_dev[0 .. t_entries) =
// t_next; with a state the step counter / RNG offset advance (tr.rows set: the advance also publishes the next step's time row).
// stochastic: the step takes its draw (z, or null: Philox at the run's RNG offset / draw_index); a deterministic step draws nothing.
// Held: x = hold(x, known + level z, m), level = hold.levels[step].next (hold.lv.next without a state), z = the step's draw in a
// stochastic run, else the run's draw 0 (hold.z0 or recomputed).  The history is not held.
int sbgm_launch_dpmpp_2m(float* x, float* x_copy, const float* score, float* hist, const float* z, const DpmStep* table,
                         SamplerState* state, const DpmStep* sc_val, unsigned long long draw_index, unsigned long long seed,
                         int stochastic, float* t_dev, int t_entries, int n_steps, size_t n, hipStream_t st, NoiseMap nm = NoiseMap{},
                         const Hold& hold = Hold{}, const JointMap& jm = JointMap{}, const TimeRows& tr = TimeRows{});

// ---- ode.hip (rk45_sampler: Dormand-Prince 5(4) with scipy's step controller, on the device) -----------------------------------
enum { SBGM_ODE_RUNNING = 0, SBGM_ODE_FINISHED = 1, SBGM_ODE_TOO_SMALL_STEP = 2, SBGM_ODE_NONFINITE = 3, SBGM_ODE_MAX_STEPS = 4 };
enum { SBGM_ODE_PHASE_F0 = 7, SBGM_ODE_PHASE_F1 = 8 };     // stage phases besides the Runge-Kutta stages 1..6
struct OdeHeader {         // head of the device state block of a run; `groups` OdeGroup follow it
    double t0, t_bound, rtol, atol, dir;
    long long max_steps;   // attempts (accepted + rejected) a controller may use
    long long live_attempts;   // attempts during which at least one controller was still running
    float sigma;
    int groups;            // controllers: 1 (error_norm = batch) or B (error_norm = sample)
    int done;              // 1 once no controller is running; the host polls a copy of this word
    int pad_;
};
struct OdeGroup {          // one step controller
    double t, h_abs, h, t_new;     // current time, |step| to try next, signed step and end time of the attempt in flight
    double h0, d1;                 // select_initial_step carry-over
    double c[7];                   // f_s = c[s] * K[s]: the float64 coefficient of each fp32 score slab
    long long nfev, n_accepted, n_rejected;
    int status;            // SBGM_ODE_*
    int rejected;          // a rejection has occurred within the current step
    int accept;            // the last attempt was accepted: the commit kernel moves y_new, K[6] into place
    int pad_;
};
int sbgm_ode_blocks_per_sample(size_t per);
size_t sbgm_ode_state_bytes(int groups);
size_t sbgm_ode_partials_bytes(int B, size_t per);
int sbgm_launch_ode_init(void* state, int groups, double t0, double t_bound, double rtol, double atol, float sigma,
                         long long max_steps, hipStream_t st);
int sbgm_launch_ode_load(double* y, const float* x, size_t n, hipStream_t st);       // y = float64(x)
int sbgm_launch_ode_store(float* x, const double* y, size_t n, hipStream_t st);      // x = fp32(y)
// network input xs, evaluation time(s) t_dev[r * B + b] (r < t_copies) and the coefficient of the evaluation `phase` leads to
int sbgm_launch_ode_stage(void* state, int phase, const double* y, double* y_new, const float* K, size_t k_stride, float* xs,
                          float* t_dev, int t_copies, int B, size_t per, int per_sample, hipStream_t st);
// norm partials + the one-block controller; what = 0 / 1: the two halves of select_initial_step, 2: an attempt's decision
int sbgm_launch_ode_control(void* state, int what, const double* y, const double* y_new, const float* K, size_t k_stride,
                            double* partials, int B, size_t per, int per_sample, hipStream_t st);
int sbgm_launch_ode_commit(const void* state, double* y, const double* y_new, float* K, size_t k_stride, int B, size_t per,
                           int per_sample, hipStream_t st);
int sbgm_ode_read_state(const void* state, int groups, int64_t* stats_i, double* stats_d, hipStream_t st);

// ---- dsm_loss.hip (the loss around the network) -----------------------------------------------------------------------
int sbgm_dsm_nblk(int64_t per_sample);
int sbgm_launch_dsm_perturb(const float* x, const float* z_in, const float* t_in, const unsigned long long* rng,
                            unsigned long long seed, float t_eps, float sigma, float* xp, float* z_out, float* t_out, float* std_out, int B, size_t per, hipStream_t st);
int sbgm_launch_dsm_loss_fwd(const float* score, const float* z, const float* std, const float* sdf, double* partial_ws, float* loss,
                             unsigned long long* rng_advance, int B, size_t per, hipStream_t st);
int sbgm_launch_dsm_loss_bwd(const float* score, const float* z, const float* std, const float* sdf, const float* dloss, float* dscore,
                             int B, size_t per, hipStream_t st);

// ---- batch_pack.hip (before the network) ------------------------------------------------------------------------------
struct sbgm_assemble_args;
int sbgm_launch_assemble_conditions(const sbgm_assemble_args& a, hipStream_t st);

// ---- tiling.hip (full-domain tiles) -----------------------------------------------------------------------------------
int sbgm_launch_extract_tiles(const float* dom, const int* origins, float* tiles, int T, int C, int Hd, int Wd, int th, int tw,
                              hipStream_t st);
int sbgm_launch_stitch_tiles(const float* tiles, const int* origins, float* dom, int T, int C, int Hd, int Wd, int th, int tw,
                             int ramp_len, hipStream_t st);
// out[T][1][th][tw] = the joint blend of scores[T][1][th][tw] (tile_blend.h), out of place; the host checks nothing about the origins
int sbgm_launch_blend_tile_scores(const float* scores, float* out, const JointMap& jm, hipStream_t st);

// ---- cutout.hip (device-resident cutout batches) ----------------------------------------------------------------------
int sbgm_launch_cutout_draw(unsigned long long seed, unsigned long long draw, int B, const int* rect, int h, int w, int Hd, int Wd,
                            int* origins, hipStream_t st);
struct CutoutProgram {                        // one row of the device program table: SBGM_CUTOUT_PROGRAM_WORDS 32-bit words
    int n_ops, is_mask;
    int ops[12];
    float consts[12];
};
int sbgm_launch_cutout_gather(const float* const* srcs, float* const* dsts, const int* n_items, int n_fields, const CutoutProgram* programs,
                              const int* items, const int* origins, int B, int Hd, int Wd, int h, int w, hipStream_t st);
int sbgm_launch_domain_gather(const float* const* srcs, float* const* dsts, const int* n_items, int n_fields, const CutoutProgram* programs,
                              const int* items, int B, int Hd, int Wd, int Wp, hipStream_t st);
long long sbgm_sdf_ws_bytes(int B, int h, int w);
int sbgm_launch_sdf_from_mask(const float* mask, float* sdf, int* d2, void* ws, int B, int h, int w, hipStream_t st);

// ---- postproc.hip (after the sampler) ---------------------------------------------------------------------------------
int sbgm_launch_pointwise_chain(const float* x, float* y, size_t n, int n_ops, const int* ops, const float* consts, hipStream_t st);
int sbgm_launch_sample_extremes(const float* x, int B, size_t per, float q, float* out_max, float* out_q, hipStream_t st);

// ---- conv_wgrad.hip (training path: weight gradients; the plan and flush declarations above are its too) ---------------
int sbgm_launch_conv_wgrad(const float* dy, const float* x, float* dw_oihw, float* dwp_ws, int B, int H, int W, int Cs, int Cin,
                           int Cout, int KH, int KW, int S, int PAD, hipStream_t st,
                           float* dbias = nullptr);   // optional bias gradient [Cout] (zeroed by the launcher unless pre-zeroed)

// ---- backward.hip (training path) ------------------------------------------------------------------------------------
// OIHW operator [4*Cin][Cout][5][5] of the phase-decomposed data gradient of an 8x8/s2/p3 convolution (see backward.hip)
int sbgm_launch_dgrad_phase_weight(const float* w_oihw, float* out, int Cout, int Cin, hipStream_t st);
int sbgm_launch_colsum(const float* x, const float* y, float* out, int M, int C, hipStream_t st);
int sbgm_launch_samplesum(const float* x, float* out, int B, int HW, int C, hipStream_t st);
int sbgm_launch_groupnorm_bwd(const float* x, const float* dy, const float* gamma, const float* beta, const float* skip,
                              const float* tbias, const float* mr, int act, float* dx, float* dskip, float* dgamma, float* dbeta,
                              float* dtbias, float* s12_ws, int B, int HW, int C, int G, hipStream_t st);
int sbgm_launch_batchnorm_bwd(const float* x, const float* dy, const float* y, const float* gamma, const float* tbias_after,
                              const float* mr, int relu, float* dx, float* dres, float* dgamma, float* dbeta, float* s12_ws, int B,
                              int HW, int C, hipStream_t st);
int sbgm_launch_layernorm_bwd(const float* x, const float* dy, const float* gamma, float* dx, float* dgamma, float* dbeta, int M, int C,
                              float eps, hipStream_t st, const float* dx_add = nullptr);   // dx_add [M, C] or null: summed into dx
int sbgm_launch_mha_core_bwd(const float* qkv, const float* dout, float* dqkv, int B, int S, int C, int heads, hipStream_t st);
constexpr int MHA_BWD_MFMA = 0, MHA_BWD_LDS16 = 1, MHA_BWD_LDS32 = 2, MHA_BWD_SCALAR = 3;
struct MhaBwdPlan {
    int id;            // index into the variant table, -1 = refused
    int family;
    int d;             // head dim
    int G;             // query blocks per workgroup of the matrix-pipe kernel (1 elsewhere)
    int grid;
    size_t lds;
};
int sbgm_mha_bwd_plan(int B, int S, int C, int heads, MhaBwdPlan* p);      // returns p->id
int sbgm_mha_bwd_variant_count();
const char* sbgm_mha_bwd_variant_name(int id);
int sbgm_launch_upsample2x_bwd(const float* dy, float* dx, int B, int H, int W, int C, hipStream_t st);
int sbgm_launch_cout1_bwd(const float* dout, const float* a, const float* w_tap_c, const float* t, float sigma, float* da,
                          float* dw_tap_c, float* dbias, int B, int H, int W, int C, hipStream_t st);
int sbgm_launch_time_proj_bwd(const float* dout, const float* weight, const float* semb, const float* emb_raw, float* dW, float* dbias,
                              float* demb_accum, int B, int D, int ch, hipStream_t st);
int sbgm_launch_time_proj_multi_bwd(const float* const* douts, const float* const* sembs, float* const* dWs, float* const* dbs, const int* chs,
                                    int n_proj, int B, int D, hipStream_t st);
int sbgm_launch_label_emb_bwd(const float* demb, const int64_t* y, float* dtable, int B, int D, hipStream_t st);
int sbgm_launch_act_bwd(const float* x, const float* dy, float* dx, size_t n, int act, hipStream_t st);
int sbgm_launch_act_fwd(const float* x, float* y, size_t n, int act, hipStream_t st);
