// The network evaluation: conv / conv_pair / attention and one ScoreNet evaluation as a sequence of stages on a per-call context
// (engine.h says who owns what).
#include <cmath>
#include <cstdio>

#include "engine.h"

// what computes the time biases of B samples at times t into out[i] (rows `stride` floats apart; 0: packed)
int sbgm_model::time_biases(const float* t, const int64_t* y, int B, float* emb_ws, float* const out[9], int stride, hipStream_t st) const {
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

// The tile a convolution runs on: the tuned or static choice, its split-K factor clamped to what the shared scratch holds
ConvTile sbgm_model::settled_tile(const ConvGeom& g, const ConvParams& p, const ConvImages& im) const {
    const int OH = (p.H + 2 * g.pad - g.kh) / g.stride + 1, OW = (p.W + 2 * g.pad - g.kw) / g.stride + 1;
    const size_t mc = (size_t)p.B * OH * OW * p.Cout;
    ConvTile ct = pick_tile(g, p, im);
    if (ct.splits > 1 && mc * ct.splits > PARTIAL_FLOATS) ct.splits = (int)std::max<size_t>(1, PARTIAL_FLOATS / mc);
    return ct;
}

int sbgm_model::conv(const ConvGeom& g, ConvParams p, const Param& w, hipStream_t st) {
    const ConvImages im = w.images();
    const int OH = (p.H + 2 * g.pad - g.kh) / g.stride + 1, OW = (p.W + 2 * g.pad - g.kw) / g.stride + 1;
    if (tuning) {
        // time every candidate on this op, keep the fastest
        const ConvOpKey key = sbgm_conv_op_key(g, p);
        if (tuned.find(key) == tuned.end()) {
            ConvTile best_t = pick_tile(g, p, im);
            if (sbgm_tune_conv(g, p, im, partial, PARTIAL_FLOATS, st, &best_t)) return 1;
            tuned[key] = best_t;
            ++store.plan_gen;
        }
    }
    const ConvTile ct = settled_tile(g, p, im);
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
    const ConvTile tm = settled_tile(gm, pm, im), ta = settled_tile(ga, pa, ia);       // as conv() settles them
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

namespace {

// A decoder block's norm2 + skip + time bias + activation that the next conv_up applies to the low-res pixels it loads
struct Pending { const float* raw; const float* affine; const float* skip; int act; bool live; };

// One evaluation: what its stages share.  Every stage carves its buffers in a fixed order with fixed sizes, whether or not the route
// it takes uses them: that order IS the workspace layout, the measured high-water mark and the addresses a captured step graph holds.
struct Eval {
    sbgm_model& m;
    const float *x, *t;
    const int64_t* y;
    const float *cond, *lsm, *topo;
    float* out;
    float* const* fmaps_out;
    const int B, H, W, bn_train;
    hipStream_t st;
    float* x0 = nullptr;             // the packed network input
    bool skip_mix = false;           // the final mix forms the decoder's last skip (Routes::skip_mix): neither pack_input nor conv1
    float* tb[9] = {};               // the nine time-bias vectors: five encoder maps, four decoder blocks
    double* stats = nullptr;         // GroupNorm / BatchNorm partials
    float* fm[5] = {};               // the encoder's maps, the decoder's skips
    int fh[5] = {}, fw[5] = {};
    float* cur = nullptr;            // the current map [B][ch][cw][cc]
    int ch = 0, cw = 0, cc = 0;
    Pending pend{nullptr, nullptr, nullptr, SBGM_ACT_NONE, false};

    int groups(int c) const { return m.cfg.decoder_norm == SBGM_NORM_GROUP ? std::max(1, std::min(m.cfg.gn_groups, c)) : c; }

    // conv + BatchNorm (+res, relu, late time bias): eval folds BN into the conv epilogue, train runs it after
    int conv_bn(const ConvGeom& g, const float* in, int h, int w, int cs, const ConvW& cvw, BNW& bnw, int cout, const float* res, bool relu,
                const float* tb_after, float* o) {
        ConvParams p{};
        p.x = in; p.B = B; p.H = h; p.W = w; p.Cs = cs; p.Cout = cout;
        if (!bn_train) {
            p.out = o; p.scale = bnw.scale; p.bias = bnw.bias; p.res = res; p.act = relu ? SBGM_ACT_RELU : SBGM_ACT_NONE;
            p.tbias = tb_after; p.tbias_after_act = 1;
            return m.conv(g, p, *cvw.w, st);
        }
        const int oh = (h + 2 * g.pad - g.kh) / g.stride + 1, ow = (w + 2 * g.pad - g.kw) / g.stride + 1;
        float* raw = m.wsalloc((size_t)B * oh * ow * cout);
        if (!raw) return 1;
        p.out = raw;
        if (m.conv(g, p, *cvw.w, st)) return 1;
        return sbgm_launch_batchnorm_train(raw, o, bnw.g->dev(), bnw.b->dev(), bnw.rm->dev(), bnw.rv->dev(), res, tb_after, relu, B,
                                           oh * ow, cout, BN_EPS, BN_MOMENTUM, stats, st);
    }
    // statistics of `v` [B][hw][c] for its GroupNorm: from the convolution epilogue (chunks > 0) or a separate partial pass
    int ensure_stats(const float* v, int hw, int c, int& chunks) {
        if (chunks > 0) return 0;
        return sbgm_launch_gn_partial(v, stats, B, hw, c, groups(c), &chunks, st);
    }
    // conv_up of a block: input `in` [B][ch][cw][ci] (or the pending raw map), output raw [B][2ch][2cw][ci] (+ bias)
    int conv_up(const ConvW& cvw, const float* in, int ci, int oh, int ow, ConvParams& p, float* out_raw) {
        p = ConvParams{};
        p.out = out_raw; p.bias = cvw.b->dev(); p.B = B; p.H = oh; p.W = ow; p.Cs = ci; p.Cout = ci;
        if (m.can_fuse(cvw, ci, ow)) {
            p.in_mode = 2;
            p.x = pend.live ? pend.raw : in;
            if (pend.live) { p.in_affine = pend.affine; p.in_skip = pend.skip; p.in_act = pend.act; }
            pend.live = false;
            return 0;
        }
        SBGM_CHECK(!pend.live, "decoder: a pending normalisation reached an unfused convolution");
        float* up = m.wsalloc((size_t)B * oh * ow * ci);
        if (!up) return 1;
        if (sbgm_launch_upsample2x(in, up, B, oh / 2, ow / 2, ci, st)) return 1;
        p.x = up;
        return 0;
    }

    int begin();
    int inputs();
    int stem();
    int encoder_level(int li);
    int copy_fmaps();
    int decoder_block(int i);
    int final_block();
    int final_transpose(int ci);
    int final_lowres(int ci);
    int final_composed(int ci);
    int final_projection(ConvParams& p);
    int final_plain(ConvParams& p, int ci);
};

// ---- checks and workspace reset --------------------------------------------------------------------------------------
int Eval::begin() {
    const sbgm_model_config& cfg = m.cfg;
    SBGM_CHECK(B >= 1 && H >= 32 && W >= 32 && H % 32 == 0 && W % 32 == 0,
               "forward: H,W must be positive multiples of 32 (five stride-2 stages), got B=%d H=%d W=%d", B, H, W);
    SBGM_CHECK(x && t && out, "forward: x, t and out are required");
    SBGM_CHECK((cfg.n_cond_channels > 0) == (cond != nullptr), "forward: cond_img presence does not match the model (%d channels)", cfg.n_cond_channels);
    SBGM_CHECK((cfg.n_lsm_channels > 0) == (lsm != nullptr), "forward: lsm_cond presence does not match the model");
    SBGM_CHECK((cfg.n_topo_channels > 0) == (topo != nullptr), "forward: topo_cond presence does not match the model");
    SBGM_CHECK(!(y && !m.label_emb), "forward: y given but the model has no label embedding");
    if (sbgm_model_check_complete(&m)) return 1;
    if (!m.tuning) {
        SBGM_CHECK(m.fwd_need(B, H, W, bn_train) <= m.ws_bytes, "forward: workspace not prepared for B=%d H=%d W=%d", B, H, W);
        m.ws_used = 0;
    }
    if (m.refresh_derived(st, m.routes.up_lowres, H, W, m.routes.ln_fold, B)) return 1;
    m.partial = m.wsalloc(sbgm_model::PARTIAL_FLOATS);
    return m.partial ? 0 : 1;
}

// ---- pack inputs, time embedding -------------------------------------------------------------------------------------
int Eval::inputs() {
    const sbgm_model_config& cfg = m.cfg;
    const Routes& routes = m.routes;
    PackSrc src{};
    auto push = [&](const float* p, int c) { if (p && c) { src.ptr[src.n] = p; src.ch[src.n] = c; ++src.n; } };
    push(x, 1); push(lsm, cfg.n_lsm_channels); push(topo, cfg.n_topo_channels); push(cond, cfg.n_cond_channels);
    x0 = m.wsalloc((size_t)B * H * W * m.cs_in);
    if (!x0) return 1;
    // A step sampler's evaluation whose final mix forms the decoder's last skip itself (Routes::skip_mix) launches neither this packing
    // nor conv1 below: the composed stem reads x, and nothing else reads fm[0].  x0 and fm[0] are carved all the same, so every later
    // buffer keeps its address and the measured high-water mark covers the route.
    skip_mix = routes.skip_mix && routes.stem && routes.fin_lowres && !m.tuning && !m.prof && fmaps_out == nullptr;
    if (!skip_mix && sbgm_launch_pack_input(src, x0, B, H, W, m.cs_in, st)) return 1;

    // An EM / PC run without labels keeps its time biases itself (routes.tbrun); the workspace is carved the same either
    // way, so every later buffer keeps its address and the measured high-water mark serves both
    SBGM_CHECK(!routes.tbrun || routes.run_B == B, "forward: the run's time biases hold %d samples, not %d", routes.run_B, B);
    float* emb_ws = m.wsalloc((size_t)5 * B * m.D);
    if (!emb_ws) return 1;
    for (int i = 0; i < 9; ++i) {
        tb[i] = m.wsalloc((size_t)B * (i < 5 ? FMAP_CH[i] : m.dec[i - 5].cout));
        if (!tb[i]) return 1;
    }
    if (routes.tbrun) {
        int off4[10];
        m.time_row_layout(off4);
        for (int i = 0; i < 9; ++i) tb[i] = routes.tbrun + (size_t)B * off4[i] * 4;
    } else if (m.time_biases(t, y, B, emb_ws, tb, 0, st)) return 1;

    // GroupNorm: 64 chunks x B x G x 2 doubles (G = C <= 512 for InstanceNorm); BatchNorm: 24 B x C
    const size_t n_groups = (size_t)B * (cfg.decoder_norm == SBGM_NORM_GROUP ? std::min(cfg.gn_groups, 512) : 512);
    stats = reinterpret_cast<double*>(m.wsalloc(std::max<size_t>(6 * 512, n_groups * 64 * 4)));
    return stats ? 0 : 1;
}

// ---- encoder ---------------------------------------------------------------------------------------------------------
int Eval::stem() {
    fh[0] = H / 2; fw[0] = W / 2;
    fm[0] = m.wsalloc((size_t)B * fh[0] * fw[0] * 64);
    if (!fm[0]) return 1;
    if (!skip_mix) {
        ConvParams p{};
        p.x = x0; p.out = fm[0]; p.tbias = tb[0]; p.B = B; p.H = H; p.W = W; p.Cs = m.cs_in; p.Cout = 64;
        p.c_real = m.cin_total == 2 ? 2 : 0;
        if (m.conv(ConvGeom{8, 8, 2, 3}, p, *m.conv1.w, st)) return 1;                                    // score_unet.py:312-316
    }
    ch = H / 4; cw = W / 4; cc = 64;
    cur = m.wsalloc((size_t)B * ch * cw * 64);
    if (!cur) return 1;
    if (!m.routes.stem) return conv_bn(ConvGeom{8, 8, 2, 3}, fm[0], fh[0], fw[0], 64, m.conv2, m.bn1, 64, nullptr, true, nullptr, cur);   // :321-325
    // sampler runs: conv2(fm[0]) + bn1 + ReLU straight from x, the run's condition term and tb[0] (conv_stem22.hip); conv1 above
    // still writes fm[0], the decoder's last skip, unless the final mix forms it (skip_mix)
    BNW& bn1 = m.bn1;
    float* o = cur;
    if (bn_train) {
        o = m.wsalloc((size_t)B * ch * cw * 64);
        if (!o) return 1;
    }
    if (sbgm_launch_conv_stem22(x, 1, 0, m.cin_total, m.stem.wc, m.stem.sb, tb[0], m.routes.stem_T, bn_train ? nullptr : bn1.scale,
                                bn_train ? nullptr : bn1.bias, bn_train ? 0 : 1, o, B, H, W, st)) return 1;
    if (bn_train && sbgm_launch_batchnorm_train(o, cur, bn1.g->dev(), bn1.b->dev(), bn1.rm->dev(), bn1.rv->dev(), nullptr, nullptr, true, B,
                                                ch * cw, 64, BN_EPS, BN_MOMENTUM, stats, st)) return 1;
    return 0;
}

int Eval::encoder_level(int li) {
    const int nb = (int)m.layers[li].size();
    for (int bi = 0; bi < nb; ++bi) {
        BlockW& b = m.layers[li][bi];
        const int oh = ch / b.stride, ow = cw / b.stride;
        float* y1 = m.wsalloc((size_t)B * oh * ow * b.cout);
        if (!y1) return 1;
        const float* idn = cur;
        if (b.has_ds && !bn_train) {
            // conv1 + bn1 + ReLU and the shortcut's 1x1 + BatchNorm read the same input and do not depend on each other: one launch
            float* d = m.wsalloc((size_t)B * oh * ow * b.cout);
            if (!d) return 1;
            ConvParams pm{}, pa{};
            pm.x = cur; pm.B = B; pm.H = ch; pm.W = cw; pm.Cs = cc; pm.Cout = b.cout;
            pm.tbias_after_act = 1;
            pa = pm;
            pm.out = y1; pm.scale = b.bn1.scale; pm.bias = b.bn1.bias; pm.act = SBGM_ACT_RELU;
            pa.out = d; pa.scale = b.dsbn.scale; pa.bias = b.dsbn.bias; pa.act = SBGM_ACT_NONE;
            if (m.conv_pair(ConvGeom{3, 3, b.stride, 1}, pm, *b.c1.w, ConvGeom{1, 1, b.stride, 0}, pa, *b.ds.w, st)) return 1;
            idn = d;
        } else {
            if (conv_bn(ConvGeom{3, 3, b.stride, 1}, cur, ch, cw, cc, b.c1, b.bn1, b.cout, nullptr, true, nullptr, y1)) return 1;
            if (b.has_ds) {
                float* d = m.wsalloc((size_t)B * oh * ow * b.cout);
                if (!d) return 1;
                if (conv_bn(ConvGeom{1, 1, b.stride, 0}, cur, ch, cw, cc, b.ds, b.dsbn, b.cout, nullptr, false, nullptr, d)) return 1;
                idn = d;
            }
        }
        float* y2 = m.wsalloc((size_t)B * oh * ow * b.cout);
        if (!y2) return 1;
        const float* tba = (bi == nb - 1) ? tb[li + 1] : nullptr;                        // fmap + t_emb (:332,341,350,359)
        if (conv_bn(ConvGeom{3, 3, 1, 1}, y1, oh, ow, b.cout, b.c2, b.bn2, b.cout, idn, true, tba, y2)) return 1;
        cur = y2; ch = oh; cw = ow; cc = b.cout;
    }
    if (m.enc_has_attn[li + 1] && m.attention(m.enc_attn[li + 1], cur, B, ch * cw, st)) return 1;
    fm[li + 1] = cur; fh[li + 1] = ch; fw[li + 1] = cw;
    return 0;
}

int Eval::copy_fmaps() {
    for (int i = 0; i < 5 && fmaps_out; ++i)
        if (fmaps_out[i])
            SBGM_HIP(hipMemcpyAsync(fmaps_out[i], fm[i], (size_t)B * fh[i] * fw[i] * FMAP_CH[i] * 4, hipMemcpyDeviceToDevice, st));
    return 0;
}

// ---- decoder ---------------------------------------------------------------------------------------------------------
// Fused path (default): no GroupNorm-apply or upsample pass between the convolutions of a block.  conv_up reads the
// low-resolution map and interpolates while staging (in_mode 2, with the PREVIOUS block's pending GroupNorm + skip + time
// bias + activation applied to the low-res pixels), `conv` reads conv_up's raw output through norm1's affine (in_mode 1);
// the statistics come out of the producing convolution's epilogue and one tiny finalize launch turns them into the
// per-(sample, channel) scale / shift.  A block whose output feeds attention keeps the separate apply pass, and so do maps
// narrower than 32 pixels: the fused staging costs the (compute-bound) convolution 2-4 us more than the plain one (measured,
// tools/bench_fused_conv.py), which only pays where the pass it replaces streams more than ~8 MB (64 / 128 channels at
// 32x32 and up; at 16x16 x 256 channels the separate 4 us pass is cheaper).  SBGM_NO_FUSED_DECODER=1 forces the separate
// passes everywhere.
int Eval::decoder_block(int i) {
    const sbgm_model_config& cfg = m.cfg;
    DecW& d = m.dec[i];
    const int oh = 2 * ch, ow = 2 * cw;
    SBGM_CHECK(oh == fh[3 - i] && ow == fw[3 - i] && d.cout == FMAP_CH[3 - i], "decoder/skip shape mismatch at block %d", i);
    float* a = m.wsalloc((size_t)B * oh * ow * d.cin);
    if (!a) return 1;
    ConvParams p{};
    int gn1_chunks = 0, normed1 = 0;
    // A small-map block (up_lowres): conv_up(up(cur)) as the 1x1 tap mix on the low-res map and the gather, which also forms norm1
    // where a workgroup holds a whole group.  Z is reserved on every route, so the workspace's high-water mark, measured by a plain
    // evaluation, covers the route as well; a tuning evaluation runs both forms, so the mix and the parent convolution are both tuned.
    const bool lowres = m.up_lowres_block(i, ch, cw);
    float* zb = lowres ? m.wsalloc(sbgm_up_lowres_ws_floats(B, ch, cw, d.cin)) : nullptr;
    if (lowres && !zb) return 1;
    const bool take_lowres = lowres && m.routes.up_lowres;
    if (take_lowres) {
        SBGM_CHECK(!pend.live, "decoder: a pending normalisation reached a low-resolution conv_up");
        p.x = cur; p.out = zb; p.B = B; p.H = ch; p.W = cw; p.Cs = d.cin; p.Cout = 9 * d.cin;
        if (m.conv(ConvGeom{1, 1, 1, 0}, p, m.uplow[i].w1, st)) return 1;
        const bool gn = cfg.decoder_norm == SBGM_NORM_GROUP;
        if (sbgm_launch_up_gather(zb, d.up.b->dev(), a, d.n1g ? d.n1g->dev() : nullptr, d.n1b ? d.n1b->dev() : nullptr, stats,
                                  gn ? groups(d.cin) : 0, GN_EPS, B, ch, cw, d.cin, &gn1_chunks, &normed1, st)) return 1;
    }
    if (take_lowres && !m.tuning) {              // `a` (and what the gather did of norm1) stands
    } else if (cfg.decoder_transpose) {          // ConvTranspose2d: 1x1 conv to 4*cin phase-major channels, then depth -> space
        float* up = m.wsalloc((size_t)B * oh * ow * d.cin);
        if (!up) return 1;
        p.x = cur; p.out = up; p.bias = d.up.b->dev(); p.B = B; p.H = ch; p.W = cw; p.Cs = d.cin; p.Cout = 4 * d.cin;
        if (m.conv(ConvGeom{1, 1, 1, 0}, p, *d.up.w, st)) return 1;
        if (sbgm_launch_depth_space2(up, a, B, ch, cw, d.cin, 1, st)) return 1;
    } else {
        if (conv_up(d.up, cur, d.cin, oh, ow, p, a)) return 1;
        p.gn_stats = stats; p.gn_groups = groups(d.cin);        // GroupNorm statistics in the epilogue when the LDS kernel runs
        if (m.conv(ConvGeom{3, 3, 1, 1}, p, *d.up.w, st)) return 1;
        gn1_chunks = sbgm_tile_gn_chunks(p, m.last_tile);
        normed1 = 0;
    }
    float* c2 = m.wsalloc((size_t)B * oh * ow * d.cout);
    if (!c2) return 1;
    if (!normed1 && ensure_stats(a, oh * ow, d.cin, gn1_chunks)) return 1;
    p = ConvParams{};
    p.B = B; p.H = oh; p.W = ow; p.Cs = d.cin;
    p.x = a; p.out = c2; p.bias = d.conv.b->dev(); p.Cout = d.cout;
    if (normed1) {                               // the gather stored norm1's output
    } else if (m.can_fuse(d.conv, d.cin, ow)) {  // norm1 applied while `conv` stages its patch
        float* aff1 = m.wsalloc((size_t)B * d.cin * 2);
        if (!aff1) return 1;
        if (sbgm_launch_gn_finalize(stats, gn1_chunks, d.n1g ? d.n1g->dev() : nullptr, d.n1b ? d.n1b->dev() : nullptr, nullptr, aff1, B, oh * ow,
                                    d.cin, groups(d.cin), GN_EPS, st)) return 1;
        p.in_mode = 1; p.in_affine = aff1;
    } else if (sbgm_launch_groupnorm_apply(a, a, d.n1g ? d.n1g->dev() : nullptr, d.n1b ? d.n1b->dev() : nullptr, nullptr, nullptr,
                                           SBGM_ACT_NONE, B, oh * ow, d.cin, groups(d.cin), GN_EPS, stats, gn1_chunks, st)) return 1;
    p.gn_stats = stats; p.gn_groups = groups(d.cout);
    if (m.conv(ConvGeom{3, 3, 1, 1}, p, *d.conv.w, st)) return 1;
    int gn2_chunks = sbgm_tile_gn_chunks(p, m.last_tile);
    if (ensure_stats(c2, oh * ow, d.cout, gn2_chunks)) return 1;
    const ConvW& next_up = i < 3 ? m.dec[i + 1].up : m.fin_up;
    if (!d.has_attn && m.can_fuse(next_up, d.cout, 2 * ow)) {
        // norm2 + skip + time bias + activation stay pending: the next conv_up applies them to the low-res pixels it loads
        float* aff2 = m.wsalloc((size_t)B * d.cout * 2);
        if (!aff2) return 1;
        if (sbgm_launch_gn_finalize(stats, gn2_chunks, d.n2g ? d.n2g->dev() : nullptr, d.n2b ? d.n2b->dev() : nullptr, tb[5 + i], aff2, B, oh * ow,
                                    d.cout, groups(d.cout), GN_EPS, st)) return 1;
        pend = Pending{c2, aff2, fm[3 - i], cfg.decoder_activation, true};
    } else {
        if (sbgm_launch_groupnorm_apply(c2, c2, d.n2g ? d.n2g->dev() : nullptr, d.n2b ? d.n2b->dev() : nullptr, fm[3 - i], tb[5 + i],
                                        cfg.decoder_activation, B, oh * ow, d.cout, groups(d.cout), GN_EPS, stats, gn2_chunks, st)) return 1;
        if (d.has_attn && m.attention(d.attn, c2, B, oh * ow, st)) return 1;
    }
    cur = c2; ch = oh; cw = ow;
    return 0;
}

// ---- final block: no norms, no skip, no time, identity activation (score_unet.py:726-730, :757) ----------------------------
int Eval::final_block() {
    const int ci = m.dec[3].cout;
    if (m.cfg.decoder_transpose) return final_transpose(ci);
    // A tuning evaluation keeps timing the composed 3x3 convolution below: SBGM_NO_FINAL_LOWRES=1 still runs it.
    if (m.routes.fin_lowres && !m.tuning) return final_lowres(ci);
    if (m.routes.fin) {
        const Pending pend0 = pend;
        if (final_composed(ci)) return 1;
        if (!m.tuning) return 0;
        pend = pend0;                        // a tuning evaluation also times the projection form below (plain forward, RK45)
    }
    ConvParams p{};
    if (conv_up(m.fin_up, cur, ci, H, W, p, nullptr)) return 1;
    return ci == 64 ? final_projection(p) : final_plain(p, ci);
}

// ConvTranspose2d, then the 64 -> 1 convolution
int Eval::final_transpose(int ci) {
    float* up = m.wsalloc((size_t)B * H * W * ci);
    if (!up) return 1;
    float* a = m.wsalloc((size_t)B * H * W * ci);
    if (!a) return 1;
    ConvParams p{};
    p.x = cur; p.out = up; p.bias = m.fin_up.b->dev(); p.B = B; p.H = ch; p.W = cw; p.Cs = ci; p.Cout = 4 * ci;
    if (m.conv(ConvGeom{1, 1, 1, 0}, p, *m.fin_up.w, st)) return 1;
    if (sbgm_launch_depth_space2(up, a, B, ch, cw, ci, 1, st)) return 1;
    return sbgm_launch_conv3x3_cout1(a, m.fin_conv.w->dev(), m.fin_conv.b->dev(), t, m.cfg.sigma, out, B, H, W, ci, st);
}

// conv(conv_up(up(.))) with the channels mixed at low resolution: Z = Wz . v on the low-res map (the pending normalisation
// applied on load, or the finished map where nothing is pending), then the 5x5 gather through the bilinear x2
int Eval::final_lowres(int ci) {
    float* zb = m.wsalloc(sbgm_final_lowres_ws_floats(B, ch, cw));
    if (!zb) return 1;
    const bool live = pend.live;
    pend.live = false;
    if (skip_mix) {
        // the pending skip is fm[0], which nothing wrote: conv1(x || cond) + tb[0] inside the mix, from x, the run's Sc and tb[0]
        SBGM_CHECK(live && pend.skip == fm[0] && ci == 64, "forward: the final mix cannot form a skip that is not the stem's map");
        if (sbgm_launch_final_mix_skipx(pend.raw, pend.affine, pend.act, m.fin.wz, x, m.routes.skip_Sc, tb[0], m.stem.w1x, zb, B, ch, cw, ci,
                                        st)) return 1;
    } else if (sbgm_launch_final_mix(live ? pend.raw : cur, live ? pend.affine : nullptr, live ? pend.skip : nullptr,
                                     live ? pend.act : SBGM_ACT_NONE, m.fin.wz, zb, B, ch, cw, ci, st)) return 1;
    return sbgm_launch_final_gather(zb, m.fin.beta, t, m.cfg.sigma, out, B, ch, cw, st);
}

// conv(conv_up(.)) composed: one 3x3 convolution from ci to the 9 taps (16 channels stored), rows [M][16], then the gather
int Eval::final_composed(int ci) {
    ConvParams p{};
    if (conv_up(ConvW{&m.fin.cw, &m.fin.cb}, cur, ci, H, W, p, nullptr)) return 1;
    float* d = m.wsalloc((size_t)16 * B * H * W);
    if (!d) return 1;
    p.Cout = 16; p.out = d;
    if (m.conv(ConvGeom{3, 3, 1, 1}, p, m.fin.cw, st)) return 1;
    return sbgm_launch_tap_gather_rows(d, m.fin_conv.b->dev(), t, m.cfg.sigma, out, B, H, W, st);
}

// conv_up's 64-channel output feeds only the linear 3x3 Cout=1 conv: project onto its 9 taps in the epilogue
// (9 floats per pixel instead of 64) and finish with a 9-point gather.
int Eval::final_projection(ConvParams& p) {
    p.proj_w = m.fin_conv.w->dev();
    float* d = m.wsalloc((size_t)9 * B * H * W * 4);      // up to 4 partial planes (2-D Winograd tiles of 16 channels)
    if (!d) return 1;
    p.out = d; p.proj_out = d;
    if (m.conv(ConvGeom{3, 3, 1, 1}, p, *m.fin_up.w, st)) return 1;
    return sbgm_launch_tap_stencil(d, m.fin_conv.b->dev(), t, m.cfg.sigma, out, B, H, W, st, sbgm_tile_proj_parts(p, m.last_tile));
}

// conv_up, then the plain ci -> 1 convolution
int Eval::final_plain(ConvParams& p, int ci) {
    float* a = m.wsalloc((size_t)B * H * W * ci);
    if (!a) return 1;
    p.out = a;
    if (m.conv(ConvGeom{3, 3, 1, 1}, p, *m.fin_up.w, st)) return 1;
    return sbgm_launch_conv3x3_cout1(a, m.fin_conv.w->dev(), m.fin_conv.b->dev(), t, m.cfg.sigma, out, B, H, W, ci, st);
}

}  // namespace

int sbgm_model::forward(const float* x, const float* t, const int64_t* y, const float* cond, const float* lsm, const float* topo,
                        float* out, float* const* fmaps_out, int B, int H, int W, int bn_train, hipStream_t st) {
    Eval e{*this, x, t, y, cond, lsm, topo, out, fmaps_out, B, H, W, bn_train, st};
    int rc = e.begin();
    if (!rc) rc = e.inputs();
    if (!rc) rc = e.stem();
    for (int li = 0; li < 4 && !rc; ++li) rc = e.encoder_level(li);
    if (!rc) rc = e.copy_fmaps();
    for (int i = 0; i < 4 && !rc; ++i) rc = e.decoder_block(i);
    if (!rc) rc = e.final_block();
    if (!rc && !tuning) {                                // the evaluation's high-water mark sizes every later call of this shape
        size_t& pk = ws_peak[std::array<int, 4>{B, H, W, bn_train != 0}];
        pk = std::max(pk, ws_used);
        // (with a step sampler's condition share of conv1: a plain call between two runs must not trim what the next run asks back)
        ws_target = std::max(ws_target, pk + ((size_t)8 << 20) + sampler_keep(B, H, W, 3) + skip_sc_bytes(B, H, W));
    }
    return rc;
}

extern "C" {

int sbgm_model_forward(sbgm_model* m, const float* x, const float* t, const int64_t* y, const float* cond_img,
                       const float* lsm_cond, const float* topo_cond, float* out, float* const* fmaps, int B, int H, int W,
                       int bn_train, void* stream) {
    if (m->ensure_ws(m->ws_need(B, H, W, bn_train))) return 1;
    return m->forward(x, t, y, cond_img, lsm_cond, topo_cond, out, fmaps, B, H, W, bn_train, (hipStream_t)stream);
}

}  // extern "C"
