// The model handle: the parameter table and its placement, the weights derived from it, the workspace rule, autotune and the profiled
// forward (engine.h says who owns what).
#include <cmath>
#include <cstdio>

#include "engine.h"

// ---- weights derived from uploaded weights ---------------------------------------------------------------------
int Derived::source_uploaded(Param* p, const float* src, hipStream_t st) {
    if (!on) return 0;
    if (p->keep_oihw) {
        if (alloc(p->oihw, (size_t)p->numel)) return 1;
        SBGM_HIP(hipMemcpyAsync(p->oihw, src, (size_t)p->numel * 4, hipMemcpyDeviceToDevice, st));
    }
    dirty = true;
    return 0;
}

void Stem::build(Param* w1, Param* w2) {
    on = env_on();
    w1->feeds = w2->feeds = this; w1->keep_oihw = w2->keep_oihw = true;
}
int Stem::prepare(const Param& w1, const Param& w2, int cin_total, hipStream_t st) {
    if (!on || !dirty) return 0;
    SBGM_CHECK(w1.oihw && w2.oihw, "sampler: encoder.conv1 / conv2 weights were never uploaded");
    if (alloc(wc, sbgm_stem22_packed_floats(cin_total)) || alloc(sb, sbgm_stem22_bias_floats())) return 1;
    if (alloc(w1x, SKIP_MIX_PACKED_FLOATS)) return 1;
    if (sbgm_launch_pack_stem22(w1.oihw, w2.oihw, wc, sb, cin_total, st)) return 1;
    if (sbgm_launch_skip_mix_pack(w1.oihw, w1x, cin_total, st)) return 1;
    dirty = false;
    return 0;
}

int FinalBlock::build(const ConvW& up, const ConvW& conv, int ci, bool resize_conv) {
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
int FinalBlock::prepare(const ConvW& up, const ConvW& conv, hipStream_t st) {
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

void UpLowres::build(const ConvW& up, int ci, bool resize_conv) {
    on = env_on() && resize_conv && ci % 16 == 0;
    if (!on) return;
    up.w->feeds = this; up.w->keep_oihw = true;             // the bias is read from its Param at launch: no part of the image
    w1.name = "conv_up.taps.weight"; w1.kind = P_CONV; w1.numel = (int64_t)sbgm_up_lowres_weight_floats(ci);
    w1.cout = 9 * ci; w1.cin = ci; w1.kh = w1.kw = 1; w1.cs = ci;
    w1.floats[IMG_IGEMM] = sbgm_up_lowres_weight_floats(ci);
}
int UpLowres::prepare(const ConvW& up, hipStream_t st) {
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

void LnFold::build(Param* gamma, Param* beta, Param* weight, Param* wbias) {
    g = gamma; b = beta; w = weight; bias = wbias;
    on = env_on() && w->cin % 16 == 0 && w->cs == w->cin;
    if (!on) return;
    g->feeds = b->feeds = w->feeds = bias->feeds = this; w->keep_oihw = true;
    w2.name = w->name + ".ln_folded"; w2.kind = P_CONV; w2.numel = w->numel;
    w2.cout = w->cout; w2.cin = w2.cs = w->cin; w2.kh = w2.kw = 1;
    w2.floats[IMG_IGEMM] = (size_t)w->numel;
}
int LnFold::prepare(hipStream_t st) {
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

// ---- parameter registration ------------------------------------------------------------------------------------
Param* sbgm_model::add(const std::string& name, ParamKind kind, int64_t numel) {
    params.emplace_back(new Param());
    Param* p = params.back().get();
    p->name = name; p->kind = kind; p->numel = numel;
    by_name[name] = p;
    return p;
}
Param* sbgm_model::convw(const std::string& n, int cout, int cin, int kh, int kw, int cs, bool wino) {
    Param* p = add(n, P_CONV, (int64_t)cout * cin * kh * kw);
    p->cout = cout; p->cin = cin; p->kh = kh; p->kw = kw;
    p->cs = cs ? cs : (int)align_up(cin, 16);
    p->want_wino = wino;
    return p;
}
BNW sbgm_model::bn(const std::string& pre, int c) {
    BNW b;
    b.g = vec(pre + ".weight", c); b.b = vec(pre + ".bias", c);
    b.rm = vec(pre + ".running_mean", c); b.rv = vec(pre + ".running_var", c);
    add(pre + ".num_batches_tracked", P_IGNORE, 1);
    b.scale = b.bias = nullptr;
    return b;
}
AttnW sbgm_model::attn(const std::string& pre, int C) {
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
    SBGM_HIP(hipMalloc(&store.d_state, sizeof(SamplerState)));
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
    store.drop_step_graph();                 // its nodes point into the old workspace
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

int sbgm_model::refresh_derived(hipStream_t st, bool up_route, int H, int W, bool ln_route, int B) {
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

// =====================================================================================================================
// C ABI
// =====================================================================================================================
extern "C" {

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
    ++m->store.plan_gen;
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

}  // extern "C"
