// The convolution planner: which weight images a weight has, which kernel family a tile names and what that family reads, accepts
// and reports, the one dispatcher, the static tile choice, the autotuner's candidates and timing loop, and the tile-table text.
// Adding a kernel family means: an enumerator and a named constructor in conv_plan.h, a row in FAMILY, a case in each switch over
// the family below, and its candidates / static choice.
#include <cstdio>
#include <cstdlib>

#include "../../include/sbgm_hip.h"
#include "common.h"
#include "kernels.h"

namespace {

enum GeomClass { GEOM_ANY, GEOM_3X3_S1_P1, GEOM_8X8_S2_P3 };
struct FamilyInfo {
    const char* name;
    ConvImage image;     // the weight image the family's kernels read
    GeomClass geom;      // the geometry they accept
    int csv_px;          // profile CSV, tile_px column: pixels per unit of fpx, 0 = 16x16 pixels whatever fpx says
    int csv_ws;          // profile CSV, ws column: the family's code, 0 = ws itself (negative when the weights are a Winograd image)
    int (*gn_chunks)(const ConvParams&, const ConvTile&);   // GroupNorm statistics of the epilogue, null = the family has none
};
const FamilyInfo FAMILY[CONV_FAMILIES] = {
    {"implicit-GEMM", IMG_IGEMM, GEOM_ANY, 16, 0, nullptr},
    {"1-D Winograd", IMG_WINO, GEOM_3X3_S1_P1, 32, 0, nullptr},
    {"LDS-staged direct", IMG_IGEMM, GEOM_3X3_S1_P1, 64, 20, sbgm_conv_lds_gn_chunks},
    {"LDS-staged Winograd", IMG_WINO, GEOM_3X3_S1_P1, 128, -20, sbgm_conv_lds_gn_chunks},
    {"2-D Winograd F(2x2,3x3)", IMG_W2D, GEOM_3X3_S1_P1, 0, -40, sbgm_conv_w2d_gn_chunks},
    {"persistent 2-D Winograd F(2x2,3x3)", IMG_W2D, GEOM_3X3_S1_P1, 0, -40, sbgm_conv_w2d_gn_chunks},
    {"space-to-depth Winograd F(2x2,4x4)", IMG_S2W, GEOM_8X8_S2_P3, 0, -25, nullptr},
};
const char* const GEOM_TEXT[] = {"any geometry", "3x3 stride 1 pad 1", "8x8 stride 2 pad 3"};

bool geom_admits(GeomClass c, int kh, int kw, int stride, int pad) {
    if (c == GEOM_3X3_S1_P1) return kh == 3 && kw == 3 && stride == 1 && pad == 1;
    if (c == GEOM_8X8_S2_P3) return kh == 8 && kw == 8 && stride == 2 && pad == 3;
    return true;
}

constexpr size_t LDS_LIMIT = 160 * 1024;

}  // namespace

const ConvSwitches& sbgm_conv_switches() {
    static const ConvSwitches s{getenv("SBGM_NO_WINOGRAD") != nullptr, getenv("SBGM_NO_WINOGRAD2D") != nullptr,
                                getenv("SBGM_NO_LDS_CONV") != nullptr, getenv("SBGM_STATIC_ROUND1") != nullptr};
    return s;
}

// ---- weight images ---------------------------------------------------------------------------------------------------------------
void sbgm_conv_image_floats(int kh, int kw, int cs, int cout, bool wino, size_t floats[CONV_IMAGES]) {
    const ConvSwitches& sw = sbgm_conv_switches();
    const bool w3 = wino && kh == 3 && kw == 3 && cs % 16 == 0 && !sw.no_wino;
    const bool w8 = wino && kh == 8 && kw == 8 && cs % 16 == 0 && cout % 16 == 0 && !sw.no_wino;
    floats[IMG_IGEMM] = (size_t)sbgm_conv_nsteps(kh, kw, cs) * cout * 16;
    floats[IMG_WINO] = w3 ? sbgm_wino_packed_floats(cout, cs) : 0;
    floats[IMG_W2D] = w3 && !sw.no_w2d ? sbgm_w2d_packed_floats(cout, cs) : 0;
    floats[IMG_S2W] = w8 ? sbgm_s2w_packed_floats(cout, cs) : 0;
}

int sbgm_pack_conv_images(const float* w_oihw, float* const img[CONV_IMAGES], int cout, int cin, int kh, int kw, int cs, hipStream_t st) {
    if (img[IMG_IGEMM] && sbgm_launch_pack_conv_weight(w_oihw, img[IMG_IGEMM], cout, cin, kh, kw, cs, st)) return 1;
    if (img[IMG_WINO] && sbgm_launch_pack_wino_weight(w_oihw, img[IMG_WINO], cout, cin, cs, st)) return 1;
    if (img[IMG_W2D] && sbgm_launch_pack_w2d_weight(w_oihw, img[IMG_W2D], cout, cin, cs, st)) return 1;
    if (img[IMG_S2W] && sbgm_launch_pack_s2w_weight(w_oihw, img[IMG_S2W], cout, cin, cs, st)) return 1;
    return 0;
}

// ---- the dispatcher --------------------------------------------------------------------------------------------------------------
int sbgm_launch_tile(const ConvGeom& g, ConvParams p, const ConvImages& w, const ConvTile& ct, float* partial, hipStream_t st) {
    SBGM_CHECK(ct.well_formed(), "conv: tile kinds (winograd %d, lds %d) name no kernel family", ct.wino, ct.lds);
    const ConvFamily f = ct.family();
    const FamilyInfo& fi = FAMILY[f];
    SBGM_CHECK(geom_admits(fi.geom, g.kh, g.kw, g.stride, g.pad) && (fi.geom == GEOM_ANY || p.in_dil <= 1),
               "conv: the %s kernel is %s only (no input dilation)", fi.name, GEOM_TEXT[fi.geom]);
    SBGM_CHECK(p.in_mode >= 0 && p.in_mode <= 3 && (p.in_mode != 3 || f == FAM_IGEMM),
               "conv: input mode %d is not served by the %s kernel", p.in_mode, fi.name);
    p.wp = w.img[fi.image];
    SBGM_CHECK(p.wp != nullptr, "conv: the %s kernel reads a weight image this weight does not have", fi.name);
    switch (f) {
        case FAM_IGEMM: return sbgm_launch_conv(g, p, ct, partial, st);
        case FAM_WINO: return sbgm_launch_conv_wino(p, ct, st);
        case FAM_LDS:
        case FAM_LDS_WINO: return sbgm_launch_conv_lds(p, ct, st);
        case FAM_W2D:
        case FAM_W2DP: return sbgm_launch_conv_w2d(p, ct, st);
        default: return sbgm_launch_conv_s2w(p, ct, st);
    }
}

// Two convolutions of one input (a BasicBlock's strided 3x3 and its 1x1 shortcut): one launch where the implicit-GEMM family serves the
// pair of tiles (sbgm_conv_pair_served), else the two launches, main first.  Same bits either way.  SBGM_NO_CONV_PAIR=1: always two.
int sbgm_launch_tile_pair(const ConvGeom& gm, ConvParams pm, const ConvImages& wm, const ConvTile& tm, const ConvGeom& ga, ConvParams pa,
                          const ConvImages& wa, const ConvTile& ta, float* partial, hipStream_t st, int* paired) {
    static const bool on = getenv("SBGM_NO_CONV_PAIR") == nullptr;
    if (paired) *paired = 0;
    pm.wp = wm.img[IMG_IGEMM];
    pa.wp = wa.img[IMG_IGEMM];
    if (on && tm.well_formed() && ta.well_formed() && pm.wp && pa.wp && sbgm_conv_pair_served(gm, pm, tm, ga, pa, ta)) {
        if (paired) *paired = 1;
        return sbgm_launch_conv_pair(pm, tm, pa, ta, st);
    }
    if (sbgm_launch_tile(gm, pm, wm, tm, partial, st)) return 1;
    return sbgm_launch_tile(ga, pa, wa, ta, partial, st);
}

int sbgm_tile_gn_chunks(const ConvParams& p, const ConvTile& ct) {
    const auto chunks = FAMILY[ct.family()].gn_chunks;
    return chunks ? chunks(p, ct) : 0;
}

int sbgm_tile_proj_parts(const ConvParams& p, const ConvTile& ct) {
    return FAMILY[ct.family()].image == IMG_W2D ? sbgm_conv_w2d_proj_parts(p, ct) : 1;
}

int sbgm_conv_from_args(const sbgm_conv_args* a, ConvGeom* g, ConvParams* out, ConvImages* w, ConvTile* ct) {
    SBGM_CHECK(a && a->x && a->w_packed && a->out, "conv2d: null tensor");
    SBGM_CHECK(a->act == SBGM_NONE || a->act == SBGM_RELU || a->act == SBGM_GELU, "conv2d: act must be none, relu or gelu");
    ConvParams p{};
    p.x = a->x; p.out = a->out; p.scale = a->scale; p.bias = a->bias; p.tbias = a->tbias;
    p.res = a->residual; p.B = a->B; p.H = a->H; p.W = a->W; p.Cs = a->c_pad; p.Cout = a->Cout;
    p.act = a->act; p.tbias_after_act = a->tbias_after_act;
    p.in_dil = a->in_dil; p.out_h = a->out_h; p.out_w = a->out_w;
    p.in_mode = a->in_mode; p.in_affine = a->in_affine; p.in_skip = a->in_skip; p.in_act = a->in_act;
    *out = p;
    *g = ConvGeom{a->KH, a->KW, a->stride, a->pad};
    const int bits = a->winograd;
    // a NULL w_wino / w_wino2d with the bit that selects its kernel: w_packed is that image
    *w = ConvImages{{a->w_packed, a->w_wino ? a->w_wino : (bits & 1) ? a->w_packed : nullptr,
                     a->w_wino2d ? a->w_wino2d : (bits & 8) ? a->w_packed : nullptr, (bits & 32) ? a->w_packed : nullptr}};
    if (bits & 32) {
        SBGM_CHECK((bits & ~32) == 0 && a->in_mode == 0, "conv2d: winograd bit 5 stands alone and takes no in_mode");
        SBGM_CHECK(a->tile_co == 0 || a->tile_co == 1 || a->tile_co == 2, "conv2d: winograd bit 5 takes tile_co 1 or 2");
        *ct = ConvTile::s2w(a->tile_co ? a->tile_co : 2);
        return 0;
    }
    SBGM_CHECK(a->in_mode == 0 || (bits & 3) == 3 || (bits & 8),
               "conv2d: in_mode %d needs an LDS-staged Winograd kernel (winograd bits 0 and 1, or bit 3)", a->in_mode);
    if (bits & 8) {
        SBGM_CHECK(a->w_wino2d || !(bits & 3), "conv2d: winograd bit 3 beside bits 0/1 needs w_wino2d");
        const int fco = a->tile_co ? a->tile_co : 2;
        *ct = (bits & 16) ? ConvTile::w2d_persistent(fco) : ConvTile::w2d(fco, a->waves_per_tile == 2 ? 2 : 1, (bits & 4) != 0);
        return 0;
    }
    const int t[6] = {a->tile_co ? a->tile_co : (a->Cout % 64 == 0 ? 4 : 2), a->tile_px ? a->tile_px : ((bits & 3) ? 1 : 2),
                      a->splits ? a->splits : 1, a->waves_per_tile ? a->waves_per_tile : 1, bits & 1,
                      (bits & 2) ? ((bits & 4) ? 2 : 1) : 0};
    *ct = ConvTile::from_ints(t);
    if (ct->family() != FAM_IGEMM) return 0;
    SBGM_CHECK(a->Cout % 32 == 0, "conv2d: Cout=%d must be a multiple of 32", a->Cout);
    if (ct->splits > 1) {
        const int OH = a->out_h > 0 ? a->out_h : (a->H + 2 * a->pad - a->KH) / a->stride + 1;
        const int OW = a->out_w > 0 ? a->out_w : (a->W + 2 * a->pad - a->KW) / a->stride + 1;
        SBGM_CHECK(a->ws && a->ws_floats >= (int64_t)ct->splits * a->B * OH * OW * a->Cout, "conv2d: split-K workspace too small");
    }
    return 0;
}

// ---- the static choice -----------------------------------------------------------------------------------------------------------
// For a convolution the autotuner has not timed.  It follows what the tuner picks on the BASELINE shapes and on
// small batches (profiles/r03_c2_tiles.txt, r03_c4_tiles.txt; B = 1, 2, 8 in DESIGN.md 3.1), so a sampler that never called
// sbgm_model_autotune runs within a few per cent of a tuned one instead of on the round-1 kernels:
//   3x3 stride 1, >= 512 tiles of 16x16 pixels x 16 channels (or the final projection): 2-D Winograd F(2x2,3x3) (conv_w2d.hip) — the
//     persistent 32-channel kernel once there are >= 512 such tiles (two per CU), 16-channel double-buffered workgroups below;
//   fewer tiles, or a fused input mode: the LDS-staged 1-D Winograd kernel on 16-channel slices (conv_lds.hip);
//   3x3 stride 1 with >= 2048 pixels of >= 128 channels (the 8x8 / 4x4 maps of a full batch): 1-D Winograd (conv_wino.hip), the largest
//     tile that still gives >= 256 workgroups, the K loop split over 4 or 8 waves;
//   small problems of any geometry (< 1024 tiles of 32 channels x 16 pixels): that smallest wave tile, K split over the 4 waves of
//     a workgroup and over up to 8 workgroups;
//   8x8 stride 2 pad 3 on a 16-channel-padded input (the stem's second convolution) with >= 256 workgroups: space-to-depth Winograd
//     F(2x2,4x4) (conv_s2w.hip), 32-channel workgroups while they still fill 256 CUs, 16-channel ones below;
//   everything else (strided, 1x1, the stem): wave tiles that fill ~2 waves per SIMD.
static bool s2w_ok(const ConvGeom& g, const ConvParams& p, const ConvImages& w) {
    return w.img[IMG_S2W] != nullptr && geom_admits(GEOM_8X8_S2_P3, g.kh, g.kw, g.stride, g.pad) && p.in_dil <= 1 && p.in_mode == 0 &&
           p.proj_w == nullptr && p.c_real == 0 && p.Cs % 16 == 0 && p.Cout % 16 == 0 && p.out_h == 0 && p.out_w == 0;
}
// 16 output channels (the composed final block): only the one-co-tile LDS-staged Winograd kernels serve it.  Timed alone at batch
// 32 x 128^2 / batch 16 x 256^2 (convolution + gather, inputs evicted): 2-D Winograd one-tile with one stage buffer 89 / 162 us,
// persistent 90 / 174 us, row-only 1-D Winograd 97-100 / 172 us, every double-buffered form 113-127 / 200-237 us.  The autotuner
// picks the same one-tile kernel inside the network (profiles/r06_c2_tiles.txt, r06_c4_tiles.txt: 81 / 154 us per launch).
ConvTile sbgm_cout16_tile(const ConvParams& p, const ConvImages& w) {
    const ConvTile w2d = ConvTile::w2d(1);
    if (w.img[IMG_W2D] != nullptr && p.H % 2 == 0 && sbgm_conv_w2d_bytes(w2d, p.in_mode) <= LDS_LIMIT) return w2d;
    return ConvTile::lds_wino(1, 1);
}
ConvTile sbgm_static_tile(const ConvGeom& g, const ConvParams& p, const ConvImages& w) {
    if (p.in_mode == 3) {                    // LayerNorm on load: the tile of the plain 1x1 of the same shape, without grid split-K
        const int ns = p.Cs / 16;
        if (p.Cout % 32) return ConvTile::igemm(1, 2, 1, ns >= 8 ? 4 : ns >= 4 ? 2 : 1);       // only its 16-channel tiles serve such a Cout
        ConvParams q = p;
        q.in_mode = 0;
        ConvTile t = sbgm_static_tile(g, q, w);
        t.splits = 1;
        return t;
    }
    const int OH = (p.H + 2 * g.pad - g.kh) / g.stride + 1, OW = (p.W + 2 * g.pad - g.kw) / g.stride + 1;
    const bool round1 = sbgm_conv_switches().round1;                         // the round-1 table (A/B of this function)
    const bool lds_ok = !sbgm_conv_switches().no_lds && !round1;
    const bool has_wino = w.img[IMG_WINO] != nullptr, has_w2d = w.img[IMG_W2D] != nullptr;
    const bool s1 = geom_admits(GEOM_3X3_S1_P1, g.kh, g.kw, g.stride, g.pad) && p.in_dil <= 1;
    const int M = p.B * OH * OW;
    const int nsteps = sbgm_conv_nsteps(g.kh, g.kw, p.c_real == 2 ? 2 : p.Cs);
    if (s2w_ok(g, p, w) && !round1) {
        const long tiles = (long)p.B * ((OH + 15) / 16) * ((OW + 15) / 16);
        if (p.Cout % 32 == 0 && tiles * (p.Cout / 32) >= 256) return ConvTile::s2w(2);
        if (tiles * (p.Cout / 16) >= 256) return ConvTile::s2w(1);
    }
    if (lds_ok && s1 && p.W % 16 == 0 && p.H % 2 == 0 && p.Cs % 16 == 0) {
        const long tiles16 = (long)p.B * (p.W / 16) * ((p.H + 15) / 16) * (p.Cout / 16);
        if (p.Cout == 16 && !p.proj_w && has_wino) return sbgm_cout16_tile(p, w);
        if (has_w2d && (tiles16 >= 512 || p.proj_w)) {
            const ConvTile big = ConvTile::w2d_persistent(2), mid = ConvTile::w2d_persistent(1);
            if (p.Cout % 32 == 0 && tiles16 >= 1024 && sbgm_conv_w2d_bytes(big, p.in_mode) <= LDS_LIMIT) return big;
            if (p.proj_w && sbgm_conv_w2d_bytes(mid, p.in_mode) <= LDS_LIMIT) return mid;
            for (bool two : {true, false}) {
                const ConvTile small = ConvTile::w2d(1, 1, two);
                if (!p.proj_w && sbgm_conv_w2d_bytes(small, p.in_mode) <= LDS_LIMIT) return small;
            }
        }
        if (has_wino && !p.proj_w && (p.in_mode != 0 || tiles16 >= 256 || (tiles16 >= 128 && p.W >= 32)))
            for (bool two : {true, false}) {
                const ConvTile t = ConvTile::lds_wino(1, 1, two);
                if (sbgm_conv_lds_bytes(t, p.in_mode) <= LDS_LIMIT) return t;
            }
    }
    if (p.in_mode != 0) return ConvTile::lds_wino(p.Cout % 64 == 0 ? 4 : 2, 1);     // fused input modes: LDS-staged Winograd tiles only
    const bool wino_ok = has_wino && s1 && p.W % 2 == 0;
    if (wino_ok && p.proj_w) return ConvTile::wino1d(p.Cout / 16, 1);
    if (wino_ok && !round1 && ((M >= 2048 && p.Cs >= 128) || (M >= 512 && p.Cs >= 512 && p.Cout >= 512))) {
        const int ns = 3 * (p.Cs / 16);
        const int wt[3][2] = {{4, 2}, {4, 1}, {2, 1}};
        for (auto& t : wt) {
            if (p.Cout % (16 * t[0])) continue;
            const long wgs = (long)((M + 32 * t[1] - 1) / (32 * t[1])) * (p.Cout / (16 * t[0]));
            if (wgs >= 256 || (t[0] == 2 && t[1] == 1)) {
                int ws = t[1] == 2 ? 4 : ((p.Cs >= 512 || wgs < 512) ? 8 : 4);
                while (ws > 1 && ns / ws < 2) ws >>= 1;
                return ConvTile::wino1d(t[0], t[1], ws);
            }
        }
    }
    if (wino_ok && round1) {                          // Winograd F(2,3): 1.5x fewer MFMAs; pick waves-per-tile to fill the chip
        const int Mp = p.B * OH * OW / 2, ns = 3 * (p.Cs / 16);
        const long tiles = (long)((Mp + 31) / 32) * (p.Cout / 32);          // (2,2) tiles: 32 channels x 64 pixels
        const int ws = tiles >= 2048 ? 1 : (tiles >= 1024 || ns < 8) ? 2 : 4;
        return ConvTile::wino1d(2, 2, ws);
    }
    if (p.proj_w) return ConvTile::igemm(p.Cout / 16, 2);
    const long t21 = (long)((M + 15) / 16) * (p.Cout / 32);
    if (!round1 && p.Cout % 32 == 0 && t21 < 1024) {
        const int ws = nsteps >= 8 ? 4 : nsteps >= 4 ? 2 : 1;
        int splits = 1;
        while (splits < 8 && t21 * splits * 2 <= 256 && nsteps / (splits * 2 * ws) >= 4) splits *= 2;
        return ConvTile::igemm(2, 1, splits, ws);
    }
    const int target = 2048;                 // ~2 waves per SIMD
    const int cand[3][2] = {{4, 4}, {4, 2}, {2, 2}};
    for (auto& c : cand) {
        if (p.Cout % (16 * c[0])) continue;
        const long tiles = (long)((M + 16 * c[1] - 1) / (16 * c[1])) * (p.Cout / (16 * c[0]));
        for (int ws : {1, 2, 4})
            if (tiles * ws >= target && nsteps / ws >= 2) return ConvTile::igemm(c[0], c[1], 1, ws);
    }
    // tiny problem: 64x32 (or 32x32) tiles, 4 waves per tile, plus split-K over the grid (>= 2 K-steps per wave)
    const int fco = p.Cout % 64 == 0 ? 4 : 2, fpx = 2;
    const long tiles = (long)((M + 16 * fpx - 1) / (16 * fpx)) * (p.Cout / (16 * fco));
    const int ws = nsteps >= 8 ? 4 : nsteps >= 4 ? 2 : 1;
    const int splits = (int)std::min<long>(std::max<long>(1, target / std::max<long>(1, tiles * ws)), std::max(1, nsteps / (2 * ws)));
    return ConvTile::igemm(fco, fpx, splits, ws);
}

// ---- the autotuner ---------------------------------------------------------------------------------------------------------------
// The tile candidates (template x tile x waves-per-tile x split-K) of one convolution; split-K ones only with a partial buffer.
std::vector<ConvTile> sbgm_conv_candidates(const ConvGeom& g, const ConvParams& p, const ConvImages& w, bool partial) {
    const int OH = p.out_h > 0 ? p.out_h : (p.H + 2 * g.pad - g.kh) / g.stride + 1;
    const int OW = p.out_w > 0 ? p.out_w : (p.W + 2 * g.pad - g.kw) / g.stride + 1;
    const int nsteps = sbgm_conv_nsteps(g.kh, g.kw, p.c_real == 2 ? 2 : p.Cs);
    const bool has_wino = w.img[IMG_WINO] != nullptr, has_w2d = w.img[IMG_W2D] != nullptr, lds_ok = !sbgm_conv_switches().no_lds;
    std::vector<ConvTile> cands;
    const int tiles[9][2] = {{4, 4}, {4, 2}, {4, 1}, {2, 4}, {2, 2}, {2, 1}, {1, 4}, {1, 2}, {1, 1}};
    for (auto& t : tiles) {
        if (t[0] == 1 && p.in_mode != 3) break;       // 16-channel wave tiles: the LayerNorm-on-load kernel only
        if (p.in_mode != 0 && p.in_mode != 3) break;  // the fused input modes 1 and 2 exist in the LDS-staged Winograd kernel only
        if (p.Cout % (16 * t[0])) continue;
        if (p.proj_w && 16 * t[0] != p.Cout) continue;
        const long ntile = (long)(((size_t)p.B * OH * OW + 16 * t[1] - 1) / (16 * t[1])) * (p.Cout / (16 * t[0]));
        for (int ws : {1, 2, 4}) {
            if (ws > 1 && (nsteps / ws < 2 || ntile * ws > 32768)) continue;
            for (int sp : {1, 2, 4, 8, 16}) {
                if (sp > 1 && (p.proj_w || p.in_mode == 3 || !partial || nsteps / (sp * ws) < 2 || ntile * ws >= 4096)) continue;   // already enough waves
                cands.push_back(ConvTile::igemm(t[0], t[1], sp, ws));
            }
        }
    }
    const bool s1 = geom_admits(GEOM_3X3_S1_P1, g.kh, g.kw, g.stride, g.pad) && p.in_dil <= 1 &&
                    (p.out_h == 0 || (p.out_h == p.H && p.out_w == p.W));
    if (has_wino && s1 && p.W % 2 == 0 && p.in_mode == 0) {
        const int wt[4][2] = {{4, 1}, {2, 2}, {2, 1}, {4, 2}};
        const int nsw = 3 * (p.Cs / 16);
        for (auto& t : wt) {
            if (p.Cout % (16 * t[0])) continue;
            if (p.proj_w && 16 * t[0] != p.Cout) continue;
            for (int ws : {1, 2, 4, 8}) {
                if (ws > 1 && nsw / ws < 2) continue;
                cands.push_back(ConvTile::wino1d(t[0], t[1], ws));
            }
        }
    }
    if (s1 && p.W % 16 == 0 && p.Cs % 16 == 0 && lds_ok) {
        const int dt[6][2] = {{4, 1}, {4, 2}, {4, 4}, {2, 2}, {2, 4}, {2, 1}};
        for (auto& t : dt) {
            if (p.in_mode != 0) break;
            if (p.Cout % (16 * t[0]) || (p.proj_w && 16 * t[0] != p.Cout)) continue;
            cands.push_back(ConvTile::lds_direct(t[0], t[1]));
            const ConvTile two = ConvTile::lds_direct(t[0], t[1], true);                      // double-buffered
            if (sbgm_conv_lds_bytes(two, 0) <= LDS_LIMIT) cands.push_back(two);
        }
        const int wt2[6][2] = {{4, 1}, {4, 2}, {2, 1}, {2, 2}, {1, 1}, {1, 2}};   // 16-channel slices double the workgroup count of small layers
        if (has_wino)
            for (auto& t : wt2) {
                if (p.Cout % (16 * t[0]) || (p.proj_w && 16 * t[0] != p.Cout)) continue;
                for (bool two : {false, true}) {
                    const ConvTile ct = ConvTile::lds_wino(t[0], t[1], two);
                    if (sbgm_conv_lds_bytes(ct, p.in_mode) <= LDS_LIMIT) cands.push_back(ct);
                }
            }
    }
    // 2-D Winograd F(2x2,3x3), LDS-staged: 16x16-pixel tiles, 16 or 32 channels per workgroup; a tap projection may span several
    // channel tiles (partial planes).  ws = 2 selects the build that is held to two waves per SIMD.
    if (has_w2d && s1 && p.W % 16 == 0 && p.H % 2 == 0 && p.Cs % 16 == 0 && lds_ok)
        for (int fco : {2, 1}) {
            if (p.Cout % (16 * fco)) continue;
            for (bool two : {false, true})
                for (int ws : {1, 2}) {
                    const ConvTile ct = ConvTile::w2d(fco, ws, two);
                    if (fco == 1 && ws == 2) continue;
                    if (sbgm_conv_w2d_bytes(ct, p.in_mode) <= LDS_LIMIT) cands.push_back(ct);
                }
            cands.push_back(ConvTile::w2d_persistent(fco));      // persistent workgroups, LDS-DMA slab (two per CU)
        }
    // 8x8 stride 2 pad 3 as space-to-depth Winograd F(2x2,4x4): 16x16-output tiles, 16 or 32 channels per workgroup
    if (s2w_ok(g, p, w))
        for (int fco : {2, 1})
            if (p.Cout % (16 * fco) == 0) cands.push_back(ConvTile::s2w(fco));
    return cands;
}

// What the timing loop below runs for one call, in its order: the candidates, minus the split-K ones whose partial sums
// (B*OH*OW*Cout floats per split) the workspace of partial_floats floats cannot hold.  sbgm_conv2d_tiles hands out the same list.
std::vector<ConvTile> sbgm_conv_tune_list(const ConvGeom& g, const ConvParams& p, const ConvImages& w, bool partial, size_t partial_floats) {
    const int OH = p.out_h > 0 ? p.out_h : (p.H + 2 * g.pad - g.kh) / g.stride + 1;
    const int OW = p.out_w > 0 ? p.out_w : (p.W + 2 * g.pad - g.kw) / g.stride + 1;
    const size_t mc = (size_t)p.B * OH * OW * p.Cout;
    std::vector<ConvTile> list;
    for (auto& ct : sbgm_conv_candidates(g, p, w, partial))
        if (ct.splits <= 1 || mc * ct.splits <= partial_floats) list.push_back(ct);
    return list;
}

// Times the tile candidates (template x tile x waves-per-tile x split-K) of ONE convolution on its real operands and returns
// the fastest in *best (in: the fallback).  A launch never reads what it writes, so repeating it is harmless.  Synchronises.
int sbgm_tune_conv(const ConvGeom& g, const ConvParams& p, const ConvImages& w, float* partial, size_t partial_floats, hipStream_t st,
                   ConvTile* best) {
    auto launch = [&](const ConvTile& ct) -> int { return sbgm_launch_tile(g, p, w, ct, partial, st); };
    const std::vector<ConvTile> cands = sbgm_conv_tune_list(g, p, w, partial != nullptr, partial_floats);
    hipEvent_t e0, e1;
    SBGM_HIP(hipEventCreate(&e0));
    SBGM_HIP(hipEventCreate(&e1));
    const bool cold = getenv("SBGM_TUNE_WARM") == nullptr;
    float best_ms = 1e30f;
    int rc = 0;
    for (int round = 0; round < 3 && !rc; ++round)          // three interleaved rounds, keep each candidate's best (DVFS / noise)
        for (auto& ct : cands) {
            constexpr int REPS = 6;
            float ms = 0.f;
            if (cold && partial) {
                // In the network a convolution finds its weights cold (the layers in between have streamed hundreds of MB
                // through L2 / Infinity Cache), so every timed launch is preceded by an untimed 48 MiB fill that evicts them:
                // ranking the candidates warm (back-to-back repeats) picked tiles that were 3 % slower per sampling step.
                for (int rep = 0; rep < 3 && !rc; ++rep) {
                    (void)hipMemsetAsync(partial, 0, std::min<size_t>(partial_floats * 4, (size_t)48 << 20), st);
                    (void)hipEventRecord(e0, st);
                    rc = launch(ct);
                    (void)hipEventRecord(e1, st);
                    (void)hipEventSynchronize(e1);
                    float m1 = 0.f;
                    (void)hipEventElapsedTime(&m1, e0, e1);
                    ms += m1;
                }
                if (rc) break;
            } else {
                for (int rep = 0; rep <= REPS && !rc; ++rep) {
                    if (rep == 1) (void)hipEventRecord(e0, st);
                    rc = launch(ct);
                }
                if (rc) break;
                (void)hipEventRecord(e1, st);
                (void)hipEventSynchronize(e1);
                (void)hipEventElapsedTime(&ms, e0, e1);
            }
            if (ms < best_ms) { best_ms = ms; *best = ct; }
        }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return rc;
}

// ---- tile table <-> text ---------------------------------------------------------------------------------------------------------
int sbgm_tile_table_save(const ConvTileTable& table, const char* path) {
    SBGM_CHECK(path, "tune_save: null path");
    FILE* f = fopen(path, "w");
    SBGM_CHECK(f, "tune_save: cannot open %s", path);
    fprintf(f, "# sbgm conv tile table v2\n");
    for (auto& kv : table) {
        const ConvOpKey& k = kv.first;
        int t[6];
        kv.second.to_ints(t);
        fprintf(f, "%d %d %d %d %d %d %d %d %d %d %d | %d %d %d %d %d %d\n", k.kh, k.kw, k.s, k.p, k.B, k.H, k.W, k.Cs, k.Cout, k.proj,
                k.in_mode, t[0], t[1], t[2], t[3], t[4], t[5]);
    }
    fclose(f);
    return 0;
}

// The launchers reject tiles they do not instantiate; here: the ranges that index memory, a pair of kinds that names a family, and a
// key of the geometry that family accepts.
static bool tile_line_ok(const ConvOpKey& k, const ConvTile& t) {
    auto pow2_upto = [](int v, int hi) { return v >= 1 && v <= hi && (v & (v - 1)) == 0; };
    // LayerNorm on load: a 1x1 / stride 1 product over whole 16-channel steps on the implicit-GEMM family, one grid row
    if (k.in_mode == 3 && !(k.kh == 1 && k.kw == 1 && k.s == 1 && k.p == 0 && k.Cs >= 16 && k.Cs % 16 == 0 && k.proj == 0 && t.well_formed() &&
                            t.family() == FAM_IGEMM && t.splits == 1 && t.ws <= 4))
        return false;
    if (k.in_mode < 0 || k.in_mode > 3 || !pow2_upto(t.fco, 4) || !pow2_upto(t.fpx, 4) || t.splits < 1 || t.splits > 64 ||
        !pow2_upto(t.ws, 8) || !t.well_formed() || k.Cout % (16 * t.fco) != 0)
        return false;
    const FamilyInfo& fi = FAMILY[t.family()];
    return geom_admits(fi.geom, k.kh, k.kw, k.s, k.p) && (fi.image != IMG_S2W || t.fco <= 2);      // conv_s2w: 16 or 32 channels per workgroup
}

int sbgm_tile_table_load(ConvTileTable* table, const char* path) {
    SBGM_CHECK(path, "tune_load: null path");
    FILE* f = fopen(path, "r");
    SBGM_CHECK(f, "tune_load: cannot open %s", path);
    char line[256];
    ConvTileTable read;
    int lineno = 0;
    while (fgets(line, sizeof line, f)) {
        ++lineno;
        if (line[0] == '#' || line[0] == '\n') continue;
        ConvOpKey k{};
        int t[6];
        const int n = sscanf(line, "%d %d %d %d %d %d %d %d %d %d %d | %d %d %d %d %d %d", &k.kh, &k.kw, &k.s, &k.p, &k.B, &k.H, &k.W,
                             &k.Cs, &k.Cout, &k.proj, &k.in_mode, &t[0], &t[1], &t[2], &t[3], &t[4], &t[5]);
        if (n != 17 || !tile_line_ok(k, ConvTile::from_ints(t))) {
            fclose(f);
            SBGM_CHECK(false, "tune_load: %s line %d is malformed", path, lineno);
        }
        read[k] = ConvTile::from_ints(t);
    }
    fclose(f);
    for (auto& kv : read) (*table)[kv.first] = kv.second;
    return 0;
}

// ---- profile CSV -----------------------------------------------------------------------------------------------------------------
std::string sbgm_tile_kernel_name(const ConvGeom& g, const ConvTile& t, int Cs, int c_real, int in_mode, bool proj) {
    char b[96];
    const char* two = t.lds == 2 ? "true" : "false";
    switch (t.family()) {
        case FAM_S2W: snprintf(b, sizeof b, "conv8x8s2_s2w_kernel<%d>", t.fco); break;
        case FAM_W2DP: snprintf(b, sizeof b, "conv3x3_w2dp_kernel<%d; %d; %s>", t.fco, in_mode, proj ? "true" : "false"); break;
        case FAM_W2D: snprintf(b, sizeof b, "conv3x3_w2d_kernel<%d; %d; %s; %d>", t.fco, t.ws == 2 ? 2 : 1, two, in_mode); break;
        case FAM_LDS: snprintf(b, sizeof b, "conv3x3_lds_kernel<%d; %d; false; %s; %d>", t.fco, t.fpx, two, in_mode); break;
        case FAM_LDS_WINO: snprintf(b, sizeof b, "conv3x3_lds_kernel<%d; %d; true; %s; %d>", t.fco, t.fpx, two, in_mode); break;
        case FAM_WINO: snprintf(b, sizeof b, "conv3x3_wino_kernel<%d; %d; %d>", t.fco, t.fpx, t.ws); break;
        default:
            if (in_mode == 3) {      // the nine-argument form: the input mode follows the geometry
                snprintf(b, sizeof b, "conv_igemm_kernel<1; 1; 1; 0; 1; %d; %d; 0; %d>", t.fco, t.fpx, t.ws);
                break;
            }
            snprintf(b, sizeof b, "conv_igemm_kernel<%d; %d; %d; %d; %d; %d; %d; %d>", g.kh, g.kw, g.stride, g.pad, t.fco, t.fpx,
                     c_real == 2 ? 2 : (Cs >= 16 ? 0 : Cs), t.ws);
    }
    return b;
}

int sbgm_tile_csv_px(const ConvTile& t) {
    const int unit = FAMILY[t.family()].csv_px;
    return unit ? unit * t.fpx : 256;
}

int sbgm_tile_csv_ws(const ConvTile& t) {
    const FamilyInfo& fi = FAMILY[t.family()];
    return fi.csv_ws ? fi.csv_ws : fi.image == IMG_WINO ? -t.ws : t.ws;
}
