// The convolution plan format: which kernel family a tile names, which weight image that family reads, and everything that follows
// from the two (conv_plan.hip).  Nothing outside this module and the five launchers (conv_igemm / conv_wino / conv_lds / conv_w2d /
// conv_s2w.hip, each reading its own family's fields) looks at ConvTile::wino or ConvTile::lds.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstring>
#include <map>
#include <string>
#include <vector>

struct sbgm_conv_args;

struct ConvGeom {
    int kh, kw, stride, pad;
};

// The packed forms of one convolution weight.  A weight always has the implicit-GEMM image; sbgm_conv_image_floats says which others.
enum ConvImage {
    IMG_IGEMM = 0,   // [nsteps][Cout][16] (sbgm_launch_pack_conv_weight); index 0 is also where a non-convolution parameter lives
    IMG_WINO,        // 1-D Winograd F(2,3) of a 3x3 weight (conv_wino.hip pack)
    IMG_W2D,         // 2-D Winograd F(2x2,3x3) of a 3x3 weight (conv_w2d.hip pack)
    IMG_S2W,         // space-to-depth Winograd F(2x2,4x4) of an 8x8 weight (conv_s2w.hip pack)
    CONV_IMAGES
};
struct ConvImages {  // host side, beside ConvParams: launch_tile puts the one the tile's family reads into ConvParams::wp
    const float* img[CONV_IMAGES];
};

enum ConvFamily {
    FAM_IGEMM = 0,   // conv_igemm.hip, any geometry: wave tile (16*fco) channels x (16*fpx) pixels, split-K over the grid and over ws waves
    FAM_WINO,        // conv_wino.hip, 3x3/s1/p1: F(2,3) along rows, fpx counts 32-pixel PAIR fragments, K loop over ws waves
    FAM_LDS,         // conv_lds.hip, 3x3/s1/p1, LDS-staged halo patch + weight slab, direct: fpx = tile rows per wave
    FAM_LDS_WINO,    // conv_lds.hip, the same with the F(2,3) slab: 2*fpx tile rows per wave; the only family with every input mode
    FAM_W2D,         // conv_w2d.hip, 3x3/s1/p1: F(2x2,3x3) on 16x16-pixel tiles, fpx unused, ws = 2: the two-waves-per-SIMD build
    FAM_W2DP,        // conv_w2d.hip, persistent workgroups with an LDS-DMA weight slab, ws = workgroups per CU
    FAM_S2W,         // conv_s2w.hip, 8x8/s2/p3: space-to-depth F(2x2,4x4) on 16x16-output tiles
    CONV_FAMILIES
};

// The six ints are the storage: they are the tile columns of the "v2" tile-table text and the tile[6] of the public ABI.
//   wino: 0 none, 1 F(2,3), 2 F(2x2,3x3), 3 space-to-depth F(2x2,4x4);  lds: 0 not staged, 1 one stage buffer, 2 two, 3 (wino 2) persistent
struct ConvTile {
    int fco, fpx;   // (16*fco) output channels per tile; fpx: see the family
    int splits;     // split-K over gridDim.y (partials + reduce kernel), FAM_IGEMM only
    int ws;         // waves of a workgroup cooperating on one tile (in-workgroup split-K through LDS); see the family
    int wino, lds;

    bool well_formed() const { return wino >= 0 && wino <= 3 && lds >= (wino >= 2 ? 1 : 0) && lds <= (wino == 2 ? 3 : 2); }
    ConvFamily family() const {      // of a well-formed tile
        if (wino == 3) return FAM_S2W;
        if (wino == 2) return lds == 3 ? FAM_W2DP : FAM_W2D;
        if (lds) return wino ? FAM_LDS_WINO : FAM_LDS;
        return wino ? FAM_WINO : FAM_IGEMM;
    }
    static ConvTile igemm(int fco, int fpx, int splits = 1, int ws = 1) { return {fco, fpx, splits, ws, 0, 0}; }
    static ConvTile wino1d(int fco, int fpx, int ws = 1) { return {fco, fpx, 1, ws, 1, 0}; }
    static ConvTile lds_direct(int fco, int rows, bool two_buffers = false) { return {fco, rows, 1, 1, 0, two_buffers ? 2 : 1}; }
    static ConvTile lds_wino(int fco, int rows, bool two_buffers = false) { return {fco, rows, 1, 1, 1, two_buffers ? 2 : 1}; }
    static ConvTile w2d(int fco, int ws = 1, bool two_buffers = false) { return {fco, 1, 1, ws, 2, two_buffers ? 2 : 1}; }
    static ConvTile w2d_persistent(int fco, int ws = 2) { return {fco, 1, 1, ws, 2, 3}; }
    static ConvTile s2w(int fco) { return {fco, 1, 1, 1, 3, 1}; }
    static ConvTile from_ints(const int* t) { return {t[0], t[1], t[2], t[3], t[4], t[5]}; }
    void to_ints(int* t) const { const int v[6] = {fco, fpx, splits, ws, wino, lds}; std::memcpy(t, v, sizeof v); }
};

struct ConvParams {
    const float* x;       // NHWC [B][H][W][Cs]
    const float* wp;      // the weight image the launched kernel reads (set by sbgm_launch_tile from the ConvImages beside this struct)
    float* out;           // NHWC [M][Cout]
    const float* scale;   // [Cout] or null   (folded BatchNorm gamma/sqrt(var+eps))
    const float* bias;    // [Cout] or null
    const float* tbias;   // [B][Cout] or null (time-projection bias, broadcast over pixels)
    const float* res;     // [M][Cout] or null (residual / skip)
    int B, H, W, Cs, Cout;
    int act, tbias_after_act;
    const float* proj_w;  // [9][Cout] or null: fuse the following 3x3 Cout=1 conv's per-tap channel dot products
    float* proj_out;      // [9][M] planar tap sums (then `out` is not written)
    double* gn_stats;     // conv_lds only, or null: per-workgroup GroupNorm partial sums of the OUTPUT (sum, sum of squares per
                          // group) in the [b][chunk][G][2] layout groupnorm_apply reads -> no separate statistics pass
    int gn_groups;        // G of that GroupNorm (channels per group must divide or be a multiple of the tile's channel slice)
    int c_real;           // 0, or 2 with Cs == 4: only 2 of the 4 stored channels are real (the 2-channel stem): a K step is then
                          // 8 taps x 2 channels (weights packed with cs = 2) instead of 4 taps x 4 slots, halving the MFMA work
    int in_dil;           // 1, or 2: read the input through a zero-inserted grid (data-gradient of a stride-2 conv)
    int out_h, out_w;     // explicit output size (required with in_dil == 2), else 0
    // conv_lds only (modes 1, 2) — what happens to the input while the halo patch is staged (conv_lds.hip, "Input modes");
    // conv_igemm only (mode 3) — LayerNorm on load: implicit GEMM 1x1 only, see ln_eps below:
    int in_mode;          // 0 plain; 1 affine on load (x*scale + shift per (sample, channel), zero padding kept); 2 bilinear x2 on
                          // load: x is the LOW-resolution map [B][H/2][W/2][Cs] (H, W stay the convolution's own size), optionally
                          // transformed act(x*scale + shift + skip) before the interpolation
    const float* in_affine;  // [B][Cs/4][2][4] (scale quad, shift quad) from sbgm_launch_gn_finalize, or null
    const float* in_skip;    // mode 2: [B][H/2][W/2][Cs] added before the activation, or null
    int in_act;              // mode 2: SBGM_ACT_* applied to the low-res value
    // filled by sbgm_launch_conv:
    int OH, OW, M, cb_per_tap, nsteps, steps_per_split, n_px_tiles, n_co_tiles;
    uint32_t x_bytes, w_bytes;
    // conv_igemm only — in_mode 3, LayerNorm on load: implicit GEMM 1x1 / stride 1 only.  The rows of x are raw, wp is the folded weight
    // W'' and bias the folded h (sbgm_launch_ln_fold); the kernel finds each row's 1/sqrt(var + ln_eps) from the B operand it loads and
    // scales the accumulator by it.  Cs is the real channel count, a multiple of 16; no grid split-K, no scale, no tap projection.
    // (An input like in_mode, set by the caller; it sits last, in what was the struct's tail padding, so no other field moved.)
    float ln_eps;
};

// ---- weight images ---------------------------------------------------------------------------------------------------------------
// floats[i] = size of image i of an OIHW weight [cout][.][kh][kw] stored with cs input-channel slots, 0 = the weight has no such image.
// wino: the caller wants the Winograd copies its geometry has (a 3x3 layer that runs at stride 1, the stem's second 8x8 / stride 2).
// SBGM_NO_WINOGRAD / SBGM_NO_WINOGRAD2D take images away.
void sbgm_conv_image_floats(int kh, int kw, int cs, int cout, bool wino, size_t floats[CONV_IMAGES]);
// packs every image whose pointer is non-null from the OIHW source
int sbgm_pack_conv_images(const float* w_oihw, float* const img[CONV_IMAGES], int cout, int cin, int kh, int kw, int cs, hipStream_t st);

// ---- one launch of a tile: the only place that selects a launcher and sets p.wp; checks the geometry the tile's family accepts ------
int sbgm_launch_tile(const ConvGeom& g, ConvParams p, const ConvImages& w, const ConvTile& ct, float* partial, hipStream_t st);
// a BasicBlock's strided 3x3 (main) and 1x1 shortcut (aux) of one input: one launch where served, else the two, main first; same bits.
// *paired (may be null): 1 when it was one launch
int sbgm_launch_tile_pair(const ConvGeom& gm, ConvParams pm, const ConvImages& wm, const ConvTile& tm, const ConvGeom& ga, ConvParams pa,
                          const ConvImages& wa, const ConvTile& ta, float* partial, hipStream_t st, int* paired = nullptr);
// GroupNorm statistics that launch leaves in p.gn_stats (chunks per sample), 0 = none
int sbgm_tile_gn_chunks(const ConvParams& p, const ConvTile& ct);
// partial planes [parts][9][M] a tap-projection launch of this tile writes
int sbgm_tile_proj_parts(const ConvParams& p, const ConvTile& ct);
// sbgm_conv_args -> what sbgm_launch_tile takes (winograd bits, zero-means-default tile fields, NULL w_wino / w_wino2d = w_packed)
int sbgm_conv_from_args(const sbgm_conv_args* a, ConvGeom* g, ConvParams* p, ConvImages* w, ConvTile* ct);

// ---- choosing a tile -------------------------------------------------------------------------------------------------------------
struct ConvSwitches { bool no_wino, no_w2d, no_lds, round1; };   // SBGM_NO_WINOGRAD, SBGM_NO_WINOGRAD2D, SBGM_NO_LDS_CONV, SBGM_STATIC_ROUND1
const ConvSwitches& sbgm_conv_switches();                          // read from the environment once
ConvTile sbgm_static_tile(const ConvGeom& g, const ConvParams& p, const ConvImages& w);   // for a convolution the autotuner has not timed
ConvTile sbgm_cout16_tile(const ConvParams& p, const ConvImages& w);                      // ... of 16 output channels (composed final block)
std::vector<ConvTile> sbgm_conv_candidates(const ConvGeom& g, const ConvParams& p, const ConvImages& w, bool partial);
// the candidates the tuner times for one call: sbgm_conv_candidates minus the split-K tiles a workspace of partial_floats floats cannot hold
std::vector<ConvTile> sbgm_conv_tune_list(const ConvGeom& g, const ConvParams& p, const ConvImages& w, bool partial, size_t partial_floats);
// times the candidates of ONE convolution on its real operands, fastest in *best (in: the fallback); synchronises
int sbgm_tune_conv(const ConvGeom& g, const ConvParams& p, const ConvImages& w, float* partial, size_t partial_floats, hipStream_t st,
                   ConvTile* best);

// ---- tile table ------------------------------------------------------------------------------------------------------------------
struct ConvOpKey {
    int kh, kw, s, p, B, H, W, Cs, Cout, proj, in_mode;
    bool operator<(const ConvOpKey& o) const { return std::memcmp(this, &o, sizeof(*this)) < 0; }
};
inline ConvOpKey sbgm_conv_op_key(const ConvGeom& g, const ConvParams& p) {
    return ConvOpKey{g.kh, g.kw, g.stride, g.pad, p.B, p.H, p.W, p.Cs, p.Cout, p.proj_w != nullptr, p.in_mode};
}
typedef std::map<ConvOpKey, ConvTile> ConvTileTable;
// text file, one line per convolution: "kh kw stride pad B H W Cin_pad Cout proj in_mode | fco fpx splits ws wino lds"
// (a linear with a folded LayerNorm, in_mode 3, has a row of its own beside the plain linear of the same shape: 1x1 / stride 1,
// implicit-GEMM tiles with fco in {1, 2, 4} and splits = 1; any other geometry or family under in_mode 3 is refused on load)
int sbgm_tile_table_save(const ConvTileTable& table, const char* path);
int sbgm_tile_table_load(ConvTileTable* table, const char* path);      // adds to / overrides *table; untouched when a line is malformed

// ---- profile CSV -----------------------------------------------------------------------------------------------------------------
std::string sbgm_tile_kernel_name(const ConvGeom& g, const ConvTile& t, int Cs, int c_real, int in_mode, bool proj);
int sbgm_tile_csv_px(const ConvTile& t);    // the tile_px column
int sbgm_tile_csv_ws(const ConvTile& t);    // the ws column: negative codes name the Winograd / LDS families
