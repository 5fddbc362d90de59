// The partition-of-unity blend of full-domain tiling, shared by the stitch (tiling.hip) and by the joint update kernels
// (sampler.hip): ONE definition of the ramp weight and ONE gather, so a joint run blends scores exactly as the stitch blends tiles.
#pragma once
#include "common.h"
#include "kernels.h"

// weight of position i of a tile axis of length L that starts at `origin` of a domain axis of length dom_len:
// min(d_lo, d_hi, R) / R with d_lo = i + 1, d_hi = L - i; an edge lying on the domain boundary does not ramp
__device__ __forceinline__ float ramp(int i, int L, int origin, int dom_len, int R) {
    const int lo = origin == 0 ? R : i + 1;                    // distance to the tile's low edge (no ramp on the domain edge)
    const int hi = origin + L == dom_len ? R : L - i;
    return (float)min(min(lo, hi), R) / (float)R;
}

// Joint tiled sampling: the score an update kernel uses at quad i of a [T][1][H][W] score batch whose samples are the T tiles of one
// domain.  For the quad's domain position P it is  sum_t w_t(P) s_t(P) / sum_t w_t(P)  over the tiles t that cover P, in ascending
// tile index with the reading tile at its own place, w_t = ramp_y * ramp_x, fp32 `acc += w * s; wsum += w; acc / wsum` (what
// stitch_tiles_kernel does).  Tile widths and x origins are multiples of 4, so a quad of one tile is a whole quad of every tile that
// covers it.  A quad only its own tile covers is returned as loaded: no arithmetic.  Every copy of P runs the same instruction
// sequence on the same operands, so all copies receive the same bits.  The tile loop is uniform (origins[t] are scalar loads); any number
// of tiles may cover a pixel.  Every read is bounds-checked against the tile, whatever the origins hold.
__device__ __forceinline__ f32x4 joint_score4(const float* __restrict__ score, const JointMap& jm, size_t i) {
    const int w4 = jm.tile_w >> 2;
    const size_t per4 = (size_t)jm.tile_h * w4;
    const size_t b = i / per4, rem = i - b * per4;
    const int y = (int)(rem / w4), x = ((int)(rem - (size_t)y * w4)) << 2;
    const int Y = jm.origins[2 * b] + y, X = jm.origins[2 * b + 1] + x;
    int covers = 0;
    for (int t = 0; t < jm.T; ++t) {
        const int yy = Y - jm.origins[2 * t], xx = X - jm.origins[2 * t + 1];
        covers += (yy >= 0 && yy < jm.tile_h && xx >= 0 && xx + 4 <= jm.tile_w) ? 1 : 0;
    }
    if (covers <= 1) return reinterpret_cast<const f32x4*>(score)[i];
    f32x4 acc = {0.f, 0.f, 0.f, 0.f}, wsum = {0.f, 0.f, 0.f, 0.f};
    for (int t = 0; t < jm.T; ++t) {
        const int y0 = jm.origins[2 * t], x0 = jm.origins[2 * t + 1];
        const int yy = Y - y0, xx = X - x0;
        if (yy < 0 || yy >= jm.tile_h || xx < 0 || xx + 4 > jm.tile_w) continue;
        const f32x4 s = reinterpret_cast<const f32x4*>(score)[(size_t)t * per4 + (size_t)yy * w4 + (xx >> 2)];
        const float wy = ramp(yy, jm.tile_h, y0, jm.dom_h, jm.R);
        for (int k = 0; k < 4; ++k) {
            const float w = wy * ramp(xx + k, jm.tile_w, x0, jm.dom_w, jm.R);
            acc[k] += w * s[k];
            wsum[k] += w;
        }
    }
    for (int k = 0; k < 4; ++k) acc[k] = acc[k] / wsum[k];
    return acc;
}
