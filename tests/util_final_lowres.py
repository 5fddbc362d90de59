"""fp64 reference of the final block mixed at low resolution (csrc/conv_final.hip, second half), in plain torch on the CPU:

    Z_c[s] = sum_ci Wz[c][s][ci] v[ci]                                   low-res, s = (sy, sx) in 5x5, c one of 9 border classes
    out[o] = beta[c(o)] + sum_{s, o + s - 2 inside} up(Z_c(o)[s])[o + s - 2]

`conv` zero-pads conv_up's output, so per axis the first output row drops conv's tap 0 and the last one its tap 2: 3 classes per axis.
The eight non-interior sets are formed on 2-pixel border strips only (NaN elsewhere), as the kernels store them: a read outside a
strip poisons the result."""
import torch

VALID = ((1, 2), (0, 1, 2), (0, 1))          # conv's taps on an axis: first, interior, last output row / column


def class_sets(w1, b1, w2, b2):
    """-> Wz [9][25][C], beta [9] in fp64; class index 3 * cy + cx, position index 5 * sy + sx with s = tap + v"""
    w1, b1, w2, b2 = w1.double(), b1.double(), w2.double(), b2.double()
    C = w1.shape[1]
    wc = torch.einsum("oyx,ocvb->yxcvb", w2[0], w1)          # Wc[ty][tx][ci][vy][vx]
    bc = torch.einsum("oyx,o->yx", w2[0], b1)
    wz, beta = torch.zeros(9, 5, 5, C, dtype=torch.float64), torch.zeros(9, dtype=torch.float64)
    for cy in range(3):
        for cx in range(3):
            c = 3 * cy + cx
            beta[c] = b2[0]
            for ty in VALID[cy]:
                for tx in VALID[cx]:
                    beta[c] += bc[ty, tx]
                    for vy in range(3):
                        for vx in range(3):
                            wz[c, ty + vy, tx + vx] += wc[ty, tx, :, vy, vx]
    return wz.reshape(9, 25, C), beta


def _axis(n_lo):
    """bilinear x2, align_corners=False, along one axis: hi-res position p -> (index a, index b, weight of a), neighbour clamped"""
    p = torch.arange(2 * n_lo)
    k = p // 2
    odd = (p % 2) == 1
    a = torch.where(odd, k, (k - 1).clamp_min(0))
    b = torch.where(odd, (k + 1).clamp_max(n_lo - 1), k)
    wa = torch.where(odd, torch.tensor(0.75, dtype=torch.float64), torch.tensor(0.25, dtype=torch.float64))
    return a, b, wa


def upsample2x(z):
    """[..., h, w] -> [..., 2h, 2w]"""
    h, w = z.shape[-2:]
    ay, by, wy = _axis(h)
    ax, bx, wx = _axis(w)
    rows = z[..., ay, :] * wy[:, None] + z[..., by, :] * (1 - wy)[:, None]
    return rows[..., :, ax] * wx + rows[..., :, bx] * (1 - wx)


def _strip(cls, n):
    return {0: slice(0, 2), 1: slice(0, n), 2: slice(n - 2, n)}[cls]


def lowres_reference(v, w1, b1, w2, b2):
    """v: the block's low-resolution input after any on-load affine / skip / activation, [B][C][h][w] -> [B][1][2h][2w] in fp64"""
    v = v.double()
    B, C, h, w = v.shape
    H, W = 2 * h, 2 * w
    wz, beta = class_sets(w1, b1, w2, b2)
    out = torch.full((B, 1, H, W), float("nan"), dtype=torch.float64)
    rows = {0: slice(0, 1), 1: slice(1, H - 1), 2: slice(H - 1, H)}
    cols = {0: slice(0, 1), 1: slice(1, W - 1), 2: slice(W - 1, W)}
    for cy in range(3):
        for cx in range(3):
            c = 3 * cy + cx
            z = torch.full((B, 25, h, w), float("nan"), dtype=torch.float64)
            sy, sx = _strip(cy, h), _strip(cx, w)
            z[:, :, sy, sx] = torch.einsum("sc,bchw->bshw", wz[c], v[:, :, sy, sx])
            up = torch.nn.functional.pad(upsample2x(z), (2, 2, 2, 2))          # zeros outside the image
            acc = torch.zeros(B, H, W, dtype=torch.float64)
            for s in range(25):
                acc = acc + up[:, s, s // 5:s // 5 + H, s % 5:s % 5 + W]
            out[:, 0, rows[cy], cols[cx]] = (beta[c] + acc)[:, rows[cy], cols[cx]]
    return out
