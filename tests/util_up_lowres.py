"""fp64 statement of a small-map decoder block's conv_up at low resolution (csrc/conv_uplow.hip), in plain torch on the CPU:

    Z_tap[co] = sum_ci W[co][ci][k][l] x[ci]                                                 on the low-res map, tap = 3 k + l
    out[co][o] = b[co] + sum_{tap, o + tap - 1 inside the HIGH-res map} up(Z_tap)[co][o + tap - 1]

`up` is bilinear x2 with align_corners=False, the neighbour clamped at the map edge; a tap whose intermediate pixel lies outside the
high-res map is skipped (the zero padding of conv_up's input).  Optionally followed by GroupNorm."""
import torch


def taps_weight(w):
    """OIHW [C][C][3][3] -> the mix's 1x1 weight [9C][C], row tap * C + co"""
    c = w.shape[0]
    return w.permute(2, 3, 0, 1).reshape(9 * c, c)


def _axis(n_lo):
    """hi-res position p -> (index a, index b, weight of a): an even p = 2j reads 0.25 Z[j-1] + 0.75 Z[j], an odd one 0.75 Z[j] + 0.25 Z[j+1]"""
    p = torch.arange(2 * n_lo)
    j = p // 2
    odd = (p % 2) == 1
    a = torch.where(odd, j, (j - 1).clamp_min(0))
    b = torch.where(odd, (j + 1).clamp_max(n_lo - 1), j)
    wa = torch.where(odd, torch.tensor(0.75, dtype=torch.float64), torch.tensor(0.25, dtype=torch.float64))
    return a, b, wa


def upsample2x(z):
    """[..., h, w] -> [..., 2h, 2w]"""
    h, w = z.shape[-2:]
    ay, by, wy = _axis(h)
    ax, bx, wx = _axis(w)
    rows = z[..., ay, :] * wy[:, None] + z[..., by, :] * (1 - wy)[:, None]
    return rows[..., :, ax] * wx + rows[..., :, bx] * (1 - wx)


def group_norm(v, groups, gamma=None, beta=None, eps=1e-5):
    """GroupNorm over [B][C][H][W] in fp64: biased variance per (sample, group), then the per-channel affine"""
    B, C, H, W = v.shape
    g = v.reshape(B, groups, -1)
    mean = g.mean(dim=2, keepdim=True)
    var = ((g - mean) ** 2).mean(dim=2, keepdim=True)
    out = ((g - mean) / torch.sqrt(var + eps)).reshape(B, C, H, W)
    if gamma is not None:
        out = out * gamma.double()[None, :, None, None] + beta.double()[None, :, None, None]
    return out


def up_lowres_reference(x, w, b, groups=0, gamma=None, beta=None, eps=1e-5):
    """x: low-res [B][C][h][w] -> conv_up(up(x)) (+ GroupNorm when groups > 0), [B][C][2h][2w] in fp64"""
    x, w, b = x.double(), w.double(), b.double()
    B, C, h, wd = x.shape
    H, W = 2 * h, 2 * wd
    z = torch.einsum("nc,bchw->bnhw", taps_weight(w), x).reshape(B, 9, C, h, wd)      # the tap mix on the low-res map
    up = torch.nn.functional.pad(upsample2x(z), (1, 1, 1, 1))                        # zeros outside the high-res map
    out = b[None, :, None, None].expand(B, C, H, W).clone()
    for k in range(3):
        for l in range(3):
            out = out + up[:, 3 * k + l, :, k:k + H, l:l + W]
    return group_norm(out, groups, gamma, beta, eps) if groups else out
