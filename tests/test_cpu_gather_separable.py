"""The two-pass (separable) form of the low-resolution gathers (csrc/conv_uplow.hip), restated in fp64 torch on the CPU.

The bilinear x2 is a tensor product up = Uy (x) Ux, so the K x K gather through it splits into a horizontal pass over the LOW-res rows
and a vertical pass over the result:

    R[ky][j][ox] = sum_kx in_x(ox + kx - r) (wx Z[ky, kx][j][xa] + (1 - wx) Z[ky, kx][j][xb])        low-res row j, high-res column ox
    out[oy][ox]  = b + sum_ky in_y(oy + ky - r) (wy R[ky][ya][ox] + (1 - wy) R[ky][yb][ox])          r = (K - 1) / 2

with (a, b, weight) the two clamped low-res neighbours of a high-res position and in(p) false where p lies outside the high-res map
(the zero padding of the convolution's input: that tap is skipped).  It must equal the 2-D statements the kernels are tested against:
tests/util_up_lowres.py (3 x 3) and tests/util_final_lowres.py (5 x 5 with nine border classes) on 1x1, 2x3 and 5x7 maps."""
import pytest
import torch

import util_final_lowres as FL
import util_up_lowres as UL

MAPS = [(1, 1), (2, 3), (5, 7)]
BOUND = 1e-12


def axis(n_lo):
    """high-res position p -> (first neighbour, second neighbour, weight of the first): an even p = 2j reads 0.25 Z[j-1] + 0.75 Z[j],
    an odd one 0.75 Z[j] + 0.25 Z[j+1], the neighbour clamped at the map edge"""
    out = []
    for p in range(2 * n_lo):
        j = p // 2
        out.append((j, min(j + 1, n_lo - 1), 0.75) if p % 2 else (max(j - 1, 0), j, 0.25))
    return out


def separable_gather(z, K):
    """z: [..., K*K, h, w] (tap = K ky + kx) -> [..., 2h, 2w], the sum over the taps of the upsampled, shifted, zero-padded tap maps"""
    h, w = z.shape[-2:]
    H, W, r = 2 * h, 2 * w, (K - 1) // 2
    z = z.double().reshape(*z.shape[:-3], K, K, h, w)
    ax, ay = axis(w), axis(h)
    R = torch.zeros(*z.shape[:-4], K, h, W, dtype=torch.float64)
    for ox in range(W):
        for kx in range(K):
            p = ox + kx - r
            if not 0 <= p < W:
                continue                                   # a skipped tap: outside the high-res map
            a, b, wa = ax[p]
            R[..., :, :, ox] += wa * z[..., :, kx, :, a] + (1 - wa) * z[..., :, kx, :, b]
    out = torch.zeros(*z.shape[:-4], H, W, dtype=torch.float64)
    for oy in range(H):
        for ky in range(K):
            p = oy + ky - r
            if not 0 <= p < H:
                continue
            a, b, wa = ay[p]
            out[..., oy, :] += wa * R[..., ky, a, :] + (1 - wa) * R[..., ky, b, :]
    return out


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed + sum(shape)), dtype=torch.float64)


def relerr(got, want):
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-30))


def up_separable(x, w, b):
    B, C, h, wd = x.shape
    z = torch.einsum("nc,bchw->bnhw", UL.taps_weight(w.double()), x.double()).reshape(B, 9, C, h, wd)
    return separable_gather(z.transpose(1, 2), 3) + b.double()[None, :, None, None]


@pytest.mark.parametrize("hw", MAPS, ids=lambda v: "x".join(map(str, v)))
@pytest.mark.parametrize("groups", [0, 4], ids=["raw", "groupnorm"])
def test_3x3_two_pass_equals_the_2d_reference(hw, groups):
    c = 8
    x, w, b = rnd(2, c, *hw, seed=1), rnd(c, c, 3, 3, seed=2) / 6, rnd(c, seed=3)
    gamma, beta = rnd(c, seed=4).abs() + 0.5, rnd(c, seed=5)
    want = UL.up_lowres_reference(x, w, b, groups, gamma if groups else None, beta if groups else None)
    got = up_separable(x, w, b)
    if groups:
        got = UL.group_norm(got, groups, gamma, beta)
    assert got.shape == want.shape
    assert relerr(got, want) < BOUND


@pytest.mark.parametrize("hw", [(1, 1), (2, 3), (3, 5)], ids=lambda v: "x".join(map(str, v)))
def test_3x3_one_hot_corners_and_edges(hw):
    """a single low-res pixel at each corner and at an edge midpoint: clamped neighbours and skipped taps, position by position"""
    h, w = hw
    pts = sorted({(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 2), (h // 2, 0)})
    c = 4
    wt, b = rnd(c, c, 3, 3, seed=7), torch.zeros(c, dtype=torch.float64)
    x = torch.zeros(len(pts), c, h, w, dtype=torch.float64)
    for i, (py, px) in enumerate(pts):
        x[i, i % c, py, px] = 1.0
    want = UL.up_lowres_reference(x, wt, b)
    got = up_separable(x, wt, b)
    for i in range(len(pts)):
        assert relerr(got[i], want[i]) < BOUND, pts[i]


@pytest.mark.parametrize("hw", MAPS, ids=lambda v: "x".join(map(str, v)))
def test_5x5_two_pass_equals_the_final_blocks_reference(hw):
    """the final block: nine border classes, each formed on its 2-pixel strips only (NaN elsewhere, as the kernels store them); the
    two-pass form reads, for the outputs of a class, nothing outside that class's strips either"""
    c = 6
    h, w = hw
    H, W = 2 * h, 2 * w
    v = rnd(2, c, h, w, seed=11)
    w1, b1, w2, b2 = rnd(c, c, 3, 3, seed=12) / 5, rnd(c, seed=13), rnd(1, c, 3, 3, seed=14) / 5, rnd(1, seed=15)
    want = FL.lowres_reference(v, w1, b1, w2, b2)
    wz, beta = FL.class_sets(w1, b1, w2, b2)
    got = torch.full((2, 1, H, W), float("nan"), dtype=torch.float64)
    rows = {0: slice(0, 1), 1: slice(1, H - 1), 2: slice(H - 1, H)}
    cols = {0: slice(0, 1), 1: slice(1, W - 1), 2: slice(W - 1, W)}
    strip = lambda cls, n: {0: slice(0, 2), 1: slice(0, n), 2: slice(max(n - 2, 0), n)}[cls]  # noqa: E731
    for cy in range(3):
        for cx in range(3):
            k = 3 * cy + cx
            z = torch.full((2, 25, h, w), float("nan"), dtype=torch.float64)
            sy, sx = strip(cy, h), strip(cx, w)
            z[:, :, sy, sx] = torch.einsum("sc,bchw->bshw", wz[k], v[:, :, sy, sx])
            # run on the whole map twice: with the part outside the strips zeroed (the values) and poisoned (what was read)
            out = separable_gather(torch.nan_to_num(z, nan=0.0), 5) + beta[k]
            poisoned = separable_gather(z, 5)
            sel = (slice(None), rows[cy], cols[cx])
            assert torch.isfinite(poisoned[sel]).all()          # the class's outputs read inside its strips only
            got[:, 0, rows[cy], cols[cx]] = out[sel]
    assert torch.isfinite(want).all() and torch.isfinite(got).all()
    assert relerr(got, want) < BOUND
