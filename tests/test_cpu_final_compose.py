"""The identity behind the composed final block (csrc/conv_final.hip), in fp64 with torch on the CPU: the final DecoderBlock has
nothing non-linear between its two convolutions, so conv(conv_up(up(x))) equals one 3x3 convolution to the 9 taps of `conv`
followed by a 9-point gather that treats taps outside the image as zero."""
import pytest
import torch
import torch.nn.functional as F


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def compose(w1, b1, w2):
    """Wc [9][ci][3][3] = sum_co w2[0][co][tap] w1[co][ci][v][b],  bc [9] = sum_co w2[0][co][tap] b1[co]"""
    w2t = w2[0].reshape(w2.shape[1], 9)
    return torch.einsum("ot,ocvb->tcvb", w2t, w1), w2t.t() @ b1


def gather(d, b2):
    """out[o] = b2 + sum_tap d[tap][o + tap - 1], d = 0 outside the image"""
    H, W = d.shape[-2:]
    dp = F.pad(d, (1, 1, 1, 1))
    out = sum(dp[:, kh * 3 + kw, kh:kh + H, kw:kw + W] for kh in range(3) for kw in range(3))
    return out[:, None] + b2.view(1, 1, 1, 1)


@pytest.mark.parametrize("B,C,h,w", [(2, 64, 16, 16), (1, 64, 8, 24), (2, 16, 4, 4), (1, 32, 5, 7)])
def test_composed_block_equals_the_two_convolutions(B, C, h, w):
    x = rnd(B, C, h, w)
    w1, b1 = rnd(C, C, 3, 3, seed=1) / (3 * C ** 0.5), rnd(C, seed=2)
    w2, b2 = rnd(1, C, 3, 3, seed=3) / (3 * C ** 0.5), rnd(1, seed=4)
    up = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
    want = F.conv2d(F.conv2d(up, w1, b1, padding=1), w2, b2, padding=1)
    wc, bc = compose(w1, b1, w2)
    got = gather(F.conv2d(up, wc, bc, padding=1), b2)
    err = float((got - want).abs().max() / want.abs().max())
    print(f"composed final block {B}x{C}x{h}x{w}: max-rel {err:.2e} in fp64")
    assert got.shape == want.shape and err < 1e-12


def test_bias_term_differs_on_the_border_ring():
    """zero input: b2 + the sum of bc over the taps that fall inside the image, so the border ring differs from the interior"""
    C, H = 16, 6
    w1, b1, w2, b2 = rnd(C, C, 3, 3, seed=5), rnd(C, seed=6), rnd(1, C, 3, 3, seed=7), rnd(1, seed=8)
    z = torch.zeros(1, C, H, H, dtype=torch.float64)
    want = F.conv2d(F.conv2d(z, w1, b1, padding=1), w2, b2, padding=1)
    wc, bc = compose(w1, b1, w2)
    got = gather(F.conv2d(z, wc, bc, padding=1), b2)
    assert float((got - want).abs().max()) < 1e-12 * float(want.abs().max())
    assert abs(float(got[0, 0, 2, 2] - (b2 + bc.sum()))) < 1e-12 * float(want.abs().max())
    assert abs(float(got[0, 0, 0, 0] - got[0, 0, 2, 2])) > 1e-3
