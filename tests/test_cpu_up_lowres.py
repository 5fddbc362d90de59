"""The formulation behind the decoder's low-resolution conv_up route, pinned on the CPU in fp64 independently of any kernel: the tap
mix on the low-res map, the clamped bilinear gather and the padding rule of the high-res map (util_up_lowres.py) against
conv2d(interpolate(x)), followed by GroupNorm.  The GPU tests (test_gpu_up_lowres.py) reuse the same statement."""
import pytest
import torch
import torch.nn.functional as F

from util_up_lowres import group_norm, taps_weight, up_lowres_reference, upsample2x

C, G = 8, 2
BOUND = 1e-12


def _operands(seed, h, w):
    g = torch.Generator().manual_seed(seed)
    r = lambda *sh: torch.randn(*sh, generator=g, dtype=torch.float64)  # noqa: E731
    return r(2, C, h, w), r(C, C, 3, 3) * (9 * C) ** -0.5, r(C) * 0.5, r(C).abs() + 0.5, r(C)


def _relerr(got, want):
    return float((got - want).abs().max() / want.abs().max())


@pytest.mark.parametrize("h,w", [(1, 1), (2, 3), (3, 5), (4, 4), (8, 8)])
def test_formulation_matches_conv_of_interpolate(h, w):
    x, wt, b, gamma, beta = _operands(10 * h + w, h, w)
    up = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
    want = F.conv2d(up, wt, b, padding=1)
    err = _relerr(up_lowres_reference(x, wt, b), want)
    err_n = _relerr(up_lowres_reference(x, wt, b, G, gamma, beta), F.group_norm(want, G, gamma, beta, eps=1e-5))
    print(f"low-res conv_up {h}x{w}: max-rel {err:.1e} raw, {err_n:.1e} with GroupNorm against conv2d(interpolate(x)) in fp64")
    assert err <= BOUND and err_n <= BOUND


def test_upsample_and_group_norm_match_torch():
    z = torch.randn(2, 3, 5, 7, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    assert float((upsample2x(z) - F.interpolate(z, scale_factor=2, mode="bilinear", align_corners=False)).abs().max()) <= 1e-14
    v = torch.randn(2, C, 4, 6, generator=torch.Generator().manual_seed(2), dtype=torch.float64) + 3.0
    assert float((group_norm(v, G) - F.group_norm(v, G, eps=1e-5)).abs().max()) <= 1e-12


def test_taps_weight_is_a_copy_of_every_element():
    w = torch.arange(C * C * 9, dtype=torch.float64).reshape(C, C, 3, 3)
    w1 = taps_weight(w)
    assert w1.shape == (9 * C, C)
    for tap, co, ci in ((0, 0, 0), (4, 3, 5), (8, C - 1, C - 1), (5, 2, 7)):
        assert w1[tap * C + co, ci] == w[co, ci, tap // 3, tap % 3]
    assert torch.equal(w1.flatten().sort().values, w.flatten())


def test_a_tap_outside_the_high_res_map_is_skipped():
    """zero bias, constant input 1 and a weight of ones: an interior output sums 9 taps x C, a corner 4 taps x C: up(Z) of a constant
    is that constant, so only the padding rule decides"""
    x, w, b = torch.ones(1, C, 3, 3, dtype=torch.float64), torch.ones(C, C, 3, 3, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    out = up_lowres_reference(x, w, b)
    assert float(out[0, 0, 2, 2]) == 9 * C and float(out[0, 0, 0, 0]) == 4 * C and float(out[0, 0, 0, 3]) == 6 * C
    assert float(out[0, 0, 5, 5]) == 4 * C
