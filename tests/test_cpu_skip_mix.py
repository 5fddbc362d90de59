"""Host side of the skip formed inside the final mix (csrc/conv_final.hip, skip_from_x): conv1 splits exactly into its share over x
and its share over the condition channels, and the packed image with the kernel's (k step, quarter) -> tap order reproduces the x share.
The kernels run in test_gpu_skip_mix.py."""
import pytest
import torch

from sbgm_danra_amd import _native as N
from util_skip_mix import conv1, conv1_x_by_steps, pack_w1x, skip_parts, tap_of


@pytest.mark.parametrize("n_cond", [1, 4])
def test_conv1_splits_into_x_share_and_condition_share(n_cond):
    g = torch.Generator().manual_seed(7 + n_cond)
    w1 = torch.randn(64, 1 + n_cond, 8, 8, generator=g, dtype=torch.float64) * (64 * (1 + n_cond)) ** -0.5
    x = torch.randn(2, 1, 24, 48, generator=g, dtype=torch.float64)
    cond = torch.randn(2, n_cond, 24, 48, generator=g, dtype=torch.float64)
    tb0 = torch.randn(2, 64, generator=g, dtype=torch.float64)
    whole, xpart, cpart = skip_parts(w1, x, cond, tb0)
    split = xpart + cpart + tb0[:, :, None, None]
    err = float((whole - split).abs().max() / whole.abs().max())
    print(f"conv1(x || cond) + tb0 against its two shares, {n_cond} condition channels: max-rel {err:.2e}")
    assert whole.shape == (2, 64, 12, 24) and err <= 1e-13


def test_tap_order_covers_the_filter_once():
    taps = [tap_of(s, kq) for s in range(16) for kq in range(4)]
    assert sorted(taps) == [(v, u) for v in range(8) for u in range(8)]
    assert tap_of(0, 3) == (0, 3) and tap_of(1, 0) == (0, 4) and tap_of(2, 1) == (1, 1) and tap_of(15, 3) == (7, 7)


@pytest.mark.parametrize("shape", [(24, 48), (40, 56), (8, 8)])
def test_packed_image_and_tap_order_reproduce_conv1_x_on_integers(shape):
    """integer data: every product and sum is exact in fp32, so a permuted k order or a wrong tap shows as a non-zero difference (on
    smooth data it would hide in the rounding); the map edges exercise the row / column masks"""
    g = torch.Generator().manual_seed(3)
    w1 = torch.randint(-4, 5, (64, 3, 8, 8), generator=g).float()
    x = torch.randint(-8, 9, (2, 1) + shape, generator=g).float()
    img = pack_w1x(w1)
    assert img.shape == (16, 64, 4) and img.numel() == 64 * 64
    assert float(img[5, 17, 2]) == float(w1[17, 0, 2, 6])             # k step 5, quarter 2: tap 22 = row 2, column 6
    got = conv1_x_by_steps(img, x)
    want = conv1(w1[:, :1], x)
    assert torch.equal(got, want)
    bad = img.clone()
    bad[[2, 3]] = bad[[3, 2]]                                         # two k steps swapped: the check must notice
    assert not torch.equal(conv1_x_by_steps(bad, x), want)


def test_the_library_declares_the_entries():
    assert "sbgm_skip_mix_pack" in N.SIGNATURES and "sbgm_final_lowres_skip_fwd" in N.SIGNATURES
    assert "sbgm_skip_mix_packed_numel" in N.SIGNATURES
