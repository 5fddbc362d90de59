"""The formulation behind the final block's low-resolution route, pinned on the CPU in fp64 independently of any kernel: nine
(Wz, beta) border-class sets, Z per class on its strip, the zero-padded 25-term sum through the bilinear x2 (util_final_lowres.py)
against conv2d(conv2d(interpolate(v))).  The GPU tests (test_gpu_final_lowres.py) reuse the same reference."""
import pytest
import torch
import torch.nn.functional as F

from util_final_lowres import class_sets, lowres_reference, upsample2x

C = 8


def _weights(seed):
    g = torch.Generator().manual_seed(seed)
    s = (9 * C) ** -0.5
    r = lambda *sh: torch.randn(*sh, generator=g, dtype=torch.float64)  # noqa: E731
    return r(C, C, 3, 3) * s, r(C) * 0.5, r(1, C, 3, 3) * s, r(1)


def _chain(v, w1, b1, w2, b2):
    up = F.interpolate(v, scale_factor=2, mode="bilinear", align_corners=False)
    return F.conv2d(F.conv2d(up, w1, b1, padding=1), w2, b2, padding=1)


@pytest.mark.parametrize("h,w", [(5, 7), (4, 4)])
def test_lowres_reference_matches_the_two_convolutions(h, w):
    w1, b1, w2, b2 = _weights(h * 10 + w)
    v = torch.randn(2, C, h, w, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    got, want = lowres_reference(v, w1, b1, w2, b2), _chain(v, w1, b1, w2, b2)
    assert torch.isfinite(got).all()              # no output reads a border class outside its 2-pixel strip
    err = float((got - want).abs().max())
    print(f"low-res formulation {h}x{w}: max abs error {err:.1e} against conv2d(conv2d(interpolate(v))) in fp64")
    assert err <= 1e-12


def test_upsample_matches_interpolate():
    z = torch.randn(2, 3, 5, 7, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    assert float((upsample2x(z) - F.interpolate(z, scale_factor=2, mode="bilinear", align_corners=False)).abs().max()) <= 1e-14


def test_border_classes_differ_where_they_should():
    """the interior set is the full 5x5 composition; a first-row set has lost conv's tap 0 and so has no weight at sy = 0"""
    w1, b1, w2, b2 = _weights(7)
    wz, beta = class_sets(w1, b1, w2, b2)
    wz = wz.reshape(9, 5, 5, C)
    assert wz[4].abs().min() > 0
    assert torch.equal(wz[1][0], torch.zeros(5, C, dtype=torch.float64)) and wz[1][1:].abs().min() > 0
    assert torch.equal(wz[5][:, 4], torch.zeros(5, C, dtype=torch.float64))
    assert len({round(float(b), 12) for b in beta}) == 9
