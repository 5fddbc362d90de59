"""The data gradient of a convolution, for the tests of the data-gradient operator (test_cpu_conv_tiles.py, test_gpu_conv_dgrad.py).

Reference: x.grad of F.conv2d(x, w, None, stride, pad) in float64 on the CPU, by autograd (no hand-written transposed convolution),
plus the residual where the call carries one.  Computed once per geometry and handed out read-only.

The device call: ConvFn.backward (train_graph.py) computes dx by running the FORWARD kernels on dy with the transposed, 180-degree
flipped weight image: stride 1, pad = k - 1 - pad, the forward Cout as input channels and the forward Cin as output channels, an
explicit output size (H, W), and for a stride-2 layer in_dil = 2 (dy read through a zero-inserted grid).  dgrad_call derives that call
from the forward geometry (B, Cin, H, W, Cout, k, s, p), so no test restates it by hand."""
import functools
import math

import torch
import torch.nn.functional as F

# forward geometries (B, Cin, H, W, Cout, k, s, p) whose data gradient the GPU test runs on every candidate tile
CASES = [
    (2, 64, 16, 16, 64, 3, 1, 1),     # every family takes part (W % 16 == 0)
    (1, 256, 4, 16, 64, 3, 1, 1),     # 16 channel stages; 4-row map
    (1, 64, 34, 32, 32, 3, 1, 1),     # ragged tile rows; Cin != Cout
    (2, 64, 8, 8, 128, 3, 2, 1),      # in_dil = 2, even size: the output row past the dilated grid must read zeros
    (1, 64, 7, 10, 128, 3, 2, 1),     # in_dil = 2, odd H, non-square: out_h / out_w decide the size
    (2, 192, 10, 10, 64, 1, 2, 0),    # 1x1 stride-2 shortcut: three of every four output pixels are pure zero reads
    (1, 32, 15, 15, 64, 8, 2, 3),     # the 8x8 / stride 1 / pad 4 instantiation (the stem's data gradient on an odd map)
]
PHASE_CASE = (1, 32, 16, 16, 64, 8, 2, 3)    # the stem's data gradient as a 5x5 / s1 / p2 phase operator + depth-to-space
# The localised check.  The stride-1 geometry has 32 input channels: a data gradient of 16 output channels (forward Cin = 16) is no
# call of the training path (ConvFn.backward refuses it, and sbgm_conv2d_tune / _tiles refuse Cout % 32 != 0), see REFUSED_CASE.
LOCALISED_CASES = [(1, 32, 32, 32, 32, 3, 1, 1), (1, 32, 16, 16, 32, 3, 2, 1)]
REFUSED_CASE = (1, 16, 32, 32, 32, 3, 1, 1)

FAMILIES = {(0, 0): "implicit-GEMM", (1, 0): "1-D Winograd", (0, 1): "LDS-staged direct", (0, 2): "LDS-staged direct",
            (1, 1): "LDS-staged Winograd", (1, 2): "LDS-staged Winograd", (2, 1): "2-D Winograd F(2x2,3x3)",
            (2, 2): "2-D Winograd F(2x2,3x3)", (2, 3): "persistent 2-D Winograd F(2x2,3x3)", (3, 1): "space-to-depth Winograd F(2x2,4x4)"}


def family(tile):
    """kernel family of a tile[6] = {tile_co, tile_px, splits, waves_per_tile, winograd kind, LDS kind}"""
    return FAMILIES[(tile[4], tile[5])]


def image_of(tile):
    """the weight image the tile's family reads: 'g' implicit GEMM, 'w' Winograd F(2,3), 'd' F(2x2,3x3)"""
    return "d" if tile[4] == 2 else "w" if tile[4] == 1 else "g"


def args_tile(tile):
    """tile[6] -> (tile_co, tile_px, splits, waves_per_tile, winograd bits) of sbgm_conv_args (include/sbgm_hip.h): bit 0 F(2,3), bit 1
    LDS-staged, bit 2 two stage buffers, bit 3 F(2x2,3x3), bit 4 its persistent form"""
    co, px, splits, waves, wino, lds = tile
    if wino == 2:
        return co, 0, 0, waves, 8 | (16 if lds == 3 else 4 if lds == 2 else 0)
    return co, px, splits, waves, wino | (2 if lds else 0) | (4 if lds == 2 else 0)


def dgrad_call(geom):
    """the sbgm_conv_args geometry of the data gradient of forward geometry (B, Cin, H, W, Cout, k, s, p), as ConvFn.backward sets it, and
    which Winograd images that call brings (train_graph._wino_ok / _w2d_ok)"""
    B, Cin, H, W, Cout, k, s, p = geom
    assert s in (1, 2)
    oh, ow = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    in_dil = 2 if s == 2 else 0
    w3 = k == 3 and k - 1 - p == 1 and not in_dil and Cout % 16 == 0 and Cin % 32 == 0
    return dict(B=B, H=oh, W=ow, c_pad=Cout, Cout=Cin, k=k, stride=1, pad=k - 1 - p, in_dil=in_dil, out_h=H, out_w=W,
                wino=w3 and ow % 2 == 0, w2d=w3 and ow % 16 == 0 and oh % 2 == 0)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return torch.randn(*shape, generator=g) * scale


def _grad64(geom, w, dy):
    B, Cin, H, W, Cout, k, s, p = geom
    x = torch.zeros(B, Cin, H, W, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, w.double(), None, s, p).backward(dy.double())
    return x.grad


@functools.lru_cache(maxsize=None)
def case(geom):
    """fp32 operands (w OIHW, dy and res NCHW) and the float64 gradients ref (no residual) and ref_res (+ res); read-only"""
    B, Cin, H, W, Cout, k, s, p = geom
    w = rnd(Cout, Cin, k, k, seed=1, scale=1.0 / math.sqrt(Cin * k * k))
    oh, ow = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    dy, res = rnd(B, Cout, oh, ow, seed=5), rnd(B, Cin, H, W, seed=6)
    ref = _grad64(geom, w, dy)
    return dict(w=w, dy=dy, res=res, ref=ref, ref_res=ref + res.double())


def one_hot_pixels(oh, ow):
    """the four corners, one pixel on each edge, and an interior pixel of each (row, column) parity"""
    assert oh >= 8 and ow >= 8
    ym, xm = oh // 2, ow // 2                                        # the last four: rows and columns 1 .. size - 2, all four parities
    return [(0, 0), (0, ow - 1), (oh - 1, 0), (oh - 1, ow - 1), (0, xm + 1), (oh - 1, xm - 2), (ym - 2, 0), (ym + 1, ow - 1),
            (ym, xm), (ym - 2, xm - 1), (ym - 1, xm + 2), (ym + 1, xm - 3)]


@functools.lru_cache(maxsize=None)
def localised_case(geom):
    """dy zero except one-hot pixels (distinct channels, values near 1): dx must reproduce the flipped stencil around each"""
    B, Cin, H, W, Cout, k, s, p = geom
    w = rnd(Cout, Cin, k, k, seed=9, scale=0.3)
    oh, ow = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    pixels = one_hot_pixels(oh, ow)
    assert {(y % 2, x % 2) for y, x in pixels[8:]} == {(0, 0), (0, 1), (1, 0), (1, 1)} and len(pixels) <= Cout
    assert all(1 <= y <= oh - 2 and 1 <= x <= ow - 2 for y, x in pixels[8:]) and len(set(pixels)) == len(pixels)
    dy = torch.zeros(B, Cout, oh, ow)
    for i, (yy, xx) in enumerate(pixels):
        dy[0, (5 * i + 3) % Cout, yy, xx] = 1.0 + 0.01 * i
    assert int((dy != 0).sum()) == len(pixels) and len({int(c) for c in dy.nonzero()[:, 1]}) == len(pixels)
    return dict(w=w, dy=dy, ref=_grad64(geom, w, dy))
