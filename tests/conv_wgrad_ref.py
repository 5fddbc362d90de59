"""The weight gradient of a convolution, for the tests of the weight-gradient launcher (test_cpu_wgrad_plan.py, test_gpu_conv_wgrad.py).

Reference: w.grad of F.conv2d(x, w, None, stride, pad).backward(dy) in float64 on the CPU, by autograd, on the unpadded channels, and
db = dy.sum((0, 2, 3)); `abs` / `absdb` are the same two quantities of |x| and |dy|.  Computed once per (geometry, data set, seed) and
handed out read-only.

Bound (no tuned number): every element of dW is a sum of M = B*OH*OW products of fp32 values.  Each product rounds once (relative
2^-24), a sum of M terms in ANY order (tile by tile, wave by wave, fp32 atomics in whatever order they land) makes at most M - 1 more
roundings, each relative to a partial sum that |x| . |dy| bounds, and one more rounding covers a final copy, so to first order

    |got - ref64| <= (M + 2) * 2^-24 * abs64            |db - db64| <= (M + 1) * 2^-24 * absdb64

elementwise.  Every case keeps M <= 2048, where a dropped or doubled pixel (about abs64 / M) stands three orders above the bound.

The device call takes x NHWC with c_pad >= Cin channels; the pad channels hold 7.0 here (a kernel that lets them into dW, or that stores
ci >= Cin, shows), dy NHWC, dW OIHW, and a slab of k*k*Cout*c_pad floats."""
import functools

import torch
import torch.nn.functional as F

U = 2.0 ** -24
PAD_VALUE = 7.0
GENERAL1, GENERAL2, GENERAL4, HALO16, HALO8, TAP64, TAP128, STEM = range(8)
FAMILY_NAMES = ["general<1>", "general<2>", "general<4>", "halo-16", "halo-8x8", "tap-64", "tap-128", "stem"]
GENERAL = (GENERAL1, GENERAL2, GENERAL4)
TILE_PX = {TAP64: 128, TAP128: 64, STEM: 128}          # pixels per tile of the per-tap bodies


def full(geom):
    """(B, Cin, H, W, Cout, k, s, p[, c_pad]) -> the same with c_pad"""
    return tuple(geom) if len(geom) == 9 else tuple(geom) + (geom[1],)


def out_hw(geom):
    B, Cin, H, W, Cout, k, s, p, cs = full(geom)
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def pixels(geom):
    oh, ow = out_hw(geom)
    return geom[0] * oh * ow


# (geometry, family, expectations): direct = stores OIHW itself; multi = tiles_per_wg > 1 and a last workgroup with fewer tiles; plan = exact
# {gx, gy, tpw, n_tiles} where the issue states them.  test_cpu_wgrad_plan.py holds every row to its claims through the plan query.
CASES = [
    ((1, 32, 16, 16, 64, 3, 1, 1), HALO16, dict(direct=True)),
    ((3, 64, 16, 32, 64, 3, 1, 1), HALO16, dict(direct=False, plan=dict(gy=6))),
    ((5, 256, 16, 16, 256, 3, 1, 1), HALO16, dict(direct=False, multi=True, plan=dict(gx=64, tpw=2, gy=3))),
    ((2, 20, 16, 16, 64, 3, 1, 1, 32), HALO16, dict()),                                  # padded channels
    ((1, 64, 8, 8, 64, 3, 1, 1), HALO8, dict(direct=True)),                              # B < 4: one tile, not full
    ((6, 96, 8, 8, 64, 3, 1, 1), HALO8, dict(direct=False, plan=dict(n_tiles=2))),       # last tile holds 2 of 4 images
    ((21, 256, 8, 8, 256, 3, 1, 1), HALO8, dict(direct=False, plan=dict(tpw=2, n_tiles=6))),   # last tile has one image
    ((2, 64, 8, 8, 128, 3, 2, 1), TAP64, dict()),                                        # stride 2
    ((1, 64, 7, 10, 128, 3, 2, 1), TAP64, dict()),                                       # odd, non-square
    ((2, 50, 6, 6, 64, 1, 1, 0, 64), TAP64, dict(direct=True)),                          # padded, direct
    ((1, 64, 1, 130, 64, 1, 1, 0), TAP64, dict(direct=False, plan=dict(n_tiles=2))),     # linear shape, 2-pixel last tile; also run aliased
    ((2, 192, 10, 10, 64, 1, 2, 0), TAP64, dict()),                                      # 1x1 stride 2
    ((1, 64, 16, 16, 64, 8, 2, 3), TAP64, dict()),                                       # 8x8 stride 2 with 64 channels
    ((6, 512, 24, 24, 64, 3, 2, 1), TAP64, dict(direct=False, multi=True, plan=dict(gx=72, n_tiles=7, tpw=2))),
    ((3, 128, 4, 4, 128, 3, 1, 1), TAP128, dict(direct=True)),
    ((1, 128, 1, 300, 384, 1, 1, 0), TAP128, dict(direct=False)),                        # ragged 64-pixel tile, split
    ((36, 256, 4, 4, 256, 3, 1, 1), TAP128, dict(direct=False, multi=True, plan=dict(n_tiles=9, tpw=2))),
    ((1, 5, 32, 32, 64, 8, 2, 3, 8), STEM, dict(direct=False)),                          # Cin = 5 padded to 8
    ((2, 7, 15, 17, 64, 8, 2, 3, 8), STEM, dict(direct=False)),                          # odd map
    ((2, 32, 6, 6, 64, 3, 1, 1), GENERAL2, dict(plan=dict(gy=2))),
    ((1, 96, 6, 6, 64, 3, 1, 1), GENERAL2, dict(plan=dict(gy=1))),
    ((1, 13, 9, 9, 64, 3, 2, 1, 16), GENERAL1, dict()),                                  # padded to 16
    ((1, 3, 12, 12, 64, 8, 2, 3, 4), GENERAL1, dict()),                                  # c_pad = 4
    ((1, 48, 5, 7, 128, 1, 1, 0), GENERAL1, dict()),                                     # 1x1 with 48 channels
]
# general<4> is reached only with the LDS-staged bodies taken away (SBGM_NO_LDS_WGRAD); the geometries test_gpu_backward.py uses for it
GENERAL4_CASES = [(2, 64, 8, 8, 64, 3, 1, 1), (1, 128, 4, 4, 64, 3, 2, 1)]
# calls the launcher refuses: Cout % 64, a c_pad that is neither 4, 8 nor a multiple of 16, c_pad < Cin
REFUSED = [(1, 32, 16, 16, 48, 3, 1, 1), (1, 20, 16, 16, 64, 3, 1, 1, 24), (1, 40, 16, 16, 64, 3, 1, 1, 32)]
ALIAS_REFUSED = (2, 64, 8, 8, 128, 3, 2, 1)            # ws == dw with a 3x3 kernel
# one geometry per family whose one-hot dy must come back bit for bit
ONE_HOT_CASES = [
    ((1, 32, 32, 32, 64, 3, 1, 1), HALO16),
    ((5, 64, 8, 8, 64, 3, 1, 1), HALO8),
    ((2, 64, 16, 16, 128, 3, 2, 1), TAP64),
    ((2, 128, 16, 16, 128, 3, 2, 1), TAP128),
    ((1, 5, 32, 32, 64, 8, 2, 3, 8), STEM),
    ((2, 32, 9, 9, 64, 3, 1, 1), GENERAL2),
]
DATA_SETS = ["centred", "off-centre"]

assert all(pixels(g) <= 2048 for g, _, _ in CASES) and all(pixels(g) <= 2048 for g in GENERAL4_CASES)


def label(geom):
    return "-".join(map(str, geom))


def rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _wgrad64(geom, x, dy):
    B, Cin, H, W, Cout, k, s, p, cs = full(geom)
    w = torch.zeros(Cout, Cin, k, k, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), w, None, s, p).backward(dy.double())
    return w.grad


def _pack(geom, x, dy):
    """fp32 NCHW operands -> the device call's operands and the float64 references"""
    B, Cin, H, W, Cout, k, s, p, cs = full(geom)
    x_nhwc = torch.full((B, H, W, cs), PAD_VALUE)
    x_nhwc[..., :Cin] = x.permute(0, 2, 3, 1)
    return dict(x=x_nhwc, dy=dy.permute(0, 2, 3, 1).contiguous(), ref=_wgrad64(geom, x, dy), abs=_wgrad64(geom, x.abs(), dy.abs()),
                db=dy.double().sum((0, 2, 3)), absdb=dy.double().abs().sum((0, 2, 3)), M=pixels(geom))


@functools.lru_cache(maxsize=None)
def case(geom, data="centred", seed=0):
    """x NHWC [B, H, W, c_pad] (pad channels 7.0), dy NHWC, and float64 ref / abs [Cout, Cin, k, k], db / absdb [Cout]; read-only"""
    B, Cin, H, W, Cout, k, s, p, cs = full(geom)
    oh, ow = out_hw(geom)
    x, dy = rnd(B, Cin, H, W, seed=1000 * seed + 1), rnd(B, Cout, oh, ow, seed=1000 * seed + 2)
    if data == "off-centre":
        x, dy = x + 3.0, 0.5 * dy + 1.5
    else:
        assert data == "centred"
    return _pack(geom, x, dy)


def one_hot_pixels(oh, ow):
    """the four corners, one pixel on each edge, and an interior pixel of each (row, column) parity (as conv_dgrad_ref.one_hot_pixels)"""
    assert oh >= 8 and ow >= 8
    ym, xm = oh // 2, ow // 2
    return [(0, 0), (0, ow - 1), (oh - 1, 0), (oh - 1, ow - 1), (0, xm + 1), (oh - 1, xm - 2), (ym - 2, 0), (ym + 1, ow - 1),
            (ym, xm), (ym - 2, xm - 1), (ym - 1, xm + 2), (ym + 1, xm - 3)]


@functools.lru_cache(maxsize=None)
def one_hot_case(geom):
    """dy zero except the one-hot pixels, each on its own output channel with a power of two, spread over the first, the middle and the
    last image: every element of dW[co] is one x value times a power of two (or zero), so the float64 reference IS an fp32 number and
    sums that only add zeros must reproduce it bit for bit"""
    B, Cin, H, W, Cout, k, s, p, cs = full(geom)
    oh, ow = out_hw(geom)
    px = one_hot_pixels(oh, ow)
    assert {(y % 2, x % 2) for y, x in px[8:]} == {(0, 0), (0, 1), (1, 0), (1, 1)} and len(set(px)) == len(px) <= Cout
    x = rnd(B, Cin, H, W, seed=77)
    dy = torch.zeros(B, Cout, oh, ow)
    images = [0, B - 1, B // 2]
    for i, (yy, xx) in enumerate(px):
        dy[images[i % 3], (5 * i + 3) % Cout, yy, xx] = (0.5, 1.0, 2.0)[(i // 3) % 3]
    assert int((dy != 0).sum()) == len(px) and len({int(c) for c in dy.nonzero()[:, 1]}) == len(px)
    assert B == 1 or int((dy[B - 1] != 0).sum()) >= 4
    c = _pack(geom, x, dy)
    c["exact"], c["exact_db"] = c["ref"].float(), c["db"].float()
    assert torch.equal(c["exact"].double(), c["ref"]) and torch.equal(c["exact_db"].double(), c["db"]) and float(c["ref"].abs().max()) > 0.5
    return c


def bounds(c):
    """elementwise (bound on |dW - ref64|, bound on |db - db64|) of a case"""
    return (c["M"] + 2) * U * c["abs"], (c["M"] + 1) * U * c["absdb"]


def ratio(got, ref, bound):
    """elementwise |got - ref| / bound in float64 (0 where both vanish, inf where only the bound does); NaN where got is not finite"""
    err = (got.double() - ref).abs()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return torch.where(torch.isfinite(got), r, torch.full_like(r, float("nan")))


def worst(r):
    """(max ratio, index of it) with NaN counting as the worst"""
    flat = torch.nan_to_num(r, nan=float("inf")).flatten()
    i = int(flat.argmax())
    idx = []
    for n in reversed(r.shape):
        idx.append(i % n)
        i //= n
    return float(r.flatten()[int(flat.argmax())]), tuple(reversed(idx))
