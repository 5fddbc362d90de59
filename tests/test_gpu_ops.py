"""Per-kernel parity, through the C ABI, against plain PyTorch-CPU fp32 references of the same op.
Tolerance: 1e-4 max-rel (north_star), most ops land at ~1e-6."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from sbgm_danra_amd import _native as N  # noqa: E402

DEV = "cuda"


def lib():
    return N.lib()


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def relerr(got, want):
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-30))


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return torch.randn(*shape, generator=g) * scale


def pad_c(c):
    return 4 if c <= 4 else 8 if c <= 8 else (c + 15) // 16 * 16


def run_conv(x, w, stride, pad, scale=None, bias=None, tbias=None, res=None, relu=False, after=False, tile=(0, 0), splits=0, wpt=0,
             gelu=False):
    B, Cin, H, W = x.shape
    Cout, _, KH, KW = w.shape
    cp = pad_c(Cin)
    xp = torch.zeros(B, H, W, cp)
    xp[..., :Cin] = nhwc(x)
    xd, wd = xp.to(DEV), w.contiguous().to(DEV)
    packed = torch.empty(lib().sbgm_conv_packed_numel(Cout, KH, KW, cp), device=DEV)
    N.check(lib().sbgm_conv_pack_weight(wd.data_ptr(), packed.data_ptr(), Cout, Cin, KH, KW, cp, N.stream()))
    OH, OW = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
    out = torch.empty(B, OH, OW, Cout, device=DEV)
    dv = lambda t: None if t is None else t.contiguous().to(DEV)  # noqa: E731
    sc, bi, tb, rs = dv(scale), dv(bias), dv(tbias), dv(None if res is None else nhwc(res))
    ws = torch.empty(max(1, splits) * out.numel(), device=DEV)
    a = N.ConvArgs(xd.data_ptr(), packed.data_ptr(), out.data_ptr(), N.ptr(sc), N.ptr(bi), N.ptr(tb), N.ptr(rs), B, H, W, cp,
                   Cout, KH, KW, stride, pad, N.GELU if gelu else (N.RELU if relu else N.NONE), int(after), tile[0], tile[1], splits, wpt,
                   0, 0, 0, 0, ws.data_ptr(), ws.numel())
    N.check(lib().sbgm_conv2d_fwd(C.byref(a), N.stream()))
    torch.cuda.synchronize()
    return nchw(out.cpu())


def ref_conv(x, w, stride, pad, scale=None, bias=None, tbias=None, res=None, relu=False, after=False):
    y = F.conv2d(x, w, None, stride, pad)
    if scale is not None:
        y = y * scale.view(1, -1, 1, 1)
    if bias is not None:
        y = y + bias.view(1, -1, 1, 1)
    if tbias is not None and not after:
        y = y + tbias[:, :, None, None]
    if res is not None:
        y = y + res
    if relu:
        y = F.relu(y)
    if tbias is not None and after:
        y = y + tbias[:, :, None, None]
    return y


CONV_CASES = [
    # (B, Cin, H, W, Cout, K, stride, pad)
    (2, 2, 32, 32, 64, 8, 2, 3),     # stem conv1, 4-channel padded mode
    (1, 7, 32, 32, 64, 8, 2, 3),     # stem conv1, 8-channel padded mode
    (1, 13, 32, 32, 64, 8, 2, 3),    # stem conv1, 16-channel padded mode
    (2, 64, 16, 16, 64, 8, 2, 3),    # stem conv2
    (2, 64, 8, 8, 64, 3, 1, 1),      # layer1
    (2, 64, 8, 8, 128, 3, 2, 1),     # layer2.0.conv1
    (2, 64, 8, 8, 128, 1, 2, 0),     # downsample
    (3, 128, 4, 4, 128, 3, 1, 1),
    (1, 256, 2, 2, 512, 3, 2, 1),    # 2x2 -> 1x1 (64^2 input deepest stage), M < 16
    (2, 64, 16, 20, 64, 3, 1, 1),    # non-square
    (1, 256, 1, 24, 768, 1, 1, 0),   # linear: 24 tokens, C=256 -> 3C
]


@pytest.mark.parametrize("case", CONV_CASES)
@pytest.mark.parametrize("tile", [(4, 4), (4, 2), (4, 1), (2, 4), (2, 2), (2, 1)])
def test_conv_tiles(case, tile):
    B, Cin, H, W, Cout, K, s, p = case
    x, w = rnd(B, Cin, H, W), rnd(Cout, Cin, K, K, seed=1, scale=1.0 / math.sqrt(Cin * K * K))
    got = run_conv(x, w, s, p, tile=tile)
    assert relerr(got, ref_conv(x, w, s, p)) < 2e-5


@pytest.mark.parametrize("case", CONV_CASES)
@pytest.mark.parametrize("wpt", [2, 4])
@pytest.mark.parametrize("tile", [(4, 4), (4, 1), (2, 2)])
def test_conv_in_workgroup_splitk(case, wpt, tile):
    B, Cin, H, W, Cout, K, s, p = case
    x, w = rnd(B, Cin, H, W), rnd(Cout, Cin, K, K, seed=1, scale=1.0 / math.sqrt(Cin * K * K))
    got = run_conv(x, w, s, p, tile=tile, wpt=wpt)
    assert relerr(got, ref_conv(x, w, s, p)) < 2e-5


def test_conv_gelu_epilogue_and_combined_splits():
    B, Cin, H, W, Cout = 1, 256, 1, 40, 256
    x, w, b = rnd(B, Cin, H, W), rnd(Cout, Cin, 1, 1, seed=2, scale=0.06), rnd(Cout, seed=4)
    want = F.gelu(F.conv2d(x, w, b))
    for kw in (dict(), dict(wpt=4), dict(wpt=2, splits=2), dict(splits=4)):
        got = run_conv(x, w, 1, 0, bias=b, gelu=True, tile=(4, 2), **kw)
        assert relerr(got, want) < 2e-5, kw


def run_wino(x, w, tile, wpt, scale=None, bias=None, tbias=None, res=None, relu=False, after=False, mode=1):
    B, Cin, H, W = x.shape
    Cout = w.shape[0]
    cp = pad_c(Cin)
    xp = torch.zeros(B, H, W, cp)
    xp[..., :Cin] = nhwc(x)
    xd, wd = xp.to(DEV), w.contiguous().to(DEV)
    if mode & 1:
        packed = torch.empty(lib().sbgm_conv_wino_packed_numel(Cout, cp), device=DEV)
        N.check(lib().sbgm_conv_wino_pack_weight(wd.data_ptr(), packed.data_ptr(), Cout, Cin, cp, N.stream()))
    else:
        packed = torch.empty(lib().sbgm_conv_packed_numel(Cout, 3, 3, cp), device=DEV)
        N.check(lib().sbgm_conv_pack_weight(wd.data_ptr(), packed.data_ptr(), Cout, Cin, 3, 3, cp, N.stream()))
    out = torch.empty(B, H, W, Cout, device=DEV)
    dv = lambda t: None if t is None else t.contiguous().to(DEV)  # noqa: E731
    sc, bi, tb, rs = dv(scale), dv(bias), dv(tbias), dv(None if res is None else nhwc(res))
    a = N.ConvArgs(xd.data_ptr(), packed.data_ptr(), out.data_ptr(), N.ptr(sc), N.ptr(bi), N.ptr(tb), N.ptr(rs), B, H, W, cp, Cout, 3, 3, 1, 1,
                   N.RELU if relu else N.NONE, int(after), tile[0], tile[1], 0, wpt, mode, 0, 0, 0, None, 0)
    N.check(lib().sbgm_conv2d_fwd(C.byref(a), N.stream()))
    torch.cuda.synchronize()
    return nchw(out.cpu())


@pytest.mark.parametrize("shape", [(2, 64, 8, 8, 64), (1, 64, 16, 32, 64), (2, 128, 4, 4, 128), (1, 512, 4, 4, 256), (3, 64, 2, 2, 64),
                                   (1, 16, 6, 10, 64)])
@pytest.mark.parametrize("tile", [(4, 1), (2, 2), (2, 1), (4, 2)])
@pytest.mark.parametrize("wpt", [1, 2, 4, 8])
def test_conv_winograd_f23(shape, tile, wpt):
    B, Cin, H, W, Cout = shape
    x, w = rnd(B, Cin, H, W), rnd(Cout, Cin, 3, 3, seed=1, scale=1.0 / math.sqrt(Cin * 9))
    got = run_wino(x, w, tile, wpt)
    assert relerr(got, ref_conv(x, w, 1, 1)) < 2e-5


@pytest.mark.parametrize("shape", [(2, 64, 8, 16, 64), (1, 64, 16, 32, 128), (2, 128, 12, 16, 64), (1, 16, 20, 48, 64), (1, 256, 4, 16, 64)])
@pytest.mark.parametrize("mode,tile", [(2, (4, 1)), (2, (4, 2)), (2, (4, 4)), (2, (2, 2)), (2, (2, 4)), (3, (4, 1)), (3, (4, 2)), (3, (2, 1)),
                                       (3, (2, 2)),
                                       (6, (4, 1)), (6, (2, 4)), (7, (2, 1)), (7, (2, 2)), (7, (4, 1)),      # +4: double-buffered stages
                                       (2, (2, 1)), (3, (1, 1)), (3, (1, 2)), (7, (1, 1))])
def test_conv_lds_staged(shape, mode, tile):
    B, Cin, H, W, Cout = shape
    x, w = rnd(B, Cin, H, W), rnd(Cout, Cin, 3, 3, seed=1, scale=1.0 / math.sqrt(Cin * 9))
    kw = dict(bias=rnd(Cout, seed=4), res=rnd(B, Cout, H, W, seed=6), relu=True)
    got = run_wino(x, w, tile, 0, mode=mode, **kw)
    assert relerr(got, ref_conv(x, w, 1, 1, **kw)) < 2e-5


def run_wino2d(x, w, fco, minw, db, **kw):
    """2-D Winograd F(2x2,3x3) LDS kernel (csrc/conv_w2d.hip) through sbgm_conv2d_fwd: winograd bit 3 (+ bit 2 = double-buffered)"""
    B, Cin, H, W = x.shape
    Cout = w.shape[0]
    cp = pad_c(Cin)
    xp = torch.zeros(B, H, W, cp)
    xp[..., :Cin] = nhwc(x)
    xd, wd = xp.to(DEV), w.contiguous().to(DEV)
    packed = torch.empty(lib().sbgm_conv_wino2d_packed_numel(Cout, cp), device=DEV)
    N.check(lib().sbgm_conv_wino2d_pack_weight(wd.data_ptr(), packed.data_ptr(), Cout, Cin, cp, N.stream()))
    out = torch.empty(B, H, W, Cout, device=DEV)
    dv = lambda t: None if t is None else t.contiguous().to(DEV)  # noqa: E731
    sc, bi, tb, rs = dv(kw.get("scale")), dv(kw.get("bias")), dv(kw.get("tbias")), dv(None if kw.get("res") is None else nhwc(kw["res"]))
    a = N.ConvArgs(xd.data_ptr(), packed.data_ptr(), out.data_ptr(), N.ptr(sc), N.ptr(bi), N.ptr(tb), N.ptr(rs), B, H, W, cp, Cout, 3, 3, 1, 1,
                   N.RELU if kw.get("relu") else N.NONE, int(kw.get("after", False)), fco, 0, 0, 0 if minw == "p" else minw,
                   8 | (16 if minw == "p" else (4 if db else 0)), 0, 0, 0, None, 0)
    N.check(lib().sbgm_conv2d_fwd(C.byref(a), N.stream()))
    torch.cuda.synchronize()
    return nchw(out.cpu())


@pytest.mark.parametrize("shape", [(2, 64, 16, 16, 64), (1, 64, 32, 48, 128), (2, 128, 12, 16, 64), (1, 16, 20, 48, 32), (1, 256, 4, 16, 64),
                                   (3, 32, 2, 16, 32), (1, 64, 34, 32, 64)])
@pytest.mark.parametrize("fco,minw", [(1, 1), (2, 1), (2, 2), (1, "p"), (2, "p")])       # "p": the persistent LDS-DMA kernel
@pytest.mark.parametrize("db", [False, True])
def test_conv_winograd_f2x2_3x3(shape, fco, minw, db):
    if minw == "p" and db:
        pytest.skip("one persistent form")
    """nn.Conv2d(3, padding=1) (reference score_unet.py:468, :489, BasicBlock convs) on the 2-D Winograd kernel: ragged tile rows
    (H = 2, 4, 12, 20, 34), several tiles per row, 1..16 channel stages, the full epilogue"""
    B, Cin, H, W, Cout = shape
    x, w = rnd(B, Cin, H, W), rnd(Cout, Cin, 3, 3, seed=1, scale=1.0 / math.sqrt(Cin * 9))
    assert relerr(run_wino2d(x, w, fco, minw, db), ref_conv(x, w, 1, 1)) < 2e-5
    kw = dict(scale=rnd(Cout, seed=3).abs() + 0.5, bias=rnd(Cout, seed=4), tbias=rnd(B, Cout, seed=5), res=rnd(B, Cout, H, W, seed=6),
              relu=True, after=True)
    assert relerr(run_wino2d(x, w, fco, minw, db, **kw), ref_conv(x, w, 1, 1, **kw)) < 2e-5


def test_conv_winograd_f2x2_3x3_localised():
    """element-wise check on a sparse input: one hot pixel per corner / edge / interior must reproduce the 3x3 stencil exactly
    where a global-norm error measure would hide a wrong border coefficient"""
    B, Cin, H, W, Cout = 1, 16, 32, 32, 32
    x = torch.zeros(B, Cin, H, W)
    for (yy, xx) in [(0, 0), (0, 31), (31, 0), (31, 31), (15, 16), (16, 15), (0, 17), (17, 0), (31, 14), (14, 31)]:
        x[0, (yy + xx) % Cin, yy, xx] = 1.0 + 0.01 * yy
    w = rnd(Cout, Cin, 3, 3, seed=9, scale=0.3)
    want = ref_conv(x, w, 1, 1)
    for minw in (1, "p"):
        assert float((run_wino2d(x, w, 2, minw, False) - want).abs().max()) < 2e-6


def test_conv_winograd_f2x2_3x3_persistent_many_tiles():
    """more tiles than resident workgroups (2 per CU): every workgroup of the persistent kernel walks over several tiles of several
    images and channel slices, with the stage pipeline running across the tile boundaries; B = 40 x 64 x 64 is 640 tiles x 4 slices"""
    B, Cin, H, W, Cout = 40, 32, 64, 64, 64
    x, w = rnd(B, Cin, H, W), rnd(Cout, Cin, 3, 3, seed=1, scale=1.0 / math.sqrt(Cin * 9))
    kw = dict(bias=rnd(Cout, seed=4), res=rnd(B, Cout, H, W, seed=6), relu=True)
    want = ref_conv(x, w, 1, 1, **kw)
    for fco in (1, 2):
        assert relerr(run_wino2d(x, w, fco, "p", False, **kw), want) < 2e-5


def test_conv_winograd_epilogue():
    B, Cin, H, W, Cout = 2, 64, 8, 12, 64
    x, w = rnd(B, Cin, H, W), rnd(Cout, Cin, 3, 3, seed=2, scale=0.04)
    kw = dict(scale=rnd(Cout, seed=3).abs() + 0.5, bias=rnd(Cout, seed=4), tbias=rnd(B, Cout, seed=5), res=rnd(B, Cout, H, W, seed=6),
              relu=True, after=True)
    assert relerr(run_wino(x, w, (4, 1), 2, **kw), ref_conv(x, w, 1, 1, **kw)) < 2e-5


@pytest.mark.parametrize("splits", [2, 3, 4, 9])
def test_conv_splitk_epilogue(splits):
    B, Cin, H, W, Cout = 2, 128, 4, 4, 128
    x, w = rnd(B, Cin, H, W), rnd(Cout, Cin, 3, 3, seed=2, scale=0.03)
    kw = dict(scale=rnd(Cout, seed=3).abs() + 0.5, bias=rnd(Cout, seed=4), tbias=rnd(B, Cout, seed=5), res=rnd(B, Cout, H, W, seed=6),
              relu=True, after=True)
    got = run_conv(x, w, 1, 1, tile=(4, 2), splits=splits, **kw)
    assert relerr(got, ref_conv(x, w, 1, 1, **kw)) < 2e-5


@pytest.mark.parametrize("after", [False, True])
def test_conv_epilogue(after):
    B, Cin, H, W, Cout = 2, 64, 8, 8, 64
    x, w = rnd(B, Cin, H, W), rnd(Cout, Cin, 3, 3, seed=2, scale=0.04)
    kw = dict(scale=rnd(Cout, seed=3).abs() + 0.5, bias=rnd(Cout, seed=4), tbias=rnd(B, Cout, seed=5), res=rnd(B, Cout, H, W, seed=6),
              relu=True, after=after)
    got = run_conv(x, w, 1, 1, **kw)
    assert relerr(got, ref_conv(x, w, 1, 1, **kw)) < 2e-5


def test_pack_input_and_transposes():
    B, H, W = 2, 8, 12
    srcs = [rnd(B, 1, H, W), rnd(B, 2, H, W, seed=1), rnd(B, 2, H, W, seed=2), rnd(B, 3, H, W, seed=3)]
    dv = [s.to(DEV) for s in srcs]
    out = torch.empty(B, H, W, 8, device=DEV)
    ptrs = (C.c_void_p * 4)(*[d.data_ptr() for d in dv])
    chs = (C.c_int * 4)(1, 2, 2, 3)
    N.check(lib().sbgm_pack_input(ptrs, chs, 4, out.data_ptr(), B, H, W, 8, N.stream()))
    want = nhwc(torch.cat(srcs, 1))
    assert torch.equal(out.cpu(), want)
    x = rnd(B, 40, H, W).to(DEV)
    y = torch.empty(B, H, W, 40, device=DEV)
    N.check(lib().sbgm_nchw_to_nhwc(x.data_ptr(), y.data_ptr(), B, H, W, 40, N.stream()))
    assert torch.equal(y.cpu(), nhwc(x.cpu()))
    z = torch.empty_like(x)
    N.check(lib().sbgm_nhwc_to_nchw(y.data_ptr(), z.data_ptr(), B, H, W, 40, N.stream()))
    assert torch.equal(z.cpu(), x.cpu())


@pytest.mark.parametrize("shape", [(2, 64, 4, 4), (1, 128, 8, 6), (2, 512, 1, 1)])
def test_upsample2x(shape):
    x = rnd(*shape)
    B, Cc, H, W = shape
    xd = nhwc(x).to(DEV)
    y = torch.empty(B, 2 * H, 2 * W, Cc, device=DEV)
    N.check(lib().sbgm_upsample2x_fwd(xd.data_ptr(), y.data_ptr(), B, H, W, Cc, N.stream()))
    want = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
    assert relerr(nchw(y.cpu()), want) < 1e-6


@pytest.mark.parametrize("C_,G,hw", [(64, 8, 64 * 64), (512, 8, 16), (128, 128, 100), (256, 8, 4)])
@pytest.mark.parametrize("full", [False, True])
def test_groupnorm(C_, G, hw, full):
    B = 3
    H = int(math.isqrt(hw)) if math.isqrt(hw) ** 2 == hw else 1
    W = hw // H
    x = rnd(B, C_, H, W) * 3 + 0.7
    affine = G != C_
    gamma, beta = (rnd(C_, seed=1), rnd(C_, seed=2)) if affine else (None, None)
    skip, tb = (rnd(B, C_, H, W, seed=3), rnd(B, C_, seed=4)) if full else (None, None)
    xd = nhwc(x).to(DEV)
    y = torch.empty_like(xd)
    ws = torch.empty(1024 * B * G, dtype=torch.uint8, device=DEV)
    dv = lambda t: None if t is None else t.contiguous().to(DEV)  # noqa: E731
    g_, b_, s_, t_ = dv(gamma), dv(beta), dv(None if skip is None else nhwc(skip)), dv(tb)
    N.check(lib().sbgm_groupnorm_fwd(xd.data_ptr(), y.data_ptr(), N.ptr(g_), N.ptr(b_), N.ptr(s_), N.ptr(t_),
                                     N.SILU if full else N.NONE, B, H * W, C_, G, 1e-5, ws.data_ptr(), None, N.stream()))
    want = F.group_norm(x, G, gamma, beta, 1e-5)
    if full:
        want = F.silu(want + skip + tb[:, :, None, None])
    assert relerr(nchw(y.cpu()), want) < 1e-5


@pytest.mark.parametrize("M,C_", [(64, 256), (7, 512), (300, 128), (5, 64)])
def test_layernorm(M, C_):
    x, g, b = rnd(M, C_) * 2 + 1, rnd(C_, seed=1), rnd(C_, seed=2)
    xd, gd, bd = x.to(DEV), g.to(DEV), b.to(DEV)
    y = torch.empty_like(xd)
    N.check(lib().sbgm_layernorm_fwd(xd.data_ptr(), y.data_ptr(), gd.data_ptr(), bd.data_ptr(), M, C_, 1e-5, N.stream()))
    assert relerr(y.cpu(), F.layer_norm(x, (C_,), g, b, 1e-5)) < 1e-5


@pytest.mark.parametrize("with_res", [False, True])
def test_batchnorm_train(with_res):
    B, C_, H, W = 4, 128, 6, 6
    x = rnd(B, C_, H, W) * 2 + 0.5
    g, b = rnd(C_, seed=1), rnd(C_, seed=2)
    rm, rv = rnd(C_, seed=3) * 0.1, rnd(C_, seed=4).abs() + 0.5
    res, tb = (rnd(B, C_, H, W, seed=5), rnd(B, C_, seed=6)) if with_res else (None, None)
    rm_ref, rv_ref = rm.clone(), rv.clone()
    want = F.batch_norm(x, rm_ref, rv_ref, g, b, True, 0.1, 1e-5)
    if with_res:
        want = F.relu(want + res) + tb[:, :, None, None]
    xd, gd, bd, rmd, rvd = nhwc(x).to(DEV), g.to(DEV), b.to(DEV), rm.to(DEV), rv.to(DEV)
    rd = None if res is None else nhwc(res).to(DEV)
    td = None if tb is None else tb.to(DEV)
    y = torch.empty_like(xd)
    ws = torch.empty(24 * C_ + 64, dtype=torch.uint8, device=DEV)
    N.check(lib().sbgm_batchnorm_train_fwd(xd.data_ptr(), y.data_ptr(), gd.data_ptr(), bd.data_ptr(), rmd.data_ptr(), rvd.data_ptr(),
                                           N.ptr(rd), N.ptr(td), int(with_res), B, H * W, C_, 1e-5, 0.1, ws.data_ptr(), None, N.stream()))
    assert relerr(nchw(y.cpu()), want) < 1e-5
    assert relerr(rmd.cpu(), rm_ref) < 1e-5 and relerr(rvd.cpu(), rv_ref) < 1e-5


@pytest.mark.parametrize("B,S,C_,heads", [(2, 64, 256, 4), (2, 16, 512, 4), (1, 256, 128, 4), (3, 4, 256, 2), (1, 1024, 128, 8),
                                          (2, 40, 128, 1), (2, 88, 128, 2), (1, 200, 96, 2),
                                          (32, 256, 128, 4), (2, 1024, 128, 4), (3, 300, 64, 2), (1, 130, 256, 4),     # LDS-staged K/V (S >= 128), ragged S
                                          (2, 64, 128, 16), (1, 256, 128, 16), (2, 40, 96, 4), (1, 144, 48, 4)])      # head dims 8, 24, 12 (d % 4 == 0)
def test_mha_core(B, S, C_, heads):
    qkv = rnd(B, S, 3 * C_)
    d = C_ // heads
    q, k, v = [t.view(B, S, heads, d).transpose(1, 2) for t in qkv.split(C_, dim=-1)]
    att = torch.softmax((q / math.sqrt(d)) @ k.transpose(-1, -2), -1) @ v
    want = att.transpose(1, 2).reshape(B, S, C_)
    qd = qkv.to(DEV)
    out = torch.empty(B, S, C_, device=DEV)
    N.check(lib().sbgm_mha_core_fwd(qd.data_ptr(), out.data_ptr(), B, S, C_, heads, N.stream()))
    assert relerr(out.cpu(), want) < 1e-5


def _pack_linear(w):
    co, ci = w.shape
    wd = w.contiguous().to(DEV)
    packed = torch.empty(lib().sbgm_conv_packed_numel(co, 1, 1, ci), device=DEV)
    N.check(lib().sbgm_conv_pack_weight(wd.data_ptr(), packed.data_ptr(), co, ci, 1, 1, ci, N.stream()))
    return packed


@pytest.mark.parametrize("M,C_", [(256, 128), (40, 64), (16, 256), (100, 512), (8192, 128), (33, 256)])
def test_attention_token_kernels(M, C_):
    """sbgm_attn_qkv_fwd = LayerNorm1 + in_proj, sbgm_attn_tail_fwd = out_proj + residual + LayerNorm2 + FF + residual
    (reference sbgm/score_unet.py:141-145), ragged last token tile included"""
    F = torch.nn.functional
    x, att = rnd(M, C_, seed=1) * 1.5 + 0.3, rnd(M, C_, seed=2)
    g1, b1, g2, b2 = rnd(C_, seed=3) * 0.2 + 1, rnd(C_, seed=4) * 0.2, rnd(C_, seed=5) * 0.2 + 1, rnd(C_, seed=6) * 0.2
    sc = 1.0 / math.sqrt(C_)
    win, bin_ = rnd(3 * C_, C_, seed=7, scale=sc), rnd(3 * C_, seed=8, scale=0.1)
    wo, bo = rnd(C_, C_, seed=9, scale=sc), rnd(C_, seed=10, scale=0.1)
    w1, bb1, w2, bb2 = rnd(C_, C_, seed=11, scale=sc), rnd(C_, seed=12, scale=0.1), rnd(C_, C_, seed=13, scale=sc), rnd(C_, seed=14, scale=0.1)
    want_qkv = F.linear(F.layer_norm(x, (C_,), g1, b1, 1e-5), win, bin_)
    h = x + F.linear(att, wo, bo)
    want = h + F.linear(F.gelu(F.linear(F.layer_norm(h, (C_,), g2, b2, 1e-5), w1, bb1)), w2, bb2)
    d = lambda t: t.contiguous().to(DEV)  # noqa: E731
    xd, attd = d(x), d(att)
    qkv = torch.full((M, 3 * C_), float("nan"), device=DEV)
    head = [d(g1), d(b1), _pack_linear(win), d(bin_)]                       # keep the device tensors alive across the call
    N.check(lib().sbgm_attn_qkv_fwd(xd.data_ptr(), *[t.data_ptr() for t in head], qkv.data_ptr(), M, C_, 1e-5, N.stream()))
    assert relerr(qkv.cpu(), want_qkv) < 1e-5
    out = torch.full((M, C_), float("nan"), device=DEV)
    args = [d(t) for t in (wo, bo, g2, b2)] + [_pack_linear(w1), d(bb1), _pack_linear(w2), d(bb2)]
    args[0] = _pack_linear(wo)
    N.check(lib().sbgm_attn_tail_fwd(attd.data_ptr(), xd.data_ptr(), *[t.data_ptr() for t in args], out.data_ptr(), M, C_, 1e-5, N.stream()))
    assert relerr(out.cpu(), want) < 1e-5
    # in place on x (how the engine calls it)
    N.check(lib().sbgm_attn_tail_fwd(attd.data_ptr(), xd.data_ptr(), *[t.data_ptr() for t in args], xd.data_ptr(), M, C_, 1e-5, N.stream()))
    assert torch.equal(xd, out)
    with pytest.raises(N.NativeError):
        N.check(lib().sbgm_attn_qkv_fwd(xd.data_ptr(), *[t.data_ptr() for t in head], qkv.data_ptr(), M, 96, 1e-5, N.stream()))


@pytest.mark.parametrize("scale", [1, 3, 4, 8])
def test_bilinear_upsample_integer_scales(scale):
    """sbgm_upsample_bilinear_fwd / _bwd == nn.Upsample(scale_factor=s, mode="bilinear", align_corners=False) and its autograd"""
    F = torch.nn.functional
    B, H, W, C_ = 2, 5, 7, 8
    x = rnd(B, C_, H, W, seed=scale).requires_grad_(True)
    y = F.interpolate(x, scale_factor=float(scale), mode="bilinear", align_corners=False)
    go = rnd(B, C_, scale * H, scale * W, seed=scale + 10)
    y.backward(go)
    xd = x.detach().permute(0, 2, 3, 1).contiguous().to(DEV)
    yd = torch.full((B, scale * H, scale * W, C_), float("nan"), device=DEV)
    N.check(lib().sbgm_upsample_bilinear_fwd(xd.data_ptr(), yd.data_ptr(), B, H, W, C_, scale, N.stream()))
    assert relerr(yd.permute(0, 3, 1, 2).cpu(), y.detach()) < 1e-6
    gd = go.permute(0, 2, 3, 1).contiguous().to(DEV)
    dxd = torch.full((B, H, W, C_), float("nan"), device=DEV)
    N.check(lib().sbgm_upsample_bilinear_bwd(gd.data_ptr(), dxd.data_ptr(), B, H, W, C_, scale, N.stream()))
    assert relerr(dxd.permute(0, 3, 1, 2).cpu(), x.grad) < 1e-6
    with pytest.raises(N.NativeError):
        N.check(lib().sbgm_upsample_bilinear_fwd(xd.data_ptr(), yd.data_ptr(), B, H, W, C_, 0, N.stream()))


def test_mha_online_softmax_rescale_branch():
    """spike late keys so the running max jumps in a later key block (guide rule: force the rescale path)"""
    B, S, C_, heads = 1, 64, 64, 2
    qkv = rnd(B, S, 3 * C_)
    qkv[0, 50, C_:2 * C_] *= 25.0          # key 50 dominates every query that aligns with it
    d = C_ // heads
    q, k, v = [t.view(B, S, heads, d).transpose(1, 2) for t in qkv.split(C_, dim=-1)]
    want = (torch.softmax((q.double() / math.sqrt(d)) @ k.double().transpose(-1, -2), -1) @ v.double()).float()
    want = want.transpose(1, 2).reshape(B, S, C_)
    qd = qkv.to(DEV)
    out = torch.empty(B, S, C_, device=DEV)
    N.check(lib().sbgm_mha_core_fwd(qd.data_ptr(), out.data_ptr(), B, S, C_, heads, N.stream()))
    assert relerr(out.cpu(), want) < 1e-5


@pytest.mark.parametrize("with_y", [False, True])
def test_time_projection(with_y):
    B, D, ch = 5, 256, 128
    t = torch.tensor([1e-3, 0.013, 0.37, 0.81, 1.0])
    freqs = rnd(D // 2) * 30.0
    w, b = rnd(ch, D, seed=1) * 0.05, rnd(ch, seed=2)
    table = rnd(5, D, seed=3)
    table[0] = 0
    y = torch.tensor([0, 3, 1, 4, 2]) if with_y else None
    p = t[:, None] * freqs[None, :] * (2.0 * torch.pi)
    emb = torch.cat([p.sin(), p.cos()], -1)
    if with_y:
        emb = emb + table[y]
    want = F.linear(F.silu(emb), w, b)
    td, fd, wd, bd, tabd = t.to(DEV), freqs.to(DEV), w.to(DEV), b.to(DEV), table.to(DEV)
    yd = None if y is None else y.to(DEV)
    out, ws = torch.empty(B, ch, device=DEV), torch.empty(B * D, device=DEV)
    N.check(lib().sbgm_time_proj_fwd(td.data_ptr(), N.ptr(yd), tabd.data_ptr() if with_y else None, fd.data_ptr(), wd.data_ptr(),
                                     bd.data_ptr(), out.data_ptr(), ws.data_ptr(), None, B, D, ch, N.stream()))
    assert relerr(out.cpu(), want) < 2e-5


def test_conv3x3_cout1_with_sigma_division():
    B, C_, H, W = 2, 64, 12, 10
    x, w, b = rnd(B, C_, H, W), rnd(1, C_, 3, 3, seed=1) * 0.05, rnd(1, seed=2)
    t = torch.tensor([0.002, 0.9])
    ls = math.log(25.0)
    std = torch.sqrt((torch.exp(2 * t * ls) - 1) / (2 * ls)).clamp_min(1e-5)
    want = F.conv2d(x, w, b, 1, 1) / std.view(-1, 1, 1, 1)
    xd, wd, bd, td = nhwc(x).to(DEV), w.to(DEV), b.to(DEV), t.to(DEV)
    wp = torch.empty(9 * C_, device=DEV)
    N.check(lib().sbgm_cout1_pack_weight(wd.data_ptr(), wp.data_ptr(), C_, N.stream()))
    out = torch.empty(B, 1, H, W, device=DEV)
    N.check(lib().sbgm_conv3x3_cout1_fwd(xd.data_ptr(), wp.data_ptr(), bd.data_ptr(), td.data_ptr(), 25.0, out.data_ptr(), B, H, W, C_,
                                         N.stream()))
    assert relerr(out.cpu(), want) < 1e-5


def test_sampler_update_kernels():
    B, H = 3, 16
    x, s, z = rnd(B, 1, H, H) * 10, rnd(B, 1, H, H, seed=1), rnd(B, 1, H, H, seed=2)
    g2, dt, nc = 3.7, 0.001, 0.06
    xd, sd, zd = x.to(DEV), s.to(DEV), z.to(DEV)
    xm = torch.empty_like(xd)
    N.check(lib().sbgm_em_step(xd.data_ptr(), xm.data_ptr(), sd.data_ptr(), zd.data_ptr(), g2, dt, nc, 0, 0, x.numel(), N.stream()))
    mean = x + (g2 * s) * dt
    assert relerr(xm.cpu(), mean) < 1e-6 and relerr(xd.cpu(), mean + nc * z) < 1e-6
    # Langevin
    xd = x.to(DEV)
    snr_nn = 0.16 * math.sqrt(H * H)
    ws = torch.empty(B, dtype=torch.float64, device=DEV)
    N.check(lib().sbgm_langevin_step(xd.data_ptr(), sd.data_ptr(), zd.data_ptr(), snr_nn, ws.data_ptr(), 0, 0, B, H * H, N.stream()))
    gn = torch.norm(s.reshape(B, -1), dim=-1).mean()
    eps = 2 * (snr_nn / gn) ** 2
    assert relerr(xd.cpu(), x + eps * s + torch.sqrt(2 * eps) * z) < 1e-5
    # CFG combine
    od = torch.empty_like(sd)
    N.check(lib().sbgm_cfg_combine(od.data_ptr(), sd.data_ptr(), zd.data_ptr(), 1.5, s.numel(), N.stream()))
    assert relerr(od.cpu(), 2.5 * s - 1.5 * z) < 1e-6


def test_philox_normal_statistics_and_streams():
    n = 1 << 20
    a, b = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
    N.check(lib().sbgm_randn_scaled(a.data_ptr(), 2.0, 1234, 0, n, N.stream()))
    N.check(lib().sbgm_randn_scaled(b.data_ptr(), 2.0, 1234, 1, n, N.stream()))
    a, b = a.cpu().double(), b.cpu().double()
    assert abs(a.mean()) < 0.01 and abs(a.std() - 2.0) < 0.01
    assert abs(((a / 2) ** 4).mean() - 3.0) < 0.05                       # kurtosis of a normal
    assert abs((a * b).mean()) < 0.02 and not torch.equal(a, b)           # independent draws per index
    c = torch.empty(n, device=DEV)
    N.check(lib().sbgm_randn_scaled(c.data_ptr(), 2.0, 1234, 0, n, N.stream()))
    assert torch.equal(c.cpu().double(), a)                               # counter-based: reproducible


@pytest.mark.parametrize("transposed", [0, 1])
def test_batched_weight_pack_equals_single_packs(transposed):
    """sbgm_conv_pack_weights_batched (tiled through LDS for >= 16 channels) == one sbgm_conv_pack_weight[_dgrad] per weight"""
    import ctypes
    shapes = [(64, 64, 3), (128, 64, 3), (64, 48, 3), (256, 128, 1), (64, 5, 8), (64, 64, 8), (32, 16, 3), (48, 80, 3)]   # (Cout, Cin, k)
    ws = [rnd(co, ci, k, k, seed=i).to(DEV) for i, (co, ci, k) in enumerate(shapes)]
    descs, outs, blk = [], [], 0
    for w, (co, ci, k) in zip(ws, shapes):
        if transposed:
            if ci % 16 or co % 16:
                continue
            pco, pci, cs = ci, co, co                       # operator sizes of the data gradient
        else:
            pco, pci, cs = co, ci, (2 if ci <= 2 else 4 if ci <= 4 else 8 if ci <= 8 else (ci + 15) // 16 * 16)
        numel = lib().sbgm_conv_packed_numel(pco, k, k, cs)
        single, batched = torch.empty(numel, device=DEV), torch.full((numel,), 7.0, device=DEV)
        if transposed:
            N.check(lib().sbgm_conv_pack_weight_dgrad(w.data_ptr(), single.data_ptr(), co, ci, k, k, N.stream()))
        else:
            N.check(lib().sbgm_conv_pack_weight(w.data_ptr(), single.data_ptr(), co, ci, k, k, cs, N.stream()))
        descs.append(N.PackDesc(w.data_ptr(), batched.data_ptr(), pco, pci, k, k, cs, numel // (pco * 16), transposed, blk))
        blk += lib().sbgm_conv_pack_weights_batched_blocks(pco, k, k, cs)
        outs.append((single, batched))
    raw = (N.PackDesc * len(descs))(*descs)
    dev = torch.frombuffer(bytearray(bytes(raw)), dtype=torch.uint8).to(DEV)
    N.check(lib().sbgm_conv_pack_weights_batched(dev.data_ptr(), len(descs), blk, N.stream()))
    torch.cuda.synchronize()
    assert len(outs) >= 4
    for single, batched in outs:
        assert torch.equal(single, batched)


@pytest.mark.parametrize("transposed,image", [(0, 2), (1, 2), (0, 4), (1, 4)], ids=["0", "1", "0-f2x2", "1-f2x2"])
def test_batched_weight_pack_winograd_layout(transposed, image):
    """sbgm_pack_desc.transposed bit 1 (image 2): the Winograd F(2,3) image of the forward operator == sbgm_conv_wino_pack_weight; of
    the data-gradient operator == sbgm_conv_wino_pack_weight of the explicitly transposed + 180-degree-flipped weight.  Bit 2 (image
    4): the same, bit for bit, for the F(2x2,3x3) image against sbgm_conv_wino2d_pack_weight.  (A convolution through these images
    against the float64 input gradient: test_gpu_conv_dgrad.py.)"""
    numel_of, pack_one = ((lib().sbgm_conv_wino_packed_numel, lib().sbgm_conv_wino_pack_weight) if image == 2 else
                          (lib().sbgm_conv_wino2d_packed_numel, lib().sbgm_conv_wino2d_pack_weight))
    shapes = [(64, 64), (128, 64), (64, 48), (32, 128)]                                          # (Cout, Cin), 3x3
    ws = [rnd(co, ci, 3, 3, seed=i, scale=0.1).to(DEV) for i, (co, ci) in enumerate(shapes)]
    descs, outs, blk, keep = [], [], 0, []
    for w, (co, ci) in zip(ws, shapes):
        if transposed:
            if ci % 16 or co % 16:
                continue
            weff = w.permute(1, 0, 2, 3).flip(2, 3).contiguous()                                   # the dgrad operator's OIHW weight
            pco, pci, cs = ci, co, co
        else:
            weff, pco, pci, cs = w, co, ci, (ci + 15) // 16 * 16
        numel = numel_of(pco, cs)
        single, batched = torch.empty(numel, device=DEV), torch.full((numel,), 7.0, device=DEV)
        N.check(pack_one(weff.data_ptr(), single.data_ptr(), pco, pci, cs, N.stream()))
        descs.append(N.PackDesc(w.data_ptr(), batched.data_ptr(), pco, pci, 3, 3, cs, 0, transposed | image, blk))
        blk += lib().sbgm_conv_pack_weights_batched_blocks(pco, 3, 3, cs)
        outs.append((single, batched))
        keep.append(weff)
    raw = (N.PackDesc * len(descs))(*descs)
    dev = torch.frombuffer(bytearray(bytes(raw)), dtype=torch.uint8).to(DEV)
    N.check(lib().sbgm_conv_pack_weights_batched(dev.data_ptr(), len(descs), blk, N.stream()))
    torch.cuda.synchronize()
    assert len(outs) >= 3
    for single, batched in outs:
        assert torch.equal(single, batched)
