"""The stem's 8x8 stride-2 pad-3 convolution as a space-to-depth Winograd F(2x2,4x4) (conv_s2w.hip, sbgm_conv_args.winograd bit 5):
parity against an fp64 CPU convolution, the pad-3 border by one-hot inputs, graph replay, and the static plan of the C2 shape."""
import csv
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from sbgm_danra_amd import _native as N
from util_models import build_pair, check_parity, maxrel

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = 1e-4


def relerr(got, want):
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-30))


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return torch.randn(*shape, generator=g) * scale


def s2w_conv(x, w, scale=None, bias=None, tbias=None, res=None, relu=False, tile_co=0):
    """x NCHW (CPU), w OIHW [Cout][Cin][8][8] -> NCHW output of sbgm_conv2d_fwd with winograd bit 5."""
    B, Cin, H, W = x.shape
    Cout = w.shape[0]
    cp = (Cin + 15) // 16 * 16
    xp = torch.zeros(B, H, W, cp)
    xp[..., :Cin] = x.permute(0, 2, 3, 1)
    xd, wd = xp.to(DEV), w.contiguous().to(DEV)
    lib = N.lib()
    packed = torch.empty(lib.sbgm_conv8x8s2_wino_packed_numel(Cout, cp), device=DEV)
    N.check(lib.sbgm_conv8x8s2_wino_pack_weight(wd.data_ptr(), packed.data_ptr(), Cout, Cin, cp, N.stream()))
    OH, OW = (H - 2) // 2 + 1, (W - 2) // 2 + 1
    out = torch.full((B, OH, OW, Cout), float("nan"), device=DEV)
    dv = lambda t: None if t is None else t.contiguous().to(DEV)  # noqa: E731
    sc, bi, tb, rs = dv(scale), dv(bias), dv(tbias), dv(None if res is None else res.permute(0, 2, 3, 1))
    a = N.ConvArgs(xd.data_ptr(), packed.data_ptr(), out.data_ptr(), N.ptr(sc), N.ptr(bi), N.ptr(tb), N.ptr(rs), B, H, W, cp, Cout,
                   8, 8, 2, 3, N.RELU if relu else N.NONE, 1, tile_co, 0, 0, 0, 32, 0, 0, 0, None, 0)
    N.check(lib.sbgm_conv2d_fwd(C.byref(a), N.stream()))
    torch.cuda.synchronize()
    return out.cpu().permute(0, 3, 1, 2).contiguous()


def ref_conv(x, w, scale=None, bias=None, tbias=None, res=None, relu=False):
    y = F.conv2d(x.double(), w.double(), None, 2, 3)
    if scale is not None:
        y = y * scale.double().view(1, -1, 1, 1)
    if bias is not None:
        y = y + bias.double().view(1, -1, 1, 1)
    if res is not None:
        y = y + res.double()
    if relu:
        y = F.relu(y)
    if tbias is not None:                                  # tbias_after_act = 1, as the stem's conv2 + bn1 runs it
        y = y + tbias.double()[:, :, None, None]
    return y.float()


CASES = [
    # (B, Cin, H, W, Cout)
    (1, 64, 64, 64, 64),
    (2, 16, 64, 64, 32),
    (2, 64, 128, 128, 64),
    (32, 64, 64, 64, 64),        # C2: encoder.conv2
    (2, 64, 40, 56, 32),         # 20 x 28 outputs: not a multiple of the 16 x 16 tile
    (1, 16, 38, 30, 64),         # 19 x 15 outputs: odd, partial blocks
    (2, 13, 64, 64, 32),         # Cin padded to 16
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("epilogue", [False, True])
@pytest.mark.parametrize("tile_co", [1, 2])
def test_s2w_conv_matches_cpu(case, epilogue, tile_co):
    B, Cin, H, W, Cout = case
    x = rnd(B, Cin, H, W)
    w = rnd(Cout, Cin, 8, 8, seed=1, scale=(Cin * 64) ** -0.5)
    kw = {}
    if epilogue:
        OH, OW = (H - 2) // 2 + 1, (W - 2) // 2 + 1
        kw = dict(scale=rnd(Cout, seed=2).abs() + 0.5, bias=rnd(Cout, seed=3), tbias=rnd(B, Cout, seed=4),
                  res=rnd(B, Cout, OH, OW, seed=5), relu=True)
    got = s2w_conv(x, w, tile_co=tile_co, **kw)
    want = ref_conv(x, w, **kw)
    assert got.shape == want.shape
    assert torch.isfinite(got).all()
    assert relerr(got, want) < 2e-5


@pytest.mark.parametrize("H,W", [(64, 64), (38, 30)])
def test_s2w_one_hot_border(H, W):
    """One input pixel at a time at the corners, edges and both phases of each axis: a wrong pad-3 border or phase shows as a
    misplaced or missing copy of the filter."""
    Cin, Cout = 16, 32
    w = rnd(Cout, Cin, 8, 8, seed=7)
    pts = [(0, 0), (0, 1), (1, 0), (1, 1), (H - 1, W - 1), (H - 2, W - 1), (H - 1, W - 2), (0, W - 1), (H - 1, 0), (2, W // 2),
           (H // 2 + 1, 3), (H - 3, W - 4)]
    x = torch.zeros(len(pts), Cin, H, W)
    for i, (py, px) in enumerate(pts):
        x[i, i % Cin, py, px] = 1.0
    got = s2w_conv(x, w)
    want = ref_conv(x, w)
    for i in range(len(pts)):
        assert relerr(got[i], want[i]) < 2e-5, pts[i]


def test_s2w_graph_replay_equals_eager():
    B, Cin, H, W, Cout = 4, 64, 64, 64, 64
    lib = N.lib()
    x = torch.randn(B, H, W, Cin, device=DEV)
    w = torch.randn(Cout, Cin, 8, 8, device=DEV) * (Cin * 64) ** -0.5
    packed = torch.empty(lib.sbgm_conv8x8s2_wino_packed_numel(Cout, Cin), device=DEV)
    N.check(lib.sbgm_conv8x8s2_wino_pack_weight(w.data_ptr(), packed.data_ptr(), Cout, Cin, Cin, N.stream()))
    bias = torch.randn(Cout, device=DEV)
    out = torch.empty(B, H // 2, W // 2, Cout, device=DEV)
    a = N.ConvArgs(x.data_ptr(), packed.data_ptr(), out.data_ptr(), None, bias.data_ptr(), None, None, B, H, W, Cin, Cout,
                   8, 8, 2, 3, N.RELU, 1, 2, 0, 0, 0, 32, 0, 0, 0, None, 0)
    N.check(lib.sbgm_conv2d_fwd(C.byref(a), N.stream()))
    torch.cuda.synchronize()
    eager = out.clone()
    out.zero_()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        N.check(lib.sbgm_conv2d_fwd(C.byref(a), N.stream()))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    out.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        N.check(lib.sbgm_conv2d_fwd(C.byref(a), N.stream()))
    for _ in range(3):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


def test_static_plan_runs_the_stem_conv2_on_s2w(tmp_path):
    """At the C2 shape (B = 32, 128 x 128) the static plan puts encoder.conv2 (8x8 / s2 on 64 channels) on the space-to-depth
    Winograd kernel; one sample of the batch matches the oracle and equals that sample run alone."""
    ora, net, _ = build_pair(1)
    ora.eval(), net.eval()
    g = torch.Generator().manual_seed(11)
    B, HW = 32, 128
    x, c = torch.randn(B, 1, HW, HW, generator=g), torch.randn(B, 1, HW, HW, generator=g)
    t = torch.rand(B, generator=g) * 0.999 + 1e-3
    xd, cd, td = x.cuda(), c.cuda(), t.cuda()
    with torch.no_grad():
        full = net(xd, td, cond_img=cd)
    eng = net._engine(None, None, cd)
    prof, o, path = N.Profile(), torch.empty_like(xd), str(tmp_path / "convs.csv")
    N.check(N.lib().sbgm_model_profile_forward(eng.h, xd.data_ptr(), td.data_ptr(), None, cd.data_ptr(), None, None, o.data_ptr(), B, HW,
                                               HW, C.byref(prof), path.encode(), N.stream()))
    rows = list(csv.DictReader(open(path)))
    stem2 = [r for r in rows if r["kh"] == "8" and r["Cin_pad"] == "64"]
    assert len(stem2) == 1 and "s2w" in stem2[0]["kernel"], [r["kernel"] for r in stem2]
    k = 9
    with torch.no_grad():
        solo = net(xd[k:k + 1], td[k:k + 1], cond_img=cd[k:k + 1])
        want = ora(x[k:k + 1], t[k:k + 1], cond_img=c[k:k + 1])
    assert torch.isfinite(full).all()
    check_parity(full[k:k + 1].cpu(), want, TOL, "C2 sample with the stem on s2w")
    assert maxrel(full[k:k + 1].cpu(), solo.cpu()) <= 2e-5


def test_tile_table_round_trips_the_s2w_tile(tmp_path):
    """The tuner puts encoder.conv2 of the C2 shape on the F(2x2,4x4) kernel (wino field 3); a second model loads that table and
    evaluates bit-identically; the loader refuses the value on a shape or tile the kernel does not take."""
    _, a, _ = build_pair(1)
    _, b, _ = build_pair(1)
    a.eval(), b.eval()
    path = str(tmp_path / "tiles.txt")
    a.autotune(32, 128, 128, cache=path)
    stem2 = [ln.split() for ln in open(path) if ln.startswith("8 8 2 3 32 64 64 64 64 ")]
    assert len(stem2) == 1 and stem2[0][-2:] == ["3", "1"], stem2
    b.autotune(32, 128, 128, cache=path)                 # loads
    g = torch.Generator().manual_seed(5)
    x, c = torch.randn(32, 1, 128, 128, generator=g).cuda(), torch.randn(32, 1, 128, 128, generator=g).cuda()
    t = (torch.rand(32, generator=g) * 0.999 + 1e-3).cuda()
    with torch.no_grad():
        assert torch.equal(a(x, t, cond_img=c), b(x, t, cond_img=c))
    for line in ("8 8 2 3 32 64 64 64 64 0 0 | 4 1 1 1 3 1\n", "3 3 1 1 32 32 32 64 64 0 0 | 1 1 1 1 3 1\n"):
        bad = str(tmp_path / "bad.txt")
        open(bad, "w").write(line)
        with pytest.raises(N.NativeError):
            b.autotune(32, 128, 128, cache=bad)
