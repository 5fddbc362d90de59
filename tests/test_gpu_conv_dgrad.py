"""The data-gradient operator of the training path, candidate by candidate against float64 (tests/conv_dgrad_ref.py).

ConvFn.backward computes dx with the FORWARD convolution kernels on a second weight image (transposed, 180-degree flipped; pad = k-1-pad;
for stride 2: in_dil = 2 and an explicit output size; the pending partial sum of x's other consumers as the residual epilogue), on
whichever candidate the tuner timed fastest.  Here every candidate sbgm_conv2d_tiles lists for that call is forced once through
sbgm_conv2d_fwd (tile_co / tile_px / splits / waves_per_tile / winograd), into a NaN-filled output, without and with a residual:

    max|got - ref64| / max|ref64| < 2e-5   and no NaN                         (the bound test_gpu_ops.py holds these kernels to)
    localised (one-hot dy): max|got - ref64| < 2e-6 absolute                 (a wrong parity or border coefficient a norm dilutes)

ref64 = x.grad of F.conv2d in float64 by CPU autograd (+ res).  Every test prints `DGRAD-WORST <geometry> <family> ...`, the worst
measured value per kernel family (DESIGN.md 5 records them); a failure names the tile's six ints and its family."""
import ctypes as C

import pytest
import torch

import conv_dgrad_ref as R
from attention_ref import Poisoned
from sbgm_danra_amd import _native as N
from sbgm_danra_amd import train_graph as T

pytestmark = pytest.mark.gpu

DEV = "cuda"
WS_FLOATS = 1 << 21            # split-K workspace: holds 16 splits of the largest output here (69632 floats)
BOUND, LOCAL_BOUND = 2e-5, 2e-6


def lib():
    return N.lib()


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def pack_batched(w, cout, cin, k, cs, flags):
    """one weight through sbgm_conv_pack_weights_batched; flags = sbgm_pack_desc.transposed (bit 0 data-gradient operator, bit 1 the
    F(2,3) image, bit 2 the F(2x2,3x3) image)"""
    numel = (lib().sbgm_conv_wino_packed_numel(cout, cs) if flags & 2 else lib().sbgm_conv_wino2d_packed_numel(cout, cs) if flags & 4
             else lib().sbgm_conv_packed_numel(cout, k, k, cs))
    dst = torch.full((numel,), float("nan"), device=DEV)
    d = N.PackDesc(w.data_ptr(), dst.data_ptr(), cout, cin, k, k, cs, numel // (cout * 16), flags, 0)
    dev = torch.frombuffer(bytearray(bytes(d)), dtype=torch.uint8).to(DEV)
    N.check(lib().sbgm_conv_pack_weights_batched(dev.data_ptr(), 1, lib().sbgm_conv_pack_weights_batched_blocks(cout, k, k, cs), N.stream()))
    return dst


def dgrad_images(w, geom, call):
    """the images ConvFn.backward brings for weight w (device, OIHW of the forward layer): implicit GEMM from
    sbgm_conv_pack_weight_dgrad, and where the geometry admits them F(2,3) (transposed = 1|2) and F(2x2,3x3) (1|4)"""
    B, Cin, H, W, Cout, k, s, p = geom
    g = torch.full((lib().sbgm_conv_packed_numel(Cin, k, k, Cout),), float("nan"), device=DEV)
    N.check(lib().sbgm_conv_pack_weight_dgrad(w.data_ptr(), g.data_ptr(), Cout, Cin, k, k, N.stream()))
    return dict(g=g, w=pack_batched(w, Cin, Cout, k, Cout, 1 | 2) if call["wino"] else None,
                d=pack_batched(w, Cin, Cout, k, Cout, 1 | 4) if call["w2d"] else None)


class Launch:
    """one sbgm_conv2d_fwd call (geometry `call`, images `imgs`, NHWC input x) whose tile is forced per run; the input and the
    output sit inside NaN-poisoned allocations and the output is refilled with NaN before every run"""

    def __init__(self, call, imgs, x_nhwc, res_nhwc=None):
        self.call, self.imgs = call, imgs
        oh = call["out_h"] or (call["H"] + 2 * call["pad"] - call["k"]) // call["stride"] + 1
        ow = call["out_w"] or (call["W"] + 2 * call["pad"] - call["k"]) // call["stride"] + 1
        assert tuple(x_nhwc.shape) == (call["B"], call["H"], call["W"], call["c_pad"])
        self.x = Poisoned(tuple(x_nhwc.shape), DEV, x_nhwc)
        self.out = Poisoned((call["B"], oh, ow, call["Cout"]), DEV)
        self.res = None if res_nhwc is None else Poisoned(tuple(self.out.t.shape), DEV, res_nhwc)
        self.ws = torch.empty(WS_FLOATS, device=DEV)
        assert 16 * self.out.t.numel() <= WS_FLOATS

    def args(self, tile=None):
        c = self.call
        co, px, splits, waves, bits = R.args_tile(tile) if tile is not None else (0, 0, 0, 0, 0)
        return N.ConvArgs(self.x.ptr(), self.imgs["g"].data_ptr(), self.out.ptr(), None, None, None, None if self.res is None else self.res.ptr(),
                          c["B"], c["H"], c["W"], c["c_pad"], c["Cout"], c["k"], c["k"], c["stride"], c["pad"], N.NONE, 0, co, px, splits, waves,
                          bits, c["in_dil"], c["out_h"], c["out_w"], self.ws.data_ptr(), WS_FLOATS, 0, None, None, 0, N.ptr(self.imgs["w"]),
                          N.ptr(self.imgs["d"]))

    def candidates(self):
        a = self.args()
        buf = (C.c_int * (6 * 512))()
        n = lib().sbgm_conv2d_tiles(C.byref(a), buf, 512)
        assert 0 < n <= 512, lib().sbgm_last_error()
        return [tuple(buf[6 * i:6 * i + 6]) for i in range(n)]

    def run(self, tile):
        self.out.t.fill_(float("nan"))
        a = self.args(tile)
        N.check(lib().sbgm_conv2d_fwd(C.byref(a), N.stream()))
        return self.out.t


def errors(got, ref):
    """(max|got - ref| / max|ref|, max|got - ref|) in float64 on the device; NaN when got holds a NaN or an Inf"""
    if not bool(torch.isfinite(got).all()):
        return float("nan"), float("nan")
    d = float((got.double() - ref).abs().max())
    return d / float(ref.abs().max()), d


def sweep(label, launch, ref, finish=None, absolute=None):
    """every candidate of the launch once; finish: what turns the launch's output into dx (the phase operator's depth-to-space)"""
    cands = launch.candidates()
    worst, fails = {}, []
    for tile in cands:
        fam = R.family(tile)
        assert fam != "space-to-depth Winograd F(2x2,4x4)" and (launch.imgs[R.image_of(tile)] is not None), (tile, fam)
        got = launch.run(tile)
        if finish is not None:
            got = finish(got)
        rel, ab = errors(got, ref)
        val, bound = (ab, absolute) if absolute is not None else (rel, BOUND)
        worst[fam] = max(worst.get(fam, 0.0), val) if val == val else float("nan")
        if not val < bound:
            fails.append(f"{label} tile={tile} ({fam}): {'max|got - ref64|' if absolute is not None else 'max|got - ref64| / max|ref64|'} = "
                         f"{val:.3e}, bound {bound:g}")
    torch.cuda.synchronize()
    assert launch.out.surround_unchanged() and launch.x.surround_unchanged(), f"{label}: a kernel wrote outside its tensors"
    for fam, v in sorted(worst.items()):
        print(f"DGRAD-WORST {label} {fam}: {v:.3e} over {sum(R.family(t) == fam for t in cands)} tiles")
    assert not fails, f"{len(fails)} of {len(cands)} candidates:\n" + "\n".join(fails)
    return cands


@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("geom", R.CASES, ids=lambda g: "-".join(map(str, g)))
def test_every_candidate_against_float64(geom, with_res):
    c = R.case(geom)
    call = R.dgrad_call(geom)
    imgs = dgrad_images(c["w"].to(DEV), geom, call)
    launch = Launch(call, imgs, nhwc(c["dy"]).to(DEV), nhwc(c["res"]).to(DEV) if with_res else None)
    ref = nhwc(c["ref_res" if with_res else "ref"]).to(DEV)
    cands = sweep(f"{geom} {'residual' if with_res else 'plain'}", launch, ref)
    fams = {R.family(t) for t in cands}
    if geom[6] == 2:
        assert call["in_dil"] == 2 and fams == {"implicit-GEMM"}
    elif geom[5] == 3:
        assert len(fams) == 6, fams                           # the three stride-1 cases bring every family


@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "residual"])
def test_phase_operator_every_candidate_against_float64(with_res):
    """dx of the 8x8 / s2 / p3 stem convolution as ConvFn.backward assembles it on even maps: sbgm_conv8x8s2_dgrad_phase_weight ->
    sbgm_conv_pack_weight -> a 5x5 / s1 / p2 convolution of dy to 4 Cin phase-major channels -> sbgm_depth_to_space2.  The residual
    rides in the convolution's epilogue in the phase layout (sbgm_space_to_depth2 of it)."""
    geom = R.PHASE_CASE
    B, Cin, H, W, Cout, k, s, p = geom
    c = R.case(geom)
    w = c["w"].to(DEV)
    wph = torch.full((4 * Cin, Cout, 5, 5), float("nan"), device=DEV)
    N.check(lib().sbgm_conv8x8s2_dgrad_phase_weight(w.data_ptr(), wph.data_ptr(), Cout, Cin, N.stream()))
    pk = torch.full((lib().sbgm_conv_packed_numel(4 * Cin, 5, 5, Cout),), float("nan"), device=DEV)
    N.check(lib().sbgm_conv_pack_weight(wph.data_ptr(), pk.data_ptr(), 4 * Cin, Cout, 5, 5, Cout, N.stream()))
    call = dict(B=B, H=H // 2, W=W // 2, c_pad=Cout, Cout=4 * Cin, k=5, stride=1, pad=2, in_dil=0, out_h=0, out_w=0)
    res_ph = None
    if with_res:
        res, res_ph = nhwc(c["res"]).to(DEV), torch.full((B, H // 2, W // 2, 4 * Cin), float("nan"), device=DEV)
        N.check(lib().sbgm_space_to_depth2(res.data_ptr(), res_ph.data_ptr(), B, H // 2, W // 2, Cin, N.stream()))
    launch = Launch(call, dict(g=pk, w=None, d=None), nhwc(c["dy"]).to(DEV), res_ph)
    dx = Poisoned((B, H, W, Cin), DEV)

    def finish(ph):
        dx.t.fill_(float("nan"))
        N.check(lib().sbgm_depth_to_space2(ph.data_ptr(), dx.ptr(), B, H // 2, W // 2, Cin, N.stream()))
        return dx.t

    cands = sweep(f"{geom} phase operator {'residual' if with_res else 'plain'}", launch, nhwc(c["ref_res" if with_res else "ref"]).to(DEV), finish)
    assert {R.family(t) for t in cands} == {"implicit-GEMM"} and dx.surround_unchanged()


@pytest.mark.parametrize("geom", R.LOCALISED_CASES, ids=lambda g: "-".join(map(str, g)))
def test_localised_one_hot_dy_reproduces_the_flipped_stencil(geom):
    """dy zero except the four corners, a pixel on each edge and an interior pixel of each (row, column) parity, on distinct channels
    with values near 1: every dx element is one weight times one value (or zero), to 2e-6 absolute, on every candidate"""
    c = R.localised_case(geom)
    call = R.dgrad_call(geom)
    launch = Launch(call, dgrad_images(c["w"].to(DEV), geom, call), nhwc(c["dy"]).to(DEV))
    assert float(c["ref"].abs().max()) > 0.5
    cands = sweep(f"{geom} localised", launch, nhwc(c["ref"]).to(DEV), absolute=LOCAL_BOUND)
    assert len({R.family(t) for t in cands}) == (6 if geom[6] == 1 else 1)


def test_a_sixteen_channel_data_gradient_is_no_call_of_this_path():
    """forward Cin = 16: the tuner lists nothing for its data gradient (Cout % 32), and ConvFn.backward refuses it"""
    geom = R.REFUSED_CASE
    call = R.dgrad_call(geom)
    a = N.ConvArgs(64, 64, 64, None, None, None, None, call["B"], call["H"], call["W"], call["c_pad"], call["Cout"], 3, 3, 1, 1, N.NONE, 0, 0, 0, 0,
                   0, 0, 0, call["out_h"], call["out_w"], None, 0)
    assert lib().sbgm_conv2d_tiles(C.byref(a), (C.c_int * 6)(), 1) == 0
    B, Cin, H, W, Cout, k, s, p = geom
    T._zero_reset(torch.device(DEV))
    x = torch.zeros(B, H, W, Cin, device=DEV, requires_grad=True)
    y = T.ConvFn.apply(x, R.rnd(Cout, Cin, k, k).to(DEV), None, None, None, s, p)
    with pytest.raises(NotImplementedError):
        y.sum().backward()


FORCED = {"g": (2, 1, 2, 2, 0, 0), "w": (4, 1, 1, 2, 1, 0), "d": (2, 1, 1, 1, 2, 1)}      # grid + in-workgroup split-K; F(2,3); F(2x2,3x3)


@pytest.mark.parametrize("layout", ["g", "w", "d"])
def test_convfn_backward_under_a_forced_tile(layout, monkeypatch):
    """the Python glue: two ConvFn consumers of one x share a gradient slot, so the second data gradient carries the first as its
    residual epilogue; no pack plan, so _conv_with_images packs every image on the spot.  Then one _conv_with_images call that
    brings only an image the forced tile does not read: the _MissingImage fallback."""
    geom = R.CASES[0]
    B, Cin, H, W, Cout, k, s, p = geom
    c = R.case(geom)
    call = R.dgrad_call(geom)
    forced = FORCED[layout]
    fixed = T._tile_from_tune(forced)
    assert fixed == R.args_tile(forced) and T._tile_layout(fixed) == layout == R.image_of(forced)
    w1, w2 = c["w"], R.rnd(Cout, Cin, k, k, seed=11, scale=float(c["w"].std()))
    g1, g2 = c["dy"], R.rnd(*c["dy"].shape, seed=12)
    x64 = torch.zeros(B, Cin, H, W, dtype=torch.float64, requires_grad=True)
    conv = lambda w: torch.nn.functional.conv2d(x64, w.double(), None, s, p)  # noqa: E731
    ((conv(w1) * g1.double()).sum() + (conv(w2) * g2.double()).sum()).backward()
    ref = nhwc(x64.grad).to(DEV)
    saved = dict(T._TILES)
    T._TILES.clear()
    monkeypatch.setattr(T, "_tile_from_tune", lambda t6: fixed)
    try:
        dev = torch.device(DEV)
        T._zero_reset(dev)
        x = torch.zeros(B, H, W, Cin, device=DEV, requires_grad=True)
        slot = T._slot(2)
        assert slot is not None
        w1d, w2d = w1.to(DEV), w2.to(DEV)
        y1 = T.ConvFn.apply(x, w1d, None, None, None, s, p, slot)
        y2 = T.ConvFn.apply(x, w2d, None, None, None, s, p, slot)
        ((y1 * nhwc(g1).to(DEV)).sum() + (y2 * nhwc(g2).to(DEV)).sum()).backward()
        assert T._TILES and all(t == fixed for t in T._TILES.values())
        keys = [key for key in T._TILES if key[11]]                                     # the data-gradient call that carried a residual
        assert len(keys) == 1 and keys[0][9] == (H, W)
        rel, _ = errors(x.grad, ref)
        print(f"DGRAD-GLUE layout {layout} tile={forced} ({R.family(forced)}): ConvFn dx with a slot partial sum {rel:.3e}")
        assert rel < BOUND, (forced, R.family(forced), rel)
        # _MissingImage: the plan's images hold another layout than the tile reads
        imgs = dgrad_images(w2d, geom, call)
        other = (None, imgs["w"], None) if layout == "g" else (imgs["g"], None, None)
        dy2, extra, dx = nhwc(g2).to(DEV), nhwc(c["res"]).to(DEV), torch.full((B, H, W, Cin), float("nan"), device=DEV)
        used, packed_here = T._conv_with_images(dy2, w2d, dx, other, True, Cout, Cin, k, 1, k - 1 - p, res=extra, in_dil=0, out_hw=(H, W))
        assert (used, packed_here) == (layout, True)
        x64.grad = None
        (conv(w2) * g2.double()).sum().backward()
        rel, _ = errors(dx, nhwc(x64.grad + c["res"].double()).to(DEV))
        print(f"DGRAD-GLUE layout {layout} tile={forced}: _conv_with_images after _MissingImage {rel:.3e}")
        assert rel < BOUND, (forced, R.family(forced), rel)
    finally:
        T._TILES.clear()
        T._TILES.update(saved)
