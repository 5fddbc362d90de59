"""The composed final block (csrc/conv_final.hip): final_layer.conv(final_layer.conv_up(up(x))) as one 3x3 convolution to the 9 taps
of `conv` plus a 9-point gather.  The weight composition against an fp64 einsum, the block alone against the fp64 CPU chain on every
kernel family the autotuner offers for it (random, one-hot and zero inputs), the whole network against the projection path
(SBGM_NO_FINAL_COMPOSE=1), graph replay, and weight changes reaching the composed images.  The step samplers (EM, PC, EDM Heun) and
the profiled forward take the composed route; the plain forward and RK45 keep the projection path (engine.h, set_routes)."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from sbgm_danra_amd import _native as N
from util_models import build_pair, check_parity

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
TOL = 1e-4              # the project's per-evaluation tolerance
SAMPLER_TOL = 1e-3      # the project's short-horizon sampler tolerance
BOUND = 2e-5            # the project's bound for a kernel against fp64 (test_gpu_stem_compose.py, test_gpu_stem_winograd.py)
C = 64


def relerr(got, want):
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-30))


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return torch.randn(*shape, generator=g) * scale


def weights(seed=1, c=C):
    s = (9 * c) ** -0.5
    return rnd(c, c, 3, 3, seed=seed, scale=s), rnd(c, seed=seed + 1, scale=0.5), rnd(1, c, 3, 3, seed=seed + 2, scale=s), rnd(1, seed=seed + 3)


def compose_pack(w1, b1, w2):
    c = w1.shape[0]
    wc, bc = torch.full((16, c, 3, 3), float("nan"), device=DEV), torch.full((16,), float("nan"), device=DEV)
    a, b, d = w1.contiguous().to(DEV), b1.contiguous().to(DEV), w2.contiguous().to(DEV)
    N.check(N.lib().sbgm_final_compose_pack(a.data_ptr(), b.data_ptr(), d.data_ptr(), wc.data_ptr(), bc.data_ptr(), c, N.stream()))
    torch.cuda.synchronize()
    return wc, bc


class Block:
    """the composed block's device operands: Wc in the three packed layouts, bc, b2"""

    def __init__(self, w1, b1, w2, b2):
        lib, c = N.lib(), w1.shape[0]
        self.c = c
        self.wc, self.bc = compose_pack(w1, b1, w2)
        self.b2 = b2.to(DEV)
        self.igemm = torch.empty(lib.sbgm_conv_packed_numel(16, 3, 3, c), device=DEV)
        self.wino = torch.empty(lib.sbgm_conv_wino_packed_numel(16, c), device=DEV)
        self.w2d = torch.empty(lib.sbgm_conv_wino2d_packed_numel(16, c), device=DEV)
        N.check(lib.sbgm_conv_pack_weight(self.wc.data_ptr(), self.igemm.data_ptr(), 16, c, 3, 3, c, N.stream()))
        N.check(lib.sbgm_conv_wino_pack_weight(self.wc.data_ptr(), self.wino.data_ptr(), 16, c, c, N.stream()))
        N.check(lib.sbgm_conv_wino2d_pack_weight(self.wc.data_ptr(), self.w2d.data_ptr(), 16, c, c, N.stream()))
        torch.cuda.synchronize()

    def run(self, x, tile=None, scale=None, shift=None, skip=None, act=N.NONE):
        """x: low-resolution NCHW (CPU) -> the block's output [B,1,2h,2w] (CPU)"""
        B, c, h, w = x.shape
        H, W = 2 * h, 2 * w
        nhwc = lambda t: None if t is None else t.permute(0, 2, 3, 1).contiguous().to(DEV)  # noqa: E731
        xd, sk = nhwc(x), nhwc(skip)
        aff = None
        if scale is not None:                     # [B][c/4][2][4]: scale quad, shift quad
            aff = torch.stack([scale.view(B, c // 4, 4), shift.view(B, c // 4, 4)], dim=2).contiguous().to(DEV)
        ws = torch.full((B * H * W * (16 + c),), float("nan"), device=DEV)
        out = torch.full((B, 1, H, W), float("nan"), device=DEV)
        tl = None if tile is None else (ctypes.c_int * 6)(*tile)
        N.check(N.lib().sbgm_final_block_fwd(xd.data_ptr(), N.ptr(aff), N.ptr(sk), act, self.igemm.data_ptr(), self.wino.data_ptr(),
                                             self.w2d.data_ptr(), self.bc.data_ptr(), self.b2.data_ptr(), None, 1.0, out.data_ptr(),
                                             ws.data_ptr(), ws.numel(), B, H, W, c, tl, N.stream()))
        torch.cuda.synchronize()
        return out.cpu()


def tiles_of(B, H, W, c=C):
    buf = (ctypes.c_int * (6 * 64))()
    n = N.lib().sbgm_final_block_tiles(B, H, W, c, buf, 64)
    assert 0 < n <= 64
    return [tuple(buf[6 * i:6 * i + 6]) for i in range(n)]


def chain(x, w1, b1, w2, b2, scale=None, shift=None, skip=None, silu=False):
    """conv(conv_up(interpolate(act(x * scale + shift + skip)))) in fp64 on the CPU"""
    v = x.double()
    if scale is not None:
        v = v * scale.double()[:, :, None, None] + shift.double()[:, :, None, None]
    if skip is not None:
        v = v + skip.double()
    if silu:
        v = F.silu(v)
    up = F.interpolate(v, scale_factor=2, mode="bilinear", align_corners=False)
    return F.conv2d(F.conv2d(up, w1.double(), b1.double(), padding=1), w2.double(), b2.double(), padding=1).float()


@pytest.fixture(scope="module")
def block():
    w = weights()
    return w, Block(*w)


def test_compose_pack_matches_fp64_einsum():
    w1, b1, w2, _ = weights(seed=11)
    wc, bc = compose_pack(w1, b1, w2)
    wc, bc = wc.cpu(), bc.cpu()
    w2t = w2[0].reshape(C, 9).double()
    want_w = torch.einsum("ot,ocvb->tcvb", w2t, w1.double()).float()
    want_b = (w2t.t() @ b1.double()).float()
    assert torch.equal(wc[9:], torch.zeros(7, C, 3, 3)) and torch.equal(bc[9:], torch.zeros(7))

    def ulps(got, want):                       # distance in units of the last place of `want`
        spacing = torch.nextafter(want.abs(), torch.full_like(want, float("inf"))) - want.abs()
        return float(((got - want).abs() / spacing).max())
    uw, ub = ulps(wc[:9], want_w), ulps(bc[:9], want_b)
    print(f"compose pack: weights within {uw:.1f} ulp, bias within {ub:.1f} ulp of the fp64 einsum")
    assert uw <= 1.0 and ub <= 1.0


# low-resolution shape -> output: 32x32 the narrowest fused width; 24x48 a partial tile row and a non-square map; 16x16 the unfused
# route (upsample2x + a plain 16-channel convolution), which applies nothing on load (the decoder normalises in a pass of its own there)
CASES = [((2, 16, 16), False), ((2, 16, 16), True), ((2, 12, 24), False), ((2, 12, 24), True), ((2, 8, 8), False)]


@pytest.mark.parametrize("shape,on_load", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else ("on_load" if v else "plain"))
def test_block_matches_fp64_chain_on_every_kernel_family(block, shape, on_load):
    (w1, b1, w2, b2), blk = block
    B, h, w = shape
    x = rnd(B, C, h, w, seed=2)
    kw, ckw = {}, {}
    if on_load:
        scale, shift, skip = rnd(B, C, seed=3).abs() + 0.5, rnd(B, C, seed=4), rnd(B, C, h, w, seed=5)
        kw = dict(scale=scale, shift=shift, skip=skip, act=N.SILU)
        ckw = dict(scale=scale, shift=shift, skip=skip, silu=True)
    want = chain(x, w1, b1, w2, b2, **ckw)
    tiles = tiles_of(B, 2 * h, 2 * w)
    kinds = {(t[4], t[5]) for t in tiles}
    # one-tile single / double buffer and persistent 2-D Winograd, row-only LDS single / double buffer
    assert {(2, 1), (2, 2), (2, 3), (1, 1), (1, 2)} <= kinds, tiles
    for tile in [None] + tiles:
        got = blk.run(x, tile, **kw)
        assert got.shape == want.shape and torch.isfinite(got).all(), tile
        err = relerr(got, want)
        print(f"final block {shape} on_load={on_load} tile={tile}: max-rel {err:.2e} against the fp64 chain (bound {BOUND:.0e})")
        assert err < BOUND, tile


@pytest.mark.parametrize("h,w", [(16, 16), (12, 24)])
def test_block_one_hot_inputs(block, h, w):
    """single low-resolution pixels at the four corners, along two edges and in the interior: a wrong clamp, pad or tap shift shows
    as a misplaced copy of the filter"""
    (w1, b1, w2, b2), blk = block
    pts = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)]
    pts += [(r, 0) for r in (1, 3, h // 2, h - 2)] + [(h - 1, c) for c in (1, 7, 8, w - 2)]
    pts += [(h // 2, w // 2), (7, 8), (8, 7), (3, w - 4)]
    x = torch.zeros(len(pts), C, h, w)
    for i, (py, px) in enumerate(pts):
        x[i, (7 * i) % C, py, px] = 1.0
    want = chain(x, w1, torch.zeros_like(b1), w2, torch.zeros_like(b2))
    nob = Block(w1, torch.zeros_like(b1), w2, torch.zeros_like(b2))
    for tile in [None] + [t for t in tiles_of(len(pts), 2 * h, 2 * w) if t[5] != 2]:       # each family once (double buffer = same arithmetic)
        got = nob.run(x, tile)
        worst = max(relerr(got[i], want[i]) for i in range(len(pts)))
        print(f"one-hot {h}x{w} tile={tile}: worst max-rel {worst:.2e} over {len(pts)} points")
        for i in range(len(pts)):
            assert relerr(got[i], want[i]) < BOUND, (tile, pts[i])


@pytest.mark.parametrize("h,w", [(16, 16), (8, 8)])
def test_zero_input_leaves_the_bias_term(block, h, w):
    """zero input, non-zero b1: the output is b2 + the sum of bc over the taps inside the image, so the border ring differs from the
    interior; a bias added outside the image would fill the ring in"""
    (w1, b1, w2, b2), blk = block
    got = blk.run(torch.zeros(1, C, h, w))
    want = chain(torch.zeros(1, C, h, w), w1, b1, w2, b2)
    bc = blk.bc.cpu().double()
    inner = float(b2.double() + bc[:9].sum())
    corner = float(b2.double() + bc[[4, 5, 7, 8]].sum())
    err = relerr(got, want)
    print(f"bias term alone {2 * h}x{2 * w}: max-rel {err:.2e}")
    assert err < BOUND
    scale = float(want.abs().max())
    assert abs(float(got[0, 0, 5, 5]) - inner) < BOUND * scale and abs(float(got[0, 0, 0, 0]) - corner) < BOUND * scale
    assert abs(inner - corner) > 1e-3 * scale


# ---- the whole network ---------------------------------------------------------------------------------------------------------------
_CHILD = r"""
import ctypes, sys, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from util_models import build_pair
import sbgm_danra_amd as S
from sbgm_danra_amd import _native as N
_, net, _ = build_pair(1)
net.eval()
g = torch.Generator().manual_seed(3)
x, c, t = torch.randn(2, 1, 64, 64, generator=g).cuda(), torch.randn(2, 1, 64, 64, generator=g).cuda(), (torch.rand(2, generator=g) * 0.9 + 0.05).cuda()
kw = dict(batch_size=2, device="cuda", img_size=64, cond_img=c, seed=5)
a = (net, S.marginal_prob_std_fn, S.diffusion_coeff_fn)
out = {}
with torch.no_grad():
    out["forward_plain"] = net(x, t, cond_img=c)
    # one evaluation on the route the samplers take: the profiled forward (composed unless the switch is set)
    eng, o = net._engine(None, None, c), torch.empty_like(x)
    N.check(N.lib().sbgm_model_profile_forward(eng.h, x.data_ptr(), t.data_ptr(), None, c.data_ptr(), None, None, o.data_ptr(), 2, 64, 64,
                                               ctypes.byref(N.Profile()), None, N.stream()))
    torch.cuda.synchronize()
    out["forward"] = o
    out["em"] = S.Euler_Maruyama_sampler(*a, num_steps=5, **kw)
    out["em_eager"] = S.Euler_Maruyama_sampler(*a, num_steps=5, use_graph=False, **kw)
    out["pc"] = S.pc_sampler(*a, num_steps=3, **kw)
torch.save({k: v.cpu() for k, v in out.items()}, sys.argv[2])
"""


def test_network_matches_the_projection_path(tmp_path):
    """composed final block (default) against SBGM_NO_FINAL_COMPOSE=1 in fresh processes (the switch is read once), same seed; and
    with the composed path on, graph replay equals the eager launches bit for bit"""
    outs = {}
    for tag, env in (("composed", {}), ("projection", {"SBGM_NO_FINAL_COMPOSE": "1"})):
        path = str(tmp_path / f"{tag}.pt")
        base = {k: v for k, v in os.environ.items() if k != "SBGM_NO_FINAL_COMPOSE"}
        r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, path], env=dict(base, **env), capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[tag] = torch.load(path, weights_only=True)
    for kind, tol in (("forward", TOL), ("em", SAMPLER_TOL), ("pc", SAMPLER_TOL)):
        assert torch.isfinite(outs["composed"][kind]).all()
        check_parity(outs["composed"][kind], outs["projection"][kind], tol, f"final compose vs projection, {kind}")
    assert not torch.equal(outs["composed"]["forward"], outs["projection"]["forward"])      # the switch selects another computation
    assert not torch.equal(outs["composed"]["em"], outs["projection"]["em"])
    assert torch.equal(outs["composed"]["forward_plain"], outs["projection"]["forward_plain"])      # the plain forward keeps the projection path
    assert torch.equal(outs["composed"]["em"], outs["composed"]["em_eager"])


def _em(net, c, steps=3, seed=11):
    import sbgm_danra_amd as S
    with torch.no_grad():
        return S.Euler_Maruyama_sampler(net, S.marginal_prob_std_fn, S.diffusion_coeff_fn, batch_size=c.shape[0], num_steps=steps,
                                        device=DEV, img_size=c.shape[-1], cond_img=c, seed=seed).cpu()


def test_weight_updates_reach_the_composed_block():
    """after an in-place update of a final_layer tensor (what the EMA swap does) the next sampler call, on the cached step graph,
    equals a fresh model with those weights bit for bit; and so after a load_state_dict back"""
    _, net, sd = build_pair(1)
    _, fresh, _ = build_pair(1)
    net.eval(), fresh.eval()
    c = torch.randn(2, 1, 64, 64, generator=torch.Generator().manual_seed(31)).cuda()
    before = _em(net, c)
    cur = dict(sd)
    fin = net.decoder.final_layer
    for key, p in (("conv_up.weight", fin.conv_up.weight), ("conv_up.bias", fin.conv_up.bias), ("conv.weight", fin.conv.weight)):
        last = _em(net, c)
        with torch.no_grad():
            p.mul_(0.5)
        after = _em(net, c)
        cur["decoder.final_layer." + key] = cur["decoder.final_layer." + key] * 0.5
        fresh.load_state_dict(cur)
        assert not torch.equal(last, after), key
        assert torch.equal(after, _em(fresh, c)), key
    net.load_state_dict(sd)
    assert torch.equal(_em(net, c), before)


def test_evaluations_after_a_training_step_use_the_new_weights():
    """a training step (which must not rebuild the composed images itself) followed by an eval forward and a sampler call: both
    equal a fresh model loaded with the stepped weights bit for bit"""
    _, net, _ = build_pair(1)
    net.eval()
    g = torch.Generator().manual_seed(41)
    x, c = torch.randn(2, 1, 64, 64, generator=g).cuda(), torch.randn(2, 1, 64, 64, generator=g).cuda()
    t = (torch.rand(2, generator=g) * 0.9 + 0.05).cuda()
    with torch.no_grad():
        before = net(x, t, cond_img=c).cpu()
    em_before = _em(net, c)
    w_before = net.decoder.final_layer.conv_up.weight.detach().clone()
    opt = torch.optim.SGD(net.parameters(), lr=1e-6)
    net(x, t, cond_img=c).square().mean().backward()
    opt.step()
    assert not torch.equal(w_before, net.decoder.final_layer.conv_up.weight.detach())
    with torch.no_grad():
        after = net(x, t, cond_img=c).cpu()
    em_after = _em(net, c)
    _, fresh, _ = build_pair(1)
    fresh.eval()
    fresh.load_state_dict({k: v.detach().clone() for k, v in net.state_dict().items()})
    with torch.no_grad():
        want = fresh(x, t, cond_img=c).cpu()
    assert not torch.equal(before, after) and not torch.equal(em_before, em_after)
    assert torch.equal(after, want)
    assert torch.equal(em_after, _em(fresh, c))
