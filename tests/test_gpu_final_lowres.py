"""The final block mixed at low resolution (csrc/conv_final.hip: final_mix + final_gather): conv(conv_up(up(x))) as a 1x1 product to
the 25 positions of the composed 5x5 stencil on the LOW-resolution map and a gather through the bilinear x2, with nine border-class
weight sets.  The pack against the fp64 sums, the block alone against the fp64 CPU chain (random, one-hot and zero inputs, plain and
with the normalisation applied on load), and the whole network against the composed 3x3 route (SBGM_NO_FINAL_LOWRES=1).  The step
samplers and the profiled forward take this route; the plain forward and RK45 keep the projection path (engine.h, set_routes)."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from sbgm_danra_amd import _native as N
from util_final_lowres import class_sets, lowres_reference
from util_models import check_parity

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
TOL = 1e-4              # the project's per-evaluation tolerance
SAMPLER_TOL = 1e-3      # the project's short-horizon sampler tolerance
BOUND = 2e-5            # the project's bound for a kernel against fp64 (test_gpu_final_compose.py)
C = 64


def relerr(got, want):
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-30))


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return torch.randn(*shape, generator=g) * scale


def weights(seed=1, c=C):
    s = (9 * c) ** -0.5
    return rnd(c, c, 3, 3, seed=seed, scale=s), rnd(c, seed=seed + 1, scale=0.5), rnd(1, c, 3, 3, seed=seed + 2, scale=s), rnd(1, seed=seed + 3)


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


class Block:
    """the block's device operands: Wz of the nine classes (plain and packed) and beta"""

    def __init__(self, w1, b1, w2, b2):
        lib, c = N.lib(), w1.shape[0]
        self.c = c
        self.wz = torch.full((9, 25, c), float("nan"), device=DEV)
        self.beta = torch.full((9,), float("nan"), device=DEV)
        self.packed = torch.full((lib.sbgm_final_lowres_packed_numel(c),), float("nan"), device=DEV)
        ops = [t.contiguous().to(DEV) for t in (w1, b1, w2, b2)]
        N.check(lib.sbgm_final_lowres_pack(*[t.data_ptr() for t in ops], self.wz.data_ptr(), self.beta.data_ptr(), self.packed.data_ptr(),
                                           c, N.stream()))
        torch.cuda.synchronize()

    def run(self, x, scale=None, shift=None, skip=None, act=N.NONE):
        """x: low-resolution NCHW (CPU) -> the block's output [B,1,2h,2w] (CPU); the workspace starts as NaN, so a strip pixel that is
        read but never written shows in the output"""
        B, c, h, w = x.shape
        H, W = 2 * h, 2 * w
        nhwc = lambda t: None if t is None else t.permute(0, 2, 3, 1).contiguous().to(DEV)  # noqa: E731
        xd, sk = nhwc(x), nhwc(skip)
        aff = None
        if scale is not None:                     # [B][c/4][2][4]: scale quad, shift quad
            aff = torch.stack([scale.view(B, c // 4, 4), shift.view(B, c // 4, 4)], dim=2).contiguous().to(DEV)
        ws = torch.full((N.lib().sbgm_final_lowres_ws_numel(B, H, W),), float("nan"), device=DEV)
        out = torch.full((B, 1, H, W), float("nan"), device=DEV)
        N.check(N.lib().sbgm_final_lowres_fwd(xd.data_ptr(), N.ptr(aff), N.ptr(sk), act, self.packed.data_ptr(), self.beta.data_ptr(), None,
                                              1.0, out.data_ptr(), ws.data_ptr(), ws.numel(), B, H, W, c, N.stream()))
        torch.cuda.synchronize()
        return out.cpu()


@pytest.fixture(scope="module")
def block():
    w = weights()
    return w, Block(*w)


def test_pack_matches_fp64_sums_for_all_nine_classes():
    w = weights(seed=11)
    blk = Block(*w)
    want_w, want_b = class_sets(*w)

    def ulps(got, want):                       # distance in units of the last place of `want`
        want = want.float()
        spacing = torch.nextafter(want.abs(), torch.full_like(want, float("inf"))) - want.abs()
        return float(((got - want).abs() / spacing).max())
    uw, ub = ulps(blk.wz.cpu(), want_w), ulps(blk.beta.cpu(), want_b)
    print(f"low-res pack: weights within {uw:.1f} ulp, beta within {ub:.1f} ulp of the fp64 sums")
    assert uw <= 1.0 and ub <= 1.0
    img = blk.packed.cpu().view(9, C // 16, 32, 16)            # [class][k step][row][16]
    assert torch.equal(img[:, :, 25:], torch.zeros(9, C // 16, 7, 16))
    assert torch.equal(img[:, :, :25].permute(0, 2, 1, 3).reshape(9, 25, C), blk.wz.cpu())


def on_load_terms(B, c, h, w):
    scale, shift, skip = rnd(B, c, seed=3).abs() + 0.5, rnd(B, c, seed=4), rnd(B, c, h, w, seed=5)
    return dict(scale=scale, shift=shift, skip=skip, act=N.SILU), dict(scale=scale, shift=shift, skip=skip, silu=True)


# the smallest maps with interior, strip and corner classes and a gather-tile boundary (16 x 32 outputs) inside the map; 12x24 is
# non-square with partial tiles on both axes; 8x8 is the width at which the decoder has nothing pending
CASES = [((2, 16, 16), 64, False), ((2, 16, 16), 64, True), ((2, 12, 24), 64, False), ((2, 12, 24), 64, True), ((2, 8, 8), 64, False),
         ((1, 16, 16), 32, True)]


@pytest.mark.parametrize("shape,c,on_load", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_block_matches_fp64_chain(block, shape, c, on_load):
    if c == C:
        w, blk = block
    else:
        w = weights(c=c)
        blk = Block(*w)
    B, h, wd = shape
    x = rnd(B, c, h, wd, seed=2)
    kw, ckw = on_load_terms(B, c, h, wd) if on_load else ({}, {})
    want = chain(x, *w, **ckw)
    got = blk.run(x, **kw)
    assert got.shape == want.shape and torch.isfinite(got).all()
    err = relerr(got, want)
    print(f"low-res final block {shape} C={c} on_load={on_load}: max-rel {err:.2e} against the fp64 chain (bound {BOUND:.0e})")
    assert err < BOUND


def test_block_matches_the_lowres_reference(block):
    """the kernels against the fp64 statement of their own formulation (tests/util_final_lowres.py), tighter than the chain's rounding
    of two convolutions would need: the same bound"""
    w, blk = block
    x = rnd(2, C, 12, 24, seed=9)
    err = relerr(blk.run(x), lowres_reference(x, *w).float())
    print(f"low-res final block against its fp64 formulation: max-rel {err:.2e}")
    assert err < BOUND


@pytest.mark.parametrize("h,w", [(16, 16), (12, 24)])
def test_block_one_hot_inputs(block, h, w):
    """single low-resolution pixels: the four corners, rows / columns 0, 1, 2 and n-3, n-2, n-1 along two edges, and interior points
    on either side of a gather-tile boundary (low-res row 8, column 16): a wrong class, clamp or shift shows as a misplaced or missing
    copy of the filter"""
    (w1, b1, w2, b2), _ = block
    pts = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)]
    pts += [(r, 0) for r in (1, 2, h - 3, h - 2)] + [(h - 1, c) for c in (1, 2, w - 3, w - 2)]
    pts += [(r, w // 2) for r in (0, 1, 2, h - 3, h - 2)] + [(h // 2, c) for c in (0, 1, 2, w - 3, w - 2, w - 1)]
    pts += [(7, 5), (8, 5), (7, 8), (8, 7), (5, min(15, w - 4)), (5, min(16, w - 3))]
    x = torch.zeros(len(pts), C, h, w)
    for i, (py, px) in enumerate(pts):
        x[i, (7 * i) % C, py, px] = 1.0
    zb1, zb2 = torch.zeros_like(b1), torch.zeros_like(b2)
    want = chain(x, w1, zb1, w2, zb2)
    got = Block(w1, zb1, w2, zb2).run(x)
    assert torch.isfinite(got).all()
    worst = max(relerr(got[i], want[i]) for i in range(len(pts)))
    print(f"one-hot {h}x{w}: worst max-rel {worst:.2e} over {len(pts)} points")
    for i in range(len(pts)):
        assert relerr(got[i], want[i]) < BOUND, pts[i]


def test_zero_input_leaves_beta_per_class(block):
    """zero input, non-zero b1: the output is beta[c] of the pixel's class; interior and corner values are b2 + the sum of bc over
    the valid taps and differ from each other"""
    (w1, b1, w2, b2), blk = block
    h = w = 16
    got = blk.run(torch.zeros(1, C, h, w))
    want = chain(torch.zeros(1, C, h, w), w1, b1, w2, b2)
    bc = torch.einsum("oyx,o->yx", w2[0].double(), b1.double())
    inner = float(b2.double() + bc.sum())
    corner = float(b2.double() + bc[1:, 1:].sum())
    err = relerr(got, want)
    print(f"beta alone {2 * h}x{2 * w}: max-rel {err:.2e}")
    assert torch.isfinite(got).all() and err < BOUND
    scale = float(want.abs().max())
    assert abs(float(got[0, 0, 5, 5]) - inner) < BOUND * scale and abs(float(got[0, 0, 0, 0]) - corner) < BOUND * scale
    assert abs(float(got[0, 0, 2 * h - 1, 2 * w - 1]) - float(b2.double() + bc[:2, :2].sum())) < BOUND * scale
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
    # one evaluation on the route the samplers take: the profiled forward
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


def test_network_matches_the_composed_3x3_route(tmp_path):
    """low-resolution route (default) against SBGM_NO_FINAL_LOWRES=1 in fresh processes (the switch is read once), same seed; and on
    the new route graph replay equals the eager launches bit for bit"""
    outs = {}
    for tag, env in (("lowres", {}), ("composed", {"SBGM_NO_FINAL_LOWRES": "1"})):
        path = str(tmp_path / f"{tag}.pt")
        base = {k: v for k, v in os.environ.items() if k not in ("SBGM_NO_FINAL_LOWRES", "SBGM_NO_FINAL_COMPOSE")}
        r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, path], env=dict(base, **env), capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[tag] = torch.load(path, weights_only=True)
    for kind, tol in (("forward", TOL), ("em", SAMPLER_TOL), ("pc", SAMPLER_TOL)):
        assert torch.isfinite(outs["lowres"][kind]).all()
        check_parity(outs["lowres"][kind], outs["composed"][kind], tol, f"final low-res vs composed 3x3, {kind}")
    assert not torch.equal(outs["lowres"]["forward"], outs["composed"]["forward"])          # the switch selects another computation
    assert not torch.equal(outs["lowres"]["em"], outs["composed"]["em"])
    assert torch.equal(outs["lowres"]["forward_plain"], outs["composed"]["forward_plain"])  # the plain forward keeps the projection path
    assert torch.equal(outs["lowres"]["em"], outs["lowres"]["em_eager"])
