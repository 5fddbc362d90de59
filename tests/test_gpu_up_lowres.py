"""A small-map decoder block's conv_up at low resolution (csrc/conv_uplow.hip): conv_up(up(x)) as a 1x1 product to the 9 taps on the
LOW-resolution map and a gather through the bilinear x2 that also forms norm1 where a workgroup holds a whole (sample, group).  The
pack against the source weight, the block alone against the fp64 CPU chain (random, one-hot and zero inputs, raw and with GroupNorm,
fused and through the partial-statistics fallback), and the whole network against today's path (SBGM_NO_UP_LOWRES=1).  The step
samplers and the profiled forward take this route; the plain forward and RK45 keep the convolution on the upsampled map."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from sbgm_danra_amd import _native as N
from util_models import check_parity
from util_up_lowres import taps_weight, up_lowres_reference

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
TOL = 1e-4              # the project's per-evaluation tolerance
SAMPLER_TOL = 1e-3      # the project's short-horizon sampler tolerance
BOUND = 2e-5            # the project's bound for a kernel against fp64 (test_gpu_final_lowres.py)
EPS = 1e-5


def relerr(got, want):
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-30))


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return torch.randn(*shape, generator=g) * scale


def weights(c, seed=1):
    """conv_up's weight and bias, norm1's gamma and beta"""
    return rnd(c, c, 3, 3, seed=seed, scale=(9 * c) ** -0.5), rnd(c, seed=seed + 1, scale=0.5), rnd(c, seed=seed + 2).abs() + 0.5, rnd(c, seed=seed + 3)


def chain(x, w, b, groups=0, gamma=None, beta=None):
    """group_norm(conv_up(interpolate(x))) in fp64 on the CPU"""
    up = F.interpolate(x.double(), scale_factor=2, mode="bilinear", align_corners=False)
    out = F.conv2d(up, w.double(), b.double(), padding=1)
    if groups:
        out = F.group_norm(out, groups, None if gamma is None else gamma.double(), None if beta is None else beta.double(), eps=EPS)
    return out.float()


class Block:
    """the block's device operands: the mix's 1x1 weight (plain and packed)"""

    def __init__(self, w):
        lib, c = N.lib(), w.shape[0]
        self.c = c
        n = lib.sbgm_up_lowres_weight_numel(c)
        assert n == 9 * c * c
        self.taps = torch.full((n,), float("nan"), device=DEV)
        self.packed = torch.full((n,), float("nan"), device=DEV)
        N.check(lib.sbgm_up_lowres_pack(w.contiguous().to(DEV).data_ptr(), self.taps.data_ptr(), self.packed.data_ptr(), c, N.stream()))
        torch.cuda.synchronize()

    def run(self, x, b, groups=0, gamma=None, beta=None):
        """x: low-resolution NCHW (CPU) -> the block's output NCHW [B,C,2h,2w] (CPU); output and workspace start as NaN, so an element
        that is read but never written shows"""
        B, c, h, w = x.shape
        H, W = 2 * h, 2 * w
        lib = N.lib()
        xd = x.permute(0, 2, 3, 1).contiguous().to(DEV)
        dev = lambda t: None if t is None else t.contiguous().to(DEV)  # noqa: E731
        bd, gd, btd = dev(b), dev(gamma), dev(beta)
        ws = torch.full((lib.sbgm_up_lowres_ws_numel(B, H, W, c, groups),), float("nan"), device=DEV)
        out = torch.full((B, H, W, c), float("nan"), device=DEV)
        N.check(lib.sbgm_up_lowres_fwd(xd.data_ptr(), self.packed.data_ptr(), bd.data_ptr(), N.ptr(gd), N.ptr(btd), groups, EPS,
                                       out.data_ptr(), ws.data_ptr(), ws.numel(), B, H, W, c, N.stream()))
        torch.cuda.synchronize()
        return out.permute(0, 3, 1, 2).cpu()


@pytest.fixture(scope="module")
def block64():
    w = weights(64)
    return w, Block(w[0])


def test_pack_copies_every_weight_element():
    c = 32
    w = weights(c, seed=11)[0]
    blk = Block(w)
    w1 = taps_weight(w)                                               # [9c][c], row tap * c + co
    assert torch.equal(blk.taps.cpu().view(9 * c, c), w1)
    img = blk.packed.cpu().view(c // 16, 9 * c, 16)                    # the implicit-GEMM image [k step][row][16]
    assert torch.equal(img.permute(1, 0, 2).reshape(9 * c, c), w1)


# (low-res map, C, groups): C = 64 in 8 groups on 1x1 (everything clamped), 2x3 and 5x7 (non-square, odd), 4x4 and 8x8 (the two maps of the
# 128 x 128 network); C = 32 (4-channel groups); 16x16 with 32-channel groups, whose 288 KiB of Z rows per (sample, group) do not fit one
# workgroup's LDS: row chunks and partial statistics; 64 one-channel groups, which no channel-quad slice can hold: the raw map and the
# separate statistics pass
CASES = [((1, 1), 64, 8), ((2, 3), 64, 8), ((4, 4), 64, 8), ((5, 7), 64, 8), ((8, 8), 64, 8), ((4, 4), 32, 8), ((16, 16), 64, 2), ((4, 4), 64, 64)]


@pytest.mark.parametrize("norm", [False, True], ids=["raw", "groupnorm"])
@pytest.mark.parametrize("hw,c,groups", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_block_matches_fp64_chain(block64, hw, c, groups, norm):
    if c == 64:
        (w, b, gamma, beta), blk = block64
    else:
        w, b, gamma, beta = weights(c)
        blk = Block(w)
    x = rnd(2, c, *hw, seed=2)
    kw = dict(groups=groups, gamma=gamma, beta=beta) if norm else {}
    want = chain(x, w, b, **kw)
    got = blk.run(x, b, **kw)
    assert got.shape == want.shape and torch.isfinite(got).all()
    err = relerr(got, want)
    print(f"low-res conv_up {hw} C={c} groups={groups if norm else 0}: max-rel {err:.2e} against the fp64 chain (bound {BOUND:.0e})")
    assert err < BOUND


def test_block_matches_its_own_formulation(block64):
    """the kernels against the fp64 statement of their own formulation (tests/util_up_lowres.py): the same bound"""
    (w, b, gamma, beta), blk = block64
    x = rnd(2, 64, 5, 7, seed=9)
    err = relerr(blk.run(x, b, 8, gamma, beta), up_lowres_reference(x, w, b, 8, gamma, beta, EPS).float())
    print(f"low-res conv_up against its fp64 formulation: max-rel {err:.2e}")
    assert err < BOUND


def test_norm_without_affine(block64):
    (w, b, _, _), blk = block64
    x = rnd(2, 64, 4, 4, seed=5)
    err = relerr(blk.run(x, b, 8), chain(x, w, b, 8))
    print(f"low-res conv_up, GroupNorm without affine: max-rel {err:.2e}")
    assert err < BOUND


@pytest.mark.parametrize("h,w", [(5, 7), (16, 16)])
def test_block_one_hot_inputs(block64, h, w):
    """single low-resolution pixels: the four corners, the first two and last two rows and columns, an interior point (16x16: in row
    chunks): a wrong clamp, shift or padding test shows as a misplaced or missing copy of the filter"""
    (wt, _, _, _), blk = block64
    pts = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)]
    pts += [(r, w // 2) for r in (0, 1, h - 2, h - 1)] + [(h // 2, c) for c in (0, 1, w - 2, w - 1)]
    pts += [(1, 1), (h - 2, w - 2), (h // 2, w // 2)]
    x = torch.zeros(len(pts), 64, h, w)
    for i, (py, px) in enumerate(pts):
        x[i, (7 * i) % 64, py, px] = 1.0
    zb = torch.zeros(64)
    want = chain(x, wt, zb)
    got = blk.run(x, zb)
    assert torch.isfinite(got).all()
    worst = max(relerr(got[i], want[i]) for i in range(len(pts)))
    print(f"one-hot {h}x{w}: worst max-rel {worst:.2e} over {len(pts)} points")
    for i in range(len(pts)):
        assert relerr(got[i], want[i]) < BOUND, pts[i]
    if (h, w) == (16, 16):       # one group of 64 channels: the gather runs in row chunks of 4 output rows, so every point above meets a chunk edge
        got_n, want_n = blk.run(x, zb, 1), chain(x, wt, zb, 1)
        for i in range(len(pts)):
            assert relerr(got_n[i], want_n[i]) < BOUND, pts[i]


def test_zero_input_leaves_the_bias(block64):
    (_, b, _, _), blk = block64
    got = blk.run(torch.zeros(2, 64, 5, 7), b)
    assert torch.equal(got, b[None, :, None, None].expand(2, 64, 10, 14))


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


def test_network_matches_the_convolution_on_the_upsampled_map(tmp_path):
    """low-resolution route (default) against SBGM_NO_UP_LOWRES=1 in fresh processes (the switch is read once), same seed; and on the
    new route graph replay equals the eager launches bit for bit"""
    outs = {}
    for tag, env in (("lowres", {}), ("parent", {"SBGM_NO_UP_LOWRES": "1"})):
        path = str(tmp_path / f"{tag}.pt")
        base = {k: v for k, v in os.environ.items() if k != "SBGM_NO_UP_LOWRES"}
        r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, path], env=dict(base, **env), capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[tag] = torch.load(path, weights_only=True)
    for kind, tol in (("forward", TOL), ("em", SAMPLER_TOL), ("pc", SAMPLER_TOL)):
        assert torch.isfinite(outs["lowres"][kind]).all()
        check_parity(outs["lowres"][kind], outs["parent"][kind], tol, f"conv_up low-res vs upsampled map, {kind}")
        assert not torch.equal(outs["lowres"][kind], outs["parent"][kind])             # the switch selects another computation
    assert torch.equal(outs["lowres"]["forward_plain"], outs["parent"]["forward_plain"])    # the plain forward keeps today's path
    assert torch.equal(outs["lowres"]["em"], outs["lowres"]["em_eager"])
