"""The samplers' composed stem (conv_stem22.hip): conv2(conv1(in) + tb0) as one 22x22 / stride-4 correlation with 25 border classes.
The composed launch alone against the fp64 CPU chain (random inputs, one-hot inputs, the time-bias term alone), and the samplers
with the composed path against the two-convolution path (SBGM_NO_STEM_COMPOSE=1), graph replay, changing condition contents and
changing weights."""
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
TOL = 1e-4
BOUND = 2e-5            # the project's bound for a stem kernel against fp64 (test_gpu_stem_winograd.py)


def relerr(got, want):
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-30))


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return torch.randn(*shape, generator=g) * scale


def pack(w1, w2):
    lib, cin = N.lib(), w1.shape[1]
    wc = torch.empty(lib.sbgm_stem22_packed_numel(cin), device=DEV)
    s = torch.empty(lib.sbgm_stem22_bias_numel(), device=DEV)
    w1d, w2d = w1.contiguous().to(DEV), w2.contiguous().to(DEV)
    N.check(lib.sbgm_stem22_pack_weight(w1d.data_ptr(), w2d.data_ptr(), wc.data_ptr(), s.data_ptr(), cin, N.stream()))
    torch.cuda.synchronize()
    return wc, s


def launch(src, c0, cin, wc, s, tb0=None, addend=None, scale=None, bias=None, relu=False):
    """src NCHW (CPU) = the weight channels c0 .. c0 + src.shape[1] - 1 -> NCHW output of sbgm_stem22_fwd"""
    B, nch, H, W = src.shape
    dv = lambda t: None if t is None else t.contiguous().to(DEV)  # noqa: E731
    sd, tb, sc, bi = dv(src), dv(tb0), dv(scale), dv(bias)
    ad = None if addend is None else addend.permute(0, 2, 3, 1).contiguous().to(DEV)
    out = torch.full((B, H // 4, W // 4, 64), float("nan"), device=DEV)
    N.check(N.lib().sbgm_stem22_fwd(sd.data_ptr(), nch, c0, cin, wc.data_ptr(), s.data_ptr(), N.ptr(tb), N.ptr(ad), N.ptr(sc), N.ptr(bi),
                                    int(relu), out.data_ptr(), B, H, W, N.stream()))
    torch.cuda.synchronize()
    return out.cpu().permute(0, 3, 1, 2).contiguous()


def chain(u, w1, w2, tb0=None, extra=None, scale=None, bias=None, relu=False):
    """conv2(conv1(u) + tb0) in fp64 on the CPU (+ extra, folded BatchNorm, ReLU)"""
    f1 = F.conv2d(u.double(), w1.double(), None, 2, 3)
    if tb0 is not None:
        f1 = f1 + tb0.double()[:, :, None, None]
    y = F.conv2d(f1, w2.double(), None, 2, 3)
    if extra is not None:
        y = y + extra.double()
    if scale is not None:
        y = y * scale.double().view(1, -1, 1, 1)
    if bias is not None:
        y = y + bias.double().view(1, -1, 1, 1)
    if relu:
        y = F.relu(y)
    return y.float()


def weights(cin, seed=1):
    return rnd(64, cin, 8, 8, seed=seed, scale=(cin * 64) ** -0.5), rnd(64, 64, 8, 8, seed=seed + 1, scale=(64 * 64) ** -0.5)


CASES = [(1, 1, 64, 64), (2, 2, 64, 64), (32, 1, 128, 128), (32, 2, 128, 128), (16, 2, 256, 256), (2, 5, 32, 32), (2, 2, 64, 96)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("epilogue", [False, True])
def test_composed_launch_matches_fp64_chain(case, epilogue):
    """Without the epilogue: one launch over all input channels with the time-bias term.  With it: as a sampler runs it, the
    condition channels first (the once-per-run term T; a random tensor stands in for it when there is no condition channel), then
    channel 0 with tb0, + T, scale, bias and ReLU."""
    B, Cin, H, W = case
    u, tb0 = rnd(B, Cin, H, W), rnd(B, 64, seed=4)
    w1, w2 = weights(Cin)
    wc, s = pack(w1, w2)
    if not epilogue:
        got = launch(u, 0, Cin, wc, s, tb0=tb0)
        want = chain(u, w1, w2, tb0)
    else:
        scale, bias = rnd(64, seed=2).abs() + 0.5, rnd(64, seed=3)
        if Cin > 1:
            T, extra = launch(u[:, 1:], 1, Cin, wc, s), None
        else:
            T = extra = rnd(B, 64, H // 4, W // 4, seed=5)
        got = launch(u[:, :1], 0, Cin, wc, s, tb0=tb0, addend=T, scale=scale, bias=bias, relu=True)
        want = chain(u, w1, w2, tb0, extra, scale, bias, True)
    assert got.shape == want.shape and torch.isfinite(got).all()
    err = relerr(got, want)
    print(f"composed stem {case} epilogue={epilogue}: max-rel {err:.2e} against the fp64 chain (bound {BOUND:.0e})")
    assert err < BOUND


@pytest.mark.parametrize("H,W", [(64, 64), (64, 96)])
def test_composed_one_hot_inputs(H, W):
    """single input pixels at the corners, at rows / columns 0..12 and the last 13 of two edges, and in the interior: a wrong class
    table, tap range or pad shows as a misplaced or truncated copy of the filter"""
    w1, w2 = weights(1, seed=7)
    wc, s = pack(w1, w2)
    edge_r, edge_c = list(range(13)) + list(range(H - 13, H)), list(range(13)) + list(range(W - 13, W))
    pts = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]
    pts += [(r, 0) for r in edge_r] + [(0, c) for c in edge_c] + [(r, W - 1) for r in edge_r[::3]] + [(H - 1, c) for c in edge_c[::3]]
    pts += [(H // 2, W // 2), (H // 2 + 1, W // 2 - 3), (17, 22), (9, 9), (H - 10, W - 10)]
    u = torch.zeros(len(pts), 1, H, W)
    for i, (py, px) in enumerate(pts):
        u[i, 0, py, px] = 1.0
    got, want = launch(u, 0, 1, wc, s), chain(u, w1, w2)
    worst = max(relerr(got[i], want[i]) for i in range(len(pts)))
    print(f"one-hot {H}x{W}: worst max-rel {worst:.2e} over {len(pts)} points")
    for i in range(len(pts)):
        assert relerr(got[i], want[i]) < BOUND, pts[i]


def test_time_bias_term_alone():
    """zero input: the result is conv2 of the constant map tb0[b][ci], borders (fewer valid taps) included"""
    B, H, W = 3, 64, 96
    w1, w2 = weights(2, seed=9)
    wc, s = pack(w1, w2)
    tb0 = rnd(B, 64, seed=6)
    got = launch(torch.zeros(B, 2, H, W), 0, 2, wc, s, tb0=tb0)
    want = F.conv2d(tb0.double()[:, :, None, None].expand(B, 64, H // 2, W // 2), w2.double(), None, 2, 3).float()
    err = relerr(got, want)
    print(f"time-bias term alone: max-rel {err:.2e}")
    assert err < BOUND
    assert relerr(got[:, :, 0, 0], want[:, :, 0, 0]) < BOUND and relerr(got[:, :, -1, -2], want[:, :, -1, -2]) < BOUND


# ---- the samplers ------------------------------------------------------------------------------------------------------------------
GUIDED = {"classifier_free_guidance": {"enabled": True, "guidance_scale": 2.5, "guidance_scale_max": 1.5}}

_CHILD = r"""
import sys, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from util_models import build_pair
import sbgm_danra_amd as S
GUIDED = {"classifier_free_guidance": {"enabled": True, "guidance_scale": 2.5, "guidance_scale_max": 1.5}}
_, net, _ = build_pair(1)
net.eval()
g = torch.Generator().manual_seed(3)
c = torch.randn(2, 1, 64, 64, generator=g).cuda()
kw = dict(batch_size=2, device="cuda", img_size=64, cond_img=c, seed=5)
a = (net, S.marginal_prob_std_fn, S.diffusion_coeff_fn)
out = {}
with torch.no_grad():
    out["em"] = S.Euler_Maruyama_sampler(*a, num_steps=4, **kw)
    out["em_guided"] = S.Euler_Maruyama_sampler(*a, num_steps=4, cfg=GUIDED, **kw)
    out["em_eager"] = S.Euler_Maruyama_sampler(*a, num_steps=4, use_graph=False, **kw)
    out["pc"] = S.pc_sampler(*a, num_steps=3, **kw)
    out["edm_heun"] = S.edm_heun_sampler(*a, num_steps=4, **kw)
    out["rk45"] = S.rk45_sampler(*a, rtol=1e-2, atol=1e-2, **kw)
torch.save({k: v.cpu() for k, v in out.items()}, sys.argv[2])
"""


def test_samplers_match_the_two_convolution_path(tmp_path):
    """every sampler kind, composed stem (default) against SBGM_NO_STEM_COMPOSE=1 in fresh processes, same seed (RK45 keeps the
    two-convolution stem on both sides: its Python loop must stay one computation with the native one); and with the composed path
    on, graph replay equals the eager launches bit for bit"""
    outs = {}
    for tag, env in (("composed", {}), ("two_conv", {"SBGM_NO_STEM_COMPOSE": "1"})):
        path = str(tmp_path / f"{tag}.pt")
        base = {k: v for k, v in os.environ.items() if k != "SBGM_NO_STEM_COMPOSE"}
        r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, path], env=dict(base, **env), capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[tag] = torch.load(path, weights_only=True)
    for kind in ("em", "em_guided", "pc", "edm_heun", "rk45"):
        assert torch.isfinite(outs["composed"][kind]).all()
        check_parity(outs["composed"][kind], outs["two_conv"][kind], TOL, f"stem compose vs two convolutions, {kind}")
    assert torch.equal(outs["composed"]["em"], outs["composed"]["em_eager"])


def _em(net, c, steps=3, seed=11):
    import sbgm_danra_amd as S
    with torch.no_grad():
        return S.Euler_Maruyama_sampler(net, S.marginal_prob_std_fn, S.diffusion_coeff_fn, batch_size=c.shape[0], num_steps=steps,
                                        device=DEV, img_size=c.shape[-1], cond_img=c, seed=seed).cpu()


def test_condition_contents_change_at_the_same_address():
    """two graphed runs on one model whose condition tensor is rewritten in place between them: the second run equals a fresh
    model's run on the new contents (the once-per-run condition term is rebuilt on every call, outside the cached step graph)"""
    _, net, _ = build_pair(1)
    _, fresh, _ = build_pair(1)
    net.eval(), fresh.eval()
    g = torch.Generator().manual_seed(21)
    c1, c2 = torch.randn(2, 1, 64, 64, generator=g), torch.randn(2, 1, 64, 64, generator=g)
    c = c1.cuda()
    first = _em(net, c)
    c.copy_(c2)
    second = _em(net, c)
    want = _em(fresh, c2.cuda())
    assert not torch.equal(first, second)
    assert torch.equal(second, want)


@pytest.mark.parametrize("which", ["conv1", "conv2"])
def test_weight_updates_reach_the_composed_stem(which):
    """after an in-place update or a load_state_dict of a stem weight the next sampler call runs on the new composed filter"""
    _, net, sd = build_pair(1)
    net.eval()
    c = torch.randn(2, 1, 64, 64, generator=torch.Generator().manual_seed(31)).cuda()
    before = _em(net, c)
    key = f"encoder.{which}.weight"
    with torch.no_grad():
        getattr(net.encoder, which).weight.mul_(0.5)
    after = _em(net, c)
    sd2 = {k: (v * 0.5 if k == key else v) for k, v in sd.items()}
    _, fresh, _ = build_pair(1)
    fresh.eval()
    fresh.load_state_dict(sd2)
    want = _em(fresh, c)
    assert not torch.equal(before, after)
    assert torch.equal(after, want)
    net.load_state_dict(sd)                                   # and back, through load_state_dict
    assert torch.equal(_em(net, c), before)


def test_a_run_leaves_nothing_behind():
    """a plain eval-mode forward gives the same bits before and after a graphed EM run and a sampler call the engine refuses once its
    routes are set (tile origins with a domain narrower than the tile): neither leaves the composed routes or a truncated workspace
    on the model"""
    import sbgm_danra_amd as S
    _, net, _ = build_pair(1)
    net.eval()
    g = torch.Generator().manual_seed(41)
    x, c = torch.randn(2, 1, 32, 32, generator=g).cuda(), torch.randn(2, 1, 32, 32, generator=g).cuda()
    t = (torch.rand(2, generator=g) * 0.9 + 0.05).cuda()

    def forward():
        with torch.no_grad():
            return net(x, t, cond_img=c).cpu()

    first = forward()
    assert torch.isfinite(_em(net, c)).all()
    handle = net._engine(None, None, c).h
    ws_bytes = N.lib().sbgm_model_workspace_bytes(handle)
    with pytest.raises(N.NativeError):
        S.Euler_Maruyama_sampler(net, S.marginal_prob_std_fn, S.diffusion_coeff_fn, batch_size=2, num_steps=3, device=DEV, img_size=32,
                                 cond_img=c, seed=11, tile_origins=torch.zeros(2, 2, dtype=torch.int32).cuda(), domain_width=16)
    assert N.lib().sbgm_model_workspace_bytes(handle) == ws_bytes
    assert torch.equal(forward(), first)
