"""The decoder's last skip formed inside the final mix (csrc/conv_final.hip: final_mix_kernel<4, true>, skip_from_x): the step samplers
launch neither pack_input nor conv1; the mix computes conv1(x || cond) + tb0 at its pixel as the run's condition share Sc + tb0 + the
x share, 16 MFMA k steps over the planar input.  The pack against the host model, mix + gather through the C entries against the fp64
CPU chain conv(conv_up(up(SiLU(raw * scale + shift + conv1(x || cond) + tb0)))), and the whole network against SBGM_NO_SKIP_MIX=1."""
import pytest
import torch

from sbgm_danra_amd import _native as N
from util_models import check_parity, maxrel
from util_skip_mix import chain, pack_w1x, skip_parts
from util_skip_mix_runs import B as RUN_B, HW as RUN_HW, run

pytestmark = pytest.mark.gpu

DEV = "cuda"
SAMPLER_TOL = 1e-3      # the project's short-horizon sampler tolerance
BOUND = 2e-5            # the project's bound for a kernel against fp64 (test_gpu_final_lowres.py)
C = 64


def relerr(got, want):
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-30))


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return torch.randn(*shape, generator=g) * scale


def final_weights(seed=1):
    s = (9 * C) ** -0.5
    return rnd(C, C, 3, 3, seed=seed, scale=s), rnd(C, seed=seed + 1, scale=0.5), rnd(1, C, 3, 3, seed=seed + 2, scale=s), rnd(1, seed=seed + 3)


def stem_weight(cin, seed=21):
    return rnd(C, cin, 8, 8, seed=seed, scale=(64 * cin) ** -0.5)


class Block:
    """the device operands of the final block (Wz of the nine classes, beta) and of the skip (w1x)"""

    def __init__(self, fw, w1):
        lib = N.lib()
        self.fw, self.w1 = fw, w1
        self.beta = torch.full((9,), float("nan"), device=DEV)
        self.packed = torch.full((lib.sbgm_final_lowres_packed_numel(C),), float("nan"), device=DEV)
        ops = [t.contiguous().to(DEV) for t in fw]
        N.check(lib.sbgm_final_lowres_pack(*[t.data_ptr() for t in ops], None, self.beta.data_ptr(), self.packed.data_ptr(), C, N.stream()))
        self.w1x = torch.full((lib.sbgm_skip_mix_packed_numel(),), float("nan"), device=DEV)
        w1d = w1.contiguous().to(DEV)
        N.check(lib.sbgm_skip_mix_pack(w1d.data_ptr(), self.w1x.data_ptr(), w1.shape[1], N.stream()))
        torch.cuda.synchronize()

    def run(self, raw, scale, shift, x, sc, tb0):
        """raw [B][64][h][w], x [B][1][2h][2w], sc [B][64][h][w] or None (all CPU) -> the block's output [B][1][2h][2w] (CPU); the
        workspace starts as NaN, so a strip pixel that is read but never written shows in the output"""
        Bn, c, h, w = raw.shape
        H, W = 2 * h, 2 * w
        nhwc = lambda t: None if t is None else t.permute(0, 2, 3, 1).contiguous().to(DEV)  # noqa: E731
        rd, sd, xd, td = nhwc(raw), nhwc(sc), x.contiguous().to(DEV), tb0.contiguous().to(DEV)
        aff = torch.stack([scale.view(Bn, c // 4, 4), shift.view(Bn, c // 4, 4)], dim=2).contiguous().to(DEV)
        ws = torch.full((N.lib().sbgm_final_lowres_ws_numel(Bn, H, W),), float("nan"), device=DEV)
        out = torch.full((Bn, 1, H, W), float("nan"), device=DEV)
        N.check(N.lib().sbgm_final_lowres_skip_fwd(rd.data_ptr(), aff.data_ptr(), N.SILU, self.packed.data_ptr(), self.beta.data_ptr(),
                                                   xd.data_ptr(), N.ptr(sd), td.data_ptr(), self.w1x.data_ptr(), None, 1.0, out.data_ptr(),
                                                   ws.data_ptr(), ws.numel(), Bn, H, W, c, N.stream()))
        torch.cuda.synchronize()
        return out.cpu()


@pytest.fixture(scope="module")
def blocks():
    fw = final_weights()
    return {cin: Block(fw, stem_weight(cin)) for cin in (1, 2, 5)}


def operands(Bn, h, w, cin, seed=2):
    raw, x = rnd(Bn, C, h, w, seed=seed), rnd(Bn, 1, 2 * h, 2 * w, seed=seed + 1)
    cond = rnd(Bn, cin - 1, 2 * h, 2 * w, seed=seed + 2) if cin > 1 else None
    return raw, rnd(Bn, C, seed=seed + 3).abs() + 0.5, rnd(Bn, C, seed=seed + 4), x, cond, rnd(Bn, C, seed=seed + 5, scale=0.5)


def want_and_got(blk, raw, scale, shift, x, cond, tb0):
    whole, _, cpart = skip_parts(blk.w1, x, cond, tb0)
    want = chain(raw, scale, shift, whole, *blk.fw).float()
    got = blk.run(raw, scale, shift, x, None if cpart is None else cpart.float(), tb0)
    assert got.shape == want.shape and torch.isfinite(got).all()
    return want, got


def test_pack_equals_the_host_image(blocks):
    for cin, blk in blocks.items():
        assert torch.equal(blk.w1x.cpu().view(16, 64, 4), pack_w1x(blk.w1)), cin


# the smallest maps with interior, strip and corner classes and a gather-tile boundary (16 x 32 outputs) inside the map: low-res 12 x 24
# (input 24 x 48), and a ragged 20 x 28 whose 16-pixel fragments straddle rows; 1 input channel: no condition, a null Sc
@pytest.mark.parametrize("h,w", [(12, 24), (20, 28)])
@pytest.mark.parametrize("cin", [2, 5, 1])
def test_block_matches_fp64_chain(blocks, h, w, cin):
    blk = blocks[cin]
    want, got = want_and_got(blk, *operands(2, h, w, cin))
    err = relerr(got, want)
    print(f"skip in the mix, low-res {h}x{w}, C_in={cin}: max-rel {err:.2e} against the fp64 chain (bound {BOUND:.0e})")
    assert err < BOUND


@pytest.mark.parametrize("h,w", [(12, 24), (20, 28)])
def test_one_hot_x_at_the_borders(blocks, h, w):
    """single input pixels, everything else zero, so the output is the block's answer to SiLU(conv1_x(one-hot)): the four corners, a
    point on each edge, and columns W - 1 / 0 of neighbouring rows (a tap that wrapped into the next row would see them)"""
    blk = blocks[1]
    H, W = 2 * h, 2 * w
    pts = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2 + 1), (H // 2, 0), (H // 2 + 1, W - 1),
           (5, W - 1), (6, 0), (H - 3, W - 2), (H - 2, 1), (2, 3), (15, 31), (16, 32)]
    x = torch.zeros(len(pts), 1, H, W)
    for i, (py, px) in enumerate(pts):
        x[i, 0, py, px] = 4.0
    n = len(pts)
    raw, tb0 = torch.zeros(n, C, h, w), torch.zeros(n, C)
    want, got = want_and_got(blk, raw, torch.ones(n, C), torch.zeros(n, C), x, None, tb0)
    worst = max(relerr(got[i], want[i]) for i in range(n))
    print(f"one-hot x {H}x{W}: worst max-rel {worst:.2e} over {n} points")
    for i in range(n):
        assert relerr(got[i], want[i]) < BOUND, pts[i]


@pytest.mark.parametrize("h,w", [(12, 24)])
def test_one_hot_raw(blocks, h, w):
    """single low-resolution pixels of the raw map under a live skip, as test_gpu_final_lowres.py has them: corners, the rows / columns
    next to the edges, and interior points on either side of a gather-tile boundary (low-res row 8, column 16)"""
    blk = blocks[2]
    pts = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)]
    pts += [(r, 0) for r in (1, 2, h - 3, h - 2)] + [(h - 1, c) for c in (1, 2, w - 3, w - 2)]
    pts += [(r, w // 2) for r in (0, 1, 2, h - 3, h - 2)] + [(h // 2, c) for c in (0, 1, 2, w - 3, w - 2, w - 1)]
    pts += [(7, 5), (8, 5), (7, 8), (8, 7), (5, min(15, w - 4)), (5, min(16, w - 3))]
    n = len(pts)
    _, scale, shift, x, cond, tb0 = operands(n, h, w, 2, seed=6)
    raw = torch.zeros(n, C, h, w)
    for i, (py, px) in enumerate(pts):
        raw[i, (7 * i) % C, py, px] = 8.0
    want, got = want_and_got(blk, raw, scale, shift, x, cond, tb0)
    worst = max(relerr(got[i], want[i]) for i in range(n))
    print(f"one-hot raw {h}x{w}: worst max-rel {worst:.2e} over {n} points")
    for i in range(n):
        assert relerr(got[i], want[i]) < BOUND, pts[i]


# ---- the whole network ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("skip_mix")
    return run({}, d / "mix.npz"), run({"SBGM_NO_SKIP_MIX": "1"}, d / "conv1.npz")


def t_(a):
    return torch.from_numpy(a)


def test_samplers_match_the_conv1_route(runs):
    mix, ref = runs
    for kind in ("em", "pc", "guided", "cond4", "nocond"):
        assert torch.isfinite(t_(mix[kind])).all()
        check_parity(t_(mix[kind]), t_(ref[kind]), SAMPLER_TOL, f"skip in the mix vs conv1 launch, {kind}")
    assert not (mix["em"] == ref["em"]).all() and not (mix["pc"] == ref["pc"]).all()      # the switch selects another computation


def test_plain_forward_is_untouched(runs):
    mix, ref = runs
    assert (mix["forward"] == ref["forward"]).all() and (mix["forward_after"] == ref["forward_after"]).all()
    assert (mix["forward"] == mix["forward_after"]).all()


def test_graph_replay_equals_eager_launches(runs):
    mix, _ = runs
    assert (mix["em"] == mix["em_eager"]).all()


def test_condition_share_is_rebuilt_per_call(runs):
    """second call on the same buffers with new cond_img contents (the cached step graph is replayed) against a fresh model's run"""
    mix, _ = runs
    assert (mix["em_new_cond"] == mix["em_new_cond_fresh"]).all()
    assert not (mix["em_new_cond"] == mix["em"]).all()


def test_conv1_upload_reaches_the_packed_weights(runs):
    mix, ref = runs
    check_parity(t_(mix["em_new_w1"]), t_(ref["em_new_w1"]), SAMPLER_TOL, "skip in the mix vs conv1 launch after an upload of conv1.weight")
    moved = maxrel(t_(mix["em_new_w1"]), t_(mix["em"]))
    print(f"conv1.weight x 1.25 moves the samples by max-rel {moved:.2e}")
    assert moved > 10 * SAMPLER_TOL


def test_workspace_grows_by_the_condition_share_on_the_run_only(runs):
    mix, ref = runs
    assert int(mix["ws_forward"]) == int(ref["ws_forward"])
    assert int(mix["ws_run"]) - int(ref["ws_run"]) == RUN_B * RUN_HW * RUN_HW * 64
