"""Joint full-domain sampling on the GPU: the blend kernel against the stitch specification, bit-equality of all copies
of a domain pixel through Euler-Maruyama, predictor-corrector and EDM Heun runs, the runs against the host restatements of
joint_tiles_ref.py around the oracle network, the reductions to the non-joint tiled run (tiles that do not overlap, a one-tile domain),
composition with held pixels, guidance and the step graph, and `FullDomainTiler.sample(joint=True)` with its refusals.

Geometries, tile 32 throughout: A = 44 x 54, halo 8: 2 x 3 tiles, Wd_pad = 56, x origins 0 / 12 / 24 so that columns 24..31 lie in three
tiles and up to six tiles cover one pixel; B = 32 x 64, halo 0: two tiles that do not overlap; C = 32 x 32: one tile."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import tiler_ref as OT  # noqa: E402
from util_models import build_pair, check_parity, maxrel  # noqa: E402

import joint_tiles_ref as J  # noqa: E402
import sbgm_danra_amd as S  # noqa: E402
from sbgm_danra_amd import _native as N  # noqa: E402
from sbgm_danra_amd.tiling import FullDomainTiler  # noqa: E402

GUIDED = {"classifier_free_guidance": {"enabled": True, "guidance_scale": 2.5, "guidance_scale_max": 1.5}}
SAMPLERS = {"em": S.Euler_Maruyama_sampler, "pc": S.pc_sampler, "edm": S.edm_heun_sampler}
RESTATED = {"em": J.em_joint, "pc": J.pc_joint, "edm": J.heun_joint}
STD = (S.marginal_prob_std_fn, S.diffusion_coeff_fn)
SEED = 77 + (5 << 32)
CASES = [("em", 3, {}), ("pc", 2, {}), ("edm", 3, {}), ("edm", 3, dict(s_churn=30.0))]
IDS = ["em", "pc", "edm", "edm-churn"]


@pytest.fixture(scope="module")
def pair():
    ora, net, _ = build_pair(1)
    return ora.eval(), net.eval()


@pytest.fixture(scope="module")
def A():
    """the tiler of geometry A, its host twin, a random domain condition and its tiles"""
    t, geo = FullDomainTiler((44, 54), 32, 8), J.Geometry((44, 54), 32, 8)
    assert t.origins == geo.origins and t.Wd_pad == geo.Wd_pad == 56 and len(t) == 6 and geo.coverage().max() == 6
    cond = torch.randn(1, 44, 54, generator=torch.Generator().manual_seed(4))
    return t, geo, cond.cuda(), t.extract(cond.cuda())


def run(net, kind, n, t, tiles, joint=True, seed=SEED, **kw):
    jt = {"joint_tiles": (t.Hd, max(1, t.overlap))} if joint else {}
    return SAMPLERS[kind](net, *STD, batch_size=len(t), num_steps=n, device="cuda", img_size=t.tile, seed=seed, cond_img=tiles,
                          tile_origins=t.origins_dev, domain_width=t.Wd_pad, **jt, **kw)


@pytest.fixture(scope="module")
def joint_runs(pair, A):
    """the joint run of every case on A, computed once: (tiles, the same call again)"""
    t, _, _, tiles = A
    return {i: run(pair[1], k, n, t, tiles, **kw) for i, (k, n, kw) in zip(IDS, CASES)}


def shared_rectangles(t):
    """(a, b, window in a, window in b) for every pair of tiles that intersect"""
    out = []
    for a, (ya, xa) in enumerate(t.origins):
        for b, (yb, xb) in enumerate(t.origins):
            y0, y1, x0, x1 = max(ya, yb), min(ya, yb) + t.tile, max(xa, xb), min(xa, xb) + t.tile
            if a < b and y0 < y1 and x0 < x1:
                out.append((a, b, (slice(y0 - ya, y1 - ya), slice(x0 - xa, x1 - xa)), (slice(y0 - yb, y1 - yb), slice(x0 - xb, x1 - xb))))
    return out


def copies_equal(tiles, t):
    rects = shared_rectangles(t)
    assert rects
    return all(torch.equal(tiles[a, 0][wa], tiles[b, 0][wb]) for a, b, wa, wb in rects)


def stitch_vs_windows(tiles, t):
    """max over tiles of max-rel(tiler.stitch(tiles) on the tile's window, the tile), over the unpadded columns"""
    dom = t.stitch(tiles)
    return max(maxrel(dom[:, y:y + t.tile, x:x + t.tile], tiles[i, :, :, :t.Wd - x]) for i, (y, x) in enumerate(t.origins))


# ---- 1. the blend kernel -----------------------------------------------------------------------------------------------------------
def test_blend_kernel_matches_the_stitch_specification(A):
    t, geo, _, _ = A
    assert len(shared_rectangles(t)) == 15                                  # every pair of the six tiles intersects
    scores = torch.randn(6, 1, 32, 32, generator=torch.Generator().manual_seed(5))              # "scores" that disagree
    dev, out = scores.cuda(), torch.full((6, 1, 32, 32), float("nan"), device="cuda")
    N.check(N.lib().sbgm_blend_tile_scores(dev.data_ptr(), t.origins_dev.data_ptr(), out.data_ptr(), 6, 32, 32, t.Hd, t.Wd_pad,
                                           max(1, t.overlap), N.stream()))
    want = OT.extract(OT.stitch(scores.numpy(), t.origins, t.Hd, t.Wd_pad, geo.R), t.origins, 32)
    err = maxrel(out.cpu(), torch.from_numpy(want))
    print(f"blend kernel vs extract(stitch(.)): max-rel {err:.2e}")
    assert err <= 1e-6
    assert copies_equal(out, t) and not copies_equal(dev, t)
    single = torch.from_numpy(OT.extract((geo.coverage() == 1)[None].astype(np.float32), t.origins, 32)) == 1
    assert single.any() and not single.all()
    assert torch.equal(out.cpu()[single], scores[single])
    assert not torch.equal(out.cpu()[~single], scores[~single])


# ---- 2. copies stay equal ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(4), ids=IDS)
def test_copies_of_a_domain_pixel_stay_bit_equal(pair, A, joint_runs, case):
    t, _, _, tiles = A
    kind, n, kw = CASES[case]
    got = joint_runs[IDS[case]]
    assert got.shape == (6, 1, 32, 32) and torch.isfinite(got).all()
    assert copies_equal(got, t)
    err = stitch_vs_windows(got, t)
    print(f"joint {IDS[case]}: stitch vs each tile's own window, max-rel {err:.2e}")
    assert err <= 1e-6
    plain = run(pair[1], kind, n, t, tiles, joint=False, **kw)                 # not vacuous: independent tiles do differ there
    assert torch.isfinite(plain).all() and not copies_equal(plain, t)
    assert not torch.equal(plain, got)


# ---- 3. against the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(4), ids=IDS)
def test_joint_run_matches_the_host_restatement(pair, A, joint_runs, case):
    """bound: the 1e-4 test_gpu_constrained.py allows its network-score restatement comparisons; the blend is a convex combination and
    cannot amplify the evaluation error"""
    t, geo, _, tiles = A
    kind, n, kw = CASES[case]
    cond = tiles.cpu()
    score = lambda x, tt: pair[0](x, tt, cond_img=cond)  # noqa: E731
    with torch.no_grad():
        want = RESTATED[kind](score, SEED, n, geo, **kw)
    got = t.stitch(joint_runs[IDS[case]]).cpu()
    assert got.shape == want.shape == (1, 44, 54)
    check_parity(got, want, 1e-4, f"joint {IDS[case]} 44x54 N={n} vs restatement")


# ---- 4. reductions to today's behaviour ------------------------------------------------------------------------------------------------
def test_tiles_that_do_not_overlap_are_the_non_joint_run(pair):
    t = FullDomainTiler((32, 64), 32, 0)
    assert t.origins == [(0, 0), (0, 32)]
    tiles = t.extract(torch.randn(1, 32, 64, generator=torch.Generator().manual_seed(6)).cuda())
    for kind, n, kw in (CASES[0], CASES[2]):
        assert torch.equal(run(pair[1], kind, n, t, tiles, **kw), run(pair[1], kind, n, t, tiles, joint=False, **kw)), kind


def test_one_tile_domain_is_the_plain_tiled_run(pair):
    t = FullDomainTiler((32, 32), 32, 8)
    assert t.origins == [(0, 0)]
    tiles = t.extract(torch.randn(1, 32, 32, generator=torch.Generator().manual_seed(7)).cuda())
    for kind, n, kw in (CASES[0], CASES[2]):
        assert torch.equal(run(pair[1], kind, n, t, tiles, **kw), run(pair[1], kind, n, t, tiles, joint=False, **kw)), kind
    kind, n, kw = CASES[1]                                                   # PC: the mean over one tile's norm is that tile's norm
    assert maxrel(run(pair[1], kind, n, t, tiles, **kw), run(pair[1], kind, n, t, tiles, joint=False, **kw)) <= 1e-6


# ---- 5. composition ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(3), ids=IDS[:3])
def test_held_pixels_compose_with_the_blend(pair, A, case):
    t, _, _, tiles = A
    kind, n, kw = CASES[case]
    known = torch.randn(1, 44, 54, generator=torch.Generator().manual_seed(8)).cuda()
    mask = torch.zeros(1, 44, 54)
    mask[0, :5, :7] = 1.0                                                    # the corner
    mask[0, 5:30, 9:41] = 1.0                                                # a block across the overlap bands of both axes
    mask[0, 30, 9:41:2] = 0.25                                               # one feathered row
    mask[0, 30, 10:41:2] = 0.5
    mask[0, :, 51:] = 1.0                                                    # the strip at the padded edge
    mask[0, 3::7, 5::9] = 1.0                                                # stations
    kt, mt = t.extract(known), t.extract(mask.cuda())
    got = run(pair[1], kind, n, t, tiles, known=kt, known_mask=mt, **kw)
    assert torch.isfinite(got).all()
    assert torch.equal(got[mt == 1], kt[mt == 1])
    assert copies_equal(got, t)
    assert not torch.equal(got[mt == 0], run(pair[1], kind, n, t, tiles, **kw)[mt == 0])     # the free pixels feel the held ones


def test_guided_run_keeps_copies_equal(A):
    t, _, _, tiles = A
    _, net, _ = build_pair(1, 4)
    y = torch.full((6,), 2, dtype=torch.int64, device="cuda")
    got = run(net.eval(), "em", 3, t, tiles, y=y, cfg=GUIDED)
    assert torch.isfinite(got).all() and copies_equal(got, t)
    assert not copies_equal(run(net, "em", 3, t, tiles, joint=False, y=y, cfg=GUIDED), t)


@pytest.mark.parametrize("case", range(4), ids=IDS)
def test_step_graph_replay_and_key(pair, A, joint_runs, case):
    t, _, _, tiles = A
    kind, n, kw = CASES[case]
    before = run(pair[1], kind, n, t, tiles, joint=False, **kw)
    again = run(pair[1], kind, n, t, tiles, **kw)
    assert torch.equal(again, joint_runs[IDS[case]])                                           # same seed, replayed
    assert torch.equal(run(pair[1], kind, n, t, tiles, use_graph=False, **kw), again)          # replay == eager
    assert torch.equal(run(pair[1], kind, n, t, tiles, joint=False, **kw), before)             # a joint step is not reused for it
    assert not torch.equal(run(pair[1], kind, n, t, tiles, seed=SEED + 1, **kw), again)


# ---- 6. the tiler and the refusals -----------------------------------------------------------------------------------------------------
def test_tiler_samples_the_domain_jointly(pair, A, joint_runs):
    t, _, cond, tiles = A
    sample = lambda **kw: t.sample(pair[1], S.pc_sampler, *STD, num_steps=2, cond_img=cond, seed=SEED, joint=True, **kw)  # noqa: E731
    dom = sample()
    assert dom.shape == (1, 44, 54) and torch.isfinite(dom).all()
    assert torch.equal(sample(tiles_per_batch=6), dom)
    assert torch.equal(dom, t.stitch(joint_runs["pc"]))
    assert not torch.equal(dom, t.sample(pair[1], S.pc_sampler, *STD, num_steps=2, cond_img=cond, seed=SEED))
    with pytest.raises(ValueError, match="one batch"):
        sample(tiles_per_batch=2)
    with pytest.raises(ValueError, match="joint_tiles"):
        t.sample(pair[1], S.rk45_sampler, *STD, num_steps=None, cond_img=cond, seed=SEED, joint=True)


def test_refusals(pair, A):
    t, _, _, tiles = A
    kw = dict(batch_size=6, num_steps=2, device="cuda", img_size=32, cond_img=tiles, seed=SEED)
    with pytest.raises(ValueError, match="tile_origins"):
        S.pc_sampler(pair[1], *STD, joint_tiles=(44, 16), **kw)
    with pytest.raises(ValueError, match="noise"):
        S.pc_sampler(pair[1], *STD, joint_tiles=(44, 16), tile_origins=t.origins_dev, domain_width=56,
                     noise=torch.zeros(5, 6, 1, 32, 32), **kw)
    with pytest.raises(N.NativeError, match="domain"):                       # the last row of tiles ends at 44 > 40
        S.pc_sampler(pair[1], *STD, joint_tiles=(40, 16), tile_origins=t.origins_dev, domain_width=56, **kw)
    with pytest.raises(N.NativeError, match="domain"):                       # x0 + W = 56 > 52
        S.Euler_Maruyama_sampler(pair[1], *STD, joint_tiles=(44, 16), tile_origins=t.origins_dev, domain_width=52, **kw)
    with pytest.raises(N.NativeError, match="joint"):                        # a host-driven loop (a plain callable)
        S.Euler_Maruyama_sampler(lambda x, tt, *a: pair[1](x, tt, *a), *STD, joint_tiles=(44, 16), tile_origins=t.origins_dev,
                                 domain_width=56, **kw)
    good = S.pc_sampler(pair[1], *STD, joint_tiles=(44, 16), tile_origins=t.origins_dev, domain_width=56, **kw)
    assert torch.isfinite(good).all()                                        # a refused call leaves the engine usable
