"""Joint full-domain sampling without a device: the host restatements of joint_tiles_ref.py against the independent-tile and
plain recurrences where the two must coincide, the ABI header, and the argument checks that run before anything touches the GPU."""
import inspect
import os
import re

import pytest
import torch

import constrained_ref as R
import joint_tiles_ref as J
import sbgm_danra_amd as S
from sbgm_danra_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STD = (S.marginal_prob_std_fn, S.diffusion_coeff_fn)
A = J.Geometry((44, 54), 32, 8)
SEED = 77 + (5 << 32)


def maxrel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def test_geometries_are_what_the_gpu_tests_assume():
    assert A.Wd_pad == 56 and A.R == 16
    assert A.origins == [(0, 0), (0, 12), (0, 24), (12, 0), (12, 12), (12, 24)]
    cov = A.coverage()
    assert cov.max() == 6 and cov.min() == 1 and (cov[:, 24:32] >= 3).all()          # three tiles per axis cover columns 24..31
    B = J.Geometry((32, 64), 32, 0)
    assert B.origins == [(0, 0), (0, 32)] and B.R == 1 and B.coverage().max() == 1
    C = J.Geometry((32, 32), 32, 8)
    assert C.origins == [(0, 0)] and C.Wd_pad == 32


def test_blend_of_equal_copies_is_the_copy_and_single_cover_is_untouched():
    g = torch.Generator().manual_seed(1)
    dom = torch.randn(1, A.Hd, A.Wd_pad, generator=g)
    assert maxrel(A.stitch(A.extract(dom)), dom) <= 1e-6                              # partition of unity
    tiles = torch.randn(len(A), 1, 32, 32, generator=g)                               # tiles that disagree
    out = A.stitch(tiles)
    single = torch.from_numpy(A.coverage() == 1)
    assert single.any() and single[0, :12].all()
    assert torch.equal(out[0, :12, :12], tiles[0, 0, :12, :12])                       # w s / w with w = 1: exact


@pytest.mark.parametrize("kind,n,kw", [("em", 8, {}), ("pc", 8, {}), ("edm", 6, {}), ("edm", 6, dict(s_churn=30.0))])
def test_pixel_independent_score_makes_joint_and_independent_tiles_agree(kind, n, kw):
    """every tile computes the same score at a shared pixel, so the blend is a convex combination of equal numbers and the joint run is
    the independent-tile run with the same domain-keyed noise (PC: both use the batch-mean norm over the six tiles)"""
    score = R.gaussian_score(1.0)
    joint = {"em": J.em_joint, "pc": J.pc_joint, "edm": J.heun_joint}[kind](score, SEED, n, A, **kw)
    noise = J.tile_noise(SEED, 1 + 2 * n, A)
    tiles = {"em": R.em_restatement, "pc": R.pc_restatement, "edm": R.heun_restatement}[kind](score, noise, n, **kw)
    assert joint.shape == (1, A.Hd, A.Wd) and tiles.shape == (len(A), 1, 32, 32)
    # tile by tile over the unpadded columns (the padded ones are sampled pixels too, but the restatement crops them)
    err = max(maxrel(tiles[t, :, :, :A.Wd - x], joint[:, y:y + 32, x:x + 32]) for t, (y, x) in enumerate(A.origins))
    print(f"joint vs independent tiles, gaussian score, {kind} N={n} {kw}: max-rel {err:.2e}")
    assert err <= 1e-6


@pytest.mark.parametrize("kind,kw", [("em", {}), ("pc", {}), ("edm", {}), ("edm", dict(s_churn=30.0))])
def test_one_tile_domain_is_the_plain_recurrence(kind, kw):
    C = J.Geometry((32, 32), 32, 8)
    g = torch.Generator().manual_seed(2)
    w = torch.randn(1, 1, 32, 32, generator=g)
    score = lambda x, t: -x / (1.0 + t.view(-1, 1, 1, 1)) + 0.1 * torch.roll(x, 1, -1) * w  # noqa: E731  (not pixel-independent)
    joint = {"em": J.em_joint, "pc": J.pc_joint, "edm": J.heun_joint}[kind](score, SEED, 5, C, **kw)
    noise = J.tile_noise(SEED, 11, C)
    plain = {"em": R.em_restatement, "pc": R.pc_restatement, "edm": R.heun_restatement}[kind](score, noise, 5, **kw)
    assert torch.equal(joint, plain[0])


def test_held_restatement_returns_known_on_the_mask():
    g = torch.Generator().manual_seed(3)
    known = A.pad(torch.randn(1, 1, A.Hd, A.Wd, generator=g))
    mask = torch.zeros(1, 1, A.Hd, A.Wd_pad)
    mask[0, 0, 5:30, 8:40] = 1.0                                                      # crosses the overlap bands of both axes
    for fn in (J.em_joint, J.pc_joint, J.heun_joint):
        out = fn(R.gaussian_score(1.0), SEED, 4, A, known=known, mask=mask)
        on = mask[0, :, :, :A.Wd] == 1
        assert torch.equal(out[on], known[0, :, :, :A.Wd][on])


def test_header_and_binding_declare_the_entry_points():
    header = open(os.path.join(ROOT, "include", "sbgm_hip.h")).read()
    for name in ("sbgm_sampler_run_joint", "sbgm_sampler_run_edm_joint", "sbgm_blend_tile_scores"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in N.SIGNATURES, name
    n_args = lambda name: len(re.search(name + r"\s*\(([^;]*)\);", header).group(1).split(","))  # noqa: E731
    for name in ("sbgm_sampler_run_joint", "sbgm_sampler_run_edm_joint", "sbgm_blend_tile_scores"):
        assert n_args(name) == len(N.SIGNATURES[name][1]), name
    assert "sbgm_sampler_args" in header and "domain_h" not in re.search(r"typedef struct sbgm_sampler_args \{(.*?)\}", header, re.S).group(1)


def test_which_samplers_take_joint_tiles():
    for f in (S.Euler_Maruyama_sampler, S.pc_sampler, S.edm_heun_sampler):
        assert inspect.signature(f).parameters["joint_tiles"].default is None
    for f in (S.rk45_sampler, S.ode_sampler):
        assert "joint_tiles" not in inspect.signature(f).parameters
    from sbgm_danra_amd.tiling import FullDomainTiler
    assert inspect.signature(FullDomainTiler.sample).parameters["joint"].default is False


@pytest.mark.parametrize("sampler", [S.Euler_Maruyama_sampler, S.pc_sampler, S.edm_heun_sampler])
def test_argument_checks_before_the_device(sampler):
    org = torch.zeros(2, 2, dtype=torch.int32)
    f = R.gaussian_score(1.0)
    run = lambda **kw: sampler(f, *STD, batch_size=2, num_steps=3, device="cpu", img_size=32, **kw)  # noqa: E731
    with pytest.raises(ValueError, match="tile_origins"):
        run(joint_tiles=(32, 16))
    with pytest.raises(ValueError, match="noise"):
        run(joint_tiles=(32, 16), tile_origins=org, domain_width=32, noise=torch.zeros(8, 2, 1, 32, 32))
    with pytest.raises(ValueError, match="ramp_len"):
        run(joint_tiles=(32, 0), tile_origins=org, domain_width=32)
    with pytest.raises(ValueError, match="joint_tiles"):
        run(joint_tiles=32, tile_origins=org, domain_width=32)


def test_host_driven_loops_refuse_joint_tiles():
    from sbgm_danra_amd.score_sampling import _host_start
    with pytest.raises(N.NativeError, match="joint"):
        _host_start(N.SAMPLER_EM, 2, 3, 32, "cpu", None, 1, 1.0, torch.zeros(2, 2, dtype=torch.int32), joint=(32, 16))
