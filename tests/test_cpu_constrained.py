"""CPU suite: host side of constrained sampling (known pixels held in EM, PC and EDM Heun runs) -- the restatements the GPU tests
compare against, checked on a pixel-independent score; the hold levels against float64 marginal_prob_std; argument handling before any
device work; the `constraint:` config section."""
import math

import numpy as np
import pytest
import torch

import sbgm_danra_amd as S
from sbgm_danra_amd import score_sampling as SS
from sbgm_danra_amd.evaluate_sbgm.generation import constraint_mask

import constrained_ref as R

SIG, EPS = 25.0, 1e-3


def _case(B=2, hw=32, draws=12, seed=0):
    g = torch.Generator().manual_seed(seed)
    noise = torch.randn(draws, B, 1, hw, hw, generator=g)
    known = torch.randn(B, 1, hw, hw, generator=g)
    mask = (R.standard_mask(B, hw) >= 1).float()                        # binary: the self-check is about held / free pixels
    return noise, known, mask


@pytest.mark.parametrize("kind", ["em", "edm", "edm_churn"])
def test_restatement_free_pixels_do_not_move_and_held_pixels_equal_known(kind):
    noise, known, mask = _case()
    score = R.gaussian_score(1.0)
    if kind == "em":
        run = lambda **kw: R.em_restatement(score, noise, 6, **kw)  # noqa: E731
    else:
        run = lambda **kw: R.heun_restatement(score, noise, 6, s_churn=20.0 if kind == "edm_churn" else 0.0, **kw)  # noqa: E731
    free, held = run(), run(known=known, mask=mask)
    assert torch.isfinite(held).all()
    assert torch.equal(held[mask == 0], free[mask == 0])               # a pixel-independent score: bit-equal off the mask
    assert torch.equal(held[mask == 1], known[mask == 1])
    assert not torch.equal(held, free)
    # NaN under a zero mask is never touched
    poisoned = torch.where(mask == 0, torch.full_like(known, float("nan")), known)
    assert torch.equal(run(known=poisoned, mask=mask), held)


def test_restatement_pc_holds_known_and_soft_mask_blends():
    noise, known, _ = _case()
    mask = R.standard_mask(2, 32)
    out = R.pc_restatement(R.gaussian_score(1.0), noise, 5, known=known, mask=mask)
    assert torch.equal(out[mask == 1], known[mask == 1])
    free = R.pc_restatement(R.gaussian_score(1.0), noise, 5)
    soft = (mask > 0) & (mask < 1)
    assert soft.any() and not torch.equal(out[soft], known[soft]) and not torch.equal(out[soft], free[soft])
    v, t = torch.tensor([1.0, 2.0, 3.0]), torch.tensor([5.0, float("nan"), 7.0])
    assert torch.equal(R.hold(v, t, torch.tensor([1.0, 0.0, 0.5])), torch.tensor([5.0, 2.0, 5.0]))
    assert torch.equal(R.hold(v, t, torch.tensor([7.0, -3.0, 0.5])), torch.tensor([5.0, 2.0, 5.0]))    # clamped


@pytest.mark.parametrize("kind,n", [("em", 2), ("em", 5), ("em", 500), ("pc", 2), ("pc", 6), ("pc", 800)])
def test_hold_levels_equal_float64_marginal_prob_std(kind, n):
    lv = SS.sde_hold_levels(kind, n, SIG, EPS)
    t = lv["t"]
    assert t.shape == (n,) and t.dtype == np.float64 and np.array_equal(t, t.astype(np.float32).astype(np.float64))
    assert t[0] == 1.0 and t[-1] == pytest.approx(EPS, rel=1e-6) and np.all(np.diff(t) < 0)
    want = np.array([math.sqrt((SIG ** (2.0 * v) - 1.0) / (2.0 * math.log(SIG))) for v in t])
    assert lv["s_cur"].dtype == np.float32 and lv["s_next"].dtype == np.float32
    np.testing.assert_allclose(lv["s_cur"].astype(np.float64), want, rtol=2.0 ** -23)     # fp32 rounding of the float64 value
    assert np.array_equal(lv["s_next"][:-1], lv["s_cur"][1:]) and lv["s_next"][-1] == 0.0
    # the times are the table's: the same fp32 values the Python loops feed to the network
    if kind == "pc":
        assert np.array_equal(t, np.linspace(1.0, EPS, n).astype(np.float32).astype(np.float64))
    else:
        assert np.array_equal(t, torch.linspace(1.0, EPS, n).double().numpy())
    with pytest.raises(ValueError):
        SS.sde_hold_levels("heun", n)


SAMPLERS = [S.Euler_Maruyama_sampler, S.pc_sampler, S.edm_heun_sampler]


@pytest.mark.parametrize("sampler", SAMPLERS)
def test_argument_validation_before_device_work(sampler):
    def never(*a, **k):
        raise AssertionError("the score model must not be called")
    kw = dict(batch_size=2, num_steps=4, device="cuda", img_size=32)
    good, gm = torch.zeros(2, 1, 32, 32), torch.zeros(32, 32)
    for bad in (dict(known=good), dict(known_mask=gm),                                   # one of the pair
                dict(known=torch.zeros(2, 1, 16, 16), known_mask=gm), dict(known=torch.zeros(32, 32), known_mask=gm),
                dict(known=torch.zeros(1, 1, 32, 32), known_mask=gm),                    # known is per sample: no broadcast
                dict(known=good, known_mask=torch.zeros(3, 1, 32, 32)), dict(known=good, known_mask=torch.zeros(32))):
        with pytest.raises(ValueError):
            sampler(never, S.marginal_prob_std_fn, S.diffusion_coeff_fn, **kw, **bad)
    assert not torch.cuda.is_initialized()
    for fn in (S.rk45_sampler, S.ode_sampler):                                           # out of scope: they do not take the arguments
        with pytest.raises(TypeError):
            fn(never, S.marginal_prob_std_fn, S.diffusion_coeff_fn, known=good, known_mask=gm)


def test_mask_broadcasting():
    known = torch.arange(2 * 8 * 8, dtype=torch.float64).reshape(2, 8, 8)
    m2 = (torch.arange(64).reshape(8, 8) % 3 == 0).to(torch.uint8)
    for mask in (m2, m2.reshape(1, 1, 8, 8), m2.expand(2, 8, 8), m2.expand(2, 1, 8, 8)):
        k, m = SS._prep_known(known, mask, 2, 8, "cpu", "test")
        assert k.shape == m.shape == (2, 1, 8, 8) and k.dtype == m.dtype == torch.float32
        assert k.is_contiguous() and m.is_contiguous()
        assert torch.equal(k[:, 0], known.float()) and torch.equal(m[0, 0], m2.float()) and torch.equal(m[1, 0], m2.float())
    assert SS._prep_known(None, None, 2, 8, "cpu", "test") == (None, None)


def test_constraint_section():
    from sbgm_danra_amd.config_loader import to_config
    base = {"sampler": {"sampler_type": "pc_sampler"}}
    assert constraint_mask(to_config(base), (16, 20)) is None
    assert constraint_mask(to_config(dict(base, constraint=None)), (16, 20)) is None
    assert constraint_mask(to_config(dict(base, constraint={"enabled": False, "station_fraction": 0.5})), (16, 20)) is None
    sec = {"enabled": True, "station_fraction": 0.25, "seed": 3}
    a = constraint_mask(to_config(dict(base, constraint=sec)), (64, 48))
    b = constraint_mask(to_config(dict(base, constraint=dict(sec))), (64, 48))
    c = constraint_mask(to_config(dict(base, constraint=dict(sec, seed=4))), (64, 48))
    assert a.shape == (64, 48) and a.dtype == np.float32 and set(np.unique(a)) == {0.0, 1.0}
    assert np.array_equal(a, b) and not np.array_equal(a, c)                               # deterministic in its seed
    assert 0.15 < a.mean() < 0.35
    for st in ("rk45_sampler",):
        with pytest.raises(ValueError):
            constraint_mask(to_config({"sampler": {"sampler_type": st}, "constraint": sec}), (64, 48))
    assert constraint_mask(to_config({"sampler": {"sampler_type": "rk45_sampler"}, "constraint": {"enabled": False}}), (8, 8)) is None
    with pytest.raises(ValueError):
        constraint_mask(to_config(dict(base, constraint={"enabled": True, "station_fraction": 1.5})), (8, 8))


def test_constraint_mask_file(tmp_path):
    from sbgm_danra_amd.config_loader import to_config
    m = (np.arange(12 * 12).reshape(12, 12) % 5 == 0).astype(np.float64)
    np.save(tmp_path / "m.npy", m)
    cfg = to_config({"sampler": {}, "constraint": {"enabled": True, "mask_file": str(tmp_path / "m.npy")}})
    got = constraint_mask(cfg, (12, 12))
    assert got.dtype == np.float32 and np.array_equal(got, m.astype(np.float32))
    with pytest.raises(ValueError):
        constraint_mask(cfg, (12, 16))


def test_tiler_refuses_one_of_the_pair_and_samplers_that_cannot_hold():
    from sbgm_danra_amd.tiling import FullDomainTiler
    t = FullDomainTiler.__new__(FullDomainTiler)             # the checks come before any device work: no device needed
    t.Hd, t.Wd, t.device = 40, 44, torch.device("cpu")
    k = torch.zeros(1, 40, 44)
    with pytest.raises(ValueError):
        t.sample(None, S.pc_sampler, None, None, 4, known=k)
    with pytest.raises(ValueError):
        t.sample(None, S.rk45_sampler, None, None, None, known=k, known_mask=k)
    with pytest.raises(ValueError):
        t.sample(None, S.pc_sampler, None, None, 4, known=torch.zeros(1, 40, 40), known_mask=k)
