"""CPU suite: host side of the EDM Heun sampler — the sigma ladder / t(sigma) table of `edm_heun_schedule`, clipping to the
trained range, evaluation and noise-draw counts, churn bounds, argument validation before any device work, and the config
dispatch (`sampler_type: edm_heun_sampler`, the optional `edm:` section)."""
import logging
import math

import numpy as np
import pytest
import torch

import sbgm_danra_amd as S
from sbgm_danra_amd import score_sampling as SS

SIG, EPS = 25.0, 1e-3


def std64(t):
    return math.sqrt((SIG ** (2.0 * t) - 1.0) / (2.0 * math.log(SIG)))


@pytest.mark.parametrize("n", [2, 5, 18, 32, 64])
def test_ladder_matches_karras_formula(n):
    smin, smax, rho = 0.05, 8.0, 7.0
    sch = SS.edm_heun_schedule(n, SIG, EPS, sigma_min=smin, sigma_max=smax, rho=rho)
    ref = S.edm_sigma_schedule(n, smin, smax, rho, device="cpu").double().numpy()
    assert sch["sigma"].shape == (n + 1,) and sch["sigma"][-1] == 0.0
    np.testing.assert_allclose(sch["sigma"][:n], ref, rtol=1e-6)
    assert np.all(np.diff(sch["sigma"]) < 0)
    assert sch["sigma_min"] == smin and sch["sigma_max"] == smax


def test_time_round_trip_and_defaults():
    n = 16
    sch = SS.edm_heun_schedule(n, SIG, EPS)
    s = sch["sigma"][:n]
    t = np.clip(np.log1p(2 * math.log(SIG) * s ** 2) / (2 * math.log(SIG)), EPS, 1.0)
    back = np.array([std64(v) for v in t])
    np.testing.assert_allclose(back, s, rtol=1e-6)
    assert sch["t_hat"][0] == 1.0                                   # clamped to 1 exactly
    assert sch["t_next"][n - 2] == pytest.approx(EPS, rel=1e-9)      # t(sigma_{N-1}): the last evaluated time
    assert sch["sigma"][0] == pytest.approx(std64(1.0), rel=1e-12) and sch["sigma"][n - 1] == pytest.approx(std64(EPS), rel=1e-12)
    assert sch["sigma"][0] == pytest.approx(9.845, abs=1e-3) and sch["sigma"][n - 1] == pytest.approx(0.0317, abs=1e-4)
    # the network's own fp32 std(t) maps the table's times back onto the ladder
    got = S.marginal_prob_std_fn(torch.tensor(sch["t_hat"], dtype=torch.float32)).double().numpy()
    np.testing.assert_allclose(got, sch["sigma_hat"], rtol=1e-5)


def test_out_of_range_sigmas_clip_with_one_warning(caplog):
    with caplog.at_level(logging.WARNING, logger=SS.__name__):
        sch = SS.edm_heun_schedule(8, SIG, EPS, sigma_min=0.002, sigma_max=80.0)
    assert len([r for r in caplog.records if r.levelno == logging.WARNING]) == 1
    assert sch["sigma_min"] == pytest.approx(std64(EPS), rel=1e-12) and sch["sigma_max"] == pytest.approx(std64(1.0), rel=1e-12)
    assert sch["t_hat"].max() <= 1.0 and sch["t_next"].min() >= EPS
    caplog.clear()
    with caplog.at_level(logging.WARNING, logger=SS.__name__):
        SS.edm_heun_schedule(8, SIG, EPS)
        SS.edm_heun_schedule(8, SIG, EPS, sigma_min=0.1, sigma_max=5.0)
    assert not [r for r in caplog.records if r.levelno == logging.WARNING]


@pytest.mark.parametrize("n", [2, 5, 32])
def test_counts_and_churn_bounds(n):
    det = SS.edm_heun_schedule(n, SIG, EPS)
    assert det["nfe"] == 2 * n - 1 and det["draws"] == 1
    assert np.all(det["gamma"] == 0) and np.array_equal(det["sigma_hat"], det["sigma"][:n]) and np.all(det["churn_coef"] == 0)
    sto = SS.edm_heun_schedule(n, SIG, EPS, s_churn=40.0)
    assert sto["nfe"] == 2 * n - 1 and sto["draws"] == 1 + n
    assert np.all(sto["sigma_hat"] <= sto["sigma"][0] * (1 + 1e-15))
    assert np.all(sto["gamma"] <= math.sqrt(2) - 1 + 1e-15) and np.all(sto["gamma"] >= 0)
    assert sto["gamma"][0] == 0.0                                    # sigma_hat is capped at sigma_0
    assert np.all(sto["t_hat"] <= 1.0)
    np.testing.assert_allclose(sto["churn_coef"], np.sqrt(sto["sigma_hat"] ** 2 - sto["sigma"][:n] ** 2), rtol=1e-12)
    if n == 5:
        np.testing.assert_allclose(sto["gamma"][1:], math.sqrt(2) - 1, rtol=1e-12)
    win = SS.edm_heun_schedule(n, SIG, EPS, s_churn=40.0, s_tmin=0.5, s_tmax=3.0, s_noise=1.007)
    s = win["sigma"][:n]
    assert np.all(win["gamma"][(s < 0.5) | (s > 3.0)] == 0)
    assert np.all(win["churn_coef"][win["gamma"] == 0] == 0)


@pytest.mark.parametrize("kw", [dict(num_steps=1), dict(rho=0.0), dict(rho=-1.0), dict(s_noise=-0.1), dict(s_churn=-1.0),
                                dict(sigma_min=5.0, sigma_max=2.0)])
def test_argument_validation_before_device_work(kw):
    def never(*a, **k):
        raise AssertionError("the score model must not be called")
    args = dict(num_steps=8)
    args.update(kw)
    with pytest.raises(ValueError):
        S.edm_heun_sampler(never, S.marginal_prob_std_fn, S.diffusion_coeff_fn, batch_size=2, device="cuda", img_size=32, **args)
    assert not torch.cuda.is_initialized()


def test_config_dispatch_and_edm_section():
    from sbgm_danra_amd import training
    from sbgm_danra_amd.config_loader import to_config
    assert training._SAMPLERS["edm_heun_sampler"] is S.edm_heun_sampler
    assert SS.edm_sampler_kwargs({}) == {} and SS.edm_sampler_kwargs(None) == {}
    assert SS.edm_sampler_kwargs({"edm": None}) == {}
    cfg = to_config({"edm": {"enabled": False, "sigma_min": 0.002, "sigma_max": 80, "rho": 7}})
    assert SS.edm_sampler_kwargs(cfg) == {"sigma_min": 0.002, "sigma_max": 80.0, "rho": 7.0}
    full = {"edm": {"sigma_min": 0.05, "sigma_max": 5.0, "rho": 5, "s_churn": 10, "s_tmin": 0.1, "s_tmax": 2.0, "s_noise": 1.003}}
    assert SS.edm_sampler_kwargs(full) == {k: float(v) for k, v in full["edm"].items()}
    import sbgm
    assert sbgm.score_sampling.edm_heun_sampler is S.edm_heun_sampler
