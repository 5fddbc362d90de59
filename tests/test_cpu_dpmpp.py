"""dpmpp_2m_sampler without a device: the step table's invariants, the order of the recurrence on the analytic Gaussian problem (and
its error next to the Heun recurrence's at the same step count), the config section, the registry, the alias and the C interface."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from dpmpp_ref import SIG, dpm_restatement, gaussian_exact, gaussian_score_f64, heun_f64
from sbgm_danra_amd import _native as N
from sbgm_danra_amd import score_sampling as SS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n", [2, 3, 8, 32])
@pytest.mark.parametrize("kw", [{}, dict(sigma_min=0.05, sigma_max=40.0, rho=5.0)])
def test_schedule_deterministic(n, kw):
    s = SS.dpmpp_2m_schedule(n, SIG, **kw)
    assert np.array_equal(s["sigma"], SS.edm_heun_schedule(n, SIG, **kw)["sigma"])
    assert s["sigma"].shape == (n + 1,) and s["sigma"][n] == 0.0
    for k in ("t", "c_x", "c_0", "c_1", "c_z"):
        assert s[k].shape == (n,) and s[k].dtype == np.float64, k
    assert np.array_equal(s["t"], SS.edm_heun_schedule(n, SIG, **kw)["t_hat"])     # no churn: evaluated at t(sigma_i)
    assert s["c_1"][0] == 0.0
    assert (s["c_x"][-1], s["c_0"][-1], s["c_1"][-1], s["c_z"][-1]) == (0.0, 1.0, 0.0, 0.0)
    assert np.abs(s["c_x"] + s["c_0"] + s["c_1"] - 1.0).max() <= 1e-12         # a constant denoised estimate is reproduced
    assert (s["c_z"] == 0.0).all()
    assert (s["c_1"][1:-1] < 0).all() and (s["c_x"][:-1] > 0).all()
    assert s["nfe"] == n and s["draws"] == 1


@pytest.mark.parametrize("n", [2, 5, 32])
@pytest.mark.parametrize("eta", [0.3, 1.0, 2.5])
def test_schedule_stochastic_conserves_the_noise_level(n, eta):
    s = SS.dpmpp_2m_schedule(n, SIG, eta=eta)
    sg = s["sigma"]
    got = s["c_x"][:-1] ** 2 * sg[:n - 1] ** 2 + s["c_z"][:-1] ** 2
    assert np.abs(got / sg[1:n] ** 2 - 1.0).max() <= 1e-12
    assert s["c_1"][0] == 0.0 and (s["c_x"][-1], s["c_0"][-1], s["c_1"][-1], s["c_z"][-1]) == (0.0, 1.0, 0.0, 0.0)
    assert s["nfe"] == n and s["draws"] == 1 + n
    assert np.allclose(SS.dpmpp_2m_schedule(n, SIG, eta=eta, s_noise=0.5)["c_z"], 0.5 * s["c_z"], rtol=1e-15)
    assert SS._counts(N.SAMPLER_DPMPP_2M, n, True) == (1, 1 + n) and SS._counts(N.SAMPLER_DPMPP_2M, n) == (1, 1)


def test_schedule_argument_errors(caplog):
    for kw in (dict(num_steps=1), dict(num_steps=8, rho=0.0), dict(num_steps=8, eta=-0.1), dict(num_steps=8, s_noise=-1.0),
               dict(num_steps=8, sigma_min=3.0, sigma_max=2.0), dict(num_steps=8, sigma_min=1e4, sigma_max=1e5)):
        with pytest.raises(ValueError, match="dpmpp_2m_sampler"):
            SS.dpmpp_2m_schedule(**kw)
    caplog.clear()
    with caplog.at_level("WARNING"):
        s =SS.dpmpp_2m_schedule(8, SIG, sigma_min=1e-6, sigma_max=1e6)
    assert sum("clipped" in r.message for r in caplog.records) == 1
    d = SS.dpmpp_2m_schedule(8, SIG)
    assert s["sigma_min"] == d["sigma_min"] and s["sigma_max"] == d["sigma_max"]


@pytest.mark.parametrize("s0", [0.5, 1.0, 2.0])
def test_host_recurrence_is_second_order_and_no_worse_than_heun(s0):
    f = gaussian_score_f64(s0)
    g = torch.Generator().manual_seed(int(s0 * 10))
    z = torch.randn(1, 4, 1, 16, 16, generator=g, dtype=torch.float64)
    err, err_heun = {}, {}
    for n in (8, 16, 32):
        sch = SS.dpmpp_2m_schedule(n, SIG)
        x0 = z[0] * sch["sigma"][0]
        exact = gaussian_exact(x0, s0, sch)
        rel = lambda a: float((a - exact).abs().max() / exact.abs().max())  # noqa: E731
        err[n] = rel(dpm_restatement(f, z, n, dtype=torch.float64, x_init=x0))
        err_heun[n] = rel(heun_f64(f, x0, n))
    print(f"s0={s0}: 2M {err}, Heun {err_heun}")
    assert err[8] > err[16] > err[32]
    assert err[16] / err[32] >= 3.6, err                               # second order: the error falls ~4x per doubling
    for n in (16, 32):
        assert err[n] <= 1.25 * err_heun[n], (n, err[n], err_heun[n])  # N evaluations against 2N - 1


def test_kwargs_registry_alias_and_signature():
    assert SS.dpm_sampler_kwargs({}) == {} and SS.dpm_sampler_kwargs(None) == {} and SS.dpm_sampler_kwargs({"dpm": None}) == {}
    kw = SS.dpm_sampler_kwargs({"dpm": {"sigma_min": 0.01, "rho": 5, "eta": 1, "s_noise": None, "other": 3}})
    assert kw == {"sigma_min": 0.01, "rho": 5.0, "eta": 1.0} and all(isinstance(v, float) for v in kw.values())
    import sbgm.score_sampling as alias
    import sbgm_danra_amd as S
    from sbgm_danra_amd.training import _SAMPLERS
    assert _SAMPLERS["dpmpp_2m_sampler"] is SS.dpmpp_2m_sampler is S.dpmpp_2m_sampler is alias.dpmpp_2m_sampler
    p = inspect.signature(SS.dpmpp_2m_sampler).parameters
    for name in ("joint_tiles", "known", "known_mask", "tile_origins", "domain_width", "eta", "s_noise", "noise", "seed", "use_graph"):
        assert name in p and p[name].kind is inspect.Parameter.KEYWORD_ONLY, name
    assert p["eta"].default == 0.0 and p["num_steps"].default == 32 and p["rho"].default == 7.0
    assert list(p)[:13] == list(inspect.signature(SS.edm_heun_sampler).parameters)[:13]


def test_header_and_signatures_agree():
    header = open(os.path.join(ROOT, "include", "sbgm_hip.h")).read()
    assert re.search(r"SBGM_SAMPLER_DPMPP_2M\s*=\s*4\b", header) and N.SAMPLER_DPMPP_2M == 4
    n_args = lambda name: len(re.search(name + r"\s*\(([^;]*)\);", header).group(1).split(","))  # noqa: E731
    for name, n in (("sbgm_sampler_run_dpmpp", 12), ("sbgm_dpmpp_2m_step", 13)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in N.SIGNATURES and n_args(name) == len(N.SIGNATURES[name][1]) == n, name
        assert hasattr(N.lib(), name)
    assert N.lib().sbgm_abi_version() == N.ABI_VERSION >= 5
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "sbgm_sampler_run_dpmpp" in doc and "sbgm_dpmpp_2m_step" in doc and "dpm:" in doc
