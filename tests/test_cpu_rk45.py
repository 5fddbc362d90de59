"""rk45_sampler on the CPU: the numpy restatement of its solver (`rk45_host_solve`) against scipy's `solve_ivp(method="RK45")` on the
analytic score of Gaussian data, the per-sample controllers, the failure paths, argument validation (before any device work) and the
config wiring of `sampler_type: rk45_sampler`."""
import numpy as np
import pytest
import torch
from scipy.integrate import solve_ivp

import sbgm_danra_amd as S
from sbgm_danra_amd import score_sampling as SS

SIG = 25.0


def gaussian_rhs(s0):
    """f(t, x) = c(t) * score(x, t) for data ~ N(0, s0^2): score = -x / (s0^2 + std(t)^2), rounded to fp32 like a network output,
    c(t) = fp32(-0.5 fp32(g g)), g = sigma^fp32(t) in fp32, the product taken in float64 (the precision of ode_sampler's rhs).
    `s0` and `t` may be arrays [B] with x [B, m] (the per-sample form)."""
    s0 = np.asarray(s0, dtype=np.float64)

    def f(t, x):
        tf = np.asarray(t, dtype=np.float32)
        g = np.float32(SIG) ** tf
        c = np.float32(-0.5) * (g * g).astype(np.float32)
        var = s0 ** 2 + SS._ve_std(tf.astype(np.float64), SIG) ** 2
        var, c = (var[:, None], c[:, None]) if np.ndim(x) == 2 else (var, c)
        return c.astype(np.float64) * (-x / var).astype(np.float32).astype(np.float64)
    return f


def start(s0, t0, shape, seed=0):
    return np.random.default_rng(seed).standard_normal(shape) * np.sqrt(s0 ** 2 + SS._ve_std(t0, SIG) ** 2)


# ---- 1. the restatement is scipy's algorithm ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("span", [(1.0, 1e-3), (1e-3, 1.0)], ids=["sample", "encode"])
@pytest.mark.parametrize("s0", [0.5, 1.0, 2.0])
@pytest.mark.parametrize("tol", [1e-5, 1e-3])
def test_host_solve_equals_scipy_rk45(span, s0, tol):
    """the stage sums are scipy's own np.dot expressions, so the endpoints are bit-equal and the evaluation counts equal"""
    y0 = start(s0, span[0], 2 * 32 * 32)
    ref = solve_ivp(gaussian_rhs(s0), span, y0, method="RK45", rtol=tol, atol=tol)
    y, st = S.rk45_host_solve(gaussian_rhs(s0), span[0], span[1], y0, tol, tol)
    print(f"span {span} s0 {s0} tol {tol}: nfev {st['nfev']} (scipy {ref.nfev}), rejected {st['n_rejected']}, "
          f"max diff {np.abs(y - ref.y[:, -1]).max():.1e}")
    assert ref.status == 0 and st["nfev"] == ref.nfev
    assert st["nfev"] == 2 + 6 * (st["n_accepted"] + st["n_rejected"]) and st["t_final"] == span[1]
    assert np.array_equal(y, ref.y[:, -1])


def test_encode_direction_rejects_steps():
    """the rejection branch is exercised (the encoding runs reject up to three attempts)"""
    rej = [S.rk45_host_solve(gaussian_rhs(s0), 1e-3, 1.0, start(s0, 1e-3, 2048), 1e-5, 1e-5)[1]["n_rejected"] for s0 in (0.5, 1.0, 2.0)]
    assert min(rej) >= 1, rej


# ---- 2. one controller per sample ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("span", [(1.0, 1e-3), (1e-3, 1.0)], ids=["sample", "encode"])
def test_sample_mode_rows_do_not_depend_on_their_batch(span):
    s0 = np.array([0.5, 1.0, 2.0])
    y0 = np.stack([start(s, span[0], 1024, seed=i) for i, s in enumerate(s0)])
    y, st = S.rk45_host_solve(gaussian_rhs(s0), span[0], span[1], y0, 1e-5, 1e-5, error_norm="sample")
    assert y.shape == (3, 1024) and st["nfev"].shape == (3,)
    for b in range(3):
        y1, st1 = S.rk45_host_solve(gaussian_rhs(s0[b:b + 1]), span[0], span[1], y0[b:b + 1], 1e-5, 1e-5, error_norm="sample")
        assert np.array_equal(y[b], y1[0]), b
        assert (st["nfev"][b], st["n_accepted"][b], st["n_rejected"][b]) == (st1["nfev"][0], st1["n_accepted"][0], st1["n_rejected"][0])
        # and a one-row sample-mode solve is the batch-mode solve of that row
        yb, stb = S.rk45_host_solve(gaussian_rhs(s0[b]), span[0], span[1], y0[b], 1e-5, 1e-5)
        assert np.array_equal(yb, y1[0]) and stb["nfev"] == st1["nfev"][0]
    assert len(set(st["nfev"].tolist())) > 1, st["nfev"]            # the rows really took different numbers of steps
    assert np.all(st["t_final"] == span[1])
    # the flat form with `batch`
    y2, _ = S.rk45_host_solve(lambda t, x: gaussian_rhs(s0)(t, x), span[0], span[1], y0.reshape(-1), 1e-5, 1e-5, error_norm="sample", batch=3)
    assert np.array_equal(y2.reshape(3, 1024), y)


# ---- 3. failure paths ----------------------------------------------------------------------------------------------------------------------
def test_nan_right_hand_side_raises_at_once():
    calls = []

    def f(t, x):
        calls.append(t)
        return np.full_like(x, np.nan) if len(calls) > 4 else gaussian_rhs(1.0)(t, x)
    with pytest.raises(SS.OdeSolverError, match="non-finite error norm"):
        S.rk45_host_solve(f, 1.0, 1e-3, start(1.0, 1.0, 256), 1e-5, 1e-5)
    assert len(calls) == 8                                            # the attempt that saw the NaN was the last
    calls.clear()
    with pytest.raises(SS.OdeSolverError, match="non-finite error norm"):
        S.rk45_host_solve(lambda t, x: np.full_like(x, np.nan), 1.0, 1e-3, start(1.0, 1.0, 256), 1e-5, 1e-5)


def test_step_budget_raises():
    with pytest.raises(SS.OdeSolverError, match=r"step budget \(max_steps=3\)"):
        S.rk45_host_solve(gaussian_rhs(1.0), 1.0, 1e-3, start(1.0, 1.0, 256), 1e-5, 1e-5, max_steps=3)
    y, st = S.rk45_host_solve(gaussian_rhs(1.0), 1.0, 1e-3, start(1.0, 1.0, 256), 1e-3, 1e-3, max_steps=4)
    assert st["n_accepted"] + st["n_rejected"] == 4                   # a budget that is just enough is not an error


# ---- 4. argument validation happens before any device work ---------------------------------------------------------------------------------
def must_not_be_called(*a, **k):
    raise AssertionError("the score model was called")


@pytest.mark.parametrize("kw,match", [
    (dict(t_span=(1.0, 1e-4)), "t_span"),
    (dict(t_span=(1.5, 1e-3)), "t_span"),
    (dict(t_span=(0.5, 0.5)), "t_span"),
    (dict(t_span=(1e-3, 1.0)), "pass it as z"),
    (dict(tile_origins=torch.zeros(2, 2, dtype=torch.int32)), "error_norm='sample'"),
    (dict(error_norm="tile"), "error_norm"),
    (dict(rtol=0.0), "rtol"),
    (dict(rtol=-1e-3), "rtol"),
    (dict(atol=-1.0), "atol"),
    (dict(max_steps=0), "max_steps"),
    (dict(z=torch.zeros(2, 1, 32, 32), noise=torch.zeros(1, 2, 1, 32, 32)), "not both"),
    (dict(z=torch.zeros(2, 32, 32)), "z must be"),
])
def test_arguments_are_checked_before_any_device_work(kw, match):
    with pytest.raises(ValueError, match=match):
        S.rk45_sampler(must_not_be_called, S.marginal_prob_std_fn, S.diffusion_coeff_fn, batch_size=2, device="cuda", img_size=32, **kw)
    with pytest.raises(ValueError):
        SS.rk45_host_solve(must_not_be_called, 1.0, 1e-3, np.zeros(4), -1.0, 1e-5)


# ---- 5. config wiring ------------------------------------------------------------------------------------------------------------------------
def test_config_dispatch_and_ode_sampler_kwargs():
    import sbgm
    from sbgm_danra_amd import training
    from sbgm_danra_amd.evaluate_sbgm import generation
    assert training._SAMPLERS["rk45_sampler"] is S.rk45_sampler is sbgm.score_sampling.rk45_sampler
    assert generation.rk45_sampler is S.rk45_sampler
    assert training._SAMPLERS["ode_sampler"] is S.ode_sampler         # the scipy-driven sampler keeps its name and place
    assert SS.ode_sampler_kwargs({}) == {} and SS.ode_sampler_kwargs(None) == {} and SS.ode_sampler_kwargs({"ode": None}) == {}
    got = SS.ode_sampler_kwargs({"ode": {"rtol": "1e-4", "atol": 1e-6, "error_norm": "sample", "max_steps": 500, "other": 1}})
    assert got == {"rtol": 1e-4, "atol": 1e-6, "error_norm": "sample", "max_steps": 500}
    assert isinstance(got["max_steps"], int)
    assert SS.ode_sampler_kwargs({"ode": {"rtol": 1e-3}}) == {"rtol": 1e-3}
    assert SS._counts(S._native.SAMPLER_RK45, 0) == (6, 1)
    import inspect
    sig = inspect.signature(S.rk45_sampler)
    assert list(sig.parameters)[:13] == ["score_model", "marginal_prob_std", "diffusion_coeff", "batch_size", "device", "eps", "img_size",
                                         "y", "cond_img", "lsm_cond", "topo_cond", "cfg", "rtol"]
    assert sig.parameters["rtol"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["error_norm"].default == "batch"
