"""CPU suite for the row-keyed, temporally correlated sampling noise: the weights and their autocorrelation against the closed form, the
statistics of the reference mix over the host Philox draws, the two new keys of `evaluation.series`, the C ABI, and the samplers'
argument checks, which fire before anything touches a device."""
import os
import re

import numpy as np
import pytest
import torch

import philox_ref as P
import temporal_noise_ref as R
import sbgm_danra_amd as S
from sbgm_danra_amd import _native as N
from sbgm_danra_amd import score_sampling as SS
from sbgm_danra_amd.config_loader import to_config
from sbgm_danra_amd.evaluate_sbgm import generation as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STD = (S.marginal_prob_std_fn, S.diffusion_coeff_fn)
CASES = [(0.6, 32), (0.6, 8), (0.9, 32), (0.3, 4), (-0.5, 16), (0, 1)]


# ---- 1: weights and acf -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rho,lags", CASES)
def test_weights_are_normalised_and_their_acf_is_the_closed_form(rho, lags):
    w = SS.temporal_noise_weights(rho, lags)
    assert w.dtype == np.float32 and w.shape == (lags,)
    assert np.array_equal(w.view(np.uint32), R.weights(rho, lags).view(np.uint32))
    ss = float((w.astype(np.float64) ** 2).sum())
    acf = SS.temporal_noise_acf(w)
    err = float(np.abs(acf - R.acf_closed(rho, lags)).max())
    print(f"rho {rho} lags {lags}: |sum w^2 - 1| = {abs(ss - 1):.2e}, max |acf - closed form| = {err:.2e}")
    assert abs(ss - 1.0) <= 1e-6
    assert acf.dtype == np.float64 and acf.shape == (lags,) and err <= 1e-6
    if (rho, lags) == (0, 1):
        assert w.tolist() == [1.0]


def test_white_weights_and_refused_parameters():
    assert SS.temporal_noise_weights(0.0, 5).tolist() == [1.0, 0.0, 0.0, 0.0, 0.0]
    assert SS.temporal_noise_weights(0.7, 1).tolist() == [1.0]
    for rho, lags in ((1.0, 4), (-1.0, 4), (0.5, 0), (0.5, 33)):
        with pytest.raises(ValueError, match="rho" if abs(rho) >= 1 else "lags"):
            SS.temporal_noise_weights(rho, lags)


# ---- 2: the reference mix has the stated second moments ----------------------------------------------------------------------------------
def test_reference_mix_has_unit_variance_and_the_weights_acf():
    rows, per, K, seed = 64, 1024, 8, 1234 + (7 << 32)
    w = R.weights(0.6, K)
    acf = SS.temporal_noise_acf(w)
    plain = P.draw(seed, 3, (rows + K - 1) * per).astype(np.float32)
    z = R.mix_rows(plain, range(K - 1, K - 1 + rows), per, w).astype(np.float64)        # [64, 1024]: consecutive rows
    n0 = z.size
    var = float((z * z).mean())
    print(f"lag 0: variance {var:.5f} (5 se = {5 / np.sqrt(n0):.5f})")
    assert abs(var - acf[0]) <= 5 / np.sqrt(n0)
    for j in (1, 2):
        n = (rows - j) * per
        c = float((z[:-j] * z[j:]).mean())
        print(f"lag {j}: correlation {c:.5f}, acf {acf[j]:.5f} (5 se = {5 / np.sqrt(n):.5f})")
        assert abs(c - acf[j]) <= 5 / np.sqrt(n)
    # the float32 loop is the definition: a float64 mix of the same draws is close to it and is not it
    wide = sum(float(w[k]) * plain[(K - 1 - k) * per:(K - k) * per].astype(np.float64) for k in range(K))
    assert np.abs(z[0] - wide).max() <= 16 * 2.0 ** -23 * np.abs(wide).max() and not np.array_equal(z[0], wide)


# ---- 3: evaluation.series.seed / temporal_noise ------------------------------------------------------------------------------------------
def _series(sec):
    return to_config({"evaluation": {"series": sec}})


def test_series_noise_config():
    assert G.series_noise_config(to_config({"evaluation": {}})) == (None, None)
    assert G.series_noise_config(_series({"members": 3})) == (None, None)
    seed, w = G.series_noise_config(_series({"seed": 5}))
    assert seed == 5 and w.dtype == np.float32 and w.tolist() == [1.0]
    seed, w = G.series_noise_config(_series({"temporal_noise": {"rho": 0.6, "lags": 4}}))
    assert seed is None and np.array_equal(w, SS.temporal_noise_weights(0.6, 4))
    seed, w = G.series_noise_config(_series({"members": 2, "seed": 2 ** 40, "temporal_noise": {"weights": [0.6, 0.8]}}))
    assert seed == 2 ** 40 and np.array_equal(w, np.array([0.6, 0.8], dtype=np.float32))
    broken = [({"seed": -1}, "seed"), ({"seed": 1.5}, "seed"), ({"seed": True}, "seed"), ({"seed": 2 ** 63}, "seed"),
              ({"temporal_noise": 3}, "temporal_noise"), ({"temporal_noise": {"rho": 0.5}}, "temporal_noise"),
              ({"temporal_noise": {"rho": 0.5, "lags": 4, "weights": [1.0]}}, "temporal_noise"),
              ({"temporal_noise": {"rho": 1.0, "lags": 4}}, "rho"), ({"temporal_noise": {"rho": "a", "lags": 4}}, "rho"),
              ({"temporal_noise": {"rho": 0.5, "lags": 0}}, "lags"), ({"temporal_noise": {"rho": 0.5, "lags": 33}}, "lags"),
              ({"temporal_noise": {"rho": 0.5, "lags": 2.0}}, "lags"), ({"temporal_noise": {"weights": [0.5, 0.5]}}, "weights"),
              ({"temporal_noise": {"weights": []}}, "weights"), ({"temporal_noise": {"weights": [1.0] + [0.0] * 32}}, "weights"),
              ({"temporal_noise": {"weights": ["x"]}}, "weights")]
    for sec, key in broken:
        with pytest.raises(ValueError, match=key):
            G.series_noise_config(_series(sec))


def test_series_config_is_what_it_was():
    assert G.series_config(to_config({"evaluation": {}})) == (1, None)
    assert G.series_config(_series({"members": 3, "max_days": 10})) == (3, 10)
    assert G.series_config(_series({"members": 2, "seed": 7, "temporal_noise": {"rho": 0.6, "lags": 4}})) == (2, None)
    for sec, key in (({"members": 0}, "members"), ({"max_days": True}, "max_days"), ({"days": 3}, "series")):
        with pytest.raises(ValueError, match=key):
            G.series_config(_series(sec))


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------------
def test_symbols_and_abi_version():
    lib = N.lib()
    header = open(os.path.join(ROOT, "include", "sbgm_hip.h")).read()
    assert lib.sbgm_abi_version() == N.ABI_VERSION >= 15
    for name, n in (("sbgm_sampler_set_noise_rows", 5), ("sbgm_randn_rows", 11)):
        assert name in N.SIGNATURES and getattr(lib, name) is not None and len(N.SIGNATURES[name][1]) == n
        decl = re.search(rf"\bint {name}\((.*?)\);", header, flags=re.S).group(1)
        assert decl.count(",") + 1 == n, name
    # no device is touched by a refused call
    assert lib.sbgm_sampler_set_noise_rows(None, None, 1, None, 0) != 0 and b"null model" in lib.sbgm_last_error()
    assert lib.sbgm_randn_rows(None, 1.0, 0, 0, None, 1, 4, 1, None, 1, None) != 0 and b"randn_rows" in lib.sbgm_last_error()


# ---- 4: the samplers' argument checks ------------------------------------------------------------------------------------------------------
def _never(*a, **k):
    raise AssertionError("the score model must not be evaluated")


SAMPLERS = {"em": (S.Euler_Maruyama_sampler, {}), "pc": (S.pc_sampler, {}), "edm": (S.edm_heun_sampler, {}),
            "dpm": (S.dpmpp_2m_sampler, {"eta": 1.0}), "rk45": (S.rk45_sampler, {})}


@pytest.mark.parametrize("kind", list(SAMPLERS))
def test_sampler_argument_checks_name_the_argument(kind):
    sampler, kw = SAMPLERS[kind]
    B, hw = 3, 32
    steps = {} if kind == "rk45" else {"num_steps": 4}
    run = lambda **how: sampler(_never, *STD, batch_size=B, device="cpu", img_size=hw, seed=1, **steps, **kw, **how)  # noqa: E731
    w3 = SS.temporal_noise_weights(0.6, 3)
    noise = torch.zeros(9, B, 1, hw, hw)
    origins = torch.zeros(B, 2, dtype=torch.int32)
    cases = [(dict(noise_rows=[4, 5]), "noise_rows"),                                                   # wrong length
             (dict(noise_rows=torch.tensor([[4, 5, 6]])), "noise_rows"),
             (dict(noise_rows=[4.0, 5.0, 6.0]), "noise_rows"),
             (dict(noise_rows=[4, -1, 6]), "noise_rows"),                                               # negative
             (dict(noise_rows=[4, 3, 6], noise_weights=w3, noise_row_stride=2), "noise_rows"),          # below (K - 1) * stride = 4
             (dict(noise_rows=[40, 41, 42], noise_weights=np.full(33, 33 ** -0.5)), "noise_weights"),   # K > 32
             (dict(noise_rows=[4, 5, 6], noise_weights=[0.6, 0.7]), "noise_weights"),                   # sum w^2 = 0.85
             (dict(noise_rows=[4, 5, 6], noise_weights=[]), "noise_weights"),
             (dict(noise_rows=[4, 5, 6], noise_row_stride=0), "noise_row_stride"),
             (dict(noise_weights=w3), "noise_rows"), (dict(noise_row_stride=2), "noise_rows"),          # a plan needs its rows
             (dict(noise_rows=[4, 5, 6], noise=noise), "noise"),
             (dict(noise_rows=[4, 5, 6], tile_origins=origins, **({"error_norm": "sample"} if kind == "rk45" else {})), "tile_origins")]
    if kind == "rk45":
        cases.append((dict(noise_rows=[4, 5, 6], z=torch.zeros(B, 1, hw, hw)), "z"))
    else:
        cases.append((dict(noise_rows=[4, 5, 6], tile_origins=origins, domain_width=64, joint_tiles=(64, 8)), "noise_rows"))
    for how, name in cases:
        with pytest.raises(ValueError, match=name):
            run(**how)
    # a plan that passes the checks reaches the loop: a callable that is no ScoreNet has no native loop to carry it
    with pytest.raises(N.NativeError, match="noise_rows"):
        run(noise_rows=torch.tensor([4, 5, 6]), noise_weights=w3, noise_row_stride=2)


def test_temporal_noise_checks_before_the_device():
    for how, name in ((dict(rows=[2, 1], per_sample=8, weights=SS.temporal_noise_weights(0.5, 3)), "noise_rows"),
                      (dict(rows=[2, 3], per_sample=6), "per_sample"), (dict(rows=[2, 3], per_sample=8, weights=[2.0]), "noise_weights"),
                      (dict(rows=[2, 3], per_sample=8, stride=0), "noise_row_stride")):
        with pytest.raises(ValueError, match=name):
            SS.temporal_noise(1, 0, **how)
    with pytest.raises(N.NativeError, match="device"):
        SS.temporal_noise(1, 0, [2, 3], 8, device="cpu")
