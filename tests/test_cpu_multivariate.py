"""CPU suite for the multivariate ensemble scores: the numpy restatement (tests/multivariate_ref.py) against a brute-force double
loop and against properties known in closed form, the offset table, the argument checks of the two device wrappers (they fire
before anything touches the device), the new C symbols, and how evaluate mode reads `evaluation.multivariate_scores` — with
the section absent it runs exactly the statistics it ran before."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch
import yaml

import multivariate_ref as R
from sbgm_danra_amd import _native as N
from sbgm_danra_amd import verification as V
from sbgm_danra_amd._native import NativeError
from sbgm_danra_amd.config_loader import load_config, to_config
from sbgm_danra_amd.evaluate_sbgm import evaluation as E
from sbgm_danra_amd.evaluate_sbgm import evaluation_main as EM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "sbgm_danra_amd", "config", "default_config.yaml")


def _case(seed=0, M=3, H=4, W=5):
    rng = np.random.default_rng(seed)
    ens = rng.normal(size=(M, H, W)).astype(np.float32)
    obs = rng.normal(size=(H, W)).astype(np.float32)
    mask = np.ones((H, W), np.uint8)
    mask[1, 2] = 0
    ens[1, 3, 0] = np.nan
    obs[0, 4] = np.nan
    return ens, obs, mask


# ---- the restatement against brute force -------------------------------------------------------------------------------------

def test_energy_restatement_against_a_double_loop():
    ens, obs, mask = _case()
    M, H, W = ens.shape
    rows = list(ens) + [obs]
    valid = [(y, x) for y in range(H) for x in range(W)
             if mask[y, x] and not math.isnan(obs[y, x]) and not any(math.isnan(e[y, x]) for e in ens)]
    assert len(valid) == H * W - 3
    d2 = [[sum((float(a[p]) - float(b[p])) ** 2 for p in valid) for b in rows] for a in rows]
    dist = [[math.sqrt(v / len(valid)) for v in row] for row in d2]
    obs_mean = sum(dist[m][M] for m in range(M)) / M
    pair = sum(dist[m][k] for m in range(M) for k in range(M) if m != k)
    r = R.energy_scores(ens, obs, mask)
    np.testing.assert_allclose(r["dist2"], d2, rtol=1e-14, atol=0)
    want = [len(valid), obs_mean - pair / (2 * M * (M - 1)), obs_mean - pair / (2 * M * M), obs_mean, pair / (M * (M - 1)),
            min(dist[m][k] for m in range(M) for k in range(M) if m != k)]
    np.testing.assert_allclose(r["scores"], want, rtol=1e-14)
    assert dict(zip(R.ENERGY_KEYS, want)).keys() == dict.fromkeys(V.ENERGY_KEYS).keys()


@pytest.mark.parametrize("order,weights", [(0.5, "inverse_distance"), (1.0, "unit"), (2.0, "inverse_distance")])
def test_variogram_restatement_against_a_double_loop(order, weights):
    ens, obs, mask = _case(1)
    M, H, W = ens.shape
    ok = R.valid_pixels(ens, obs, mask)
    offs = R.offsets(2)
    vs_map = np.zeros((H, W))
    ge_s, go_s, n_s = np.zeros(len(offs)), np.zeros(len(offs)), np.zeros(len(offs), int)
    num = den = unum = cond = 0.0
    for y in range(H):
        for x in range(W):
            for k, (dy, dx) in enumerate(offs):
                yy, xx = y + dy, x + dx
                if not (yy < H and 0 <= xx < W and ok[y, x] and ok[yy, xx]):
                    continue
                w = float(np.float32(1 / math.sqrt(dy * dy + dx * dx))) if weights == "inverse_distance" else 1.0
                ge = sum(float(np.float32(abs(np.float32(e[y, x] - e[yy, xx])) ** np.float32(order))) for e in ens) / M
                go = float(np.float32(abs(np.float32(obs[y, x] - obs[yy, xx])) ** np.float32(order)))
                t = (go - ge) ** 2
                vs_map[y, x] += w * t
                ge_s[k] += ge
                go_s[k] += go
                n_s[k] += 1
                num, den, unum, cond = num + w * t, den + w, unum + t, cond + w * 2 * abs(go - ge) * ge
    r = R.variogram_scores(ens, obs, radius=2, order=order, weights=weights, mask=mask)
    tol = dict(rtol=3e-7 if order == 0.5 else 1e-13, atol=1e-12)    # python's fp32 pow against sqrt: within an fp32 ulp per term
    np.testing.assert_array_equal(r["pairs"], n_s)
    np.testing.assert_array_equal(np.isnan(r["vs_map"]), ~ok)
    np.testing.assert_allclose(np.nan_to_num(r["vs_map"]), vs_map, **tol)
    np.testing.assert_allclose(r["gamma_ens"], ge_s / n_s, **tol)
    np.testing.assert_allclose(r["gamma_obs"], go_s / n_s, **tol)
    np.testing.assert_allclose(r["scores"], [num / den, n_s.sum(), den, unum / n_s.sum()], **tol)
    np.testing.assert_allclose(r["cond"], cond / den, **tol)
    assert r["offsets"].tolist() == [list(o) for o in offs]


def test_fair_energy_score_of_a_one_pixel_field_is_the_fair_crps():
    rng = np.random.default_rng(2)
    x, y = rng.normal(size=7).astype(np.float32), np.float32(0.3)
    r = R.energy_scores(x.reshape(7, 1, 1), np.full((1, 1), y, np.float32))
    xd = x.astype(np.float64)
    crps_fair = np.abs(xd - float(y)).mean() - np.abs(xd[:, None] - xd[None, :]).sum() / (2 * 7 * 6)
    crps_std = np.abs(xd - float(y)).mean() - np.abs(xd[:, None] - xd[None, :]).sum() / (2 * 7 * 7)
    assert r["scores"][0] == 1
    np.testing.assert_allclose(r["scores"][1:3], [crps_fair, crps_std], rtol=1e-14)


def test_variogram_is_invariant_to_a_common_shift_and_sees_the_covariance():
    rng = np.random.default_rng(3)
    ens = (rng.integers(-20, 20, size=(4, 9, 11)) * 0.25).astype(np.float32)
    obs = (rng.integers(-20, 20, size=(9, 11)) * 0.25).astype(np.float32)
    for order in (0.5, 1.0, 2.0):
        a = R.variogram_scores(ens, obs, radius=3, order=order)
        b = R.variogram_scores(ens + np.float32(64), obs + np.float32(64), radius=3, order=order)
        for k in ("vs_map", "gamma_ens", "gamma_obs", "pairs", "scores"):
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    # members equal to the truth up to a constant each: every difference agrees, the score is exactly 0
    same = np.stack([obs + np.float32(c) for c in (0, 1, -2)])
    z = R.variogram_scores(same, obs, radius=2, order=1.0)
    assert z["scores"][0] == 0 and z["scores"][3] == 0 and z["scores"][1] == z["pairs"].sum() > 0
    e = R.energy_scores(same, obs)
    assert e["scores"][5] == 1.0 and e["dist2"][0, 3] == 0                    # ... which the energy score does see as distance


def test_offset_table():
    for radius, n in ((1, 2), (2, 6), (8, 98)):
        offs = V.variogram_offsets(radius)
        assert len(offs) == n == len(R.offsets(radius)) and offs == R.offsets(radius)
        assert all((dy > 0 or (dy == 0 and dx > 0)) and dy * dy + dx * dx <= radius * radius for dy, dx in offs)
        assert len(set(offs)) == n and offs == sorted(offs)
        full = {(dy, dx) for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1)
                if 0 < dy * dy + dx * dx <= radius * radius}
        assert set(offs) | {(-dy, -dx) for dy, dx in offs} == full            # each unordered pair once
        cnt, buf = C.c_int(), (C.c_int * (2 * V.MAX_VARIOGRAM_OFFSETS))()
        N.check(N.lib().sbgm_variogram_offsets(radius, C.byref(cnt), buf))          # the table the C entry point builds
        assert [(buf[2 * k], buf[2 * k + 1]) for k in range(cnt.value)] == offs
    assert V.MAX_VARIOGRAM_OFFSETS == 98
    for bad in (0, 9, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="radius"):
            V.variogram_offsets(bad)
    assert N.lib().sbgm_variogram_offsets(9, C.byref(C.c_int()), (C.c_int * 196)()) != 0


# ---- the wrappers and the C ABI ---------------------------------------------------------------------------------------------

def test_symbols_and_abi_version():
    names = ("sbgm_energy_scores", "sbgm_energy_scores_workspace_bytes", "sbgm_variogram_scores", "sbgm_variogram_scores_workspace_bytes",
             "sbgm_variogram_offsets")
    lib = N.lib()
    for name in names:
        assert name in N.SIGNATURES and getattr(lib, name) is not None
    assert lib.sbgm_abi_version() == N.ABI_VERSION >= 10
    header = open(os.path.join(ROOT, "include", "sbgm_hip.h")).read()
    assert all(f"{name}(" in header for name in names)
    assert V.ENERGY_KEYS == R.ENERGY_KEYS and V.VARIOGRAM_KEYS == R.VARIOGRAM_KEYS
    # the workspace queries answer on the host, and with 0 for what the calls reject
    assert lib.sbgm_energy_scores_workspace_bytes(16, 589 * 789) > 589 * 789
    assert lib.sbgm_variogram_scores_workspace_bytes(16, 589, 789, 8) > 589 * 789
    assert lib.sbgm_energy_scores_workspace_bytes(1, 100) == 0 and lib.sbgm_energy_scores_workspace_bytes(4096, 100) == 0
    assert lib.sbgm_variogram_scores_workspace_bytes(4, 8, 8, 9) == 0 and lib.sbgm_variogram_scores_workspace_bytes(4, 8, 8, 0) == 0
    # null pointers and bad sizes are refused by the entry points themselves, before any launch
    assert lib.sbgm_energy_scores(None, None, None, 0, 4, 100, None, None, None, 0, None) != 0
    assert lib.sbgm_variogram_scores(None, None, None, 0, 4, 8, 8, 2, 0.5, 1, None, None, None, None, None, None, 0, None) != 0


def test_wrappers_check_before_the_device():
    ens, obs = torch.zeros(3, 8, 9), torch.zeros(8, 9)
    bad = [dict(ens=torch.zeros(1, 8, 9)), dict(ens=torch.zeros(4096, 2, 2), obs=torch.zeros(2, 2)), dict(ens=torch.zeros(8, 9)),
           dict(obs=torch.zeros(9, 8)), dict(obs=torch.zeros(2, 8, 9)), dict(mask=torch.ones(2, 8, 9)), dict(mask=torch.ones(8, 8)),
           dict(ens=torch.zeros(2, 1025, 1024), obs=torch.zeros(1025, 1024)), dict(ens=torch.zeros(3, 8, 9, dtype=torch.int32))]
    for kw in bad:
        args = dict(ens=ens, obs=obs)
        args.update(kw)
        with pytest.raises((ValueError, TypeError)):
            V.energy_scores(**args)
        with pytest.raises((ValueError, TypeError)):
            V.variogram_scores(**args)
    for kw in (dict(radius=0), dict(radius=9), dict(radius=2.5), dict(order=0.7), dict(order=3), dict(order="1"), dict(order=True),
               dict(weights="distance"), dict(weights=None)):
        with pytest.raises(ValueError):
            V.variogram_scores(ens, obs, **kw)
    with pytest.raises(NativeError):                                         # well-formed arguments reach the device check
        V.energy_scores(ens, obs)
    with pytest.raises(NativeError):
        V.variogram_scores(ens, obs, radius=8, order=2, weights="unit", mask=torch.ones(8, 9, dtype=torch.bool))


# ---- evaluation.multivariate_scores in the config ---------------------------------------------------------------------------

def test_multivariate_section_parsing():
    full = {"energy": True, "variogram": {"radius": 3, "order": 1, "weights": "unit"}}
    c = to_config({"evaluation": {"multivariate_scores": full}})
    assert E.multivariate_scores_config(c) == (True, {"radius": 3, "order": 1.0, "weights": "unit"})
    assert EM.unit_statistics(c, "repeated") == ["pixel_stats", "spatial_stats", "multivariate_stats"]
    assert EM.unit_statistics(c, "multiple") == ["pixel_stats", "spatial_stats"] == EM.unit_statistics(c, "single")
    sec = lambda s: E.multivariate_scores_config(to_config({"evaluation": {"multivariate_scores": s}}))  # noqa: E731
    assert sec({"energy": True}) == (True, None)
    assert sec({"variogram": {}}) == (False, {"radius": 4, "order": 0.5, "weights": "inverse_distance"})
    assert sec({"energy": False, "variogram": {"order": 2}}) == (False, {"radius": 4, "order": 2.0, "weights": "inverse_distance"})
    for broken, key in (({}, "multivariate_scores"), ({"energy": False}, "multivariate_scores"), ({"energy": 1}, "energy"),
                        ({"energy": "yes"}, "energy"), ({"energy": True, "fss": True}, "multivariate_scores"),
                        ({"variogram": {"radius": 0}}, "radius"), ({"variogram": {"radius": 9}}, "radius"),
                        ({"variogram": {"radius": 2.0}}, "radius"), ({"variogram": {"radius": True}}, "radius"),
                        ({"variogram": {"order": 0.7}}, "order"), ({"variogram": {"order": "0.5"}}, "order"),
                        ({"variogram": {"weights": "distance"}}, "weights"), ({"variogram": {"weights": 1}}, "weights"),
                        ({"variogram": {"p": 0.5}}, "variogram"), ({"variogram": 4}, "variogram"), ([True], "multivariate_scores")):
        with pytest.raises(ValueError, match=key):
            sec(broken)


def test_absent_multivariate_section_leaves_the_statistics_unchanged():
    assert E.multivariate_scores_config(load_config(CFG)) is None            # the shipped defaults do not opt in
    assert "multivariate_scores" not in yaml.safe_load(open(CFG))["evaluation"]
    for ev in ({}, {"eval_stat_methods": ["daily_stats", "ensemble_stats"]}, {"object_scores": {"thresholds": [1.0]}}):
        c = to_config({"evaluation": ev})
        assert E.multivariate_scores_config(c) is None
        for t in E.GEN_TYPES:
            assert "multivariate_stats" not in EM.unit_statistics(c, t)
    assert not set(EM.MULTIVARIATE_METHODS) & set(EM.METHODS)                  # and it is no eval_stat_methods name
    with pytest.raises(ValueError, match="multivariate_stats"):
        EM.eval_stat_methods(to_config({"evaluation": {"eval_stat_methods": ["multivariate_stats"]}}))
    assert hasattr(E.Evaluation, "multivariate_statistics")
