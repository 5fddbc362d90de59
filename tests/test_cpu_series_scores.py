"""CPU suite for the pooled ensemble verification of a series: the numpy restatement of the contract (tests/series_scores_ref.py)
against brute-force loops and closed forms (the leave-one-out identity among them); the C ABI; the argument checks of the device
wrapper (they fire before anything touches the device); how evaluate mode reads `evaluation.series_scores`; and the errors of
Evaluation.series_ensemble_statistics that need no device."""
import os

import numpy as np
import pytest
import torch
import yaml

import series_scores_ref as R
from sbgm_danra_amd import _native as N
from sbgm_danra_amd import verification as V
from sbgm_danra_amd._native import NativeError
from sbgm_danra_amd.config_loader import load_config, to_config
from sbgm_danra_amd.evaluate_sbgm import evaluation as E
from sbgm_danra_amd.evaluate_sbgm import evaluation_main as EM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "sbgm_danra_amd", "config", "default_config.yaml")
f32 = np.float32


# ---- the restatement ------------------------------------------------------------------------------------------------------------

def _fair_crps(members, y):
    """fair CRPS of a Python list of members against y, float64"""
    m = len(members)
    a = sum(abs(np.float64(x) - np.float64(y)) for x in members) / m
    b = sum(abs(np.float64(x) - np.float64(z)) for x in members for z in members)
    return a - b / (2.0 * m * (m - 1))


def test_leave_one_out_identity():
    """the sum over the days of the fair CRPS of the leave-one-out ensemble of the other days is S / (2 (n - 1)), S the sum over
    the ordered pairs of |y_i - y_j|"""
    rng = np.random.default_rng(5)
    for n in list(range(3, 41)):
        y = (rng.integers(0, 40, size=n) * 0.25).astype(f32) if n % 2 else rng.gamma(0.7, 3.0, size=n).astype(f32)
        direct = sum(_fair_crps([y[j] for j in range(n) if j != i], y[i]) for i in range(n))
        S = sum(abs(np.float64(a) - np.float64(b)) for a in y for b in y)
        assert direct == pytest.approx(S / (2.0 * (n - 1)), rel=1e-12)


def _small_case():
    rng = np.random.default_rng(11)
    D, M, H, W = 9, 5, 3, 4
    ens = (rng.integers(0, 13, size=(D, M, H, W)) * 0.25).astype(f32)
    obs = (rng.integers(0, 13, size=(D, H, W)) * 0.25).astype(f32)
    ens[rng.random(ens.shape) < 0.03] = np.nan
    obs[rng.random(obs.shape) < 0.05] = np.nan
    obs[:, 0, 0] = np.nan                                     # no valid day
    obs[2:, 0, 1] = np.nan                                    # two valid days at most: no reference
    obs[:, 0, 2], ens[:, :, 0, 2] = 1.0, (rng.integers(0, 13, size=(D, M)) * 0.25).astype(f32)      # constant truth
    mask = rng.random((H, W)) < 0.9
    mask[0, :3] = True
    groups = np.array([0, 0, 1, 1, 1, 2, 2, 0, 1])
    return ens, obs, mask, groups


def test_restatement_against_brute_force_loops():
    ens, obs, mask, groups = _small_case()
    thr = [0.5, 1.0]
    r = R.series_ensemble_scores(ens, obs, thr, groups, mask, seed=3)
    D, M, H, W = ens.shape
    valid = R.valid_cells(ens, obs, mask)
    assert r["count"][0, 0] == 0 and r["count"][0, 1] <= 2 and (r["count"] >= 3).any() and set(r) >= set(R.KEYS)
    assert r["scores"].shape == (4, 6) and r["rank_hist"].shape == (4, M + 1) and r["table"].shape == (4, 2, M + 1, 2)
    for i in range(H):
        for j in range(W):
            days = [d for d in range(D) if valid[d, i, j]]
            assert r["count"][i, j] == len(days)
            if not days:
                assert all(np.isnan(r[k][i, j]) for k in R.MAP_KEYS + R.CLIM_MAP_KEYS)
                continue
            crps = [_fair_crps(list(ens[d, :, i, j]), obs[d, i, j]) for d in days]
            assert r["crps"][i, j] == pytest.approx(np.mean(crps), rel=1e-6, abs=1e-7)
            var = [np.var(ens[d, :, i, j].astype(np.float64), ddof=1) for d in days]
            se = [(ens[d, :, i, j].astype(np.float64).mean() - obs[d, i, j]) ** 2 for d in days]
            assert r["spread"][i, j] == pytest.approx(np.sqrt(np.mean(var)), rel=1e-6)
            assert r["skill"][i, j] == pytest.approx(np.sqrt(np.mean(se)), rel=1e-6, abs=1e-7)
            if len(days) < 3:
                assert np.isnan(r["clim_crps"][i, j]) and np.isnan(r["crpss"][i, j])
                continue
            ref = [_fair_crps([obs[e, i, j] for e in days if e != d], obs[d, i, j]) for d in days]
            assert r["clim_crps"][i, j] == pytest.approx(np.mean(ref), rel=1e-6, abs=1e-7)
            if sum(ref) == 0:
                assert np.isnan(r["crpss"][i, j])
            else:
                assert r["crpss"][i, j] == pytest.approx(1 - sum(crps) / sum(ref), rel=1e-5, abs=1e-6)
    assert np.isnan(r["crpss"][0, 2]) and r["clim_crps"][0, 2] == 0                 # constant truth: C = 0
    # rows: the group rows add up to row 0, and the group scores are those of the group's days alone
    np.testing.assert_array_equal(r["rank_hist"][1:].sum(0), r["rank_hist"][0])
    np.testing.assert_array_equal(r["table"][1:].sum(0), r["table"][0])
    assert r["rank_hist"][0].sum() == valid.sum() == r["scores"][0, 0] and (r["table"][0, :, :, 0].sum(1) == valid.sum()).all()
    for g in range(3):
        sel = groups == g
        sub = R.series_ensemble_scores(ens[sel], obs[sel], thr, None, mask, seed=3)
        np.testing.assert_allclose(r["scores"][1 + g], sub["scores"][0], rtol=1e-12)
        np.testing.assert_array_equal(r["table"][1 + g], sub["table"][0])
        np.testing.assert_allclose(r["exceedance"][1 + g], sub["exceedance"][0], rtol=1e-12)
        np.testing.assert_allclose(r["skill_scores"][1 + g], sub["skill_scores"][0], rtol=1e-12)
    # the table and its scores against the direct definitions
    for t, th in enumerate(thr):
        k = (ens >= f32(th)).sum(1)[valid]
        o = (obs >= f32(th))[valid]
        assert r["exceedance"][0, 0, t] == pytest.approx(((k / M - o) ** 2).mean(), rel=1e-12)
        assert r["exceedance"][0, 4, t] == pytest.approx(o.mean(), rel=1e-12)
    # ranks lie between the strict and the weak count, and the sorted pair sum is the direct one
    rk = R.ranks(ens, obs, 3)
    with np.errstate(invalid="ignore"):
        assert ((rk >= (ens < obs[:, None]).sum(1)) & (rk <= (ens <= obs[:, None]).sum(1)))[valid].all()
    rows = [np.ones(D, bool)] + [groups == g for g in range(3)]
    direct = R.pair_sums(obs, valid, rows)
    old, R.SORTED_FROM = R.SORTED_FROM, 1
    try:
        np.testing.assert_allclose(R.pair_sums(obs, valid, rows), direct, rtol=1e-12, atol=1e-12)
    finally:
        R.SORTED_FROM = old


def test_restatement_one_day_is_the_ensemble_score():
    """a one-day series draws the rank of `ensemble_scores` (Philox block (seed, 0, pixel)) and has no reference"""
    ens, obs, mask, _ = _small_case()
    r = R.series_ensemble_scores(ens[:1], obs[:1], [1.0], None, mask, seed=7)
    assert np.isnan(r["clim_crps"]).all() and r["skill_scores"][0, 0] == 0 and np.isnan(r["skill_scores"][0, 1:]).all()
    np.testing.assert_array_equal(r["daily"][0], r["scores"][0])
    import philox_ref
    u = philox_ref.uniform4(7, 0, np.arange(12, dtype=np.uint64))[..., 0].reshape(3, 4)
    with np.errstate(invalid="ignore"):
        lt, le = (ens[0] < obs[0]).sum(0), (ens[0] <= obs[0]).sum(0)
    np.testing.assert_array_equal(R.ranks(ens[:1], obs[:1], 7)[0], np.minimum(le, lt + np.floor(u * (le - lt + 1).astype(f32)).astype(int)))


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------

def test_symbols_and_abi_version():
    names = ("sbgm_series_scores", "sbgm_series_scores_workspace_bytes")
    lib = N.lib()
    for name in names:
        assert name in N.SIGNATURES and getattr(lib, name) is not None
    assert lib.sbgm_abi_version() == N.ABI_VERSION >= 16
    header = open(os.path.join(ROOT, "include", "sbgm_hip.h")).read()
    assert all(f"{name}(" in header for name in names)
    assert "#define SBGM_SERIES_MAX_GROUPS 16" in header and "#define SBGM_TEMPORAL_MAX_DAYS 4095" in header
    assert V.MAX_SERIES_GROUPS == 16 and V.MAX_SERIES_MEMBERS == 4095 and V.MAX_TEMPORAL_DAYS == 4095 and V.MAX_THRESHOLDS == 16
    assert V.SERIES_KEYS == R.KEYS and V.SERIES_MAP_KEYS == R.MAP_KEYS and V.SERIES_CLIM_MAP_KEYS == R.CLIM_MAP_KEYS
    assert V.SERIES_SKILL_KEYS == R.SKILL_KEYS and V.ENSEMBLE_KEYS == R.ENSEMBLE_KEYS and V.EXCEEDANCE_KEYS == R.EXCEEDANCE_KEYS


def test_workspace_query():
    q = N.lib().sbgm_series_scores_workspace_bytes
    big = 1 << 40
    HW, slots = 37 * 53, 8 * 4                                              # 8 workgroups of 4 waves
    fixed = 3 * HW * 8 + 100 * 5 * 8 + 4 * HW * 4                           # per-pixel sums, day sums, validity words of 100 days
    assert q(100, 16, 37, 53, 4, 0, 0, big) == fixed + 100 * slots * 5 * 8
    clim = 2 * 4 * HW * 8 + 5 * slots * 3 * 8                               # per-group per-pixel sums; skill partials of 5 rows
    assert q(100, 16, 37, 53, 4, 4, 1, big) == fixed + clim + 100 * slots * 5 * 8
    assert q(100, 16, 37, 53, 4, 4, 0, big) == fixed + 100 * slots * 5 * 8
    # chunks of days: a multiple of 32 within max_bytes, at least 32, never more than D
    assert q(100, 16, 37, 53, 4, 0, 0, 0) == fixed + 32 * slots * 5 * 8
    assert q(100, 16, 37, 53, 4, 0, 0, fixed + 70 * slots * 5 * 8) == fixed + 64 * slots * 5 * 8
    assert q(20, 16, 37, 53, 4, 0, 0, 0) == q(20, 16, 37, 53, 4, 0, 0, big)
    assert q(3650, 16, 589, 789, 4, 4, 1, V.DEFAULT_WORKSPACE_BYTES) <= max(V.DEFAULT_WORKSPACE_BYTES,
                                                                           q(3650, 16, 589, 789, 4, 4, 1, 0))
    for bad in ((0, 16, 8, 8, 0, 0, 1), (4096, 16, 8, 8, 0, 0, 1), (4, 1, 8, 8, 0, 0, 1), (4, 4096, 8, 8, 0, 0, 1),
                (4, 16, 1, 8, 0, 0, 1), (4, 16, 8, 2049, 0, 0, 1), (4, 16, 1024, 1025, 0, 0, 1), (4, 16, 8, 8, 17, 0, 1),
                (4, 16, 8, 8, -1, 0, 1), (4, 16, 8, 8, 0, 17, 1), (4, 16, 8, 8, 0, -1, 1)):
        assert q(*bad, big) == 0, bad


def test_entry_point_refuses_before_any_launch():
    lib = N.lib()
    call = lambda *a: lib.sbgm_series_scores(*a)                          # noqa: E731
    nulls = [None] * 10
    assert call(None, 64, 64, None, None, 0, 1, None, 0, 4, 3, 8, 8, None, 0, 0, 1, *nulls, 0, None) != 0
    assert b"null" in lib.sbgm_last_error()
    p = 4096                                                                # a non-null pointer that is never followed
    outs = [p] * 10
    for kw, word in ((dict(D=0), b"D=0"), (dict(D=4096), b"D=4096"), (dict(M=1), b"M=1"), (dict(M=4096), b"M=4096"),
                     (dict(H=1), b"field size"), (dict(day_stride=63), b"day_stride"), (dict(member_stride=0), b"member_stride"),
                     (dict(Nm=2), b"mask"), (dict(G=17), b"G=17"), (dict(G=2), b"G=2"), (dict(T=17), b"T=17"), (dict(T=1), b"T=1"),
                     (dict(ws_bytes=8), b"workspace")):
        a = dict(day_stride=64 * 3, member_stride=64, Nm=1, G=0, D=4, M=3, H=8, W=8, T=0, ws_bytes=1 << 30)
        a.update(kw)
        mask = p if "Nm" in kw else None
        rc = call(p, a["day_stride"], a["member_stride"], p, mask, 1, a["Nm"], None, a["G"], a["D"], a["M"], a["H"], a["W"], None, a["T"],
                  0, 1, *outs, a["ws_bytes"], None)
        assert rc != 0 and word in lib.sbgm_last_error(), (kw, lib.sbgm_last_error())
    assert call(p, 192, 64, p, None, 0, 1, None, 0, 4, 3, 8, 8, None, 0, 0, 1, *([p] * 7), None, None, p, 1 << 30, None) != 0
    assert b"clim_maps" in lib.sbgm_last_error()


def test_wrapper_checks_before_the_device():
    ens, obs = torch.zeros(5, 3, 8, 9), torch.zeros(5, 8, 9)
    bad = [dict(ens=torch.zeros(5, 1, 8, 9)), dict(ens=torch.zeros(5, 4096, 2, 2), obs=torch.zeros(5, 2, 2)),
           dict(ens=torch.zeros(4096, 2, 2, 2), obs=torch.zeros(4096, 2, 2)), dict(ens=torch.zeros(0, 3, 8, 9), obs=torch.zeros(0, 8, 9)),
           dict(ens=torch.zeros(3, 8, 9)), dict(obs=torch.zeros(8, 9)), dict(obs=torch.zeros(4, 8, 9)), dict(obs=torch.zeros(5, 9, 8)),
           dict(ens=torch.zeros(5, 3, 1, 9), obs=torch.zeros(5, 1, 9)), dict(ens=torch.zeros(5, 3, 8, 9, dtype=torch.int32)),
           dict(obs=torch.zeros(5, 8, 9, dtype=torch.int64)), dict(mask=torch.ones(2, 8, 9)), dict(mask=torch.ones(8, 8)),
           dict(mask=torch.ones(5, 8, 9, dtype=torch.int32)), dict(thresholds=[1.0] * 17), dict(thresholds=[float("nan")]),
           dict(thresholds=[float("inf")]), dict(thresholds=[1e39]), dict(groups=[0, 1, 0, 1]), dict(groups=[0, 1, 0, 1, 16]),
           dict(groups=[0, -1, 0, 1, 0]), dict(groups=[0, 1.5, 0, 1, 0]), dict(groups=[0, True, 0, 1, 0]),
           dict(groups=torch.zeros(5)), dict(groups=torch.zeros(5, 1, dtype=torch.int64)), dict(groups=torch.arange(5) + 12),
           dict(seed=1.5), dict(seed="1")]
    for kw in bad:
        args = dict(ens=ens, obs=obs)
        args.update(kw)
        with pytest.raises((ValueError, TypeError)):
            V.series_ensemble_scores(**args)
    with pytest.raises(NativeError):                                         # well-formed arguments reach the device check
        V.series_ensemble_scores(ens, obs)
    with pytest.raises(NativeError):
        V.series_ensemble_scores(ens.permute(1, 0, 2, 3).contiguous().permute(1, 0, 2, 3), obs, [0.5] * 16, groups=torch.arange(5) * 3,
                                 mask=torch.ones(5, 8, 9, dtype=torch.bool), seed=2**63, climatology=False, max_workspace_bytes=0)


# ---- evaluation.series_scores in the config ---------------------------------------------------------------------------------------

def test_series_section_parsing():
    sec = lambda s: E.series_scores_config(to_config({"evaluation": {"series_scores": s}}))  # noqa: E731
    assert sec({}) == ([], True, None, None)
    assert sec({"thresholds": [1, 2.5], "climatology": False, "groups": [0, 1, 1], "seed": 4}) == ([1.0, 2.5], False, [0, 1, 1], 4)
    assert sec({"groups": "seasons.npy", "thresholds": None, "seed": None}) == ([], True, "seasons.npy", None)
    for broken, key in (({"threshold": [1.0]}, "threshold"), ({"thresholds": 1.0}, "series_scores.thresholds"),
                        ({"thresholds": [float("nan")]}, "series_scores.thresholds"), ({"thresholds": ["1"]}, "series_scores.thresholds"),
                        ({"thresholds": [1.0] * 17}, "series_scores.thresholds"), ({"climatology": 1}, "series_scores.climatology"),
                        ({"climatology": "yes"}, "series_scores.climatology"), ({"groups": [0, 16]}, "series_scores.groups"),
                        ({"groups": [0, -1]}, "series_scores.groups"), ({"groups": [0.5]}, "series_scores.groups"),
                        ({"groups": [True]}, "series_scores.groups"), ({"groups": []}, "series_scores.groups"),
                        ({"groups": 3}, "series_scores.groups"), ({"groups": "seasons.txt"}, "series_scores.groups"),
                        ({"seed": 1.5}, "series_scores.seed"), ({"seed": True}, "series_scores.seed"), ({"seed": "0"}, "series_scores.seed")):
        with pytest.raises(ValueError, match=key):
            sec(broken)
    with pytest.raises(ValueError, match="series_scores"):
        sec([1.0])
    assert EM.STATISTICS["series_ensemble_stats"] == ("series_ensemble_statistics", E.series_scores_config, False)
    assert all(len(v) == 3 for v in EM.STATISTICS.values()) and EM.SERIES_STATISTICS == ("series_ensemble_stats",)


def test_unit_statistics_with_and_without_the_section():
    assert E.series_scores_config(load_config(CFG)) is None                   # the shipped defaults do not opt in
    assert "series_scores" not in yaml.safe_load(open(CFG))["evaluation"]
    # without the section: what each type ran before this statistic existed, spelled out
    base = ["pixel_stats", "spatial_stats"]
    expected = {
        "plain": ({}, {t: base for t in E.GEN_TYPES}),
        "methods": ({"eval_stat_methods": ["daily_stats", "spectral_stats"]}, {t: ["daily_stats", "spectral_stats"] for t in E.GEN_TYPES}),
        "spatial": ({"spatial_scores": {"thresholds": [1.0], "scales": [3]}},
                    {t: base + ["neighbourhood_stats"] + (["exceedance_stats"] if t == "repeated" else []) for t in E.GEN_TYPES}),
        "products": ({"ensemble_products": {"quantiles": [0.5]}}, {t: base + (["product_stats"] if t == "repeated" else []) for t in E.GEN_TYPES}),
        "objects": ({"object_scores": {"thresholds": [1.0]}}, {t: base + ["object_stats"] for t in E.GEN_TYPES}),
        "multivariate": ({"multivariate_scores": {"energy": True}},
                         {t: base + (["multivariate_stats"] if t == "repeated" else []) for t in E.GEN_TYPES}),
        "climate": ({"climate_indices": {"quantiles": [0.5]}},
                    {t: base + (["climate_stats"] if t in ("multiple", "series") else []) for t in E.GEN_TYPES}),
    }
    for name, (ev, want) in expected.items():
        for t in E.GEN_TYPES:
            assert EM.unit_statistics(to_config({"evaluation": ev}), t) == want[t], (name, t)
            with_s = EM.unit_statistics(to_config({"evaluation": dict(ev, series_scores={"thresholds": [1.0]})}), t)
            assert with_s == want[t] + (["series_ensemble_stats"] if t == "series" else []), (name, t)
    assert not set(EM.SERIES_METHODS) & set(EM.METHODS)                       # and it is no eval_stat_methods name
    with pytest.raises(ValueError, match="series_ensemble_stats"):
        EM.eval_stat_methods(to_config({"evaluation": {"eval_stat_methods": ["series_ensemble_stats"]}}))


def _write_series(tmp_path, monkeypatch, members, section):
    for k in ("DATA_DIR", "CKPT_DIR", "SAMPLE_DIR", "STATS_LOAD_DIR"):
        monkeypatch.setenv(k, str(tmp_path / k.lower()))
    monkeypatch.setenv("SLURM_CPUS_PER_TASK", "2")
    raw = yaml.safe_load(open(CFG))
    raw["evaluation"]["series_scores"] = section
    p = tmp_path / f"series_{members}.yaml"
    p.write_text(yaml.safe_dump(raw))
    cfg = load_config(str(p))
    from sbgm_danra_amd.utils import get_model_string
    d = os.path.join(cfg.paths.sample_dir, "generation", get_model_string(cfg), "generated_samples")
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(1)
    np.savez_compressed(os.path.join(d, "gen_samples_series_n_6.npz"), rng.random((6, members, 4, 5)).astype(f32))
    np.savez_compressed(os.path.join(d, "eval_samples_series_n_6.npz"), rng.random((6, 4, 5)).astype(f32))
    np.savez_compressed(os.path.join(d, "gen_samples_multi_n_2.npz"), np.zeros((2, 4, 5), f32))
    np.savez_compressed(os.path.join(d, "eval_samples_multi_n_2.npz"), np.zeros((2, 4, 5), f32))
    return cfg


def test_series_statistics_errors_on_the_host(tmp_path, monkeypatch):
    cfg = _write_series(tmp_path, monkeypatch, 1, {"thresholds": [0.5]})
    one = E.Evaluation(cfg, "series", None, device=torch.device("cpu"))
    with pytest.raises(ValueError, match="evaluation.series.members"):
        one.series_ensemble_statistics()
    with pytest.raises(ValueError, match="'series' samples"):
        E.Evaluation(cfg, "multiple", 2, device=torch.device("cpu")).series_ensemble_statistics()
    cfg = _write_series(tmp_path, monkeypatch, 3, {"thresholds": [0.5], "groups": [0, 1, 0, 1]})
    ev = E.Evaluation(cfg, "series", None, device=torch.device("cpu"))
    assert ev.metrics["members"] == 3 and tuple(ev.members.shape) == (3, 6, 4, 5)
    with pytest.raises(ValueError, match="groups holds 4 ids.*6 days"):
        ev.series_ensemble_statistics()
    np.save(tmp_path / "g.npy", np.arange(5))
    with pytest.raises(ValueError, match="groups holds 5 ids"):
        ev.series_ensemble_statistics(groups=str(tmp_path / "g.npy"))
    with pytest.raises(ValueError, match="integer id"):
        ev.series_ensemble_statistics(groups=np.zeros(6))
    with pytest.raises(NativeError):                                           # arguments fine; the fields are on the CPU
        ev.series_ensemble_statistics(groups=[0, 0, 1, 1, 2, 2], thresholds=[0.5])
    assert "series_ensemble" not in ev.metrics
    no_section = load_config(CFG)
    ev.cfg = no_section
    with pytest.raises(ValueError, match="series_scores"):
        ev.series_ensemble_statistics()
