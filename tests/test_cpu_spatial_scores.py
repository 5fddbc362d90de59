"""CPU suite for the neighbourhood and threshold-exceedance scores: the numpy restatement (tests/spatial_scores_ref.py) against
closed forms, the argument checks of the two device wrappers (they fire before anything touches the device), and how evaluate
mode reads `evaluation.spatial_scores` — with the section absent it runs exactly the statistics it ran before."""
import math
import os

import numpy as np
import pytest
import torch
import yaml

import spatial_scores_ref as R
from sbgm_danra_amd import verification as V
from sbgm_danra_amd._native import NativeError
from sbgm_danra_amd.config_loader import load_config, to_config
from sbgm_danra_amd.evaluate_sbgm import evaluation as E
from sbgm_danra_amd.evaluate_sbgm import evaluation_main as EM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "sbgm_danra_amd", "config", "default_config.yaml")


# ---- the restatement against closed forms ---------------------------------------------------------------------------------------

def test_identical_fields_score_one():
    rng = np.random.default_rng(0)
    f = rng.standard_normal((2, 11, 13)).astype(np.float32)
    r = R.neighbourhood_scores(f, f, [0.0, 0.5], [1, 3, 7])
    assert not r["num"].any() and (r["den"] > 0).all()
    assert (r["fss"] == 1.0).all() and (r["fss_field"] == 1.0).all() and (r["freq_bias"] == 1.0).all()
    np.testing.assert_array_equal(r["events_gen"], r["events_obs"])
    assert list(r["valid"]) == [11 * 13] * 2


def test_two_single_pixel_events_d_apart():
    """gen has one event at (10, 8), obs one at (10, 12): d = 4.  An n x n window sees each event from n^2 centres and both
    from n (n - d) centres when n > d, from none otherwise; so num = 2 n^2 - 2 n max(n - d, 0), den = 2 n^2 and
    fss = max(n - d, 0) / n: 0 for n <= d, 1/5 at n = 5, 3/7 at n = 7 (all windows stay inside the 21 x 21 field)."""
    gen, obs = np.zeros((1, 21, 21), np.float32), np.zeros((1, 21, 21), np.float32)
    gen[0, 10, 8] = obs[0, 10, 12] = 1.0
    r = R.neighbourhood_scores(gen, obs, [0.5], [1, 3, 5, 7])
    assert r["num"][0, 0].tolist() == [2, 18, 40, 56] and r["den"][0, 0].tolist() == [2, 18, 50, 98]
    assert r["fss"][0, :2].tolist() == [0.0, 0.0]
    assert r["fss"][0, 2] == pytest.approx(0.2, rel=1e-15) and r["fss"][0, 3] == pytest.approx(3.0 / 7.0, rel=1e-15)
    assert r["events_gen"].tolist() == [[1]] and r["events_obs"].tolist() == [[1]] and r["freq_bias"].tolist() == [1.0]
    assert r["fss_useful"][0] == pytest.approx(0.5 + 0.5 / 441.0, rel=1e-15)


def test_window_is_zero_padded_not_renormalised():
    """a corner event is seen by (r + 1)^2 centres only, and an invalid pixel is no event but still a window centre"""
    gen, obs = np.zeros((1, 6, 7), np.float32), np.zeros((1, 6, 7), np.float32)
    gen[0, 0, 0] = 1.0
    obs[0, 2, 3] = np.nan
    r = R.neighbourhood_scores(gen, obs, [0.5], [1, 3, 5])
    assert r["num"][0, 0].tolist() == [1, 4, 9] and r["den"][0, 0].tolist() == [1, 4, 9] and r["valid"].tolist() == [41]
    assert r["fss"][0].tolist() == [0.0, 0.0, 0.0] and r["freq_bias"][0] == math.inf


def test_empty_threshold_gives_nan():
    rng = np.random.default_rng(1)
    gen, obs = rng.random((2, 9, 8)).astype(np.float32), rng.random((1, 9, 8)).astype(np.float32)
    r = R.neighbourhood_scores(gen, obs, [2.0, -1.0], [1, 5])
    assert not r["den"][:, 0].any() and np.isnan(r["fss"][0]).all() and np.isnan(r["fss_field"][:, 0]).all()
    assert math.isnan(r["freq_bias"][0]) and r["fss_useful"][0] == 0.5
    assert r["events_gen"][:, 1].tolist() == [72, 72] and r["fss_useful"][1] == 1.0 and (r["fss"][1] == 1.0).all()


def test_window_past_both_sides_covers_the_field():
    rng = np.random.default_rng(2)
    gen, obs = rng.random((2, 5, 7)).astype(np.float32), rng.random((2, 5, 7)).astype(np.float32)
    r = R.neighbourhood_scores(gen, obs, [0.5], [11, 13, 15, 21])
    for k in ("num", "den"):
        assert (r[k][:, :, 1:] == r[k][:, :, 1:2]).all(), k                # n >= 2 max(H, W) - 1 = 13: every window is the field
        assert (r[k][:, :, 0] != r[k][:, :, 1]).any(), k
    eg, eo = r["events_gen"][:, 0], r["events_obs"][:, 0]
    np.testing.assert_array_equal(r["num"][:, 0, 1], 35 * (eg - eo) ** 2)
    np.testing.assert_array_equal(r["den"][:, 0, 1], 35 * (eg ** 2 + eo ** 2))


def test_brier_decomposition_is_exact_for_this_binning():
    rng = np.random.default_rng(3)
    ens = rng.standard_normal((7, 23, 19)).astype(np.float32)
    obs = rng.standard_normal((23, 19)).astype(np.float32)
    ens[2, 4, 5] = np.nan
    r = R.exceedance_scores(ens, obs, [-0.5, 0.0, 1.0], mask=rng.random((23, 19)) < 0.8)
    np.testing.assert_allclose(r["brier_reliability"] - r["brier_resolution"] + r["brier_uncertainty"], r["brier"], rtol=0, atol=1e-12)
    assert (r["table"][:, :, 0].sum(1) == r["count"]).all() and (r["table"][..., 1] <= r["table"][..., 0]).all()
    assert (abs(r["roc_area"] - 0.5) < 0.1).all()                                 # independent fields: no skill either way
    np.testing.assert_allclose(r["base_rate"], r["table"][..., 1].sum(1) / r["count"], rtol=1e-15)


def test_sharp_and_correct_ensemble():
    rng = np.random.default_rng(4)
    obs = rng.standard_normal((12, 10)).astype(np.float32)
    r = R.exceedance_scores(np.repeat(obs[None], 5, axis=0), obs, [0.0, 0.7])
    assert r["brier"].tolist() == [0.0, 0.0] and r["roc_area"].tolist() == [1.0, 1.0]
    assert r["brier_reliability"].tolist() == [0.0, 0.0]
    np.testing.assert_allclose(r["brier_resolution"], r["brier_uncertainty"], rtol=1e-15)
    assert not r["table"][:, 1:5].any()                                           # every pixel has k = 0 or k = M
    never = R.exceedance_scores(np.repeat(obs[None], 5, axis=0), obs, [9.0])
    assert math.isnan(never["roc_area"][0]) and never["brier"][0] == 0.0 and never["base_rate"][0] == 0.0


# ---- argument checks of the device wrappers: before any launch, before any look at the device ---------------------------------------

def test_neighbourhood_scores_argument_checks():
    x = torch.zeros(3, 8, 8)
    bad = [dict(scales=[1, 4]), dict(scales=[0]), dict(scales=[-3]), dict(scales=[]), dict(scales=[1] * 17), dict(scales=[3.5]),
           dict(thresholds=[0.1] * 17), dict(thresholds=[]), dict(thresholds=[float("nan")]), dict(thresholds=[float("inf")]),
           dict(thresholds=[1e39]),                                                # not finite in fp32
           dict(obs=torch.zeros(2, 8, 8)), dict(obs=torch.zeros(3, 8, 9)), dict(mask=torch.ones(2, 8, 8, dtype=torch.uint8)),
           dict(gen=torch.zeros(8, 8)), dict(gen=torch.zeros(1, 1025, 1024), obs=torch.zeros(1, 1025, 1024)),
           dict(gen=torch.zeros(1, 1, 64), obs=torch.zeros(1, 1, 64)), dict(gen=torch.zeros(1, 2, 2049), obs=torch.zeros(1, 2, 2049))]
    for kw in bad:
        args = dict(gen=x, obs=x, thresholds=[0.5], scales=[1, 3], mask=None)
        args.update(kw)
        with pytest.raises(ValueError):
            V.neighbourhood_scores(**args)
    with pytest.raises(NativeError):                                               # well-formed, but on the CPU: no fallback
        V.neighbourhood_scores(x, x[:1], [0.5], [1, 3])


def test_exceedance_scores_argument_checks():
    ens, obs = torch.zeros(4, 8, 8), torch.zeros(8, 8)
    bad = [dict(ens=ens[:1]), dict(ens=torch.zeros(4096, 2, 2), obs=torch.zeros(2, 2)), dict(thresholds=[0.0] * 17),
           dict(thresholds=[]), dict(thresholds=[float("nan")]), dict(obs=torch.zeros(4, 8, 8)), dict(obs=torch.zeros(8, 9)),
           dict(mask=torch.ones(4, 8, 8)), dict(ens=obs)]
    for kw in bad:
        args = dict(ens=ens, obs=obs, thresholds=[0.5], mask=None)
        args.update(kw)
        with pytest.raises(ValueError):
            V.exceedance_scores(**args)
    with pytest.raises(NativeError):
        V.exceedance_scores(ens, obs, [0.5])


# ---- evaluation.spatial_scores in the config ----------------------------------------------------------------------------------------

def test_spatial_scores_section_parsing():
    sec = {"thresholds": [1, 5.0, 10.0], "scales": [1, 3, 65]}
    c = to_config({"evaluation": {"spatial_scores": sec}})
    assert EM.spatial_scores_config(c) == ([1.0, 5.0, 10.0], [1, 3, 65])
    assert EM.unit_statistics(c, "multiple") == ["pixel_stats", "spatial_stats", "neighbourhood_stats"]
    assert EM.unit_statistics(c, "repeated") == ["pixel_stats", "spatial_stats", "neighbourhood_stats", "exceedance_stats"]
    for broken in ({"thresholds": [1.0]}, {"scales": [3]}, {"thresholds": [], "scales": [3]}, {"thresholds": [1.0], "scales": [2]},
                   {"thresholds": [1.0], "scales": [3.0]}, {"thresholds": [float("nan")], "scales": [3]},
                   {"thresholds": ["wet"], "scales": [3]}, {"thresholds": [1.0] * 17, "scales": [3]}, {}):
        with pytest.raises(ValueError, match="spatial_scores"):
            EM.spatial_scores_config(to_config({"evaluation": {"spatial_scores": broken}}))


def test_absent_section_leaves_the_statistics_unchanged():
    assert E.spatial_scores_config(load_config(CFG)) is None                      # the shipped defaults do not opt in
    assert "spatial_scores" not in yaml.safe_load(open(CFG))["evaluation"]
    for ev in ({}, {"eval_stat_methods": ["daily_stats", "ensemble_stats", "spectral_stats"]}):
        c = to_config({"evaluation": ev})
        assert EM.spatial_scores_config(c) is None
        for t in E.GEN_TYPES:
            assert EM.unit_statistics(c, t) == EM.eval_stat_methods(c)
    assert not set(EM.SPATIAL_METHODS) & set(EM.METHODS)                           # and they are no eval_stat_methods names
    with pytest.raises(ValueError, match="neighbourhood_stats"):
        EM.eval_stat_methods(to_config({"evaluation": {"eval_stat_methods": ["neighbourhood_stats"]}}))


@pytest.mark.parametrize("with_section", [False, True])
def test_evaluation_main_calls(tmp_path, monkeypatch, with_section):
    """the methods evaluation_main calls on each unit: the two new ones only with the section, exceedance only for `repeated`"""
    for k in ("DATA_DIR", "CKPT_DIR", "SAMPLE_DIR", "STATS_LOAD_DIR"):
        monkeypatch.setenv(k, str(tmp_path / k.lower()))
    monkeypatch.setenv("SLURM_CPUS_PER_TASK", "2")
    cfg = load_config(CFG)
    cfg.evaluation.eval_gen_type = ["multiple", "repeated"]
    cfg.evaluation.eval_stat_methods = ["pixel_stats", "daily_stats"]
    if with_section:
        cfg.evaluation.spatial_scores = to_config({"thresholds": [0.5], "scales": [1, 3]})
    calls = {}

    class Recorder:
        def __init__(self, cfg, generated_sample_type, n_samples, rank):
            self.label, self.metrics, self.n_samples = generated_sample_type, {}, 3
            calls[self.label] = []

        def __getattr__(self, name):
            return lambda *a, **k: calls[self.label].append(name)

    monkeypatch.setattr(EM, "Evaluation", Recorder)
    monkeypatch.setattr(EM, "sample_units", lambda d, t, n: [(None, {})])
    EM.evaluation_main(cfg)
    base = ["full_pixel_statistics", "daily_statistics"]
    extra = ["neighbourhood_statistics"] if with_section else []
    assert calls == {"multiple": base + extra + ["save"],
                     "repeated": base + extra + (["exceedance_statistics"] if with_section else []) + ["save"]}


def test_methods_need_thresholds_from_somewhere(tmp_path, monkeypatch):
    for k in ("DATA_DIR", "CKPT_DIR", "SAMPLE_DIR", "STATS_LOAD_DIR"):
        monkeypatch.setenv(k, str(tmp_path / k.lower()))
    monkeypatch.setenv("SLURM_CPUS_PER_TASK", "2")
    cfg = load_config(CFG)
    from sbgm_danra_amd.utils import get_model_string
    d = os.path.join(cfg.paths.sample_dir, "generation", get_model_string(cfg), "generated_samples")
    os.makedirs(d)
    for n in ("gen_samples_multi_n_2.npz", "eval_samples_multi_n_2.npz"):
        np.savez_compressed(os.path.join(d, n), np.zeros((2, 4, 5), np.float32))
    ev = E.Evaluation(cfg, "multiple", 2, device=torch.device("cpu"))
    with pytest.raises(ValueError, match="spatial_scores"):
        ev.neighbourhood_statistics()
    with pytest.raises(ValueError, match="repeated"):                              # as ensemble_statistics
        ev.exceedance_statistics([0.5])
    with pytest.raises(NativeError):                                               # arguments fine; the fields are on the CPU
        ev.neighbourhood_statistics([0.5], [1, 3])
