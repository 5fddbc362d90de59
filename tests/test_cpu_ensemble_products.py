"""CPU suite for the ensemble products: the numpy restatement of the contract (tests/ensemble_products_ref.py) against
numpy's own quantile, mean and standard deviation in float64, how generate and evaluate mode read
`evaluation.ensemble_products`, and the argument checks of the device wrapper (they fire before anything touches the device)."""
import functools
import os

import numpy as np
import pytest
import torch
import yaml

import ensemble_products_ref as R
from sbgm_danra_amd import verification as V
from sbgm_danra_amd._native import NativeError
from sbgm_danra_amd.config_loader import load_config, to_config
from sbgm_danra_amd.evaluate_sbgm import evaluation as E
from sbgm_danra_amd.evaluate_sbgm import evaluation_main as EM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "sbgm_danra_amd", "config", "default_config.yaml")
MEMBERS = [2, 3, 5, 16, 17, 64, 65, 257, 1000]
KINDS = ["grid", "normal", "rain"]
QUANTILES = [0, 0.05, 0.25, 1 / 3, 0.5, 0.9, 0.99, 1]
SHAPE = (37, 53)


def make_ens(rng, kind, M, shape):
    """grid: multiples of 0.25 in [-2, 3] (heavy ties); normal; rain: max(3 z - 2, 0), more than half exact zeros"""
    if kind == "grid":
        return (rng.integers(-8, 13, size=(M, *shape)) * 0.25).astype(np.float32)
    z = rng.standard_normal((M, *shape)).astype(np.float32)
    return z if kind == "normal" else np.maximum(np.float32(3.0) * z - np.float32(2.0), np.float32(0.0))


@functools.lru_cache(maxsize=None)
def _case(kind, M):
    ens = make_ens(np.random.default_rng([KINDS.index(kind), M]), kind, M, SHAPE)
    return ens, R.ensemble_products(ens, QUANTILES, [0.5])


def _ulp32(x):
    """one fp32 unit in the last place at magnitude |x| (that of the smallest normal below it)"""
    return np.spacing(np.maximum(np.abs(x), np.finfo(np.float32).tiny).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("M", MEMBERS)
@pytest.mark.parametrize("kind", KINDS)
def test_restatement_against_numpy_quantile(kind, M):
    """inside [x_(lo), x_(hi)], and within one fp32 ulp of max(|x_(lo)|, |x_(hi)|) of np.quantile in float64 rounded to fp32:
    numpy lerps from the far end for g >= 0.5, both forms are fp64-accurate before the one rounding"""
    ens, r = _case(kind, M)
    srt = np.sort(ens, axis=0)
    want = np.quantile(ens.astype(np.float64), QUANTILES, axis=0).astype(np.float32)
    worst = 0.0
    for i, q in enumerate(QUANTILES):
        lo, hi, _ = R.rank_weights(q, M)
        a, b, got = srt[lo], srt[hi], r["quantiles"][i]
        assert ((a <= got) & (got <= b)).all(), (kind, M, q)
        dev = np.abs(got.astype(np.float64) - want[i].astype(np.float64)) / _ulp32(np.maximum(np.abs(a), np.abs(b)))
        worst = max(worst, float(dev.max()))
    print(f"quantile {kind} M={M}: largest deviation from np.quantile {worst:.3f} ulp")
    assert worst <= 1.0
    np.testing.assert_array_equal(r["quantiles"][0], r["min"])
    np.testing.assert_array_equal(r["quantiles"][-1], r["max"])
    np.testing.assert_array_equal(r["min"], ens.min(axis=0))
    np.testing.assert_array_equal(r["max"], ens.max(axis=0))


@pytest.mark.parametrize("M", MEMBERS)
@pytest.mark.parametrize("kind", KINDS)
def test_restatement_against_numpy_moments(kind, M):
    """mean and std (ddof 1) against numpy's float64 results (pairwise sums, the rounded mean), to one fp32 ulp"""
    ens, r = _case(kind, M)
    e64 = ens.astype(np.float64)
    for key, want in (("mean", e64.mean(axis=0)), ("std", e64.std(axis=0, ddof=1))):
        dev = np.abs(r[key].astype(np.float64) - want) / _ulp32(want)
        print(f"{key} {kind} M={M}: largest deviation {float(dev.max()):.3f} ulp")
        assert dev.max() <= 1.0, (key, kind, M)


def test_restatement_validity_and_exceedance():
    rng = np.random.default_rng(5)
    ens = make_ens(rng, "grid", 7, (6, 9))
    ens[3, 2, 4] = np.nan
    mask = np.ones((6, 9), np.uint8)
    mask[0, 0] = 0
    r = R.ensemble_products(ens, [0.5], [0.5, -5.0, 10.0], mask)
    assert r["count"] == 6 * 9 - 2
    for k in ("mean", "std", "min", "max"):
        assert np.isnan(r[k][2, 4]) and np.isnan(r[k][0, 0]) and np.isnan(r[k]).sum() == 2, k
    assert np.isnan(r["quantiles"][:, 2, 4]).all() and np.isnan(r["exceed_prob"][:, 0, 0]).all()
    ok = ~np.isnan(r["mean"])
    np.testing.assert_array_equal(r["exceed_prob"][0][ok], ((ens >= 0.5).sum(0) / np.float64(7)).astype(np.float32)[ok])
    assert (r["exceed_prob"][1][ok] == 1.0).all() and (r["exceed_prob"][2][ok] == 0.0).all()
    np.testing.assert_array_equal(r["quantiles"][0][ok], np.median(ens, axis=0)[ok])       # M odd: the middle member, exact


# ---- evaluation.ensemble_products in the config --------------------------------------------------------------------------------

def test_products_section_parsing():
    assert E.ensemble_products_config(load_config(CFG)) is None                   # the shipped defaults do not opt in
    assert "ensemble_products" not in yaml.safe_load(open(CFG))["evaluation"]
    assert E.ensemble_products_config(to_config({"evaluation": {}})) is None
    sec = {"quantiles": [0, 0.5, 1], "thresholds": [1, 5.0]}
    assert E.ensemble_products_config(to_config({"evaluation": {"ensemble_products": sec}})) == ([0.0, 0.5, 1.0], [1.0, 5.0])
    assert E.ensemble_products_config(to_config({"evaluation": {"ensemble_products": {"quantiles": [0.9]}}})) == ([0.9], [])
    assert E.ensemble_products_config(to_config({"evaluation": {"ensemble_products": {"quantiles": [], "thresholds": [2]}}})) == ([], [2.0])
    for broken in ({"quantiles": [], "thresholds": []}, {}, {"quantiles": [1.5]}, {"quantiles": [-0.1]}, {"quantiles": [float("nan")]},
                   {"quantiles": ["median"]}, {"quantiles": [0.5] * 17}, {"thresholds": [1.0] * 17},
                   {"quantiles": [0.5], "thresholds": [float("inf")]}, {"thresholds": [float("nan")]}, {"quantiles": 0.5}):
        with pytest.raises(ValueError, match="ensemble_products"):
            E.ensemble_products_config(to_config({"evaluation": {"ensemble_products": broken}}))


def test_products_run_only_with_the_section_and_only_for_repeated():
    sec = {"quantiles": [0.5], "thresholds": []}
    c = to_config({"evaluation": {"ensemble_products": sec}})
    assert EM.unit_statistics(c, "multiple") == EM.unit_statistics(c, "single") == ["pixel_stats", "spatial_stats"]
    assert EM.unit_statistics(c, "repeated") == ["pixel_stats", "spatial_stats", "product_stats"]
    both = to_config({"evaluation": {"ensemble_products": sec, "spatial_scores": {"thresholds": [1.0], "scales": [3]}}})
    assert EM.unit_statistics(both, "repeated") == ["pixel_stats", "spatial_stats", "neighbourhood_stats", "exceedance_stats",
                                                    "product_stats"]
    none = to_config({"evaluation": {}})
    for t in E.GEN_TYPES:
        assert EM.unit_statistics(none, t) == EM.eval_stat_methods(none)
    assert not set(EM.PRODUCT_METHODS) & (set(EM.METHODS) | set(EM.SPATIAL_METHODS))
    with pytest.raises(ValueError, match="product_stats"):
        EM.eval_stat_methods(to_config({"evaluation": {"eval_stat_methods": ["product_stats"]}}))


def test_product_statistics_needs_an_ensemble_and_levels(tmp_path, monkeypatch):
    for k in ("DATA_DIR", "CKPT_DIR", "SAMPLE_DIR", "STATS_LOAD_DIR"):
        monkeypatch.setenv(k, str(tmp_path / k.lower()))
    monkeypatch.setenv("SLURM_CPUS_PER_TASK", "2")
    cfg = load_config(CFG)
    from sbgm_danra_amd.utils import get_model_string
    d = os.path.join(cfg.paths.sample_dir, "generation", get_model_string(cfg), "generated_samples")
    os.makedirs(d)
    for n, k in (("gen_samples_multi_n_2.npz", 2), ("eval_samples_multi_n_2.npz", 2), ("gen_samples_repeated_n_3.npz", 3),
                 ("eval_samples_repeated_n_3.npz", 1)):
        np.savez_compressed(os.path.join(d, n), np.zeros((k, 4, 5), np.float32))
    np.savez_compressed(os.path.join(d, "ens_products_repeated_n_3.npz"), mean=np.zeros((4, 5), np.float32))
    assert [sorted(f) for _, f in E.sample_units(d, "repeated", 3)] == [["eval_samples", "gen_samples"]]      # the products file is no sample file
    with pytest.raises(ValueError, match="repeated"):
        E.Evaluation(cfg, "multiple", 2, device=torch.device("cpu")).product_statistics([0.5], [])
    ev = E.Evaluation(cfg, "repeated", 3, device=torch.device("cpu"))
    with pytest.raises(ValueError, match="ensemble_products"):
        ev.product_statistics()
    with pytest.raises(NativeError):                                               # arguments fine; the fields are on the CPU
        ev.product_statistics([0.5], [1.0])


# ---- the wrapper's argument checks ----------------------------------------------------------------------------------------------

def test_ensemble_products_argument_checks():
    ens = torch.zeros(4, 8, 8)
    bad = [dict(ens=ens[:1]), dict(ens=torch.zeros(4096, 2, 2)), dict(ens=ens[0]), dict(quantiles=[1.01]), dict(quantiles=[-1e-9]),
           dict(quantiles=[float("nan")]), dict(quantiles=[float("inf")]), dict(quantiles=[0.5] * 17), dict(thresholds=[0.0] * 17),
           dict(thresholds=[float("nan")]), dict(thresholds=[float("-inf")]), dict(thresholds=[1e39]),      # not finite in fp32
           dict(mask=torch.ones(4, 8, 8)), dict(mask=torch.ones(8, 9))]
    for kw in bad:
        args = dict(ens=ens, quantiles=[0.5], thresholds=[0.5], mask=None)
        args.update(kw)
        with pytest.raises(ValueError):
            V.ensemble_products(**args)
    assert V.MAX_PRODUCT_QUANTILES == 16 and V.MAX_PRODUCT_MEMBERS == 4095
    with pytest.raises(NativeError):                                               # well-formed, but on the CPU: no fallback
        V.ensemble_products(ens, [0.5], [0.5])
    with pytest.raises(NativeError):
        V.ensemble_products(ens)
