"""CPU suite for the object-based verification: the numpy / scipy restatement (tests/objects_ref.py) against cases computed by
hand, the argument checks of the two device wrappers (they fire before anything touches the device), and how evaluate mode
reads `evaluation.object_scores` — with the section absent it runs exactly the statistics it ran before."""
import math
import os

import numpy as np
import pytest
import torch
import yaml

import objects_ref as R
from sbgm_danra_amd import _native as N
from sbgm_danra_amd import verification as V
from sbgm_danra_amd._native import NativeError
from sbgm_danra_amd.config_loader import load_config, to_config
from sbgm_danra_amd.evaluate_sbgm import evaluation as E
from sbgm_danra_amd.evaluate_sbgm import evaluation_main as EM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "sbgm_danra_amd", "config", "default_config.yaml")
H, W = 21, 31
D = math.sqrt((H - 1) ** 2 + (W - 1) ** 2)


def _blob(r0, c0, values):
    """a zero field with the 2-D array `values` placed with its corner at (r0, c0)"""
    f = np.zeros((1, H, W), np.float32)
    v = np.asarray(values, np.float32)
    f[0, r0:r0 + v.shape[0], c0:c0 + v.shape[1]] = v
    return f


# ---- labels ----------------------------------------------------------------------------------------------------------------

def test_canonical_labels_and_connectivity():
    img = np.array([[1, 0, 0, 1],
                    [0, 1, 0, 1],
                    [0, 0, 0, 0],
                    [1, 1, 0, 1]], bool)
    want4 = np.array([[1, 0, 0, 4], [0, 6, 0, 4], [0, 0, 0, 0], [13, 13, 0, 16]], np.int32)
    want8 = np.array([[1, 0, 0, 4], [0, 1, 0, 4], [0, 0, 0, 0], [13, 13, 0, 16]], np.int32)
    np.testing.assert_array_equal(R.label(img, 4), want4)
    np.testing.assert_array_equal(R.label(img, 8), want8)
    f = np.where(img, 2.0, 0.0).astype(np.float32)[None]
    np.testing.assert_array_equal(R.object_labels(f, 2.0, connectivity=4)[0], want4)          # >= : the edge value is an object pixel
    assert not R.object_labels(f, 2.5).any()
    m = np.ones((1, 4, 4), np.uint8)
    m[0, 3, 1] = 0                                                                            # the mask cuts the bottom run
    f[0, 0, 3] = np.nan                                                                       # and a NaN the right column
    want = want8.copy()
    want[3, 1], want[0, 3], want[1, 3] = 0, 0, 8
    np.testing.assert_array_equal(R.object_labels(f, 1.0, mask=m)[0], want)


# ---- SAL by hand -----------------------------------------------------------------------------------------------------------

def test_identical_fields_score_zero():
    rng = np.random.default_rng(0)
    f = (rng.integers(0, 9, size=(3, H, W)) * 0.5).astype(np.float32)
    r = R.object_scores(f, f, [1.0, 2.5], relative=dict(factor=0.5, quantile=0.9, wet=0.5))
    for k in ("S", "A", "L1", "L2", "L"):
        assert (r[k] == 0.0).all(), k
    np.testing.assert_array_equal(r["n_objects"][0], r["n_objects"][1])
    assert (r["n_objects"] > 0).all()


def test_translated_object_moves_only_L1():
    vals = [[1, 2, 1], [2, 5, 2], [1, 2, 1]]
    obs, gen = _blob(4, 6, vals), _blob(4 + 5, 6 + 12, vals)
    r = R.object_scores(gen, obs, [0.5])
    assert r["n_objects"].tolist() == [[[1]], [[1]]] and r["area"].tolist() == [[[9]], [[9]]]
    np.testing.assert_array_equal(r["com"], [[[10.0, 19.0]], [[5.0, 7.0]]])
    assert r["L1"][0] == pytest.approx(13.0 / D, rel=1e-15)                 # |(5, 12)| = 13
    assert r["S"][0, 0] == 0.0 and r["A"][0] == 0.0 and r["L2"][0, 0] == 0.0
    assert r["L"][0, 0] == r["L1"][0]


def test_doubled_field_moves_only_A():
    obs = _blob(3, 3, [[1, 3, 1], [1, 1, 1]]) + _blob(12, 20, [[2, 2], [2, 6]])
    r = R.object_scores(2 * obs, obs, [0.5])
    assert r["A"][0] == pytest.approx(2.0 / 3.0, rel=1e-15)
    assert r["S"][0, 0] == 0.0 and r["L1"][0] == 0.0 and r["L2"][0, 0] == 0.0
    np.testing.assert_array_equal(r["mass"][0], 2 * r["mass"][1])


def test_flat_against_peaked_object_of_equal_mass():
    gen = _blob(8, 10, np.ones((2, 4)))                                      # flat: mass 8, peak 1 -> V = 8
    obs = _blob(8, 10, [[0, 1, 0], [1, 4, 1], [0, 1, 0]])                    # peaked: mass 8, peak 4 -> V = 2
    r = R.object_scores(gen, obs, [0.5], connectivity=4)
    np.testing.assert_array_equal(r["mass"], [[[8.0]], [[8.0]]])
    np.testing.assert_array_equal(r["V"], [[[8.0]], [[2.0]]])
    assert r["S"][0, 0] == pytest.approx((8.0 - 2.0) / (0.5 * 10.0), rel=1e-15) and r["A"][0] == 0.0
    assert r["area_hist"][0, 0].tolist() == [0, 0, 0, 1] + [0] * 17          # 8 pixels: floor(log2 8) = 3
    assert r["area_hist"][1, 0].tolist() == [0, 0, 1] + [0] * 18             # 5 pixels: bin 2


def test_objects_moved_apart_symmetrically_move_only_L2():
    one = [[3.0]]
    obs = _blob(10, 15 - 2, one) + _blob(10, 15 + 2, one)
    gen = _blob(10, 15 - 5, one) + _blob(10, 15 + 5, one)
    r = R.object_scores(gen, obs, [1.0])
    assert r["n_objects"].tolist() == [[[2]], [[2]]]
    np.testing.assert_array_equal(r["r"], [[[5.0]], [[2.0]]])
    assert r["L1"][0] == 0.0 and r["S"][0, 0] == 0.0 and r["A"][0] == 0.0
    assert r["L2"][0, 0] == pytest.approx(2.0 * 3.0 / D, rel=1e-15) and r["L2"][0, 0] > 0


def test_a_side_without_objects_gives_nan_structure_and_location():
    obs, gen = _blob(4, 6, [[1, 2], [2, 1]]), _blob(4, 6, [[3, 4], [4, 3]])
    r = R.object_scores(gen, obs, [2.5, 0.5])
    assert r["n_objects"].tolist() == [[[1, 1]], [[0, 1]]]
    assert np.isnan(r["S"][0, 0]) and np.isnan(r["L2"][0, 0]) and np.isnan(r["L"][0, 0]) and np.isnan(r["V"][1, 0, 0])
    assert np.isfinite(r["S"][0, 1]) and r["L2"][0, 1] == 0.0
    assert r["A"][0] == pytest.approx((3.5 - 1.5) / (0.5 * 5.0) , rel=1e-15) and r["L1"][0] == 0.0
    z = R.object_scores(gen, np.zeros_like(obs), [0.5])                       # a side that sums to zero: no amplitude, no centre
    assert np.isnan(z["A"][0]) and np.isnan(z["L1"][0]) and np.isnan(z["com"][1]).all() and z["domain_mean"][1, 0] == 0.0
    nan = R.object_scores(np.full_like(gen, np.nan), obs, [0.5])              # no valid pixel
    assert nan["valid"][0] == 0 and np.isnan(nan["A"][0]) and np.isnan(nan["domain_mean"]).all() and not nan["n_objects"].any()


def test_relative_threshold_against_numpy_quantile():
    rng = np.random.default_rng(3)
    v = (rng.gamma(0.4, 4.0, size=5000)).astype(np.float32)
    for q in (0.0, 0.25, 0.95, 0.999, 1.0):
        wetv = v[v >= np.float32(0.1)].astype(np.float64)
        want = (1.0 / 15.0) * np.quantile(wetv, q)
        got = R.relative_threshold(v, 1.0 / 15.0, q, 0.1)
        assert got.dtype == np.float32 and got == pytest.approx(want, rel=2e-7), q          # two roundings to fp32
    d = (rng.integers(0, 65, size=4001) * 0.25).astype(np.float32)                           # dyadic: the lerp is exact in both
    for q in (0.5, 0.95, 0.125):
        assert R.relative_threshold(d, 0.5, q, 1.0) == np.float32(0.5 * np.quantile(d[d >= 1.0].astype(np.float64), q))
    assert np.isnan(R.relative_threshold(d, 0.5, 0.95, 100.0))                                # nothing is wet
    f = np.zeros((1, H, W), np.float32)
    f[0, 5, 5:9] = [1, 2, 3, 4]
    r = R.object_scores(f, f * 0, [], relative=dict(factor=0.5, quantile=0.5, wet=0.5))       # median of 1..4 = 2.5 -> 1.25
    assert r["threshold"][0, 0, 0] == np.float32(1.25) and np.isnan(r["threshold"][1, 0, 0])
    assert r["n_objects"].tolist() == [[[1]], [[0]]] and r["area"][0, 0, 0] == 3


# ---- argument checks of the wrappers ---------------------------------------------------------------------------------------

def test_object_wrappers_check_before_the_device():
    f = torch.zeros(3, 8, 9)
    bad_scores = [dict(thresholds=[]), dict(thresholds=[0.0] * 17), dict(thresholds=[float("nan")]), dict(thresholds=[float("inf")]),
                  dict(connectivity=6), dict(connectivity=True), dict(obs=torch.zeros(2, 8, 9)), dict(obs=torch.zeros(3, 9, 8)),
                  dict(mask=torch.ones(2, 8, 9)), dict(gen=torch.zeros(8, 9)), dict(gen=torch.zeros(1, 1, 9), obs=torch.zeros(1, 1, 9)),
                  dict(gen=torch.zeros(1, 2049, 2), obs=torch.zeros(1, 2049, 2)),
                  dict(gen=torch.zeros(1, 1025, 1024), obs=torch.zeros(1, 1025, 1024)),
                  dict(relative={"factor": 1.0, "quantile": 0.95}), dict(relative={"factor": 1.0, "quantile": 1.5, "wet": 0.1}),
                  dict(relative={"factor": float("nan"), "quantile": 0.5, "wet": 0.1}), dict(relative=[1.0, 0.95, 0.1])]
    for kw in bad_scores:
        args = dict(gen=f, obs=f, thresholds=[0.5])
        args.update(kw)
        with pytest.raises(ValueError):
            V.object_scores(**args)
    for kw in (dict(threshold=float("nan")), dict(connectivity=5), dict(mask=torch.ones(2, 8, 9)), dict(fields=torch.zeros(8, 9)),
               dict(fields=torch.zeros(1, 2, 2049))):
        args = dict(fields=f, threshold=0.5)
        args.update(kw)
        with pytest.raises(ValueError):
            V.object_labels(**args)
    with pytest.raises(NativeError):                                         # well-formed arguments reach the device check
        V.object_scores(f, f, [0.5], relative={"factor": 1 / 15, "quantile": 0.95, "wet": 0.1})
    with pytest.raises(NativeError):
        V.object_labels(f, 0.5, connectivity=4)
    for name in ("sbgm_object_labels", "sbgm_object_scores", "sbgm_object_scores_workspace_bytes"):
        assert name in N.SIGNATURES


# ---- evaluation.object_scores in the config ---------------------------------------------------------------------------------

def test_object_scores_section_parsing():
    rel = {"factor": 0.0667, "quantile": 0.95, "wet": 0.1}
    c = to_config({"evaluation": {"object_scores": {"thresholds": [1, 5.0], "relative": rel, "connectivity": 4}}})
    assert E.object_scores_config(c) == ([1.0, 5.0], rel, 4)
    assert EM.unit_statistics(c, "multiple") == ["pixel_stats", "spatial_stats", "object_stats"]
    assert EM.unit_statistics(c, "repeated") == ["pixel_stats", "spatial_stats", "object_stats"]
    assert E.object_scores_config(to_config({"evaluation": {"object_scores": {"thresholds": [2]}}})) == ([2.0], None, 8)
    assert E.object_scores_config(to_config({"evaluation": {"object_scores": {"relative": rel}}})) == ([], rel, 8)
    for broken in ({}, {"thresholds": []}, {"thresholds": 1.0}, {"thresholds": [float("nan")]}, {"thresholds": ["wet"]},
                   {"thresholds": [True]}, {"thresholds": [1.0] * 17}, {"thresholds": [1.0], "connectivity": 6},
                   {"thresholds": [1.0], "connectivity": "8"}, {"relative": {"factor": 1.0, "quantile": 0.95}},
                   {"relative": {"factor": 1.0, "quantile": 1.2, "wet": 0.1}}, {"relative": {"factor": "x", "quantile": 0.9, "wet": 0.1}},
                   {"relative": {"factor": 1.0, "quantile": 0.9, "wet": 0.1, "extra": 1}}, {"thresholds": [1.0], "relative": 0.95}):
        with pytest.raises(ValueError, match="object_scores"):
            E.object_scores_config(to_config({"evaluation": {"object_scores": broken}}))


def test_absent_object_section_leaves_the_statistics_unchanged():
    assert E.object_scores_config(load_config(CFG)) is None                  # the shipped defaults do not opt in
    assert "object_scores" not in yaml.safe_load(open(CFG))["evaluation"]
    for ev in ({}, {"eval_stat_methods": ["daily_stats", "spectral_stats"]}, {"spatial_scores": {"thresholds": [1.0], "scales": [3]}}):
        c = to_config({"evaluation": ev})
        assert E.object_scores_config(c) is None
        for t in E.GEN_TYPES:
            assert "object_stats" not in EM.unit_statistics(c, t)
    assert not set(EM.OBJECT_METHODS) & set(EM.METHODS)                       # and it is no eval_stat_methods name
    with pytest.raises(ValueError, match="object_stats"):
        EM.eval_stat_methods(to_config({"evaluation": {"eval_stat_methods": ["object_stats"]}}))
    assert hasattr(E.Evaluation, "object_statistics")
