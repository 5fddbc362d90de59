"""Neighbourhood scores (K45) and threshold-exceedance scores (K46) of csrc/verify_spatial.hip against the numpy restatement in
tests/spatial_scores_ref.py: the integer outputs exactly, the fp64 scores to the rounding of their one sum and division, their
statistical behaviour on exchangeable / biased ensembles and displaced fields, and `--mode evaluate` end to end with and
without the `evaluation.spatial_scores` section."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spatial_scores_ref as R  # noqa: E402
from sbgm_danra_amd import _native as N  # noqa: E402
from sbgm_danra_amd import verification as V  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda")
# data are multiples of 0.25 in [-2, 3]: 0.5 equals data values (the >= edge), 0.6 falls between two, 10 is above the maximum
# (no event: den = 0, fss = NaN) and -5 below the minimum (every valid pixel an event)
THRESHOLDS = [0.5, 0.6, 10.0, -5.0]
ROWS = [(5, 1, 1, "u8"), (3, 3, 3, "f32"), (4, 4, 0, None), (1, 1, 1, "bool")]
INT_KEYS = ("num", "den", "events_gen", "events_obs", "valid")
F64_KEYS = ("fss", "fss_field", "freq_bias", "fss_useful")


def _shapes():
    """(H, W, widths): odd sides with W % 4 != 0; aligned sides; windows larger than both sides; one strip plus a ragged one"""
    return [(37, 53, (1, 3, 9, 21)), (32, 48, (1, 3, 9, 21)), (5, 7, (1, 3, 15)), (9, V.neighbourhood_strip_columns() + 37, (1, 5, 41))]


def _grid(rng, n, shape, nan_frac=0.01):
    a = (rng.integers(-8, 13, size=(n, *shape)) * 0.25).astype(np.float32)
    a[rng.random(a.shape) < nan_frac] = np.nan
    return a


def _mask_tensor(mask, mdtype):
    if mask is None:
        return None
    t = torch.from_numpy(mask).to(DEV)
    return t.to(torch.uint8) if mdtype == "u8" else (t.float() if mdtype == "f32" else t)


@functools.lru_cache(maxsize=None)
def _neighbourhood_case(shape_idx, n, no, nm):
    """inputs and their restatement, computed once per case and shared by the tests below"""
    H, W, scales = _shapes()[shape_idx]
    rng = np.random.default_rng([shape_idx, n, no, nm])
    gen, obs = _grid(rng, n, (H, W)), _grid(rng, no, (H, W))
    mask = (rng.random((nm, H, W)) < 0.7) if nm else None
    return gen, obs, mask, scales, R.neighbourhood_scores(gen, obs, THRESHOLDS, scales, mask)


def _check_neighbourhood(got, want):
    for k in INT_KEYS:
        assert got[k].dtype == torch.int64
        assert torch.equal(got[k].cpu(), torch.from_numpy(want[k])), k
    for k in F64_KEYS:                       # rel 1e-12: an fp64 sum over the N <= 8192 fields, then one division
        assert got[k].dtype == torch.float64
        np.testing.assert_allclose(got[k].cpu().numpy(), want[k], rtol=1e-12, atol=0, equal_nan=True, err_msg=k)


@pytest.mark.parametrize("shape_idx", range(4))
@pytest.mark.parametrize("n,no,nm,mdtype", ROWS)
def test_neighbourhood_scores_match_restatement(shape_idx, n, no, nm, mdtype):
    gen, obs, mask, scales, want = _neighbourhood_case(shape_idx, n, no, nm)
    got = V.neighbourhood_scores(torch.from_numpy(gen).to(DEV), torch.from_numpy(obs).to(DEV), THRESHOLDS, scales,
                                 mask=_mask_tensor(mask, mdtype))
    assert tuple(got["num"].shape) == (n, 4, len(scales)) and tuple(got["fss"].shape) == (4, len(scales))
    assert tuple(got["events_gen"].shape) == (n, 4) and tuple(got["valid"].shape) == (n,) and tuple(got["freq_bias"].shape) == (4,)
    _check_neighbourhood(got, want)
    assert not want["den"][:, 2].any() and np.isnan(want["fss"][2]).all()                  # the cases hold what they are for
    np.testing.assert_array_equal(want["events_gen"][:, 3], want["valid"])
    assert (want["events_gen"][:, 0] >= want["events_gen"][:, 1]).all()                    # 0.5 catches the values equal to it
    assert shape_idx == 2 or (want["events_gen"][:, 0] > want["events_gen"][:, 1]).all()   # (5 x 7 may hold none)


@pytest.mark.parametrize("shape_idx", [0, 3])
def test_neighbourhood_chunking_and_repeat_are_bit_equal(shape_idx):
    n = 5
    gen, obs, mask, scales, want = _neighbourhood_case(shape_idx, n, 1, 1)
    H, W = gen.shape[1:]
    g, o, m = torch.from_numpy(gen).to(DEV), torch.from_numpy(obs).to(DEV), _mask_tensor(mask, "u8")
    T, S = len(THRESHOLDS), len(scales)
    size = lambda cap: N.lib().sbgm_neighbourhood_scores_workspace_bytes(n, H, W, T, S, cap)
    pair = size(0)                                                   # the floor: one field x one threshold
    assert 0 < pair and size(V.DEFAULT_WORKSPACE_BYTES) == n * T * pair
    assert size(3 * pair + 1) == 3 * pair and size(2 * T * pair + pair) == 2 * T * pair
    base = V.neighbourhood_scores(g, o, THRESHOLDS, scales, mask=m)
    _check_neighbourhood(base, want)
    for cap in (V.DEFAULT_WORKSPACE_BYTES, 0, 3 * pair, 2 * T * pair):   # again; thresholds one by one; 3 + 1; two fields at a time
        again = V.neighbourhood_scores(g, o, THRESHOLDS, scales, mask=m, max_workspace_bytes=cap)
        for k in INT_KEYS:
            assert torch.equal(again[k], base[k]), (cap, k)
        for k in F64_KEYS:
            assert torch.equal(again[k].view(torch.int64), base[k].view(torch.int64)), (cap, k)


def _window_sum_sat(img, n):
    """the same window sum from a summed-area table — only for the full-domain case, where the direct loop is too slow"""
    r = (n - 1) // 2
    H, W = img.shape[-2:]
    sat = np.zeros(img.shape[:-2] + (H + 1, W + 1), dtype=np.int64)
    sat[..., 1:, 1:] = img.cumsum(-2).cumsum(-1)
    i0, i1 = np.clip(np.arange(H) - r, 0, H), np.clip(np.arange(H) + r + 1, 0, H)
    j0, j1 = np.clip(np.arange(W) - r, 0, W), np.clip(np.arange(W) + r + 1, 0, W)
    return (sat[..., i1[:, None], j1[None, :]] - sat[..., i0[:, None], j1[None, :]] - sat[..., i1[:, None], j0[None, :]] +
            sat[..., i0[:, None], j0[None, :]])


def test_neighbourhood_scores_full_domain():
    gen, obs, mask, scales, want = _neighbourhood_case(0, 3, 3, 3)
    sat = R.neighbourhood_scores(gen, obs, THRESHOLDS, scales, mask, window_sum=_window_sum_sat)
    for k in INT_KEYS:                                              # the table form first proves itself on the direct loop
        np.testing.assert_array_equal(sat[k], want[k], err_msg=k)
    rng = np.random.default_rng(589)
    gen, obs = _grid(rng, 2, (589, 789)), _grid(rng, 1, (589, 789))
    mask = rng.random((1, 589, 789)) < 0.7
    want = R.neighbourhood_scores(gen, obs, [0.5], [1, 65], mask, window_sum=_window_sum_sat)
    got = V.neighbourhood_scores(torch.from_numpy(gen).to(DEV), torch.from_numpy(obs).to(DEV), [0.5], [1, 65],
                                 mask=torch.from_numpy(mask).to(DEV))
    _check_neighbourhood(got, want)


EXC_THRESHOLDS = [0.5, 0.6, -0.25, 10.0, -5.0]
# 1500 members: the tables of 2 thresholds fill the LDS budget of a workgroup, so the 5 thresholds spread over the grid (2, 2, 1)
EXC_CASES = [(2, (37, 53), "u8"), (5, (37, 53), "f32"), (64, (37, 53), None), (257, (37, 53), "bool"),
             (2, (32, 48), "bool"), (5, (32, 48), None), (64, (32, 48), "u8"), (257, (32, 48), "f32"), (1500, (32, 48), "u8")]


@pytest.mark.parametrize("M,shape,mdtype", EXC_CASES)
def test_exceedance_scores_match_restatement(M, shape, mdtype):
    """The table and the count are exact.  The kernel derives the fp64 scores from the table, the restatement from direct sums
    over the pixels; both are fp64, bound rel 1e-10.  Largest relative deviation seen on the MI355X over these cases: 2.9e-15
    (brier_resolution at M = 1500; 6.7e-16 for M <= 257), more than 10^4 below the bound, so the bound stays."""
    rng = np.random.default_rng([M, shape[0]])
    signal = (rng.integers(-4, 5, size=shape) * 0.25).astype(np.float32)      # shared by truth and members; still multiples of 0.25
    ens = _grid(rng, M, shape, nan_frac=0.0) + signal
    obs = _grid(rng, 1, shape, nan_frac=0.01)[0] + signal
    bad = rng.random(shape) < 0.01                                           # a NaN in ONE member invalidates the pixel
    ens[rng.integers(0, M, size=shape)[bad], np.nonzero(bad)[0], np.nonzero(bad)[1]] = np.nan
    mask = (rng.random(shape) < 0.8) if mdtype is not None else None
    want = R.exceedance_scores(ens, obs, EXC_THRESHOLDS, mask)
    e, o = torch.from_numpy(ens).to(DEV), torch.from_numpy(obs).to(DEV)
    m = _mask_tensor(mask, mdtype)
    got = V.exceedance_scores(e, o, EXC_THRESHOLDS, mask=m)
    assert got["table"].dtype == torch.int64 and tuple(got["table"].shape) == (5, M + 1, 2)
    assert torch.equal(got["table"].cpu(), torch.from_numpy(want["table"])) and int(got["count"]) == want["count"]
    nan_pixels = np.isnan(ens).any(0) & ~np.isnan(obs) & (mask if mask is not None else True)
    assert nan_pixels.any() and want["count"] < (mask.sum() if mask is not None else obs.size)
    worst = 0.0
    for k in V.EXCEEDANCE_KEYS:
        a, b = got[k].cpu().numpy(), want[k]
        assert got[k].dtype == torch.float64 and a.shape == (5,)
        with np.errstate(invalid="ignore", divide="ignore"):
            dev = np.nanmax(np.where(b != 0, np.abs(a - b) / np.abs(b), np.abs(a - b)))
        worst = max(worst, float(dev))
        print(f"exceedance M={M} {shape} {k}: largest relative deviation {dev:.3e}")
        np.testing.assert_allclose(a, b, rtol=1e-10, atol=0, equal_nan=True, err_msg=k)
    assert np.isnan(want["roc_area"][3:]).all() and not np.isnan(want["roc_area"][:3]).any()
    np.testing.assert_allclose((got["brier_reliability"] - got["brier_resolution"] + got["brier_uncertainty"]).cpu().numpy(),
                               got["brier"].cpu().numpy(), rtol=0, atol=1e-12)
    again = V.exceedance_scores(e, o, EXC_THRESHOLDS, mask=m)               # two calls are bit-equal
    for k in ("table", "count") + V.EXCEEDANCE_KEYS:
        x, y = again[k], got[k]
        assert torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x, y.view(torch.int64) if y.dtype == torch.float64 else y), k


def test_exceedance_member_limit():
    with pytest.raises(ValueError):
        V.exceedance_scores(torch.zeros(4096, 4, 4, device=DEV), torch.zeros(4, 4, device=DEV), [0.5])
    r = V.exceedance_scores(torch.zeros(4095, 4, 4, device=DEV), torch.ones(4, 4, device=DEV), [0.5])     # one threshold per workgroup
    assert int(r["count"]) == 16 and r["table"][0, 0].tolist() == [16, 16] and int(r["table"].sum()) == 32
    assert r["brier"].item() == 1.0 and torch.isnan(r["roc_area"]).all()


# ---- statistical sanity -----------------------------------------------------------------------------------------------------------

def _exchangeable(shift=0.0):
    """truth and 64 members drawn alike around a shared signal: obs = s + e_0, member_i = s + e_i (+ shift), 64 x 64, seeded"""
    rng = np.random.default_rng(2008)
    s = rng.standard_normal((64, 64))
    obs = (s + 0.5 * rng.standard_normal((64, 64))).astype(np.float32)
    ens = (s + 0.5 * rng.standard_normal((64, 64, 64)) + shift).astype(np.float32)
    return ens, obs


def test_exchangeable_ensemble_is_reliable_and_a_shifted_one_is_not():
    """on the restatement, for this seed: reliability / uncertainty is 0.0104 and 0.0131 at the two thresholds when
    exchangeable (bound 0.05), and the +1 sigma shift multiplies the reliability term by 65 and 102 (bound 5)"""
    thr = [0.0, 1.0]
    ens, obs = _exchangeable()
    r = V.exceedance_scores(torch.from_numpy(ens).to(DEV), torch.from_numpy(obs).to(DEV), thr)
    rel, res, unc = (r[k].cpu().numpy() for k in ("brier_reliability", "brier_resolution", "brier_uncertainty"))
    assert (rel < 0.05 * unc).all() and (rel < 0.05 * (res + unc)).all(), (rel, res, unc)
    assert (r["roc_area"].cpu().numpy() > 0.9).all()
    sigma = float(np.sqrt(1.0 + 0.25))
    ens2, _ = _exchangeable(shift=sigma)
    r2 = V.exceedance_scores(torch.from_numpy(ens2).to(DEV), torch.from_numpy(obs).to(DEV), thr)
    assert (r2["brier_reliability"].cpu().numpy() > 5.0 * rel).all(), (r2["brier_reliability"], rel)


def _blobs(dx):
    """16 discs of radius 2.5 on 96 x 96, at least 24 pixels from the border, moved dx pixels along x"""
    rng = np.random.default_rng(33)
    yy, xx = np.mgrid[:96, :96]
    f = np.zeros((96, 96), np.float32)
    for cy, cx in zip(rng.integers(24, 72, 16), rng.integers(24, 68, 16)):
        f[(yy - cy) ** 2 + (xx - cx - dx) ** 2 <= 2.5 ** 2] = 1.0
    return f


def test_displaced_field_gains_skill_with_scale():
    """on the restatement: fss = 0.24, 0.36, 0.55, 0.82, 0.95, 0.98 at n = 1, 3, 5, 9, 17, 33"""
    scales = [1, 3, 5, 9, 17, 33]
    r = V.neighbourhood_scores(torch.from_numpy(_blobs(4)[None]).to(DEV), torch.from_numpy(_blobs(0)[None]).to(DEV), [0.5], scales)
    fss = r["fss"][0].cpu().numpy()
    assert (np.diff(fss) >= 0).all() and fss[0] < 0.5 and fss[-1] > 0.9, fss
    assert r["freq_bias"].item() == 1.0


# ---- --mode evaluate end to end ---------------------------------------------------------------------------------------------------

SPATIAL = {"thresholds": [0.5, 0.6, 10.0], "scales": [1, 3, 9]}
BASE_METRICS = {"gen_type", "rank", "n_samples", "n_obs", "shape", "mask_stats", "pixel_stats", "spatial_stats", "daily_stats"}
BASE_FIELDS = ({f"pixel_{k}" for k in ("hist_gen", "hist_obs", "hist_value_edges", "hist_absdiff", "hist_absdiff_edges")} |
               {f"spatial_{k}_per_pixel" for k in ("count", "mae", "rmse", "bias")} | {f"daily_{k}" for k in ("count", "mae", "rmse")})


def _evaluate(tmp_path, monkeypatch, tag, section):
    from sbgm_danra_amd.config_loader import load_config
    from sbgm_danra_amd.utils import get_model_string
    for k in ("DATA_DIR", "CKPT_DIR", "SAMPLE_DIR", "STATS_LOAD_DIR"):
        monkeypatch.setenv(k, str(tmp_path / k.lower()))
    monkeypatch.setenv("SLURM_CPUS_PER_TASK", "2")
    monkeypatch.setenv("PYTHONPATH", ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    raw = yaml.safe_load(open(os.path.join(ROOT, "sbgm_danra_amd", "config", "default_config.yaml")))
    raw["paths"]["evaluation_dir"] = str(tmp_path / f"ev_{tag}")
    raw["evaluation"].update(batch_size=3, n_repeats=4, eval_gen_type=["multiple", "repeated"], mask_stats=True,
                             eval_stat_methods=["pixel_stats", "spatial_stats", "daily_stats"])
    if section is not None:
        raw["evaluation"]["spatial_scores"] = section
    cfg_path = tmp_path / f"run_{tag}.yaml"
    cfg_path.write_text(yaml.safe_dump(raw))
    name = get_model_string(load_config(str(cfg_path)))
    samples = tmp_path / "sample_dir" / "generation" / name / "generated_samples"
    if not samples.exists():
        samples.mkdir(parents=True)
        rng = np.random.default_rng(24)
        for suffix, n, no in (("multi_n_3", 3, 3), ("repeated_n_4", 4, 1)):
            np.savez_compressed(samples / f"gen_samples_{suffix}.npz", _grid(rng, n, (1, 24, 40), nan_frac=0.0))
            np.savez_compressed(samples / f"eval_samples_{suffix}.npz", _grid(rng, no, (1, 24, 40), nan_frac=0.01))
            np.savez_compressed(samples / f"lsm_samples_{suffix}.npz", (rng.random((no, 1, 24, 40)) < 0.7).astype(np.float32))
    subprocess.run([sys.executable, "-m", "sbgm_danra_amd.cli.main_app", "--config_path", str(cfg_path), "--mode", "evaluate"],
                   cwd=ROOT, check=True, capture_output=True, text=True, timeout=300)
    stats = tmp_path / f"ev_{tag}" / name / "statistics"
    out = {label: (json.load(open(stats / f"{label}_metrics.json")), dict(np.load(stats / f"{label}_fields.npz")))
           for label in ("multiple", "repeated")}
    return out, samples


def test_evaluate_mode_with_and_without_the_section(tmp_path, monkeypatch):
    with_s, samples = _evaluate(tmp_path, monkeypatch, "with", SPATIAL)
    without, _ = _evaluate(tmp_path, monkeypatch, "without", None)
    T, S = len(SPATIAL["thresholds"]), len(SPATIAL["scales"])
    for label, suffix in (("multiple", "multi_n_3"), ("repeated", "repeated_n_4")):
        met, fld = with_s[label]
        met0, fld0 = without[label]
        # without the section: exactly the keys these three statistics always wrote, and the section changes none of their values
        assert set(met0) == BASE_METRICS and set(fld0) == BASE_FIELDS
        new_m = {"neighbourhood_stats"} | ({"exceedance_stats"} if label == "repeated" else set())
        new_f = ({f"neighbourhood_{k}" for k in ("num", "den", "fss_field", "events_gen", "events_obs")} |
                 ({"exceedance_table"} if label == "repeated" else set()))
        assert set(met) == BASE_METRICS | new_m and set(fld) == BASE_FIELDS | new_f
        assert json.dumps({k: met[k] for k in BASE_METRICS}, sort_keys=True) == json.dumps(met0, sort_keys=True)
        for k in BASE_FIELDS:
            np.testing.assert_array_equal(fld[k], fld0[k], err_msg=k)
        # with it: the values of direct calls on the same files
        g = torch.from_numpy(np.load(samples / f"gen_samples_{suffix}.npz")["arr_0"][:, 0]).to(DEV)
        o = torch.from_numpy(np.load(samples / f"eval_samples_{suffix}.npz")["arr_0"][:, 0]).to(DEV)
        m = torch.from_numpy(np.load(samples / f"lsm_samples_{suffix}.npz")["arr_0"][:, 0] > 0.5).to(DEV)
        n = g.shape[0]
        r = V.neighbourhood_scores(g, o, SPATIAL["thresholds"], SPATIAL["scales"], mask=m)
        ns = met["neighbourhood_stats"]
        assert ns["thresholds"] == SPATIAL["thresholds"] and ns["scales"] == SPATIAL["scales"]
        np.testing.assert_array_equal(np.array(ns["fss"], dtype=np.float64), r["fss"].cpu().numpy())
        np.testing.assert_array_equal(np.array(ns["freq_bias"], dtype=np.float64), r["freq_bias"].cpu().numpy())
        np.testing.assert_array_equal(np.array(ns["fss_useful"], dtype=np.float64), r["fss_useful"].cpu().numpy())
        fss, useful = r["fss"].cpu().numpy(), r["fss_useful"].cpu().numpy()
        want_scale = [next((sc for sc, f in zip(SPATIAL["scales"], fss[t]) if f >= useful[t]), None) for t in range(T)]
        assert ns["useful_scale"] == want_scale and ns["useful_scale"][2] is None and np.isnan(ns["fss"][2]).all()
        for k, shape, dtype in (("num", (n, T, S), np.int64), ("den", (n, T, S), np.int64), ("fss_field", (n, T, S), np.float64),
                                ("events_gen", (n, T), np.int64), ("events_obs", (n, T), np.int64)):
            a = fld[f"neighbourhood_{k}"]
            assert a.shape == shape and a.dtype == dtype, k
            np.testing.assert_array_equal(a, r[k].cpu().numpy(), err_msg=k)
        if label == "repeated":
            x = V.exceedance_scores(g, o[0], SPATIAL["thresholds"], mask=m[0])
            es = met["exceedance_stats"]
            assert es["M"] == 4 and es["count"] == int(x["count"]) and es["thresholds"] == SPATIAL["thresholds"]
            for k in V.EXCEEDANCE_KEYS:
                np.testing.assert_array_equal(np.array(es[k], dtype=np.float64), x[k].cpu().numpy(), err_msg=k)
            assert fld["exceedance_table"].shape == (T, 5, 2) and fld["exceedance_table"].dtype == np.int64
            np.testing.assert_array_equal(fld["exceedance_table"], x["table"].cpu().numpy())
