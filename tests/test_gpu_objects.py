"""Connected objects (K51) and SAL scores (K52) of csrc/verify_objects.hip against the numpy / scipy restatement in
tests/objects_ref.py: the labels exactly as a partition with canonical numbers, the integer outputs and the dyadic sums
exactly, the fp64 scores to the rounding of their sums, reproducibility across calls and chunkings, and `--mode evaluate` end
to end with and without the `evaluation.object_scores` section."""
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
import objects_ref as R  # noqa: E402
from sbgm_danra_amd import verification as V  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda")
# 261 x 2047: every thread of the row kernel owns columns and the last one a ragged set; more rows than any workgroup covers, a
# pixel count that is no multiple of the 256-pixel and 2048-pixel blocks of the merge and accumulation kernels
LABEL_SHAPES = [(2, 2), (5, 7), (37, 53), (64, 128), (70, 131), (261, 2047), (589, 789)]
CONTENTS = ("random_0.40", "random_0.59", "random_0.75", "serpentine", "rings", "comb_down", "comb_across", "checkerboard", "all",
            "empty", "cut")


def _content(name, H, W, rng):
    """(bool image, uint8 mask, bool NaN positions) of one label case"""
    r, c = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    mask, nan = np.ones((H, W), np.uint8), np.zeros((H, W), bool)
    if name.startswith("random"):
        img = rng.random((H, W)) < float(name.split("_")[1])
    elif name == "serpentine":                   # full even rows joined at alternating ends: one object as long as the field
        img = (r % 2 == 0) | ((r % 4 == 1) & (c == W - 1)) | ((r % 4 == 3) & (c == 0))
    elif name == "rings":
        img = np.maximum(abs(r - H // 2), abs(c - W // 2)) % 2 == 0
    elif name == "comb_down":                    # a spine along the first row, teeth down every other column: they cross every row
        img = (r == 0) | (c % 2 == 0)
    elif name == "comb_across":                  # a spine down the first column, teeth along every other row: every block border
        img = (c == 0) | (r % 2 == 0)
    elif name == "checkerboard":
        img = (r + c) % 2 == 0
    elif name == "all":
        img = np.ones((H, W), bool)
    elif name == "empty":
        img = np.zeros((H, W), bool)
    else:                                        # an all-object field cut by a masked column and a row of NaNs
        img = np.ones((H, W), bool)
        mask[:, W // 2] = 0
        nan[H // 2, :] = True
    return img, mask, nan


@functools.lru_cache(maxsize=None)
def _label_case(shape_idx):
    """fields [len(CONTENTS), H, W] with object value 1 and background 0, their mask, and the restatement's labels for both
    connectivities — computed once per shape"""
    H, W = LABEL_SHAPES[shape_idx]
    rng = np.random.default_rng([51, shape_idx])
    parts = [_content(name, H, W, rng) for name in CONTENTS]
    fields = np.stack([p[0] for p in parts]).astype(np.float32)
    fields[np.stack([p[2] for p in parts])] = np.nan
    mask = np.stack([p[1] for p in parts])
    want = {conn: R.object_labels(fields, 1.0, mask=mask, connectivity=conn) for conn in (4, 8)}
    return fields, mask, want


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("shape_idx", range(len(LABEL_SHAPES)))
def test_labels_match_scipy_as_a_partition(shape_idx, connectivity):
    fields, mask, want = _label_case(shape_idx)
    got, status = V.object_labels(torch.from_numpy(fields).to(DEV), 1.0, mask=torch.from_numpy(mask).to(DEV),
                                  connectivity=connectivity, return_status=True)
    assert got.dtype == torch.int32 and got.shape == fields.shape and int(status) == 0
    got = got.cpu().numpy()
    for i, name in enumerate(CONTENTS):
        np.testing.assert_array_equal(got[i], want[connectivity][i], err_msg=f"{name} at {LABEL_SHAPES[shape_idx]}")
    if min(LABEL_SHAPES[shape_idx]) >= 5:        # the cases are what they are meant to be
        n = {name: len(np.unique(want[connectivity][i][want[connectivity][i] > 0])) for i, name in enumerate(CONTENTS)}
        H, W = LABEL_SHAPES[shape_idx]
        assert n["serpentine"] == 1 and n["comb_down"] == 1 and n["comb_across"] == 1 and n["all"] == 1 and n["empty"] == 0
        assert n["cut"] == 4 and n["checkerboard"] == (1 if connectivity == 8 else (H * W + 1) // 2)


def test_labels_without_mask_and_shared_mask():
    fields, mask, _ = _label_case(2)
    x = torch.from_numpy(fields).to(DEV)
    np.testing.assert_array_equal(V.object_labels(x, 1.0, connectivity=4).cpu().numpy(), R.object_labels(fields, 1.0, connectivity=4))
    shared = np.random.default_rng(5).random((1,) + fields.shape[1:]) < 0.8
    for m in (torch.from_numpy(shared).to(DEV), torch.from_numpy(shared.astype(np.float32)).to(DEV)):
        np.testing.assert_array_equal(V.object_labels(x, 0.5, mask=m).cpu().numpy(), R.object_labels(fields, 0.5, mask=shared))


# ---- scores ----------------------------------------------------------------------------------------------------------------
# data are multiples of 0.25 in [0, 16]: 4.0 equals data values (the >= edge), 4.1 falls between two, 17 is above the maximum (no
# objects: S, L2 NaN); the relative threshold comes last
THRESHOLDS = [4.0, 4.1, 17.0]
RELATIVE = {"factor": 0.5, "quantile": 0.9, "wet": 0.25}
ROWS = [(5, 1, 1), (3, 3, 3), (4, 4, 0)]
SCORE_SHAPES = [(37, 53), (70, 131)]
EXACT_KEYS = ("threshold", "n_objects", "area", "valid", "area_hist", "mass", "com", "domain_mean")
CLOSE_KEYS = ("S", "A", "L1", "L2", "L", "V", "r")
DTYPES = dict(threshold=torch.float32, n_objects=torch.int64, area=torch.int64, valid=torch.int64, area_hist=torch.int64,
              status=torch.int32)


def _dyadic(rng, n, H, W, nan_frac=0.01):
    """blocky fields with speckle, multiples of 0.25 in [0, 16]: objects of every size, holes, and diagonal contacts"""
    coarse = rng.integers(0, 65, size=(n, -(-H // 4), -(-W // 4)))
    a = np.kron(coarse, np.ones((4, 4), np.int64))[:, :H, :W]
    speck = rng.random(a.shape) < 0.3
    a = np.where(speck, rng.integers(0, 65, size=a.shape), a)
    a = (a * 0.25).astype(np.float32)
    a[rng.random(a.shape) < nan_frac] = np.nan
    return a


@functools.lru_cache(maxsize=None)
def _score_case(shape_idx, n, no, nm, connectivity):
    H, W = SCORE_SHAPES[shape_idx]
    rng = np.random.default_rng([52, shape_idx, n, no, nm])
    gen, obs = _dyadic(rng, n, H, W), _dyadic(rng, no, H, W)
    mask = (rng.random((nm, H, W)) < 0.8) if nm else None
    return gen, obs, mask, R.object_scores(gen, obs, THRESHOLDS, RELATIVE, mask, connectivity)


def _run(gen, obs, mask, thresholds, relative, connectivity, **kw):
    m = None if mask is None else torch.from_numpy(mask).to(DEV)
    return V.object_scores(torch.from_numpy(gen).to(DEV), torch.from_numpy(obs).to(DEV), thresholds, relative=relative, mask=m,
                           connectivity=connectivity, **kw)


def _check_exact(got, want):
    assert int(got["status"]) == 0
    for k in EXACT_KEYS:
        assert got[k].dtype == DTYPES.get(k, torch.float64), k
        np.testing.assert_array_equal(got[k].cpu().numpy(), want[k], err_msg=k)        # NaNs compare equal here


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("n,no,nm", ROWS)
@pytest.mark.parametrize("shape_idx", range(len(SCORE_SHAPES)))
def test_scores_match_restatement_on_dyadic_data(shape_idx, n, no, nm, connectivity):
    gen, obs, mask, want = _score_case(shape_idx, n, no, nm, connectivity)
    got = _run(gen, obs, mask, THRESHOLDS, RELATIVE, connectivity)
    _check_exact(got, want)
    # 1e-9 absolute: at most 2^18 objects per fixed-order fp64 sum (3e-11 relative), a handful of sums and quotients on values
    # bounded by 2; V and r are larger (up to the area and the diagonal) but every R_n is exact on these data, so they too carry
    # only the rounding of their fp64 sums
    for k in CLOSE_KEYS:
        assert got[k].dtype == torch.float64 and got[k].shape == want[k].shape, k
        np.testing.assert_allclose(got[k].cpu().numpy(), want[k], rtol=0, atol=1e-9, equal_nan=True, err_msg=k)
    assert not want["n_objects"][:, :, 2].any() and np.isnan(want["S"][:, 2]).all()     # 17 is above every value
    assert (want["n_objects"][:, :, :2] > 0).all() and (want["threshold"][:, :, 3] > 0.25).all()


def test_scores_full_domain_and_long_objects():
    """589 x 789 (several accumulation blocks per field): a blocky field against a serpentine and a checkerboard of dyadic values"""
    H, W = 589, 789
    rng = np.random.default_rng(53)
    gen = _dyadic(rng, 2, H, W, nan_frac=0.0)
    gen[1][rng.random((H, W)) < 0.01] = np.nan                   # invalid pixels cut the checkerboard's field, not the serpentine's
    r, c = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    snake = (r % 2 == 0) | ((r % 4 == 1) & (c == W - 1)) | ((r % 4 == 3) & (c == 0))
    obs = np.stack([np.where(snake, 4.0 + 0.25 * (c % 8), 0.0), np.where((r + c) % 2 == 0, 4.0 + 0.25 * (r % 16), 1.0)]).astype(np.float32)
    for conn in (4, 8):
        want = R.object_scores(gen, obs, [4.0], None, None, conn)
        got = _run(gen, obs, None, [4.0], None, conn)
        _check_exact(got, want)
        for k in CLOSE_KEYS:
            g, w = got[k].cpu().numpy(), want[k]
            print(k, conn, "largest absolute error", float(np.nanmax(np.abs(g - w), initial=0.0)), "largest value", float(np.nanmax(np.abs(w))))
            np.testing.assert_allclose(g, w, rtol=0, atol=1e-9, equal_nan=True, err_msg=k)
    assert want["n_objects"][1, 0, 0] == 1 and want["area"][1, 0, 0] == snake.sum()


def test_scores_on_arbitrary_fp32_data_stay_within_the_fixed_point_bound():
    """uniform data in [0, 100), thresholds >= 1: mass within (vmax / thr) 2^-29 relative of the fp64 sum, the scores S, A, L1,
    L2 and L within 8 times that bound, absolute.  V and r are not dimensionless: V = sum R^2 / Rmax / sum R is a quotient of
    two sums that are each within the bound relative (Rmax is exact), so it is held to 8 times the bound relative; r is a
    weighted mean of distances between centres whose coordinates are quotients of such sums, which bounds its error by
    (4 sqrt 2 + 2) bound d < 8 bound d, and it is held to the stricter 8 times the bound relative to r itself (r <= d)."""
    rng = np.random.default_rng(54)
    n, H, W = 3, 70, 131
    gen, obs = ((rng.random((k, H, W)) * 100.0).astype(np.float32) for k in (n, n))
    thr = [1.0, 50.0, 90.0]
    rel = {"factor": 1.0 / 15.0, "quantile": 0.95, "wet": 1.0}
    want = R.object_scores(gen, obs, thr, rel, None, 8)
    got = _run(gen, obs, None, thr, rel, 8)
    for k in ("threshold", "n_objects", "area", "valid", "area_hist"):
        np.testing.assert_array_equal(got[k].cpu().numpy(), want[k], err_msg=k)
    assert int(got["status"]) == 0
    vmax = np.stack([gen.reshape(n, -1).max(axis=1), obs.reshape(n, -1).max(axis=1)]).astype(np.float64)
    bound = vmax[:, :, None] / want["threshold"].astype(np.float64) * 2.0 ** -29                   # [2, N, T]
    mass = got["mass"].cpu().numpy()
    print("mass: largest relative error / bound", float((np.abs(mass - want["mass"]) / want["mass"] / bound).max()))
    assert (np.abs(mass - want["mass"]) <= bound * want["mass"]).all()
    worst = bound.max(axis=0)                                                                        # [N, T]: the looser side
    for k in CLOSE_KEYS:
        g, w = got[k].cpu().numpy(), want[k]
        if k in ("V", "r"):
            err, lim = np.abs(g - w) / np.abs(w), 8 * bound
        else:
            err, lim = np.abs(g - w), 8 * (worst if w.ndim == 2 else worst.max(axis=1))
        print(k, "largest error / (8 x bound)", float(np.nanmax(err / lim)))
        assert np.array_equal(np.isnan(g), np.isnan(w)) and (err[~np.isnan(w)] <= lim[~np.isnan(w)]).all(), k


def _bits(t):
    return t.contiguous().view(torch.int64 if t.element_size() == 8 else torch.int32)


@pytest.mark.parametrize("n,no,nm", ROWS[:2])
def test_repeat_and_chunking_are_bit_equal(n, no, nm):
    gen, obs, mask, _ = _score_case(1, n, no, nm, 8)
    a = _run(gen, obs, mask, THRESHOLDS, RELATIVE, 8)
    b = _run(gen, obs, mask, THRESHOLDS, RELATIVE, 8)
    H, W = SCORE_SHAPES[1]
    one_pair = _run(gen, obs, mask, THRESHOLDS, RELATIVE, 8, max_workspace_bytes=0)                 # one field x one threshold a chunk
    one_field = _run(gen, obs, mask, THRESHOLDS, RELATIVE, 8, max_workspace_bytes=4096 + 4 * 72 * H * W + 1000)
    for other in (b, one_pair, one_field):
        assert int(other["status"]) == 0
        for k in V.OBJECT_KEYS:
            assert torch.equal(_bits(a[k].reshape(-1)), _bits(other[k].reshape(-1))), k


# ---- --mode evaluate end to end ---------------------------------------------------------------------------------------------

SECTION = {"thresholds": [2.0, 20.0], "relative": {"factor": 0.5, "quantile": 0.9, "wet": 0.25}, "connectivity": 8}
BASE_METRICS = {"gen_type", "rank", "n_samples", "n_obs", "shape", "mask_stats", "pixel_stats", "spatial_stats", "daily_stats"}
BASE_FIELDS = ({f"pixel_{k}" for k in ("hist_gen", "hist_obs", "hist_value_edges", "hist_absdiff", "hist_absdiff_edges")} |
               {f"spatial_{k}_per_pixel" for k in ("count", "mae", "rmse", "bias")} | {f"daily_{k}" for k in ("count", "mae", "rmse")})
OBJECT_FIELDS = {f"objects_{k}" for k in V.OBJECT_KEYS if k != "status"}


def _write_samples(samples):
    samples.mkdir(parents=True)
    rng = np.random.default_rng(25)
    for suffix, n, no in (("multi_n_3", 3, 3), ("repeated_n_4", 4, 1)):
        np.savez_compressed(samples / f"gen_samples_{suffix}.npz", _dyadic(rng, n, 24, 40, nan_frac=0.0)[:, None])
        np.savez_compressed(samples / f"eval_samples_{suffix}.npz", _dyadic(rng, no, 24, 40)[:, None])
        np.savez_compressed(samples / f"lsm_samples_{suffix}.npz", (rng.random((no, 1, 24, 40)) < 0.8).astype(np.float32))


def _config(tmp_path, monkeypatch, tag, section):
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
        raw["evaluation"]["object_scores"] = section
    cfg_path = tmp_path / f"run_{tag}.yaml"
    cfg_path.write_text(yaml.safe_dump(raw))
    cfg = load_config(str(cfg_path))
    name = get_model_string(cfg)
    samples = tmp_path / "sample_dir" / "generation" / name / "generated_samples"
    if not samples.exists():
        _write_samples(samples)
    return cfg, cfg_path, name, samples


def _evaluate(tmp_path, monkeypatch, tag, section):
    _, cfg_path, name, samples = _config(tmp_path, monkeypatch, tag, section)
    subprocess.run([sys.executable, "-m", "sbgm_danra_amd.cli.main_app", "--config_path", str(cfg_path), "--mode", "evaluate"],
                   cwd=ROOT, check=True, capture_output=True, text=True, timeout=300)
    stats = tmp_path / f"ev_{tag}" / name / "statistics"
    out = {label: (json.load(open(stats / f"{label}_metrics.json")), dict(np.load(stats / f"{label}_fields.npz")))
           for label in ("multiple", "repeated")}
    return out, samples


def test_evaluate_mode_with_and_without_the_section(tmp_path, monkeypatch):
    with_s, samples = _evaluate(tmp_path, monkeypatch, "with", SECTION)
    without, _ = _evaluate(tmp_path, monkeypatch, "without", None)
    T = len(SECTION["thresholds"]) + 1
    for label, suffix in (("multiple", "multi_n_3"), ("repeated", "repeated_n_4")):
        met, fld = with_s[label]
        met0, fld0 = without[label]
        # without the section: exactly what these statistics always wrote; the section changes none of their values
        assert set(met0) == BASE_METRICS and set(fld0) == BASE_FIELDS
        assert set(met) == BASE_METRICS | {"objects"} and set(fld) == BASE_FIELDS | OBJECT_FIELDS
        assert json.dumps({k: met[k] for k in BASE_METRICS}, sort_keys=True) == json.dumps(met0, sort_keys=True)
        for k in BASE_FIELDS:
            np.testing.assert_array_equal(fld[k], fld0[k], err_msg=k)
        # with it: the values of a direct call on the same files
        g = torch.from_numpy(np.load(samples / f"gen_samples_{suffix}.npz")["arr_0"][:, 0]).to(DEV)
        o = torch.from_numpy(np.load(samples / f"eval_samples_{suffix}.npz")["arr_0"][:, 0]).to(DEV)
        m = torch.from_numpy(np.load(samples / f"lsm_samples_{suffix}.npz")["arr_0"][:, 0] > 0.5).to(DEV)
        n = g.shape[0]
        r = V.object_scores(g, o, SECTION["thresholds"], relative=SECTION["relative"], mask=m, connectivity=8)
        for k in V.OBJECT_KEYS:
            if k != "status":
                np.testing.assert_array_equal(fld[f"objects_{k}"], r[k].cpu().numpy(), err_msg=k)
        assert fld["objects_S"].shape == (n, T) and fld["objects_A"].shape == (n,) and fld["objects_n_objects"].shape == (2, n, T)
        ob = met["objects"]
        assert ob["thresholds"] == SECTION["thresholds"] and ob["relative"] == SECTION["relative"] and ob["connectivity"] == 8
        assert ob["n_fields"] == n and [row["threshold"] for row in ob["per_threshold"]] == ["2", "20", "relative"]
        S, A, L = (r[k].cpu().numpy() for k in ("S", "A", "L"))
        for t, row in enumerate(ob["per_threshold"]):
            for key, col in (("S", S[:, t]), ("A", A), ("L", L[:, t])):
                good = col[~np.isnan(col)]
                assert row[key]["nan"] == int(np.isnan(col).sum()), key
                if good.size:
                    assert [row[key]["p25"], row[key]["median"], row[key]["p75"]] == [float(v) for v in np.percentile(good, [25, 50, 75])]
                else:
                    assert np.isnan(row[key]["median"])
            assert [row["n_objects_gen"], row["n_objects_obs"]] == r["n_objects"][:, :, t].sum(dim=1).tolist()
            assert row["area_hist_gen"] == r["area_hist"][0, t].tolist() and row["area_hist_obs"] == r["area_hist"][1, t].tolist()
        assert ob["per_threshold"][1]["S"]["nan"] == n and ob["per_threshold"][1]["n_objects_gen"] == 0      # 20 is above every value
        assert ob["per_threshold"][0]["S"]["nan"] == 0 and ob["per_threshold"][0]["n_objects_obs"] > 0


def test_evaluation_raises_on_a_nonzero_status(tmp_path, monkeypatch):
    from sbgm_danra_amd.evaluate_sbgm import evaluation as E
    cfg, _, _, _ = _config(tmp_path, monkeypatch, "status", SECTION)
    ev = E.Evaluation(cfg, generated_sample_type="multiple", n_samples=3)
    res = ev.object_statistics()
    assert "objects" in ev.metrics and res["S"].shape == (3, 3)
    real = V.object_scores

    def capped(*a, **kw):
        out = real(*a, **kw)
        out["status"] = out["status"] + 1
        return out

    monkeypatch.setattr(E.V, "object_scores", capped)
    with pytest.raises(RuntimeError, match="status 1"):
        ev.object_statistics()
