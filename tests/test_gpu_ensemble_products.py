"""Ensemble products (K47, csrc/verify_products.hip) against the numpy restatement in tests/ensemble_products_ref.py: validity,
the count, and min / max / quantiles / exceedance probabilities equal to the restatement, the mean and the standard deviation
bit-equal (the bound set for the latter is one fp32 ulp; the MI355X shows none, so equality is asserted); the
invariants of the maps, their independence of the member order, the limits, the full DANRA domain, and `--mode generate` /
`--mode evaluate` end to end with and without the `evaluation.ensemble_products` section."""
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
import ensemble_products_ref as R  # noqa: E402
from sbgm_danra_amd import verification as V  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda")
MEMBERS = [2, 3, 5, 16, 17, 64, 65, 257, 1500]
SHAPES = [(37, 53), (32, 48)]                       # HW odd and no multiple of 64; aligned
KINDS = ["grid", "normal", "rain"]
MASKS = ["u8", "f32", "bool", None]
QUANTILES = [0, 0.05, 0.25, 1 / 3, 0.5, 0.9, 0.99, 1]
# grid data are multiples of 0.25 in [-2, 3]: 0.5 and 0.0 equal data values (the >= edge; 0.0 is also the rain floor), 0.6 falls
# between two, 10 is above the maximum and -5 below the minimum
THRESHOLDS = [0.5, 0.6, 0.0, 10.0, -5.0]
MAPS = ("mean", "std", "min", "max", "quantiles", "exceed_prob")


def make_ens(rng, kind, M, shape, nan_frac=0.01):
    """grid: multiples of 0.25 in [-2, 3] (heavy ties); normal; rain: max(3 z - 2, 0), more than half exact zeros.  nan_frac of
    the pixels get a NaN in one member."""
    if kind == "grid":
        ens = (rng.integers(-8, 13, size=(M, *shape)) * 0.25).astype(np.float32)
    else:
        z = rng.standard_normal((M, *shape)).astype(np.float32)
        ens = z if kind == "normal" else np.maximum(np.float32(3.0) * z - np.float32(2.0), np.float32(0.0))
    ys, xs = np.nonzero(rng.random(shape) < nan_frac)
    ens[rng.integers(0, M, size=ys.shape[0]), ys, xs] = np.nan
    return ens


def _mask_tensor(mask, mdtype):
    if mdtype is None:
        return None
    t = torch.from_numpy(mask).to(DEV)
    return t.to(torch.uint8) if mdtype == "u8" else (t.float() if mdtype == "f32" else t)


@functools.lru_cache(maxsize=None)
def _case(M, shape, kind, masked):
    """inputs and their restatement, computed once per case and shared by the mask dtypes"""
    rng = np.random.default_rng([MEMBERS.index(M), SHAPES.index(shape), KINDS.index(kind)])
    ens = make_ens(rng, kind, M, shape)
    mask = rng.random(shape) < 0.8
    return ens, mask, R.ensemble_products(ens, QUANTILES, THRESHOLDS, mask if masked else None)


def _equal(got, want):
    """torch.equal semantics on numpy arrays: numerically equal (-0 == +0) with the NaN positions matched"""
    return got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)) and bool((got[~np.isnan(got)] == want[~np.isnan(want)]).all())


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _bit_equal(a, b):
    return all(torch.equal(_bits(a[k]), _bits(b[k])) for k in MAPS + ("count",))


@pytest.mark.parametrize("mdtype", MASKS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("M", MEMBERS)
def test_products_match_restatement(M, shape, kind, mdtype):
    """std: the bound set for it is one fp32 ulp; on the MI355X the largest deviation over all 216 cases was 0 (the device's fp64
    division and square root round as numpy's do), so the check is tightened to bit equality, as for the mean"""
    ens, mask, want = _case(M, shape, kind, mdtype is not None)
    got = V.ensemble_products(torch.from_numpy(ens).to(DEV), QUANTILES, THRESHOLDS, mask=_mask_tensor(mask, mdtype))
    assert int(got["count"]) == want["count"]
    g = {k: got[k].cpu().numpy() for k in MAPS}
    for k in MAPS:
        assert g[k].dtype == np.float32 and g[k].shape == want[k].shape, k
        np.testing.assert_array_equal(np.isnan(g[k]), np.isnan(want[k]), err_msg=k)
    for k in ("min", "max", "quantiles", "exceed_prob"):
        assert _equal(g[k], want[k]), k
    np.testing.assert_array_equal(g["mean"].view(np.int32), want["mean"].view(np.int32))
    ok = ~np.isnan(want["std"])
    dev = np.abs(g["std"][ok].astype(np.float64) - want["std"][ok].astype(np.float64)) / np.spacing(np.abs(want["std"][ok])).astype(np.float64)
    print(f"products M={M} {shape} {kind} mask={mdtype}: std largest deviation {float(dev.max()) if dev.size else 0.0:.3f} ulp")
    np.testing.assert_array_equal(g["std"][ok].view(np.int32), want["std"][ok].view(np.int32))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M", [2, 17, 64])
def test_invariants_on_the_device_output(M, kind):
    ens, mask, _ = _case(M, SHAPES[0], kind, True)
    r = V.ensemble_products(torch.from_numpy(ens).to(DEV), QUANTILES, THRESHOLDS, mask=torch.from_numpy(mask).to(DEV))
    q, e = r["quantiles"], r["exceed_prob"]
    assert torch.equal(_bits(q[0]), _bits(r["min"])) and torch.equal(_bits(q[-1]), _bits(r["max"]))
    ok = ~torch.isnan(r["mean"])
    assert int(ok.sum()) == int(r["count"]) > 0
    assert bool((q[1:][:, ok] >= q[:-1][:, ok]).all())                          # QUANTILES ascend
    order = sorted(range(len(THRESHOLDS)), key=lambda i: THRESHOLDS[i])
    es = e[order][:, ok]
    assert bool((es[1:] <= es[:-1]).all())
    # exactly 1 where no member lies below the threshold and exactly 0 where none reaches it: everywhere for -5 and 10 on the
    # grid data; a rain or normal member can pass 10 (3 z - 2 >= 10 at z >= 4), and that pixel then holds at least 1 / M
    for thr in (-5.0, 10.0):
        et = e[THRESHOLDS.index(thr)][ok]
        all_in, none_in = r["min"][ok] >= thr, r["max"][ok] < thr
        assert bool((et[all_in] == 1.0).all()) and bool((et[none_in] == 0.0).all())
        assert bool((et[~all_in] <= 1.0 - 1.0 / M + 1e-6).all()) and bool((et[~none_in] >= 1.0 / M - 1e-6).all())
    assert bool((r["min"][ok] >= -5.0).all())
    if kind == "grid":
        assert bool((r["max"][ok] < 10.0).all())
    if M == 2:
        a, b = r["min"].double(), r["max"].double()
        med = (a + 0.5 * (b - a)).float()
        assert torch.equal(q[QUANTILES.index(0.5)][ok], med[ok])


@pytest.mark.parametrize("kind", KINDS)
def test_member_order_and_repeatability(kind):
    ens, mask, _ = _case(65, SHAPES[0], kind, True)
    e, m = torch.from_numpy(ens).to(DEV), torch.from_numpy(mask).to(DEV)
    first = V.ensemble_products(e, QUANTILES, THRESHOLDS, mask=m)
    assert _bit_equal(first, V.ensemble_products(e, QUANTILES, THRESHOLDS, mask=m))
    perm = torch.from_numpy(np.random.default_rng(7).permutation(65)).to(DEV)
    shuffled = V.ensemble_products(e[perm], QUANTILES, THRESHOLDS, mask=m)
    for k in ("min", "max", "quantiles", "exceed_prob", "count"):
        assert torch.equal(_bits(first[k]), _bits(shuffled[k])), k


def test_limits():
    with pytest.raises(ValueError):
        V.ensemble_products(torch.zeros(1, 4, 4, device=DEV), [0.5], [0.5])
    with pytest.raises(ValueError):
        V.ensemble_products(torch.zeros(4096, 4, 4, device=DEV), [0.5], [0.5])
    rng = np.random.default_rng(11)
    ens = make_ens(rng, "normal", 4095, (4, 4), nan_frac=0.0)
    want = R.ensemble_products(ens, [0.5, 0.999], [0.0])
    e = torch.from_numpy(ens).to(DEV)
    r = V.ensemble_products(e, [0.5, 0.999], [0.0])
    assert int(r["count"]) == 16
    for k in ("min", "max", "quantiles", "exceed_prob"):
        assert _equal(r[k].cpu().numpy(), want[k]), k
    only_t = V.ensemble_products(e, [], [0.0])                                  # Q = 0 with T > 0
    assert only_t["quantiles"].shape == (0, 4, 4) and torch.equal(only_t["exceed_prob"], r["exceed_prob"])
    only_q = V.ensemble_products(e, [0.5, 0.999], [])                           # T = 0 with Q > 0
    assert only_q["exceed_prob"].shape == (0, 4, 4) and torch.equal(only_q["quantiles"], r["quantiles"])
    assert torch.equal(only_q["mean"], r["mean"]) and torch.equal(only_t["std"], r["std"])
    many = [i / 15 for i in range(16)]                                          # 16 levels: two launches of 8
    q16 = V.ensemble_products(e[:9], many, [])["quantiles"].cpu().numpy()
    assert _equal(q16, R.ensemble_products(ens[:9], many)["quantiles"])
    q11 = V.ensemble_products(e[:9], many[:11], [])["quantiles"].cpu().numpy()  # 8 + a short rest of 3
    assert _equal(q11, q16[:11])


def test_full_domain():
    rng = np.random.default_rng(3)
    ens = make_ens(rng, "rain", 8, (589, 789), nan_frac=0.001)
    mask = rng.random((589, 789)) < 0.8
    want = R.ensemble_products(ens, [0.5, 0.9], [0.5], mask)
    got = V.ensemble_products(torch.from_numpy(ens).to(DEV), [0.5, 0.9], [0.5], mask=torch.from_numpy(mask).to(DEV))
    assert int(got["count"]) == want["count"]
    for k in ("min", "max", "quantiles", "exceed_prob", "mean"):
        assert _equal(got[k].cpu().numpy(), want[k]), k
    s, ok = got["std"].cpu().numpy(), ~np.isnan(want["std"])
    np.testing.assert_array_equal(np.isnan(s), ~ok)
    np.testing.assert_array_equal(s[ok].view(np.int32), want["std"][ok].view(np.int32))


# ---- --mode generate end to end -----------------------------------------------------------------------------------------------------

PRODUCTS = {"quantiles": [0.0, 0.25, 0.5, 1.0], "thresholds": [0.0, 0.5]}
FILE_KEYS = {"mean", "std", "min", "max", "quantiles", "exceed_prob", "quantile_levels", "thresholds", "members"}


def _generate(tmp_path, monkeypatch, tag, section):
    """one `--mode generate` run of a tiny configuration into its own sample directory; returns that directory's file folder"""
    from oracle import torch_ref as O
    from sbgm_danra_amd.cli import main_app
    from sbgm_danra_amd.config_loader import load_config
    from sbgm_danra_amd.utils import get_model_string
    for k in ("DATA_DIR", "CKPT_DIR", "STATS_LOAD_DIR"):
        monkeypatch.setenv(k, str(tmp_path / k.lower()))
    monkeypatch.setenv("SAMPLE_DIR", str(tmp_path / f"samples_{tag}"))
    monkeypatch.setenv("SLURM_CPUS_PER_TASK", "2")
    raw = yaml.safe_load(open(os.path.join(ROOT, "sbgm_danra_amd", "config", "default_config.yaml")))
    raw["highres"]["data_size"] = [64, 64]
    raw["lowres"]["data_size"] = [64, 64]
    raw["lowres"]["condition_variables"] = ["temp", "prcp"]
    raw["stationary_conditions"]["geographic_conditions"]["sample_w_geo"] = True
    raw["stationary_conditions"]["seasonal_conditions"]["sample_w_cond_season"] = True
    raw["sampler"]["n_timesteps"] = 4
    raw["evaluation"].update(batch_size=3, gen_type=["repeated"], n_repeats=4)
    if section is not None:
        raw["evaluation"]["ensemble_products"] = section
    p = tmp_path / f"run_{tag}.yaml"
    p.write_text(yaml.safe_dump(raw))
    cfg = load_config(str(p))
    ckpt_dir = os.path.join(cfg.paths.path_save, cfg.paths.checkpoint_dir)
    os.makedirs(ckpt_dir, exist_ok=True)
    ckpt = os.path.join(ckpt_dir, get_model_string(cfg) + ".pth.tar")
    if not os.path.exists(ckpt):
        torch.save({"network_params": O.synth_state_dict(O.build_scorenet(6, num_classes=4)), "optimizer_params": {}}, ckpt)
    main_app.main(["--config_path", str(p), "--mode", "generate"])
    return os.path.join(cfg.paths.sample_dir, "generation", get_model_string(cfg), "generated_samples")


def test_generate_mode_with_and_without_the_section(tmp_path, monkeypatch):
    without = _generate(tmp_path, monkeypatch, "without", None)
    with_s = _generate(tmp_path, monkeypatch, "with", PRODUCTS)
    assert not [f for f in os.listdir(without) if f.startswith("ens_products")]
    assert [f for f in os.listdir(with_s) if f.startswith("ens_products")] == ["ens_products_repeated_n_4.npz"]
    assert sorted(set(os.listdir(with_s)) - {"ens_products_repeated_n_4.npz"}) == sorted(os.listdir(without))
    gen = np.load(os.path.join(with_s, "gen_samples_repeated_n_4.npz"))["arr_0"]
    assert gen.shape == (4, 64, 64)
    np.testing.assert_array_equal(gen.view(np.int32), np.load(os.path.join(without, "gen_samples_repeated_n_4.npz"))["arr_0"].view(np.int32))
    f = dict(np.load(os.path.join(with_s, "ens_products_repeated_n_4.npz")))
    assert set(f) == FILE_KEYS and int(f["members"]) == 4
    assert f["quantile_levels"].tolist() == PRODUCTS["quantiles"] and f["thresholds"].tolist() == PRODUCTS["thresholds"]
    r = V.ensemble_products(torch.from_numpy(gen).to(DEV), PRODUCTS["quantiles"], PRODUCTS["thresholds"])
    for k in MAPS:
        assert f[k].dtype == np.float32, k
        np.testing.assert_array_equal(f[k].view(np.int32), r[k].cpu().numpy().view(np.int32), err_msg=k)
    assert f["quantiles"].shape == (4, 64, 64) and f["exceed_prob"].shape == (2, 64, 64) and np.isfinite(f["mean"]).all()


# ---- --mode evaluate end to end -----------------------------------------------------------------------------------------------------

BASE_METRICS = {"gen_type", "rank", "n_samples", "n_obs", "shape", "mask_stats", "pixel_stats", "spatial_stats", "daily_stats"}
BASE_FIELDS = ({f"pixel_{k}" for k in ("hist_gen", "hist_obs", "hist_value_edges", "hist_absdiff", "hist_absdiff_edges")} |
               {f"spatial_{k}_per_pixel" for k in ("count", "mae", "rmse", "bias")} | {f"daily_{k}" for k in ("count", "mae", "rmse")})


def _grid(rng, n, shape, nan_frac=0.01):
    a = (rng.integers(-8, 13, size=(n, *shape)) * 0.25).astype(np.float32)
    a[rng.random(a.shape) < nan_frac] = np.nan
    return a


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
        raw["evaluation"]["ensemble_products"] = section
    cfg_path = tmp_path / f"run_{tag}.yaml"
    cfg_path.write_text(yaml.safe_dump(raw))
    name = get_model_string(load_config(str(cfg_path)))
    samples = tmp_path / "sample_dir" / "generation" / name / "generated_samples"
    if not samples.exists():
        samples.mkdir(parents=True)
        rng = np.random.default_rng(24)
        for suffix, n, no in (("multi_n_3", 3, 3), ("repeated_n_4", 4, 1)):
            np.savez_compressed(samples / f"gen_samples_{suffix}.npz", _grid(rng, n, (1, 24, 40), nan_frac=0.0 if n == 3 else 0.002))
            np.savez_compressed(samples / f"eval_samples_{suffix}.npz", _grid(rng, no, (1, 24, 40), nan_frac=0.01))
            np.savez_compressed(samples / f"lsm_samples_{suffix}.npz", (rng.random((no, 1, 24, 40)) < 0.7).astype(np.float32))
        np.savez_compressed(samples / "ens_products_repeated_n_4.npz", mean=np.zeros((24, 40), np.float32))   # invisible to evaluate
    subprocess.run([sys.executable, "-m", "sbgm_danra_amd.cli.main_app", "--config_path", str(cfg_path), "--mode", "evaluate"],
                   cwd=ROOT, check=True, capture_output=True, text=True, timeout=300)
    stats = tmp_path / f"ev_{tag}" / name / "statistics"
    out = {label: (json.load(open(stats / f"{label}_metrics.json")), dict(np.load(stats / f"{label}_fields.npz")))
           for label in ("multiple", "repeated")}
    return out, samples


def test_evaluate_mode_with_and_without_the_section(tmp_path, monkeypatch):
    with_s, samples = _evaluate(tmp_path, monkeypatch, "with", PRODUCTS)
    without, _ = _evaluate(tmp_path, monkeypatch, "without", None)
    for label in ("multiple", "repeated"):
        met0, fld0 = without[label]
        assert set(met0) == BASE_METRICS and set(fld0) == BASE_FIELDS
    met, fld = with_s["multiple"]                                               # products are for `repeated` only
    assert set(met) == BASE_METRICS and set(fld) == BASE_FIELDS
    met, fld = with_s["repeated"]
    met0, fld0 = without["repeated"]
    assert set(met) == BASE_METRICS | {"product_stats"} and set(fld) == BASE_FIELDS | {f"products_{k}" for k in MAPS}
    assert json.dumps({k: met[k] for k in BASE_METRICS}, sort_keys=True) == json.dumps(met0, sort_keys=True)
    for k in BASE_FIELDS:
        np.testing.assert_array_equal(fld[k], fld0[k], err_msg=k)
    gen = np.load(samples / "gen_samples_repeated_n_4.npz")["arr_0"][:, 0]
    obs = np.load(samples / "eval_samples_repeated_n_4.npz")["arr_0"][0, 0]
    lsm = np.load(samples / "lsm_samples_repeated_n_4.npz")["arr_0"][0, 0] > 0.5
    r = V.ensemble_products(torch.from_numpy(gen).to(DEV), PRODUCTS["quantiles"], PRODUCTS["thresholds"], mask=torch.from_numpy(lsm).to(DEV))
    for k in MAPS:
        np.testing.assert_array_equal(fld[f"products_{k}"].view(np.int32), r[k].cpu().numpy().view(np.int32), err_msg=k)
    ps = met["product_stats"]
    assert ps["quantile_levels"] == PRODUCTS["quantiles"] and ps["thresholds"] == PRODUCTS["thresholds"]
    assert ps["M"] == 4 and ps["count"] == int(r["count"]) and isinstance(ps["definition"], str)
    assert 0 < ps["count"] < 24 * 40                                            # the mask and the NaN members both bite
    assert ps["coverage_nominal"] == [(q * 3 + 1) / 5 for q in PRODUCTS["quantiles"]]
    qmaps = r["quantiles"].cpu().numpy()
    valid = ~np.isnan(qmaps[0]) & ~np.isnan(obs)
    with np.errstate(invalid="ignore"):
        want = [float(((obs <= qm) & valid).sum()) / float(valid.sum()) for qm in qmaps]
    assert ps["coverage"] == want and want[0] < want[-1]
