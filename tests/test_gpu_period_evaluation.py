"""GPU suite for the period climate indices in evaluate mode: a small dated 'series' (40 days with a hole in the dates, 2
members, 16 x 16) in the files a series generation writes (gen_samples / eval_samples / series_index with `dates`), evaluated
through evaluation_main with an evaluation.period_indices section and `periods: month_year`.  series_periods.npz equals a
direct verification.period_indices call on the stacked members, the metrics entry is there, and without the section the file
list and series_metrics.json are what they were."""
import json
import os

import numpy as np
import pytest
import torch
import yaml

from sbgm_danra_amd import calendar as cal
from sbgm_danra_amd import verification as V

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "sbgm_danra_amd", "config", "default_config.yaml")
f32 = np.float32
D, M, H, W = 40, 2, 16, 16
# 20 January .. 12 February 2021 and, after a hole of five days, 18 February .. 5 March: three months, one broken link
DATES = np.concatenate([np.datetime64("2021-01-20") + np.arange(24), np.datetime64("2021-02-18") + np.arange(16)])
SECTION = {"windows": [1, 5], "thresholds": [1.0, 4.0], "wet": 0.5, "periods": "month_year", "min_days": 5, "calendar": None}


def _series(tmp_path, monkeypatch, tag, section):
    from sbgm_danra_amd.config_loader import load_config
    from sbgm_danra_amd.utils import get_model_string
    for k in ("DATA_DIR", "CKPT_DIR", "STATS_LOAD_DIR"):
        monkeypatch.setenv(k, str(tmp_path / k.lower()))
    monkeypatch.setenv("SAMPLE_DIR", str(tmp_path / "samples"))
    monkeypatch.setenv("SLURM_CPUS_PER_TASK", "2")
    raw = yaml.safe_load(open(CFG))
    raw["paths"]["evaluation_dir"] = str(tmp_path / f"ev_{tag}")
    raw["evaluation"].update(eval_gen_type=["series"], eval_stat_methods=["daily_stats"])
    if section is not None:
        raw["evaluation"]["period_indices"] = section
    p = tmp_path / f"run_{tag}.yaml"
    p.write_text(yaml.safe_dump(raw))
    cfg = load_config(str(p))
    d = os.path.join(cfg.paths.sample_dir, "generation", get_model_string(cfg), "generated_samples")
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(5)
    gen = np.maximum(f32(3.0) * rng.standard_normal((D, M, H, W)).astype(f32) - f32(1.0), f32(0.0))
    truth = np.maximum(f32(3.0) * rng.standard_normal((D, H, W)).astype(f32) - f32(1.0), f32(0.0))
    gen[7, 1, 3, 4], truth[36, 5, 6] = np.nan, np.nan                      # 27 January in member 1; 2 March in the truth
    np.savez_compressed(os.path.join(d, f"gen_samples_series_n_{D}.npz"), gen)
    np.savez_compressed(os.path.join(d, f"eval_samples_series_n_{D}.npz"), truth)
    np.savez(os.path.join(d, f"series_index_series_n_{D}.npz"), dates=cal.day_numbers(DATES))
    return cfg, gen, truth


def test_evaluate_mode_writes_the_period_file_and_the_metrics_entry(tmp_path, monkeypatch):
    from sbgm_danra_amd.evaluate_sbgm.evaluation import statistics_dir
    from sbgm_danra_amd.evaluate_sbgm.evaluation_main import evaluation_main
    cfg, gen, truth = _series(tmp_path, monkeypatch, "with", SECTION)
    out = evaluation_main(cfg)
    stats = statistics_dir(cfg)
    assert {"series_fields.npz", "series_metrics.json", "series_periods.npz"} <= set(os.listdir(stats))
    f = dict(np.load(os.path.join(stats, "series_periods.npz")))
    dn = cal.day_numbers(DATES)
    ids, names = cal.periods_from_dates(dn, "month_year")
    assert names == ["2021-01", "2021-02", "2021-03"] and [ids.count(g) for g in range(3)] == [12, 23, 5]
    assert f["dates"].tolist() == dn.tolist() and f["periods"].tolist() == ids and f["period_names"].tolist() == names
    assert f["windows"].tolist() == [1, 5] and f["thresholds"].tolist() == [1.0, 4.0] and float(f["wet"]) == 0.5
    assert int(f["members"]) == M and int(f["min_days"]) == 5
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()              # noqa: E731
    r = V.period_indices(dev(gen.transpose(1, 0, 2, 3)), dev(truth), (1, 5), [1.0, 4.0], 0.5, day_numbers=dn, periods=ids, min_days=5)
    assert set(r) <= set(f) and r["gen_rx"].shape == (M, 2, H, W) and r["period_gen_count"].shape == (M, 3, 2, H, W)
    for k, v in r.items():
        a, b = f[k], v.cpu().numpy()
        assert a.shape == b.shape and a.dtype == b.dtype, k
        np.testing.assert_array_equal(a.view(np.int32), b.view(np.int32), err_msg=k)
    # the hole is known: no 5-day window ends on 18 .. 21 February, so February's Rx5day differs from the uncalendared call's somewhere
    plain = V.period_indices(dev(gen.transpose(1, 0, 2, 3)), dev(truth), (1, 5), [1.0, 4.0], 0.5, periods=ids, min_days=5)
    assert not torch.equal(plain["period_obs_rx"][1, 1], r["period_obs_rx"][1, 1])
    assert torch.equal(plain["period_obs_rx"][:, 0], r["period_obs_rx"][:, 0])
    assert f["days"][3, 4] == D - 1 and f["days"][5, 6] == D - 1 and f["period_days"][2, 5, 6] == 4      # below min_days there
    assert f["obs_period_n_prcptot"][5, 6] == 2 and f["obs_period_n_prcptot"][0, 0] == 3
    met = json.load(open(os.path.join(stats, "series_metrics.json")))
    pi = met["period_indices"]
    assert set(out["series"]["period_indices"]) == set(pi)
    assert list(pi["indices"]) == ["rx_1", "rx_5", "count_1", "count_4", "prcptot"] and pi["period_names"] == names
    assert pi["calendar"] is True and pi["n_links_broken"] == 1 and pi["n_periods"] == 3 and pi["members"] == M and pi["n_days"] == D
    assert isinstance(pi["definition"], str) and "Rx5day" in pi["definition"]
    for entry in pi["indices"].values():
        assert list(entry) == ["record", "period_mean", "period_std"]
        for row in entry.values():
            assert len(row["per_member"]) == M and row["pixels"] == [H * W] * M
            assert set(row["bias"]) == {"mean", "min", "max"} and np.isfinite(row["rmse"]["mean"])
    want = float(np.mean(f["gen_period_mean_rx"][1, 1].astype(np.float64)) - np.mean(f["obs_period_mean_rx"][1].astype(np.float64)))
    assert abs(pi["indices"]["rx_5"]["period_mean"]["per_member"][1]["bias"] - want) < 1e-9


def test_without_the_section_nothing_changes(tmp_path, monkeypatch):
    from sbgm_danra_amd.evaluate_sbgm.evaluation import statistics_dir
    from sbgm_danra_amd.evaluate_sbgm.evaluation_main import evaluation_main
    cfg, _, _ = _series(tmp_path, monkeypatch, "without", None)
    evaluation_main(cfg)
    stats = statistics_dir(cfg)
    files = sorted(os.listdir(stats))
    assert "series_periods.npz" not in files and {"series_fields.npz", "series_metrics.json"} <= set(files)
    bare = json.load(open(os.path.join(stats, "series_metrics.json")))
    assert "period_indices" not in bare
    cfg, _, _ = _series(tmp_path, monkeypatch, "with", SECTION)
    evaluation_main(cfg)
    assert sorted(set(os.listdir(statistics_dir(cfg))) - {"series_periods.npz"}) == files
    met = json.load(open(os.path.join(statistics_dir(cfg), "series_metrics.json")))
    met.pop("period_indices")
    assert json.dumps(met, sort_keys=True) == json.dumps(bare, sort_keys=True)          # NaN spelled the same way in both
    a, b = (dict(np.load(os.path.join(statistics_dir(c), "series_fields.npz"))) for c in (cfg, _series(tmp_path, monkeypatch, "without", None)[0]))
    assert set(a) == set(b) and all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)
