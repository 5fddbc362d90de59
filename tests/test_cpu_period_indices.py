"""CPU suite for the period climate indices (verification.period_indices; csrc/verify_periods.hip): the
symbols and the ABI version, calendar.periods_from_dates, the evaluation.period_indices section and its place in evaluate mode,
the wrapper's argument checks (reachable without a device), and the numpy restatement tests/period_indices_ref.py against
hand-computed tiny cases, the two that define the semantics among them."""
import os

import numpy as np
import pytest
import torch
import yaml

import period_indices_ref as PR
from sbgm_danra_amd import _native as N
from sbgm_danra_amd import calendar as cal
from sbgm_danra_amd import verification as V
from sbgm_danra_amd._native import NativeError
from sbgm_danra_amd.config_loader import load_config, to_config
from sbgm_danra_amd.evaluate_sbgm import evaluation as E
from sbgm_danra_amd.evaluate_sbgm import evaluation_main as EM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "sbgm_danra_amd", "config", "default_config.yaml")
f32 = np.float32
nan = float("nan")


def test_symbols_and_abi_version():
    header = open(os.path.join(ROOT, "include", "sbgm_hip.h")).read()
    for sym in ("sbgm_period_indices_workspace_bytes", "sbgm_period_indices"):
        assert sym in N.SIGNATURES and f"{sym}(" in header, sym
    for name, value in (("SBGM_PERIOD_MAX_WINDOWS", 4), ("SBGM_PERIOD_MAX_WINDOW", 32), ("SBGM_PERIOD_MAX_THRESHOLDS", 8),
                        ("SBGM_PERIOD_MAX_PERIODS", 256), ("SBGM_PERIOD_MAX_MEMBERS", 4095)):
        assert f"#define {name} {value}\n" in header, name
    assert (V.MAX_PERIOD_WINDOWS, V.MAX_PERIOD_WINDOW, V.MAX_PERIOD_THRESHOLDS, V.MAX_PERIODS) == (4, 32, 8, 256) == (
        4, 32, 8, cal.MAX_PERIODS)
    assert V.MAX_PERIOD_MEMBERS == 4095 == V.MAX_SERIES_MEMBERS              # the member limit of the series scores
    lib = N.lib()
    assert lib.sbgm_abi_version() == N.ABI_VERSION >= 20
    assert "verify_periods.hip" in open(os.path.join(ROOT, "sbgm_danra_amd", "csrc", "Makefile")).read()
    # the workspace query answers 0 for what the call would reject
    q = lib.sbgm_period_indices_workspace_bytes
    assert q(365, 1, 16, 16, 2, 2, 0) == 12 * 256 * 4 + 365 * 4
    assert q(365, 3, 16, 16, 2, 2, 10) == 4 * 10 * 256 * 8 + 12 * 256 * 4 + (365 + 10) * 4
    for bad in ((1, 1, 16, 16, 1, 0, 0), (4096, 1, 16, 16, 1, 0, 0), (10, 0, 16, 16, 1, 0, 0), (10, 1, 1, 16, 1, 0, 0),
                (10, 1, 16, 16, 0, 0, 0), (10, 1, 16, 16, 5, 0, 0), (10, 1, 16, 16, 1, 9, 0), (10, 1, 16, 16, 1, 0, 257)):
        assert q(*bad) == 0, bad


def test_the_c_entry_checks_its_arguments():
    """every check comes before the first launch, so a host buffer serves as every pointer"""
    import ctypes as C
    lib = N.lib()
    buf = (C.c_char * 64)()
    p = C.addressof(buf)

    def call(N_=10, M=1, H=16, W=16, windows=(1, 5), thresholds=(), wet=1.0, min_days=1, P=0, periods=None, ws=1 << 30, gen=p, Nm=1,
             mask=None, dstride=256, mstride=0):
        Kw, T = len(windows), len(thresholds)
        rc = lib.sbgm_period_indices(gen, mstride, dstride, p, mask, 1, N_, Nm, M, H, W, (C.c_int * max(Kw, 1))(*windows), Kw,
                                     (C.c_float * max(T, 1))(*thresholds), T, wet, min_days, None, periods, P, *([p] * 12), ws, None)
        return rc, lib.sbgm_last_error().decode()

    for kwargs, text in ((dict(gen=None), "null argument"), (dict(N_=1), "N=1 days"), (dict(N_=4096), "N=4096 days"),
                         (dict(M=0), "M=0 members"), (dict(H=1), "field size 1x16"), (dict(dstride=255), "strides"),
                         (dict(M=2, mstride=100), "strides"), (dict(mask=p, Nm=3), "mask of 3 fields"),
                         (dict(windows=()), "0 windows"), (dict(windows=(1, 2, 3, 4, 5)), "5 windows"),
                         (dict(windows=(0,)), "window 0 is 0 days"), (dict(windows=(33,)), "window 0 is 33 days"),
                         (dict(windows=(5, 1)), "distinct and ascending"), (dict(windows=(5, 5)), "distinct and ascending"),
                         (dict(thresholds=(1.0,) * 9), "9 thresholds"), (dict(thresholds=(nan,)), "threshold 0 is not finite"),
                         (dict(wet=float("inf")), "wet-day threshold"), (dict(min_days=0), "min_days=0"),
                         (dict(P=257, periods=p), "P=257 periods"), (dict(P=3), "P=3 periods"), (dict(periods=p), "P=0 periods"),
                         (dict(ws=8), "workspace of 8 bytes")):
        rc, msg = call(**kwargs)
        assert rc != 0 and msg.startswith("period_indices: ") and text in msg, (kwargs, msg)


def _dn(*dates):
    return cal.day_numbers(np.asarray([np.datetime64(d) for d in dates]))


def test_periods_from_dates():
    assert cal.PERIODS == ("year", "season_year", "month_year") and cal.GROUPINGS == ("season", "month")
    # December goes with the following January and February, named by that year
    dn = _dn("2001-11-30", "2001-12-01", "2001-12-31", "2002-01-01", "2002-02-28", "2002-03-01", "2002-12-01")
    ids, names = cal.periods_from_dates(dn, "season_year")
    assert ids == [0, 1, 1, 1, 1, 2, 3] and names == ["2001-SON", "2002-DJF", "2002-MAM", "2003-DJF"]
    ids, names = cal.periods_from_dates(dn, "year")
    assert ids == [0, 0, 0, 1, 1, 1, 1] and names == ["2001", "2002"]
    ids, names = cal.periods_from_dates(dn, "month_year")
    assert ids == [0, 1, 1, 2, 3, 4, 5] and names == ["2001-11", "2001-12", "2002-01", "2002-02", "2002-03", "2002-12"]
    # a leap year: 366 days, 29 February in 2020-02 and in 2020-DJF
    dn = cal.day_numbers(np.datetime64("2020-01-01") + np.arange(366 + 365))
    ids, names = cal.periods_from_dates(dn, "year")
    assert names == ["2020", "2021"] and ids.count(0) == 366 and ids.count(1) == 365
    ids, names = cal.periods_from_dates(dn, "month_year")
    assert len(names) == 24 and names[1] == "2020-02" and ids.count(1) == 29 and ids.count(13) == 28
    ids, names = cal.periods_from_dates(dn, "season_year")
    assert names[0] == "2020-DJF" and ids.count(0) == 31 + 29 and names[4] == "2021-DJF" and ids.count(4) == 31 + 31 + 28
    assert names[-1] == "2022-DJF" and ids.count(8) == 31
    # a file starting mid-year with a hole of a whole year: ids count from the first period present, none for an absent one
    dn = np.concatenate([cal.day_numbers(np.datetime64("2001-07-15") + np.arange(200)), cal.day_numbers(np.datetime64("2003-03-01") + np.arange(5))])
    ids, names = cal.periods_from_dates(dn, "year")
    assert names == ["2001", "2002", "2003"] and ids[0] == 0 and ids[-1] == 2 and ids.count(0) == 170
    dn = np.concatenate([dn[:3], dn[-2:]])
    assert cal.periods_from_dates(dn, "year") == ([0, 0, 0, 1, 1], ["2001", "2003"])
    assert cal.periods_from_dates(dn, "month_year") == ([0, 0, 0, 1, 1], ["2001-07", "2003-03"])
    # 257 periods: the error says how many; 256 is fine
    months = cal.day_numbers(np.arange(np.datetime64("2000-01"), np.datetime64("2021-06"), dtype="datetime64[M]").astype("datetime64[D]"))
    assert len(months) == 257
    with pytest.raises(ValueError, match="257 periods"):
        cal.periods_from_dates(months, "month_year")
    assert len(cal.periods_from_dates(months[:256], "month_year")[1]) == 256
    assert len(cal.periods_from_dates(months, "year")[1]) == 22
    with pytest.raises(ValueError, match="periods"):
        cal.periods_from_dates(months, "season")


def test_period_section_parsing():
    sec = lambda s: E.period_indices_config(to_config({"evaluation": {"period_indices": s}}))   # noqa: E731
    assert E.period_indices_config(to_config({"evaluation": {}})) is None
    assert sec({}) == ([1, 5], [], 1.0, None, 1, None)
    assert sec({"windows": [1, 5], "thresholds": [10.0, 20.0], "wet": 1.0, "periods": "year", "min_days": 1, "calendar": None}) == (
        [1, 5], [10.0, 20.0], 1.0, "year", 1, None)
    assert sec({"windows": [2, 3, 5, 32], "thresholds": [1] * 8, "wet": 0, "periods": [-1, 0, 255], "min_days": 300, "calendar": False}) == (
        [2, 3, 5, 32], [1.0] * 8, 0.0, [-1, 0, 255], 300, False)
    assert sec({"periods": "ids.npy", "calendar": True})[3:] == ("ids.npy", 1, True)
    for p in cal.PERIODS:
        assert sec({"periods": p})[3] == p
    key = "evaluation.period_indices"
    for broken, match in (({"window": [1]}, "'window'"), ({"groups": "season"}, "'groups'"), ({"windows": 5}, "windows"),
                          ({"windows": []}, "windows"), ({"windows": [0]}, "windows"), ({"windows": [33]}, "windows"),
                          ({"windows": [1, 2, 3, 4, 5]}, "windows"), ({"windows": [5, 1]}, "windows"), ({"windows": [5, 5]}, "windows"),
                          ({"windows": [1.5]}, "windows"), ({"windows": [True]}, "windows"), ({"thresholds": 10.0}, "thresholds"),
                          ({"thresholds": [1.0] * 9}, "thresholds"), ({"thresholds": [nan]}, "thresholds"), ({"thresholds": ["10"]}, "thresholds"),
                          ({"wet": "1"}, "wet"), ({"wet": nan}, "wet"), ({"wet": True}, "wet"), ({"periods": "season"}, "periods"),
                          ({"periods": "month"}, "periods"), ({"periods": "ids.txt"}, "periods"), ({"periods": [0, 256]}, "periods"),
                          ({"periods": [0, -2]}, "periods"), ({"periods": [0.5]}, "periods"), ({"periods": []}, "periods"),
                          ({"periods": 3}, "periods"), ({"min_days": 0}, "min_days"), ({"min_days": 1.5}, "min_days"),
                          ({"min_days": True}, "min_days"), ({"calendar": 1}, "calendar"), ({"calendar": "yes"}, "calendar")):
        with pytest.raises(ValueError, match=f"{key}.*{match}"):
            sec(broken)
    with pytest.raises(ValueError, match=key):
        sec([1, 5])
    # the climate section still rejects the new keys: this is a section of its own
    with pytest.raises(ValueError, match="climate_indices"):
        E.climate_indices_config(to_config({"evaluation": {"climate_indices": {"windows": [1, 5]}}}))


def test_unit_statistics_with_and_without_the_section():
    assert E.period_indices_config(load_config(CFG)) is None                  # the shipped defaults do not opt in
    assert "period_indices" not in yaml.safe_load(open(CFG))["evaluation"]
    assert EM.STATISTICS["period_stats"] == ("period_statistics", E.period_indices_config, False)
    assert "period_stats" in EM.TIME_AXIS_STATISTICS and EM.PERIOD_METHODS == {"period_stats": "period_statistics"}
    base = ["pixel_stats", "spatial_stats"]
    c = to_config({"evaluation": {"period_indices": {"periods": "year"}}})
    assert EM.unit_statistics(c, "multiple") == EM.unit_statistics(c, "series") == base + ["period_stats"]
    assert EM.unit_statistics(c, "single") == EM.unit_statistics(c, "repeated") == base
    both = to_config({"evaluation": {"period_indices": {}, "climate_indices": {"quantiles": [0.5]}, "series_scores": {"thresholds": [1.0]}}})
    assert EM.unit_statistics(both, "series") == base + ["climate_stats", "period_stats", "series_ensemble_stats"]
    none = to_config({"evaluation": {"climate_indices": {"quantiles": [0.5]}}})
    for t in E.GEN_TYPES:
        assert "period_stats" not in EM.unit_statistics(none, t)
    with pytest.raises(ValueError, match="period_stats"):                      # and it is no eval_stat_methods name
        EM.eval_stat_methods(to_config({"evaluation": {"eval_stat_methods": ["period_stats"]}}))
    with pytest.raises(ValueError, match="period_indices.windows"):            # validated before any file is read
        EM.unit_statistics(to_config({"evaluation": {"period_indices": {"windows": [0]}}}), "series")


def _write_series(tmp_path, monkeypatch, section, dates):
    for k in ("DATA_DIR", "CKPT_DIR", "SAMPLE_DIR", "STATS_LOAD_DIR"):
        monkeypatch.setenv(k, str(tmp_path / k.lower()))
    monkeypatch.setenv("SLURM_CPUS_PER_TASK", "2")
    raw = yaml.safe_load(open(CFG))
    if section is not None:
        raw["evaluation"]["period_indices"] = section
    p = tmp_path / "series.yaml"
    p.write_text(yaml.safe_dump(raw))
    cfg = load_config(str(p))
    from sbgm_danra_amd.utils import get_model_string
    d = os.path.join(cfg.paths.sample_dir, "generation", get_model_string(cfg), "generated_samples")
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(1)
    np.savez_compressed(os.path.join(d, "gen_samples_series_n_6.npz"), rng.random((6, 2, 4, 5)).astype(f32))
    np.savez_compressed(os.path.join(d, "eval_samples_series_n_6.npz"), rng.random((6, 4, 5)).astype(f32))
    if dates:
        np.savez(os.path.join(d, "series_index_series_n_6.npz"), dates=np.int64(11000) + np.arange(6))
    np.savez_compressed(os.path.join(d, "gen_samples_repeated_n_3.npz"), np.zeros((3, 4, 5), f32))
    np.savez_compressed(os.path.join(d, "eval_samples_repeated_n_3.npz"), np.zeros((1, 4, 5), f32))
    return cfg


def test_period_statistics_errors_on_the_host(tmp_path, monkeypatch):
    cpu = torch.device("cpu")
    cfg = _write_series(tmp_path, monkeypatch, {"periods": "year"}, dates=False)
    ev = E.Evaluation(cfg, "series", None, device=cpu)
    with pytest.raises(ValueError, match="'year' needs the dates"):           # a named grouping without dates
        ev.period_statistics()
    with pytest.raises(ValueError, match="calendar is true"):
        ev.period_statistics(periods=[0] * 6, calendar_aware=True)
    with pytest.raises(ValueError, match="holds 4 ids.*6 days"):
        ev.period_statistics(periods=[0, 0, 1, 1])
    with pytest.raises(ValueError, match="integer id"):
        ev.period_statistics(periods=np.zeros(6))
    with pytest.raises(ValueError, match="one truth per day"):
        E.Evaluation(cfg, "repeated", 3, device=cpu).period_statistics()
    with pytest.raises(NativeError):                                           # arguments fine; the fields are on the CPU
        ev.period_statistics(periods=[0, 0, 0, 1, 1, 1])
    cfg = _write_series(tmp_path, monkeypatch, {"periods": "month_year"}, dates=True)
    ev = E.Evaluation(cfg, "series", None, device=cpu)
    with pytest.raises(NativeError):                                           # with dates the named grouping gets to the device call
        ev.period_statistics()
    assert "period_indices" not in ev.metrics
    ev.cfg = load_config(CFG)
    with pytest.raises(ValueError, match="period_indices section"):
        ev.period_statistics()


def test_wrapper_checks_before_the_device():
    g, o = torch.zeros(10, 4, 5), torch.zeros(10, 4, 5)                       # CPU tensors: a passing check ends in NativeError
    with pytest.raises(NativeError):
        V.period_indices(g, o)
    with pytest.raises(NativeError):
        V.period_indices(torch.zeros(3, 10, 4, 5), o, windows=(2, 3, 5, 32), thresholds=[1.0] * 8, periods=[-1] * 5 + [255] * 5, min_days=40)
    for kwargs, match in ((dict(windows=(0,)), "windows"), (dict(windows=(33,)), "windows"), (dict(windows=(1, 2, 3, 4, 5)), "5 windows"),
                          (dict(windows=()), "0 windows"), (dict(windows=(5, 1)), "ascending"), (dict(windows=(5, 5)), "ascending"),
                          (dict(windows=(1.5,)), "windows"), (dict(thresholds=[1.0] * 9), "9 thresholds"),
                          (dict(thresholds=[nan]), "finite"), (dict(thresholds=[1e39]), "finite"), (dict(wet=nan), "wet"),
                          (dict(wet="1"), "wet"), (dict(periods=[0] * 9 + [256]), "-1..255"), (dict(periods=[0] * 9 + [-2]), "-1..255"),
                          (dict(periods=[0] * 9), "9 period ids for N=10"), (dict(periods=[0.5] * 10), "integers"),
                          (dict(periods=torch.zeros(10)), "integer tensor"), (dict(min_days=0), "min_days"),
                          (dict(min_days=1.5), "min_days"), (dict(min_days=True), "min_days"),
                          (dict(day_numbers=[0, 1, 2, 3, 4, 5, 6, 7, 9, 9]), "increasing"), (dict(day_numbers=[0, 1]), "day numbers"),
                          (dict(mask=torch.zeros(3, 4, 5)), "mask"), (dict(mask=torch.zeros(4, 5, dtype=torch.int32)), "mask")):
        with pytest.raises((ValueError, TypeError), match=match):
            V.period_indices(g, o, **kwargs)
    for gen, obs, match in ((torch.zeros(4, 5), o, "gen"), (g, torch.zeros(9, 4, 5), "obs"), (g.double(), o, "float32"),
                            (g, o.half(), "float32"), (torch.zeros(1, 4, 5), torch.zeros(1, 4, 5), "N=1 days"),
                            (torch.zeros(2, 1, 5), torch.zeros(2, 1, 5), "field size"), (torch.zeros(2, 9, 4, 5), o, "obs")):
        with pytest.raises((ValueError, TypeError), match=match):
            V.period_indices(gen, obs)


def _col(values):
    """a [N, 2, 2] record whose four pixels hold the same column"""
    return np.broadcast_to(np.asarray(values, f32)[:, None, None], (len(values), 2, 2)).copy()


def test_restatement_december_window_belongs_to_january():
    """29, 30, 31 December and 1, 2 January: the 5-day window ends on 2 January, so it is the January year's; December's year
    has no 5-day window of its own here, and its Rx1day is its own days'"""
    dn = _dn("2001-12-29", "2001-12-30", "2001-12-31", "2002-01-01", "2002-01-02")
    ids, names = cal.periods_from_dates(dn, "year")
    assert ids == [0, 0, 0, 1, 1] and names == ["2001", "2002"]
    x = _col([10, 20, 30, 1, 2])
    r = PR.period_indices(x, x, (1, 3, 5), [10.0], 1.0, None, dn, ids, 1)
    assert r["gen_rx"][:, 0, 0].tolist() == [30.0, 60.0, 63.0] and (r["days"] == 5).all()
    assert r["period_gen_rx"][0, :, 0, 0].tolist()[:2] == [30.0, 60.0] and np.isnan(r["period_gen_rx"][0, 2]).all()
    assert r["period_gen_rx"][1, :, 0, 0].tolist() == [2.0, 51.0, 63.0]       # 30 + 31 Dec + 1 Jan = 51 ends on 1 January
    assert r["period_days"][:, 0, 0].tolist() == [3, 2]
    assert r["period_gen_count"][:, 0, 0, 0].tolist() == [3, 0] and r["gen_count"][0, 0, 0] == 3
    assert r["period_gen_prcptot"][:, 0, 0].tolist() == [60.0, 3.0] and r["gen_prcptot"][0, 0] == 63.0
    # across the two years: Rx5day counts 2002 only; Rx1day both
    assert r["gen_period_n_rx"][:, 0, 0].tolist() == [2, 2, 1]
    assert r["gen_period_mean_rx"][:, 0, 0].tolist() == [16.0, 55.5, 63.0]
    np.testing.assert_array_equal(r["gen_period_std_rx"][:2, 0, 0], np.asarray([np.sqrt(392.0), np.sqrt(40.5)], f32))
    assert np.isnan(r["gen_period_std_rx"][2]).all()
    assert r["gen_period_mean_prcptot"][0, 0] == 31.5 and r["gen_period_mean_count"][0, 0, 0] == 1.5
    # with min_days = 3 the year 2002 (2 days) no longer counts
    r3 = PR.period_indices(x, x, (1, 3, 5), [10.0], 1.0, None, dn, ids, 3)
    assert r3["gen_period_n_rx"][:, 0, 0].tolist() == [1, 1, 0] and np.isnan(r3["gen_period_mean_rx"][2]).all()
    assert r3["gen_period_mean_rx"][0, 0, 0] == 30.0 and np.isnan(r3["gen_period_std_rx"]).all()
    np.testing.assert_array_equal(r3["period_gen_rx"], r["period_gen_rx"])     # min_days touches nothing else


def test_restatement_a_broken_link_removes_the_window():
    x = _col([1, 2, 3, 4, 5, 6])
    whole = PR.period_indices(x, x, (1, 5), [], 1.0, None, [0, 1, 2, 3, 4, 5], None, 1)
    assert whole["gen_rx"][:, 0, 0].tolist() == [6.0, 20.0] and set(whole) == {"days", "gen_rx", "obs_rx", "gen_count", "obs_count",
                                                                              "gen_prcptot", "obs_prcptot"}
    assert whole["gen_count"].shape == (0, 2, 2)
    broken = PR.period_indices(x, x, (1, 5), [], 1.0, None, [0, 1, 2, 4, 5, 6], None, 1)      # a gap after the third day
    assert broken["gen_rx"][0, 0, 0] == 6.0 and np.isnan(broken["gen_rx"][1]).all() and (broken["days"] == 6).all()
    assert broken["gen_prcptot"][0, 0] == 21.0                                # the link counts nowhere else
    tail = PR.period_indices(x, x, (1, 5), [], 1.0, None, [0, 2, 3, 4, 5, 6], None, 1)        # five linked days remain
    assert tail["gen_rx"][:, 0, 0].tolist() == [6.0, 20.0]
    # an invalid day does the same, on one pixel only, and for both sides: validity is paired over everything
    g = np.stack([x, x])                                                       # two members
    g[1, 2, 0, 1] = np.nan
    r = PR.period_indices(g, x, (1, 5), [2.0], 1.0)
    assert r["gen_rx"].shape == (2, 2, 2, 2) and r["obs_rx"].shape == (2, 2, 2)
    assert r["days"].tolist() == [[6, 5], [6, 6]]
    assert np.isnan(r["gen_rx"][:, 1, 0, 1]).all() and np.isnan(r["obs_rx"][1, 0, 1]) and r["obs_rx"][1, 1, 1] == 20.0
    assert r["obs_count"][0].tolist() == [[5, 4], [5, 5]] and r["obs_prcptot"][0, 1] == 18.0


def test_restatement_rules_for_empty_and_dry_pixels_and_unused_ids():
    x = _col([0.5, 0.25, 0.0, 0.5])
    x[:, 1, 1] = np.nan
    ids = [3, 3, -1, 0]                                                        # ids 1 and 2 are unused, day 2 is in no period
    r = PR.period_indices(x, x, (1, 2), [0.5], 1.0, None, None, ids, 1)
    assert r["days"].tolist() == [[4, 4], [4, 0]]
    assert r["gen_prcptot"][0, 0] == 0.0 and np.isnan(r["gen_prcptot"][1, 1])  # valid and never wet: 0; no valid day: NaN
    assert r["period_days"][:, 0, 0].tolist() == [1, 0, 0, 2] and r["period_days"].shape == (4, 2, 2)
    assert r["period_gen_count"][:, 0, 0, 0].tolist() == [1, 0, 0, 1]
    assert np.isnan(r["period_gen_rx"][1:3]).all() and np.isnan(r["period_gen_prcptot"][1:3]).all()
    # period 0's 2-day window ends on its only day and reaches back into the day of id -1
    assert r["period_gen_rx"][0, :, 0, 0].tolist() == [0.5, 0.5] and r["period_gen_rx"][3, :, 0, 0].tolist() == [0.5, 0.75]
    assert r["gen_period_n_rx"][:, 0, 0].tolist() == [2, 2] and r["gen_period_n_rx"][:, 1, 1].tolist() == [0, 0]
    assert r["gen_period_n_count"][0, 0, 0] == 2 and r["gen_period_n_count"][0, 1, 1] == 0    # a period without days counts nowhere
    assert np.isnan(r["gen_period_mean_count"][0, 1, 1]) and r["gen_period_mean_prcptot"][0, 0] == 0.0
    # recurring ids: the second visit goes on where the first ended
    y = _col([1, 2, 4, 8, 16, 32])
    r = PR.period_indices(y, y, (1, 2), [], 1.0, None, None, [0, 1, 0, 1, 0, 1], 1)
    assert r["period_gen_prcptot"][:, 0, 0].tolist() == [21.0, 42.0] and r["period_gen_rx"][:, 1, 0, 0].tolist() == [24.0, 48.0]
    # the sum is taken oldest day first from +0.0: the order shows where a sliding form would lose it
    z = _col([-1e30, 3, 5, 7])
    r = PR.period_indices(z, z, (1, 2, 3), [], -1e38)
    assert r["gen_rx"][:, 0, 0].tolist() == [7.0, 12.0, 15.0]
    assert np.signbit(PR.period_indices(_col([-0.0, -0.0]), _col([-0.0, -0.0]), (1, 2))["gen_rx"]).sum() == 0     # -0 is impossible
