"""CPU suite for the calendar of a series: the `calendar` module (day numbers, civil dates, links, groups, the origin, the noise
rows of a date), the restatement by composition tests/climate_calendar_ref.py against tests/climate_ref.py, the new C ABI
entries, the argument checks of `verification.climate_indices` that fire before the device, and how the configuration keys
`evaluation.climate_indices.calendar` / `.groups`, `evaluation.series_scores.groups` and `evaluation.series.calendar_origin` parse."""
import datetime
import os

import numpy as np
import pytest
import torch

import climate_calendar_ref as CR
import climate_ref as R
from sbgm_danra_amd import _native as N
from sbgm_danra_amd import calendar as cal
from sbgm_danra_amd import verification as V
from sbgm_danra_amd._native import NativeError
from sbgm_danra_amd.config_loader import to_config
from sbgm_danra_amd.evaluate_sbgm import evaluation as E
from sbgm_danra_amd.evaluate_sbgm import generation as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
D = lambda s: int(np.datetime64(s, "D").astype(np.int64))       # noqa: E731


# ---- the calendar module --------------------------------------------------------------------------------------------------------

def test_day_numbers_and_civil_dates():
    dates = np.array(["2020-02-28", "2020-02-29", "2020-03-01", "2021-03-01"], dtype="datetime64[D]")
    dn = cal.day_numbers(dates)
    assert dn.dtype == np.int64 and dn.tolist() == [18320, 18321, 18322, 18687] and cal.day_numbers(dn).tolist() == dn.tolist()
    assert cal.day_numbers(np.array([0], np.int32)).tolist() == [0] and cal.day_numbers(dates.astype("datetime64[s]")).tolist() == dn.tolist()
    y, m, d = cal.civil(dn)
    assert (y.tolist(), m.tolist(), d.tolist()) == ([2020, 2020, 2020, 2021], [2, 2, 3, 3], [28, 29, 1, 1])
    assert [x.tolist() for x in cal.civil(np.array([0, -1, 11016]))] == [[1970, 1969, 2000], [1, 12, 2], [1, 31, 29]]
    assert cal.links(dn).tolist() == [False, True, True, False] and cal.links(dn[:1]).tolist() == [False]
    for bad in ([3, 3], [5, 4], np.array([[1, 2]]), np.array([1.0, 2.0]), np.array(["2020-01-01"]), np.array([True, False]),
                np.array(["2020-01-02", "2020-01-01"], dtype="datetime64[D]"), np.array(["NaT"], dtype="datetime64[D]")):
        with pytest.raises(ValueError, match="dates"):
            cal.day_numbers(bad)


def test_groups_from_dates():
    days = ["2019-12-01", "2020-02-29", "2020-03-01", "2020-05-31", "2020-06-01", "2020-08-31", "2020-09-01", "2020-11-30", "2020-12-01"]
    dn = cal.day_numbers(np.array(days, dtype="datetime64[D]"))
    ids, names = cal.groups_from_dates(dn, "season")
    assert ids == [0, 0, 1, 1, 2, 2, 3, 3, 0] and names == ["DJF", "MAM", "JJA", "SON"] and all(type(g) is int for g in ids)
    ids, names = cal.groups_from_dates(dn, "month")
    assert ids == [11, 1, 2, 4, 5, 7, 8, 10, 11] and len(names) == 12 and names[0] == "Jan" and names[11] == "Dec"
    year = cal.groups_from_dates(D("2020-01-01") + np.arange(366), "month")[0]
    assert [year.count(g) for g in range(12)] == [31, 29, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31]
    with pytest.raises(ValueError, match="groups"):
        cal.groups_from_dates(dn, "year")


def test_origin_and_noise_rows():
    assert cal.parse_origin("2020-01-01") == D("2020-01-01") == 18262 and cal.parse_origin(7) == 7 and cal.parse_origin(np.int64(-3)) == -3
    assert cal.parse_origin(datetime.date(2020, 1, 1)) == 18262                  # what YAML makes of an unquoted date
    for bad in ("2020-1-1", "01-01-2020", "2020-13-01", "yesterday", 1.5, True, None, [1]):
        with pytest.raises(ValueError, match="calendar_origin"):
            cal.parse_origin(bad)
    dates = np.array([10, 11, 12, 15, 16])
    assert cal.series_days(dates, 10).tolist() == [0, 1, 2, 5, 6] and cal.series_days(dates, 3).tolist() == [7, 8, 9, 12, 13]
    with pytest.raises(ValueError, match="origin"):
        cal.series_days(dates, 11)
    with pytest.raises(ValueError, match="strictly increasing"):                  # a shuffled loader
        cal.series_days(np.array([10, 12, 11]), 0)
    # member m of day n is row (n + K - 1) M + m: the formula of the series with the date's day in place of the position
    assert cal.noise_rows([0, 1, 2, 5, 6], 3, 2).tolist() == [4, 5, 6, 7, 8, 9, 14, 15, 16, 17]
    assert cal.noise_rows(np.arange(4), 1, 1).tolist() == [0, 1, 2, 3] and cal.noise_rows([], 3, 2).tolist() == []
    assert cal.noise_rows([(2 ** 31) // 2 - 3], 3, 2).tolist() == [2 ** 31 - 2, 2 ** 31 - 1]
    for bad in (([(2 ** 31) // 2 - 2], 3, 2), ([2 ** 31], 1, 1), ([-1], 1, 1)):
        with pytest.raises(ValueError, match="noise row"):
            cal.noise_rows(*bad)


def test_tiler_takes_day_numbers_instead_of_first_day():
    from sbgm_danra_amd.tiling import FullDomainTiler
    t = FullDomainTiler.__new__(FullDomainTiler)                             # the checks fire before anything touches the device
    with pytest.raises(ValueError, match="not both"):
        t.sample_series(None, None, None, None, 2, days=2, first_day=0, day_numbers=[0, 1])
    with pytest.raises(ValueError, match="day_numbers must hold 2"):
        t.sample_series(None, None, None, None, 2, days=2, day_numbers=[0, 1, 2])
    with pytest.raises(ValueError, match="non-negative"):
        t.sample_series(None, None, None, None, 2, days=2, day_numbers=[-1, 1])
    with pytest.raises(ValueError, match="beyond int32"):
        t.sample_series(None, None, None, None, 2, days=2, members=2, temporal_noise_weights=[1.0], day_numbers=[0, 2 ** 30])


# ---- the restatement by composition ---------------------------------------------------------------------------------------------

def _small():
    rng = np.random.default_rng(8)
    gen = (rng.integers(0, 13, size=(12, 8, 8)) * 0.25).astype(f32)
    obs = (rng.integers(0, 13, size=(12, 8, 8)) * 0.25).astype(f32)
    gen[rng.random(gen.shape) < 0.05] = np.nan
    mask = (rng.random((12, 8, 8)) < 0.9).astype(np.uint8)
    return gen, obs, mask


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_restatement_without_gaps_and_with_one_group():
    gen, obs, mask = _small()
    plain = R.climate_indices(gen, obs, 1.0, [0.5], [0.9], mask)
    _same(CR.climate_indices(gen, obs, 1.0, [0.5], [0.9], mask), plain)
    _same(CR.climate_indices(gen, obs, 1.0, [0.5], [0.9], mask, day_numbers=100 + np.arange(12)), plain)
    one = CR.climate_indices(gen, obs, 1.0, [0.5], [0.9], mask, groups=np.zeros(12, int))
    _same({k: v for k, v in one.items() if not k.startswith("group_")}, plain)
    _same({k[6:]: v[0] for k, v in one.items() if k.startswith("group_")}, plain)


def test_restatement_with_gaps_and_groups():
    gen, obs, mask = _small()
    dn = np.array([0, 1, 2, 3, 9, 10, 11, 12, 13, 20, 21, 22])
    r = CR.climate_indices(gen, obs, 1.0, [0.5], [0.9], mask, day_numbers=dn)
    plain = R.climate_indices(gen, obs, 1.0, [0.5], [0.9], mask)
    ok = R.valid_days(gen, obs, mask)
    pairs = sum((ok[t] & ok[t - 1]).astype(int) for t in range(1, 12) if dn[t] == dn[t - 1] + 1)
    np.testing.assert_array_equal(r["obs_transitions"].sum(axis=0), pairs)
    assert (r["obs_transitions"].sum(axis=0) < plain["obs_transitions"].sum(axis=0)).any() and (r["gen_cwd"] <= plain["gen_cwd"]).all()
    for k in ("days", "gen_mean", "obs_wet_freq", "gen_quantiles", "obs_wet_quantiles", "gen_heavy_fraction", "obs_max"):
        np.testing.assert_array_equal(r[k], plain[k], err_msg=k)                # a link counts nowhere else
    ids = np.array([0, 0, 2, 2, 2, 0, 0, 3, 0, 2, 2, 2])                        # id 1 unused, id 3 on one day
    g = CR.climate_indices(gen, obs, 1.0, [0.5], [0.9], mask, day_numbers=dn, groups=ids)
    assert g["group_days"].shape == (4, 8, 8) and (g["group_days"][1] == 0).all() and g["group_days"][3].max() <= 1
    np.testing.assert_array_equal(g["group_days"].sum(axis=0), g["days"])
    assert np.isnan(g["group_gen_mean"][1]).all() and (g["group_gen_cwd"][1] == 0).all() and np.isnan(g["group_obs_lag1"][3]).all()
    sel = np.flatnonzero(ids == 2)                                              # days 2 3 | 4 || 9 10 11: two broken links
    a, b, m = CR.expand(gen, obs, mask, dn, sel)
    assert a.shape[0] == len(sel) + 2 and np.isnan(a[2]).all() and np.isnan(b[4]).all() and m.shape == a.shape
    _same({k[6:]: v[2] for k, v in g.items() if k.startswith("group_")}, R.climate_indices(a, b, 1.0, [0.5], [0.9], m))
    assert CR.expand(gen, obs, mask[0], dn, np.array([], int))[0].shape == (1, 8, 8)


# ---- the C ABI and the wrapper ----------------------------------------------------------------------------------------------------

def test_symbols_and_workspace():
    lib = N.lib()
    names = ("sbgm_climate_indices_calendar", "sbgm_climate_calendar_workspace_bytes")
    header = open(os.path.join(ROOT, "include", "sbgm_hip.h")).read()
    for name in names:
        assert name in N.SIGNATURES and getattr(lib, name) is not None and f"{name}(" in header
    assert lib.sbgm_abi_version() == N.ABI_VERSION >= 19 and "#define SBGM_TEMPORAL_MAX_GROUPS 16" in header
    assert V.MAX_SERIES_GROUPS == 16
    HW = 589 * 789
    # the plain query is what it was; the calendar one adds n_wet per group slab and the tables (order 2N, start G + 2, link N)
    assert lib.sbgm_climate_indices_workspace_bytes(365, 589, 789, 3, 2) == (12 + 2) * HW * 4
    assert lib.sbgm_climate_calendar_workspace_bytes(365, 589, 789, 3, 2, 0) == ((12 + 2) * HW + 3 * 365 + 2) * 4
    assert lib.sbgm_climate_calendar_workspace_bytes(365, 589, 789, 3, 2, 4) == ((12 + 10) * HW + 3 * 365 + 6) * 4
    for bad in ((1, 8, 8, 0, 0, 0), (4096, 8, 8, 0, 0, 0), (4, 1, 8, 0, 0, 0), (4, 8, 8, 9, 0, 0), (4, 8, 8, 0, 9, 0), (4, 2049, 8, 0, 0, 0),
                (4, 8, 8, 0, 0, -1), (4, 8, 8, 0, 0, 17)):
        assert lib.sbgm_climate_calendar_workspace_bytes(*bad) == 0
    assert lib.sbgm_climate_indices_calendar(*([None] * 3), 0, 4, 1, 8, 8, 1.0, None, 0, None, 0, None, None, 0, *([None] * 15), 0, None) != 0
    assert b"null" in lib.sbgm_last_error()


def test_wrapper_checks_before_the_device():
    gen, obs = torch.zeros(3, 8, 9), torch.zeros(3, 8, 9)
    bad = [dict(day_numbers=[0, 1]), dict(day_numbers=[0, 2, 2]), dict(day_numbers=[2, 1, 0]), dict(day_numbers=np.array([0.0, 1.0, 2.0])),
           dict(day_numbers=[0, 1, 2 ** 31]), dict(groups=[0, 1]), dict(groups=[0, 1, 16]), dict(groups=[0, -1, 1]), dict(groups=[0, 1.5, 1]),
           dict(groups=[True, False, True]), dict(groups=torch.zeros(3)), dict(groups=torch.zeros(3, 1, dtype=torch.int64))]
    for kw in bad:
        with pytest.raises(ValueError, match="climate_indices|dates|groups"):
            V.climate_indices(gen, obs, **kw)
    for kw in (dict(day_numbers=[5, 6, 9]), dict(groups=[0, 3, 0]), dict(day_numbers=torch.tensor([1, 2, 3]), groups=torch.tensor([1, 0, 1])),
               dict(day_numbers=np.array(["2020-02-28", "2020-02-29", "2020-03-01"], dtype="datetime64[D]"))):
        with pytest.raises(NativeError):                                         # well-formed arguments reach the device check
            V.climate_indices(gen, obs, **kw)
    with pytest.raises(ValueError, match="series_ensemble_scores"):              # the shared helper still names its caller
        V._series_groups([0, 16], 2)


# ---- the configuration ------------------------------------------------------------------------------------------------------------

def test_config_keys():
    sec = lambda s: to_config({"evaluation": {"climate_indices": s}})            # noqa: E731
    assert E.climate_calendar_config(to_config({"evaluation": {}})) == (None, None) and E.climate_calendar_config(sec({})) == (None, None)
    assert E.climate_indices_config(sec({"wet": 0.5, "calendar": True, "groups": "season"})) == (0.5, [], [])
    assert E.climate_calendar_config(sec({"calendar": False, "groups": "month"})) == (False, "month")
    assert E.climate_calendar_config(sec({"groups": [0, 1, 15]})) == (None, [0, 1, 15])
    assert E.climate_calendar_config(sec({"groups": "ids.npy"})) == (None, "ids.npy")
    for broken, key in (({"calendar": 1}, "calendar"), ({"calendar": "yes"}, "calendar"), ({"groups": "year"}, "groups"),
                        ({"groups": [0, 16]}, "groups"), ({"groups": []}, "groups"), ({"groups": [0.5]}, "groups"), ({"groups": 3}, "groups"),
                        ({"dates": [1]}, "dates"), ({"thresholds": [1.0]}, "thresholds")):
        with pytest.raises(ValueError, match=key):
            E.climate_indices_config(sec(broken))
    ss = lambda s: E.series_scores_config(to_config({"evaluation": {"series_scores": s}}))      # noqa: E731
    assert ss({"groups": "season"})[2] == "season" and ss({"groups": "month"})[2] == "month" and ss({"groups": "g.npy"})[2] == "g.npy"
    assert ss({"groups": [0, 1]})[2] == [0, 1] and ss({})[2] is None
    for broken in ("year", "seasons", [0, 16]):
        with pytest.raises(ValueError, match="series_scores.groups"):
            ss({"groups": broken})
    assert G.series_config(to_config({"evaluation": {"series": {"members": 2, "calendar_origin": "2020-01-01"}}})) == (2, None)
    with pytest.raises(ValueError, match="series"):
        G.series_config(to_config({"evaluation": {"series": {"origin": 0}}}))

    class Loader:
        class fields:
            dates = np.array([18262, 18263, 18270])
    cfg = lambda s: to_config({"evaluation": {"series": s}})                      # noqa: E731
    assert G.series_calendar(cfg({}), Loader) == 18262 and G.series_calendar(cfg({"calendar_origin": "2019-12-25"}), Loader) == 18255
    assert G.series_calendar(cfg({"calendar_origin": 5}), Loader) == 5 and G.series_calendar(cfg({}), object()) is None
    with pytest.raises(ValueError, match="calendar_origin"):
        G.series_calendar(cfg({"calendar_origin": "2019-12-25"}), object())
    with pytest.raises(ValueError, match="calendar_origin"):
        G.series_calendar(cfg({"calendar_origin": "Christmas"}), Loader)
    served = G._SeriesDates(18260)
    assert served.days(np.array([18262, 18263])).tolist() == [2, 3] and served.days(np.array([18270])).tolist() == [10]
    with pytest.raises(ValueError, match="strictly increasing"):                  # across batches too
        served.days(np.array([18270]))
    idx = G._SeriesDates(18262)
    idx.days(np.array([18262, 18263]))
    assert idx.index()["dates"].tolist() == [18262, 18263] and int(idx.index()["calendar_origin"]) == 18262


def test_evaluation_reads_the_dates_of_a_series(tmp_path, monkeypatch):
    from sbgm_danra_amd.config_loader import load_config
    from sbgm_danra_amd.utils import get_model_string
    for k in ("DATA_DIR", "CKPT_DIR", "SAMPLE_DIR", "STATS_LOAD_DIR"):
        monkeypatch.setenv(k, str(tmp_path / k.lower()))
    monkeypatch.setenv("SLURM_CPUS_PER_TASK", "2")
    cfg = load_config(os.path.join(ROOT, "sbgm_danra_amd", "config", "default_config.yaml"))
    d = os.path.join(cfg.paths.sample_dir, "generation", get_model_string(cfg), "generated_samples")
    os.makedirs(d)
    rng = np.random.default_rng(1)
    np.savez_compressed(os.path.join(d, "gen_samples_series_n_4.npz"), rng.random((4, 2, 4, 5)).astype(f32))
    np.savez_compressed(os.path.join(d, "eval_samples_series_n_4.npz"), rng.random((4, 4, 5)).astype(f32))
    index = os.path.join(d, "series_index_series_n_4.npz")
    np.savez_compressed(index, members=np.int64(2))
    ev = E.Evaluation(cfg, "series", None, device=torch.device("cpu"))
    assert ev.dates is None
    with pytest.raises(ValueError, match="no dates"):
        ev.climate_statistics(1.0, [], [], calendar_aware=True)
    with pytest.raises(ValueError, match="needs the dates"):
        ev.climate_statistics(1.0, [], [], groups="season")
    with pytest.raises(ValueError, match="needs the dates"):
        ev.series_ensemble_statistics(groups="month")
    with pytest.raises(ValueError, match="holds 3 ids"):
        ev.climate_statistics(1.0, [], [], groups=[0, 1, 0])
    np.savez_compressed(index, members=np.int64(2), dates=np.array([18320, 18321, 18322, 18400]), calendar_origin=np.int64(18320))
    ev = E.Evaluation(cfg, "series", None, device=torch.device("cpu"))
    assert ev.dates.dtype == np.int64 and ev.dates.tolist() == [18320, 18321, 18322, 18400]
    assert ev._day_groups("k", "season", 4) == ([0, 0, 1, 1], ["DJF", "MAM"])
    assert ev._day_groups("k", [0, 2, 0, 2], 4) == ([0, 2, 0, 2], ["0", "1", "2"]) and ev._day_groups("k", None, 4) == (None, None)
    with pytest.raises(NativeError):                                             # arguments fine; the fields are on the CPU
        ev.climate_statistics(1.0, [0.5], [], groups="season")
    np.savez_compressed(index, members=np.int64(2), dates=np.array([3, 2, 1, 0]))
    with pytest.raises(ValueError, match="strictly increasing"):
        E.Evaluation(cfg, "series", None, device=torch.device("cpu"))
