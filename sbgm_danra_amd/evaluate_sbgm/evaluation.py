"""`Evaluation` — the statistics half of reference sbgm/evaluate_sbgm/evaluation.py:15-444, on the device.  Reads the npz
files `SampleGenerator` writes, moves them to the GPU once, and computes every statistic with the verification kernels
(csrc/verify.hip and csrc/verify_spatial.hip via `..verification`): the reference's pixel, spatial and daily statistics plus
ensemble scores (CRPS, rank histogram, spread/skill), radially averaged power spectra and, on request, neighbourhood scores
(Fractions Skill Score), threshold-exceedance scores (Brier, reliability table, ROC area), ensemble products (mean, spread,
envelope, quantile and exceedance-probability maps with the coverage of each quantile map), object-based scores (connected
objects and SAL: structure, amplitude, location), multivariate ensemble scores (energy score, variogram score), climate indices
along the day axis and the pooled ensemble verification of a series over days x pixels.  Only scalars, maps, per-field arrays and histograms come back to the host.
Plots are out of scope: the plotting keys are accepted and logged as skipped.

Files are found by name: `gen_samples_*`, `eval_samples_*` and `lsm_samples_*` with the suffixes `multi_n_<B>`, `single`,
`repeated_n_<n>` (this package), `repeated_<n>` (the reference) or `series_n_<D>` (gen_samples [D, M, H, W]: D days of M
members each; the per-field statistics run on member 0, the climate indices and the series scores on all members), each optionally followed by
`_rank<r>`.  Rank files of `multiple` / `single` are concatenated along the sample axis; each rank's `repeated` file is its own
unit (every rank conditions on a different sample), selected with `rank=`."""
from __future__ import annotations

import json
import logging
import math
import os
import re

import numpy as np
import torch

from .. import verification as V
from .. import calendar
from ..utils import get_model_string

logger = logging.getLogger(__name__)

GEN_TYPES = ("multiple", "single", "repeated", "series")
TIME_AXIS_TYPES = ("multiple", "series")       # gen and obs pair up day by day: what the climate indices need
PREFIXES = ("gen_samples", "eval_samples", "lsm_samples")
_SUFFIX = {"multiple": r"multi_n_(?P<n>\d+)", "single": r"single(?P<n>)", "repeated": r"repeated_(?:n_)?(?P<n>\d+)",
           "series": r"series_n_(?P<n>\d+)"}
CLIMATE_DEFINITION = (
    "per pixel over the valid days (gen and obs not NaN, mask admits; paired): wet day = value >= wet; wet_freq = n_wet / n; sdii = "
    "mean over the wet days; cwd / cdd = longest run of consecutive valid wet / dry days; p_ww = n_ww / (n_ww + n_wd), p_dw = n_dw / "
    "(n_dw + n_dd) over adjacent valid days; lag1 = lag-1 autocovariance / variance; quantiles = numpy's default (type 7) over the "
    "valid days, wet_quantiles over the valid wet days; heavy_fraction = sum of the values > the OBS wet_quantiles map / sum over the "
    "wet days (ETCCDI R95pTOT at level 0.95).  Summary per index and level over the pixels where both maps are finite: domain means, "
    "bias = mean_gen - mean_obs, rmse, Pearson pattern correlation.  cwd, cdd, transitions, p_ww, p_dw and lag1 are computed in FILE "
    "ORDER: they mean something only when the file holds consecutive days at a fixed location (a 'series' from an unshuffled loader "
    "whose cutout rectangle equals data_size)")
CLIMATE_CALENDAR_DEFINITION = (
    ".  With `calendar` a gap in the dates acts as one invalid day between the two days: it ends a spell, and no transition and no "
    "lag-1 product spans it.  `groups`: the same indices over the days of each group, which keep their dates, so a spell or a pair "
    "also ends where the group's days are not consecutive; each group has its own mean in lag1 and its own OBS wet_quantiles map in "
    "heavy_fraction")
PIXEL_BINS = 150                      # the reference's pixel-value histograms (evaluation.py:320)
CRPS_DEFINITIONS = {"crps_fair": "(1/M) sum_i |x_i - y| - sum_ij |x_i - x_j| / (2 M (M - 1))",
                    "crps_standard": "(1/M) sum_i |x_i - y| - sum_ij |x_i - x_j| / (2 M^2)"}


def sample_units(sample_dir, gen_type, n_samples=None):
    """the evaluation units of one generation type in `sample_dir`: a list of (rank or None, {prefix: [paths in rank order]}).
    `multiple` / `single` give one unit (rank files concatenated); `repeated` gives one unit per rank file.  When files of
    several sizes exist, the one of size `n_samples` is taken."""
    if gen_type not in GEN_TYPES:
        raise ValueError(f"Unknown generated sample type: {gen_type}. Choose from: {list(GEN_TYPES)}")
    pat = re.compile(rf"^(?P<prefix>{'|'.join(PREFIXES)})_{_SUFFIX[gen_type]}(?:_rank(?P<rank>\d+))?\.npz$")
    found = {}                                         # (rank, n) -> {prefix: path}
    for f in sorted(os.listdir(sample_dir)) if os.path.isdir(sample_dir) else []:
        m = pat.match(f)
        if m:
            r = None if m.group("rank") is None else int(m.group("rank"))
            found.setdefault((r, m.group("n")), {})[m.group("prefix")] = os.path.join(sample_dir, f)
    found = {k: v for k, v in found.items() if "gen_samples" in v}
    if not found:
        raise FileNotFoundError(f"no gen_samples_* file of type '{gen_type}' in {sample_dir}")
    plain = {k: v for k, v in found.items() if k[0] is None}
    pool = plain or found                               # an unranked file wins over rank files
    if plain and len(plain) != len(found):
        ranked = sorted({k[0] for k in found if k[0] is not None})
        logger.warning(f"[WARN] {sample_dir} holds both single-process '{gen_type}' files and rank files (ranks {ranked}); "
                       f"evaluating the single-process files. Remove the ones that are stale.")
    by_rank = {}
    for (r, n), files in pool.items():
        by_rank.setdefault(r, {})[n] = files
    chosen = {}
    for r, sizes in by_rank.items():
        if len(sizes) == 1:
            chosen[r] = next(iter(sizes.values()))
        elif n_samples is not None and str(n_samples) in sizes:
            chosen[r] = sizes[str(n_samples)]
        else:
            raise ValueError(f"several '{gen_type}' sample sizes {sorted(sizes)} in {sample_dir}"
                             f"{'' if r is None else f' for rank {r}'}; none matches n_samples={n_samples}")
    ranks = sorted(chosen, key=lambda r: -1 if r is None else r)
    for r in ranks:
        if "eval_samples" not in chosen[r]:
            raise FileNotFoundError(f"gen_samples of type '{gen_type}' (rank {r}) have no matching eval_samples file in {sample_dir}")
    if gen_type == "repeated":
        return [(r, {p: [chosen[r][p]] for p in chosen[r]}) for r in ranks]
    merged = {p: [chosen[r][p] for r in ranks] for p in PREFIXES if all(p in chosen[r] for r in ranks)}
    return [(None, merged)]


def _fields3(a):
    """[N,H,W] from the saved layouts: [N,H,W], [N,C,H,W] (channel 0) or [H,W]"""
    a = np.asarray(a)
    if a.ndim == 4:
        a = a[:, 0]
    elif a.ndim == 2:
        a = a[None]
    if a.ndim != 3:
        raise ValueError(f"unexpected sample array shape {a.shape}")
    return a


def _load(paths):
    return np.concatenate([_fields3(np.load(p)["arr_0"]) for p in paths], axis=0).astype(np.float32, copy=False)


def statistics_dir(cfg):
    """<paths.evaluation_dir>/<model string>/statistics, or <paths.sample_dir>/evaluation/<model string>/statistics"""
    paths = cfg["paths"]
    base = paths.get("evaluation_dir") or os.path.join(paths["sample_dir"], "evaluation")
    return os.path.join(base, get_model_string(cfg), "statistics")


def _number_list(key, values, lo=None, hi=None):
    """the config list `key` as floats: at most 16 finite numbers (no bools), within [lo, hi] when bounds are given"""
    if len(values) > V.MAX_THRESHOLDS:
        raise ValueError(f"{key}: at most {V.MAX_THRESHOLDS} entries, got {len(values)}")
    if any(isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or not (lo is None or lo <= v <= hi)
           for v in values):
        raise ValueError(f"{key} must be {'finite numbers' if lo is None else f'numbers in [{lo}, {hi}]'}, got {list(values)}")
    return [float(v) for v in values]


def spatial_scores_config(cfg):
    """(thresholds, scales) of the optional evaluation.spatial_scores section — thresholds in the units the generated files
    hold, scales as odd window widths in pixels — or None when the section is absent"""
    sec = cfg["evaluation"].get("spatial_scores")
    if sec is None:
        return None
    thresholds, scales = sec.get("thresholds"), sec.get("scales")
    if not isinstance(thresholds, (list, tuple)) or not isinstance(scales, (list, tuple)) or not thresholds or not scales:
        raise ValueError("evaluation.spatial_scores needs non-empty lists 'thresholds' and 'scales'")
    if len(scales) > V.MAX_SCALES:
        raise ValueError(f"evaluation.spatial_scores.scales: at most {V.MAX_SCALES} entries, got {len(scales)}")
    thresholds = _number_list("evaluation.spatial_scores.thresholds", thresholds)
    if any(isinstance(n, bool) or not isinstance(n, int) or n < 1 or n % 2 == 0 for n in scales):
        raise ValueError(f"evaluation.spatial_scores.scales must be odd integers >= 1 (window widths in pixels), got {list(scales)}")
    return thresholds, [int(n) for n in scales]


def ensemble_products_config(cfg):
    """(quantiles, thresholds) of the optional evaluation.ensemble_products section — quantile levels in [0, 1], thresholds in
    the units the generated files hold; either list may be empty, not both — or None when the section is absent"""
    sec = cfg["evaluation"].get("ensemble_products")
    if sec is None:
        return None
    quantiles, thresholds = sec.get("quantiles") or [], sec.get("thresholds") or []
    if not isinstance(quantiles, (list, tuple)) or not isinstance(thresholds, (list, tuple)) or not (quantiles or thresholds):
        raise ValueError("evaluation.ensemble_products needs lists 'quantiles' and 'thresholds', at least one of them non-empty")
    return (_number_list("evaluation.ensemble_products.quantiles", quantiles, 0, 1),
            _number_list("evaluation.ensemble_products.thresholds", thresholds))


def object_scores_config(cfg):
    """(thresholds, relative, connectivity) of the optional evaluation.object_scores section — `thresholds`: up to 16 finite
    numbers in the units the generated files hold (may be empty or absent when `relative` is given); `relative`: None or
    {factor, quantile, wet}, Wernli's R* = factor * R^quantile over the values >= wet; `connectivity`: 4 or 8 (default 8) — or
    None when the section is absent"""
    sec = cfg["evaluation"].get("object_scores")
    if sec is None:
        return None
    thresholds, relative, connectivity = sec.get("thresholds") or [], sec.get("relative"), sec.get("connectivity", 8)
    if not isinstance(thresholds, (list, tuple)) or not (thresholds or relative is not None):
        raise ValueError("evaluation.object_scores needs a list 'thresholds', a 'relative' section, or both")
    thresholds = _number_list("evaluation.object_scores.thresholds", thresholds)
    if relative is not None:
        if not hasattr(relative, "keys") or set(relative.keys()) != {"factor", "quantile", "wet"}:
            raise ValueError("evaluation.object_scores.relative needs exactly the keys 'factor', 'quantile' and 'wet'")
        keys = ("factor", "quantile", "wet")
        values = _number_list("evaluation.object_scores.relative: factor, quantile and wet", [relative[k] for k in keys])
        relative = dict(zip(keys, values))
        if not 0.0 <= relative["quantile"] <= 1.0:
            raise ValueError(f"evaluation.object_scores.relative.quantile must lie in [0, 1], got {relative['quantile']}")
    if isinstance(connectivity, bool) or connectivity not in (4, 8):
        raise ValueError(f"evaluation.object_scores.connectivity must be 4 or 8, got {connectivity!r}")
    return thresholds, relative, int(connectivity)


def multivariate_scores_config(cfg):
    """(energy, variogram) of the optional evaluation.multivariate_scores section — `energy`: bool (default false);
    `variogram`: None or {radius: 1..8 (default 4), order: 0.5, 1 or 2 (default 0.5), weights: 'inverse_distance' (default) or
    'unit'}; at least one of the two must be asked for — or None when the section is absent"""
    sec = cfg["evaluation"].get("multivariate_scores")
    if sec is None:
        return None
    if not hasattr(sec, "keys") or not set(sec.keys()) <= {"energy", "variogram"}:
        raise ValueError("evaluation.multivariate_scores takes the keys 'energy' and 'variogram' only")
    energy, variogram = sec.get("energy", False), sec.get("variogram")
    if not isinstance(energy, bool):
        raise ValueError(f"evaluation.multivariate_scores.energy must be true or false, got {energy!r}")
    if variogram is not None:
        if not hasattr(variogram, "keys") or not set(variogram.keys()) <= {"radius", "order", "weights"}:
            raise ValueError("evaluation.multivariate_scores.variogram takes the keys 'radius', 'order' and 'weights' only")
        radius, order, weights = variogram.get("radius", 4), variogram.get("order", 0.5), variogram.get("weights", "inverse_distance")
        if isinstance(radius, bool) or not isinstance(radius, int) or not 1 <= radius <= V.MAX_VARIOGRAM_RADIUS:
            raise ValueError(f"evaluation.multivariate_scores.variogram.radius must be an integer in 1..{V.MAX_VARIOGRAM_RADIUS}, "
                             f"got {radius!r}")
        if isinstance(order, bool) or not isinstance(order, (int, float)) or float(order) not in V.VARIOGRAM_ORDERS:
            raise ValueError(f"evaluation.multivariate_scores.variogram.order must be one of {V.VARIOGRAM_ORDERS}, got {order!r}")
        if weights not in V.VARIOGRAM_WEIGHTS:
            raise ValueError(f"evaluation.multivariate_scores.variogram.weights must be one of {V.VARIOGRAM_WEIGHTS}, got {weights!r}")
        variogram = {"radius": int(radius), "order": float(order), "weights": str(weights)}
    if not energy and variogram is None:
        raise ValueError("evaluation.multivariate_scores asks for nothing: set 'energy: true', give a 'variogram' section, or both")
    return energy, variogram


CLIMATE_CALENDAR_KEYS = ("calendar", "groups")


def climate_indices_config(cfg):
    """(wet, quantiles, wet_quantiles) of the optional evaluation.climate_indices section — `wet`: the wet-day threshold in the
    units the generated files hold (default 1.0); `quantiles`, `wet_quantiles`: at most 8 levels in [0, 1] each, either may be
    empty or absent — or None when the section is absent"""
    sec = cfg["evaluation"].get("climate_indices")
    if sec is None:
        return None
    keys = ("wet", "quantiles", "wet_quantiles")
    if not hasattr(sec, "keys") or not set(sec.keys()) <= set(keys + CLIMATE_CALENDAR_KEYS):
        unknown = sorted(set(sec.keys()) - set(keys + CLIMATE_CALENDAR_KEYS)) if hasattr(sec, "keys") else sec
        raise ValueError(f"evaluation.climate_indices takes the keys 'wet', 'quantiles', 'wet_quantiles', 'calendar' and 'groups' "
                         f"only, got {unknown!r}")
    climate_calendar_config(cfg)
    wet = sec.get("wet", 1.0)
    if isinstance(wet, bool) or not isinstance(wet, (int, float)) or not math.isfinite(wet):
        raise ValueError(f"evaluation.climate_indices.wet must be a finite number, got {wet!r}")
    levels = []
    for key in keys[1:]:
        values = sec.get(key)
        values = [] if values is None else values
        if not isinstance(values, (list, tuple)):
            raise ValueError(f"evaluation.climate_indices.{key} must be a list of levels in [0, 1], got {values!r}")
        if len(values) > V.MAX_TEMPORAL_QUANTILES:
            raise ValueError(f"evaluation.climate_indices.{key}: at most {V.MAX_TEMPORAL_QUANTILES} entries, got {len(values)}")
        levels.append(_number_list(f"evaluation.climate_indices.{key}", values, 0, 1))
    return float(wet), levels[0], levels[1]


def _groups_setting(key, groups):
    """a `groups` setting: None, "season" or "month" (from the dates of the series), a .npy path, or a list of ids in 0..15"""
    if isinstance(groups, str):
        if groups not in calendar.GROUPINGS and not groups.endswith(".npy"):
            raise ValueError(f"{key}: a string must be 'season', 'month' or the path of a .npy file, got {groups!r}")
    elif groups is not None:
        if not isinstance(groups, (list, tuple)) or not groups or any(isinstance(g, bool) or not isinstance(g, int) or
                                                                      not 0 <= g < V.MAX_SERIES_GROUPS for g in groups):
            raise ValueError(f"{key} must be null, 'season', 'month', a .npy path or a list of integers in "
                             f"0..{V.MAX_SERIES_GROUPS - 1}, one per day, got {groups!r}")
        groups = [int(g) for g in groups]
    return groups


def climate_calendar_config(cfg):
    """(calendar, groups) of the evaluation.climate_indices section — `calendar`: None (the default: true when the series has
    dates) or a bool, whether a gap in the dates ends spells and pairs; `groups`: None, "season", "month", a list of one id in
    0..15 per day, or a .npy path — (None, None) when the section is absent"""
    sec = cfg["evaluation"].get("climate_indices")
    if sec is None or not hasattr(sec, "keys"):
        return None, None
    cal = sec.get("calendar")
    if cal is not None and not isinstance(cal, bool):
        raise ValueError(f"evaluation.climate_indices.calendar must be null, true or false, got {cal!r}")
    return cal, _groups_setting("evaluation.climate_indices.groups", sec.get("groups"))


PERIOD_KEYS = ("windows", "thresholds", "wet", "periods", "min_days", "calendar")


def period_indices_config(cfg):
    """(windows, thresholds, wet, periods, min_days, calendar) of the optional evaluation.period_indices section — `windows`: 1
    to 4 distinct ascending window lengths in days, each in 1..32 (default [1, 5]: Rx1day and Rx5day); `thresholds`: up to 8
    finite numbers in the units the generated files hold (default none; 10 gives R10mm); `wet`: the wet-day threshold of PRCPTOT
    (default 1.0); `periods`: None, "year", "season_year" or "month_year" (from the dates of the series), a list of one id in
    -1..255 per day (-1: no period), or a .npy path; `min_days`: the valid days a period needs at a pixel to count in the mean
    and spread across the periods (default 1); `calendar`: None (the default: true when the series has dates) or a bool, whether
    a gap in the dates breaks a window — or None when the section is absent"""
    sec = cfg["evaluation"].get("period_indices")
    if sec is None:
        return None
    key = "evaluation.period_indices"
    if not hasattr(sec, "keys") or not set(sec.keys()) <= set(PERIOD_KEYS):
        unknown = sorted(set(sec.keys()) - set(PERIOD_KEYS)) if hasattr(sec, "keys") else sec
        raise ValueError(f"{key} takes the keys {', '.join(repr(k) for k in PERIOD_KEYS)} only, got {unknown!r}")
    windows = sec.get("windows")
    windows = [1, 5] if windows is None else windows
    if (not isinstance(windows, (list, tuple)) or not 1 <= len(windows) <= V.MAX_PERIOD_WINDOWS or
            any(isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= V.MAX_PERIOD_WINDOW for k in windows) or
            any(b <= a for a, b in zip(windows, windows[1:]))):
        raise ValueError(f"{key}.windows must be a list of 1..{V.MAX_PERIOD_WINDOWS} distinct ascending integers in "
                         f"1..{V.MAX_PERIOD_WINDOW}, got {windows!r}")
    thresholds = sec.get("thresholds")
    thresholds = [] if thresholds is None else thresholds
    if not isinstance(thresholds, (list, tuple)):
        raise ValueError(f"{key}.thresholds must be a list of numbers, got {thresholds!r}")
    if len(thresholds) > V.MAX_PERIOD_THRESHOLDS:
        raise ValueError(f"{key}.thresholds: at most {V.MAX_PERIOD_THRESHOLDS} entries, got {len(thresholds)}")
    thresholds = _number_list(f"{key}.thresholds", thresholds)
    wet = sec.get("wet", 1.0)
    if isinstance(wet, bool) or not isinstance(wet, (int, float)) or not math.isfinite(wet):
        raise ValueError(f"{key}.wet must be a finite number, got {wet!r}")
    periods = sec.get("periods")
    if isinstance(periods, str):
        if periods not in calendar.PERIODS and not periods.endswith(".npy"):
            raise ValueError(f"{key}.periods: a string must be one of {calendar.PERIODS} or the path of a .npy file, got {periods!r}")
    elif periods is not None:
        if not isinstance(periods, (list, tuple)) or not periods or any(isinstance(g, bool) or not isinstance(g, int) or
                                                                        not -1 <= g < V.MAX_PERIODS for g in periods):
            raise ValueError(f"{key}.periods must be null, one of {calendar.PERIODS}, a .npy path or a list of integers in "
                             f"-1..{V.MAX_PERIODS - 1}, one per day, got {periods!r}")
        periods = [int(g) for g in periods]
    min_days = sec.get("min_days", 1)
    if isinstance(min_days, bool) or not isinstance(min_days, int) or min_days < 1:
        raise ValueError(f"{key}.min_days must be an integer >= 1, got {min_days!r}")
    cal = sec.get("calendar")
    if cal is not None and not isinstance(cal, bool):
        raise ValueError(f"{key}.calendar must be null, true or false, got {cal!r}")
    return [int(k) for k in windows], thresholds, float(wet), periods, int(min_days), cal


PERIOD_DEFINITION = (
    "per pixel along the day axis; a day is valid where the truth and every member are not NaN and the mask admits it.  A window of "
    "K days ending on day t exists when the K days are valid and linked (consecutive in the file, or with `calendar` consecutive "
    "dates); rx_K = the largest window sum (K = 1: Rx1day, K = 5: Rx5day).  count_T = the valid days with value >= T (R10mm at "
    "10).  prcptot = the sum over the valid days with value >= wet.  Per period (year, season of a year with December counted to "
    "the following year, month of a year): count and prcptot over the period's days, rx over the windows whose last day lies in "
    "the period (a window may begin in the period before, as in climdex).  period_mean / period_std = mean and standard deviation "
    "(n - 1) across the periods with at least min_days valid days and a defined value.  Each entry compares the model's map with "
    "the truth's: domain means, bias, RMSE and pattern correlation per member, with mean, minimum and maximum over the members")


def series_scores_config(cfg):
    """(thresholds, climatology, groups, seed) of the optional evaluation.series_scores section — `thresholds`: up to 16 finite
    numbers in the units the generated files hold (default none); `climatology`: bool (default true), the leave-one-out
    climatological reference and the CRPS skill score; `groups`: None, a list of one integer group id in 0..15 per day, the
    path of a .npy file holding one, or "season" / "month" (from the dates of the series); `seed`: None (evaluation.seed) or an integer, the seed of the rank ties — or None when the
    section is absent"""
    sec = cfg["evaluation"].get("series_scores")
    if sec is None:
        return None
    keys = ("thresholds", "climatology", "groups", "seed")
    if not hasattr(sec, "keys") or not set(sec.keys()) <= set(keys):
        unknown = sorted(set(sec.keys()) - set(keys)) if hasattr(sec, "keys") else sec
        raise ValueError(f"evaluation.series_scores takes the keys 'thresholds', 'climatology', 'groups' and 'seed' only, got {unknown!r}")
    thresholds = sec.get("thresholds")
    thresholds = [] if thresholds is None else thresholds
    if not isinstance(thresholds, (list, tuple)):
        raise ValueError(f"evaluation.series_scores.thresholds must be a list of numbers, got {thresholds!r}")
    thresholds = _number_list("evaluation.series_scores.thresholds", thresholds)
    climatology = sec.get("climatology", True)
    if not isinstance(climatology, bool):
        raise ValueError(f"evaluation.series_scores.climatology must be true or false, got {climatology!r}")
    groups = _groups_setting("evaluation.series_scores.groups", sec.get("groups"))
    seed = sec.get("seed")
    if seed is not None and (isinstance(seed, bool) or not isinstance(seed, int)):
        raise ValueError(f"evaluation.series_scores.seed must be null or an integer, got {seed!r}")
    return thresholds, climatology, groups, seed


SERIES_DEFINITION = (
    "pooled over days x pixels of the series; a cell (day, pixel) is valid when the truth and every member are not NaN and the mask "
    "admits it.  crps_fair, crps_standard, skill, spread, spread_skill_ratio: as ensemble_stats, over the cells.  rank histogram: rank "
    "of the truth among the M members, ties broken at random.  rank_reliability_index = sum_k |h_k / N - 1 / (M + 1)|; outside_fraction "
    "= (h_0 + h_M) / N.  brier scores from the table (members >= threshold, truth >= threshold) over the cells; brier_skill = 1 - brier "
    "/ brier_uncertainty.  crpss = 1 - sum F / sum C over the cells of the pixels with at least 3 valid days, F the forecast's fair CRPS, "
    "C that of the leave-one-out ensemble of the truth on the other valid days of the same pixel (and group).  pooled = all days; "
    "groups = the days with that group id")


def _pattern_summary(gen, obs):
    """float64 summary of a gen map against the obs map over the pixels where both are finite"""
    g, o = np.asarray(gen, np.float64), np.asarray(obs, np.float64)
    ok = np.isfinite(g) & np.isfinite(o)
    g, o = g[ok], o[ok]
    nan = float("nan")
    if g.size == 0:
        return {"pixels": 0, "mean_gen": nan, "mean_obs": nan, "bias": nan, "rmse": nan, "pattern_corr": nan}
    dg, do = g - g.mean(), o - o.mean()
    den = math.sqrt(float((dg * dg).sum()) * float((do * do).sum()))
    return {"pixels": int(g.size), "mean_gen": float(g.mean()), "mean_obs": float(o.mean()), "bias": float(g.mean() - o.mean()),
            "rmse": float(np.sqrt(((g - o) ** 2).mean())), "pattern_corr": float((dg * do).sum()) / den if den > 0 else nan}


def _members_summary(gen_maps, obs_map):
    """the pattern summary of every member's map against the truth's map: `per_member`, each statistic as its mean, minimum and
    maximum over the members (NaNs left out), and `pixels` per member"""
    per = [_pattern_summary(g, obs_map) for g in gen_maps]
    row = {"per_member": per}
    for stat in ("mean_gen", "mean_obs", "bias", "rmse", "pattern_corr"):
        vals = np.asarray([p[stat] for p in per], np.float64)
        good = vals[~np.isnan(vals)]
        row[stat] = {"mean": float(good.mean()) if good.size else float("nan"),
                     "min": float(good.min()) if good.size else float("nan"),
                     "max": float(good.max()) if good.size else float("nan")}
    row["pixels"] = [p["pixels"] for p in per]
    return row


def _nan_quartiles(a):
    """(median, 25th, 75th percentile, NaN count) of a 1-D array, NaNs ignored; NaN quartiles when nothing is left"""
    a = np.asarray(a, np.float64)
    good = a[~np.isnan(a)]
    if good.size == 0:
        return float("nan"), float("nan"), float("nan"), int(a.size)
    q25, q50, q75 = np.percentile(good, [25, 50, 75])
    return float(q50), float(q25), float(q75), int(a.size - good.size)


class Evaluation:
    def __init__(self, cfg, generated_sample_type="repeated", n_samples=4, rank=None, device=None):
        self.cfg = cfg
        self.generated_sample_type = generated_sample_type
        self.model_name_str = get_model_string(cfg)
        self.generated_sample_path = os.path.join(cfg["paths"]["sample_dir"], "generation", self.model_name_str, "generated_samples")
        self.evaluation_stats_path = statistics_dir(cfg)
        os.makedirs(self.evaluation_stats_path, exist_ok=True)
        units = sample_units(self.generated_sample_path, generated_sample_type, n_samples)
        if rank is None and len(units) > 1:
            raise ValueError(f"'{generated_sample_type}' files of ranks {[u[0] for u in units]}: pick one with rank=")
        match = [u for u in units if rank is None or u[0] == rank]
        if not match:
            raise FileNotFoundError(f"no '{generated_sample_type}' files of rank {rank} in {self.generated_sample_path}")
        self.rank, files = match[0]
        self.label = generated_sample_type + ("" if self.rank is None else f"_rank{self.rank}")
        self.device = device if device is not None else torch.device("cuda", torch.cuda.current_device() if torch.cuda.is_available() else 0)
        logger.info(f"[INFO] Evaluating {self.label} from {files['gen_samples']}")
        self.members = None
        self.dates = self._series_dates(files["gen_samples"]) if generated_sample_type == "series" else None
        if generated_sample_type == "series":
            # [D, M, H, W]: every per-field statistic runs on member 0, the climate indices on all members
            arrs = [np.asarray(np.load(p)["arr_0"]) for p in files["gen_samples"]]
            if any(a.ndim != 4 for a in arrs):
                raise ValueError(f"'series' gen_samples must be [days, members, H, W], got {[a.shape for a in arrs]}")
            self.members = torch.from_numpy(np.concatenate(arrs, axis=0).astype(np.float32, copy=False)).to(self.device)
            self.members = self.members.permute(1, 0, 2, 3).contiguous()              # [M, D, H, W]
            self.gen_imgs = self.members[0]
        else:
            self.gen_imgs = torch.from_numpy(_load(files["gen_samples"])).to(self.device)
        self.eval_imgs = torch.from_numpy(_load(files["eval_samples"])).to(self.device)
        n, no = self.gen_imgs.shape[0], self.eval_imgs.shape[0]
        if self.eval_imgs.shape[1:] != self.gen_imgs.shape[1:] or no not in (1, n):
            raise ValueError(f"eval_samples {tuple(self.eval_imgs.shape)} do not match gen_samples {tuple(self.gen_imgs.shape)}")
        self.mask = None
        if cfg["evaluation"].get("mask_stats", False):
            if "lsm_samples" not in files:
                raise FileNotFoundError(f"evaluation.mask_stats is set but there is no lsm_samples file for {self.label} in "
                                        f"{self.generated_sample_path}")
            lsm = torch.from_numpy(_load(files["lsm_samples"])).to(self.device)
            if lsm.shape[1:] != self.gen_imgs.shape[1:] or lsm.shape[0] not in (1, n):
                raise ValueError(f"lsm_samples {tuple(lsm.shape)} do not match gen_samples {tuple(self.gen_imgs.shape)}")
            self.mask = (lsm > 0.5).to(torch.uint8)         # land pixels (channel 0)
        self.n_samples = n
        self.metrics = {"gen_type": generated_sample_type, "rank": self.rank, "n_samples": n, "n_obs": no,
                        "shape": list(self.gen_imgs.shape[1:]), "mask_stats": self.mask is not None}
        if self.members is not None:
            self.metrics.update(member=0, members=int(self.members.shape[0]))
        self.fields = {}
        self._err = None

    @staticmethod
    def _series_dates(gen_paths):
        """int64 day numbers [D] from the `dates` of series_index_<suffix>.npz beside every gen_samples file, else None"""
        parts = []
        for p in gen_paths:
            index = os.path.join(os.path.dirname(p), os.path.basename(p).replace("gen_samples_", "series_index_", 1))
            if not os.path.exists(index):
                return None
            with np.load(index) as f:
                if "dates" not in f.files:
                    return None
                parts.append(np.asarray(f["dates"]))
        return calendar.day_numbers(np.concatenate(parts))

    def _day_groups(self, key, groups, D):
        """(ids list or None, names or None) of a `groups` setting for the D days of this unit"""
        names = None
        if isinstance(groups, str) and groups in calendar.GROUPINGS:
            if self.dates is None:
                raise ValueError(f"{key}: '{groups}' needs the dates of the series; {self.label} has none (no `dates` in its "
                                 f"series_index file)")
            groups, names = calendar.groups_from_dates(self.dates, groups)
        elif isinstance(groups, str):
            groups = np.load(groups)
        if groups is None:
            return None, None
        groups = np.asarray(groups)
        if groups.ndim != 1 or groups.dtype.kind not in "iu":
            raise ValueError(f"{key} must hold one integer id per day, got shape {groups.shape} of {groups.dtype}")
        if len(groups) != D:
            raise ValueError(f"{key} holds {len(groups)} ids; {self.label} has {D} days")
        groups = [int(g) for g in groups]
        G = max(groups) + 1                                 # names of the G = largest id + 1 groups the scores have rows for
        return groups, (names[:G] if names is not None else [str(g) for g in range(G)])

    def _need_ensemble(self, what):
        """the `repeated` samples are an ensemble for one condition: `what` needs them, and at least 2 members"""
        if self.generated_sample_type != "repeated":
            raise ValueError(f"{what} needs 'repeated' samples (an ensemble for one condition), not '{self.generated_sample_type}'")
        if self.n_samples < 2:
            raise ValueError(f"{what} needs at least 2 members; {self.label} has {self.n_samples}")

    def _error_stats(self):
        if self._err is None:
            self._err = V.error_stats(self.gen_imgs, self.eval_imgs, self.mask)
        return self._err

    def _valid(self):
        """host copies of the valid (gen, obs) pixel values, flattened — only for the reference's save_stats files"""
        g = self.gen_imgs
        o = self.eval_imgs.expand_as(g)
        v = ~(torch.isnan(g) | torch.isnan(o))
        if self.mask is not None:
            v &= self.mask.expand_as(g).bool()
        return g[v].cpu().numpy(), o[v].cpu().numpy()

    def full_pixel_statistics(self, show_figs=False, save_figs=False, save_stats=False, save_path=None, n_samples=None):
        """global count / means / bias / MAE / RMSE / extremes, 150-bin histograms of gen and obs over their joint range and of
        |gen - obs| over [0, its bound] (reference evaluation.py:266-389)"""
        if show_figs or save_figs:
            logger.info("[INFO] full_pixel_statistics: figures are not produced (plotting is out of scope)")
        g = self._error_stats()["global"].cpu().numpy()
        out = dict(zip(V.GLOBAL_KEYS, (float(v) for v in g)))
        out["count"] = int(g[0])
        res = {"metrics": out}
        if out["count"] > 0:
            lo, hi = min(out["min_gen"], out["min_obs"]), max(out["max_gen"], out["max_obs"])
            hi = hi if hi > lo else lo + 1.0
            dmax = max(out["max_gen"] - out["min_obs"], out["max_obs"] - out["min_gen"], 0.0)
            dmax = dmax if dmax > 0 else 1.0
            res["hist_gen"] = V.histogram(self.gen_imgs, PIXEL_BINS, lo, hi, ref=self.eval_imgs, mask=self.mask).cpu().numpy()
            res["hist_obs"] = V.histogram(self.eval_imgs.expand_as(self.gen_imgs), PIXEL_BINS, lo, hi, ref=self.gen_imgs,
                                          mask=self.mask).cpu().numpy()
            res["hist_value_edges"] = V.histogram_edges(PIXEL_BINS, lo, hi).numpy()
            res["hist_absdiff"] = V.histogram(self.gen_imgs, PIXEL_BINS, 0.0, dmax, ref=self.eval_imgs, mask=self.mask,
                                              absdiff=True).cpu().numpy()
            res["hist_absdiff_edges"] = V.histogram_edges(PIXEL_BINS, 0.0, dmax).numpy()
        self.metrics["pixel_stats"] = out
        self.fields.update({f"pixel_{k}": v for k, v in res.items() if k != "metrics"})
        if save_stats:
            n = self.n_samples if n_samples is None else n_samples
            gf, of = self._valid()
            np.savez(os.path.join(self.evaluation_stats_path, f"n_samples_{n}_pixel_statistics.npz"), gen_imgs_flat=gf, eval_imgs_flat=of)
            d = np.abs(gf.astype(np.float32) - of.astype(np.float32))
            np.savez(os.path.join(self.evaluation_stats_path, f"n_samples_{n}_RMSE_MAE_statistics.npz"), mae_all=d, rmse_all=d)
        return res

    def spatial_statistics(self, show_figs=False, save_figs=False, save_stats=False, save_path=None, n_samples=None):
        """per-pixel count, MAE, RMSE and bias = nanmean(gen) - nanmean(obs) over the samples (reference evaluation.py:414-444)"""
        if show_figs or save_figs:
            logger.info("[INFO] spatial_statistics: figures are not produced (plotting is out of scope)")
        e = self._error_stats()
        res = {k: e[k].cpu().numpy() for k in ("count", "mae", "rmse", "bias")}
        self.metrics["spatial_stats"] = {"mean_mae_per_pixel": float(np.nanmean(res["mae"])) if (res["count"] > 0).any() else float("nan")}
        self.fields.update({f"spatial_{k}_per_pixel": v for k, v in res.items()})
        return res

    def daily_statistics(self, plot_stats=False, save_plots=False, save_stats=False, save_path=None):
        """per-sample MAE and RMSE over the valid pixels (reference evaluation.py:393-410)"""
        e = self._error_stats()
        res = {k: e[f"sample_{k}"].cpu().numpy() for k in ("count", "mae", "rmse")}
        res["count"] = res["count"].astype(np.int64)
        self.metrics["daily_stats"] = {"n_days": int(res["count"].shape[0])}
        self.fields.update({f"daily_{k}": v for k, v in res.items()})
        return res

    def ensemble_statistics(self, seed=None):
        """CRPS (fair map, fair and standard means), rank histogram, skill, spread and spread/skill ratio of the `repeated`
        samples as an ensemble of M members against their one truth"""
        self._need_ensemble("ensemble_statistics")
        seed = int(self.cfg["evaluation"].get("seed", 0)) if seed is None else int(seed)
        mask = None if self.mask is None else self.mask[0]
        r = V.ensemble_scores(self.gen_imgs, self.eval_imgs[0], mask=mask, seed=seed)
        s = r["scores"].cpu().numpy()
        out = dict(zip(V.ENSEMBLE_KEYS, (float(v) for v in s)))
        out.update(count=int(s[0]), M=self.n_samples, crps_map="crps_fair", crps_definitions=CRPS_DEFINITIONS, rank_seed=seed)
        res = {k: r[k].cpu().numpy() for k in ("mean", "var", "crps", "rank", "rank_hist")}
        self.metrics["ensemble_stats"] = out
        self.fields.update({f"ensemble_{k}": v for k, v in res.items()})
        return dict(res, metrics=out)

    def spectral_statistics(self):
        """radially averaged power spectral density of the generated and the true fields (each field mean-removed; a field
        with a NaN is skipped and counted).  Spectra need whole rectangles, so mask_stats does not apply here."""
        k, pg, sg = V.rapsd(self.gen_imgs)
        _, po, so = V.rapsd(self.eval_imgs)
        res = {"wavenumber": k.cpu().numpy(), "psd_gen": pg.cpu().numpy(), "psd_obs": po.cpu().numpy()}
        out = {"skipped_gen": int(sg), "skipped_obs": int(so), "n_wavenumbers": int(res["wavenumber"].shape[0])}
        self.metrics["spectral_stats"] = out
        self.fields.update({f"spectral_{k}": v for k, v in res.items()})
        return dict(res, metrics=out)

    def _spatial_scores(self, thresholds, scales=None):
        """the given thresholds / scales, each defaulting to the evaluation.spatial_scores section of the config"""
        if thresholds is not None and scales is not None:
            return thresholds, scales
        sec = spatial_scores_config(self.cfg)
        if sec is None:
            raise ValueError("no thresholds / scales given and the config has no evaluation.spatial_scores section")
        return (sec[0] if thresholds is None else thresholds), (sec[1] if scales is None else scales)

    def neighbourhood_statistics(self, thresholds=None, scales=None):
        """Fractions Skill Score over thresholds x odd window widths (pixels) of the generated fields against their truth:
        the fss matrix, the frequency bias, the useful-skill level 0.5 + f_o/2 and, per threshold, the smallest width
        that reaches it; the exact integer numerators, denominators and event counts go to the fields file"""
        thresholds, scales = self._spatial_scores(thresholds, scales)
        r = V.neighbourhood_scores(self.gen_imgs, self.eval_imgs, thresholds, scales, mask=self.mask)
        res = {k: r[k].cpu().numpy() for k in V.NEIGHBOURHOOD_KEYS}
        thresholds, scales = [float(t) for t in thresholds], [int(n) for n in scales]
        useful = []
        for t in range(len(thresholds)):
            ok = [n for n, f in zip(scales, res["fss"][t]) if f >= res["fss_useful"][t]]          # NaN compares false
            useful.append(min(ok) if ok else None)
        out = {"thresholds": thresholds, "scales": scales, "fss": res["fss"].tolist(), "freq_bias": res["freq_bias"].tolist(),
               "fss_useful": res["fss_useful"].tolist(), "useful_scale": useful, "valid": int(res["valid"].sum()),
               "definition": "fss = 1 - sum (C_gen - C_obs)^2 / sum (C_gen^2 + C_obs^2); C = events (v >= threshold) in the "
                             "n x n window, zero beyond the domain"}
        self.metrics["neighbourhood_stats"] = out
        self.fields.update({f"neighbourhood_{k}": res[k] for k in ("num", "den", "fss_field", "events_gen", "events_obs")})
        return dict(res, metrics=out)

    def exceedance_statistics(self, thresholds=None):
        """Brier score with Murphy's reliability / resolution / uncertainty, base rate and ROC area per threshold of the
        `repeated` samples as an ensemble forecasting P(value >= threshold); the table behind them (the reliability
        diagram) goes to the fields file"""
        self._need_ensemble("exceedance_statistics")
        thresholds, _ = self._spatial_scores(thresholds, scales=[1])
        mask = None if self.mask is None else self.mask[0]
        r = V.exceedance_scores(self.gen_imgs, self.eval_imgs[0], thresholds, mask=mask)
        res = {k: r[k].cpu().numpy() for k in ("table",) + V.EXCEEDANCE_KEYS}
        out = {"thresholds": [float(t) for t in thresholds], "M": self.n_samples, "count": int(r["count"])}
        out.update({k: res[k].tolist() for k in V.EXCEEDANCE_KEYS})
        self.metrics["exceedance_stats"] = out
        self.fields["exceedance_table"] = res["table"]
        return dict(res, metrics=out)

    def product_statistics(self, quantiles=None, thresholds=None):
        """ensemble products of the `repeated` samples — mean, standard deviation, minimum, maximum, quantile maps and
        exceedance-probability maps, all to the fields file — and, per quantile level, the coverage: the fraction of valid
        pixels with a non-NaN truth that lies at or below the quantile map, beside its nominal value"""
        self._need_ensemble("product_statistics")
        if quantiles is None or thresholds is None:
            sec = ensemble_products_config(self.cfg)
            if sec is None:
                raise ValueError("no quantiles / thresholds given and the config has no evaluation.ensemble_products section")
            quantiles, thresholds = (sec[0] if quantiles is None else quantiles), (sec[1] if thresholds is None else thresholds)
        quantiles, thresholds = [float(q) for q in quantiles], [float(t) for t in thresholds]
        mask = None if self.mask is None else self.mask[0]
        r = V.ensemble_products(self.gen_imgs, quantiles, thresholds, mask=mask)
        M, obs = self.n_samples, self.eval_imgs[0]
        ok = ~(torch.isnan(r["mean"]) | torch.isnan(obs))
        n_ok = int(ok.sum())
        coverage = [float(((obs <= qmap) & ok).sum()) / n_ok if n_ok else float("nan") for qmap in r["quantiles"]]
        res = {k: r[k].cpu().numpy() for k in ("mean", "std", "min", "max", "quantiles", "exceed_prob")}
        out = {"quantile_levels": quantiles, "thresholds": thresholds, "M": M, "count": int(r["count"]), "coverage": coverage,
               "coverage_nominal": [(q * (M - 1) + 1) / (M + 1) for q in quantiles],
               "definition": "quantiles: numpy's default (Hyndman-Fan type 7) over the members of each pixel; exceed_prob = "
                             "#{members >= threshold} / M; std with ddof 1; coverage = fraction of valid pixels whose truth is <= "
                             "the quantile map; coverage_nominal = (q (M - 1) + 1) / (M + 1), exact for an exchangeable "
                             "continuous ensemble where q (M - 1) is an integer"}
        self.metrics["product_stats"] = out
        self.fields.update({f"products_{k}": v for k, v in res.items()})
        return dict(res, metrics=out)

    def object_statistics(self, thresholds=None, relative=None, connectivity=None):
        """SAL (structure, amplitude, location; Wernli et al. 2008) of the generated fields against their truth, from the
        connected objects of both at each threshold.  The metrics entry `objects` holds, per threshold, the median and the
        quartiles over the fields of S, A and L (NaNs ignored, and counted), the object counts of both sides and the
        area histogram; the per-field arrays go to the fields file.  Arguments default to the evaluation.object_scores
        section.  Meant for non-negative fields such as precipitation."""
        if thresholds is None and relative is None:
            sec = object_scores_config(self.cfg)
            if sec is None:
                raise ValueError("no thresholds / relative given and the config has no evaluation.object_scores section")
            thresholds, relative = sec[0], sec[1]
            connectivity = sec[2] if connectivity is None else connectivity
        thresholds = [float(t) for t in (thresholds or [])]
        connectivity = 8 if connectivity is None else connectivity
        r = V.object_scores(self.gen_imgs, self.eval_imgs, thresholds, relative=relative, mask=self.mask, connectivity=connectivity)
        status = int(r["status"])
        if status != 0:
            raise RuntimeError(f"object_scores: the labelling kernels reported status {status} (a union-find walk hit its step cap); "
                               f"the object statistics of {self.label} are not usable")
        res = {k: r[k].cpu().numpy() for k in V.OBJECT_KEYS if k != "status"}
        names = [f"{t:g}" for t in thresholds] + (["relative"] if relative is not None else [])
        per_thr = []
        a50, a25, a75, a_nan = _nan_quartiles(res["A"])
        for t, name in enumerate(names):
            row = {"threshold": name, "A": {"median": a50, "p25": a25, "p75": a75, "nan": a_nan}}
            for key in ("S", "L"):
                q50, q25, q75, n_nan = _nan_quartiles(res[key][:, t])
                row[key] = {"median": q50, "p25": q25, "p75": q75, "nan": n_nan}
            row["n_objects_gen"], row["n_objects_obs"] = (int(v) for v in res["n_objects"][:, :, t].sum(axis=1))
            row["area_hist_gen"], row["area_hist_obs"] = (res["area_hist"][side, t].tolist() for side in (0, 1))
            per_thr.append(row)
        out = {"thresholds": thresholds, "relative": relative, "connectivity": int(connectivity), "n_fields": self.n_samples,
               "valid": int(res["valid"].sum()), "per_threshold": per_thr,
               "definition": "objects: connected components of the valid pixels with value >= threshold; S = (V_gen - V_obs) / "
                             "(0.5 (V_gen + V_obs)), V = sum_n R_n (R_n / Rmax_n) / sum_n R_n; A = (D_gen - D_obs) / (0.5 (D_gen + "
                             "D_obs)), D the domain mean; L = L1 + L2, L1 = |x_gen - x_obs| / d, L2 = 2 |r_gen - r_obs| / d, r the "
                             "mass-weighted mean distance of the objects' centres from the field's centre x, d the domain diagonal; "
                             "area_hist: objects with floor(log2 area) = bin"}
        self.metrics["objects"] = out
        self.fields.update({f"objects_{k}": v for k, v in res.items()})
        return dict(res, metrics=out)

    def multivariate_statistics(self, energy=None, variogram=None):
        """energy score and variogram score of the `repeated` samples as an ensemble against their one truth: the scalar
        scores go to the metrics entry `multivariate`; the distance matrix `energy_dist2` and the variogram's `vs_map`,
        `gamma_ens`, `gamma_obs`, `offsets` and `pairs` go to a file of their own, <label>_multivariate.npz, which save() writes
        beside the fields file.  Arguments default to the evaluation.multivariate_scores section."""
        self._need_ensemble("multivariate_statistics")
        if energy is None and variogram is None:
            sec = multivariate_scores_config(self.cfg)
            if sec is None:
                raise ValueError("no energy / variogram given and the config has no evaluation.multivariate_scores section")
            energy, variogram = sec
        mask = None if self.mask is None else self.mask[0]
        out, res = {"M": self.n_samples}, {}
        if energy:
            r = V.energy_scores(self.gen_imgs, self.eval_imgs[0], mask=mask)
            s = r["scores"].cpu().numpy()
            out["energy"] = dict(zip(V.ENERGY_KEYS, (float(v) for v in s)))
            out["energy"]["count"] = int(s[0])
            out["energy"]["definition"] = ("es_fair = (1/M) sum_m |x_m - y| - 1/(2 M (M-1)) sum_{m != k} |x_m - x_k|; es_standard "
                                           "with 1/(2 M^2); |a - b| = sqrt(sum over the valid pixels of (a - b)^2 / count)")
            res["energy_dist2"] = r["dist2"].cpu().numpy()
        if variogram is not None:
            r = V.variogram_scores(self.gen_imgs, self.eval_imgs[0], mask=mask, **variogram)
            s = r["scores"].cpu().numpy()
            out["variogram"] = dict(variogram, **dict(zip(V.VARIOGRAM_KEYS, (float(v) for v in s))))
            out["variogram"]["n_pairs"] = int(s[1])
            out["variogram"]["definition"] = ("vs = sum w (g_obs - g_ens)^2 / sum w over the pixel pairs with offset in the half "
                                              "disc of the radius; g_ens = (1/M) sum_m |x_i^m - x_j^m|^order, g_obs = |y_i - "
                                              "y_j|^order; w = 1 / distance or 1")
            res.update({f"variogram_{k}": r[k].cpu().numpy() for k in ("vs_map", "gamma_ens", "gamma_obs", "offsets", "pairs")})
        self.metrics["multivariate"] = out
        self.multivariate_fields = res
        return dict(res, metrics=out)

    def climate_statistics(self, wet=None, quantiles=None, wet_quantiles=None, calendar_aware=None, groups=None):
        """per-pixel climate indices along the day axis of the generated fields against their truth ('multiple' or 'series':
        one truth per day), once per member.  The maps go to a file of their own, <label>_climate.npz, which save() writes: the
        obs maps `obs_<index>`, the gen maps `gen_<index>` stacked over the members [M, ...], `days`, the levels and `wet`.  The
        metrics entry `climate` holds, per float index and level, the domain means, bias, RMSE and pattern correlation per
        member with their mean, minimum and maximum over the members.  With several members a day is valid only where every
        member is a number, so `days` and the obs maps hold for all of them.  Arguments default to the evaluation.climate_indices
        section.  The order-dependent indices are computed in file order (see `definition`).
        `calendar_aware` (evaluation.climate_indices.calendar; default: true when the series has dates) makes a gap in the
        dates end spells, transitions and lag-1 pairs; true without dates is an error.  `groups` (None, "season", "month", ids
        or a .npy path; the two names need dates) adds the same indices per group of days: `groups`, `group_names`,
        `group_days`, `group_obs_<index>` [G, ...] and `group_gen_<index>` [M, G, ...] in the file, and `calendar`,
        `n_links_broken` and `groups` = [{name, n_days, indices}] in the metrics entry."""
        if self.generated_sample_type not in TIME_AXIS_TYPES:
            raise ValueError(f"climate_statistics needs one truth per day ('multiple' or 'series' samples), not "
                             f"'{self.generated_sample_type}'")
        if wet is None and quantiles is None and wet_quantiles is None:
            sec = climate_indices_config(self.cfg)
            if sec is None:
                raise ValueError("no wet / quantiles / wet_quantiles given and the config has no evaluation.climate_indices section")
            wet, quantiles, wet_quantiles = sec
        cfg_calendar, cfg_groups = climate_calendar_config(self.cfg)
        calendar_aware = cfg_calendar if calendar_aware is None else bool(calendar_aware)
        groups = cfg_groups if groups is None else groups
        if calendar_aware and self.dates is None:
            raise ValueError(f"evaluation.climate_indices.calendar is true but {self.label} has no dates (no `dates` in its "
                             f"series_index file)")
        calendar_aware = self.dates is not None if calendar_aware is None else calendar_aware
        wet = 1.0 if wet is None else float(wet)
        quantiles, wet_quantiles = [float(q) for q in (quantiles or [])], [float(q) for q in (wet_quantiles or [])]
        if self.eval_imgs.shape[0] != self.gen_imgs.shape[0]:
            raise ValueError(f"climate_statistics needs as many truths as days; {self.label} has {self.eval_imgs.shape[0]} for "
                             f"{self.gen_imgs.shape[0]}")
        members = self.members if self.members is not None else self.gen_imgs[None]
        # validity is paired with the truth; with several members a day also has to be a number in every member, so that `days` and
        # the obs maps are the same for all of them
        mask = self.mask
        if members.shape[0] > 1:
            finite = ~torch.isnan(members).any(dim=0)
            if not bool(finite.all()):
                mask = (finite if mask is None else mask.bool() & finite).to(torch.uint8)
        D = int(self.gen_imgs.shape[0])
        gids, names = self._day_groups("evaluation.climate_indices.groups", groups, D)
        dn = self.dates if calendar_aware else None
        runs = []
        for gen in members:
            r = V.climate_indices(gen, self.eval_imgs, wet, quantiles, wet_quantiles, mask=mask, day_numbers=dn, groups=gids)
            runs.append({k: v.cpu().numpy() for k, v in r.items()})
        res = {"days": runs[0]["days"], "wet": np.float64(wet), "quantile_levels": np.asarray(quantiles, np.float64),
               "wet_quantile_levels": np.asarray(wet_quantiles, np.float64), "members": np.int64(len(runs))}
        for k in V.CLIMATE_FLOAT_KEYS + V.CLIMATE_INT_KEYS:
            res[f"obs_{k}"] = runs[0][f"obs_{k}"]
            res[f"gen_{k}"] = np.stack([r[f"gen_{k}"] for r in runs])
        levels = {"quantiles": quantiles, "wet_quantiles": wet_quantiles, "heavy_fraction": wet_quantiles}

        def summary(pick):
            """per index and level: the pattern summary of every member's map against the obs map; pick(map) selects the slab"""
            indices = {}
            for k in V.CLIMATE_FLOAT_KEYS:
                for j, name in enumerate([f"{k}_{q:g}" for q in levels[k]] if k in levels else [k]):
                    sel = (lambda a: a[j]) if k in levels else (lambda a: a)
                    indices[name] = _members_summary([sel(pick(r, f"gen_{k}")) for r in runs], sel(pick(runs[0], f"obs_{k}")))
            return indices

        out = {"wet": wet, "quantile_levels": quantiles, "wet_quantile_levels": wet_quantiles, "members": len(runs),
               "n_days": D, "pixels": int((res["days"] > 0).sum()), "indices": summary(lambda r, k: r[k]),
               "definition": CLIMATE_DEFINITION}
        if self.dates is not None:
            res["dates"] = np.asarray(self.dates, np.int64)
        if calendar_aware or gids is not None:
            out["calendar"] = bool(calendar_aware)
            out["n_links_broken"] = int((~calendar.links(self.dates)[1:]).sum()) if calendar_aware else 0
            out["definition"] = CLIMATE_DEFINITION + CLIMATE_CALENDAR_DEFINITION
        if gids is not None:
            res["groups"], res["group_names"] = np.asarray(gids, np.int64), np.asarray(names)
            res["group_days"] = runs[0]["group_days"]
            for k in V.CLIMATE_FLOAT_KEYS + V.CLIMATE_INT_KEYS:
                res[f"group_obs_{k}"] = runs[0][f"group_obs_{k}"]
                res[f"group_gen_{k}"] = np.stack([r[f"group_gen_{k}"] for r in runs])
            out["groups"] = [{"name": names[g], "n_days": gids.count(g), "indices": summary(lambda r, k, g=g: r[f"group_{k}"][g])}
                             for g in range(max(gids) + 1)]
        self.metrics["climate"] = out
        self.climate_fields = res
        return dict(res, metrics=out)

    def period_statistics(self, windows=None, thresholds=None, wet=None, periods=None, min_days=None, calendar_aware=None):
        """period climate indices (RxNday, RNNmm, PRCPTOT) along the day axis of the generated fields against their truth
        ('multiple' or 'series': one truth per day), over the record and per period, all members in one call.  The maps go to a
        file of their own, <label>_periods.npz, which save() writes: every key of verification.period_indices with the gen maps
        [M, ...], `windows`, `thresholds`, `wet`, `min_days`, `members` and, when there are any, `dates`, `periods` and
        `period_names`.  The metrics entry `period_indices` holds, per index (rx_<K>, count_<T>, prcptot) the pattern summary
        of the model's record map against the truth's and, with periods, of its period_mean and period_std maps, per member and
        as mean, minimum and maximum over the members.  Arguments default to the evaluation.period_indices section; `periods`
        is None, "year", "season_year", "month_year" (these need dates), ids in -1..255 or a .npy path."""
        if self.generated_sample_type not in TIME_AXIS_TYPES:
            raise ValueError(f"period_statistics needs one truth per day ('multiple' or 'series' samples), not "
                             f"'{self.generated_sample_type}'")
        sec = period_indices_config(self.cfg)
        if sec is None and windows is None:
            raise ValueError("no windows given and the config has no evaluation.period_indices section")
        sec = sec if sec is not None else ([1, 5], [], 1.0, None, 1, None)
        windows, thresholds, wet, periods, min_days, calendar_aware = (
            d if a is None else a for a, d in zip((windows, thresholds, wet, periods, min_days, calendar_aware), sec))
        key = "evaluation.period_indices"
        if calendar_aware and self.dates is None:
            raise ValueError(f"{key}.calendar is true but {self.label} has no dates (no `dates` in its series_index file)")
        calendar_aware = self.dates is not None if calendar_aware is None else bool(calendar_aware)
        D = int(self.gen_imgs.shape[0])
        if self.eval_imgs.shape[0] != D:
            raise ValueError(f"period_statistics needs as many truths as days; {self.label} has {self.eval_imgs.shape[0]} for {D}")
        names = None
        if isinstance(periods, str) and periods in calendar.PERIODS:
            if self.dates is None:
                raise ValueError(f"{key}.periods: '{periods}' needs the dates of the series; {self.label} has none (no `dates` in "
                                 f"its series_index file)")
            periods, names = calendar.periods_from_dates(self.dates, periods)
        elif isinstance(periods, str):
            periods = np.load(periods)
        if periods is not None:
            periods = np.asarray(periods)
            if periods.ndim != 1 or periods.dtype.kind not in "iu":
                raise ValueError(f"{key}.periods must hold one integer id per day, got shape {periods.shape} of {periods.dtype}")
            if len(periods) != D:
                raise ValueError(f"{key}.periods holds {len(periods)} ids; {self.label} has {D} days")
            periods = [int(g) for g in periods]
            names = names if names is not None else [str(g) for g in range(max(periods) + 1)]
        windows, thresholds = [int(k) for k in windows], [float(t) for t in thresholds]
        members = self.members if self.members is not None else self.gen_imgs[None]
        r = V.period_indices(members, self.eval_imgs, windows, thresholds, float(wet), mask=self.mask,
                             day_numbers=self.dates if calendar_aware else None, periods=periods, min_days=int(min_days))
        res = {k: v.cpu().numpy() for k, v in r.items()}
        M = int(members.shape[0])
        res.update(windows=np.asarray(windows, np.int64), thresholds=np.asarray(thresholds, np.float64), wet=np.float64(wet),
                   min_days=np.int64(min_days), members=np.int64(M))
        if self.dates is not None:
            res["dates"] = np.asarray(self.dates, np.int64)
        with_periods = "period_days" in res
        if with_periods:
            res["periods"], res["period_names"] = np.asarray(periods, np.int64), np.asarray(names)

        indices = {}
        levels = {"rx": [f"rx_{k}" for k in windows], "count": [f"count_{t:g}" for t in thresholds], "prcptot": ["prcptot"]}
        for k in V.PERIOD_INDICES:
            for j, name in enumerate(levels[k]):
                sel = (lambda a: a) if k == "prcptot" else (lambda a, j=j: a[..., j, :, :])
                entry = {"record": _members_summary(sel(res[f"gen_{k}"]), sel(res[f"obs_{k}"]))}
                if with_periods:
                    for stat in ("period_mean", "period_std"):
                        entry[stat] = _members_summary(sel(res[f"gen_{stat}_{k}"]), sel(res[f"obs_{stat}_{k}"]))
                indices[name] = entry
        out = {"windows": windows, "thresholds": thresholds, "wet": float(wet), "min_days": int(min_days), "members": M, "n_days": D,
               "pixels": int((res["days"] > 0).sum()), "calendar": bool(calendar_aware),
               "n_links_broken": int((~calendar.links(self.dates)[1:]).sum()) if calendar_aware else 0,
               "n_periods": len(names) if with_periods else 0, "period_names": list(names) if with_periods else [],
               "indices": indices, "definition": PERIOD_DEFINITION}
        self.metrics["period_indices"] = out
        self.period_fields = res
        return dict(res, metrics=out)

    def series_ensemble_statistics(self, thresholds=None, climatology=None, groups=None, seed=None):
        """pooled ensemble verification of a 'series' (D days of M >= 2 members, one truth per day) over days x pixels: CRPS,
        spread and skill maps, daily and pooled scores, rank histogram, reliability table with the Brier scores, and the CRPS
        skill score against the leave-one-out climatology, pooled and per group of days.  The arrays go to a file of their own,
        <label>_series_scores.npz, which save() writes; the metrics entry is `series_ensemble`.  Arguments default to the
        evaluation.series_scores section; `groups` is one id in 0..15 per day (a list, an array or a .npy path)."""
        if self.generated_sample_type != "series":
            raise ValueError(f"series_ensemble_statistics needs 'series' samples (days x members), not '{self.generated_sample_type}'")
        if thresholds is None and climatology is None and groups is None and seed is None:
            sec = series_scores_config(self.cfg)
            if sec is None:
                raise ValueError("no arguments given and the config has no evaluation.series_scores section")
            thresholds, climatology, groups, seed = sec
        M, D = int(self.members.shape[0]), int(self.members.shape[1])
        if M < 2:
            raise ValueError(f"series_ensemble_statistics needs at least 2 members; {self.label} has {M}: generate with "
                             f"evaluation.series.members >= 2")
        if self.eval_imgs.shape[0] != D:
            raise ValueError(f"series_ensemble_statistics needs as many truths as days; {self.label} has {self.eval_imgs.shape[0]} for {D}")
        thresholds = [float(t) for t in (thresholds or [])]
        climatology = True if climatology is None else bool(climatology)
        seed = int(self.cfg["evaluation"].get("seed", 0)) if seed is None else int(seed)
        groups, _ = self._day_groups("evaluation.series_scores.groups", groups, D)
        r = V.series_ensemble_scores(self.members.permute(1, 0, 2, 3), self.eval_imgs, thresholds, groups=groups, mask=self.mask,
                                     seed=seed, climatology=climatology)
        res = {k: r[k].cpu().numpy() for k in V.SERIES_KEYS}
        res["thresholds"] = np.asarray(thresholds, np.float64)
        res["groups"] = np.asarray([] if groups is None else groups, np.int64)

        def row(i):
            s, h = res["scores"][i], res["rank_hist"][i].astype(np.float64)
            n = h.sum()
            out = dict(zip(V.ENSEMBLE_KEYS, (float(v) for v in s)))
            out["count"] = int(s[0])
            out["rank_reliability_index"] = float(np.abs(h / n - 1.0 / (M + 1)).sum()) if n > 0 else float("nan")
            out["outside_fraction"] = float((h[0] + h[M]) / n) if n > 0 else float("nan")
            out.update({k: res["exceedance"][i, j].tolist() for j, k in enumerate(V.EXCEEDANCE_KEYS)})
            bs, unc = res["exceedance"][i, 0], res["exceedance"][i, 3]
            with np.errstate(divide="ignore", invalid="ignore"):
                out["brier_skill"] = np.where(unc > 0, 1.0 - bs / unc, np.nan).tolist()
            if climatology:                  # over the cells of the pixels with >= 3 valid days in the row, a subset of `count`
                out["climatology"] = dict(zip(V.SERIES_SKILL_KEYS, (float(v) for v in res["skill_scores"][i])))
                out["climatology"]["cells"] = int(res["skill_scores"][i, 0])
                out["crpss"] = out["climatology"]["crpss"]
            return out

        G = res["scores"].shape[0] - 1
        out = {"M": M, "D": D, "thresholds": thresholds, "climatology": climatology, "rank_seed": seed, "n_groups": G,
               "pixels": int((res["count"] > 0).sum()), "pooled": row(0), "groups": [row(1 + g) for g in range(G)],
               "crps_definitions": CRPS_DEFINITIONS, "definition": SERIES_DEFINITION}
        out["crpss"] = out["pooled"].get("crpss", float("nan"))
        self.metrics["series_ensemble"] = out
        self.series_fields = res
        return dict(res, metrics=out)

    def save(self):
        """<label>_metrics.json and <label>_fields.npz under the statistics directory; returns their paths.  After
        multivariate_statistics also <label>_multivariate.npz, after climate_statistics also <label>_climate.npz, after
        series_ensemble_statistics also <label>_series_scores.npz, after period_statistics also <label>_periods.npz."""
        if getattr(self, "series_fields", None):
            np.savez(os.path.join(self.evaluation_stats_path, f"{self.label}_series_scores.npz"), **self.series_fields)
        if getattr(self, "period_fields", None):
            np.savez(os.path.join(self.evaluation_stats_path, f"{self.label}_periods.npz"), **self.period_fields)
        if getattr(self, "climate_fields", None):
            np.savez(os.path.join(self.evaluation_stats_path, f"{self.label}_climate.npz"), **self.climate_fields)
        if getattr(self, "multivariate_fields", None):
            np.savez(os.path.join(self.evaluation_stats_path, f"{self.label}_multivariate.npz"), **self.multivariate_fields)
        mpath = os.path.join(self.evaluation_stats_path, f"{self.label}_metrics.json")
        fpath = os.path.join(self.evaluation_stats_path, f"{self.label}_fields.npz")
        with open(mpath, "w") as f:
            json.dump(self.metrics, f, indent=2, default=float)
        np.savez(fpath, **self.fields)
        logger.info(f"[INFO] Saved {mpath} and {fpath}")
        return mpath, fpath
