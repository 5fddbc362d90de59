"""`evaluation_main(cfg)` — reference sbgm/evaluate_sbgm/evaluation_main.py:45-111: seed from evaluation.seed, then for every
generation type in evaluation.eval_gen_type (default: evaluation.gen_type, then ['multiple']) run the methods of
evaluation.eval_stat_methods (default ['pixel_stats', 'spatial_stats'], as in the reference) and write each unit's
`<type>[_rank<r>]_metrics.json` / `_fields.npz`.  Plotting keys are accepted and logged as skipped.  An
`evaluation.spatial_scores` section (thresholds, scales) adds the neighbourhood scores for every type and the exceedance
scores for `repeated`; an `evaluation.ensemble_products` section (quantiles, thresholds) adds the ensemble products for
`repeated`; an `evaluation.object_scores` section (thresholds, relative, connectivity) adds the object-based scores (SAL) for
every type; an `evaluation.multivariate_scores` section (energy, variogram) adds the energy and variogram scores for
`repeated` (their arrays go to `<type>[_rank<r>]_multivariate.npz`; for another type the section is logged as skipped); an
`evaluation.climate_indices` section (wet, quantiles, wet_quantiles) adds the per-pixel climate indices along the day axis for
`multiple` and `series` (their maps go to `<type>_climate.npz`; for `single` and `repeated` it is logged as skipped); an
`evaluation.series_scores` section (thresholds, climatology, groups, seed) adds the pooled ensemble verification of a `series`
over days x pixels (its arrays go to `series_series_scores.npz`; for another type it is logged as skipped); an
`evaluation.period_indices` section (windows, thresholds, wet, periods, min_days, calendar) adds the period climate indices
(RxNday, RNNmm, PRCPTOT per year, season or month of a year, and their mean and spread across those) for `multiple` and `series`
(their maps go to `<type>_periods.npz`; for `single` and `repeated` it is logged as skipped); without
a section its statistics do not run and the output files hold what they always held."""
from __future__ import annotations

import os

import numpy as np
import torch

from ..training_utils import setup_logger
from ..utils import get_model_string
from .evaluation import (GEN_TYPES, TIME_AXIS_TYPES, Evaluation, climate_indices_config, ensemble_products_config, multivariate_scores_config, object_scores_config,
                         period_indices_config, sample_units, series_scores_config, spatial_scores_config)

# statistic -> (method of Evaluation, config function of the section that switches it on or None, for 'repeated' only).
# Without a config function the statistic is one evaluation.eval_stat_methods may list; with one it runs, without arguments
# (it reads its section), after those and in this order whenever the section is there.  'climate_stats' is no ensemble statistic
# but needs one truth per day, as 'period_stats' does: TIME_AXIS_STATISTICS keeps them to 'multiple' and 'series'.  'series_ensemble_stats' needs days x
# members: SERIES_STATISTICS keeps it to 'series'.
STATISTICS = {
    "pixel_stats": ("full_pixel_statistics", None, False),
    "spatial_stats": ("spatial_statistics", None, False),
    "daily_stats": ("daily_statistics", None, False),
    "ensemble_stats": ("ensemble_statistics", None, False),
    "spectral_stats": ("spectral_statistics", None, False),
    "neighbourhood_stats": ("neighbourhood_statistics", spatial_scores_config, False),
    "exceedance_stats": ("exceedance_statistics", spatial_scores_config, True),
    "product_stats": ("product_statistics", ensemble_products_config, True),
    "object_stats": ("object_statistics", object_scores_config, False),
    "multivariate_stats": ("multivariate_statistics", multivariate_scores_config, True),
    "climate_stats": ("climate_statistics", climate_indices_config, False),
    "period_stats": ("period_statistics", period_indices_config, False),
    "series_ensemble_stats": ("series_ensemble_statistics", series_scores_config, False),
}
# statistics along the day axis: they need one truth per day, which 'multiple' and 'series' have
TIME_AXIS_STATISTICS = ("climate_stats", "period_stats")
# statistics over days x members: only a 'series' has both
SERIES_STATISTICS = ("series_ensemble_stats",)


def _methods_of(config):
    """{statistic: method} of the table's rows with this config function"""
    return {name: method for name, (method, c, _) in STATISTICS.items() if c is config}


# views of the table: the names evaluation.eval_stat_methods may list, and the statistics of each section
METHODS = _methods_of(None)
SPATIAL_METHODS, PRODUCT_METHODS = _methods_of(spatial_scores_config), _methods_of(ensemble_products_config)
OBJECT_METHODS, MULTIVARIATE_METHODS = _methods_of(object_scores_config), _methods_of(multivariate_scores_config)
CLIMATE_METHODS = _methods_of(climate_indices_config)
PERIOD_METHODS = _methods_of(period_indices_config)
SERIES_METHODS = _methods_of(series_scores_config)
PLOT_KEYS = ("plot_examples", "save_figs", "show_plots", "show_figs", "mask_plots", "plot_w_cond", "plot_w_lsm")


def eval_gen_types(cfg):
    ev = cfg["evaluation"]
    types = list(ev.get("eval_gen_type") or ev.get("gen_type") or ["multiple"])
    for t in types:
        if t not in GEN_TYPES:
            raise ValueError(f"Invalid generated sample type: {t}. Must be one of {list(GEN_TYPES)}")
    return types


def eval_stat_methods(cfg):
    methods = list(cfg["evaluation"].get("eval_stat_methods") or ["pixel_stats", "spatial_stats"])
    for m in methods:
        if m not in METHODS:
            raise ValueError(f"Invalid evaluation method: {m}. Must be one of {list(METHODS)}")
    return methods


def unit_statistics(cfg, gen_type):
    """the statistics evaluate mode runs for one generation type, in order: evaluation.eval_stat_methods, then — only with an
    evaluation.spatial_scores section — 'neighbourhood_stats' and, for 'repeated', 'exceedance_stats'; then — only with an
    evaluation.ensemble_products section, for 'repeated' — 'product_stats'; then — only with an evaluation.object_scores
    section — 'object_stats'; then — only with an evaluation.multivariate_scores section, for 'repeated' —
    'multivariate_stats'; then — only with an evaluation.climate_indices section, for 'multiple' and 'series' —
    'climate_stats'; then — only with an evaluation.period_indices section, for 'multiple' and 'series' — 'period_stats';
    then — only with an evaluation.series_scores section, for 'series' — 'series_ensemble_stats'"""
    stats = eval_stat_methods(cfg)
    for name, (_, config, ensemble_only) in STATISTICS.items():
        if name in TIME_AXIS_STATISTICS and gen_type not in TIME_AXIS_TYPES:
            continue
        if name in SERIES_STATISTICS and gen_type != "series":
            continue
        if config is not None and config(cfg) is not None and (gen_type == "repeated" or not ensemble_only):
            stats.append(name)
    return stats


def n_samples_of(cfg, gen_type):
    ev = cfg["evaluation"]
    return {"multiple": ev.get("batch_size"), "single": 1, "repeated": ev.get("n_repeats"), "series": None}[gen_type]


def evaluation_main(cfg):
    """returns {unit label: metrics dict}"""
    ev = cfg["evaluation"]
    seed = int(ev.get("seed", 0))
    torch.manual_seed(seed)
    torch.cuda.manual_seed(seed)
    np.random.seed(seed)
    types = eval_gen_types(cfg)
    methods = {t: unit_statistics(cfg, t) for t in types}             # all validated before any file is read
    model_name_str = get_model_string(cfg)
    log = setup_logger(os.path.join(cfg["paths"]["sample_dir"], "generation", model_name_str, "logs"), name="eval_log")
    skipped = [k for k in PLOT_KEYS if ev.get(k, False)]
    if skipped:
        log.info(f"[INFO] Plotting is not part of this evaluation; skipped: {skipped}")
    sample_dir = os.path.join(cfg["paths"]["sample_dir"], "generation", model_name_str, "generated_samples")
    # a section all of whose statistics are for 'repeated' only does nothing for another type: say so
    for config in dict.fromkeys(c for _, c, _ in STATISTICS.values() if c is not None):
        if all(only for _, c, only in STATISTICS.values() if c is config) and config(cfg) is not None:
            for t in types:
                if t != "repeated":
                    log.info(f"[INFO] evaluation.{config.__name__[:-len('_config')]} needs 'repeated' samples (an ensemble); "
                             f"skipped for '{t}'")
    if climate_indices_config(cfg) is not None:
        for t in types:
            if t not in TIME_AXIS_TYPES:
                log.info(f"[INFO] evaluation.climate_indices needs one truth per day ('multiple' or 'series' samples); skipped for '{t}'")
    if period_indices_config(cfg) is not None:
        for t in types:
            if t not in TIME_AXIS_TYPES:
                log.info(f"[INFO] evaluation.period_indices needs one truth per day ('multiple' or 'series' samples); skipped for '{t}'")
    if series_scores_config(cfg) is not None:
        for t in types:
            if t != "series":
                log.info(f"[INFO] evaluation.series_scores needs 'series' samples (days x members); skipped for '{t}'")
    out = {}
    for gen_type in types:
        n = n_samples_of(cfg, gen_type)
        for rank, _ in sample_units(sample_dir, gen_type, n):
            runner = Evaluation(cfg, generated_sample_type=gen_type, n_samples=n, rank=rank)
            log.info(f"[INFO] Running evaluation for {runner.label}")
            for method in methods[gen_type]:
                log.info(f"[INFO] Running evaluation method: {method}")
                fn = getattr(runner, STATISTICS[method][0])
                if method in ("pixel_stats", "spatial_stats"):
                    fn(save_stats=bool(ev.get("save_stats", False)), n_samples=n if n is not None else runner.n_samples)
                else:
                    fn()
            runner.save()
            out[runner.label] = runner.metrics
    log.info("[INFO] Evaluation completed for all generated sample types")
    return out
