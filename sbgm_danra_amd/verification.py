"""Device-tensor wrappers of the verification kernels (csrc/verify.hip, csrc/verify_spatial.hip, csrc/verify_products.hip,
csrc/verify_objects.hip, csrc/verify_multivariate.hip and csrc/verify_temporal.hip, their shared helpers in csrc/verify_common.h): error
statistics, histograms, ensemble scores (CRPS, rank histogram, spread/skill), radially averaged power spectra, neighbourhood scores (Fractions Skill Score), threshold-exceedance scores (Brier, reliability
table, ROC area), ensemble products (per-pixel mean, spread, envelope, quantile and exceedance-probability maps) and
object-based scores (connected objects and SAL: structure, amplitude, location) and multivariate ensemble scores (energy score,
variogram score) and per-pixel climate indices along the day axis (wet-day frequency and intensity, spells, transitions,
lag-1 autocorrelation, quantiles, heavy-rain fraction), period climate indices (csrc/verify_periods.hip: RxNday, RNNmm and PRCPTOT
over the record and per year, their mean and spread across the years) and pooled ensemble scores of a series over days x pixels (csrc/verify_series.hip:
CRPS and spread/skill maps, rank histogram, reliability table, climatological CRPS skill score, per group of days).  Every function takes tensors on
the ROCm device and returns tensors on the device; arguments and shapes are checked before any launch and nothing is copied
to the host.  A pixel is valid when gen (every member) and obs are not NaN and the mask admits it (uint8/bool != 0, or float
> 0.5); every statistic uses the valid pixels only."""
from __future__ import annotations

import torch

import ctypes as C
import math

from . import _native as N

GLOBAL_KEYS = ("count", "mean_gen", "mean_obs", "bias", "mae", "rmse", "min_gen", "max_gen", "min_obs", "max_obs")
ENSEMBLE_KEYS = ("count", "crps_fair", "crps_standard", "skill", "spread", "spread_skill_ratio")
NEIGHBOURHOOD_KEYS = ("num", "den", "events_gen", "events_obs", "valid", "fss", "fss_field", "freq_bias", "fss_useful")
EXCEEDANCE_KEYS = ("brier", "brier_reliability", "brier_resolution", "brier_uncertainty", "base_rate", "roc_area")
MAX_THRESHOLDS = MAX_SCALES = 16                 # include/sbgm_hip.h: SBGM_SPATIAL_MAX_THRESHOLDS / _SCALES
MAX_FIELDS, MAX_FIELD_SIDE, MAX_FIELD_PIXELS = 65535, 2048, 1 << 20        # csrc/verify_common.h
MAX_EXCEEDANCE_MEMBERS = MAX_PRODUCT_MEMBERS = MAX_MULTIVARIATE_MEMBERS = 4095
MAX_PRODUCT_QUANTILES = 16                       # include/sbgm_hip.h: SBGM_PRODUCTS_MAX_QUANTILES; thresholds: MAX_THRESHOLDS
DEFAULT_WORKSPACE_BYTES = 256 << 20
OBJECT_KEYS = ("threshold", "n_objects", "area", "mass", "V", "r", "domain_mean", "com", "valid", "S", "L2", "A", "L1", "L",
               "area_hist", "status")               # the argument order of sbgm_object_scores
OBJECT_AREA_BINS = 21                            # include/sbgm_hip.h: SBGM_OBJECTS_AREA_BINS; fixed thresholds: MAX_THRESHOLDS
ENERGY_KEYS = ("count", "es_fair", "es_standard", "mean_dist_obs", "mean_dist_pair", "min_dist_pair")
VARIOGRAM_KEYS = ("vs", "n_pairs", "sum_w", "vs_unweighted")
MAX_VARIOGRAM_RADIUS, MAX_VARIOGRAM_OFFSETS = 8, 98    # include/sbgm_hip.h: SBGM_VARIOGRAM_MAX_OFFSETS
VARIOGRAM_ORDERS = (0.5, 1.0, 2.0)
VARIOGRAM_WEIGHTS = ("inverse_distance", "unit")
MAX_TEMPORAL_DAYS, MAX_TEMPORAL_QUANTILES = 4095, 8    # include/sbgm_hip.h: SBGM_TEMPORAL_MAX_DAYS / _QUANTILES
CLIMATE_STATS = ("mean", "wet_freq", "sdii", "max", "p_ww", "p_dw", "lag1")      # the order of SBGM_TEMPORAL_STAT_*
CLIMATE_FLOAT_KEYS = CLIMATE_STATS + ("quantiles", "wet_quantiles", "heavy_fraction")
CLIMATE_INT_KEYS = ("cwd", "cdd", "transitions")
MAX_SERIES_GROUPS, MAX_SERIES_MEMBERS = 16, 4095        # include/sbgm_hip.h: SBGM_SERIES_MAX_GROUPS; days: MAX_TEMPORAL_DAYS
# include/sbgm_hip.h: SBGM_PERIOD_MAX_WINDOWS / _WINDOW / _THRESHOLDS / _PERIODS / _MEMBERS
MAX_PERIOD_WINDOWS, MAX_PERIOD_WINDOW, MAX_PERIOD_THRESHOLDS, MAX_PERIODS, MAX_PERIOD_MEMBERS = 4, 32, 8, 256, 4095
PERIOD_INDICES = ("rx", "count", "prcptot")
SERIES_MAP_KEYS = ("crps", "spread", "skill", "ssr")
SERIES_CLIM_MAP_KEYS = ("clim_crps", "crpss")
SERIES_SKILL_KEYS = ("cells", "crps_fair", "crps_reference", "crpss")
SERIES_KEYS = (("count",) + SERIES_MAP_KEYS + ("daily", "scores", "rank_hist", "table", "exceedance") + SERIES_CLIM_MAP_KEYS +
               ("skill_scores",))


def _rows(t, name, HW, allowed):
    """t viewed as fp32-or-mask [rows, HW] with rows in `allowed`"""
    if t.dim() < 2 or t[0].numel() != HW:
        raise ValueError(f"{name}: shape {tuple(t.shape)} does not hold fields of {HW} pixels")
    r = t.shape[0]
    if r not in allowed:
        raise ValueError(f"{name}: {r} fields; expected one of {sorted(set(allowed))}")
    return r


def _fields(x, name):
    """[N, H, W] (or [H, W] as one field) -> contiguous fp32 [N, H*W]"""
    N.require_device(x)
    if x.dim() == 2:
        x = x.unsqueeze(0)
    if x.dim() != 3:
        raise ValueError(f"{name}: expected [N, H, W] or [H, W], got {tuple(x.shape)}")
    if not x.is_floating_point():
        raise TypeError(f"{name}: expected a floating tensor, got {x.dtype}")
    return N.f32c(x).view(x.shape[0], -1)


def _mask(mask, HW, allowed):
    """(pointer-holding tensor, is_u8, rows) of an optional mask"""
    if mask is None:
        return None, 0, 1
    N.require_device(mask)
    if mask.dim() == 2:
        mask = mask.unsqueeze(0)
    if mask.dtype == torch.bool:
        mask = mask.to(torch.uint8)
    if mask.dtype == torch.uint8:
        m, u8 = mask.contiguous(), 1
    elif mask.is_floating_point():
        m, u8 = N.f32c(mask), 0
    else:
        raise TypeError(f"mask: expected uint8, bool or float, got {mask.dtype}")
    return m, u8, _rows(m, "mask", HW, allowed)


def _ws(nbytes, device):
    return torch.empty(max(int(nbytes), 8), dtype=torch.uint8, device=device)


def error_stats(gen, obs, mask=None):
    """gen [N,H,W] against obs [No,H,W] (No in {1, N}), optional mask [Nm,H,W] (Nm in {1, N}).  Returns a dict of device tensors:
    per pixel over samples `count` (int32), `mae`, `rmse`, `bias` [H,W]; per sample over pixels `sample_count`, `sample_mae`,
    `sample_rmse` [N] (fp64); and `global` fp64 [10] in GLOBAL_KEYS order."""
    shape = gen.shape[-2:]
    g = _fields(gen, "gen")
    n, HW = g.shape
    o = _fields(obs, "obs")
    _rows(o, "obs", HW, (1, n))
    if o.device != g.device:
        raise ValueError("gen and obs must be on the same device")
    m, u8, nm = _mask(mask, HW, (1, n))
    dev = g.device
    out = dict(count=torch.empty(HW, dtype=torch.int32, device=dev), mae=torch.empty(HW, device=dev),
               rmse=torch.empty(HW, device=dev), bias=torch.empty(HW, device=dev))
    smp = torch.empty(n, 3, dtype=torch.float64, device=dev)
    glob = torch.empty(10, dtype=torch.float64, device=dev)
    ws = _ws(N.lib().sbgm_error_stats_workspace_bytes(n, HW), dev)
    N.check(N.lib().sbgm_error_stats(g.data_ptr(), o.data_ptr(), N.ptr(m), u8, n, o.shape[0], nm, HW, out["count"].data_ptr(),
                                     out["mae"].data_ptr(), out["rmse"].data_ptr(), out["bias"].data_ptr(), smp.data_ptr(),
                                     glob.data_ptr(), ws.data_ptr(), N.stream()))
    out = {k: v.view(shape) for k, v in out.items()}
    out.update(sample_count=smp[:, 0], sample_mae=smp[:, 1], sample_rmse=smp[:, 2], **{"global": glob})
    return out


def histogram(x, bins, lo, hi, ref=None, mask=None, absdiff=False):
    """int64 [bins] counts of x [N,H,W] (or of |x - ref| with absdiff) over its valid pixels in `bins` equal bins on [lo, hi]:
    v is kept iff lo <= v <= hi, idx = floor((v - lo) * bins / (hi - lo)) in fp64, clamped so v == hi lands in the last bin
    (numpy.histogram's range and closed-last-bin convention with the floor rule; numpy's extra correction against its edges
    can move a value within rounding of an interior edge by one bin).  ref [Nr,H,W] (Nr in {1, N}) also decides validity:
    a NaN ref pixel is dropped."""
    xs = _fields(x, "x")
    n, HW = xs.shape
    r = None
    if ref is not None:
        r = _fields(ref, "ref")
        _rows(r, "ref", HW, (1, n))
    elif absdiff:
        raise ValueError("histogram: absdiff needs ref")
    bins, lo, hi = int(bins), float(lo), float(hi)
    if not 1 <= bins <= 8192:
        raise ValueError(f"histogram: bins={bins} outside 1..8192")
    if not (lo < hi) or lo in (float("inf"), float("-inf")) or hi in (float("inf"), float("-inf")):
        raise ValueError(f"histogram: bad range [{lo}, {hi}]")
    m, u8, nm = _mask(mask, HW, (1, n))
    counts = torch.empty(bins, dtype=torch.int64, device=xs.device)
    N.check(N.lib().sbgm_histogram(xs.data_ptr(), N.ptr(r), N.ptr(m), u8, n, 1 if r is None else r.shape[0], nm, HW,
                                   int(bool(absdiff)), lo, hi, bins, counts.data_ptr(), N.stream()))
    return counts


def histogram_edges(bins, lo, hi):
    """the bin edges histogram() uses (numpy.linspace(lo, hi, bins + 1)), fp64 on the host side of the caller's choosing"""
    return torch.linspace(float(lo), float(hi), int(bins) + 1, dtype=torch.float64)


def ensemble_scores(ens, obs, mask=None, seed=0):
    """members ens [M,H,W] (M >= 2) against truth obs [H,W], optional mask [H,W].  Returns device tensors: per pixel `mean`,
    `var` (ddof 1), `crps` (fair) [H,W] fp32 and `rank` int32 [H,W] (-1 where invalid; ties broken by a Philox draw keyed by
    (seed, pixel)); `rank_hist` int64 [M+1]; `scores` fp64 [6] in ENSEMBLE_KEYS order."""
    shape = ens.shape[-2:]
    e = _fields(ens, "ens")
    M, HW = e.shape
    if M < 2 or M > 8191:
        raise ValueError(f"ensemble_scores: M={M} members; need 2..8191")
    o = _fields(obs, "obs")
    _rows(o, "obs", HW, (1,))
    m, u8, _ = _mask(mask, HW, (1,))
    dev = e.device
    mean, var, crps = (torch.empty(HW, device=dev) for _ in range(3))
    rank = torch.empty(HW, dtype=torch.int32, device=dev)
    rank_hist = torch.empty(M + 1, dtype=torch.int64, device=dev)
    scores = torch.empty(6, dtype=torch.float64, device=dev)
    ws = _ws(N.lib().sbgm_ensemble_scores_workspace_bytes(HW), dev)
    N.check(N.lib().sbgm_ensemble_scores(e.data_ptr(), o.data_ptr(), N.ptr(m), u8, M, HW, int(seed) & (2**64 - 1), mean.data_ptr(),
                                         var.data_ptr(), crps.data_ptr(), rank.data_ptr(), rank_hist.data_ptr(), scores.data_ptr(),
                                         ws.data_ptr(), N.stream()))
    return dict(mean=mean.view(shape), var=var.view(shape), crps=crps.view(shape), rank=rank.view(shape), rank_hist=rank_hist,
                scores=scores)


def rapsd(fields):
    """radially averaged power spectral density of fields [F,H,W] (each mean-removed, then |torch.fft.fft2|^2), averaged over the
    fields.  A field holding a NaN cannot be transformed: it is skipped and counted.  Returns (wavenumbers int64 [L//2+1],
    psd fp64 [L//2+1], n_skipped int64 scalar), L = max(H, W); bin k holds the pixels with round(L * |f|) == k, f in cycles
    per pixel (numpy.fft.fftfreq), so corners beyond L//2 are dropped."""
    x = _fields(fields, "fields").view(-1, *fields.shape[-2:])
    F, H, W = x.shape
    if min(H, W) < 2 or max(H, W) > 2048:
        raise ValueError(f"rapsd: field size {H}x{W}; sides must be 2..2048")
    ok = ~torch.isnan(x).flatten(1).any(dim=1)
    x = torch.where(ok[:, None, None], x, torch.zeros((), device=x.device))
    x = x - x.mean(dim=(1, 2), keepdim=True)
    power = torch.fft.fft2(x).abs().square().float().contiguous()
    okb = ok.to(torch.uint8).contiguous()
    nb = max(H, W) // 2 + 1
    psd = torch.empty(nb, dtype=torch.float64, device=x.device)
    cnt = torch.empty(nb, dtype=torch.int64, device=x.device)
    nf = torch.empty(1, dtype=torch.int64, device=x.device)
    ws = _ws(N.lib().sbgm_radial_spectrum_workspace_bytes(H, W), x.device)
    N.check(N.lib().sbgm_radial_spectrum(power.data_ptr(), okb.data_ptr(), F, H, W, psd.data_ptr(), cnt.data_ptr(), nf.data_ptr(),
                                         ws.data_ptr(), N.stream()))
    return torch.arange(nb, device=x.device), psd, F - nf[0]


def _thresholds(thresholds, name):
    """1..16 finite thresholds as a host float array (fp32: the comparison is `v >= thr` in fp32)"""
    thr = [float(t) for t in thresholds]
    if not 1 <= len(thr) <= MAX_THRESHOLDS:
        raise ValueError(f"{name}: {len(thr)} thresholds; need 1..{MAX_THRESHOLDS}")
    arr = (C.c_float * len(thr))(*thr)
    if not all(math.isfinite(t) and math.isfinite(a) for t, a in zip(thr, arr)):
        raise ValueError(f"{name}: thresholds must be finite in fp32, got {thr}")
    return arr


def _scales(scales, name):
    """1..16 odd window widths >= 1 as a host int array"""
    sc = list(scales)
    if not 1 <= len(sc) <= MAX_SCALES:
        raise ValueError(f"{name}: {len(sc)} window widths; need 1..{MAX_SCALES}")
    for n in sc:
        if isinstance(n, bool) or int(n) != n or int(n) < 1 or int(n) % 2 == 0 or int(n) >= 2**31:
            raise ValueError(f"{name}: window widths must be odd integers >= 1, got {sc}")
    return (C.c_int * len(sc))(*(int(n) for n in sc))


def _shape_rows(t, name, hw, allowed):
    """shape check of an optional [rows, H, W] (or [H, W]) argument, before anything touches the device"""
    if t is None:
        return
    shape = tuple(t.shape)
    if len(shape) == 2:
        shape = (1,) + shape
    if len(shape) != 3 or shape[1:] != tuple(hw):
        raise ValueError(f"{name}: shape {tuple(t.shape)} does not hold fields of {hw[0]}x{hw[1]} pixels")
    if shape[0] not in allowed:
        raise ValueError(f"{name}: {shape[0]} fields; expected one of {sorted(set(allowed))}")


def _field_shape(x, name, what):
    """(N, H, W) of the fields `what` = x [N,H,W] of the function `name`, within the limits of the chunked scores"""
    if x.dim() != 3:
        raise ValueError(f"{what}: expected [N, H, W], got {tuple(x.shape)}")
    n, H, W = x.shape
    if not (2 <= H <= MAX_FIELD_SIDE and 2 <= W <= MAX_FIELD_SIDE) or H * W > MAX_FIELD_PIXELS:
        raise ValueError(f"{name}: field size {H}x{W}; sides must be 2..{MAX_FIELD_SIDE} and H*W <= 2^20")
    if not 1 <= n <= MAX_FIELDS:
        raise ValueError(f"{name}: {n} fields; need 1..{MAX_FIELDS}")
    return n, H, W


def _paired(name, gen, obs, mask, what="gen"):
    """paired fields: gen [N,H,W] within the field limits, obs [No,H,W] (None: no second side) and mask [Nm,H,W] with No, Nm in
    {1, N}, all shapes checked before anything touches the device -> (gen [N, HW], obs [No, HW] or None, mask, is_u8, Nm)"""
    n, H, W = _field_shape(gen, name, what)
    _shape_rows(obs, "obs", (H, W), (1, n))
    _shape_rows(mask, "mask", (H, W), (1, n))
    g = _fields(gen, what)
    o = None
    if obs is not None:
        o = _fields(obs, "obs")
        if o.device != g.device:
            raise ValueError("gen and obs must be on the same device")
    return (g, o) + _mask(mask, H * W, (1, n))


def _members(name, ens, max_members):
    """(M, H, W) of an ensemble ens [M,H,W] with 2 <= M <= max_members"""
    if ens.dim() != 3:
        raise ValueError(f"ens: expected [M, H, W], got {tuple(ens.shape)}")
    M, H, W = ens.shape
    if not 2 <= M <= max_members:
        raise ValueError(f"{name}: M={M} members; need 2..{max_members}")
    return M, H, W


def _ensemble(name, ens, obs, mask, max_members, max_pixels=None, strict=False):
    """ensemble: ens [M,H,W] with 2 <= M <= max_members (and 1 <= H*W <= max_pixels, if given), obs [H,W] (None: no truth) and
    mask [H,W], all shapes checked before anything touches the device -> (ens [M, HW], obs [1, HW] or None, mask, is_u8).
    strict: ens and a given obs must also be floating before they are converted, and on one device."""
    M, H, W = _members(name, ens, max_members)
    if max_pixels is not None and (H < 1 or W < 1 or H * W > max_pixels):
        raise ValueError(f"{name}: field size {H}x{W}; need H*W in 1..2^20")
    _shape_rows(obs, "obs", (H, W), (1,))
    _shape_rows(mask, "mask", (H, W), (1,))
    if strict and obs is not None and not (ens.is_floating_point() and obs.is_floating_point()):
        raise TypeError(f"{name}: ens and obs must be floating tensors, got {ens.dtype} and {obs.dtype}")
    e = _fields(ens, "ens")
    o = None if obs is None else _fields(obs, "obs")
    if strict and o is not None and o.device != e.device:
        raise ValueError("ens and obs must be on the same device")
    m, u8, _ = _mask(mask, H * W, (1,))
    return e, o, m, u8


def neighbourhood_strip_columns():
    """columns one workgroup of the neighbourhood window pass owns (fields wider than this are walked in several strips)"""
    return int(N.lib().sbgm_neighbourhood_scores_strip_columns())


def neighbourhood_scores(gen, obs, thresholds, scales, mask=None, max_workspace_bytes=DEFAULT_WORKSPACE_BYTES):
    """Fractions Skill Score (Roberts & Lean 2008) ingredients of gen [N,H,W] against obs [No,H,W] (No in {1, N}), optional
    mask [Nm,H,W] (Nm in {1, N}), for T thresholds (event: v >= thr in fp32 at a valid pixel) and S odd window widths n.
    With C_g, C_o the event counts in the n x n window around each of the H*W centres (zero beyond the domain, never
    renormalised): `num` = sum (C_g - C_o)^2 and `den` = sum (C_g^2 + C_o^2), int64 [N,T,S], exact; `events_gen`, `events_obs`
    int64 [N,T]; `valid` int64 [N]; `fss_field` fp64 [N,T,S] = 1 - num/den; `fss` fp64 [T,S] = 1 - sum_f num / sum_f den (NaN
    where den is 0); `freq_bias` fp64 [T] = sum events_gen / sum events_obs; `fss_useful` fp64 [T] = 0.5 + f_o/2 with f_o the
    observed event frequency.  The fields are processed in chunks whose workspace stays within `max_workspace_bytes` (at
    least one field x one threshold); the result does not depend on the chunking."""
    thr, sc = _thresholds(thresholds, "neighbourhood_scores"), _scales(scales, "neighbourhood_scores")
    g, o, m, u8, nm = _paired("neighbourhood_scores", gen, obs, mask)
    (n, H, W), T, S, dev = gen.shape, len(thr), len(sc), g.device
    i64 = dict(dtype=torch.int64, device=dev)
    f64 = dict(dtype=torch.float64, device=dev)
    out = dict(num=torch.empty(n, T, S, **i64), den=torch.empty(n, T, S, **i64), events_gen=torch.empty(n, T, **i64),
               events_obs=torch.empty(n, T, **i64), valid=torch.empty(n, **i64), fss=torch.empty(T, S, **f64),
               fss_field=torch.empty(n, T, S, **f64), freq_bias=torch.empty(T, **f64), fss_useful=torch.empty(T, **f64))
    nbytes = N.lib().sbgm_neighbourhood_scores_workspace_bytes(n, H, W, T, S, max(int(max_workspace_bytes), 0))
    ws = _ws(nbytes, dev)
    N.check(N.lib().sbgm_neighbourhood_scores(g.data_ptr(), o.data_ptr(), N.ptr(m), u8, n, o.shape[0], nm, H, W, thr, T, sc, S,
                                              *(out[k].data_ptr() for k in NEIGHBOURHOOD_KEYS), ws.data_ptr(), nbytes, N.stream()))
    return out


def exceedance_scores(ens, obs, thresholds, mask=None):
    """threshold-exceedance probability scores of members ens [M,H,W] (2 <= M <= 4095) against truth obs [H,W], optional mask
    [H,W].  A pixel is valid when every member and obs are not NaN there and the mask admits it.  Per threshold and valid
    pixel, k = #{members >= thr} and o = [obs >= thr].  Returns device tensors: `table` int64 [T, M+1, 2] (pixels with that k;
    those of them with o = 1 — the reliability diagram), `count` int64 scalar, and fp64 [T] `brier`, `brier_reliability`,
    `brier_resolution`, `brier_uncertainty` (Murphy's decomposition over the M+1 probabilities p_k = k/M: reliability -
    resolution + uncertainty = brier), `base_rate` and `roc_area` (trapezoids over the M+1 cut-offs; NaN when the event
    never or always occurs), all computed from the table."""
    thr = _thresholds(thresholds, "exceedance_scores")
    e, o, m, u8 = _ensemble("exceedance_scores", ens, obs, mask, MAX_EXCEEDANCE_MEMBERS)
    (M, HW), T, dev = e.shape, len(thr), e.device
    table = torch.empty(T, M + 1, 2, dtype=torch.int64, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    scores = torch.empty(len(EXCEEDANCE_KEYS), T, dtype=torch.float64, device=dev)
    N.check(N.lib().sbgm_exceedance_scores(e.data_ptr(), o.data_ptr(), N.ptr(m), u8, M, HW, thr, T, table.data_ptr(),
                                           count.data_ptr(), scores.data_ptr(), None, N.stream()))
    return dict(table=table, count=count[0], **{k: scores[i] for i, k in enumerate(EXCEEDANCE_KEYS)})


def ensemble_products(ens, quantiles=(), thresholds=(), mask=None):
    """per-pixel products of members ens [M,H,W] (2 <= M <= 4095), optional mask [H,W].  A pixel is valid when no member is NaN
    there and the mask admits it; every map is NaN elsewhere.  Returns device tensors: `mean`, `std` (ddof 1), `min`, `max`
    [H,W] fp32; `quantiles` [Q,H,W], numpy's default (Hyndman-Fan type 7: h = q (M - 1), lo = floor(h), g = h - lo; x_(lo) when
    g == 0 or x_(lo) == x_(hi), else (float)(x_(lo) + g (x_(hi) - x_(lo))) in fp64 — exact order statistics, so q = 0 is
    `min` and q = 1 is `max` bit for bit); `exceed_prob` [T,H,W] = #{members >= thr} / M (comparison in fp32); `count` int64
    scalar, the valid pixels.  Up to 16 quantile levels in [0, 1] and 16 finite thresholds; either list may be empty."""
    _members("ensemble_products", ens, MAX_PRODUCT_MEMBERS)               # the member count first, then the levels
    qs, thr = [float(q) for q in quantiles], list(thresholds)
    if len(qs) > MAX_PRODUCT_QUANTILES:
        raise ValueError(f"ensemble_products: {len(qs)} quantiles; at most {MAX_PRODUCT_QUANTILES}")
    if not all(math.isfinite(q) and 0.0 <= q <= 1.0 for q in qs):
        raise ValueError(f"ensemble_products: quantiles must lie in [0, 1], got {qs}")
    tarr = _thresholds(thr, "ensemble_products") if thr else None
    e, _, m, u8 = _ensemble("ensemble_products", ens, None, mask, MAX_PRODUCT_MEMBERS)
    (M, HW), shape, Q, T, dev = e.shape, tuple(ens.shape[1:]), len(qs), len(thr), e.device
    mean, std, vmin, vmax = (torch.empty(HW, device=dev) for _ in range(4))
    quant, exceed = torch.empty(Q, HW, device=dev), torch.empty(T, HW, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    N.check(N.lib().sbgm_ensemble_products(e.data_ptr(), N.ptr(m), u8, M, HW, (C.c_double * Q)(*qs) if Q else None, Q,
                                           tarr, T, mean.data_ptr(), std.data_ptr(), vmin.data_ptr(), vmax.data_ptr(),
                                           quant.data_ptr() if Q else None, exceed.data_ptr() if T else None, count.data_ptr(), None,
                                           N.stream()))
    return dict(mean=mean.view(shape), std=std.view(shape), min=vmin.view(shape), max=vmax.view(shape),
                quantiles=quant.view(Q, *shape), exceed_prob=exceed.view(T, *shape), count=count[0])


def _connectivity(connectivity, name):
    if isinstance(connectivity, bool) or connectivity not in (4, 8):
        raise ValueError(f"{name}: connectivity must be 4 or 8, got {connectivity!r}")
    return int(connectivity)


def _relative(relative, name):
    """(factor, quantile, wet) of a relative threshold R* = factor * R^quantile over the values >= wet"""
    if not isinstance(relative, dict) or set(relative) != {"factor", "quantile", "wet"}:
        raise ValueError(f"{name}: relative must be a dict with the keys factor, quantile and wet, got {relative!r}")
    vals = [relative[k] for k in ("factor", "quantile", "wet")]
    if any(isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) for v in vals):
        raise ValueError(f"{name}: relative.factor, .quantile and .wet must be finite numbers, got {relative!r}")
    factor, quantile, wet = (float(v) for v in vals)
    if not 0.0 <= quantile <= 1.0 or not math.isfinite(C.c_float(wet).value):
        raise ValueError(f"{name}: relative.quantile must lie in [0, 1] and relative.wet be finite in fp32, got {relative!r}")
    return factor, quantile, wet


def object_labels(fields, threshold, mask=None, connectivity=8, return_status=False):
    """connected objects of fields [N,H,W] (sides 2..2048, H*W <= 2^20), optional mask [Nm,H,W] (Nm in {1, N}): an object pixel
    is a valid pixel (not NaN, admitted by the mask) with `v >= threshold` in fp32, objects are its 4- or 8-connected
    (`connectivity`) components.  Returns int32 [N,H,W] canonical labels: 1 + the smallest linear index row * W + col among the
    pixels of the object, 0 for background.  At most 65535 fields per call.  With return_status also the int32 device scalar
    that is non-zero only if a union-find walk of the kernel hit its step cap (a defect, never an input's fault; the labels are
    then not to be used).  Nothing is copied to the host here, so by default that status is NOT checked: a caller who needs
    to know must pass return_status=True and look at it."""
    conn = _connectivity(connectivity, "object_labels")
    thr = _thresholds([threshold], "object_labels")[0]
    x, _, m, u8, nm = _paired("object_labels", fields, None, mask, what="fields")
    n, H, W = fields.shape
    labels = torch.empty(n, H, W, dtype=torch.int32, device=x.device)
    status = torch.empty(1, dtype=torch.int32, device=x.device)
    N.check(N.lib().sbgm_object_labels(x.data_ptr(), N.ptr(m), u8, n, nm, H, W, thr, conn, labels.data_ptr(), status.data_ptr(),
                                       N.stream()))
    return (labels, status[0]) if return_status else labels


def object_scores(gen, obs, thresholds=(), relative=None, mask=None, connectivity=8, max_workspace_bytes=DEFAULT_WORKSPACE_BYTES):
    """SAL (structure, amplitude, location; Wernli et al. 2008) of gen [N,H,W] against obs [No,H,W] (No in {1, N}), optional mask
    [Nm,H,W] (Nm in {1, N}), N <= 65535; meant for non-negative fields such as precipitation (not checked).  For a side F in {gen, obs} and a
    threshold, objects are the 4- or 8-connected components of the valid pixels with `F >= thr` in fp32.  `thresholds`: up to 16
    finite values, the same on both sides; `relative` = {factor, quantile, wet} adds, as the last threshold index, Wernli's
    R* = factor * R^quantile per side and field: thr = (float)(factor * q), q the type-7 quantile (as ensemble_products defines it)
    of that side's valid values >= wet, NaN (no objects) where there is none.  With T thresholds in all, per object n the area
    a_n, mass R_n = sum F, peak Rmax_n and centre x_n = sum F (row, col) / R_n; per field D = mean of F and x = F-weighted centre
    over the valid pixels; d = sqrt((H-1)^2 + (W-1)^2).  Returns device tensors, index 0 of a leading [2] being gen and 1 obs:
    `threshold` fp32 [2,N,T]; `n_objects`, `area` int64 [2,N,T]; `mass` = sum_n R_n, `V` = sum_n R_n (R_n / Rmax_n) / mass,
    `r` = sum_n R_n |x - x_n| / mass fp64 [2,N,T]; `domain_mean` fp64 [2,N]; `com` fp64 [2,N,2]; `valid` int64 [N];
    `S` = (V_g - V_o) / (0.5 (V_g + V_o)), `L2` = 2 |r_g - r_o| / d, `L` = L1 + L2 fp64 [N,T]; `A` = (D_g - D_o) / (0.5 (D_g + D_o)),
    `L1` = |x_g - x_o| / d fp64 [N] (NaN where a denominator is 0; S, L2 where a side has no object; A, L1 where there is no valid
    pixel or a side sums to 0); `area_hist` int64 [2,T,21], objects with floor(log2 a_n) = b over all fields; `status` int32
    scalar, 0 unless a union-find walk hit its step cap.  The (field, threshold) pairs are processed in chunks whose workspace
    stays within `max_workspace_bytes` (at least one pair); the result does not depend on the chunking, and two calls give
    bit-equal results."""
    conn = _connectivity(connectivity, "object_scores")
    fixed = list(thresholds)
    if len(fixed) > MAX_THRESHOLDS:
        raise ValueError(f"object_scores: {len(fixed)} thresholds; at most {MAX_THRESHOLDS}")
    thr = _thresholds(fixed, "object_scores") if fixed else None
    rel = None if relative is None else _relative(relative, "object_scores")
    T = len(fixed) + (rel is not None)
    if T < 1:
        raise ValueError("object_scores: no threshold given (thresholds is empty and relative is None)")
    g, o, m, u8, nm = _paired("object_scores", gen, obs, mask)
    (n, H, W), dev = gen.shape, g.device
    i64, f64 = dict(dtype=torch.int64, device=dev), dict(dtype=torch.float64, device=dev)
    out = dict(threshold=torch.empty(2, n, T, device=dev), n_objects=torch.empty(2, n, T, **i64), area=torch.empty(2, n, T, **i64),
               mass=torch.empty(2, n, T, **f64), V=torch.empty(2, n, T, **f64), r=torch.empty(2, n, T, **f64),
               domain_mean=torch.empty(2, n, **f64), com=torch.empty(2, n, 2, **f64), valid=torch.empty(n, **i64),
               S=torch.empty(n, T, **f64), L2=torch.empty(n, T, **f64), A=torch.empty(n, **f64), L1=torch.empty(n, **f64),
               L=torch.empty(n, T, **f64), area_hist=torch.empty(2, T, OBJECT_AREA_BINS, **i64),
               status=torch.empty(1, dtype=torch.int32, device=dev))
    nbytes = N.lib().sbgm_object_scores_workspace_bytes(n, H, W, T, max(int(max_workspace_bytes), 0))
    ws = _ws(nbytes, dev)
    factor, quantile, wet = rel if rel is not None else (0.0, 0.0, 0.0)
    N.check(N.lib().sbgm_object_scores(g.data_ptr(), o.data_ptr(), N.ptr(m), u8, n, o.shape[0], nm, H, W, thr, len(fixed),
                                       int(rel is not None), factor, quantile, wet, conn, *(out[k].data_ptr() for k in OBJECT_KEYS),
                                       ws.data_ptr(), nbytes, N.stream()))
    out["status"] = out["status"][0]
    return out


def variogram_offsets(radius):
    """the pixel-pair offsets (dy, dx) of variogram_scores for a radius 1..8, in the kernel's order: the half-plane (dy > 0, or
    dy == 0 and dx > 0) of the disc dy^2 + dx^2 <= radius^2, dy ascending, then dx ascending"""
    if isinstance(radius, bool) or not isinstance(radius, int) or not 1 <= radius <= MAX_VARIOGRAM_RADIUS:
        raise ValueError(f"variogram: radius must be an integer in 1..{MAX_VARIOGRAM_RADIUS}, got {radius!r}")
    return [(dy, dx) for dy in range(radius + 1) for dx in range(-radius, radius + 1)
            if (dy > 0 or dx > 0) and dy * dy + dx * dx <= radius * radius]


def energy_scores(ens, obs, mask=None):
    """energy score (Gneiting et al. 2008) of members ens [M,H,W] (2 <= M <= 4095, H*W <= 2^20) against truth obs [H,W],
    optional mask [H,W].  A pixel is valid when every member and obs are not NaN there and the mask admits it.  Returns device
    tensors: `dist2` fp64 [M+1, M+1], the squared Euclidean distances over the valid pixels between all members and the truth
    (row / column M), accumulated in fp64 from differences (symmetric bit for bit, zero diagonal, an exact 0 between
    duplicated members); `scores` fp64 [6] in ENERGY_KEYS order: count, es_fair = (1/M) sum_m |x_m - y| - 1/(2 M (M-1))
    sum_{m != k} |x_m - x_k|, es_standard (the same with 1/(2 M^2)), mean_dist_obs, mean_dist_pair and min_dist_pair, every
    norm |a - b| = sqrt(dist2 / count), an RMS distance.  No valid pixel gives count 0 and NaN scores.  Two calls give
    bit-equal results."""
    e, o, m, u8 = _ensemble("energy_scores", ens, obs, mask, MAX_MULTIVARIATE_MEMBERS, MAX_FIELD_PIXELS, strict=True)
    M, HW = e.shape
    dev = e.device
    dist2 = torch.empty(M + 1, M + 1, dtype=torch.float64, device=dev)
    scores = torch.empty(len(ENERGY_KEYS), dtype=torch.float64, device=dev)
    nbytes = N.lib().sbgm_energy_scores_workspace_bytes(M, HW)
    ws = _ws(nbytes, dev)
    N.check(N.lib().sbgm_energy_scores(e.data_ptr(), o.data_ptr(), N.ptr(m), u8, M, HW, dist2.data_ptr(), scores.data_ptr(),
                                       ws.data_ptr(), nbytes, N.stream()))
    return dict(dist2=dist2, scores=scores)


def variogram_scores(ens, obs, radius=4, order=0.5, weights="inverse_distance", mask=None):
    """variogram score of order p = `order` (Scheuerer & Hamill 2015) of members ens [M,H,W] (2 <= M <= 4095, H*W <= 2^20)
    against truth obs [H,W], optional mask [H,W], over the pixel pairs (i, j = i + (dy, dx)) of variogram_offsets(radius) with
    both pixels valid and inside the field.  Per pair g_ens = (1/M) sum_m |x_i^m - x_j^m|^p, g_obs = |y_i - y_j|^p (difference
    and power in fp32, sums in fp64) and term = (g_obs - g_ens)^2; w = 1 / sqrt(dy^2 + dx^2) for weights "inverse_distance", 1
    for "unit".  order is 0.5, 1 or 2; radius 1..8.  Returns device tensors: `vs_map` fp32 [H,W], each pixel's sum of w term
    over its own pairs (NaN at an invalid pixel); `offsets` int32 [n_off, 2]; `gamma_ens`, `gamma_obs` fp64 [n_off], the
    domain-mean variograms per offset (NaN without pairs); `pairs` int64 [n_off]; `scores` fp64 [4] in VARIOGRAM_KEYS order:
    vs = sum w term / sum w, n_pairs, sum_w, vs_unweighted = sum term / n_pairs.  Two calls give bit-equal results."""
    offsets = variogram_offsets(radius)
    if isinstance(order, bool) or not isinstance(order, (int, float)) or float(order) not in VARIOGRAM_ORDERS:
        raise ValueError(f"variogram_scores: order must be one of {VARIOGRAM_ORDERS}, got {order!r}")
    if weights not in VARIOGRAM_WEIGHTS:
        raise ValueError(f"variogram_scores: weights must be one of {VARIOGRAM_WEIGHTS}, got {weights!r}")
    e, o, m, u8 = _ensemble("variogram_scores", ens, obs, mask, MAX_MULTIVARIATE_MEMBERS, MAX_FIELD_PIXELS, strict=True)
    M, (H, W) = e.shape[0], ens.shape[1:]
    dev, n_off = e.device, len(offsets)
    f64 = dict(dtype=torch.float64, device=dev)
    vs_map = torch.empty(H, W, device=dev)
    gamma_ens, gamma_obs = torch.empty(n_off, **f64), torch.empty(n_off, **f64)
    pairs = torch.empty(n_off, dtype=torch.int64, device=dev)
    scores = torch.empty(len(VARIOGRAM_KEYS), **f64)
    nbytes = N.lib().sbgm_variogram_scores_workspace_bytes(M, H, W, radius)
    ws = _ws(nbytes, dev)
    N.check(N.lib().sbgm_variogram_scores(e.data_ptr(), o.data_ptr(), N.ptr(m), u8, M, H, W, radius, float(order),
                                          int(weights == "inverse_distance"), vs_map.data_ptr(), gamma_ens.data_ptr(),
                                          gamma_obs.data_ptr(), pairs.data_ptr(), scores.data_ptr(), ws.data_ptr(), nbytes, N.stream()))
    return dict(vs_map=vs_map, offsets=torch.tensor(offsets, dtype=torch.int32, device=dev), gamma_ens=gamma_ens,
                gamma_obs=gamma_obs, pairs=pairs, scores=scores)


def _levels(levels, name):
    """at most 8 quantile levels in [0, 1] as a host double array (None when empty)"""
    qs = [float(q) for q in levels]
    if len(qs) > MAX_TEMPORAL_QUANTILES:
        raise ValueError(f"climate_indices: {len(qs)} {name}; at most {MAX_TEMPORAL_QUANTILES}")
    if not all(math.isfinite(q) and 0.0 <= q <= 1.0 for q in qs):
        raise ValueError(f"climate_indices: {name} must lie in [0, 1], got {qs}")
    return qs, ((C.c_double * len(qs))(*qs) if qs else None)


def climate_indices(gen, obs, wet=1.0, quantiles=(), wet_quantiles=(), mask=None, day_numbers=None, groups=None):
    """per-pixel climate indices along the day axis of gen [N,H,W] against obs [N,H,W], both fp32 (2 <= N <= 4095; sides 2..2048,
    H*W <= 2^20), optional mask [H,W] or [N,H,W] (uint8/bool != 0, or fp32 > 0.5).  Day t is valid at a pixel when gen and obs
    are both not NaN there and the mask admits it — paired, so both sides use the same days; a valid day is wet on a side when
    its value is >= wet (fp32), else dry.  Returns a dict of device tensors, every float map fp32 and NaN where undefined, each
    index for both sides as `gen_<name>` and `obs_<name>`: `days` int32 [H,W] (n, the valid days; one map); `mean`; `wet_freq`
    = n_wet / n; `sdii` = sum over the wet days / n_wet; `max`; `cwd`, `cdd` int32, the longest run of consecutive valid wet
    (dry) days, an invalid day ending a run; `transitions` int32 [4,H,W] = n_ww, n_wd, n_dw, n_dd over the adjacent pairs of
    valid days; `p_ww` = n_ww / (n_ww + n_wd), `p_dw` = n_dw / (n_dw + n_dd); `lag1` = c1 / c0 with c0 = sum (x - mu)^2 / n and
    c1 = sum over the pairs (x_t - mu)(x_t+1 - mu) / n_pairs; `quantiles` [Q,H,W], numpy's default (type 7) over the n valid
    days; `wet_quantiles` [QW,H,W], the same over the valid wet days; `heavy_fraction` [QW,H,W] = sum over the valid days with
    x > tau of x / sum over the valid wet days of x, tau the OBS side's wet_quantiles map for both sides (ETCCDI R95pTOT for
    level 0.95).  Sums are fp64 in day order (the order of axis 0), rounded to fp32 once; two calls give bit-equal results.
    At most 8 levels in [0, 1] in each list; either may be empty.  cwd, cdd, transitions, p_ww, p_dw and lag1 depend on the day
    order and mean something only for consecutive days at a fixed location.
    `day_numbers`: one integer per day, strictly increasing (checked on the host; calendar.day_numbers gives them for dates).
    Day t is linked to day t - 1 iff day_numbers[t] == day_numbers[t-1] + 1; None links every adjacent pair.  A broken link
    acts exactly as one invalid day inserted between the two days: it ends a wet or dry run, and no transition and no lag-1
    product spans it; it counts nowhere else (not in n, the sums, the quantiles or heavy_fraction).
    `groups`: a group id in 0..15 per day (a sequence or an integer tensor; G = the largest id + 1), e.g. the season.  The
    indices of group g are the calendar-aware indices of the subsequence of days with id g, which keeps its own day numbers
    (positions without `day_numbers`), so a link is also broken where consecutive days of the group are not consecutive days
    of the record; the group has its own mean in `lag1` and its own obs wet-day quantile map as tau of `heavy_fraction`.  The
    dict then gains `group_days` int32 [G,H,W] and `group_<side>_<name>` with a leading [G] axis for every index.  A group of
    0 or 1 days is legal: its maps follow the rules for n = 0 or n = 1.  With both None every key keeps its bits; a grouped
    call sweeps the record twice where the plain call sweeps it once, whatever G is (measured: 1.45 - 1.58 plain calls with four
    seasons at 589 x 789)."""
    for name, x in (("gen", gen), ("obs", obs)):
        if x.dim() != 3:
            raise ValueError(f"{name}: expected [N, H, W], got {tuple(x.shape)}")
        if x.dtype != torch.float32:
            raise TypeError(f"{name}: expected a float32 tensor, got {x.dtype}")
    n, H, W = _field_shape(gen, "climate_indices", "gen")
    if not 2 <= n <= MAX_TEMPORAL_DAYS:
        raise ValueError(f"climate_indices: N={n} days; need 2..{MAX_TEMPORAL_DAYS}")
    if tuple(obs.shape) != (n, H, W):
        raise ValueError(f"obs: shape {tuple(obs.shape)} does not match gen {(n, H, W)}")
    _shape_rows(mask, "mask", (H, W), (1, n))
    if mask is not None and not (mask.dtype in (torch.uint8, torch.bool) or mask.is_floating_point()):
        raise TypeError(f"mask: expected uint8, bool or float, got {mask.dtype}")
    if isinstance(wet, bool) or not isinstance(wet, (int, float)) or not math.isfinite(wet) or not math.isfinite(C.c_float(wet).value):
        raise ValueError(f"climate_indices: wet must be a number finite in fp32, got {wet!r}")
    (qs, qarr), (qw, qwarr) = _levels(quantiles, "quantiles"), _levels(wet_quantiles, "wet_quantiles")
    dn = _day_numbers(day_numbers, n)
    gids, G = _series_groups(groups, n, "climate_indices")
    g, o = _fields(gen, "gen"), _fields(obs, "obs")
    if o.device != g.device:
        raise ValueError("gen and obs must be on the same device")
    m, u8, nm = _mask(mask, H * W, (1, n))
    Q, QW, HW, dev = len(qs), len(qw), H * W, g.device
    i32 = dict(dtype=torch.int32, device=dev)
    # every output as [1 + G, ...]: row 0 is the record, row 1 + g is group g
    days, spells, trans = torch.empty(1 + G, HW, **i32), torch.empty(1 + G, 2, 2, HW, **i32), torch.empty(1 + G, 2, 4, HW, **i32)
    stats = torch.empty(1 + G, 2, len(CLIMATE_STATS), HW, device=dev)
    quant, wquant, heavy = (torch.empty(1 + G, 2, k, HW, device=dev) for k in (Q, QW, QW))
    dn_dev = None if dn is None else torch.tensor(dn, dtype=torch.int32, device=dev)
    g_dev = None if gids is None else torch.tensor(gids, dtype=torch.int32, device=dev)
    ptr = lambda t, row, have=True: t[row].data_ptr() if have and row < 1 + G else None              # noqa: E731
    if dn is None and gids is None:
        nbytes = N.lib().sbgm_climate_indices_workspace_bytes(n, H, W, Q, QW)
        ws = _ws(nbytes, dev)
        N.check(N.lib().sbgm_climate_indices(g.data_ptr(), o.data_ptr(), N.ptr(m), u8, n, nm, H, W, float(wet), qarr, Q, qwarr, QW,
                                             days.data_ptr(), stats.data_ptr(), spells.data_ptr(), trans.data_ptr(),
                                             ptr(quant, 0, Q), ptr(wquant, 0, QW), ptr(heavy, 0, QW), ws.data_ptr(), nbytes,
                                             N.stream()))
    else:
        nbytes = N.lib().sbgm_climate_calendar_workspace_bytes(n, H, W, Q, QW, G)
        ws = _ws(nbytes, dev)
        N.check(N.lib().sbgm_climate_indices_calendar(
            g.data_ptr(), o.data_ptr(), N.ptr(m), u8, n, nm, H, W, float(wet), qarr, Q, qwarr, QW, N.ptr(dn_dev), N.ptr(g_dev), G,
            days.data_ptr(), stats.data_ptr(), spells.data_ptr(), trans.data_ptr(), ptr(quant, 0, Q), ptr(wquant, 0, QW),
            ptr(heavy, 0, QW), ptr(days, 1), ptr(stats, 1), ptr(spells, 1), ptr(trans, 1), ptr(quant, 1, Q), ptr(wquant, 1, QW),
            ptr(heavy, 1, QW), ws.data_ptr(), nbytes, N.stream()))

    def maps(pre, rows, lead):
        r = {}
        for s, side in enumerate(("gen", "obs")):
            r.update({f"{pre}{side}_{k}": stats[rows, s, i].view(*lead, H, W) for i, k in enumerate(CLIMATE_STATS)})
            r.update({f"{pre}{side}_cwd": spells[rows, s, 0].view(*lead, H, W), f"{pre}{side}_cdd": spells[rows, s, 1].view(*lead, H, W),
                      f"{pre}{side}_transitions": trans[rows, s].view(*lead, 4, H, W),
                      f"{pre}{side}_quantiles": quant[rows, s].view(*lead, Q, H, W),
                      f"{pre}{side}_wet_quantiles": wquant[rows, s].view(*lead, QW, H, W),
                      f"{pre}{side}_heavy_fraction": heavy[rows, s].view(*lead, QW, H, W)})
        return r

    out = {"days": days[0].view(H, W)}
    out.update(maps("", 0, ()))
    if G:
        out["group_days"] = days[1:].view(G, H, W)
        out.update(maps("group_", slice(1, None), (G,)))
    return out


def _day_numbers(day_numbers, n):
    """host int list of the optional day numbers relative to the first (they must fit int32), or None"""
    if day_numbers is None:
        return None
    from .calendar import day_numbers as normalise
    if isinstance(day_numbers, torch.Tensor):
        day_numbers = day_numbers.cpu().numpy()
    dn = normalise(day_numbers)
    if dn.shape[0] != n:
        raise ValueError(f"climate_indices: {dn.shape[0]} day numbers for N={n} days")
    dn = dn - dn[0]
    if int(dn[-1]) >= 2 ** 31 - 1:
        raise ValueError(f"climate_indices: the day numbers span {int(dn[-1])} days; they must fit int32")
    return dn.tolist()


def _series_groups(groups, D, name="series_ensemble_scores"):
    """(host int list or None, G) of the optional group ids, one per day, each in 0..15; G = the largest id + 1"""
    if groups is None:
        return None, 0
    if isinstance(groups, torch.Tensor):
        if groups.dim() != 1 or groups.is_floating_point() or groups.dtype == torch.bool:
            raise ValueError(f"groups: expected a 1-D integer tensor, got {tuple(groups.shape)} of {groups.dtype}")
        groups = groups.tolist()
    groups = list(groups)
    if any(isinstance(g, bool) or int(g) != g for g in groups):
        raise ValueError(f"{name}: groups must be integers, got {groups}")
    groups = [int(g) for g in groups]
    if len(groups) != D:
        raise ValueError(f"{name}: {len(groups)} group ids for D={D} days")
    if min(groups) < 0 or max(groups) >= MAX_SERIES_GROUPS:
        raise ValueError(f"{name}: group ids must lie in 0..{MAX_SERIES_GROUPS - 1} (G <= {MAX_SERIES_GROUPS}), got "
                         f"{min(groups)}..{max(groups)}")
    return groups, max(groups) + 1


def series_ensemble_scores(ens, obs, thresholds=(), groups=None, mask=None, seed=0, climatology=True,
                           max_workspace_bytes=DEFAULT_WORKSPACE_BYTES):
    """pooled ensemble verification of a series: members ens with logical dims [D,M,H,W] (1 <= D <= 4095 days, 2 <= M <= 4095)
    against one truth per day obs [D,H,W], optional mask [H,W] or [D,H,W], pooled over days x pixels.  Any fp32 view of ens whose
    last two dims are dense (such as a permuted [M,D,H,W] tensor) is passed by its strides; anything else is copied.  A cell
    (d, p) is valid when the truth and every member are not NaN there and the mask admits it.  `groups`: a group id in 0..15 per
    day (a sequence or an integer tensor; G = the largest id + 1), e.g. the season; row 0 of every [G+1] axis below is all days,
    row 1 + g is group g.  Up to 16 finite `thresholds`, or none.  Returns a dict of device tensors: `count` int32 [H,W], the valid
    days n_p; fp32 [H,W] maps, NaN where n_p = 0: `crps` (mean fair CRPS over the days), `spread` = sqrt(mean var), `skill` =
    sqrt(mean (mean - y)^2), `ssr` = sqrt((M+1)/M) spread / skill; `daily` fp64 [D,6] and `scores` fp64 [G+1,6] in ENSEMBLE_KEYS
    order (each day's valid pixels; the row's valid cells); `rank_hist` int64 [G+1,M+1] of the randomised ranks (ties broken by
    a Philox draw keyed by (seed, day, pixel): day 0 draws what ensemble_scores draws); `table` int64 [G+1,T,M+1,2] and
    `exceedance` fp64 [G+1,6,T] in EXCEEDANCE_KEYS order, exceedance_scores' table and scores per row.  With `climatology` the
    reference forecast for a day is the leave-one-out ensemble of the truth on the other valid days of the same row at that
    pixel, scored with the same fair CRPS (it needs n >= 3 days): `clim_crps` fp32 [H,W], its mean over the days; `crpss` fp32
    [H,W] = 1 - F_p / C_p of the per-pixel sums (NaN where n_p < 3 or C_p = 0); `skill_scores` fp64 [G+1,4] in
    SERIES_SKILL_KEYS order over the cells of the pixels with n >= 3 in that row; without it the three hold NaN.  The days are
    worked through in chunks whose workspace stays within `max_workspace_bytes` (at least 32 days); the result does not depend
    on the chunking, and two calls give bit-equal results."""
    name = "series_ensemble_scores"
    if ens.dim() != 4:
        raise ValueError(f"ens: expected [D, M, H, W], got {tuple(ens.shape)}")
    if obs.dim() != 3:
        raise ValueError(f"obs: expected [D, H, W], got {tuple(obs.shape)}")
    if not (ens.is_floating_point() and obs.is_floating_point()):
        raise TypeError(f"{name}: ens and obs must be floating tensors, got {ens.dtype} and {obs.dtype}")
    D, M, H, W = ens.shape
    if not (2 <= H <= MAX_FIELD_SIDE and 2 <= W <= MAX_FIELD_SIDE) or H * W > MAX_FIELD_PIXELS:
        raise ValueError(f"{name}: field size {H}x{W}; sides must be 2..{MAX_FIELD_SIDE} and H*W <= 2^20")
    if not 1 <= D <= MAX_TEMPORAL_DAYS:
        raise ValueError(f"{name}: D={D} days; need 1..{MAX_TEMPORAL_DAYS}")
    if not 2 <= M <= MAX_SERIES_MEMBERS:
        raise ValueError(f"{name}: M={M} members; need 2..{MAX_SERIES_MEMBERS}")
    if tuple(obs.shape) != (D, H, W):
        raise ValueError(f"obs: shape {tuple(obs.shape)} does not match ens days and fields {(D, H, W)}")
    _shape_rows(mask, "mask", (H, W), (1, D))
    if mask is not None and not (mask.dtype in (torch.uint8, torch.bool) or mask.is_floating_point()):
        raise TypeError(f"mask: expected uint8, bool or float, got {mask.dtype}")
    thr = list(thresholds)
    if len(thr) > MAX_THRESHOLDS:
        raise ValueError(f"{name}: {len(thr)} thresholds; at most {MAX_THRESHOLDS}")
    tarr = _thresholds(thr, name) if thr else None
    gids, G = _series_groups(groups, D)
    if isinstance(seed, bool) or not isinstance(seed, int):
        raise TypeError(f"{name}: seed must be an integer, got {seed!r}")
    N.require_device(ens, obs)
    if obs.device != ens.device:
        raise ValueError("ens and obs must be on the same device")
    e = ens if ens.dtype == torch.float32 else ens.float()
    HW = H * W
    if e.stride(3) != 1 or e.stride(2) != W or e.stride(0) < HW or e.stride(1) < HW:
        e = e.contiguous()
    o = _fields(obs, "obs")
    m, u8, nm = _mask(mask, HW, (1, D))
    T, dev, clim = len(thr), e.device, bool(climatology)
    g = None if gids is None else torch.tensor(gids, dtype=torch.int32, device=dev)
    f64, i64 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int64, device=dev)
    count = torch.empty(HW, dtype=torch.int32, device=dev)
    maps = torch.empty(len(SERIES_MAP_KEYS), HW, device=dev)
    daily, scores = torch.empty(D, len(ENSEMBLE_KEYS), **f64), torch.empty(G + 1, len(ENSEMBLE_KEYS), **f64)
    rank_hist, table = torch.empty(G + 1, M + 1, **i64), torch.empty(G + 1, T, M + 1, 2, **i64)
    exceedance = torch.empty(G + 1, len(EXCEEDANCE_KEYS), T, **f64)
    clim_maps = torch.full((len(SERIES_CLIM_MAP_KEYS), HW), float("nan"), device=dev)
    skill = torch.full((G + 1, len(SERIES_SKILL_KEYS)), float("nan"), **f64)
    nbytes = N.lib().sbgm_series_scores_workspace_bytes(D, M, H, W, T, G, int(clim), max(int(max_workspace_bytes), 0))
    ws = _ws(nbytes, dev)
    N.check(N.lib().sbgm_series_scores(e.data_ptr(), e.stride(0), e.stride(1), o.data_ptr(), N.ptr(m), u8, nm, N.ptr(g), G, D, M, H, W,
                                       tarr, T, seed & (2**64 - 1), int(clim), count.data_ptr(), maps.data_ptr(), daily.data_ptr(),
                                       scores.data_ptr(), rank_hist.data_ptr(), table.data_ptr() if T else None,
                                       exceedance.data_ptr() if T else None, clim_maps.data_ptr(), skill.data_ptr(), ws.data_ptr(),
                                       nbytes, N.stream()))
    out = dict(count=count.view(H, W), daily=daily, scores=scores, rank_hist=rank_hist, table=table, exceedance=exceedance,
               skill_scores=skill)
    out.update({k: maps[i].view(H, W) for i, k in enumerate(SERIES_MAP_KEYS)})
    out.update({k: clim_maps[i].view(H, W) for i, k in enumerate(SERIES_CLIM_MAP_KEYS)})
    return out


def _period_ids(periods, n):
    """(host int list or None, P) of the optional period ids, one per day, each in -1..255; P = the largest id + 1"""
    if periods is None:
        return None, 0
    if isinstance(periods, torch.Tensor):
        if periods.dim() != 1 or periods.is_floating_point() or periods.dtype == torch.bool:
            raise ValueError(f"periods: expected a 1-D integer tensor, got {tuple(periods.shape)} of {periods.dtype}")
        periods = periods.tolist()
    periods = list(periods)
    if any(isinstance(g, bool) or int(g) != g for g in periods):
        raise ValueError(f"period_indices: periods must be integers, got {periods}")
    periods = [int(g) for g in periods]
    if len(periods) != n:
        raise ValueError(f"period_indices: {len(periods)} period ids for N={n} days")
    if min(periods) < -1 or max(periods) >= MAX_PERIODS:
        raise ValueError(f"period_indices: period ids must lie in -1..{MAX_PERIODS - 1} (P <= {MAX_PERIODS}), got "
                         f"{min(periods)}..{max(periods)}")
    P = max(periods) + 1
    return (periods, P) if P > 0 else (None, 0)                  # every day outside every period: as without periods


def period_indices(gen, obs, windows=(1, 5), thresholds=(), wet=1.0, mask=None, day_numbers=None, periods=None, min_days=1):
    """multi-day accumulation and threshold-count indices (ETCCDI RxNday, RNNmm, PRCPTOT) per pixel along the day axis, over
    the record and per period, for gen [N,H,W] or [M,N,H,W] (M members, read by their strides: any fp32 view whose last two
    dims are dense is not copied) against obs [N,H,W], both fp32 (2 <= N <= 4095; sides 2..2048, H*W <= 2^20), optional mask
    [H,W] or [N,H,W] by the rules of climate_indices.  `windows`: 1 to 4 distinct ascending lengths in 1..32; `thresholds`: 0
    to 8 values finite in fp32; `wet`: a number finite in fp32; `day_numbers` as in climate_indices.
    Validity is paired over everything: day t is valid at pixel p when the mask admits it, obs[t,p] is not NaN and gen[m,t,p]
    is not NaN for EVERY member m, so `days`, the period day counts and which windows exist are one map for all series.
    Run length: r[t] = valid[t] ? (linked[t] ? r[t-1] : 0) + 1 : 0 with r[-1] = 0; linked[t] is day_numbers[t] ==
    day_numbers[t-1] + 1, without day_numbers it is true for t > 0: a broken link acts as one invalid day in between, the
    rule of climate_indices.  Window K ending on day t exists iff r[t] >= K; its sum is S = ((((+0.0 + x[t-K+1]) + x[t-K+2])
    + ...) + x[t]) in fp64, oldest day first, each fp32 value widened first (starting from +0.0 makes -0 impossible).
    Returns a dict of device tensors, for both sides as `gen_<name>` (with a leading [M] axis iff gen was 4-D) and
    `obs_<name>`: `days` int32 [H,W] (one map); `rx` fp32 [Kw,H,W], the largest S over the windows that exist, rounded to fp32
    once, NaN where none exists (K = 1 is Rx1day, K = 5 Rx5day); `count` int32 [T,H,W], the valid days with x >= threshold_j
    compared in fp32 (R10mm at 10); `prcptot` fp32 [H,W], the fp64 sum in day order over the valid days with x >= wet, rounded
    once, 0 where there is a valid day and no wet one, NaN where days == 0.
    `periods`: one id per day in -1..255 (a sequence or an integer tensor; P = the largest id + 1); -1 belongs to no period;
    any order, ids may recur (seasons) or stay unused (calendar.periods_from_dates gives years, seasons and months of years).
    The dict gains `period_days` int32 [P,H,W], the valid days with id g, and `period_<side>_rx`, `period_<side>_count`,
    `period_<side>_prcptot` with [P, ...] after the member axis: count and prcptot run over the days of the id, rx over the
    windows whose LAST day has id g.  A window may reach back into days of another id or of id -1 as long as its K days are
    linked and valid, which is what climdex does (a running sum over the record, then a maximum per year) and deliberately
    differs from the subsequence rule of climate_indices' groups.  An id no day uses gives period_days 0, count 0 and NaN
    float maps.  Across the periods, for each index (every rx window, every count threshold, prcptot) a period counts when
    period_days[g] >= min_days (>= 1) and its value is not NaN: `<side>_period_n_<index>` int32, the counting periods;
    `<side>_period_mean_<index>`, the fp64 sum of the fp32 values (counts as exact doubles) in id order / n, rounded once;
    `<side>_period_std_<index>` = sqrt(sum (v - mean)^2 / (n - 1)) against the unrounded mean for n >= 2, else NaN; index in
    rx, count, prcptot, shaped as the index.  Every element of every output is written; two calls give bit-equal results,
    whatever the strides of gen."""
    name = "period_indices"
    if gen.dim() not in (3, 4):
        raise ValueError(f"gen: expected [N, H, W] or [M, N, H, W], got {tuple(gen.shape)}")
    if obs.dim() != 3:
        raise ValueError(f"obs: expected [N, H, W], got {tuple(obs.shape)}")
    for what, x in (("gen", gen), ("obs", obs)):
        if x.dtype != torch.float32:
            raise TypeError(f"{what}: expected a float32 tensor, got {x.dtype}")
    members = gen.dim() == 4
    M = gen.shape[0] if members else 1
    n, H, W = gen.shape[-3:]
    if not (2 <= H <= MAX_FIELD_SIDE and 2 <= W <= MAX_FIELD_SIDE) or H * W > MAX_FIELD_PIXELS:
        raise ValueError(f"{name}: field size {H}x{W}; sides must be 2..{MAX_FIELD_SIDE} and H*W <= 2^20")
    if not 2 <= n <= MAX_TEMPORAL_DAYS:
        raise ValueError(f"{name}: N={n} days; need 2..{MAX_TEMPORAL_DAYS}")
    if not 1 <= M <= MAX_PERIOD_MEMBERS:
        raise ValueError(f"{name}: M={M} members; need 1..{MAX_PERIOD_MEMBERS}")
    if tuple(obs.shape) != (n, H, W):
        raise ValueError(f"obs: shape {tuple(obs.shape)} does not match gen days and fields {(n, H, W)}")
    _shape_rows(mask, "mask", (H, W), (1, n))
    if mask is not None and not (mask.dtype in (torch.uint8, torch.bool) or mask.is_floating_point()):
        raise TypeError(f"mask: expected uint8, bool or float, got {mask.dtype}")
    win = list(windows)
    if not 1 <= len(win) <= MAX_PERIOD_WINDOWS:
        raise ValueError(f"{name}: {len(win)} windows; need 1..{MAX_PERIOD_WINDOWS}")
    if any(isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= MAX_PERIOD_WINDOW for k in win):
        raise ValueError(f"{name}: windows must be integers in 1..{MAX_PERIOD_WINDOW}, got {win}")
    win = [int(k) for k in win]
    if any(b <= a for a, b in zip(win, win[1:])):
        raise ValueError(f"{name}: windows must be distinct and ascending, got {win}")
    thr = [float(t) for t in thresholds]
    if len(thr) > MAX_PERIOD_THRESHOLDS:
        raise ValueError(f"{name}: {len(thr)} thresholds; at most {MAX_PERIOD_THRESHOLDS}")
    tarr = (C.c_float * len(thr))(*thr) if thr else None
    if thr and not all(math.isfinite(t) and math.isfinite(a) for t, a in zip(thr, tarr)):
        raise ValueError(f"{name}: thresholds must be finite in fp32, got {thr}")
    if isinstance(wet, bool) or not isinstance(wet, (int, float)) or not math.isfinite(wet) or not math.isfinite(C.c_float(wet).value):
        raise ValueError(f"{name}: wet must be a number finite in fp32, got {wet!r}")
    if isinstance(min_days, bool) or not isinstance(min_days, int) or not 1 <= min_days < 2 ** 31:
        raise ValueError(f"{name}: min_days must be an integer >= 1, got {min_days!r}")
    dn = _day_numbers(day_numbers, n)
    pids, P = _period_ids(periods, n)
    N.require_device(gen, obs)
    if obs.device != gen.device:
        raise ValueError("gen and obs must be on the same device")
    HW = H * W
    if members:
        g = gen
        if g.stride(3) != 1 or g.stride(2) != W or g.stride(1) < HW or (M > 1 and g.stride(0) < HW):
            g = g.contiguous()
        mstride, dstride = (g.stride(0) if M > 1 else 0), g.stride(1)
    else:
        g = gen.contiguous()
        mstride, dstride = 0, HW
    o = obs.contiguous()
    m, u8, nm = _mask(mask, HW, (1, n))
    Kw, T, S, dev = len(win), len(thr), M + 1, g.device
    I = Kw + T + 1
    i32 = dict(dtype=torch.int32, device=dev)
    days, rx, count, prc = torch.empty(HW, **i32), torch.empty(S, Kw, HW, device=dev), torch.empty(S, T, HW, **i32), torch.empty(S, HW, device=dev)
    pdays, prx, pcount = torch.empty(P, HW, **i32), torch.empty(S, P, Kw, HW, device=dev), torch.empty(S, P, T, HW, **i32)
    pprc = torch.empty(S, P, HW, device=dev)
    an, amean, astd = torch.empty(S, I, HW, **i32), torch.empty(S, I, HW, device=dev), torch.empty(S, I, HW, device=dev)
    dn_dev = None if dn is None else torch.tensor(dn, dtype=torch.int32, device=dev)
    p_dev = None if pids is None else torch.tensor(pids, dtype=torch.int32, device=dev)
    nbytes = N.lib().sbgm_period_indices_workspace_bytes(n, M, H, W, Kw, T, P)
    ws = _ws(nbytes, dev)
    have = lambda t, on=True: t.data_ptr() if on and t.numel() else None                          # noqa: E731
    N.check(N.lib().sbgm_period_indices(
        g.data_ptr(), mstride, dstride, o.data_ptr(), N.ptr(m), u8, n, nm, M, H, W, (C.c_int * Kw)(*win), Kw, tarr, T, float(wet),
        min_days, N.ptr(dn_dev), N.ptr(p_dev), P, days.data_ptr(), rx.data_ptr(), have(count), prc.data_ptr(), have(pdays), have(prx),
        have(pcount), have(pprc), have(an, P), have(amean, P), have(astd, P), ws.data_ptr(), nbytes, N.stream()))

    def sides(t):
        """t [M + 1, ..., HW] -> (the member rows, without their axis for a 3-D gen; the obs row), each [..., H, W]"""
        v = t.unflatten(-1, (H, W))
        return (v[:M] if members else v[0]), v[M]

    out = {"days": days.view(H, W)}
    for key, t in (("rx", rx), ("count", count), ("prcptot", prc)):
        out[f"gen_{key}"], out[f"obs_{key}"] = sides(t)
    if P:
        out["period_days"] = pdays.view(P, H, W)
        for key, t in (("rx", prx), ("count", pcount), ("prcptot", pprc)):
            out[f"period_gen_{key}"], out[f"period_obs_{key}"] = sides(t)
        for stat, t in (("n", an), ("mean", amean), ("std", astd)):
            for key, sl in (("rx", slice(0, Kw)), ("count", slice(Kw, Kw + T)), ("prcptot", Kw + T)):
                out[f"gen_period_{stat}_{key}"], out[f"obs_period_{stat}_{key}"] = sides(t[:, sl])
    return out
