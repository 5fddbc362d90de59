"""numpy restatement of the neighbourhood and threshold-exceedance scores (sbgm_danra_amd.verification.neighbourhood_scores /
exceedance_scores), shared by test_cpu_spatial_scores.py and test_gpu_spatial_scores.py.

The window sums are a direct zero-padded loop over the n x n offsets on int64 images — deliberately not a summed-area table,
which is the kernel's own trick.  The exceedance table comes from np.add.at, and the Brier terms and the ROC area come from
their textbook sums over pixels (the ROC area as the Mann-Whitney statistic), not from the table the kernel derives them from.
Ratios of the exact integers are formed with fractions.Fraction, so each fp64 value here is the correctly rounded one."""
from fractions import Fraction

import numpy as np


def valid_pixels(gen, obs, mask):
    """bool [N,H,W]: gen and obs not NaN and the mask (bool, broadcast over fields) admits the pixel"""
    v = ~np.isnan(gen) & ~np.isnan(np.broadcast_to(obs, gen.shape))
    if mask is not None:
        v = v & np.broadcast_to(mask, gen.shape)
    return v


def event_images(gen, obs, thr, mask=None):
    """int64 (I_g, I_o) [N,H,W] at one threshold; the comparison is fp32 `v >= thr`"""
    v = valid_pixels(gen, obs, mask)
    t = np.float32(thr)
    with np.errstate(invalid="ignore"):
        ig = v & (gen.astype(np.float32) >= t)
        io = v & (np.broadcast_to(obs, gen.shape).astype(np.float32) >= t)
    return ig.astype(np.int64), io.astype(np.int64)


def window_sum_direct(img, n):
    """sum of img [..., H, W] (int64) over the n x n window around every pixel, zero beyond the domain: one shifted add per offset"""
    r = (n - 1) // 2
    H, W = img.shape[-2:]
    pad = np.zeros(img.shape[:-2] + (H + 2 * r, W + 2 * r), dtype=np.int64)
    pad[..., r:r + H, r:r + W] = img
    out = np.zeros(img.shape, dtype=np.int64)
    for di in range(2 * r + 1):
        for dj in range(2 * r + 1):
            out += pad[..., di:di + H, dj:dj + W]
    return out


def _ratio(a, b):
    """a / b of two Python ints as IEEE would give it for exactly representable operands: x/0 = inf, 0/0 = nan"""
    if b == 0:
        return float("nan") if a == 0 else float("inf")
    return float(Fraction(a, b))


def fss_from_counts(num, den, events_gen, events_obs, valid):
    """the fp64 scores from the exact integers: fss [T,S], fss_field [N,T,S], freq_bias [T], fss_useful [T]"""
    num, den = np.asarray(num), np.asarray(den)
    N, T, S = num.shape
    one_minus = lambda a, b: float("nan") if b == 0 else float(1 - Fraction(a, b))
    fss = np.array([[one_minus(sum(int(x) for x in num[:, t, s]), sum(int(x) for x in den[:, t, s])) for s in range(S)]
                    for t in range(T)], dtype=np.float64).reshape(T, S)
    fss_field = np.array([[[one_minus(int(num[f, t, s]), int(den[f, t, s])) for s in range(S)] for t in range(T)]
                          for f in range(N)], dtype=np.float64).reshape(N, T, S)
    eg = [sum(int(x) for x in np.asarray(events_gen)[:, t]) for t in range(T)]
    eo = [sum(int(x) for x in np.asarray(events_obs)[:, t]) for t in range(T)]
    nv = sum(int(x) for x in np.asarray(valid))
    freq_bias = np.array([_ratio(eg[t], eo[t]) for t in range(T)])
    fss_useful = np.array([float("nan") if nv == 0 else float(Fraction(1, 2) + Fraction(eo[t], nv) / 2) for t in range(T)])
    return dict(fss=fss, fss_field=fss_field, freq_bias=freq_bias, fss_useful=fss_useful)


def neighbourhood_scores(gen, obs, thresholds, scales, mask=None, window_sum=window_sum_direct):
    """gen [N,H,W], obs [No,H,W] float32, mask bool [Nm,H,W] or None -> dict of numpy arrays named as the device function's"""
    gen = np.asarray(gen, dtype=np.float32)
    obs = np.asarray(obs, dtype=np.float32)
    N, T, S = gen.shape[0], len(thresholds), len(scales)
    num = np.zeros((N, T, S), dtype=np.int64)
    den = np.zeros((N, T, S), dtype=np.int64)
    eg = np.zeros((N, T), dtype=np.int64)
    eo = np.zeros((N, T), dtype=np.int64)
    for t, thr in enumerate(thresholds):
        ig, io = event_images(gen, obs, thr, mask)
        eg[:, t], eo[:, t] = ig.sum((1, 2)), io.sum((1, 2))
        for s, n in enumerate(scales):
            cg, co = window_sum(ig, n), window_sum(io, n)
            num[:, t, s] = ((cg - co) ** 2).sum((1, 2))
            den[:, t, s] = (cg ** 2 + co ** 2).sum((1, 2))
    valid = valid_pixels(gen, obs, mask).sum((1, 2)).astype(np.int64)
    out = dict(num=num, den=den, events_gen=eg, events_obs=eo, valid=valid)
    out.update(fss_from_counts(num, den, eg, eo, valid))
    return out


def exceedance_scores(ens, obs, thresholds, mask=None):
    """ens [M,H,W], obs [H,W] float32, mask bool [H,W] or None -> table int64 [T,M+1,2], count, and fp64 [T] scores from
    direct sums over the valid pixels"""
    ens = np.asarray(ens, dtype=np.float32)
    obs = np.asarray(obs, dtype=np.float32)
    M = ens.shape[0]
    T = len(thresholds)
    valid = ~np.isnan(obs) & ~np.isnan(ens).any(0)
    if mask is not None:
        valid &= mask
    e, y = ens[:, valid], obs[valid]
    count = int(valid.sum())
    table = np.zeros((T, M + 1, 2), dtype=np.int64)
    keys = ("brier", "brier_reliability", "brier_resolution", "brier_uncertainty", "base_rate", "roc_area")
    out = {k: np.full(T, np.nan) for k in keys}
    for t, thr in enumerate(thresholds):
        th = np.float32(thr)
        k = (e >= th).sum(0).astype(np.int64)
        o = (y >= th).astype(np.int64)
        np.add.at(table[t, :, 0], k, 1)
        np.add.at(table[t, :, 1], k, o)
        if count == 0:
            continue
        p, od = k.astype(np.float64) / M, o.astype(np.float64)
        obar = od.mean()
        cond = np.zeros_like(p)                         # each pixel's conditional event frequency among the pixels sharing its p
        for kk in np.unique(k):
            sel = k == kk
            cond[sel] = od[sel].mean()
        out["brier"][t] = ((p - od) ** 2).mean()
        out["brier_reliability"][t] = ((p - cond) ** 2).mean()
        out["brier_resolution"][t] = ((cond - obar) ** 2).mean()
        out["brier_uncertainty"][t] = obar * (1.0 - obar)
        out["base_rate"][t] = obar
        ke, kq = np.sort(k[o == 1]), np.sort(k[o == 0])
        if ke.size and kq.size:                         # Mann-Whitney: P(p_event > p_non-event) + P(equal) / 2
            below = np.searchsorted(kq, ke, side="left")
            ties = np.searchsorted(kq, ke, side="right") - below
            out["roc_area"][t] = float(Fraction(2 * int(below.sum()) + int(ties.sum()), 2 * int(ke.size) * int(kq.size)))
    return dict(table=table, count=count, **out)
