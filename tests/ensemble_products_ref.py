"""numpy restatement of the ensemble products (sbgm_danra_amd.verification.ensemble_products), shared by
test_cpu_ensemble_products.py and test_gpu_ensemble_products.py.  It states the contract, not the kernel: the order statistics
come from np.sort along the member axis (the kernel never sorts), the quantile is Hyndman-Fan type 7 with the weight g
computed in fp64 and one fp64 lerp rounded once to fp32, and the two fp64 sums of the moments run over the members in an
explicit loop, in member order, as the kernel adds them."""
import numpy as np


def rank_weights(q, M):
    """(lo, hi, g) of quantile level q among M members: h = q (M - 1) in fp64, lo = floor(h), g = h - lo, hi = min(lo + 1, M - 1)"""
    h = np.float64(q) * np.float64(M - 1)
    lo = int(np.floor(h))
    return lo, min(lo + 1, M - 1), np.float64(h - np.floor(h))


def valid_pixels(ens, mask=None):
    """no member is NaN and the mask admits the pixel (bool / uint8 != 0, float > 0.5)"""
    ok = ~np.isnan(ens).any(axis=0)
    if mask is not None:
        mask = np.asarray(mask)
        ok &= (mask > 0.5) if mask.dtype.kind == "f" else (mask != 0)
    return ok


def ensemble_products(ens, quantiles=(), thresholds=(), mask=None):
    """ens fp32 [M,H,W] -> dict of mean, std, min, max [H,W] fp32, quantiles [Q,H,W], exceed_prob [T,H,W] (NaN at invalid
    pixels) and count"""
    ens = np.asarray(ens, dtype=np.float32)
    M = ens.shape[0]
    ok = valid_pixels(ens, mask)
    with np.errstate(invalid="ignore"):
        srt = np.sort(ens, axis=0)                                # NaNs go last; those pixels are dropped below
        total = np.zeros(ens.shape[1:], np.float64)
        for m in range(M):
            total = total + ens[m].astype(np.float64)
        mean64 = total / np.float64(M)
        ss = np.zeros(ens.shape[1:], np.float64)
        for m in range(M):
            d = ens[m].astype(np.float64) - mean64
            ss = ss + d * d
        out = {"mean": mean64.astype(np.float32), "std": np.sqrt(ss / np.float64(M - 1)).astype(np.float32),
               "min": srt[0].copy(), "max": srt[M - 1].copy()}
        quant = np.empty((len(quantiles),) + ens.shape[1:], np.float32)
        for i, q in enumerate(quantiles):
            lo, hi, g = rank_weights(q, M)
            a, b = srt[lo], srt[hi]
            lerp = (a.astype(np.float64) + g * (b.astype(np.float64) - a.astype(np.float64))).astype(np.float32)
            quant[i] = np.where((g == 0.0) | (a == b), a, lerp)
        exceed = np.empty((len(thresholds),) + ens.shape[1:], np.float32)
        for i, t in enumerate(thresholds):
            k = (ens >= np.float32(t)).sum(axis=0)
            exceed[i] = (k.astype(np.float64) / np.float64(M)).astype(np.float32)
    out.update(quantiles=quant, exceed_prob=exceed)
    for v in out.values():
        v[..., ~ok] = np.nan
    out["count"] = int(ok.sum())
    return out
