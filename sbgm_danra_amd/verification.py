"""Device-tensor wrappers of the verification kernels (csrc/verify.hip): error statistics, histograms,
ensemble scores (CRPS, rank histogram, spread/skill) and radially averaged power spectra.  Every function takes tensors on
the ROCm device and returns tensors on the device; arguments and shapes are checked before any launch and nothing is copied
to the host.  A pixel is valid when gen (every member) and obs are not NaN and the mask admits it (uint8/bool != 0, or float
> 0.5); every statistic uses the valid pixels only."""
from __future__ import annotations

import torch

from . import _native as N

GLOBAL_KEYS = ("count", "mean_gen", "mean_obs", "bias", "mae", "rmse", "min_gen", "max_gen", "min_obs", "max_obs")
ENSEMBLE_KEYS = ("count", "crps_fair", "crps_standard", "skill", "spread", "spread_skill_ratio")


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
