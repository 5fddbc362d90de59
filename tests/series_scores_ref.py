"""numpy float64 restatement of verification.series_ensemble_scores (csrc/verify_series.hip): pooled
ensemble verification of a series ens [D,M,H,W] against obs [D,H,W] over days x pixels, for all days (row 0) and per group of days
(row 1 + g).  The per-cell expressions and the per-pixel sums over the days are restated op for op (the members in K43's order:
chunks of 16 in registers, all members streaming past; the days in day order), so the maps can be compared bit for bit; the
pooled sums are plain numpy sums, the integer tables are exact, and the climatological pair sum is either the direct sum over all
ordered pairs or, for long records, the sorted form 2 sum_k (2k - n + 1) y_(k)."""
import numpy as np

import philox_ref

f32 = np.float32
ENSEMBLE_KEYS = ("count", "crps_fair", "crps_standard", "skill", "spread", "spread_skill_ratio")
EXCEEDANCE_KEYS = ("brier", "brier_reliability", "brier_resolution", "brier_uncertainty", "base_rate", "roc_area")
MAP_KEYS = ("crps", "spread", "skill", "ssr")
CLIM_MAP_KEYS = ("clim_crps", "crpss")
SKILL_KEYS = ("cells", "crps_fair", "crps_reference", "crpss")
KEYS = ("count",) + MAP_KEYS + ("daily", "scores", "rank_hist", "table", "exceedance") + CLIM_MAP_KEYS + ("skill_scores",)
MEMBER_CHUNK = 16
SORTED_FROM = 400                     # days from which the pair sum uses the sorted form


def admitted(mask, D, shape):
    """bool [D,H,W] from mask None, [H,W] or [D,H,W]: uint8 / bool != 0, float > 0.5"""
    if mask is None:
        return np.ones((D, *shape), bool)
    m = np.asarray(mask)
    m = m > 0.5 if m.dtype.kind == "f" else m != 0
    return np.broadcast_to(m, (D, *shape)).copy()


def valid_cells(ens, obs, mask=None):
    return ~np.isnan(obs) & ~np.isnan(ens).any(axis=1) & admitted(mask, obs.shape[0], obs.shape[1:])


def cell_scores(ens, obs):
    """(mean, var, crps_fair, crps_std, se) float64 [D,H,W] by K43's op sequence; garbage at invalid cells"""
    D, M = ens.shape[:2]
    x, y = ens.astype(np.float64), obs.astype(np.float64)
    sx, sad, spair, spair2 = (np.zeros(obs.shape) for _ in range(4))
    with np.errstate(invalid="ignore"):
        for i0 in range(0, M, MEMBER_CHUNK):
            chunk = range(i0, min(M, i0 + MEMBER_CHUNK))
            for k in chunk:
                sx = sx + x[:, k]
                sad = sad + np.abs(x[:, k] - y)
            for j in range(M):
                for k in chunk:
                    d = x[:, k] - x[:, j]
                    spair = spair + np.abs(d)
                    spair2 = spair2 + d * d
        Md = np.float64(M)
        mean = sx / Md
        var = spair2 / (2.0 * Md * (Md - 1.0))
        crps_fair = sad / Md - spair / (2.0 * Md * (Md - 1.0))
        crps_std = sad / Md - spair / (2.0 * Md * Md)
        se = (mean - y) * (mean - y)
    return mean, var, crps_fair, crps_std, se


def day_order_sum(v, valid):
    """sum over axis 0 of v where valid, one add per day in day order"""
    acc = np.zeros(v.shape[1:])
    for d in range(v.shape[0]):
        acc = acc + np.where(valid[d], v[d], 0.0)
    return acc


def scores_from_sums(v, M):
    """[6] of ENSEMBLE_KEYS from (cnt, sum crps_fair, sum crps_std, sum se, sum var)"""
    if v[0] <= 0:
        return np.array([v[0]] + [np.nan] * 5)
    skill, spread = np.sqrt(v[3] / v[0]), np.sqrt(v[4] / v[0])
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.array([v[0], v[1] / v[0], v[2] / v[0], skill, spread, np.sqrt((M + 1.0) / M) * spread / np.float64(skill)])


def ranks(ens, obs, seed):
    """int [D,H,W]: lt + floor(u (le - lt + 1)) capped at le, u the first uniform of Philox block (seed, day, pixel), in fp32"""
    D, M, H, W = ens.shape
    with np.errstate(invalid="ignore"):
        lt, le = (ens < obs[:, None]).sum(1), (ens <= obs[:, None]).sum(1)
    p = np.arange(H * W, dtype=np.uint64).reshape(H, W)
    u = np.stack([philox_ref.uniform4(seed, d, p)[..., 0] for d in range(D)]).astype(f32)
    r = lt + np.floor(u * (le - lt + 1).astype(f32)).astype(np.int64)
    return np.minimum(le, r)


def exceedance_from_table(tab, M):
    """K46's finish on one threshold's table [M+1,2] -> [6] of EXCEEDANCE_KEYS, op for op"""
    n_k, o_k = tab[:, 0].astype(np.int64), tab[:, 1].astype(np.int64)
    Nn, Oo = int(n_k.sum()), int(o_k.sum())
    if Nn == 0:
        return np.full(6, np.nan)
    N, O, Md = np.float64(Nn), np.float64(Oo), np.float64(M)
    bs = rel = res = area = np.float64(0.0)
    obar = O / N
    hits = fas = 0
    with np.errstate(divide="ignore", invalid="ignore"):
        for k in range(M, -1, -1):
            nk, ok, pk = np.float64(n_k[k]), np.float64(o_k[k]), np.float64(k) / Md
            bs = bs + (nk * pk * pk - 2.0 * ok * pk + ok)
            if n_k[k] > 0:
                obk = ok / nk
                rel = rel + nk * (pk - obk) * (pk - obk)
                res = res + nk * (obk - obar) * (obk - obar)
            h1, f1 = hits + int(o_k[k]), fas + int(n_k[k]) - int(o_k[k])
            area = area + (np.float64(f1 - fas) / (N - O)) * ((np.float64(h1) + np.float64(hits)) / O) / 2.0
            hits, fas = h1, f1
    return np.array([bs / N, rel / N, res / N, obar * (1.0 - obar), obar, area if 0 < Oo < Nn else np.nan])


def pair_sums(obs, valid, rows):
    """S [R,H,W]: per row (a bool [D] of its days) the sum over the ordered pairs of the pixel's valid days in the row of
    |y_i - y_j|"""
    D = obs.shape[0]
    y = obs.astype(np.float64)
    S = np.zeros((len(rows), *obs.shape[1:]))
    w = [valid & r[:, None, None] for r in rows]
    if D >= SORTED_FROM:
        for ri in range(len(rows)):
            ys = np.sort(np.where(w[ri], y, np.inf), axis=0)
            n = w[ri].sum(0)
            k = np.arange(D, dtype=np.float64)[:, None, None]
            S[ri] = 2.0 * np.where(k < n, (2.0 * k - n + 1.0) * np.where(np.isinf(ys), 0.0, ys), 0.0).sum(0)
        return S
    for i in range(D):
        with np.errstate(invalid="ignore"):
            a = np.abs(y - y[i])
        for ri, r in enumerate(rows):
            if r[i]:
                S[ri] += np.where(valid[i], np.where(w[ri], a, 0.0).sum(0), 0.0)
    return S


def series_ensemble_scores(ens, obs, thresholds=(), groups=None, mask=None, seed=0, climatology=True):
    """ens [D,M,H,W], obs [D,H,W] float32 -> dict of numpy arrays under KEYS, plus `_F` and `_C` [G+1,H,W] (the per-pixel sums of
    the forecast's and the reference's fair CRPS per row, NaN where n < 3 there) and `_n` [G+1,H,W]"""
    ens, obs = np.asarray(ens, f32), np.asarray(obs, f32)
    D, M, H, W = ens.shape
    T = len(thresholds)
    groups = None if groups is None else np.asarray(groups, np.int64)
    G = 0 if groups is None else int(groups.max()) + 1
    rows = [np.ones(D, bool)] + [groups == g for g in range(G)]
    valid = valid_cells(ens, obs, mask)
    mean, var, cf, cs, se = cell_scores(ens, obs)
    n = valid.sum(0).astype(np.int32)
    F, SV, SE = day_order_sum(cf, valid), day_order_sum(var, valid), day_order_sum(se, valid)
    out = {"count": n}
    with np.errstate(divide="ignore", invalid="ignore"):
        nd = n.astype(np.float64)
        spread, skill = np.sqrt(SV / nd), np.sqrt(SE / nd)
        some = n > 0
        out["crps"] = np.where(some, F / nd, np.nan).astype(f32)
        out["spread"] = np.where(some, spread, np.nan).astype(f32)
        out["skill"] = np.where(some, skill, np.nan).astype(f32)
        out["ssr"] = np.where(some, np.sqrt((M + 1.0) / M) * spread / skill, np.nan).astype(f32)
    per_day = np.stack([valid.reshape(D, -1).sum(1)] + [np.where(valid, v, 0.0).reshape(D, -1).sum(1) for v in (cf, cs, se, var)], axis=1)
    out["daily"] = np.stack([scores_from_sums(per_day[d], M) for d in range(D)])
    out["scores"] = np.stack([scores_from_sums(per_day[r].sum(0), M) for r in rows])
    r_cell = ranks(ens, obs, seed)
    out["rank_hist"] = np.stack([np.bincount(r_cell[valid & r[:, None, None]], minlength=M + 1) for r in rows]).astype(np.int64)
    table = np.zeros((G + 1, T, M + 1, 2), np.int64)
    for t, thr in enumerate(thresholds):
        with np.errstate(invalid="ignore"):
            k, o = (ens >= f32(thr)).sum(1), obs >= f32(thr)
        for ri, r in enumerate(rows):
            sel = valid & r[:, None, None]
            table[ri, t, :, 0] = np.bincount(k[sel], minlength=M + 1)
            table[ri, t, :, 1] = np.bincount(k[sel & o], minlength=M + 1)
    out["table"] = table
    out["exceedance"] = np.full((G + 1, 6, T), np.nan)
    for ri in range(G + 1):
        for t in range(T):
            out["exceedance"][ri, :, t] = exceedance_from_table(table[ri, t], M)
    out["clim_crps"], out["crpss"] = np.full((H, W), np.nan, f32), np.full((H, W), np.nan, f32)
    out["skill_scores"] = np.full((G + 1, 4), np.nan)
    if climatology:
        S = pair_sums(obs, valid, rows)
        n_r = np.stack([(valid & r[:, None, None]).sum(0) for r in rows])
        F_r = np.stack([F] + [day_order_sum(cf, valid & r[:, None, None]) for r in rows[1:]])
        with np.errstate(divide="ignore", invalid="ignore"):
            C_r = S / (2.0 * (n_r.astype(np.float64) - 1.0))
            ok = n_r >= 3
            out["clim_crps"] = np.where(ok[0], C_r[0] / n_r[0], np.nan).astype(f32)
            out["crpss"] = np.where(ok[0] & (C_r[0] != 0.0), 1.0 - F_r[0] / C_r[0], np.nan).astype(f32)
            for ri in range(G + 1):
                cells, sf, sc = n_r[ri][ok[ri]].sum(), F_r[ri][ok[ri]].sum(), C_r[ri][ok[ri]].sum()
                out["skill_scores"][ri] = [cells, sf / cells if cells else np.nan, sc / cells if cells else np.nan,
                                           1.0 - sf / sc if cells and sc != 0.0 else np.nan]
        out["_F"], out["_C"], out["_n"] = np.where(ok, F_r, np.nan), np.where(ok, C_r, np.nan), n_r
    return out
