"""Plain numpy float64 restatement of the multivariate ensemble scores of csrc/verify_multivariate.hip (DESIGN.md §11, K53 and
K54): explicit loops over members / offsets, broadcasting over pixels.  Nothing here is fast; it states what is computed."""
import numpy as np

ENERGY_KEYS = ("count", "es_fair", "es_standard", "mean_dist_obs", "mean_dist_pair", "min_dist_pair")
VARIOGRAM_KEYS = ("vs", "n_pairs", "sum_w", "vs_unweighted")


def valid_pixels(ens, obs, mask=None):
    """bool [H, W]: every member and the truth are not NaN and the mask (bool / uint8 != 0, float > 0.5) admits the pixel"""
    v = ~np.isnan(obs) & ~np.isnan(ens).any(axis=0)
    if mask is not None:
        mask = np.asarray(mask)
        v &= (mask > 0.5) if mask.dtype.kind == "f" else (mask != 0)
    return v


def offsets(radius):
    """half-plane (dy > 0, or dy == 0 and dx > 0) of the disc dy^2 + dx^2 <= radius^2, dy ascending, then dx ascending"""
    return [(dy, dx) for dy in range(radius + 1) for dx in range(-radius, radius + 1)
            if (dy > 0 or dx > 0) and dy * dy + dx * dx <= radius * radius]


def energy_rows(ens, obs, mask=None, rows=None):
    """(the given rows of dist2 [M+1, M+1] over the valid pixels — all by default; the truth is row / column M —, count)"""
    ens, obs = np.asarray(ens, np.float32), np.asarray(obs, np.float32)
    v = valid_pixels(ens, obs, mask)
    x = np.concatenate([ens[:, v], obs[v][None]]).astype(np.float64)               # [M+1, count], exact in fp64
    rows = range(x.shape[0]) if rows is None else rows
    d2 = np.zeros((len(rows), x.shape[0]))
    for n, i in enumerate(rows):
        d = x[i][None, :] - x                                                        # the difference form, nothing else
        d2[n] = (d * d).sum(axis=1)
    return d2, x.shape[1]


def energy_scores_from_dist2(d2, count):
    """the scores in ENERGY_KEYS order from dist2 [M+1, M+1] and the number of valid pixels"""
    M = d2.shape[0] - 1
    with np.errstate(invalid="ignore", divide="ignore"):
        dist = np.sqrt(d2 / count)                                                   # RMS distances; NaN when count == 0
    pair = dist[:M, :M][~np.eye(M, dtype=bool)]
    mean_obs = dist[:M, M].sum() / M
    return np.array([count, mean_obs - pair.sum() / (2.0 * M * (M - 1)), mean_obs - pair.sum() / (2.0 * M * M), mean_obs,
                     pair.sum() / (M * (M - 1)), pair.min() if count else np.nan])


def energy_scores(ens, obs, mask=None):
    """dist2 [M+1, M+1] over the valid pixels (the truth is row / column M) and the scores in ENERGY_KEYS order"""
    d2, count = energy_rows(ens, obs, mask)
    return dict(dist2=d2, scores=energy_scores_from_dist2(d2, count))


def offset_weight(dy, dx, weights):
    """1 / distance rounded to fp32 ("inverse_distance") or 1 ("unit")"""
    return float(np.float32(1.0 / np.sqrt(float(dy * dy + dx * dx)))) if weights == "inverse_distance" else 1.0


def _power(d, order):
    """|d|^order of fp32 differences, in fp32"""
    a = np.abs(d)
    return {0.5: np.sqrt(a), 1.0: a, 2.0: a * a}[float(order)].astype(np.float32)


def variogram_offset(ens, obs, v, dy, dx, order, w):
    """one offset of the variogram score: None when no pixel pair fits into the field, else (slices of pixel i, pair validity,
    g_ens, g_obs [both over the window of pixel i], term = (g_obs - g_ens)^2 or 0 where the pair is invalid)"""
    M, H, W = ens.shape
    if dy >= H or abs(dx) >= W:
        return None
    ys, xs = slice(0, H - dy), slice(max(0, -dx), W - max(0, dx))                    # pixel i
    yt, xt = slice(dy, H), slice(max(0, dx), W + min(0, dx))                         # pixel j = i + (dy, dx)
    pv = v[ys, xs] & v[yt, xt]
    with np.errstate(invalid="ignore"):
        ge = np.zeros(pv.shape)
        for m in range(M):                                                           # fp32 difference and power, fp64 sum
            ge += _power(ens[m][ys, xs] - ens[m][yt, xt], order).astype(np.float64)
        ge /= M
        go = _power(obs[ys, xs] - obs[yt, xt], order).astype(np.float64)
    ge, go = np.where(pv, ge, 0.0), np.where(pv, go, 0.0)
    return (ys, xs), pv, ge, go, (go - ge) ** 2


def variogram_scores(ens, obs, radius=4, order=0.5, weights="inverse_distance", mask=None, per_offset=None):
    """vs_map [H, W] (fp64 here, NaN at invalid pixels), offsets, gamma_ens, gamma_obs, pairs, scores in VARIOGRAM_KEYS order,
    and cond = sum w 2 |g_obs - g_ens| g_ens / sum w: how strongly a relative error of the member terms moves vs.  Likewise
    cond_unweighted (w = 1, over n_pairs) for vs_unweighted and, per pixel and for errors of both variograms, map_cond [H, W] =
    sum over the pixel's pairs of w 2 |g_obs - g_ens| (g_ens + g_obs) for vs_map.  `per_offset` may supply the results of
    variogram_offset, in offset order, computed elsewhere (in parallel, say)."""
    ens, obs = np.asarray(ens, np.float32), np.asarray(obs, np.float32)
    M, H, W = ens.shape
    v = valid_pixels(ens, obs, mask)
    offs = offsets(radius)
    vs_map, map_cond = np.zeros((H, W)), np.zeros((H, W))
    g_e, g_o, pairs = np.zeros(len(offs)), np.zeros(len(offs)), np.zeros(len(offs), np.int64)
    num = den = unum = cond = ucond = 0.0
    for k, (dy, dx) in enumerate(offs):
        w = offset_weight(dy, dx, weights)
        part = variogram_offset(ens, obs, v, dy, dx, order, w) if per_offset is None else per_offset[k]
        if part is None:
            g_e[k] = g_o[k] = np.nan
            continue
        (ys, xs), pv, ge, go, term = part
        vs_map[ys, xs] += w * term
        n = int(pv.sum())
        pairs[k] = n
        with np.errstate(invalid="ignore", divide="ignore"):
            g_e[k] = np.float64(ge.sum()) / n
            g_o[k] = np.float64(go.sum()) / n
        num += w * term.sum()
        den += w * n
        unum += term.sum()
        cond += w * (2.0 * np.abs(go - ge) * ge).sum()
        ucond += (2.0 * np.abs(go - ge) * ge).sum()
        map_cond[ys, xs] += w * 2.0 * np.abs(go - ge) * (go + ge)
    vs_map[~v] = np.nan
    n_pairs = int(pairs.sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        scores = np.array([np.float64(num) / den, n_pairs, den, np.float64(unum) / n_pairs])
        cond, ucond = np.float64(cond) / den, np.float64(ucond) / n_pairs
    return dict(vs_map=vs_map, offsets=np.array(offs, np.int32).reshape(-1, 2), gamma_ens=g_e, gamma_obs=g_o, pairs=pairs,
                scores=scores, cond=cond, cond_unweighted=ucond, map_cond=map_cond)
