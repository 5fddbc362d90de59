"""numpy restatement of verification.period_indices, written from its definitions: a plain loop over the days, vectorised over
the pixels (and the series), float64.  It calls nothing from sbgm_danra_amd.verification.
  validity  paired over everything: the mask admits (t, p), obs[t, p] is not NaN and gen[m, t, p] is not NaN for every member m.
  run       r[t] = valid[t] ? (linked[t] ? r[t-1] : 0) + 1 : 0, r[-1] = 0; linked[t] = day_numbers[t] == day_numbers[t-1] + 1
            (true for t > 0 without day numbers).
  window    K ending on day t exists iff r[t] >= K; S = ((((+0.0 + x[t-K+1]) + x[t-K+2]) + ...) + x[t]) in fp64, oldest first.
  rx        the largest S over the windows that exist (best = S where best is NaN or S > best, in day order), rounded to fp32
            once; NaN where none exists.
  count     the valid days with x >= threshold (fp32 comparison); prcptot: the fp64 sum in day order over the valid days with
            x >= wet, rounded once; NaN where days == 0.
  period g  count and prcptot over the valid days with id g; rx over the windows whose LAST day has id g.
  across    a period counts when period_days[g] >= min_days and its value is not NaN: n, mean = fp64 sum in id order / n,
            std = sqrt(sum (v - mean)^2 / (n - 1)) against the unrounded mean for n >= 2."""
import numpy as np

f32, f64 = np.float32, np.float64


def admitted(mask, N, shape):
    """bool [N, H, W]: the mask's word on every (day, pixel); uint8 / bool != 0, float > 0.5"""
    if mask is None:
        return np.ones((N, *shape), bool)
    m = np.asarray(mask)
    m = (m > f32(0.5)) if m.dtype.kind == "f" else (m != 0)
    return np.broadcast_to(m if m.ndim == 3 else m[None], (N, *shape))


def linked(day_numbers, N):
    out = np.ones(N, bool)
    out[0] = False
    if day_numbers is not None:
        dn = np.asarray(day_numbers, np.int64)
        out[1:] = dn[1:] == dn[:-1] + 1
    return out


class _Acc:
    """the accumulators of the record or of one period, for S series"""

    def __init__(self, S, Kw, T, shape):
        self.best = np.full((S, Kw, *shape), np.nan, f64)
        self.count = np.zeros((S, T, *shape), np.int32)
        self.sum = np.zeros((S, *shape), f64)
        self.days = np.zeros(shape, np.int32)

    def day(self, valid, above, wet_day, x64, exists, sums):
        self.days += valid
        self.count += (valid[None, None] & above)
        self.sum = np.where(valid[None] & wet_day, self.sum + x64, self.sum)
        for k in range(len(exists)):
            take = exists[k][None] & (np.isnan(self.best[:, k]) | (sums[k] > self.best[:, k]))
            self.best[:, k] = np.where(take, sums[k], self.best[:, k])

    def maps(self):
        prcptot = np.where(self.days[None] > 0, self.sum, np.nan).astype(f32)
        return self.best.astype(f32), self.count.copy(), prcptot, self.days.copy()


def _across(values, counts):
    """values f64 [S, P, ...] (NaN where undefined), counts bool [P, ...] broadcast over S -> n int32, mean, std fp32"""
    ok = counts[None] & ~np.isnan(values)
    n = np.zeros(values[:, 0].shape, np.int32)
    total = np.zeros(values[:, 0].shape, f64)
    for g in range(values.shape[1]):
        total = np.where(ok[:, g], total + values[:, g], total)
        n += ok[:, g]
    mean = total / n
    ss = np.zeros_like(total)
    for g in range(values.shape[1]):
        d = values[:, g] - mean
        ss = np.where(ok[:, g], ss + d * d, ss)
    std = np.where(n >= 2, np.sqrt(ss / (n - 1)), np.nan)
    return n, np.where(n > 0, mean, np.nan).astype(f32), std.astype(f32)


def period_indices(gen, obs, windows=(1, 5), thresholds=(), wet=1.0, mask=None, day_numbers=None, periods=None, min_days=1):
    gen, obs = np.asarray(gen, f32), np.asarray(obs, f32)
    members = gen.ndim == 4
    g4 = gen if members else gen[None]
    M, N = g4.shape[:2]
    shape = obs.shape[1:]
    X = np.concatenate([g4, obs[None]])                                      # [S, N, H, W], obs last
    S, Kw, T = M + 1, len(windows), len(thresholds)
    valid = admitted(mask, N, shape) & ~np.isnan(X).any(axis=0)
    link = linked(day_numbers, N)
    thr = np.asarray(thresholds, f32).reshape(1, T, 1, 1)
    ids = None if periods is None else np.asarray(periods, np.int64)
    P = 0 if ids is None else max(int(ids.max()) + 1, 0)
    rec = _Acc(S, Kw, T, shape)
    per = [_Acc(S, Kw, T, shape) for _ in range(P)]
    r = np.zeros(shape, np.int64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for t in range(N):
            r = np.where(valid[t], (r if link[t] else 0) + 1, 0)
            x = X[:, t]
            x64 = x.astype(f64)
            above = x[:, None] >= thr                                         # fp32 comparison
            wet_day = x >= f32(wet)
            exists, sums = [], []
            for K in windows:
                exists.append(r >= K)
                s = np.zeros((S, *shape), f64)                               # +0.0
                for i in range(K - 1, -1, -1):                               # oldest day first
                    if t - i >= 0:                                           # else r < K: the sum is never taken
                        s = s + X[:, t - i].astype(f64)
                sums.append(s)
            rec.day(valid[t], above, wet_day, x64, exists, sums)
            if P and ids[t] >= 0:
                per[ids[t]].day(valid[t], above, wet_day, x64, exists, sums)

        def sides(pre, a, post=""):
            mem = a[:M] if members else a[0]
            return {f"{pre}gen_{post}": mem, f"{pre}obs_{post}": a[M]}

        rx, count, prcptot, days = rec.maps()
        out = {"days": days}
        out.update(sides("", rx, "rx"))
        out.update(sides("", count, "count"))
        out.update(sides("", prcptot, "prcptot"))
        if P:
            used = np.isin(np.arange(P), ids)
            maps = [a.maps() for a in per]
            prx = np.stack([m[0] for m in maps], axis=1)                      # [S, P, Kw, H, W]
            pcount = np.stack([m[1] for m in maps], axis=1)
            pprc = np.stack([m[2] for m in maps], axis=1)
            pdays = np.stack([m[3] for m in maps])
            assert (pdays[~used] == 0).all() and np.isnan(prx[:, ~used]).all() and np.isnan(pprc[:, ~used]).all()
            out["period_days"] = pdays
            out.update(sides("period_", prx, "rx"))
            out.update(sides("period_", pcount, "count"))
            out.update(sides("period_", pprc, "prcptot"))
            counts = pdays >= min_days
            for key, v, c in (("rx", prx.astype(f64), counts[:, None]), ("count", pcount.astype(f64), counts[:, None]),
                              ("prcptot", pprc.astype(f64), counts)):
                n, mean, std = _across(v, np.broadcast_to(c, v.shape[1:]))
                out.update(sides("", n, f"period_n_{key}"))
                out.update(sides("", mean, f"period_mean_{key}"))
                out.update(sides("", std, f"period_std_{key}"))
    return out
