"""Speed probe of the pooled ensemble verification of a series (csrc/verify_series.hip) at the full DANRA domain, 589 x 789, with
M = 16 members, 4 thresholds and 4 groups (contiguous blocks of days, as seasons are), for records of D = 365 and 3650 days, with
the climatological reference on and off.  Each case is compared on the same fields with
  torch  — a restatement on the same device in fp64: broadcast pair differences [days, M, M, pixels] for the ensemble's pair sum
           (in chunks of --chunk days), torch.sort along the day axis for the climatology's pair sum (2 sum_k (2k - n + 1) y_(k),
           per row), masked reductions and bincount for the pooled sums, the rank histogram and the table.  The long record is
           timed in the first --long-torch-loops loops only (default 1).
The fields are seeded smoothed rain-like noise (a 5 x 5 box filter, then max(3 z - 2, 0): more than half exact zeros); truth and
members share half of their variance, so the ensemble is exchangeable with the truth; about 1 % of the truth is NaN.

The cases are timed in --loops alternating loops (default 6): every loop times one call of every case, so drift on a shared
host hits all of them alike; the line gives the minimum, the median and the maximum over the loops in milliseconds.  From the
minima: what the climatology costs (on minus off) and the pair terms it works through per second, n (n - 1) / 2 per pixel and
row.  The `check_<D>` entries compare the last device result with torch's: the integer table and the counts must be equal; the
rank histograms agree in their totals only (torch draws its own tie-breaks); the float outputs differ by rounding.
One JSON line, also written to --out (default profiles/series_scores_speed.json).  A record that does not fit into the free
device memory is reported as skipped, with the reason.

Usage: python tools/series_scores_speed.py [--loops 6] [--long-torch-loops 1] [--days 365 3650] [--chunk 8] [--out PATH]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from sbgm_danra_amd import verification as V  # noqa: E402

H, W, M, G = 589, 789, 16, 4
THRESHOLDS = [0.1, 1.0, 5.0, 10.0]
LONG = 1000                                    # records from this many days on are "long" for the torch restatement


def smooth(z):
    x = F.avg_pool2d(z.flatten(0, -3)[:, None], 5, stride=1, padding=2, count_include_pad=False)[:, 0]
    return (x / x.std(dim=(1, 2), keepdim=True)).view(z.shape)


def series(D, seed, dev):
    """ens [D, M, H, W], obs [D, H, W]: max(3 (a + b_m) / sqrt 2 - 2, 0) with a shared by the day's truth and members"""
    g = torch.Generator(device=dev).manual_seed(seed)
    ens, obs = torch.empty(D, M, H, W, device=dev), torch.empty(D, H, W, device=dev)
    for i in range(0, D, 10):
        n = min(10, D - i)
        a = smooth(torch.randn(n, 1, H, W, device=dev, generator=g))
        b = smooth(torch.randn(n, M + 1, H, W, device=dev, generator=g))
        x = torch.clamp_min(3.0 * (a + b) * 0.5 ** 0.5 - 2.0, 0.0)
        ens[i:i + n], o = x[:, :M], x[:, M]
        o[torch.rand(o.shape, device=dev, generator=g) < 0.01] = float("nan")
        obs[i:i + n] = o
    return ens, obs


def torch_scores(ens, obs, groups, climatology, chunk, seed=0):
    """the restatement; returns a dict under the names of verification.series_ensemble_scores (the maps flattened to [HW])"""
    D, dev = ens.shape[0], ens.device
    e2, o2 = ens.flatten(2), obs.flatten(1)
    P = e2.shape[2]
    f64, i64 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int64, device=dev)
    gen = torch.Generator(device=dev).manual_seed(seed)
    thr = torch.tensor(THRESHOLDS, device=dev)
    T = len(THRESHOLDS)
    n, sum_f, sum_v, sum_e = torch.zeros(P, **i64), torch.zeros(P, **f64), torch.zeros(P, **f64), torch.zeros(P, **f64)
    f_group = torch.zeros(G, P, **f64)
    day_sums = torch.zeros(D, 5, **f64)
    rank_hist, table = torch.zeros((G + 1) * (M + 1), **i64), torch.zeros((G + 1) * T * (M + 1) * 2, **i64)
    valid_all = torch.empty(D, P, dtype=torch.bool, device=dev)
    for d0 in range(0, D, chunk):
        e, y, g = e2[d0:d0 + chunk], o2[d0:d0 + chunk], groups[d0:d0 + chunk]
        valid = ~(torch.isnan(y) | torch.isnan(e).any(dim=1))
        valid_all[d0:d0 + chunk] = valid
        x, yd = e.double(), y.double()
        mean = x.mean(dim=1)
        sad = (x - yd[:, None]).abs().sum(dim=1)
        diff = x[:, :, None] - x[:, None, :]                                        # [days, M, M, P]
        pair, pair2 = diff.abs().sum(dim=(1, 2)), (diff * diff).sum(dim=(1, 2))
        del diff
        var = pair2 / (2.0 * M * (M - 1))
        cf, cs = sad / M - pair / (2.0 * M * (M - 1)), sad / M - pair / (2.0 * M * M)
        se = (mean - yd) ** 2
        zero = torch.zeros((), **f64)
        cols = [torch.where(valid, v, zero) for v in (cf, cs, se, var)]
        day_sums[d0:d0 + chunk] = torch.stack([valid.sum(1).double()] + [c.sum(1) for c in cols], dim=1)
        n += valid.sum(0)
        sum_f += cols[0].sum(0)
        sum_e += cols[2].sum(0)
        sum_v += cols[3].sum(0)
        f_group.index_add_(0, g, cols[0])
        lt, le = (e < y[:, None]).sum(1), (e <= y[:, None]).sum(1)
        u = torch.rand(y.shape, device=dev, generator=gen)
        r = torch.minimum(le, lt + torch.floor(u * (le - lt + 1)).long())
        row = (1 + g)[:, None].expand_as(r)
        rank_hist += torch.bincount((row * (M + 1) + r)[valid], minlength=rank_hist.numel())
        k = (e[:, :, None] >= thr[None, None, :, None]).sum(1)                       # [days, T, P]
        o = (y[:, None] >= thr[None, :, None]).long()
        idx = ((row[:, None] * T + torch.arange(T, device=dev)[None, :, None]) * (M + 1) + k) * 2
        v3 = valid[:, None].expand_as(k)
        table += torch.bincount(idx[v3], minlength=table.numel()) + torch.bincount((idx + 1)[v3 & (o > 0)], minlength=table.numel())
    rank_hist, table = rank_hist.view(G + 1, M + 1), table.view(G + 1, T, M + 1, 2)
    rank_hist[0], table[0] = rank_hist[1:].sum(0), table[1:].sum(0)
    nd = n.double()
    spread, skill = (sum_v / nd).sqrt(), (sum_e / nd).sqrt()
    out = {"count": n, "crps": (sum_f / nd).float(), "spread": spread.float(), "skill": skill.float(),
           "ssr": (((M + 1.0) / M) ** 0.5 * spread / skill).float(), "rank_hist": rank_hist, "table": table}

    def scores(v):
        sk, sp = (v[3] / v[0]).sqrt(), (v[4] / v[0]).sqrt()
        return torch.stack([v[0], v[1] / v[0], v[2] / v[0], sk, sp, ((M + 1.0) / M) ** 0.5 * sp / sk])
    out["daily"] = torch.stack([scores(v) for v in day_sums])
    rows = [torch.ones(D, dtype=torch.bool, device=dev)] + [groups == g for g in range(G)]
    out["scores"] = torch.stack([scores(day_sums[r].sum(0)) for r in rows])
    if climatology:
        kk = torch.arange(D, **f64)[:, None]
        skill_rows = []
        for ri, r in enumerate(rows):
            w = valid_all & r[:, None]
            nr = w.sum(0)
            ys = torch.sort(torch.where(w, o2, torch.full((), float("inf"), device=dev)), dim=0).values.double()
            S = 2.0 * torch.where(kk < nr, (2.0 * kk - nr + 1.0) * torch.where(torch.isinf(ys), 0.0, ys), 0.0).sum(0)
            del ys
            C = S / (2.0 * (nr.double() - 1.0))
            Fr = sum_f if ri == 0 else f_group[ri - 1]
            ok = nr >= 3
            if ri == 0:
                nan = torch.full((), float("nan"), **f64)
                out["clim_crps"] = torch.where(ok, C / nr, nan).float()
                out["crpss"] = torch.where(ok & (C != 0), 1.0 - Fr / C, nan).float()
            cells, sf, sc = nr[ok].sum().double(), Fr[ok].sum(), C[ok].sum()
            skill_rows.append(torch.stack([cells, sf / cells, sc / cells, 1.0 - sf / sc]))
        out["skill_scores"] = torch.stack(skill_rows)
    return out


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def summary(ts):
    return {"ms_min": round(min(ts), 3), "ms_median": round(float(np.median(ts)), 3), "ms_max": round(max(ts), 3), "loops": len(ts)}


def max_diff(a, b, relative=False):
    d = (a.double().flatten() - b.double().flatten()).abs()
    if relative:
        d = d / b.double().flatten().abs()
    d = d[~torch.isnan(d) & ~torch.isinf(d)]
    return float(d.max()) if d.numel() else 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loops", type=int, default=6)
    ap.add_argument("--long-torch-loops", type=int, default=1)
    ap.add_argument("--days", type=int, nargs="+", default=[365, 3650])
    ap.add_argument("--chunk", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "series_scores_speed.json"))
    a = ap.parse_args()
    dev = torch.device("cuda")
    out = {"shape": [H, W], "members": M, "days": a.days, "thresholds": THRESHOLDS, "groups": G, "chunk": a.chunk,
           "device": torch.cuda.get_device_name(0)}
    days = []
    try:
        ens_all, obs_all = series(max(a.days), 1, dev)
        days = list(a.days)
    except torch.cuda.OutOfMemoryError as err:
        free = torch.cuda.mem_get_info()[0]
        out[f"skipped_{max(a.days)}"] = f"{max(a.days)} days of {M} members need {max(a.days) * (M + 1) * H * W * 4 / 2**30:.0f} GiB; " \
                                        f"{free / 2**30:.0f} GiB were free ({type(err).__name__})"
        days = [d for d in a.days if d != max(a.days)]
        ens_all, obs_all = series(max(days), 1, dev)
    print(f"fields ready for {days} days", file=sys.stderr, flush=True)
    cases, long_cases = {}, set()
    for D in days:
        e, o = ens_all[:D], obs_all[:D]
        g = (torch.arange(D, device=dev) * G // D)
        gl = g.tolist()
        for name, clim in (("clim", True), ("noclim", False)):
            cases[f"device_{name}_{D}"] = (lambda e=e, o=o, gl=gl, clim=clim: V.series_ensemble_scores(e, o, THRESHOLDS, groups=gl, climatology=clim))
            cases[f"torch_{name}_{D}"] = (lambda e=e, o=o, g=g, clim=clim: torch_scores(e, o, g, clim, a.chunk))
            if D >= LONG:
                long_cases.add(f"torch_{name}_{D}")
    for name, fn in cases.items():                          # warm-up of every device shape; the long torch cases warm up on the short record
        if name not in long_cases:
            timed(fn)
    times, last = {k: [] for k in cases}, {}
    for loop in range(a.loops):
        for name, fn in cases.items():
            if name in long_cases and loop >= a.long_torch_loops:
                continue
            ms, last[name] = timed(fn)
            times[name].append(ms)
            print(f"loop {loop + 1}: {name} {ms:.1f} ms", file=sys.stderr, flush=True)
    for name in cases:
        if times[name]:
            out[name] = summary(times[name])
    for D in days:
        d, t = last[f"device_clim_{D}"], last.get(f"torch_clim_{D}")
        s = (out[f"device_clim_{D}"]["ms_min"] - out[f"device_noclim_{D}"]["ms_min"]) * 1e-3
        n = d["count"].flatten().double()
        pairs = float((n * (n - 1) / 2).sum()) * 2                       # row 0, and the groups' rows together about 1 / G of it each
        out[f"climatology_{D}"] = {"seconds": round(s, 6), "share_of_call": round(s * 1e3 / out[f"device_clim_{D}"]["ms_min"], 4),
                                   "pair_terms_row0": pairs / 2, "pair_terms_per_s_row0_only": round(pairs / 2 / s, -6) if s > 0 else None}
        if t is None:
            continue
        out[f"check_{D}"] = {
            "count_equal_torch": bool(torch.equal(d["count"].flatten().long(), t["count"])),
            "table_equal_torch": bool(torch.equal(d["table"], t["table"])),
            "rank_hist_totals_equal_torch": bool(torch.equal(d["rank_hist"].sum(1), t["rank_hist"].sum(1))),
            "crps_map_max_abs_diff": max_diff(d["crps"], t["crps"]), "ssr_map_max_rel_diff": max_diff(d["ssr"], t["ssr"], True),
            "scores_max_rel_diff": max_diff(d["scores"], t["scores"], True), "daily_max_rel_diff": max_diff(d["daily"], t["daily"], True),
            "clim_crps_max_rel_diff": max_diff(d["clim_crps"], t["clim_crps"], True),
            "skill_scores_max_rel_diff": max_diff(d["skill_scores"], t["skill_scores"], True),
            "pooled_crpss_device": float(d["skill_scores"][0, 3]), "pooled_crpss_torch": float(t["skill_scores"][0, 3])}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
