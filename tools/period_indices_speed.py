"""Speed probe of the period climate indices (verification.period_indices; csrc/verify_periods.hip, K62 - K64) at the full DANRA
domain, 589 x 789: records of N = 365 and 3650 days, M = 1 and 16 members, windows (1, 5), thresholds (10, 20), wet-day
threshold 1.0, without periods and with years of 365 days; the fields are those of tools/climate_indices_speed.py, one seed per
member.  Per (N, M, periods):
  device — the call;
  torch  — a restatement in torch on the same device, over chunks of pixels: paired validity, `unfold` window sums in fp64 with
           `amax`, masked counts and sums, per year by slices of the day axis, then the mean and spread across the years.  It
           sums in another order and need not be bit-equal; `check_*` gives the largest relative deviation of its float maps
           from the device call's and whether the integer maps are equal.
The cases are timed in --loops alternating loops (default 6): every loop times one call of every case, so drift on a shared host
hits all of them alike; each entry gives the minimum, the median and the maximum over the loops in milliseconds.  `traffic_*`:
the bytes one pass over the record must read (every series once, plus its validity bits), the bytes the call reads (K62's
validity pass reads every series once more) and the GB/s either figure makes of the device call's fastest time; the first is a
lower bound of what the sweep K63 reaches, since the call's time also holds K62 and K64.  One JSON line, also written to --out
(default profiles/period_indices_speed.json).

Usage: python tools/period_indices_speed.py [--loops 6] [--days 365 3650] [--members 1 16] [--windows 1 5] [--chunk 32768]
       [--no-torch] [--out PATH]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from climate_indices_speed import H, W, WET, rain, summary, timed  # noqa: E402
from sbgm_danra_amd import verification as V  # noqa: E402

WINDOWS, THRESHOLDS, YEAR = (1, 5), (10.0, 20.0), 365


def torch_indices(gen, obs, ids, chunk):
    """gen [M, N, H, W], obs [N, H, W], ids None or a list of contiguous years -> dict of [.., HW] maps, gen_ with [M]"""
    M, n = gen.shape[:2]
    g2, o2 = gen.flatten(2), obs.flatten(1)
    P = 0 if ids is None else max(ids) + 1
    bounds = [(ids.index(g), len(ids) - ids[::-1].index(g)) for g in range(P)]
    parts = []
    nan = float("nan")
    for p0 in range(0, o2.shape[1], chunk):
        x = torch.cat([g2[:, :, p0:p0 + chunk], o2[None, :, p0:p0 + chunk]])            # [S, N, C]
        valid = ~torch.isnan(x).any(dim=0)
        x64 = torch.where(valid, x, nan).double()
        wet = torch.where(valid & (x >= WET), x64, 0.0)
        above = [valid & (x >= t) for t in THRESHOLDS]
        sums = [x64.unfold(1, K, 1).sum(-1) if K <= n else x64[:, :0] for K in WINDOWS]   # NaN where a day of the window is invalid

        def rx(s, lo, hi):
            """largest window sum over the windows ending in days lo..hi-1"""
            out = []
            for K, w in zip(WINDOWS, s):
                w = w[:, max(lo - K + 1, 0):max(hi - K + 1, 0)]
                best = torch.nan_to_num(w, nan=-float("inf")).amax(dim=1) if w.shape[1] else torch.full_like(x64[:, 0], -float("inf"))
                out.append(torch.where(torch.isinf(best) & (best < 0), nan, best).float())
            return torch.stack(out, dim=1)                                              # [S, Kw, C]

        def block(lo, hi):
            days = valid[lo:hi].sum(0)
            return dict(days=days.int(), rx=rx(sums, lo, hi), count=torch.stack([a[:, lo:hi].sum(1).int() for a in above], dim=1),
                        prcptot=torch.where(days > 0, wet[:, lo:hi].sum(1), nan).float())

        res = block(0, n)
        if P:
            per = [block(lo, hi) for lo, hi in bounds]
            for k in ("days", "rx", "count", "prcptot"):
                res[f"period_{k}"] = torch.stack([b[k] for b in per], dim=0 if k == "days" else 1)
            for k in ("rx", "count", "prcptot"):
                v = res[f"period_{k}"].double()
                ok = ~torch.isnan(v) & (res["period_days"] > 0).reshape((1, P) + (1,) * (v.dim() - 3) + (-1,))
                cnt = ok.sum(1)
                mean = torch.where(ok, v, 0.0).sum(1) / cnt
                ss = torch.where(ok, (v - mean.unsqueeze(1)) ** 2, 0.0).sum(1)
                res[f"period_n_{k}"], res[f"period_mean_{k}"] = cnt.int(), mean.float()
                res[f"period_std_{k}"] = torch.where(cnt > 1, torch.sqrt(ss / (cnt - 1)), nan).float()
        parts.append(res)
    return {k: torch.cat([p[k] for p in parts], dim=-1) for k in parts[0]}


def compare(dev, ref, M):
    """largest relative deviation of the float maps, and whether the integer maps are equal"""
    worst, ints = 0.0, True
    for k, r in ref.items():
        if k in ("days", "period_days"):
            ints &= bool(torch.equal(dev[k].flatten(-2), r))
            continue
        for side, sel in (("gen", slice(0, M)), ("obs", M)):
            name = f"period_{side}_{k[7:]}" if k.startswith("period_") and k[7:] in V.PERIOD_INDICES else f"{side}_{k}"
            d, w = dev[name].flatten(-2), r[sel]
            if w.dtype == torch.int32:
                ints &= bool(torch.equal(d, w))
            else:
                ints &= bool(torch.equal(torch.isnan(d), torch.isnan(w)))
                both = ~torch.isnan(d) & ~torch.isnan(w)
                if both.any():
                    worst = max(worst, float(((d[both] - w[both]).abs() / w[both].abs().clamp_min(1e-6)).max()))
    return {"largest_relative_deviation": worst, "integer_maps_and_nan_positions_equal": ints}


def main():
    global WINDOWS
    ap = argparse.ArgumentParser()
    ap.add_argument("--loops", type=int, default=6)
    ap.add_argument("--days", type=int, nargs="+", default=[365, 3650])
    ap.add_argument("--members", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--windows", type=int, nargs="+", default=list(WINDOWS), help="other window lengths, e.g. 3 12 or 5 32")
    ap.add_argument("--chunk", type=int, default=32768)
    ap.add_argument("--no-torch", action="store_true", help="time the device call alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "period_indices_speed.json"))
    a = ap.parse_args()
    WINDOWS = tuple(a.windows)
    dev = torch.device("cuda")
    n_max, m_max = max(a.days), max(a.members)
    obs_all = rain(n_max, 2, dev)
    gen_all = torch.empty(m_max, n_max, H, W, device=dev)
    for m in range(m_max):
        gen_all[m] = rain(n_max, 100 + m, dev) if m else rain(n_max, 1, dev)
    cases = {}
    for n in a.days:
        years = [t // YEAR for t in range(n)]
        for M in a.members:
            g, o = gen_all[:M, :n], obs_all[:n]                           # a strided view: the members are not copied
            for tag, ids in (("record", None), ("years", years)):
                key = f"N{n}_M{M}_{tag}"
                cases[f"device_{key}"] = (lambda g=g, o=o, ids=ids: V.period_indices(g, o, WINDOWS, THRESHOLDS, WET, periods=ids))
                if not a.no_torch:
                    cases[f"torch_{key}"] = (lambda g=g, o=o, ids=ids: torch_indices(g, o, ids, a.chunk))
    for fn in cases.values():                                             # warm-up of every device shape
        timed(fn)
    times, last = {k: [] for k in cases}, {}
    for loop in range(a.loops):
        for name, fn in cases.items():
            ms, out = timed(fn)
            times[name].append(ms)
            if loop == a.loops - 1 and (name.startswith("device_") or "_M1_" in name):     # the check runs at M = 1
                last[name] = out
            del out
        print(f"loop {loop + 1} of {a.loops} done", file=sys.stderr, flush=True)
    out = {"shape": [H, W], "days": a.days, "members": a.members, "windows": list(WINDOWS), "thresholds": list(THRESHOLDS), "wet": WET,
           "year_days": YEAR, "device": torch.cuda.get_device_name(0)}
    for name in cases:
        out[name] = summary(times[name])
    for name in [k for k in cases if k.startswith("device_")]:
        key = name[len("device_"):]
        n, M = int(key.split("_")[0][1:]), int(key.split("_")[1][1:])
        ms = out[name]["ms_min"]
        sweep = (M + 1) * n * H * W * 4 + (M + 1) * ((n + 31) // 32) * H * W * 4
        call = sweep + (M + 1) * n * H * W * 4
        out[f"traffic_{key}"] = {"sweep_bytes": sweep, "call_bytes": call, "sweep_bytes_over_call_time_GBps": round(sweep / ms / 1e6, 1),
                                 "call_bytes_over_call_time_GBps": round(call / ms / 1e6, 1)}
        if f"torch_{key}" in out:
            t = out[f"torch_{key}"]["ms_min"]
            out[f"ratio_{key}"] = {"torch_over_device": round(t / ms, 3), "ahead": "device" if ms < t else "torch"}
            if f"torch_{key}" in last:
                out[f"check_{key}"] = compare(last[name], last[f"torch_{key}"], M)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
