"""Speed probe of the multivariate ensemble scores (csrc/verify_multivariate.hip) at the full DANRA domain, 589 x 789, for
M = 16, 64 and 1000 members against one truth: the energy score, and the variogram score of order 0.5 at radius 4 and 8 with
inverse-distance weights.  Each case is compared on the same fields with
  torch  — a restatement on the same device: torch.cdist in fp64 for the distance matrix, in its default mode (a matrix product:
           the Gram form) and from differences ("exact"), and shifted-slice differences (one offset at a time over all
           members) for the variogram; and
  host   — the numpy restatement of tests/multivariate_ref.py on 16 host threads (rows of the distance matrix, offsets of the
           variogram), downloads included; M = 16 and 64 only, in the first --host-loops loops (default 1): it takes seconds
           to minutes a call.
The fields are seeded smoothed noise (members: one 5 x 5 box filter; truth: three), all pixels valid.

The cases are timed in --loops alternating loops (default 6): every loop times one call of every case, so drift on a shared
host hits all of them alike; the line gives the minimum, the median and the maximum over the loops in milliseconds.  From the
minimum: the energy kernels' fp64 rate, counting 3 operations (subtract, multiply, add) for each of the (M+1) M / 2 distinct
pairs and each pixel, against the vector-fp64 peak (the call includes the validity pass and the reductions, so this is the
rate of the whole call, not of the pair kernel alone); and the variogram's terms per second, a term being one |x_i - x_j|^p
of one member, offset and pixel.  One JSON line, also written to --out (default profiles/multivariate_scores_speed.json).

Usage: python tools/multivariate_scores_speed.py [--loops 6] [--host-loops 1] [--members 16 64 1000] [--out PATH]"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import multivariate_ref as R  # noqa: E402
from sbgm_danra_amd import verification as V  # noqa: E402

H, W = 589, 789
ORDER, WEIGHTS, RADII = 0.5, "inverse_distance", (4, 8)
HOST_THREADS, HOST_MAX_MEMBERS = 16, 64
PEAK_FP64_VECTOR = 78.6e12        # FLOP/s, datasheet: half the 157.3 TFLOP/s fp32 vector peak


def smooth_noise(n, passes, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    out = torch.empty(n, H, W, device=dev)
    for i in range(0, n, 50):
        x = torch.randn(min(50, n - i), 1, H, W, device=dev, generator=g)
        for _ in range(passes):
            x = F.avg_pool2d(x, 5, stride=1, padding=2, count_include_pad=False)
        out[i:i + x.shape[0]] = (x / x.std(dim=(2, 3), keepdim=True))[:, 0]
    return out


def torch_energy(ens, obs, exact):
    """dist2 [M+1, M+1] and es_fair by torch.cdist in fp64 (all pixels valid): in its default mode, which forms |a|^2 + |b|^2 -
    2 <a, b> with a matrix product above 25 rows, or — `exact` — from differences"""
    x = torch.cat([ens.flatten(1), obs.flatten()[None]]).double()
    d = torch.cdist(x, x, compute_mode="donot_use_mm_for_euclid_dist" if exact else "use_mm_for_euclid_dist_if_necessary")
    M, dist = ens.shape[0], d / (H * W) ** 0.5
    return d * d, dist[:M, M].mean() - dist[:M, :M].sum() / (2.0 * M * (M - 1))


def torch_variogram(ens, obs, radius):
    """vs by shifted slices, one offset at a time (all pixels valid)"""
    num = den = torch.zeros((), dtype=torch.float64, device=ens.device)
    for dy, dx in V.variogram_offsets(radius):
        w = R.offset_weight(dy, dx, WEIGHTS)
        ys, xs = slice(0, H - dy), slice(max(0, -dx), W - max(0, dx))
        yt, xt = slice(dy, H), slice(max(0, dx), W + min(0, dx))
        ge = (ens[:, ys, xs] - ens[:, yt, xt]).abs_().sqrt_().sum(dim=0, dtype=torch.float64) / ens.shape[0]
        go = (obs[ys, xs] - obs[yt, xt]).abs().sqrt().double()
        num = num + w * (go - ge).square().sum()
        den = den + w * ge.numel()
    return num / den


def host_energy(ens, obs, pool):
    e, o = ens.cpu().numpy(), obs.cpu().numpy()
    chunks = np.array_split(np.arange(e.shape[0] + 1), HOST_THREADS)
    parts = list(pool.map(lambda rows: R.energy_rows(e, o, rows=list(rows))[0], [c for c in chunks if len(c)]))
    d2 = np.concatenate(parts)
    return d2, R.energy_scores_from_dist2(d2, H * W)


def host_variogram(ens, obs, radius, pool):
    e, o = ens.cpu().numpy(), obs.cpu().numpy()
    v = R.valid_pixels(e, o)
    parts = list(pool.map(lambda d: R.variogram_offset(e, o, v, d[0], d[1], ORDER, R.offset_weight(d[0], d[1], WEIGHTS)),
                          R.offsets(radius)))
    return R.variogram_scores(e, o, radius=radius, order=ORDER, weights=WEIGHTS, per_offset=parts)


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def summary(ts):
    return {"ms_min": round(min(ts), 3), "ms_median": round(float(np.median(ts)), 3), "ms_max": round(max(ts), 3), "loops": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loops", type=int, default=6)
    ap.add_argument("--host-loops", type=int, default=1)
    ap.add_argument("--members", type=int, nargs="+", default=[16, 64, 1000])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multivariate_scores_speed.json"))
    a = ap.parse_args()
    dev = torch.device("cuda")
    obs = smooth_noise(1, 3, 1, dev)[0]
    big = smooth_noise(max(a.members), 1, 2, dev)
    pool = ThreadPoolExecutor(HOST_THREADS)
    cases, host = {}, set()
    for M in a.members:
        ens = big[:M]
        cases[f"device_energy_{M}"] = (lambda e=ens: V.energy_scores(e, obs))
        cases[f"torch_energy_{M}"] = (lambda e=ens: torch_energy(e, obs, False))
        cases[f"torch_energy_exact_{M}"] = (lambda e=ens: torch_energy(e, obs, True))
        for r in RADII:
            cases[f"device_variogram_r{r}_{M}"] = (lambda e=ens, r=r: V.variogram_scores(e, obs, radius=r, order=ORDER, weights=WEIGHTS))
            cases[f"torch_variogram_r{r}_{M}"] = (lambda e=ens, r=r: torch_variogram(e, obs, r))
        if M <= HOST_MAX_MEMBERS:
            cases[f"host_energy_{M}"] = (lambda e=ens: host_energy(e, obs, pool))
            host.add(f"host_energy_{M}")
            for r in RADII:
                cases[f"host_variogram_r{r}_{M}"] = (lambda e=ens, r=r: host_variogram(e, obs, r, pool))
                host.add(f"host_variogram_r{r}_{M}")
    for name, fn in cases.items():                          # warm-up of every device shape
        if name not in host:
            timed(fn)
    times, last = {k: [] for k in cases}, {}
    for loop in range(a.loops):
        for name, fn in cases.items():
            if name in host and loop >= a.host_loops:
                continue
            ms, last[name] = timed(fn)
            times[name].append(ms)
        print(f"loop {loop + 1} of {a.loops} done", file=sys.stderr, flush=True)
    out = {"shape": [H, W], "members": a.members, "order": ORDER, "weights": WEIGHTS, "radii": list(RADII),
           "device": torch.cuda.get_device_name(0), "host_threads": HOST_THREADS, "peak_fp64_vector_flops": PEAK_FP64_VECTOR}
    for name in cases:
        if times[name]:
            out[name] = summary(times[name])
    for M in a.members:
        s = out[f"device_energy_{M}"]["ms_min"] * 1e-3
        flops = 3.0 * (M + 1) * M / 2 * H * W / s
        out[f"rate_energy_{M}"] = {"fp64_flops": round(flops, -9), "share_of_vector_fp64_peak": round(flops / PEAK_FP64_VECTOR, 4)}
        d, t, tx = last[f"device_energy_{M}"], last[f"torch_energy_{M}"], last[f"torch_energy_exact_{M}"]
        off = ~torch.eye(M + 1, dtype=torch.bool, device=dev)
        chk = {"dist2_max_rel_vs_torch": float(((d["dist2"] - t[0]).abs() / d["dist2"])[off].max()),
               "dist2_max_rel_vs_torch_exact": float(((d["dist2"] - tx[0]).abs() / d["dist2"])[off].max()),
               "es_fair": float(d["scores"][1]), "es_fair_torch": float(t[1]), "es_fair_torch_exact": float(tx[1])}
        if f"host_energy_{M}" in last:
            h = last[f"host_energy_{M}"]
            chk["dist2_max_rel_vs_host"] = float(np.max(np.abs(d["dist2"].cpu().numpy() - h[0]) / np.maximum(h[0], 1e-300)))
            chk["es_fair_host"] = float(h[1][1])
        out[f"check_energy_{M}"] = chk
        for r in RADII:
            n_off = len(V.variogram_offsets(r))
            s = out[f"device_variogram_r{r}_{M}"]["ms_min"] * 1e-3
            d = last[f"device_variogram_r{r}_{M}"]
            out[f"rate_variogram_r{r}_{M}"] = {"terms_per_s": round(float(d["scores"][1]) * M / s, -6), "offsets": n_off}
            chk = {"vs": float(d["scores"][0]), "vs_torch": float(last[f"torch_variogram_r{r}_{M}"])}
            if f"host_variogram_r{r}_{M}" in last:
                h = last[f"host_variogram_r{r}_{M}"]
                chk.update(vs_host=float(h["scores"][0]), pairs_equal_host=bool(np.array_equal(d["pairs"].cpu().numpy(), h["pairs"])))
            out[f"check_variogram_r{r}_{M}"] = chk
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
