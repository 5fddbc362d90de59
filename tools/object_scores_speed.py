"""Speed probe of the object-based scores (csrc/verify_objects.hip) at the full DANRA domain, 589 x 789, with three fixed
thresholds: 64 and 1000 generated fields against one truth (the `repeated` layout, No = 1), and one worst-case field, a
serpentine object that fills the domain, against itself.  Each case is compared with the host path on the same fields: the
download of the fields, scipy.ndimage.label and the numpy sums of tests/objects_ref.py.  The fields are seeded smoothed noise
shaped like precipitation (about 30 % wet, built here on the device).

The cases are timed in --loops alternating loops (default 6): every loop times one call of every case, so drift on a shared
host hits all of them alike; the line gives the minimum, the median and the maximum over the loops in milliseconds.  The host
path of the 1000-field case takes minutes a call and is timed in the first --host-large-loops loops only (default 1).  One JSON
line, also written to --out (default profiles/object_scores_speed.json).

Usage: python tools/object_scores_speed.py [--loops 6] [--host-large-loops 1] [--out PATH]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import objects_ref as R  # noqa: E402
from sbgm_danra_amd import verification as V  # noqa: E402

H, W = 589, 789
THRESHOLDS = [0.5, 2.0, 8.0]                  # mm-like units of the synthetic fields
CONNECTIVITY = 8


def precipitation_like(n, seed, dev):
    """n seeded fields [n,H,W]: white noise smoothed by three 9 x 9 box filters, standardised per field, then
    10 max(x - 0.5, 0)^2: smooth cells of a few tens of pixels over a dry background"""
    g = torch.Generator(device=dev).manual_seed(seed)
    out = torch.empty(n, H, W, device=dev)
    for i in range(0, n, 50):
        x = torch.randn(min(50, n - i), 1, H, W, device=dev, generator=g)
        for _ in range(3):
            x = F.avg_pool2d(x, 9, stride=1, padding=4, count_include_pad=False)
        x = (x - x.mean(dim=(2, 3), keepdim=True)) / x.std(dim=(2, 3), keepdim=True)
        out[i:i + x.shape[0]] = 10.0 * (x[:, 0] - 0.5).clamp_min(0.0).square()
    return out


def serpentine(dev):
    r, c = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    snake = (r % 2 == 0) | ((r % 4 == 1) & (c == W - 1)) | ((r % 4 == 3) & (c == 0))
    return torch.where(snake, 10.0 + (c % 8).float(), torch.zeros((), device=dev))[None]


def device_call(gen, obs):
    r = V.object_scores(gen, obs, THRESHOLDS, connectivity=CONNECTIVITY)
    torch.cuda.synchronize()
    return r


def host_call(gen, obs):
    """the host path: download, label, sum"""
    return R.object_scores(gen.cpu().numpy(), obs.cpu().numpy(), THRESHOLDS, None, None, CONNECTIVITY)


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
    ap.add_argument("--host-large-loops", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "object_scores_speed.json"))
    a = ap.parse_args()
    dev = torch.device("cuda")
    obs = precipitation_like(1, 1, dev)
    big = precipitation_like(1000, 2, dev)
    snake = serpentine(dev)
    data = {"fields_64": (big[:64], obs), "fields_1000": (big, obs), "serpentine_1": (snake, snake)}
    cases = {}
    for name, (g, o) in data.items():
        cases[f"device_{name}"] = (lambda g=g, o=o: device_call(g, o))
        cases[f"host_{name}"] = (lambda g=g, o=o: host_call(g, o))
    for name, (g, o) in data.items():                      # warm-up of every device shape
        device_call(g, o)
    times, last = {k: [] for k in cases}, {}
    for loop in range(a.loops):
        for name, fn in cases.items():
            if name == "host_fields_1000" and loop >= a.host_large_loops:
                continue
            ms, last[name] = timed(fn)
            times[name].append(ms)
    out = {"shape": [H, W], "thresholds": THRESHOLDS, "connectivity": CONNECTIVITY, "obs_fields": 1,
           "device": torch.cuda.get_device_name(0), "wet_fraction": round(float((big[:64] > 0).float().mean()), 4)}
    for name in cases:
        if times[name]:
            out[name] = summary(times[name])
    for name in data:
        d, h = last.get(f"device_{name}"), last.get(f"host_{name}")
        if d is None or h is None:
            continue
        same = all(np.array_equal(d[k].cpu().numpy(), h[k]) for k in ("n_objects", "area", "area_hist", "valid"))
        err = max(float(np.nanmax(np.abs(d[k].cpu().numpy() - h[k]), initial=0.0)) for k in ("S", "A", "L"))
        out[f"check_{name}"] = {"integers_equal": bool(same), "status": int(d["status"]), "max_abs_score_difference": err,
                                "objects_gen": int(h["n_objects"][0].sum()), "objects_obs": int(h["n_objects"][1].sum())}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
