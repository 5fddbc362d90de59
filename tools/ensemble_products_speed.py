"""Speed probe of the ensemble products (csrc/verify_products.hip) at the full DANRA domain, 589 x 789, with 5 quantile levels
and 4 thresholds, for ensembles of M = 16, 64 and 1000 members.  One JSON line: milliseconds per call (median of --reps timed
calls after a warm-up) of `verification.ensemble_products` and of a restatement in torch on the same device, written here:
torch.sort along the member axis, the type-7 lerp between the two neighbouring order statistics (in fp32), (ens >= thr).mean
over the members, and torch's mean and std.  The line also says whether the restatement reproduces the kernel's envelope and
exceedance maps exactly and how far its fp32 lerp is from the kernel's quantiles.

Usage: python tools/ensemble_products_speed.py [--reps 20] [--members 16 64 1000]"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from sbgm_danra_amd import verification as V  # noqa: E402

H, W = 589, 789
QUANTILES = [0.05, 0.25, 0.5, 0.75, 0.95]
THRESHOLDS = [-0.5, 0.0, 0.5, 1.0]


def time_ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def torch_products(ens):
    M = ens.shape[0]
    srt = torch.sort(ens, dim=0).values
    quant = []
    for q in QUANTILES:
        h = q * (M - 1)
        lo = math.floor(h)
        quant.append(torch.lerp(srt[lo], srt[min(lo + 1, M - 1)], h - lo))
    exceed = torch.stack([(ens >= t).float().mean(dim=0) for t in THRESHOLDS])
    return dict(mean=ens.mean(dim=0), std=ens.std(dim=0), min=srt[0], max=srt[-1], quantiles=torch.stack(quant), exceed_prob=exceed)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--members", type=int, nargs="+", default=[16, 64, 1000])
    args = ap.parse_args()
    dev = torch.device("cuda")
    out = {"shape": [H, W], "quantiles": len(QUANTILES), "thresholds": len(THRESHOLDS), "reps": args.reps,
           "device": torch.cuda.get_device_name(0), "members": {}}
    for M in args.members:
        g = torch.Generator(device=dev).manual_seed(M)
        ens = torch.randn(M, H, W, device=dev, generator=g)
        r, t = V.ensemble_products(ens, QUANTILES, THRESHOLDS), torch_products(ens)
        row = {"envelope_matches_torch": bool(torch.equal(r["min"], t["min"]) and torch.equal(r["max"], t["max"])),
               "exceed_matches_torch": bool(torch.equal(r["exceed_prob"], t["exceed_prob"])),
               "quantile_max_abs_diff_from_torch_fp32_lerp": float((r["quantiles"] - t["quantiles"]).abs().max())}
        del r, t
        row["ensemble_products"] = {"ms": round(time_ms(lambda: V.ensemble_products(ens, QUANTILES, THRESHOLDS), args.reps), 4)}
        row["torch_sort"] = {"ms": round(time_ms(lambda: torch_products(ens), args.reps), 4)}
        row["ensemble_gb"] = round(M * H * W * 4 / 1e9, 4)
        out["members"][str(M)] = row
        del ens
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
