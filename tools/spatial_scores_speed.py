"""Speed probe of the neighbourhood and threshold-exceedance scores (csrc/verify_spatial.hip) at the full DANRA domain,
589 x 789: N = 64 generated fields against one truth each, an ensemble of M = 64 members, 4 thresholds and the 7 window
widths 1 .. 65.  One JSON line: milliseconds per call (median of --reps timed calls after a warm-up) of the two entry points
and of a restatement in torch on the same device, written here: the window sums as avg_pool2d (divisor_override=1, zero
padding) over the indicator images, the exceedance table as a comparison, a sum over the members and a bincount.  The line
also says whether the restatements reproduce the kernels' integers.

Usage: python tools/spatial_scores_speed.py [--reps 20]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from sbgm_danra_amd import verification as V  # noqa: E402

H, W, NS, M = 589, 789, 64, 64
THRESHOLDS = [-0.5, 0.0, 0.5, 1.0]
SCALES = [1, 3, 5, 9, 17, 33, 65]


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


def torch_neighbourhood(gen, obs, mask):
    """num, den int64 [N,T,S]: window counts are at most 65^2, exact in fp32; the squares are summed in fp64 (exact below 2^53)"""
    valid = ~(torch.isnan(gen) | torch.isnan(obs)) & mask.bool()
    num = torch.empty(gen.shape[0], len(THRESHOLDS), len(SCALES), dtype=torch.int64, device=gen.device)
    den = torch.empty_like(num)
    for t, thr in enumerate(THRESHOLDS):
        ig = (valid & (gen >= thr)).float()[:, None]
        io = (valid & (obs >= thr)).float()[:, None]
        for s, n in enumerate(SCALES):
            cg = F.avg_pool2d(ig, n, stride=1, padding=n // 2, divisor_override=1).double()
            co = F.avg_pool2d(io, n, stride=1, padding=n // 2, divisor_override=1).double()
            num[:, t, s] = (cg - co).square().sum(dim=(1, 2, 3)).long()
            den[:, t, s] = (cg.square() + co.square()).sum(dim=(1, 2, 3)).long()
    return num, den


def torch_exceedance(ens, obs, mask):
    """table int64 [T, M+1, 2]"""
    valid = ~(torch.isnan(ens).any(0) | torch.isnan(obs)) & mask.bool()
    rows = []
    for thr in THRESHOLDS:
        k = (ens >= thr).sum(0)
        o = (obs >= thr).long()
        rows.append(torch.bincount((k * 2 + o)[valid], minlength=2 * (M + 1)).view(M + 1, 2))
    tab = torch.stack(rows)
    return torch.stack([tab.sum(-1), tab[..., 1]], dim=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    reps = ap.parse_args().reps
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    gen = torch.randn(NS, H, W, device=dev, generator=g)
    obs = torch.randn(NS, H, W, device=dev, generator=g)
    ens = torch.randn(M, H, W, device=dev, generator=g)
    mask = (torch.rand(H, W, device=dev, generator=g) < 0.6).to(torch.uint8)
    r = V.neighbourhood_scores(gen, obs, THRESHOLDS, SCALES, mask=mask)
    num, den = torch_neighbourhood(gen, obs, mask)
    x = V.exceedance_scores(ens, obs[0], THRESHOLDS, mask=mask)
    out = {"shape": [H, W], "N": NS, "M": M, "thresholds": len(THRESHOLDS), "scales": SCALES, "reps": reps,
           "device": torch.cuda.get_device_name(0),
           "neighbourhood_matches_torch": bool(torch.equal(r["num"], num) and torch.equal(r["den"], den)),
           "exceedance_matches_torch": bool(torch.equal(x["table"], torch_exceedance(ens, obs[0], mask)))}
    cases = {"neighbourhood_scores": lambda: V.neighbourhood_scores(gen, obs, THRESHOLDS, SCALES, mask=mask),
             "neighbourhood_torch": lambda: torch_neighbourhood(gen, obs, mask),
             "exceedance_scores": lambda: V.exceedance_scores(ens, obs[0], THRESHOLDS, mask=mask),
             "exceedance_torch": lambda: torch_exceedance(ens, obs[0], mask)}
    for name, fn in cases.items():
        out[name] = {"ms": round(time_ms(fn, reps), 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
