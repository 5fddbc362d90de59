"""Speed probe of the domain noise plan at the config-5 geometry: the 12 tiles of a 589 x 789 domain (tile 256, halo 32, one low-res
condition, eval mode, no autotune) as one batch, one JSON line: ms per predictor-corrector step (30 steps, one captured step graph
replayed per step) as independent tiles ("tiled") and as one joint diffusion ("joint"), each for

* no plan (the tiled sampler as it is without the arguments),
* a plan of one lag (`noise_domain_row` alone: the row-keyed domain counter, no mixing),
* plans of 4, 16 and 32 lags (`temporal_noise_weights(0.6, K)`),

each from six timed loops (a loop repeats its run to at least 0.25 s of work) that alternate between the cases in one process, after a
warm-up run of each: the median and the min - max of the six, and the cost per lag and step as the slope between K = 1 and K = 32 (a
predictor-corrector step draws twice).  `--no-plan-only` times the first case of each form alone and touches none of the new arguments,
so the same file measures the parent commit; run the two in alternating processes to compare them.

Every timing ends in a device synchronise.  Usage: python tools/domain_series_speed.py [--steps 30] [--loops 6] [--no-plan-only]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import sbgm_danra_amd as S  # noqa: E402
from edm_sampler_speed import build, timed  # noqa: E402
from sbgm_danra_amd.tiling import FullDomainTiler  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--domain", type=int, nargs=2, default=[589, 789])
    ap.add_argument("--tile", type=int, default=256)
    ap.add_argument("--halo", type=int, default=32)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--loops", type=int, default=6)
    ap.add_argument("--no-plan-only", action="store_true")
    a = ap.parse_args()
    n = a.steps
    net = build(1)
    t = FullDomainTiler(tuple(a.domain), a.tile, a.halo)
    T = len(t)
    cond = t.extract(torch.randn(1, *a.domain, generator=torch.Generator().manual_seed(1)).cuda())
    std = (S.marginal_prob_std_fn, S.diffusion_coeff_fn)
    kw = dict(num_steps=n, batch_size=T, device="cuda", img_size=a.tile, cond_img=cond, seed=1, tile_origins=t.origins_dev,
              domain_width=t.Wd_pad)
    forms = {"tiled": {}, "joint": dict(joint_tiles=(t.Hd, max(1, t.overlap)))}
    runs = {}
    for form, extra in forms.items():
        runs[f"{form}_no_plan"] = lambda extra=extra: S.pc_sampler(net, *std, **kw, **extra)
        if a.no_plan_only:
            continue
        for K in (1, 4, 16, 32):
            w = S.temporal_noise_weights(0.6, K) if K > 1 else [1.0]
            runs[f"{form}_k{K}"] = lambda extra=extra, K=K, w=w: S.pc_sampler(net, *std, **kw, **extra, noise_domain_row=K - 1 + 365,
                                                                              domain_height=t.Hd, noise_weights=w)
    reps, finite = {}, True
    for name, fn in runs.items():                                  # warm-up: workspace sizing, step-graph capture; then the loop length
        timed(fn)
        t_one, x = timed(fn)
        reps[name] = max(1, int(0.25 / max(t_one, 1e-6)) + 1)
        finite = finite and bool(torch.isfinite(x).all())
    per_step = {name: [] for name in runs}
    for _ in range(a.loops):                                       # the cases alternate: each recaptures its step graph per loop
        for name, fn in runs.items():
            dt, _ = timed(fn, reps[name])
            per_step[name].append(dt / n * 1e3)
    out = {"shape": {"domain": a.domain, "tile": a.tile, "halo": a.halo, "tiles": T, "n_cond": 1}, "sampler": "pc_sampler", "loops": a.loops,
           "steps": n, "finite": finite, "unit": "ms_per_step"}
    for name, v in per_step.items():
        out[name] = {"reps_per_loop": reps[name], "median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    if not a.no_plan_only:
        for form in forms:
            out[f"{form}_us_per_lag_and_step"] = round((out[f"{form}_k32"]["median"] - out[f"{form}_k1"]["median"]) / 31 * 1e3, 3)
            out[f"{form}_k1_over_no_plan"] = round(out[f"{form}_k1"]["median"] / out[f"{form}_no_plan"]["median"], 4)
            out[f"{form}_k32_over_no_plan"] = round(out[f"{form}_k32"]["median"] / out[f"{form}_no_plan"]["median"], 4)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
