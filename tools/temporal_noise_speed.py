"""Speed probe of the row-keyed noise plan at the C2 shape (B = 32, 128 x 128, one low-res condition, eval mode, no autotune), one JSON
line: ms per Euler-Maruyama step (200 steps, one captured step graph replayed per step) for

* no plan (the sampler as it is without the arguments),
* a plan of one lag (`noise_rows` alone: the row-keyed counter, no mixing),
* plans of 4, 16 and 32 lags (`temporal_noise_weights(0.6, K)`),

each from six timed loops (a loop repeats its run to at least 0.25 s of work) that alternate between the cases in one process, after a
warm-up run of each: the median and the min - max of the six, and the cost per lag as the slope between K = 1 and K = 32.
`--no-plan-only` times the first case alone and touches none of the new arguments, so the same file measures the parent commit.

Every timing ends in a device synchronise.  Usage: python tools/temporal_noise_speed.py [--steps 200] [--loops 6] [--no-plan-only]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--hw", type=int, default=128)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--loops", type=int, default=6)
    ap.add_argument("--no-plan-only", action="store_true")
    a = ap.parse_args()
    B, HW, n = a.batch, a.hw, a.steps
    net = build(1)
    cond = torch.randn(B, 1, HW, HW, generator=torch.Generator().manual_seed(1)).cuda()
    std = (S.marginal_prob_std_fn, S.diffusion_coeff_fn)
    run = lambda **plan: S.Euler_Maruyama_sampler(net, *std, num_steps=n, batch_size=B, device="cuda", img_size=HW, cond_img=cond,  # noqa: E731
                                                  seed=1, **plan)
    runs = {"no_plan": lambda: run()}
    if not a.no_plan_only:
        for K in (1, 4, 16, 32):
            rows = torch.arange(B, dtype=torch.int32) + (K - 1)
            w = S.temporal_noise_weights(0.6, K) if K > 1 else [1.0]
            runs[f"k{K}"] = lambda rows=rows, w=w: run(noise_rows=rows, noise_weights=w)
    reps, finite = {}, True
    for name, fn in runs.items():                                  # warm-up: workspace sizing, step-graph capture; then the loop length
        timed(fn)
        t_one, x = timed(fn)
        reps[name] = max(1, int(0.25 / max(t_one, 1e-6)) + 1)
        finite = finite and bool(torch.isfinite(x).all())
    per_step = {name: [] for name in runs}
    for _ in range(a.loops):                                       # the cases alternate: each recaptures its step graph per loop
        for name, fn in runs.items():
            t, _ = timed(fn, reps[name])
            per_step[name].append(t / n * 1e3)
    out = {"shape": {"B": B, "H": HW, "W": HW, "n_cond": 1}, "loops": a.loops, "steps": n, "finite": finite, "unit": "ms_per_step"}
    for name, v in per_step.items():
        out[name] = {"reps_per_loop": reps[name], "median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    if not a.no_plan_only:
        out["us_per_lag"] = round((out["k32"]["median"] - out["k1"]["median"]) / 31 * 1e3, 3)
        out["k1_over_no_plan"] = round(out["k1"]["median"] / out["no_plan"]["median"], 4)
        out["k32_over_no_plan"] = round(out["k32"]["median"] / out["no_plan"]["median"], 4)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
