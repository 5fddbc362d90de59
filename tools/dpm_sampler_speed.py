"""Speed probe of dpmpp_2m_sampler at the C2 shape (B = 32, 128 x 128, one low-res condition, eval mode, no autotune), one JSON line:

* ms per network evaluation of Euler_Maruyama_sampler (200 steps), edm_heun_sampler (N = 32: 63 evaluations) and dpmpp_2m_sampler
  (N = 32: 32 evaluations) at eta = 0 and eta = 1.  All of them replay one captured step graph per step, so the figures should agree;
* each from six timed loops (a loop repeats its sampler to at least 0.25 s of work) that alternate between the four samplers in one
  process, after a warm-up run of each: the median and the min - max of the six;
* wall time per batch at N = 32 of the two few-step samplers.

Every timing ends in a device synchronise.  Usage: python tools/dpm_sampler_speed.py [--steps 32] [--em-steps 200] [--loops 6]"""
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
    ap.add_argument("--em-steps", type=int, default=200)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--loops", type=int, default=6)
    a = ap.parse_args()
    B, HW, n = a.batch, a.hw, a.steps
    net = build(1)
    cond = torch.randn(B, 1, HW, HW, generator=torch.Generator().manual_seed(1)).cuda()
    kw = dict(batch_size=B, device="cuda", img_size=HW, cond_img=cond, seed=1)
    std = (S.marginal_prob_std_fn, S.diffusion_coeff_fn)
    runs = {                                                       # name: (the run, its network evaluations)
        "em": (lambda: S.Euler_Maruyama_sampler(net, *std, num_steps=a.em_steps, **kw), a.em_steps),
        "edm": (lambda: S.edm_heun_sampler(net, *std, num_steps=n, **kw), 2 * n - 1),
        "dpm": (lambda: S.dpmpp_2m_sampler(net, *std, num_steps=n, **kw), n),
        "dpm_sde": (lambda: S.dpmpp_2m_sampler(net, *std, num_steps=n, eta=1.0, **kw), n),
    }
    reps, finite = {}, True
    for name, (fn, _) in runs.items():                             # warm-up: workspace sizing, step-graph capture; then the loop length
        timed(fn)
        t_one, x = timed(fn)
        reps[name] = max(1, int(0.25 / max(t_one, 1e-6)) + 1)
        finite = finite and bool(torch.isfinite(x).all())
    per_eval = {name: [] for name in runs}
    wall = {name: [] for name in runs}
    for _ in range(a.loops):                                       # the samplers alternate: each recaptures its step graph per loop
        for name, (fn, nfe) in runs.items():
            t, _ = timed(fn, reps[name])
            wall[name].append(t)
            per_eval[name].append(t / nfe * 1e3)
    out = {"shape": {"B": B, "H": HW, "W": HW, "n_cond": 1}, "loops": a.loops, "steps": n, "em_steps": a.em_steps, "finite": finite}
    for name, (_, nfe) in runs.items():
        v = per_eval[name]
        out[name] = {"nfe": nfe, "reps_per_loop": reps[name], "ms_per_eval": round(statistics.median(v), 4),
                     "ms_per_eval_min": round(min(v), 4), "ms_per_eval_max": round(max(v), 4)}
        if name != "em":
            out[name]["s_per_batch"] = round(statistics.median(wall[name]), 4)
    lo, hi = out["edm"]["ms_per_eval_min"], out["edm"]["ms_per_eval_max"]
    v = out["dpm"]["ms_per_eval"]
    out["dpm_vs_edm_spread"] = "below" if v < lo else "above" if v > hi else "within"
    out["dpm_over_edm_per_eval"] = round(out["dpm"]["ms_per_eval"] / out["edm"]["ms_per_eval"], 4)
    out["edm_over_dpm_wall"] = round(out["edm"]["s_per_batch"] / out["dpm"]["s_per_batch"], 3)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
