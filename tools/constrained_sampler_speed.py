"""Cost of constrained sampling (known pixels held) at the C2 shape (B = 32, 128 x 128, one low-res condition, eval mode,
no autotune, step graph on), one JSON line: ms per step of Euler_Maruyama_sampler, pc_sampler and edm_heun_sampler without a constraint
("free") and with a 5 % Bernoulli mask ("held"), in the same process.  A held and an unheld run never share a step graph, so the two forms
are timed in alternating blocks (free, held, free, held), each block after one warm-up run that captures the form's graph; the median and
the min..max of a form's `--reps` runs are reported, so the difference can be read against the run-to-run spread (drift would show up as
a difference between a form's two blocks, inside its spread).  Every timing ends in a device synchronise.

Usage: python tools/constrained_sampler_speed.py [--em-steps 200] [--pc-steps 100] [--edm-steps 32] [--reps 5]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import sbgm_danra_amd as S  # noqa: E402
from tools.edm_sampler_speed import build  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--hw", type=int, default=128)
    ap.add_argument("--em-steps", type=int, default=200)
    ap.add_argument("--pc-steps", type=int, default=100)
    ap.add_argument("--edm-steps", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--mask-fraction", type=float, default=0.05)
    a = ap.parse_args()
    B, HW = a.batch, a.hw
    net = build(1)
    g = torch.Generator().manual_seed(1)
    cond = torch.randn(B, 1, HW, HW, generator=g).cuda()
    known = torch.randn(B, 1, HW, HW, generator=g).cuda()
    mask = (torch.rand(B, 1, HW, HW, generator=g) < a.mask_fraction).float().cuda()
    kw = dict(batch_size=B, device="cuda", img_size=HW, cond_img=cond, seed=1, use_graph=True)
    held = dict(known=known, known_mask=mask)
    std = (S.marginal_prob_std_fn, S.diffusion_coeff_fn)
    res = {"shape": {"B": B, "H": HW, "W": HW, "n_cond": 1}, "mask_fraction": round(float(mask.mean()), 4), "reps": a.reps}
    finite = True
    for name, fn, steps in (("em", S.Euler_Maruyama_sampler, a.em_steps), ("pc", S.pc_sampler, a.pc_steps),
                            ("edm_heun", S.edm_heun_sampler, a.edm_steps)):
        ms = {"free": [], "held": []}
        for block in range(2):                                    # free, held, free, held: drift shows up as a block difference
            for form, extra in (("free", {}), ("held", held)):
                run = lambda: fn(net, *std, num_steps=steps, **kw, **extra)  # noqa: E731
                timed(run)                                        # warm-up: the form's step graph is captured here
                for _ in range((a.reps + 1 - block) // 2):
                    t, x = timed(run)
                    ms[form].append(t / steps * 1e3)
                    finite = finite and bool(torch.isfinite(x).all())
        res[name] = {"steps": steps,
                     "free_ms_per_step": round(statistics.median(ms["free"]), 4), "held_ms_per_step": round(statistics.median(ms["held"]), 4),
                     "free_spread": [round(min(ms["free"]), 4), round(max(ms["free"]), 4)],
                     "held_spread": [round(min(ms["held"]), 4), round(max(ms["held"]), 4)],
                     "held_over_free": round(statistics.median(ms["held"]) / statistics.median(ms["free"]), 4)}
    res["finite"] = finite
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
