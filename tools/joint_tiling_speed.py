"""Cost of joint full-domain sampling (tile scores blended at every step) at the config-5 geometry: the 12 tiles of a
589 x 789 domain (tile 256, halo 32, one low-res condition, eval mode, no autotune, step graph on) as one batch, one JSON line: ms per step
of pc_sampler and edm_heun_sampler as independent tiles ("tiled") and as one joint diffusion ("joint"), in the same process.  A joint and
a non-joint run never share a step graph, so the two forms are timed in alternating blocks (tiled, joint, tiled, joint), each block after
one warm-up run that captures the form's graph; the median and the min..max of a form's `--reps` runs are reported, so the difference can
be read against the run-to-run spread.  Every timing ends in a device synchronise.

Usage: python tools/joint_tiling_speed.py [--pc-steps 30] [--edm-steps 16] [--reps 5]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import sbgm_danra_amd as S  # noqa: E402
from sbgm_danra_amd.tiling import FullDomainTiler  # noqa: E402
from tools.constrained_sampler_speed import timed  # noqa: E402
from tools.edm_sampler_speed import build  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--domain", type=int, nargs=2, default=[589, 789])
    ap.add_argument("--tile", type=int, default=256)
    ap.add_argument("--halo", type=int, default=32)
    ap.add_argument("--pc-steps", type=int, default=30)
    ap.add_argument("--edm-steps", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    net = build(1)
    t = FullDomainTiler(tuple(a.domain), a.tile, a.halo)
    T = len(t)
    cond = t.extract(torch.randn(1, *a.domain, generator=torch.Generator().manual_seed(1)).cuda())
    kw = dict(batch_size=T, device="cuda", img_size=a.tile, cond_img=cond, seed=1, use_graph=True, tile_origins=t.origins_dev,
              domain_width=t.Wd_pad)
    joint = dict(joint_tiles=(t.Hd, max(1, t.overlap)))
    std = (S.marginal_prob_std_fn, S.diffusion_coeff_fn)
    res = {"shape": {"domain": a.domain, "tile": a.tile, "halo": a.halo, "tiles": T, "n_cond": 1}, "reps": a.reps}
    finite = True
    for name, fn, steps in (("pc", S.pc_sampler, a.pc_steps), ("edm_heun", S.edm_heun_sampler, a.edm_steps)):
        ms = {"tiled": [], "joint": []}
        for block in range(2):                                    # tiled, joint, tiled, joint: drift shows up as a block difference
            for form, extra in (("tiled", {}), ("joint", joint)):
                run = lambda: fn(net, *std, num_steps=steps, **kw, **extra)  # noqa: E731
                timed(run)                                        # warm-up: the form's step graph is captured here
                for _ in range((a.reps + 1 - block) // 2):
                    dt, x = timed(run)
                    ms[form].append(dt / steps * 1e3)
                    finite = finite and bool(torch.isfinite(x).all())
        res[name] = {"steps": steps,
                     "tiled_ms_per_step": round(statistics.median(ms["tiled"]), 4), "joint_ms_per_step": round(statistics.median(ms["joint"]), 4),
                     "tiled_spread": [round(min(ms["tiled"]), 4), round(max(ms["tiled"]), 4)],
                     "joint_spread": [round(min(ms["joint"]), 4), round(max(ms["joint"]), 4)],
                     "joint_over_tiled": round(statistics.median(ms["joint"]) / statistics.median(ms["tiled"]), 4)}
    res["finite"] = finite
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
