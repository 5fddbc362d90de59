"""Speed probe of full-domain series generation at the config-5 geometry (589 x 789, tile 256, halo 32: 12 tiles, padded width 792) with
HR + two LR stacks + lsm + topo, one JSON line (also written to profiles/domain_generation_speed.json):

* "gather": ms per batch of 1 and of 8 days for `sbgm_domain_gather` (one launch, every field, padded rows) against `sbgm_cutout_gather`
  at full extent followed by `F.pad(mode="replicate")` of each field (what produced the padded layout before), both with the output
  allocation a loader makes per batch, z-score programs on the stacks, the mask flag on lsm and the min-max program on topo;
* "field": wall time per generated field (one day, one member, all 12 tiles in one batch) through ResidentDomainLoader -> extract_any ->
  FullDomainTiler.sample_series -> back-transform -> copy to the host, split into the time inside the sampler call (synchronised on both
  sides) and everything outside it (gather, assemble, extract, stitch, back-transform, copy), for `dpmpp_2m_sampler` at N = 16 and
  `pc_sampler` at 500 steps.

Six timed loops alternate between the cases of a part in one process after a warm-up of each; a gather loop repeats its case to at least
0.1 s of work, a field loop generates one field.  Median and min - max of the six; every timing ends in a device synchronise.
The model has the training initialisation and synthetic fields: this measures time, not sample quality.
Usage: python tools/domain_generation_speed.py [--loops 6] [--pc-steps 500] [--dpm-steps 16] [--days 8]"""
import argparse
import ctypes as C
import functools
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import yaml  # noqa: E402

import sbgm_danra_amd as S  # noqa: E402
from edm_sampler_speed import build, timed  # noqa: E402
from sbgm_danra_amd import _native as N  # noqa: E402
from sbgm_danra_amd import resident_data as RD  # noqa: E402
from sbgm_danra_amd import special_transforms as ST  # noqa: E402
from sbgm_danra_amd.config_loader import to_config  # noqa: E402
from sbgm_danra_amd.tiling import FullDomainTiler  # noqa: E402
from sbgm_danra_amd.utils import extract_any  # noqa: E402

STATS = {"prcp_hr": {"mean": 3.5, "std": 7.25}, "prcp_lr": {"mean": 2.5, "std": 5.5}, "temp_lr": {"mean": 8.7012, "std": 6.1923}}


def summary(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def config(path, tile):
    raw = yaml.safe_load(open(os.path.join(ROOT, "sbgm_danra_amd", "config", "default_config.yaml")))
    for sec in ("highres", "lowres"):
        raw[sec].update(data_size=[tile, tile])
    raw["highres"]["scaling_method"] = "zscore"
    raw["lowres"].update(condition_variables=["temp", "prcp"], scaling_methods=["zscore", "zscore"])
    raw["transforms"].update(scaling=True)
    raw["stationary_conditions"]["geographic_conditions"].update(sample_w_geo=True, geo_variables=["lsm", "topo"])
    raw["stationary_conditions"]["seasonal_conditions"]["sample_w_cond_season"] = False
    raw.setdefault("data_handling", {})["resident_fields"] = {"gen": path}
    return to_config(raw)


def gather_cases(loader, B):
    """the two ways to the padded batch [nf, B, 1, Hd, Wp] of the loader's plan"""
    F, lib, nf, Wp = loader.fields, N.lib(), len(loader.plan), loader.Wp
    items = torch.arange(B, dtype=torch.int32, device=F.device)
    origins = torch.zeros(B, 2, dtype=torch.int32, device=F.device)

    def pointers(block):
        srcs, dsts, counts = (N._vp * nf)(), (N._vp * nf)(), (C.c_int * nf)()
        for i, (_k, src, n, _m, _t) in enumerate(loader.plan):
            srcs[i], dsts[i], counts[i] = src.data_ptr(), block[i].data_ptr(), n
        return srcs, dsts, counts

    def domain():
        block = torch.empty(nf, B, 1, F.Hd, Wp, device=F.device)
        N.check(lib.sbgm_domain_gather(*pointers(block), nf, loader.programs.data_ptr(), items.data_ptr(), B, F.Hd, F.Wd, Wp, N.stream()))
        return block

    def cutout_then_pad():
        block = torch.empty(nf, B, 1, F.Hd, F.Wd, device=F.device)
        N.check(lib.sbgm_cutout_gather(*pointers(block), nf, loader.programs.data_ptr(), items.data_ptr(), origins.data_ptr(), B, F.Hd, F.Wd,
                                       F.Hd, F.Wd, N.stream()))
        return [torch.nn.functional.pad(block[i], (0, Wp - F.Wd, 0, 0), mode="replicate") for i in range(nf)]

    return {"domain_gather": domain, "cutout_gather_then_pad": cutout_then_pad}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--domain", type=int, nargs=2, default=[589, 789])
    ap.add_argument("--tile", type=int, default=256)
    ap.add_argument("--halo", type=int, default=32)
    ap.add_argument("--days", type=int, default=8)
    ap.add_argument("--loops", type=int, default=6)
    ap.add_argument("--pc-steps", type=int, default=500)
    ap.add_argument("--dpm-steps", type=int, default=16)
    a = ap.parse_args()
    Hd, Wd = a.domain
    rng = np.random.default_rng(0)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "gen.npz")
        np.savez(path, prcp_hr=(rng.random((a.days, Hd, Wd)) ** 4 * 60).astype(np.float32),
                 temp_lr=rng.normal(8, 6, (a.days, Hd, Wd)).astype(np.float32), prcp_lr=(rng.random((a.days, Hd, Wd)) ** 4 * 40).astype(np.float32),
                 lsm=(rng.random((Hd, Wd)) < 0.6).astype(np.float32), topo=(rng.random((Hd, Wd)) * 900).astype(np.float32))
        cfg = config(path, a.tile)
        fields = RD.ResidentFields(path, "prcp", ["temp", "prcp"])
    t = FullDomainTiler((Hd, Wd), a.tile, a.halo)
    out = {"shape": {"domain": a.domain, "tile": a.tile, "halo": a.halo, "tiles": len(t), "padded_width": t.Wd_pad, "fields": 5, "days": a.days},
           "loops": a.loops}

    # ---- the gather ----------------------------------------------------------------------------------------------------------------
    out["gather"] = {"unit": "ms_per_batch"}
    for B in (1, min(8, a.days)):
        loader = RD.ResidentDomainLoader(fields, cfg, t.Wd_pad, B, stats=STATS)
        cases = gather_cases(loader, B)
        a_, b_ = cases["domain_gather"](), cases["cutout_gather_then_pad"]()
        same = all(torch.equal(a_[i], b_[i]) for i in range(len(b_)))
        reps = {}
        for name, fn in cases.items():
            timed(fn)
            reps[name] = max(1, int(0.1 / max(timed(fn, 10)[0], 1e-6)) + 1)
        ms = {name: [] for name in cases}
        for _ in range(a.loops):
            for name, fn in cases.items():
                ms[name].append(timed(fn, reps[name])[0] * 1e3)
        row = {name: dict(summary(v), reps_per_loop=reps[name]) for name, v in ms.items()}
        row["bit_equal"] = same
        row["domain_over_cutout_then_pad"] = round(row["domain_gather"]["median"] / row["cutout_gather_then_pad"]["median"], 4)
        out["gather"][f"batch_{B}"] = row
        del a_, b_

    # ---- one generated field ---------------------------------------------------------------------------------------------------------
    net = build(6)
    loader = RD.ResidentDomainLoader(fields, cfg, t.Wd_pad, 1, stats=STATS)
    back = ST.ZScoreBackTransform(STATS["prcp_hr"]["mean"], STATS["prcp_hr"]["std"])
    host = torch.empty(1, 1, Hd, Wd)
    inside = [0.0]

    def clocked(sampler):
        @functools.wraps(sampler)                                     # the tiler inspects the sampler's signature
        def run(*args, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            x = sampler(*args, **kw)
            torch.cuda.synchronize()
            inside[0] += time.perf_counter() - t0
            return x
        return run

    def field(sampler, steps, day, **kw):
        batch = loader.gather(loader._items[day:day + 1])
        _x, _y, cond, _lh, lsm, _sdf, topo, _hp, _lp = extract_any(batch, fields.device)
        gen = t.sample_series(net, sampler, S.marginal_prob_std_fn, S.diffusion_coeff_fn, steps, cond_img=cond, lsm_cond=lsm[0],
                              topo_cond=topo[0], members=1, seed=1, first_day=day, **kw)
        host.copy_(back(gen))
        return host

    cases = {"dpmpp_2m_sampler": (clocked(S.dpmpp_2m_sampler), a.dpm_steps, {}), "pc_sampler": (clocked(S.pc_sampler), a.pc_steps, {})}
    finite = True
    for name, (fn, steps, kw) in cases.items():                       # warm-up: workspace sizing and the step graph's capture
        for _ in range(2):
            finite = finite and bool(torch.isfinite(timed(lambda: field(fn, steps, 0, **kw))[1]).all())
    total, samp = {n: [] for n in cases}, {n: [] for n in cases}
    for loop in range(a.loops):
        for name, (fn, steps, kw) in cases.items():
            inside[0] = 0.0
            dt, _ = timed(lambda: field(fn, steps, (loop + 1) % a.days, **kw))
            total[name].append(dt * 1e3)
            samp[name].append(inside[0] * 1e3)
    out["field"] = {"unit": "ms_per_field", "finite": finite}
    for name, (_fn, steps, _kw) in cases.items():
        outside = [tt - ss for tt, ss in zip(total[name], samp[name])]
        out["field"][name] = {"steps": steps, "total": summary(total[name]), "sampler": summary(samp[name]), "outside_sampler": summary(outside),
                              "outside_fraction": round(statistics.median(outside) / statistics.median(total[name]), 5)}
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "domain_generation_speed.json"), "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
