"""Speed probe of the calendar-aware, grouped climate indices (csrc/verify_temporal.hip, K61 and the slabs of K55 - K57) at the full
DANRA domain, 589 x 789, for records of N = 365 and 3650 days with three `quantiles` and two `wet_quantiles`, wet-day threshold
1.0; the fields are those of tools/climate_indices_speed.py.  Per record length:
  plain      — the unchanged call, day_numbers=None, groups=None;
  parent     — with --parent-lib PATH: sbgm_climate_indices of a libsbgm_hip.so built from the parent commit, called through ctypes
               on the same tensors (the entry's signature did not change), so case 1 compares the two builds in one session;
  calendar   — day numbers with about 2 % of the links broken, no groups (slab 0 alone, through the tables);
  seasons    — real dates from 2011-01-01 on, grouped by season (G = 4), with the same 2 % of broken links;
  by_hand    — what a user does without groups: four index_select copies of gen and obs and four plain calls.
The cases are timed in --loops alternating loops (default 6): every loop times one call of every case, so drift on a shared host
hits all of them alike; each entry gives the minimum, the median and the maximum over the loops in milliseconds.  `check_<N>`:
the seasons' maps of the grouped call against the four calls by hand, which know no calendar: the order-free indices are bit-equal
(the spells and pairs differ, because the copies run the winters of different years together); one group of all days against the
plain call, bit for bit; and, with --parent-lib, the plain call against the parent's.  One JSON line, also written to --out (default
profiles/climate_calendar_speed.json).

Usage: python tools/climate_calendar_speed.py [--loops 6] [--days 365 3650] [--parent-lib PATH] [--out PATH]"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from climate_indices_speed import H, QUANTILES, W, WET, WET_QUANTILES, rain, summary, timed  # noqa: E402
from sbgm_danra_amd import _native as N  # noqa: E402
from sbgm_danra_amd import calendar as cal  # noqa: E402
from sbgm_danra_amd import verification as V  # noqa: E402

ORDER_FREE = ("mean", "wet_freq", "sdii", "max", "quantiles", "wet_quantiles", "heavy_fraction")


def parent_call(path):
    """gen, obs -> None: sbgm_climate_indices of the library at `path` with its own outputs and workspace, as the wrapper allocates
    them"""
    lib = C.CDLL(path)
    res, args = N.SIGNATURES["sbgm_climate_indices"]
    lib.sbgm_climate_indices.restype, lib.sbgm_climate_indices.argtypes = res, args
    lib.sbgm_climate_indices_workspace_bytes.restype = C.c_int64
    lib.sbgm_climate_indices_workspace_bytes.argtypes = N.SIGNATURES["sbgm_climate_indices_workspace_bytes"][1]
    Q, QW = len(QUANTILES), len(WET_QUANTILES)
    q, qw = (C.c_double * Q)(*QUANTILES), (C.c_double * QW)(*WET_QUANTILES)

    def call(g, o):
        n, HW, dev = g.shape[0], H * W, g.device
        i32 = dict(dtype=torch.int32, device=dev)
        days, spells, trans = torch.empty(HW, **i32), torch.empty(2, 2, HW, **i32), torch.empty(2, 4, HW, **i32)
        stats = torch.empty(2, len(V.CLIMATE_STATS), HW, device=dev)
        quant, wquant, heavy = torch.empty(2, Q, HW, device=dev), torch.empty(2, QW, HW, device=dev), torch.empty(2, QW, HW, device=dev)
        nbytes = lib.sbgm_climate_indices_workspace_bytes(n, H, W, Q, QW)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        rc = lib.sbgm_climate_indices(g.data_ptr(), o.data_ptr(), None, 0, n, 1, H, W, WET, q, Q, qw, QW, days.data_ptr(), stats.data_ptr(),
                                      spells.data_ptr(), trans.data_ptr(), quant.data_ptr(), wquant.data_ptr(), heavy.data_ptr(),
                                      ws.data_ptr(), nbytes, N.stream())
        if rc:
            raise RuntimeError(f"parent sbgm_climate_indices returned {rc}")
        return {"days": days.view(H, W), "gen_mean": stats[0, 0].view(H, W), "gen_quantiles": quant[0].view(Q, H, W),
                "obs_heavy_fraction": heavy[1].view(QW, H, W), "gen_cwd": spells[0, 0].view(H, W)}
    return call


def dates_with_holes(n, broken):
    """n day numbers from 2011-01-01 on; with `broken`, about 2 % of the links skip 1..7 days (seeded)"""
    rng = np.random.default_rng(n)
    step = np.where(rng.random(n) < 0.02, rng.integers(2, 9, size=n), 1) if broken else np.ones(n, np.int64)
    step[0] = 0
    return cal.parse_origin("2011-01-01") + np.cumsum(step)


def by_hand(g, o, ids):
    out = []
    for s in range(4):
        sel = torch.nonzero(ids == s)[:, 0]
        out.append(V.climate_indices(g.index_select(0, sel), o.index_select(0, sel), WET, QUANTILES, WET_QUANTILES))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loops", type=int, default=6)
    ap.add_argument("--days", type=int, nargs="+", default=[365, 3650])
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "climate_calendar_speed.json"))
    a = ap.parse_args()
    dev = torch.device("cuda")
    gen_all, obs_all = rain(max(a.days), 1, dev), rain(max(a.days), 2, dev)
    parent = parent_call(a.parent_lib) if a.parent_lib else None
    cases, setup = {}, {}
    for n in a.days:
        g, o = gen_all[:n], obs_all[:n]
        dn = dates_with_holes(n, True)
        ids = cal.groups_from_dates(dn, "season")[0]
        ids_dev = torch.tensor(ids, device=dev)
        setup[n] = (g, o, dn, ids, ids_dev)
        cases[f"plain_{n}"] = (lambda g=g, o=o: V.climate_indices(g, o, WET, QUANTILES, WET_QUANTILES))
        if parent is not None:
            cases[f"parent_{n}"] = (lambda g=g, o=o: parent(g, o))
        cases[f"calendar_{n}"] = (lambda g=g, o=o, dn=dn: V.climate_indices(g, o, WET, QUANTILES, WET_QUANTILES, day_numbers=dn))
        cases[f"seasons_{n}"] = (lambda g=g, o=o, dn=dn, ids=ids: V.climate_indices(g, o, WET, QUANTILES, WET_QUANTILES, day_numbers=dn,
                                                                                     groups=ids))
        cases[f"by_hand_{n}"] = (lambda g=g, o=o, ids_dev=ids_dev: by_hand(g, o, ids_dev))
    for fn in cases.values():                               # warm-up of every device shape
        timed(fn)
    times, last = {k: [] for k in cases}, {}
    for loop in range(a.loops):
        for name, fn in cases.items():
            ms, last[name] = timed(fn)
            times[name].append(ms)
        print(f"loop {loop + 1} of {a.loops} done", file=sys.stderr, flush=True)
    out = {"shape": [H, W], "days": a.days, "wet": WET, "quantiles": QUANTILES, "wet_quantiles": WET_QUANTILES,
           "device": torch.cuda.get_device_name(0), "parent_lib": bool(parent)}
    for name in cases:
        out[name] = summary(times[name])
    same = lambda x, y: bool(torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)))   # noqa: E731
    for n in a.days:
        g, o, dn, ids, ids_dev = setup[n]
        p = out[f"plain_{n}"]["ms_min"]
        out[f"ratios_{n}"] = {"calendar_over_plain": round(out[f"calendar_{n}"]["ms_min"] / p, 4),
                              "seasons_over_plain": round(out[f"seasons_{n}"]["ms_min"] / p, 4),
                              "by_hand_over_seasons": round(out[f"by_hand_{n}"]["ms_min"] / out[f"seasons_{n}"]["ms_min"], 4),
                              "links_broken": int((~cal.links(dn)[1:]).sum()), "season_days": [ids.count(s) for s in range(4)]}
        chk = {}
        if parent is not None:
            out[f"ratios_{n}"]["plain_over_parent"] = round(p / out[f"parent_{n}"]["ms_min"], 4)
            chk["plain_bit_equal_parent"] = all(same(last[f"plain_{n}"][k], v) for k, v in last[f"parent_{n}"].items())
        grouped, hand = last[f"seasons_{n}"], last[f"by_hand_{n}"]
        chk["order_free_bit_equal_by_hand"] = all(same(grouped[f"group_{s}_{k}"][q], hand[q][f"{s}_{k}"])
                                                  for s in ("gen", "obs") for k in ORDER_FREE for q in range(4))
        # unbroken dates: a season's days are consecutive except across the years, which the copies by hand run together
        whole = V.climate_indices(g, o, WET, QUANTILES, WET_QUANTILES, groups=[0] * n)
        chk["one_group_bit_equal_plain"] = all(same(whole[f"group_{k}"][0], v) for k, v in last[f"plain_{n}"].items())
        out[f"check_{n}"] = chk
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
