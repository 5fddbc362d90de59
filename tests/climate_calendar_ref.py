"""numpy restatement of the calendar-aware, grouped climate indices (verification.climate_indices with `day_numbers` and
`groups`), by composition with tests/climate_ref.py and with no arithmetic of its own: the contract says
that a broken link acts exactly as one invalid day between the two days, and that group g is the subsequence of its days with
their own day numbers.  So: select the days, insert an all-NaN day into gen and obs at every broken link (if nothing is left,
pad with one NaN day), and call climate_ref.climate_indices."""
import numpy as np

import climate_ref as R


def expand(gen, obs, mask, day_numbers, sel):
    """(gen, obs, mask) of the days `sel` (ascending positions) with an all-NaN day inserted at every broken link"""
    gen, obs = np.asarray(gen, np.float32), np.asarray(obs, np.float32)
    sel = np.asarray(sel, np.int64)
    dn = np.arange(gen.shape[0], dtype=np.int64) if day_numbers is None else np.asarray(day_numbers, np.int64)
    daily = mask is not None and np.asarray(mask).ndim == 3
    hole = np.full(gen.shape[1:], np.nan, np.float32)
    g, o, m = [], [], []
    for i, t in enumerate(sel):
        if i > 0 and dn[t] != dn[sel[i - 1]] + 1:
            g.append(hole), o.append(hole)
            if daily:
                m.append(np.ones_like(mask[0]))                  # the inserted day is invalid whatever the mask says
        g.append(gen[t]), o.append(obs[t])
        if daily:
            m.append(mask[t])
    if not g:
        g.append(hole), o.append(hole)
        if daily:
            m.append(np.ones_like(mask[0]))
    return np.stack(g), np.stack(o), (np.stack(m) if daily else mask)


def climate_indices(gen, obs, wet=1.0, quantiles=(), wet_quantiles=(), mask=None, day_numbers=None, groups=None):
    """the dict of the device call: climate_ref's keys for the record and, with groups, `group_days` and `group_<key>`
    with a leading [G] axis, G = the largest id + 1"""
    n = np.asarray(gen).shape[0]
    a, b, m = expand(gen, obs, mask, day_numbers, np.arange(n))
    out = R.climate_indices(a, b, wet, quantiles, wet_quantiles, m)
    if groups is not None:
        ids = np.asarray(groups, np.int64)
        per = []
        for g in range(int(ids.max()) + 1):
            a, b, m = expand(gen, obs, mask, day_numbers, np.flatnonzero(ids == g))
            per.append(R.climate_indices(a, b, wet, quantiles, wet_quantiles, m))
        out.update({f"group_{k}": np.stack([p[k] for p in per]) for k in per[0]})
    return out
