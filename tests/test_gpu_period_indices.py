"""GPU suite for the period climate indices (verification.period_indices; csrc/verify_periods.hip)
against the numpy restatement tests/period_indices_ref.py.  Every output is asserted bit-equal to it (int32 views, as
test_gpu_climate_calendar.py compares): the kernels run the restatement's IEEE fp64 operations in its order — window sums from
+0.0, oldest day first; the wet-day sum in day order; the across-period sums in id order — and round to fp32 once, or at
points where rounding early gives the same value (a maximum: rounding is monotone)."""
import functools

import numpy as np
import pytest
import torch

import period_indices_ref as PR
import test_gpu_climate as T
import test_gpu_climate_calendar as TC
from sbgm_danra_amd import verification as V

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
f32 = np.float32
SHAPES = [(5, 7), (37, 53)]                       # fewer pixels than a wave; 8 workgroups, the last one partly filled
MASKS = [None, ("hw", "uint8"), ("nhw", "float32")]
THR8 = [0.0, 0.25, 1.0, 1.5, 2.0, 3.0, 4.75, 10.0]
WET = 1.0
MEMBERS = ["3d", "m1", "m3"]
PERIODS = [None, "years90", "runs", "sparse", "minus", "p256"]


def make_periods(rng, kind, N):
    """years90: contiguous ids t // 90.  runs: ids 0..3 in season-like runs of 2..9 days that recur.  sparse: ids 0, 2 and 5 in
    runs (1, 3, 4 and 6 unused) and id 7 on exactly one day.  minus: runs of ids -1, 0, 1, 2, beginning and ending with -1.
    p256: 256 ids in time order, one or two days each."""
    if kind is None:
        return None
    if kind == "years90":
        return np.arange(N) // 90
    if kind == "p256":
        return np.arange(N) * 256 // N
    pool = {"runs": [0, 1, 2, 3], "sparse": [0, 2, 5], "minus": [-1, 0, 1, 2]}[kind]
    ids, last = [], None
    while len(ids) < N:
        g = pool[rng.integers(len(pool))]
        if g != last:
            ids += [g] * int(rng.integers(2, 10))
            last = g
    ids = np.asarray(ids[:N], np.int64)
    if kind == "sparse":
        ids[N // 2] = 7
    if kind == "minus":
        ids[:2], ids[-2:] = -1, -1
        ids[N // 2] = 2                                                      # P = 3 whatever was drawn
    return ids


def make_members(rng, kind, N, shape):
    """(gen [N,H,W] or [M,N,H,W], obs): test_gpu_climate's rain series (2 % NaN a side, the planted pixels of row 0); further
    members carry their own NaN days, so a day can be invalid through one member only; the planted pixels stay whole"""
    gen, obs = T.make_series(rng, "rain", N, shape)
    if kind == "3d":
        return gen, obs
    if kind == "m1":
        return gen[None], obs
    more = [T.make_series(rng, "rain", N, shape)[0] for _ in range(2)]
    for a in more:
        a[:, 0, :5] = np.where(np.isnan(a[:, 0, :5]), f32(0.25), a[:, 0, :5])
    return np.stack([gen] + more), obs


@functools.lru_cache(maxsize=None)
def _case(shape, N, windows, n_thr, members, mask_index, links, periods, min_days):
    rng = np.random.default_rng([SHAPES.index(shape), N, len(windows), n_thr, MEMBERS.index(members), mask_index,
                                 TC.LINKS.index(links), PERIODS.index(periods), min_days])
    gen, obs = make_members(rng, members, N, shape)
    mask = T.make_mask(rng, MASKS[mask_index], N, shape)
    dn = None if links == "none" else TC.make_day_numbers(rng, links, N)
    ids = make_periods(rng, periods, N)
    thr = THR8[:n_thr]
    return gen, obs, mask, dn, ids, thr, PR.period_indices(gen, obs, windows, thr, WET, mask, dn, ids, min_days)


def device_call(gen, obs, windows, thr, mask=None, dn=None, ids=None, min_days=1, permuted=False, wet=WET):
    """permuted: a 4-D gen goes to the device as [N, M, H, W] and is passed as the permuted, non-contiguous [M, N, H, W] view"""
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)   # noqa: E731
    g = t(gen.transpose(1, 0, 2, 3)).permute(1, 0, 2, 3) if permuted else t(gen)
    assert not permuted or (gen.shape[0] > 1 and not g.is_contiguous())
    r = V.period_indices(g, t(obs), windows, thr, wet, mask=t(mask), day_numbers=dn, periods=None if ids is None else ids.tolist(),
                         min_days=min_days)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


def run_lengths(gen, obs, mask, dn):
    """int [N, H, W]: r[t] of the definition"""
    N = obs.shape[0]
    g4 = gen if gen.ndim == 4 else gen[None]
    valid = PR.admitted(mask, N, obs.shape[1:]) & ~np.isnan(g4).any(axis=0) & ~np.isnan(obs)
    link = PR.linked(dn, N)
    r = np.zeros((N, *obs.shape[1:]), np.int64)
    for t in range(N):
        r[t] = np.where(valid[t], (r[t - 1] if t > 0 and link[t] else 0) + 1, 0)
    return r


# (shape, N, windows, thresholds, members, mask, links, periods, min_days).  All links broken leaves windows of one day only, and a
# random 10 % leaves hardly a run of 32 days: those cases ask for what can exist, so that no case passes by being empty.
CASES = [
    (SHAPES[0], 2, (1, 5), 0, "3d", 0, "none", None, 1),                     # a window longer than N
    (SHAPES[1], 2, (1,), 8, "m1", 1, "all", None, 1),
    (SHAPES[0], 5, (2, 3, 5, 32), 8, "m3", 0, "none", None, 1),
    (SHAPES[1], 5, (1, 5), 0, "3d", 2, "none", None, 1),
    (SHAPES[1], 33, (2, 3, 5, 32), 8, "m3", 1, "none", "runs", 1),
    (SHAPES[0], 33, (1, 5), 0, "m1", 2, "edges", "sparse", 1),
    (SHAPES[1], 33, (1,), 8, "3d", 0, "all", None, 1),
    (SHAPES[0], 70, (1, 5), 8, "m3", 1, "edges", "minus", 1),
    (SHAPES[1], 70, (2, 3, 5, 32), 0, "3d", 2, "edges", "runs", 1),
    (SHAPES[0], 70, (1, 5), 8, "m1", 0, "random", "sparse", 1),
    (SHAPES[1], 70, (3, 12), 8, "m1", 0, "edges", "runs", 1),                # a largest window in 9..16: the 16-slot ring
    (SHAPES[1], 400, (1, 5), 8, "m3", 1, "random", "years90", 40),
    (SHAPES[0], 400, (2, 3, 5, 32), 0, "3d", 0, "none", "years90", 1),
    (SHAPES[1], 400, (1, 5), 8, "m1", 2, "edges", "runs", 1),
    (SHAPES[0], 400, (1, 5), 0, "m1", 1, "random", "minus", 40),
    (SHAPES[1], 300, (1, 5), 8, "m3", 0, "none", "p256", 1),
    (SHAPES[1], 1500, (1, 5), 8, "m3", 1, "random", "runs", 1),
]


@pytest.mark.parametrize("shape,N,windows,n_thr,members,mask_index,links,periods,min_days", CASES)
def test_against_the_restatement(shape, N, windows, n_thr, members, mask_index, links, periods, min_days):
    gen, obs, mask, dn, ids, thr, want = _case(shape, N, windows, n_thr, members, mask_index, links, periods, min_days)
    # not vacuous: the largest window that fits the record exists at some pixel and is missing at another
    fits = [k for k, K in enumerate(windows) if K <= N]
    for side in ("gen", "obs"):
        top = want[f"{side}_rx"][..., fits[-1], :, :]
        assert np.isnan(top).any() and (~np.isnan(top)).any(), side
        for k in range(len(windows)):
            if k not in fits:
                assert np.isnan(want[f"{side}_rx"][..., k, :, :]).all()
    assert (want["days"] == 0).any() and (want["days"] == N).any() and (np.isnan(gen).mean() > 0.015)
    if members == "m3":                                                      # a day invalid through one member only
        assert (np.isnan(gen).sum(axis=0) == 1).any() and gen.shape[0] == 3
    if ids is not None:
        P = int(ids.max()) + 1
        assert want["period_days"].shape == (P, *shape) and want["period_gen_rx"].shape[-4:] == (P, len(windows), *shape)
        K2 = min(K for K in windows if K >= 2)
        change = np.flatnonzero(ids[1:] != ids[:-1]) + 1
        assert (run_lengths(gen, obs, mask, dn)[change] >= K2).any(), "no window spans an id change"
        assert (want["gen_period_n_rx"] >= 2).any() and not np.isnan(want["obs_period_std_prcptot"]).all()
        if min_days > 1:                                                     # and min_days drops a period somewhere
            assert ((want["period_days"] > 0) & (want["period_days"] < min_days)).any()
    else:
        assert "period_days" not in want
    got = device_call(gen, obs, windows, thr, mask, dn, ids, min_days, permuted=members == "m3")
    TC.bit_equal(got, want, f"{shape} N={N} windows={windows} T={n_thr} {members} mask={MASKS[mask_index]} links={links} periods={periods}")


def test_the_cases_cover_every_pattern():
    assert {c[0] for c in CASES} == set(SHAPES) and {c[1] for c in CASES} == {2, 5, 33, 70, 400, 300, 1500}
    assert {c[2] for c in CASES} == {(1,), (1, 5), (3, 12), (2, 3, 5, 32)} and {c[3] for c in CASES} == {0, 8}
    assert {c[4] for c in CASES} == set(MEMBERS) and {c[5] for c in CASES} == set(range(len(MASKS)))
    assert {c[6] for c in CASES} == set(TC.LINKS) and {c[7] for c in CASES} == set(PERIODS) and {c[8] for c in CASES} == {1, 40}
    rng = np.random.default_rng(0)
    assert make_periods(rng, "years90", 400).tolist() == (np.arange(400) // 90).tolist()
    p = make_periods(rng, "p256", 300)
    assert p.max() == 255 and len(set(p.tolist())) == 256 and (np.diff(p) >= 0).all()
    sparse = make_periods(rng, "sparse", 70)
    assert set(sparse.tolist()) == {0, 2, 5, 7} and (sparse == 7).sum() == 1
    runs = make_periods(rng, "runs", 400)
    assert set(runs.tolist()) == {0, 1, 2, 3} and all((np.diff(np.flatnonzero(runs == g)) > 1).any() for g in range(4))   # they recur
    minus = make_periods(rng, "minus", 70)
    assert minus[0] == minus[-1] == -1 and set(minus.tolist()) <= {-1, 0, 1, 2} and minus.max() == 2 and (minus[2:-2] == -1).any()


@functools.lru_cache(maxsize=None)
def _order_case():
    """gen: every column starts with -1e30 and goes on with multiples of 0.125 in 0..50.  obs: log-normal with sigma = 6, half the
    days zero.  No NaN, no mask: every window exists from day K - 1 on."""
    rng = np.random.default_rng(66)
    N, shape = 40, SHAPES[1]
    gen = (rng.integers(0, 401, size=(N, *shape)) * 0.125).astype(f32)
    gen[0] = f32(-1e30)
    obs = np.exp(6.0 * rng.standard_normal((N, *shape))).astype(f32)
    obs[rng.random(obs.shape) < 0.5] = 0.0
    return gen, obs


def test_the_window_sum_is_ordered_not_sliding():
    gen, obs = _order_case()
    windows = (2, 3, 5, 32)
    want = PR.period_indices(gen, obs, windows, [], WET)
    # what a cumulative-sum (sliding add and subtract) form gives instead, even in fp64: 0 or garbage after the -1e30 day
    c = np.concatenate([np.zeros((1, *gen.shape[1:])), np.cumsum(gen.astype(np.float64), axis=0)])
    for k, K in enumerate(windows):
        sliding = (c[K:] - c[:-K]).max(axis=0).astype(f32)
        assert (sliding != want["gen_rx"][k]).mean() > 0.9, K
    assert (obs == 0).mean() > 0.45 and obs.max() > 1e6 * np.median(obs[obs > 0])
    assert (want["gen_rx"][0] > 50).all() and (want["gen_rx"][0] <= 100).all()        # the -1e30 day spoils no later window
    got = device_call(gen, obs, windows, [])
    TC.bit_equal(got, want, "ordered sums")
    ids = np.arange(40) // 13
    TC.bit_equal(device_call(gen, obs, windows, [], ids=ids), PR.period_indices(gen, obs, windows, [], WET, None, None, ids), "per period")


def test_cross_checks_against_climate_indices():
    """device against device, on the same inputs: the valid days, Rx1day = the maximum, and the wet-day count"""
    for mask_index, links in ((0, "none"), (1, "random"), (2, "edges")):
        gen, obs, mask, dn, _, _, _ = _case(SHAPES[1], 70, (1, 5), 8, "3d", mask_index, links, None, 1)
        got = device_call(gen, obs, (1, 5), [WET], mask, dn)
        t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)   # noqa: E731
        clim = {k: v.cpu().numpy() for k, v in V.climate_indices(t(gen), t(obs), WET, mask=t(mask), day_numbers=dn).items()}
        np.testing.assert_array_equal(got["days"], clim["days"])
        for side in ("gen", "obs"):
            np.testing.assert_array_equal(got[f"{side}_rx"][0].view(np.int32), clim[f"{side}_max"].view(np.int32), err_msg=side)
            n_wet = np.round(clim[f"{side}_wet_freq"].astype(np.float64) * clim["days"])
            ok = clim["days"] > 0
            np.testing.assert_array_equal(got[f"{side}_count"][0][ok], n_wet[ok].astype(np.int32), err_msg=side)
            assert (got[f"{side}_count"][0][~ok] == 0).all() and ok.any() and (~ok).any()


def test_two_calls_and_a_contiguous_copy_are_bit_equal():
    gen, obs, mask, dn, ids, thr, want = _case(SHAPES[1], 70, (1, 5), 8, "m3", 1, "random", "runs", 1)
    args = (gen, obs, (1, 5), thr, mask, dn, ids)
    strided = device_call(*args, permuted=True)
    TC.bit_equal(strided, want, "strided view")
    TC.bit_equal(device_call(*args, permuted=True), strided, "twice")
    TC.bit_equal(device_call(*args), strided, "contiguous copy")
    # M = 1 as a 4-D tensor is the 3-D call with a member axis
    one = device_call(gen[:1], obs, (1, 5), thr, mask, dn, ids)
    flat = device_call(gen[0], obs, (1, 5), thr, mask, dn, ids)
    assert one["gen_rx"].shape == (1, 2, *SHAPES[1]) and flat["gen_rx"].shape == (2, *SHAPES[1])
    TC.bit_equal({k: (v[0] if "gen" in k else v) for k, v in one.items()}, flat, "M = 1")
    # a period of id -1 only is no period at all
    none = device_call(gen, obs, (1, 5), thr, mask, dn, np.full(70, -1))
    TC.bit_equal(none, {k: v for k, v in strided.items() if "period" not in k}, "all days outside every period")
