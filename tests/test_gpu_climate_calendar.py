"""GPU suite for the calendar-aware, grouped climate indices (verification.climate_indices with `day_numbers` and `groups`;
csrc/verify_temporal.hip, DESIGN.md §11 K61 and the slabs of K55 - K57) against the restatement by composition
tests/climate_calendar_ref.py.  Every output is asserted bit-equal to it, as test_gpu_climate.py asserts the plain call: the
kernels run the same IEEE fp64 operations in the same order as the plain call does on the days of a slab with an all-NaN day
inserted at every broken link.  The largest deviation per index is printed in fp32 ulps before it is asserted."""
import functools

import numpy as np
import pytest
import torch

import climate_calendar_ref as CR
import climate_ref as R
import test_gpu_climate as T
from sbgm_danra_amd import calendar as cal
from sbgm_danra_amd import verification as V

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SHAPES = [(37, 53), (32, 48)]
DAYS = [2, 3, 33, 65, 366]
LINKS = ["none", "all", "edges", "random"]
GROUPS = [None, "one", "runs16", "sparse"]
MASKS = [None, ("hw", "uint8"), ("nhw", "float32")]
QS, QWS, WET = T.QS, T.QWS, T.WET


def make_day_numbers(rng, kind, N):
    """day numbers whose broken links are: none; all; exactly at t = 32 and 64 (the edges of the validity words); random 10 %"""
    broken = np.zeros(N, bool)
    if kind == "all":
        broken[1:] = True
    elif kind == "edges":
        broken[[t for t in (32, 64) if t < N]] = True
    elif kind == "random":
        broken[1:] = rng.random(N - 1) < 0.1
        broken[N // 2] = True
    step = np.where(broken, rng.integers(2, 10, size=N), 1)
    step[0] = 0
    return 18262 + np.cumsum(step)


def make_groups(rng, kind, N):
    """one: G = 1.  runs16: 16 ids in runs of 1..6 days, so every group's membership is non-contiguous and has adjacent days.
    sparse: ids 0, 2 and 5 at random (1, 3 and 4 are used by no day) and id 7 on exactly one day."""
    if kind is None:
        return None
    if kind == "one":
        return np.zeros(N, np.int64)
    if kind == "runs16":
        ids = np.concatenate([np.full(rng.integers(1, 7), rng.integers(0, 16)) for _ in range(N)])[:N]
        ids[-1] = 15                                                         # G = 16 whatever was drawn
        return ids.astype(np.int64)
    ids = rng.choice([0, 2, 5], size=N)
    ids[N // 2] = 7
    return ids.astype(np.int64)


@functools.lru_cache(maxsize=None)
def _case(shape, N, links, groups, mask_index, seasons=False):
    rng = np.random.default_rng([SHAPES.index(shape), N, LINKS.index(links), GROUPS.index(groups), mask_index])
    gen, obs = T.make_series(rng, "rain" if N % 2 else "grid", N, shape)
    mask = T.make_mask(rng, MASKS[mask_index], N, shape)
    dn = make_day_numbers(rng, links, N)
    ids = np.asarray(cal.groups_from_dates(dn, "season")[0], np.int64) if seasons else make_groups(rng, groups, N)
    return gen, obs, mask, dn, ids, CR.climate_indices(gen, obs, WET, QS, QWS, mask, dn, ids)


def device_call(gen, obs, mask=None, day_numbers=None, groups=None, qs=QS, qws=QWS):
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)   # noqa: E731
    r = V.climate_indices(t(gen), t(obs), WET, qs, qws, mask=t(mask), day_numbers=day_numbers,
                          groups=None if groups is None else groups.tolist())
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


def bit_equal(a, b, tag):
    assert set(a) == set(b), tag
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, (tag, k)
        np.testing.assert_array_equal(np.ascontiguousarray(a[k]).view(np.int32), np.ascontiguousarray(b[k]).view(np.int32),
                                      err_msg=f"{tag} {k}")


CASES = [(SHAPES[(ni + li) % 2], N, links, GROUPS[(ni + li) % len(GROUPS)], (ni + 2 * li) % len(MASKS))
         for ni, N in enumerate(DAYS) for li, links in enumerate(LINKS)] + [(SHAPES[0], 1500, "random", "runs16", 1)]


@pytest.mark.parametrize("shape,N,links,groups,mask_index", CASES)
def test_against_the_restatement(shape, N, links, groups, mask_index):
    gen, obs, mask, dn, ids, want = _case(shape, N, links, groups, mask_index)
    T.assert_planted({k: v for k, v in want.items() if not k.startswith("group_")}, N)
    if groups is not None:
        assert want["group_days"].shape == (int(ids.max()) + 1, *shape)
    got = device_call(gen, obs, mask, dn, ids)
    T.assert_equal_to_reference(got, want, f"{shape} N={N} links={links} groups={groups} mask={MASKS[mask_index]}")


def test_the_cases_cover_every_pattern():
    assert {c[2] for c in CASES} == set(LINKS) and {c[3] for c in CASES} == set(GROUPS)
    assert {c[4] for c in CASES} == set(range(len(MASKS))) and {c[0] for c in CASES} == set(SHAPES)
    for N in DAYS:                                                           # every day count meets broken links and groups
        assert {c[2] for c in CASES if c[1] == N} == set(LINKS) and len({c[3] for c in CASES if c[1] == N}) == len(GROUPS)
    rng = np.random.default_rng(0)
    edges = np.flatnonzero(np.diff(make_day_numbers(rng, "edges", 366)) != 1) + 1
    assert edges.tolist() == [32, 64]
    sparse = make_groups(rng, "sparse", 65)
    assert set(sparse.tolist()) == {0, 2, 5, 7} and (sparse == 7).sum() == 1
    runs = make_groups(rng, "runs16", 366)
    assert runs.max() == 15 and all((np.diff(np.flatnonzero(runs == g)) > 1).any() for g in range(15))     # non-contiguous


@pytest.mark.parametrize("mask_index", range(len(MASKS)))
def test_unbroken_calendar_is_the_plain_call(mask_index):
    """consecutive day numbers and one group of all days change nothing: the record's maps and the group's are the plain ones"""
    gen, obs, mask, dn, ids, want = _case(SHAPES[0], 65, "none", "one", mask_index)
    assert (np.diff(dn) == 1).all() and (ids == 0).all()
    plain = device_call(gen, obs, mask)
    T.assert_equal_to_reference(plain, R.climate_indices(gen, obs, WET, QS, QWS, mask), "plain")
    got = device_call(gen, obs, mask, dn, ids)
    bit_equal({k: v for k, v in got.items() if not k.startswith("group_")}, plain, "record")
    bit_equal({k[len("group_"):]: v[0] for k, v in got.items() if k.startswith("group_")}, plain, "the one group")
    bit_equal(device_call(gen, obs, mask, dn), plain, "day numbers alone")
    bit_equal(device_call(gen, obs, mask, None, ids), got, "groups alone")


def test_seasons_of_two_real_years():
    """2020-01-01 .. 2021-12-31: 731 days with a leap day, seasons from the calendar, a held-out month and a missing week"""
    N = 731
    rng = np.random.default_rng(2020)
    dates = np.datetime64("2020-01-01") + np.arange(N + 38)
    keep = np.ones(N + 38, bool)
    keep[(dates >= np.datetime64("2020-07-01")) & (dates <= np.datetime64("2020-07-31"))] = False
    keep[(dates >= np.datetime64("2021-02-10")) & (dates <= np.datetime64("2021-02-16"))] = False
    dn = cal.day_numbers(dates[keep])
    assert dn.shape == (N,) and np.datetime64("2020-02-29") in dates[keep] and (~cal.links(dn)).sum() == 3
    ids, names = cal.groups_from_dates(dn, "season")
    ids = np.asarray(ids, np.int64)
    assert names == ["DJF", "MAM", "JJA", "SON"] and set(ids.tolist()) == {0, 1, 2, 3}
    gen, obs = T.make_series(rng, "rain", N, SHAPES[1])
    mask = T.make_mask(rng, MASKS[1], N, SHAPES[1])
    want = CR.climate_indices(gen, obs, WET, QS, QWS, mask, dn, ids)
    got = device_call(gen, obs, mask, dn, ids)
    T.assert_equal_to_reference(got, want, "seasons 2020-2021")
    np.testing.assert_array_equal(got["group_days"].sum(axis=0), got["days"])
    for s in ("gen", "obs"):                                                  # a season loses the pairs across its ends, and only those
        assert (got[f"group_{s}_transitions"].sum(axis=(0, 1)) <= got[f"{s}_transitions"].sum(axis=0)).all()
        assert (got[f"group_{s}_cwd"].max(axis=0) <= got[f"{s}_cwd"]).all()


def test_the_calendar_call_is_the_plain_call_on_the_expanded_record():
    """device against device: a broken link is one invalid day, a group is its subsequence"""
    gen, obs, mask, dn, ids, _ = _case(SHAPES[0], 65, "random", "sparse", 2)
    got = device_call(gen, obs, mask, dn, ids)
    a, b, m = CR.expand(gen, obs, mask, dn, np.arange(65))
    assert a.shape[0] > 65
    bit_equal({k: v for k, v in got.items() if not k.startswith("group_")}, device_call(a, b, m), "record")
    for g in range(int(ids.max()) + 1):
        a, b, m = CR.expand(gen, obs, mask, dn, np.flatnonzero(ids == g))
        if a.shape[0] < 2:                                                   # the plain call needs two days: one more hole changes nothing
            hole = np.full_like(a[:1], np.nan)
            a, b, m = np.concatenate([a, hole]), np.concatenate([b, hole]), np.concatenate([m, m[:1]])
        plain = device_call(a, b, m)
        bit_equal({k[len("group_"):]: v[g] for k, v in got.items() if k.startswith("group_")}, plain, f"group {g}")


def test_the_calendar_and_the_groups_matter():
    """the guard against a vacuous pass, on the random case: the calendar shortens spells and removes transitions somewhere,
    and every used group has a pixel with at least one pair"""
    gen, obs, mask, dn, ids, want = _case(SHAPES[1], 366, "random", "runs16", 0)
    assert (gen.shape[0], LINKS[3], GROUPS[2]) == (366, "random", "runs16")
    got = device_call(gen, obs, mask, dn, ids)
    T.assert_equal_to_reference(got, want, "random case")
    plain = device_call(gen, obs, mask)
    for s in ("gen", "obs"):
        assert (got[f"{s}_cwd"] < plain[f"{s}_cwd"]).any() and (got[f"{s}_cwd"] <= plain[f"{s}_cwd"]).all()
        assert (got[f"{s}_transitions"].sum(axis=0) < plain[f"{s}_transitions"].sum(axis=0)).any()
        for k in ("mean", "wet_freq", "sdii", "max", "quantiles", "wet_quantiles", "heavy_fraction"):      # a link counts nowhere else
            np.testing.assert_array_equal(got[f"{s}_{k}"].view(np.int32), plain[f"{s}_{k}"].view(np.int32), err_msg=k)
    np.testing.assert_array_equal(got["days"], plain["days"])
    used = sorted(set(ids.tolist()))
    assert len(used) == 16
    for g in used:
        assert (got["group_gen_transitions"][g].sum(axis=0) > 0).any(), g
    nolinks = device_call(gen, obs, mask, None, ids)                         # the links reach the groups too
    assert (got["group_obs_transitions"].sum(axis=1) < nolinks["group_obs_transitions"].sum(axis=1)).any()


def test_two_calls_are_bit_equal_and_level_counts():
    gen, obs, mask, dn, ids, _ = _case(SHAPES[0], 65, "random", "sparse", 2)
    bit_equal(device_call(gen, obs, mask, dn, ids), device_call(gen, obs, mask, dn, ids), "twice")
    for qs, qws in (([], [0.95]), ([0.5], []), ([], [])):
        got = device_call(gen, obs, mask, dn, ids, qs=qs, qws=qws)
        assert got["group_gen_quantiles"].shape == (8, len(qs), 37, 53) and got["group_obs_heavy_fraction"].shape == (8, len(qws), 37, 53)
        T.assert_equal_to_reference(got, CR.climate_indices(gen, obs, WET, qs, qws, mask, dn, ids), f"Q={len(qs)} QW={len(qws)}")
