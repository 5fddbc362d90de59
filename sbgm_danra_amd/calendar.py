"""Dates of a series on the host (numpy only): day numbers, links between adjacent days and group ids from the calendar.
A day number is an int64 count of days since 1970-01-01 (numpy's datetime64[D] epoch).  The resident fields carry one per item
(`dates`), the series generation keys its noise rows by them, and the climate indices and the pooled series scores take links
and groups derived from them."""
from __future__ import annotations

import datetime

import numpy as np

SEASONS = ("DJF", "MAM", "JJA", "SON")
MONTHS = ("Jan", "Feb", "Mar", "Apr", "May", "Jun", "Jul", "Aug", "Sep", "Oct", "Nov", "Dec")
GROUPINGS = ("season", "month")
PERIODS = ("year", "season_year", "month_year")
MAX_PERIODS = 256                                 # include/sbgm_hip.h: SBGM_PERIOD_MAX_PERIODS


def day_numbers(dates):
    """1-D integer or datetime64[D] array -> int64 days since 1970-01-01, strictly increasing (ValueError otherwise)"""
    a = np.asarray(dates)
    if a.ndim != 1:
        raise ValueError(f"dates: expected a 1-D array, got shape {a.shape}")
    if a.dtype.kind == "M":
        if np.isnat(a).any():
            raise ValueError("dates: NaT is no date")
        dn = a.astype("datetime64[D]").astype(np.int64)
    elif a.dtype.kind in "iu":
        dn = a.astype(np.int64)
    else:
        raise ValueError(f"dates: expected integer day numbers or datetime64[D], got dtype {a.dtype}")
    if dn.size > 1 and not (np.diff(dn) > 0).all():
        raise ValueError("dates: the day numbers must be strictly increasing")
    return dn


def civil(dn):
    """(year, month, day) int64 arrays of day numbers"""
    d = np.asarray(dn, np.int64).astype("datetime64[D]")
    y, m = d.astype("datetime64[Y]"), d.astype("datetime64[M]")
    return y.astype(np.int64) + 1970, (m - y).astype(np.int64) + 1, (d - m).astype(np.int64) + 1


def links(dn):
    """bool [N]: links[t] is True iff day t is the calendar day after day t - 1; links[0] is False"""
    dn = np.asarray(dn, np.int64)
    out = np.zeros(dn.shape, bool)
    out[1:] = dn[1:] == dn[:-1] + 1
    return out


def groups_from_dates(dn, by):
    """(ids int list, names list): by="season" DJF = 0, MAM = 1, JJA = 2, SON = 3; by="month" January = 0 .. December = 11"""
    if by not in GROUPINGS:
        raise ValueError(f"groups: expected one of {GROUPINGS}, got {by!r}")
    month = civil(dn)[1]
    if by == "season":
        return [int(g) for g in (month % 12) // 3], list(SEASONS)
    return [int(g) for g in month - 1], list(MONTHS)


def periods_from_dates(dn, by):
    """(ids int list, names list) of the periods of a record: by="year" ("2001"), "month_year" ("2001-03") or "season_year",
    which puts December with the following January and February and names the season by that year ("2002-DJF").  Ids count
    from 0 at the first period present, in time order; a period without a day gets no id.  More than 256 periods is a
    ValueError."""
    if by not in PERIODS:
        raise ValueError(f"periods: expected one of {PERIODS}, got {by!r}")
    year, month, _ = civil(dn)
    if by == "year":
        key = year
        name = lambda k: f"{k:04d}"                                                      # noqa: E731
    elif by == "month_year":
        key = year * 12 + (month - 1)
        name = lambda k: f"{k // 12:04d}-{k % 12 + 1:02d}"                               # noqa: E731
    else:
        key = (year + (month == 12)) * 4 + (month % 12) // 3
        name = lambda k: f"{k // 4:04d}-{SEASONS[k % 4]}"                                # noqa: E731
    present = np.unique(key)                                                            # sorted: time order
    if present.size > MAX_PERIODS:
        raise ValueError(f"periods: {by!r} gives {present.size} periods; at most {MAX_PERIODS}")
    return [int(g) for g in np.searchsorted(present, key)], [name(int(k)) for k in present]


def parse_origin(x):
    """an int day number, or "YYYY-MM-DD" -> int day number"""
    if isinstance(x, (bool, np.bool_)):
        raise ValueError(f"calendar_origin: expected an int day number or 'YYYY-MM-DD', got {x!r}")
    if isinstance(x, (int, np.integer)):
        return int(x)
    if isinstance(x, datetime.date) and not isinstance(x, datetime.datetime):      # YAML reads an unquoted YYYY-MM-DD as a date
        x = x.isoformat()
    if isinstance(x, str) and len(x) == 10 and x[4] == x[7] == "-":
        try:
            return int(np.datetime64(x, "D").astype(np.int64))
        except ValueError:
            pass
    raise ValueError(f"calendar_origin: expected an int day number or 'YYYY-MM-DD', got {x!r}")


def series_days(dates, origin):
    """the absolute days n_d = dates - origin of a series (int64 [D]); the dates served must be strictly increasing (a shuffled
    loader is refused) and none may lie before the origin"""
    dn = day_numbers(dates)
    n = dn - int(origin)
    if n.size and n[0] < 0:
        raise ValueError(f"calendar_origin {int(origin)} lies after the date {int(dn[0])}: the origin must be <= every date served")
    return n


def noise_rows(days, lags, members):
    """int64 [D * M]: member m of absolute day n is drawn as noise row (n + K - 1) M + m (K = lags, the number of weights); the
    largest row must fit int32"""
    n = np.asarray(days, np.int64)
    rows = ((n + int(lags) - 1) * int(members))[:, None] + np.arange(int(members), dtype=np.int64)[None]
    if rows.size and (n.min() < 0 or int(rows.max()) > 0x7FFFFFFF):
        raise ValueError(f"days {int(n.min())}..{int(n.max())} with {lags} weights and {members} members put a noise row outside "
                         f"0..2^31 - 1")
    return rows.reshape(-1)
