"""sbgm_conv2d_wgrad_plan / sbgm_wgrad_flush_plan without a device: the case table of conv_wgrad_ref.py reaches every kernel body, store
path and tile edge of the weight-gradient launcher that test_gpu_conv_wgrad.py then runs against float64.  The queries report the
helpers the launcher and the flush themselves act on (csrc/conv_wgrad.hip: sbgm_wgrad_plan, sbgm_wgrad_flush_rows)."""
import ctypes as C
import json
import pathlib
import re

import pytest

import conv_wgrad_ref as R
from sbgm_danra_amd import _native as N

ROOT = pathlib.Path(__file__).resolve().parents[1]


def raw_plan(geom):
    """the eight integers of sbgm_conv2d_wgrad_plan, or None where the launcher refuses the call"""
    B, Cin, H, W, Cout, k, s, p, cs = R.full(geom)
    out = (C.c_int * 8)(*([-7] * 8))
    if N.lib().sbgm_conv2d_wgrad_plan(B, H, W, cs, Cin, Cout, k, k, s, p, out):
        return None
    return list(out)


def plan(geom):
    """dict of the immediate plan, or None where the launcher refuses the call"""
    out = raw_plan(geom)
    if out is None:
        return None
    fam, gx, gy, tpw, n_tiles, direct, M, zero = out
    assert M == R.pixels(geom) and zero == 0 and direct in (0, 1) and gx >= 1 and gy >= 1 and tpw >= 1
    return dict(family=fam, gx=gx, gy=gy, tpw=tpw, n_tiles=n_tiles, direct=bool(direct))


def ragged_multi(pl):
    """several tiles per workgroup, and the last workgroup has fewer of them"""
    return pl["tpw"] > 1 and pl["gy"] > 1 and pl["n_tiles"] % pl["tpw"] != 0


def test_abi_version_and_symbols():
    lib = N.lib()
    assert lib.sbgm_abi_version() == N.ABI_VERSION >= 13
    header = (ROOT / "include" / "sbgm_hip.h").read_text()
    for name in ("sbgm_conv2d_wgrad_plan", "sbgm_wgrad_flush_plan"):
        assert name in N.SIGNATURES and hasattr(lib, name) and re.search(rf"\bint {name}\(", header)
    m = re.search(r"enum \{ SBGM_WGRAD_GENERAL1 = 0, SBGM_WGRAD_GENERAL2 = 1, SBGM_WGRAD_GENERAL4 = 2, SBGM_WGRAD_HALO16 = 3, SBGM_WGRAD_HALO8 = 4,\s*"
                  r"SBGM_WGRAD_TAP64 = 5, SBGM_WGRAD_TAP128 = 6, SBGM_WGRAD_STEM = 7 \}", header)
    assert m and (R.GENERAL1, R.GENERAL2, R.GENERAL4, R.HALO16, R.HALO8, R.TAP64, R.TAP128, R.STEM) == tuple(range(8))


@pytest.mark.parametrize("geom,family,want", R.CASES, ids=[R.label(g) for g, _, _ in R.CASES])
def test_every_row_gets_the_plan_its_comment_claims(geom, family, want):
    pl = plan(geom)
    assert pl is not None, N.lib().sbgm_last_error()
    assert pl["family"] == family, (R.FAMILY_NAMES[pl["family"]], R.FAMILY_NAMES[family])
    if "direct" in want:
        assert pl["direct"] == want["direct"], pl
    if want.get("multi"):
        assert ragged_multi(pl), pl
    for key, v in want.get("plan", {}).items():
        assert pl[key] == v, (key, pl)
    if family in R.GENERAL:                                   # gy splits of tpw pixels cover the M pixels, in multiples of 4
        assert not pl["direct"] and pl["n_tiles"] == R.pixels(geom) and pl["tpw"] % 4 == 0
        assert (pl["gy"] - 1) * pl["tpw"] < pl["n_tiles"] <= pl["gy"] * pl["tpw"]
    else:                                                     # gy workgroups of tpw tiles cover the n_tiles tiles, none idle
        assert (pl["gy"] - 1) * pl["tpw"] < pl["n_tiles"] <= pl["gy"] * pl["tpw"]
        assert pl["direct"] == (pl["gy"] == 1 and family != R.STEM)
    B, Cin, H, W, Cout, k, s, p, cs = R.full(geom)
    if family == R.HALO16:
        assert pl["n_tiles"] == B * (H // 16) * (W // 16) and pl["gx"] == (Cout // 32) * (cs // 32)
    elif family == R.HALO8:
        assert pl["n_tiles"] == (B + 3) // 4 and pl["gx"] == (Cout // 32) * (cs // 32)
    elif family in R.TILE_PX:
        assert pl["n_tiles"] == -(-R.pixels(geom) // R.TILE_PX[family])


def test_the_table_reaches_every_family_and_edge():
    rows = [(R.full(g), fam, plan(g)) for g, fam, _ in R.CASES]
    fams = {fam for _, fam, _ in rows}
    assert fams == {R.GENERAL1, R.GENERAL2, R.HALO16, R.HALO8, R.TAP64, R.TAP128, R.STEM}         # general<4>: see the test below
    for fam in (R.HALO16, R.HALO8, R.TAP64, R.TAP128):
        assert {pl["direct"] for _, f, pl in rows if f == fam} == {False, True}, R.FAMILY_NAMES[fam]
    for fam in (R.HALO16, R.TAP64, R.TAP128):
        assert any(ragged_multi(pl) for _, f, pl in rows if f == fam), R.FAMILY_NAMES[fam]
    for fam in (R.TAP64, R.TAP128):
        assert any(R.pixels(g) % R.TILE_PX[fam] for g, f, _ in rows if f == fam), R.FAMILY_NAMES[fam]
    halo8 = [g[0] for g, f, _ in rows if f == R.HALO8]
    assert {b % 4 for b in halo8} >= {1, 2} and min(halo8) < 4 and any(pl["tpw"] > 1 for _, f, pl in rows if f == R.HALO8)
    padded = {("halo" if f in (R.HALO16, R.HALO8) else "tap" if f in (R.TAP64, R.TAP128) else "stem" if f == R.STEM else "general")
              for g, f, _ in rows if g[8] > g[1]}
    assert padded == {"halo", "tap", "stem", "general"}
    # the linear shape that also runs with the gradient tensor as its slab
    assert any(g[5] == 1 and g[8] == g[1] and f == R.TAP64 and not pl["direct"] for g, f, pl in rows)


def test_one_hot_geometries_get_their_families():
    for geom, fam in R.ONE_HOT_CASES:
        assert plan(geom)["family"] == fam, geom
        oh, ow = R.out_hw(geom)
        assert oh >= 8 and ow >= 8 and R.pixels(geom) <= 2048
    assert {fam for _, fam in R.ONE_HOT_CASES} >= {R.HALO16, R.HALO8, R.TAP64, R.TAP128, R.STEM, R.GENERAL2}
    assert any(g[0] == 5 and f == R.HALO8 for g, f in R.ONE_HOT_CASES) and any(g[2] == 32 and f == R.HALO16 for g, f in R.ONE_HOT_CASES)


def test_without_the_lds_bodies_every_case_is_a_general_kernel(monkeypatch):
    monkeypatch.setenv("SBGM_NO_LDS_WGRAD", "1")                          # read by the launcher's helper on every call
    want = {4: R.GENERAL1, 8: R.GENERAL1, 16: R.GENERAL1, 48: R.GENERAL1, 32: R.GENERAL2, 96: R.GENERAL2}
    for geom, _, _ in R.CASES:
        pl, cs = plan(geom), R.full(geom)[8]
        assert pl["family"] == want.get(cs, R.GENERAL4 if cs % 64 == 0 else None), (geom, pl)
        assert not pl["direct"] and pl["n_tiles"] == R.pixels(geom)
    for geom in R.GENERAL4_CASES:
        assert plan(geom)["family"] == R.GENERAL4
    monkeypatch.delenv("SBGM_NO_LDS_WGRAD")
    assert all(plan(g)["family"] not in R.GENERAL for g in R.GENERAL4_CASES)


def test_refused_calls():
    lib = N.lib()
    for geom in R.REFUSED:
        assert plan(geom) is None and b"wgrad" in lib.sbgm_last_error()
    assert lib.sbgm_conv2d_wgrad_plan(1, 16, 16, 32, 32, 64, 3, 3, 1, 1, None) != 0
    # the gradient tensor as the slab of a 3x3 kernel: refused on the host, before anything is launched or dereferenced
    B, Cin, H, W, Cout, k, s, p, cs = R.full(R.ALIAS_REFUSED)
    assert plan(R.ALIAS_REFUSED)["family"] == R.TAP64
    assert lib.sbgm_conv2d_wgrad(4096, 4096, 8192, 8192, B, H, W, cs, Cin, Cout, k, k, s, p, None) != 0
    assert b"alias" in lib.sbgm_last_error()


def test_every_plan_equals_the_one_recorded_before_the_launcher_moved(monkeypatch):
    """tests/golden/wgrad_plans_parent.json (tools/record_wgrad_plans.py) holds the eight integers the planner gave, at the commit named in
    the file, for every geometry of the case tables and of tools/bench_wgrad.py; a refused geometry is recorded as null.  Exact equality."""
    golden = json.loads((ROOT / "tests" / "golden" / "wgrad_plans_parent.json").read_text())
    assert re.fullmatch(r"[0-9a-f]{40}", golden["parent"])
    recorded = set()
    for row in golden["plans"]:
        if row["no_lds"]:
            monkeypatch.setenv("SBGM_NO_LDS_WGRAD", "1")
        else:
            monkeypatch.delenv("SBGM_NO_LDS_WGRAD", raising=False)
        assert raw_plan(tuple(row["geom"])) == row["plan"], row
        recorded.add((row["source"], tuple(row["geom"]), row["no_lds"], row["plan"] is None))
    monkeypatch.delenv("SBGM_NO_LDS_WGRAD", raising=False)
    want = {("CASES", R.full(g), False, False) for g, _, _ in R.CASES} | {("ONE_HOT_CASES", R.full(g), False, False) for g, _ in R.ONE_HOT_CASES}
    want |= {("REFUSED", R.full(g), False, True) for g in R.REFUSED} | {("GENERAL4_CASES", R.full(g), e, False) for g in R.GENERAL4_CASES for e in (False, True)}
    assert want <= recorded, want - recorded
    assert sum(1 for r in recorded if r[0].startswith("bench_wgrad.")) == 21


def test_flush_plan_of_an_empty_queue_and_its_cap():
    lib = N.lib()
    assert lib.sbgm_wgrad_flush_pending() == 0
    assert lib.sbgm_wgrad_flush_plan(None, 0) == 0
    buf = (C.c_int * (2 + 7 * 4))(*([-7] * 30))
    assert lib.sbgm_wgrad_flush_plan(buf, 4) == 0
    assert list(buf[:2]) == [0, 0] and all(v == -7 for v in buf[2:])      # header only: no rows, nothing past them
    assert lib.sbgm_wgrad_flush_plan(buf, 0) == 0 and all(v == -7 for v in buf[2:])
