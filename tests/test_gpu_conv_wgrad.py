"""The weight-gradient launcher, kernel body by kernel body and launch form by launch form, against float64 (tests/conv_wgrad_ref.py).

sbgm_conv2d_wgrad[_bias] picks one of five kernel bodies, a pixel split and a store path by arithmetic inside the launcher, and under
sbgm_wgrad_defer(3) by what else is queued at the flush.  sbgm_conv2d_wgrad_plan / sbgm_wgrad_flush_plan report those choices (the
helpers the launcher acts on), so every run here first asserts WHICH body and split it is about to run, then holds the result to

    |dW - ref64| <= (M + 2) * 2^-24 * abs64        |db - db64| <= (M + 1) * 2^-24 * absdb64        elementwise, no NaN or Inf

(any-order fp32 summation bound, M = B*OH*OW <= 2048; conv_wgrad_ref.py derives it).  x, dy, dW, db and the slab sit inside NaN-poisoned
allocations; outputs and slab are NaN-filled before every run, so a read past a tensor, a slab element left unzeroed or a store past dW
shows.  Every test prints `WGRAD-WORST <geometry> <family> <mode>: <max err/bound>` (DESIGN.md 3.4 records them); a failure names
geometry, family, mode, the tap (kh, kw) and the worst (co, ci).

The defer mask, the prezeroed switch and the queue are process-wide: every test restores them and discards the queue in a `finally`."""
import contextlib
import ctypes as C
import json
import pathlib

import pytest
import torch

import conv_wgrad_ref as R
from attention_ref import Poisoned
from sbgm_danra_amd import _native as N

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
MODES = ["immediate", "prezeroed", "unpack-deferred", "gemm-deferred"]
QUEUED = (R.HALO16, R.HALO8, R.TAP64, R.TAP128, R.STEM)           # the families sbgm_wgrad_defer bit 1 queues
GOLDEN = json.loads((pathlib.Path(__file__).parent / "golden" / "wgrad_plans_parent.json").read_text())


def lib():
    return N.lib()


@contextlib.contextmanager
def switches(defer, prezeroed):
    """the process-wide defer mask and prezeroed switch for one run; both restored and the queue dropped whatever happens"""
    assert lib().sbgm_wgrad_flush_pending() == 0
    prev_d, prev_z = lib().sbgm_wgrad_defer(defer), lib().sbgm_set_scratch_prezeroed(prezeroed)
    try:
        yield
    finally:
        lib().sbgm_wgrad_defer(prev_d)
        lib().sbgm_set_scratch_prezeroed(prev_z)
        lib().sbgm_wgrad_discard()


def immediate_plan(geom):
    B, Cin, H, W, Cout, k, s, p, cs = R.full(geom)
    out = (C.c_int * 8)()
    assert lib().sbgm_conv2d_wgrad_plan(B, H, W, cs, Cin, Cout, k, k, s, p, out) == 0, lib().sbgm_last_error()
    return dict(zip(("family", "gx", "gy", "tpw", "n_tiles", "direct"), out[:6]))


def flush_plan(cap=256):
    """(rows as dicts, layout passes, layout launches) of what is queued now; the query must stay inside cap rows"""
    n = lib().sbgm_wgrad_flush_plan(None, 0)
    buf = (C.c_int * (2 + 7 * (cap + 1)))(*([-7] * (2 + 7 * (cap + 1))))
    assert lib().sbgm_wgrad_flush_plan(buf, cap) == n
    assert all(v == -7 for v in buf[2 + 7 * min(n, cap):]), "sbgm_wgrad_flush_plan wrote past its cap"
    keys = ("family", "launch", "gx", "gy", "tpw", "n_tiles", "direct")
    return [dict(zip(keys, buf[2 + 7 * i:9 + 7 * i])) for i in range(min(n, cap))], buf[0], buf[1]


def flush_record(rows, passes, launches):
    return dict(rows=[[r[k] for k in ("family", "launch", "gx", "gy", "tpw", "n_tiles", "direct")] for r in rows], passes=passes, launches=launches)


def check_against_parent(name, rows, passes, launches):
    """exactly the flush plan this queue got at the commit named in tests/golden/wgrad_plans_parent.json (tools/record_wgrad_plans.py)"""
    assert flush_record(rows, passes, launches) == GOLDEN["flush"][name], name


def ragged_multi(row):
    return row["tpw"] > 1 and row["gy"] > 1 and row["n_tiles"] % row["tpw"] != 0


class Call:
    """one weight-gradient call: every operand inside its own NaN-poisoned allocation; `aliased`: the gradient tensor is the slab"""

    def __init__(self, geom, c, bias, aliased=False):
        B, Cin, H, W, Cout, k, s, p, cs = self.g = R.full(geom)
        self.geom, self.c, self.bias, self.aliased = geom, c, bias, aliased
        self.x, self.dy = Poisoned(tuple(c["x"].shape), DEV, c["x"]), Poisoned(tuple(c["dy"].shape), DEV, c["dy"])
        self.dw, self.db, self.ws = Poisoned((Cout, Cin, k, k), DEV), Poisoned((Cout,), DEV), Poisoned((k * k * Cout * cs,), DEV)
        self.ref, self.refdb = c["ref"].to(DEV), c["db"].to(DEV)
        self.bound, self.bounddb = (b.to(DEV) for b in R.bounds(c))
        assert not aliased or (k == 1 and cs == Cin and cs % 64 == 0)

    def fill(self, zeroed):
        """NaN everywhere the launcher must write or zero itself; `zeroed`: what the prezeroed switch promises arrives zeroed"""
        self.dw.t.fill_(0.0 if zeroed and self.aliased else NAN)
        self.db.t.fill_(0.0 if zeroed else NAN)
        self.ws.t.fill_(0.0 if zeroed else NAN)

    def launch(self):
        B, Cin, H, W, Cout, k, s, p, cs = self.g
        ws = self.dw.ptr() if self.aliased else self.ws.ptr()
        if self.bias:
            N.check(lib().sbgm_conv2d_wgrad_bias(self.dy.ptr(), self.x.ptr(), self.dw.ptr(), self.db.ptr(), ws, B, H, W, cs, Cin, Cout, k, k, s, p,
                                                 N.stream()))
        else:
            N.check(lib().sbgm_conv2d_wgrad(self.dy.ptr(), self.x.ptr(), self.dw.ptr(), ws, B, H, W, cs, Cin, Cout, k, k, s, p, N.stream()))

    def check(self, what):
        """max err/bound over dW (and db); raises with the tap and the (co, ci) of the worst element"""
        assert all(a.surround_unchanged() for a in (self.x, self.dy, self.dw, self.db, self.ws)), f"{what}: a kernel wrote outside its tensors"
        assert torch.equal(self.x.t.cpu(), self.c["x"]) and torch.equal(self.dy.t.cpu(), self.c["dy"]), f"{what}: an input was written"
        r, (co, ci, kh, kw) = R.worst(R.ratio(self.dw.t, self.ref, self.bound))
        assert r <= 1.0, (f"{what}: |dW - ref64| = {r:.3g} x bound at tap ({kh}, {kw}), (co, ci) = ({co}, {ci}): got {float(self.dw.t[co, ci, kh, kw])!r}, "
                          f"ref64 {float(self.ref[co, ci, kh, kw])!r}")
        if self.bias:
            rb, (co,) = R.worst(R.ratio(self.db.t, self.refdb, self.bounddb))
            assert rb <= 1.0, f"{what}: |db - db64| = {rb:.3g} x bound at co = {co}: got {float(self.db.t[co])!r}, ref64 {float(self.refdb[co])!r}"
            r = max(r, rb)
        return r


def run_mode(call, mode, family, what):
    """one call in one launch form; asserts the planned family, what is queued, and that nothing stays queued"""
    pl = immediate_plan(call.geom)
    assert pl["family"] == family, (what, R.FAMILY_NAMES[pl["family"]])
    defer = {"immediate": 0, "prezeroed": 0, "unpack-deferred": 1, "gemm-deferred": 3}[mode]
    with switches(defer, 1 if mode == "prezeroed" else 0):
        call.fill(mode == "prezeroed")
        call.launch()
        rows, passes, launches = flush_plan()
        if mode == "gemm-deferred" and family in QUEUED:
            assert len(rows) == 1 and rows[0]["family"] == family and rows[0]["launch"] == 0 and rows[0]["n_tiles"] == pl["n_tiles"], (what, rows)
            unpack = family == R.STEM or not (rows[0]["direct"] or call.aliased)
            assert rows[0]["direct"] == (rows[0]["gy"] == 1 and family != R.STEM) and passes == int(unpack), (what, rows, passes)
            assert lib().sbgm_wgrad_flush_pending() == 1
        else:
            unpack = defer and not (pl["direct"] or (call.aliased and family in QUEUED and family != R.STEM))
            assert rows == [] and passes == int(bool(unpack)) == lib().sbgm_wgrad_flush_pending(), (what, passes)
        assert launches == (1 if passes else 0)
        if defer:
            N.check(lib().sbgm_wgrad_flush(N.stream()))
        assert lib().sbgm_wgrad_flush_pending() == 0
        if mode == "immediate" and pl["direct"] and not call.aliased:
            assert bool(torch.isnan(call.ws.t).all()), f"{what}: a direct store touched the slab"
        return call.check(what)


def sweep(geom, family, aliased=False):
    """every data set, with and without the fused bias gradient, in every launch form"""
    worst = dict.fromkeys(MODES, 0.0)
    for data in R.DATA_SETS:
        c = R.case(geom, data)
        for bias in (False, True):
            call = Call(geom, c, bias, aliased)
            for mode in MODES:
                what = f"{geom} {R.FAMILY_NAMES[family]} {mode} {data}{' bias' if bias else ''}{' ws == dw' if aliased else ''}"
                worst[mode] = max(worst[mode], run_mode(call, mode, family, what))
    for mode in MODES:
        print(f"WGRAD-WORST {R.label(geom)}{' ws==dw' if aliased else ''} {R.FAMILY_NAMES[family]} {mode}: {worst[mode]:.3f}")


@pytest.mark.parametrize("geom,family", [(g, f) for g, f, _ in R.CASES], ids=[R.label(g) for g, _, _ in R.CASES])
def test_every_case_in_every_launch_form_against_float64(geom, family):
    sweep(geom, family)


@pytest.mark.parametrize("geom", R.GENERAL4_CASES, ids=R.label)
def test_general4_without_the_lds_bodies(geom, monkeypatch):
    monkeypatch.setenv("SBGM_NO_LDS_WGRAD", "1")                # read by the launcher on every call
    sweep(geom, R.GENERAL4)


ALIASED = [(g, f) for g, f, _ in R.CASES if g[5] == 1 and R.full(g)[8] == g[1] and g[1] % 64 == 0]


@pytest.mark.parametrize("geom,family", ALIASED, ids=[R.label(g) for g, _ in ALIASED])
def test_linear_shapes_with_the_gradient_tensor_as_the_slab(geom, family):
    assert len(ALIASED) == 3 and family in (R.TAP64, R.TAP128)
    sweep(geom, family, aliased=True)


# ---- queues: the split of a GEMM deferred with others is decided at the flush -----------------------------------------------------------------
def flush_queue(name, entries, defer, expect, bias_every=2):
    """entries (geom, aliased) queued under `defer`, each call with its own tensors and data (seed = position, data sets alternate, every
    bias_every-th call with the fused bias); expect(rows, passes, launches) judges the flush plan before the flush; every gradient and
    bias gradient against float64"""
    calls = []
    with switches(defer, 0):
        for i, (geom, aliased) in enumerate(entries):
            call = Call(geom, R.case(geom, R.DATA_SETS[i % 2], seed=i), bias=i % bias_every == 0, aliased=aliased)
            call.fill(False)
            call.launch()
            calls.append(call)
        rows, passes, launches = flush_plan()
        check_against_parent(name, rows, passes, launches)
        expect(rows, passes, launches)
        N.check(lib().sbgm_wgrad_flush(N.stream()))
        assert lib().sbgm_wgrad_flush_pending() == 0
        worst = {}
        for i, call in enumerate(calls):
            fam = immediate_plan(call.geom)["family"]
            worst[fam] = max(worst.get(fam, 0.0), call.check(f"queue {name} entry {i} {call.geom} {R.FAMILY_NAMES[fam]}"))
    for fam, v in sorted(worst.items()):
        print(f"WGRAD-WORST queue:{name} {R.FAMILY_NAMES[fam]} {'gemm-deferred' if defer == 3 else 'unpack-deferred'}: {v:.3f}")
    return rows


def test_flush_splits_halo16_direct_next_to_split_and_ragged_workgroups():
    big = (5, 256, 16, 16, 256, 3, 1, 1)
    entries = [((1, 32, 16, 16, 64, 3, 1, 1), False), ((3, 64, 16, 32, 64, 3, 1, 1), False)] + [(big, False)] * 4

    def expect(rows, passes, launches):
        assert [r["family"] for r in rows] == [R.HALO16] * 6 and {r["launch"] for r in rows} == {0}
        assert rows[0]["direct"] == 1 and rows[1]["direct"] == 0 and rows[1]["gy"] > 1
        assert all(ragged_multi(r) and r["gx"] == 64 and r["n_tiles"] == 5 for r in rows[2:]), rows
        assert passes == 5 and launches == 1

    flush_queue("halo16", entries, 3, expect)


def test_flush_splits_halo8_ragged_workgroups_and_a_one_image_tile():
    def expect(rows, passes, launches):
        assert [r["family"] for r in rows] == [R.HALO8] * 4
        assert all(ragged_multi(r) and r["n_tiles"] == 5 for r in rows), rows

    flush_queue("halo8", [((17, 256, 8, 8, 256, 3, 1, 1), False)] * 4, 3, expect)


def test_flush_splits_tap64_ragged_workgroups_with_a_stem_and_a_direct_layer():
    big = (6, 512, 24, 24, 64, 3, 2, 1)
    entries = [(big, False)] * 2 + [((1, 5, 32, 32, 64, 8, 2, 3, 8), False), ((2, 50, 6, 6, 64, 1, 1, 0, 64), False)] + [(big, False)] * 2

    def expect(rows, passes, launches):
        assert [r["family"] for r in rows] == [R.TAP64, R.TAP64, R.STEM, R.TAP64, R.TAP64, R.TAP64] and {r["launch"] for r in rows} == {0}
        assert all(ragged_multi(rows[i]) and rows[i]["n_tiles"] == 7 for i in (0, 1, 4, 5)), rows
        assert rows[2]["direct"] == 0 and rows[3]["direct"] == 1 and passes == 5         # the stem always goes through its slab

    flush_queue("tap64+stem", entries, 3, expect)


def test_flush_splits_tap128_ragged_workgroups():
    def expect(rows, passes, launches):
        assert [r["family"] for r in rows] == [R.TAP128] * 4
        assert all(ragged_multi(r) and r["n_tiles"] == 9 for r in rows), rows

    flush_queue("tap128", [((36, 256, 4, 4, 256, 3, 1, 1), False)] * 4, 3, expect)


# ---- chunk boundaries: a flush with more layers of a family than one launch's table holds -----------------------------------------------------
def test_31_halo16_layers_ride_in_two_launches():
    def expect(rows, passes, launches):
        assert len(rows) == 31 and [r["launch"] for r in rows] == [0] * 30 + [1] and all(r["family"] == R.HALO16 for r in rows)
        assert flush_plan(cap=7)[0] == rows[:7]                # a short buffer gets the first rows and nothing past them

    flush_queue("31 x halo16", [((1, 32, 16, 16, 64, 3, 1, 1), False)] * 31, 3, expect, bias_every=1)


def test_29_per_tap_layers_ride_in_two_launches():
    linear, stem = (1, 64, 1, 130, 64, 1, 1, 0), (1, 5, 32, 32, 64, 8, 2, 3, 8)
    entries = [(stem, False) if i % 3 == 2 else (linear, i % 3 == 1) for i in range(29)]          # every third linear: ws == dw

    def expect(rows, passes, launches):
        assert len(rows) == 29 and [r["launch"] for r in rows] == [0] * 28 + [1]
        assert [r["family"] for r in rows] == [R.STEM if i % 3 == 2 else R.TAP64 for i in range(29)]
        want = sum(1 for i, r in enumerate(rows) if i % 3 == 2 or (i % 3 == 0 and not r["direct"]))
        assert passes == want and launches == 1

    flush_queue("29 x per-tap", entries, 3, expect, bias_every=1)


def test_50_deferred_layout_passes_ride_in_two_launches():
    def expect(rows, passes, launches):
        assert rows == [] and passes == 50 == lib().sbgm_wgrad_flush_pending() and launches == 2

    flush_queue("50 x unpack", [((2, 20, 16, 16, 64, 3, 1, 1, 32), False)] * 50, 1, expect, bias_every=1)


# ---- one-hot dy: bit for bit ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom,family", R.ONE_HOT_CASES, ids=[R.label(g) for g, _ in R.ONE_HOT_CASES])
def test_one_hot_dy_gathers_x_bit_for_bit(geom, family):
    """every dW element is one x value times a power of two, or zero: adding zeros is exact, so direct stores and atomics alike must
    reproduce the fp32 gather exactly, and db the one-hot values"""
    c = R.one_hot_case(geom)
    want, want_db = c["exact"].to(DEV), c["exact_db"].to(DEV)
    for bias in (False, True):
        call = Call(geom, c, bias)
        for mode in ("immediate", "gemm-deferred"):
            what = f"{geom} {R.FAMILY_NAMES[family]} {mode} one-hot{' bias' if bias else ''}"
            assert run_mode(call, mode, family, what) == 0.0
            bad = (call.dw.t != want).nonzero()
            assert torch.equal(call.dw.t, want), f"{what}: {len(bad)} elements differ, first (co, ci, kh, kw) = {tuple(bad[0].tolist())}"
            assert not bias or torch.equal(call.db.t, want_db), what
    print(f"WGRAD-WORST {R.label(geom)} {R.FAMILY_NAMES[family]} one-hot: 0.000 (bit for bit)")
