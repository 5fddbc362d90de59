"""sbgm_conv2d_tiles on the host (no device): the candidate list the tuner times for one sbgm_conv2d_fwd call, for forward calls and for
the data-gradient calls ConvFn.backward makes (conv_dgrad_ref.dgrad_call).  The GPU test runs every entry of these lists; here: what
may and what must be in them."""
import ctypes as C

import conv_dgrad_ref as R

SOME = 64                      # any non-NULL value: the function looks at no pointer's target
WS_FLOATS = 1 << 21
WINO_KINDS = {"1-D Winograd", "LDS-staged Winograd"}
W2D_KINDS = {"2-D Winograd F(2x2,3x3)", "persistent 2-D Winograd F(2x2,3x3)"}
S1_ONLY = WINO_KINDS | W2D_KINDS | {"LDS-staged direct"}


def lib():
    from sbgm_danra_amd import _native as N
    return N.lib()


def tiles(call, ws=True, ws_floats=WS_FLOATS, wino=None, w2d=None, winograd=0, cap=512):
    from sbgm_danra_amd import _native as N
    wino = call["wino"] if wino is None else wino
    w2d = call["w2d"] if w2d is None else w2d
    a = N.ConvArgs(SOME, SOME, SOME, None, None, None, None, call["B"], call["H"], call["W"], call["c_pad"], call["Cout"], call["k"], call["k"],
                   call["stride"], call["pad"], N.NONE, 0, 0, 0, 0, 0, winograd, call["in_dil"], call["out_h"], call["out_w"],
                   SOME if ws else None, ws_floats if ws else 0, 0, None, None, 0, SOME if wino else None, SOME if w2d else None)
    buf = (C.c_int * (6 * max(cap, 1)))(*([-7] * (6 * max(cap, 1))))
    n = lib().sbgm_conv2d_tiles(C.byref(a), buf, cap)
    flat = list(buf)
    assert all(v == -7 for v in flat[6 * min(n, cap):]), "wrote past the entries it reported"
    return n, [tuple(flat[6 * i:6 * i + 6]) for i in range(min(n, cap))]


def forward_call(B, Cin, H, W, Cout, k, s, p, wino=False, w2d=False):
    return dict(B=B, H=H, W=W, c_pad=Cin, Cout=Cout, k=k, stride=s, pad=p, in_dil=0, out_h=0, out_w=0, wino=wino, w2d=w2d)


def out_pixels(call):
    oh = call["out_h"] or (call["H"] + 2 * call["pad"] - call["k"]) // call["stride"] + 1
    ow = call["out_w"] or (call["W"] + 2 * call["pad"] - call["k"]) // call["stride"] + 1
    return call["B"] * oh * ow


B_, Cin_, H_, W_, Cout_, k_, s_, p_ = R.PHASE_CASE
PHASE_CALL = forward_call(B_, Cout_, H_ // 2, W_ // 2, 4 * Cin_, 5, 1, 2)         # ConvFn.backward: 5x5 / s1 / p2 over dy to 4 Cin phases
CALLS = [R.dgrad_call(g) for g in R.CASES + R.LOCALISED_CASES] + [PHASE_CALL, forward_call(2, 64, 16, 16, 64, 3, 1, 1, True, True),
                                                                  forward_call(2, 64, 8, 8, 128, 3, 2, 1), forward_call(1, 256, 1, 24, 768, 1, 1, 0)]


def test_abi_version_and_symbol():
    from sbgm_danra_amd import _native as N
    assert lib().sbgm_abi_version() == N.ABI_VERSION >= 12 and "sbgm_conv2d_tiles" in N.SIGNATURES


def test_entries_are_well_formed_for_every_call():
    """every entry divides Cout, names a family, no entry twice; split-K entries only with a workspace and only those it can hold;
    the list without a workspace is the list with one, minus its split-K entries, in the same order"""
    for call in CALLS:
        n, got = tiles(call)
        assert n == len(got) > 0, call
        assert len(set(got)) == len(got), call
        for t in got:
            assert t[0] in (1, 2, 4) and call["Cout"] % (16 * t[0]) == 0 and t[1] in (1, 2, 4) and t[2] >= 1 and t[3] in (1, 2, 4, 8), (call, t)
            assert R.family(t) and (t[2] == 1 or R.family(t) == "implicit-GEMM"), (call, t)
            assert t[2] * out_pixels(call) * call["Cout"] <= WS_FLOATS, (call, t)
        assert any(t[2] > 1 for t in got), call
        n0, plain = tiles(call, ws=False)
        assert all(t[2] == 1 for t in plain) and plain == [t for t in got if t[2] == 1], call
        # a workspace that holds two splits' partial sums, not four
        small = 2 * out_pixels(call) * call["Cout"] + 1
        assert tiles(call, ws_floats=small)[1] == [t for t in got if t[2] <= 2], call


def test_dilated_calls_and_missing_images_bring_no_stride_1_family():
    """in_dil = 2 (stride-2 data gradient): implicit GEMM only, whatever images are offered; a NULL w_wino takes the F(2,3) families
    away, a NULL w_wino2d the F(2x2,3x3) ones, and the LDS-staged direct kernel (implicit-GEMM image) stays"""
    dilated = [R.dgrad_call(g) for g in R.CASES + R.LOCALISED_CASES if g[6] == 2]
    assert len(dilated) >= 5
    for call in dilated:
        assert call["in_dil"] == 2 and not call["wino"] and not call["w2d"]
        for offered in (False, True):
            fams = {R.family(t) for t in tiles(call, wino=offered, w2d=offered)[1]}
            assert fams == {"implicit-GEMM"}, (call, fams)
    call = R.dgrad_call(R.CASES[0])
    fams = lambda **kw: {R.family(t) for t in tiles(call, **kw)[1]}  # noqa: E731
    assert fams(wino=False, w2d=False) == {"implicit-GEMM", "LDS-staged direct"}
    assert fams(wino=True, w2d=False) == {"implicit-GEMM", "LDS-staged direct"} | WINO_KINDS
    assert fams(wino=False, w2d=True) == {"implicit-GEMM", "LDS-staged direct"} | W2D_KINDS


def test_stride_1_data_gradient_with_all_images_brings_every_family():
    """3x3 / s1 / p1 with out_h == H, W % 16 == 0 and all three images: the Winograd, LDS and F(2x2,3x3) families take part, and the
    data-gradient call (explicit output size) has the forward call's list"""
    for geom in R.CASES[:3] + R.LOCALISED_CASES[:1]:
        call = R.dgrad_call(geom)
        assert call["wino"] and call["w2d"] and call["out_h"] == call["H"] and call["W"] % 16 == 0
        n, got = tiles(call)
        assert {R.family(t) for t in got} == {"implicit-GEMM"} | S1_ONLY, geom
        for kind in ((1, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 1), (2, 2), (2, 3)):      # each (Winograd kind, LDS kind) at least once
            assert any((t[4], t[5]) == kind for t in got), (geom, kind)
        assert got == tiles(dict(call, out_h=0, out_w=0))[1], geom
    # an odd width takes the LDS families and F(2x2,3x3) away, an odd output size that differs from the input's everything but the GEMM
    assert {R.family(t) for t in tiles(forward_call(1, 64, 8, 24, 64, 3, 1, 1, True, True))[1]} == {"implicit-GEMM", "1-D Winograd"}
    assert {R.family(t) for t in tiles(dict(R.dgrad_call(R.CASES[0]), out_h=15, out_w=16))[1]} == {"implicit-GEMM"}


def test_cap_smaller_than_the_count():
    call = R.dgrad_call(R.CASES[0])
    n, full = tiles(call)
    assert n == len(full) > 100
    for cap in (0, 1, 7, n - 1):
        m, head = tiles(call, cap=cap)                     # tiles() checks that nothing past 6 * cap ints was written
        assert m == n and head == full[:cap]


def test_refused_calls_have_no_candidates():
    """the tuner's checks: winograd must be 0, Cout a multiple of 32 -- which is why a layer of 16 input channels has no data-gradient
    call on this path (ConvFn.backward raises for it)"""
    call = R.dgrad_call(R.CASES[0])
    assert tiles(call, winograd=1) == (0, []) and b"winograd" in lib().sbgm_last_error()
    refused = R.dgrad_call(R.REFUSED_CASE)
    assert refused["Cout"] == 16 and tiles(refused) == (0, []) and b"multiple of 32" in lib().sbgm_last_error()
    assert lib().sbgm_conv2d_tiles(None, None, 0) == 0
