"""sbgm_ln_linear_fwd (a LayerNorm folded into the linear after it, conv_igemm.hip in_mode 3) against the float64 chain
LayerNorm -> Linear (+ residual, + GELU), on every tile candidate sbgm_ln_linear_tiles returns (FCO x FPX x WS in {1, 2, 4}).

Shapes: M in {16 one fragment, 17 ragged, 48 a partial FPX = 2 / 4 tile and a tile slot without a tile under WS < 4, 2048 real},
C in {16 one K step, 48 an odd step count: the pipeline tail and an uneven WS share, 256 and 512 real}, Cout in {16, 48, 768}.
Inputs (tests/ln_fold_ref.py): centred normal rows, ReLU-like rows, rows shifted to |mean|/sigma = 4, 16 and 64, one constant row;
inputs and outputs sit inside NaN-poisoned allocations.

Bound per element, plain launch:   |got - want| <= 8 (2^-24 r sum_k |W''[co][k]| |x_k| + 2^-23 |want|)
a forward bound of the fp32 chain (the factor 8 from an fp32 simulation of that formula, worst ratio 3.1), which scales by itself
with the conditioning |mean|/sigma of the row.  With a residual and GELU the epilogue adds res (one rounding of pre = lin + res) and
applies GELU, whose slope is at most 1.13 and whose own error is a few ulp of |pre| (erf near -1 cancels, so not of |want|):
    |got - want| <= 1.13 * 8 (2^-24 r sum_k |W''| |x| + 2^-23 |pre|) + 8 * 2^-23 |pre|.
Every case prints `LN-FOLD <shape> tile=<...> <variant> ratio=<worst |got - want| / bracket, the bracket without the factor 8>`
before it asserts (plain launches: at most 8; the worst ratio per tile is recorded in DESIGN.md 3.3)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import ln_fold_ref as R
from attention_ref import Poisoned
from sbgm_danra_amd import _native as N

pytestmark = pytest.mark.gpu

DEV = "cuda"
MS, WIDTHS, COUTS = (16, 17, 48, 2048), (16, 48, 256, 512), (16, 48, 768)
GELU = 3          # SBGM_GELU


def lib():
    return N.lib()


def tiles(M, C_, Cout):
    buf = (C.c_int * (6 * 64))()
    n = lib().sbgm_ln_linear_tiles(M, C_, Cout, buf, 64)
    return [tuple(buf[6 * i:6 * i + 6]) for i in range(n)]


@functools.lru_cache(maxsize=None)
def device_case(C_, Cout):
    """the operands packed by the ABI and the float64 results of ln_fold_ref.case on the device, once per (C, Cout), read-only"""
    c = R.case(C_, Cout)
    dv = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dt)  # noqa: E731
    w, b, gamma, beta = dv(c["w"]), dv(c["b"]), dv(c["gamma"]), dv(c["beta"])
    w2 = torch.full((Cout, C_), float("nan"), device=DEV)
    h = torch.full((Cout,), float("nan"), device=DEV)
    packed = torch.full((lib().sbgm_conv_packed_numel(Cout, 1, 1, C_),), float("nan"), device=DEV)
    N.check(lib().sbgm_ln_fold_pack(w.data_ptr(), b.data_ptr(), gamma.data_ptr(), beta.data_ptr(), C_, Cout, w2.data_ptr(), packed.data_ptr(),
                                    h.data_ptr(), N.stream()))
    torch.cuda.synchronize()
    f64 = torch.float64
    return dict(host=c, w2=w2, h=h, packed=packed, want=dv(c["want"], f64), bracket=dv(c["bracket"], f64), pre=dv(c["pre"], f64),
                want_act=dv(c["want_act"], f64), res=dv(c["res"]))


@pytest.mark.parametrize("C_", WIDTHS)
def test_pack_agrees_with_the_host_restatement(C_):
    """W'' and h of the device pack against float64 sums rounded once (the device sums in another order: a last-place difference
    where the float64 value sits on a rounding boundary), and the image is the ordinary implicit-GEMM image of the W'' it wrote"""
    Cout = 48
    d = device_case(C_, Cout)
    w2f, hf, _ = R.pack_host(*(d["host"][k] for k in ("w", "b", "gamma", "beta")))
    got, goth = d["w2"].cpu().numpy(), d["h"].cpu().numpy()
    scale = float(np.abs(d["host"]["w"]).max())
    dw = np.abs(got.astype(np.float64) - w2f) - (np.spacing(np.abs(w2f)) + 1e-14 * scale)
    dh = np.abs(goth.astype(np.float64) - hf) - np.spacing(np.abs(hf))
    print(f"LN-FOLD pack C={C_}: {int((got != w2f).sum())} of {got.size} elements of W'' and {int((goth != hf).sum())} of {Cout} of h differ "
          f"from the host's rounding")
    assert (dw <= 0).all() and (dh <= 0).all()
    assert (got != w2f).mean() <= 1e-3
    image = np.ascontiguousarray(got.reshape(Cout, C_ // 16, 16).transpose(1, 0, 2)).reshape(-1)
    assert np.array_equal(d["packed"].cpu().numpy(), image)


def run(d, M, C_, Cout, tile, res, act):
    x = Poisoned((M, C_), DEV, torch.from_numpy(d["host"]["x"][:M]))
    out = Poisoned((M, Cout), DEV)
    r = Poisoned((M, Cout), DEV, d["res"][:M]) if res else None
    t = (C.c_int * 6)(*tile) if tile is not None else None
    N.check(lib().sbgm_ln_linear_fwd(x.ptr(), d["packed"].data_ptr(), d["h"].data_ptr(), r.ptr() if res else None, act, R.EPS, out.ptr(),
                                     M, C_, Cout, t, N.stream()))
    torch.cuda.synchronize()
    assert x.surround_unchanged() and out.surround_unchanged() and (r is None or r.surround_unchanged()), "the kernel wrote outside its tensors"
    assert torch.equal(x.t.cpu(), torch.from_numpy(d["host"]["x"][:M])), "the kernel wrote into its input"
    return out.t


def worst_ratio(got, want, tol):
    """max |got - want| / tol on the device in float64 (a NaN or Inf counts as infinitely wrong), and where"""
    ratio = (got.double() - want).abs() / tol
    ratio = torch.where(torch.isfinite(got), ratio, torch.full_like(ratio, float("inf")))
    i = int(ratio.argmax())
    return float(ratio.reshape(-1)[i]), divmod(i, got.shape[1])


@pytest.mark.parametrize("C_", WIDTHS)
@pytest.mark.parametrize("Cout", COUTS)
def test_every_tile_against_float64(C_, Cout):
    d = device_case(C_, Cout)
    fails, worst_of_tile = [], {}
    for M in MS:
        cand = tiles(M, C_, Cout)
        assert cand and all(t[2] == 1 and t[4] == t[5] == 0 and {t[0], t[1], t[3]} <= {1, 2, 4} for t in cand), cand
        want, bracket, pre, want_act = (d[k][:M] for k in ("want", "bracket", "pre", "want_act"))
        plain_tol = 2.0 ** -24 * bracket + 2.0 ** -23 * want.abs()
        act_tol = 1.13 * (2.0 ** -24 * bracket + 2.0 ** -23 * pre.abs()) + 2.0 ** -23 * pre.abs()
        for tile in cand + [None]:                      # None: the static tile
            got = run(d, M, C_, Cout, tile, False, 0)
            ratio, (row, co) = worst_ratio(got, want, plain_tol)
            print(f"LN-FOLD M={M} C={C_} Cout={Cout} tile={tile} plain ratio={ratio:.3g} at row {row} ({R.row_family(row)}) co {co}")
            worst_of_tile[tile] = max(worst_of_tile.get(tile, 0.0), ratio)
            if not ratio <= 8.0:
                fails.append(f"M={M} tile={tile} plain: {ratio:.3g} x the bracket at row {row} ({R.row_family(row)}) co {co}")
            if tile is not None and M in (17, 2048):
                assert torch.equal(run(d, M, C_, Cout, tile, False, 0), got), "two runs differ (there are no atomics here)"
            got = run(d, M, C_, Cout, tile, True, GELU)
            ratio, (row, co) = worst_ratio(got, want_act, act_tol)
            print(f"LN-FOLD M={M} C={C_} Cout={Cout} tile={tile} res+gelu ratio={ratio:.3g} at row {row} ({R.row_family(row)}) co {co}")
            if not ratio <= 8.0:
                fails.append(f"M={M} tile={tile} res+gelu: {ratio:.3g} x the bracket at row {row} ({R.row_family(row)}) co {co}")
    for tile, ratio in sorted(worst_of_tile.items(), key=str):
        print(f"LN-FOLD-WORST C={C_} Cout={Cout} tile={tile} worst plain ratio={ratio:.3g}")
    assert not fails, "\n".join(fails)


def test_refused_launches_write_nothing():
    """grid split-K, a family other than the implicit GEMM, a tile that does not divide Cout, C that is no multiple of 16"""
    d = device_case(256, 768)
    M = 48
    x = Poisoned((M, 256), DEV, torch.from_numpy(d["host"]["x"][:M]))
    out = Poisoned((M, 768), DEV)
    for tile, C_, Cout in (((2, 1, 2, 1, 0, 0), 256, 768), ((2, 1, 1, 1, 1, 0), 256, 768), ((4, 1, 1, 1, 0, 0), 256, 32), ((2, 1, 1, 1, 0, 0), 24, 768)):
        with pytest.raises(N.NativeError):
            N.check(lib().sbgm_ln_linear_fwd(x.ptr(), d["packed"].data_ptr(), d["h"].data_ptr(), None, 0, R.EPS, out.ptr(), M, C_, Cout,
                                             (C.c_int * 6)(*tile), N.stream()))
    torch.cuda.synchronize()
    assert out.surround_unchanged() and out.t.isnan().all()
