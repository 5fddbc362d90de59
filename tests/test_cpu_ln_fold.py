"""A LayerNorm folded into the linear after it, on the host (numpy only): the identity linear(LN(x)) = r W'' x + h in float64, the
zero row sums of W'', the host restatement of sbgm_ln_fold_pack against the definition, and the tile candidates of the launch."""
import ctypes as C

import numpy as np
import pytest

import ln_fold_ref as R

WIDTHS = (16, 48, 256, 512)


@pytest.mark.parametrize("C_", WIDTHS)
def test_folded_form_equals_layernorm_then_linear(C_):
    """r W'' x + h against Linear(LayerNorm(x)), both float64, to 1e-13 of max|want|, on rows of every family: centred, ReLU-like,
    |mean|/sigma = 4, 16, 64 and one constant row"""
    c = R.case(C_, 48)
    x = c["x"][:96].astype(np.float64)
    fams = {R.row_family(i) for i in range(96)}
    assert fams == set(R.FAMILIES)
    shifted = x[4]
    assert abs(abs(shifted.mean()) / shifted.std() - 64.0) < 1e-3 and np.ptp(x[5]) == 0.0
    want = R.layernorm_linear(x, c["w"], c["b"], c["gamma"], c["beta"])
    got = R.inv_sigma(x)[:, None] * (x @ c["w2"].T) + c["h"][None, :]
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"LN-FOLD-CPU C={C_} max|r W'' x + h - Linear(LN(x))| / max|want| = {err:.3e}")
    assert err <= 1e-13


@pytest.mark.parametrize("C_", WIDTHS)
def test_rows_of_the_folded_weight_sum_to_zero(C_):
    w2 = R.case(C_, 768)["w2"]
    assert (np.abs(w2.sum(1)) <= 4 * np.finfo(np.float64).eps * np.abs(w2).sum(1)).all()


@pytest.mark.parametrize("C_", WIDTHS)
def test_host_pack_rounds_the_definition_once(C_):
    """the restatement of the ABI's pack: each element of W'' and h within half an fp32 ulp of the float64 value, and the image is the
    implicit-GEMM layout [C/16][Cout][16] of that matrix"""
    c = R.case(C_, 48)
    w2f, hf, image = R.pack_host(c["w"], c["b"], c["gamma"], c["beta"])
    assert w2f.dtype == hf.dtype == image.dtype == np.float32
    half_ulp = np.spacing(np.abs(w2f)).astype(np.float64) / 2
    assert (np.abs(w2f.astype(np.float64) - c["w2"]) <= half_ulp).all()
    assert (np.abs(hf.astype(np.float64) - c["h"]) <= np.spacing(np.abs(hf)).astype(np.float64) / 2).all()
    img = image.reshape(C_ // 16, 48, 16)
    for co, k in ((0, 0), (47, C_ - 1), (17, 5), (3, C_ // 2)):
        assert img[k // 16, co, k % 16] == w2f[co, k]


def test_tile_candidates_of_the_folded_launch():
    """sbgm_ln_linear_tiles: implicit-GEMM tiles FCO x FPX x WS in {1, 2, 4}, one grid row, only tiles that divide Cout, waves that
    each get two K steps; nothing for shapes the launch refuses"""
    from sbgm_danra_amd import _native as N
    lib = N.lib()
    assert lib.sbgm_abi_version() == N.ABI_VERSION >= 11

    def tiles(M, C_, Cout):
        buf = (C.c_int * (6 * 64))()
        n = lib.sbgm_ln_linear_tiles(M, C_, Cout, buf, 64)
        assert 0 <= n <= 64
        return [tuple(buf[6 * i:6 * i + 6]) for i in range(n)]

    for M in (16, 17, 48, 2048):
        for C_ in WIDTHS:
            for Cout in (16, 48, 768):
                got = tiles(M, C_, Cout)
                want = [(fco, fpx, 1, ws, 0, 0) for fco in (4, 2, 1) for fpx in (4, 2, 1) for ws in (1, 2, 4)
                        if Cout % (16 * fco) == 0 and (ws == 1 or (C_ // 16) // ws >= 2)]
                assert got == want, (M, C_, Cout, got)
    assert len(tiles(2048, 256, 768)) == 27 and len(tiles(16, 16, 16)) == 3
    assert tiles(16, 24, 32) == [] and tiles(16, 32, 24) == [] and tiles(0, 32, 32) == []
