"""CPU suite for the domain noise plan (day-keyed, temporally correlated noise of tiled and joint runs): the samplers'
argument checks, which fire before anything touches a device and name their argument (the refusals that stay included), the statistics
of the host restatement of the counter and the mix (domain_noise_ref.py over philox_ref.py), and the C ABI."""
import math
import os
import re

import numpy as np
import pytest
import torch

import domain_noise_ref as D
import philox_ref as P
import sbgm_danra_amd as S
from sbgm_danra_amd import _native as N
from sbgm_danra_amd import score_sampling as SS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STD = (S.marginal_prob_std_fn, S.diffusion_coeff_fn)
A_HW, A_ORIGINS, TILE = (44, 56), [(0, 0), (0, 24), (12, 0), (12, 24)], 32          # geometry A: 44 x 53 padded to 56, halo 4


def _never(*a, **k):
    raise AssertionError("the score model must not be evaluated")


SAMPLERS = {"em": (S.Euler_Maruyama_sampler, {}), "pc": (S.pc_sampler, {}), "edm": (S.edm_heun_sampler, {}),
            "dpm": (S.dpmpp_2m_sampler, {"eta": 1.0})}


# ---- 1: the samplers' argument checks ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(SAMPLERS))
def test_sampler_argument_checks_name_the_argument(kind):
    sampler, kw = SAMPLERS[kind]
    B, hw = 4, TILE
    run = lambda **how: sampler(_never, *STD, batch_size=B, device="cpu", img_size=hw, seed=1, num_steps=4, **kw, **how)  # noqa: E731
    w3 = SS.temporal_noise_weights(0.6, 3)
    origins = torch.tensor(A_ORIGINS, dtype=torch.int32)
    tiled = dict(tile_origins=origins, domain_width=56)
    plan = dict(tiled, noise_domain_row=9, domain_height=44)
    cases = [(dict(noise_domain_row=9, domain_height=44), "tile_origins"),                                  # a domain row needs tiles
             (dict(plan, noise=torch.zeros(9, B, 1, hw, hw)), "noise"),
             (dict(plan, noise_rows=[4, 5, 6, 7]), "noise_domain_row"),                                     # the two plans exclude each other
             (dict(tiled, domain_height=44), "domain_height"),                                              # ... needs its row
             (dict(tiled, noise_domain_row=9), "domain_height"),
             (dict(plan, domain_height=31), "domain_height"),                                               # lower than a tile
             (dict(plan, domain_height=44.0), "domain_height"),
             (dict(plan, domain_height=40, joint_tiles=(44, 8)), "domain_height"),                          # two heights
             (dict(plan, noise_domain_row=[9]), "noise_domain_row"), (dict(plan, noise_domain_row=9.0), "noise_domain_row"),
             (dict(plan, noise_domain_row=-1), "noise_domain_row"),
             (dict(plan, noise_domain_row=3, noise_weights=w3, noise_row_stride=2), "noise_domain_row"),    # below (K - 1) * stride = 4
             (dict(plan, noise_domain_row=1 << 31), "noise_domain_row"),
             (dict(plan, noise_weights=np.full(33, 33 ** -0.5)), "noise_weights"),                          # K > 32
             (dict(plan, noise_weights=[0.6, 0.7]), "noise_weights"), (dict(plan, noise_weights=[]), "noise_weights"),
             (dict(plan, noise_row_stride=0), "noise_row_stride"),
             # what stays refused, under the names it had
             (dict(tiled, noise_rows=[4, 5, 6, 7]), "tile_origins"),
             (dict(tiled, noise_rows=[4, 5, 6, 7], joint_tiles=(44, 8)), "noise_rows"),
             (dict(tiled, noise_weights=w3), "noise_rows"), (dict(tiled, noise_row_stride=2), "noise_rows"),
             (dict(noise_weights=w3), "noise_rows")]
    for how, name in cases:
        with pytest.raises(ValueError, match=name):
            run(**how)
    # a plan that passes the checks reaches the loop: a callable that is no ScoreNet has no native loop to carry a tiled run
    for how in (dict(plan, noise_weights=w3, noise_row_stride=2), dict(plan, noise_domain_row=(1 << 31) - 1),
                dict(plan, joint_tiles=(44, 8)), dict(tiled, noise_domain_row=np.int64(4), joint_tiles=(44, 8))):
        with pytest.raises(N.NativeError, match="native sampler loop"):
            run(**how)
    # rk45_sampler is out of scope: it does not take the arguments
    with pytest.raises(TypeError, match="noise_domain_row"):
        S.rk45_sampler(_never, *STD, batch_size=B, device="cpu", img_size=hw, seed=1, error_norm="sample", **plan)


def test_temporal_noise_domain_checks_before_the_device():
    good = dict(row=9, origins=A_ORIGINS, tile=TILE, domain_hw=A_HW)
    w3 = SS.temporal_noise_weights(0.5, 3)
    for how, name in ((dict(good, origins=[0, 0]), "origins"), (dict(good, origins=[(0.0, 0.0)]), "origins"),
                      (dict(good, origins=[(0, 2)]), "origins"), (dict(good, origins=[(13, 0)]), "origins"),          # 13 + 32 > 44
                      (dict(good, origins=[(0, 28)]), "origins"), (dict(good, origins=[(-1, 0)]), "origins"),
                      (dict(good, tile=30), "tile"), (dict(good, domain_hw=44), "domain_hw"), (dict(good, domain_hw=(31, 56)), "domain_hw"),
                      (dict(good, row=1, weights=w3), "noise_domain_row"), (dict(good, weights=[2.0]), "noise_weights"),
                      (dict(good, stride=0), "noise_row_stride")):
        with pytest.raises(ValueError, match=name):
            SS.temporal_noise_domain(1, 0, **how)
    with pytest.raises(N.NativeError, match="device"):
        SS.temporal_noise_domain(1, 0, device="cpu", **good)
    assert S.temporal_noise_domain is SS.temporal_noise_domain


# ---- 2: the counter and the mix ------------------------------------------------------------------------------------------------------
def test_counters_are_the_tiled_draw_and_the_rows_draw():
    Hd, Wd = A_HW
    seed, off = 5 + (9 << 32), 3 + (1 << 33)
    # R = 0, one lag: the counter of today's tiled draw, quad (Y, X4) -> Y dom_w4 + X4
    c0 = D.counters(0, 0, 1, Hd, Wd)
    assert c0.dtype == np.uint64 and np.array_equal(c0.reshape(-1), np.arange(Hd * Wd // 4, dtype=np.uint64))
    assert np.array_equal(D.domain_draw(seed, off, 0, Hd, Wd, [1.0]), P.domain_draw(seed, off, Hd, Wd).astype(np.float32))
    # one tile that covers the domain: Q is the sample's quad count, the counters are those of noise_rows = [R]: (R - k s) P4 + q
    R_, s = (1 << 31) - 5, 3
    for k in (0, 2):
        c = D.counters(R_, k, s, 32, 32)
        assert np.array_equal(c.reshape(-1), np.uint64((R_ - k * s) * 256) + np.arange(256, dtype=np.uint64))
    assert int(D.counters(R_, 0, s, 32, 32).max()) > 1 << 32                                     # this row needs 64 bits
    # a width that is no multiple of 4 counts its last, partial quad: 53 -> 14 quads a row
    assert D.counters(2, 1, 1, 44, 53).shape == (44, 14) and int(D.counters(2, 1, 1, 44, 53)[0, 0]) == 44 * 14
    # rows do not overlap: the last counter of a row is one below the first of the next
    assert int(D.counters(6, 0, 1, Hd, Wd).max()) + 1 == int(D.counters(7, 0, 1, Hd, Wd).min())
    # overlapping tiles see one draw
    tiles = D.cut(D.domain_draw(seed, off, 7, Hd, Wd, SS.temporal_noise_weights(0.6, 3), 2), A_ORIGINS, TILE)
    assert np.array_equal(tiles[0][:, 24:], tiles[1][:, :8]) and np.array_equal(tiles[0][12:], tiles[2][:20])


@pytest.mark.parametrize("rho,lags,stride", [(0.6, 3, 1), (0.8, 4, 2)])
def test_consecutive_domain_rows_correlate_at_acf1(rho, lags, stride):
    Hd, Wd = A_HW
    n = Hd * Wd
    seed, off = 77 + (2 << 32), 4
    w = SS.temporal_noise_weights(rho, lags)
    acf = SS.temporal_noise_acf(w)
    R0 = (lags - 1) * stride + 5
    rows = {r: D.domain_draw(seed, off, r, Hd, Wd, w, stride).astype(np.float64).reshape(-1) for r in (R0, R0 + stride, R0 + lags * stride)}
    corr = lambda a, b: float(np.corrcoef(a, b)[0, 1])  # noqa: E731
    c1, cK = corr(rows[R0], rows[R0 + stride]), corr(rows[R0], rows[R0 + lags * stride])
    var = float(rows[R0].var())
    print(f"rho {rho} K {lags} stride {stride}: lag-1 corr {c1:.4f} (acf[1] {acf[1]:.4f}), K strides apart {cK:.4f}, var {var:.4f}; "
          f"bound {5 / math.sqrt(n):.4f}")
    assert abs(c1 - acf[1]) <= 5 / math.sqrt(n)
    assert abs(cK) <= 5 / math.sqrt(n)
    assert abs(var - 1.0) <= 5 * math.sqrt(2.0 / n)                                              # every draw stays N(0, 1)


# ---- 3: the C ABI --------------------------------------------------------------------------------------------------------------------
def test_symbols_and_abi_version():
    lib = N.lib()
    header = open(os.path.join(ROOT, "include", "sbgm_hip.h")).read()
    assert lib.sbgm_abi_version() == N.ABI_VERSION >= 17
    for name, n in (("sbgm_sampler_set_noise_domain_row", 6), ("sbgm_randn_domain_rows", 15)):
        assert name in N.SIGNATURES and getattr(lib, name) is not None and len(N.SIGNATURES[name][1]) == n
        decl = re.search(rf"\bint {name}\((.*?)\);", header, flags=re.S).group(1)
        assert decl.count(",") + 1 == n, name
    # no device is touched by a refused call
    assert lib.sbgm_sampler_set_noise_domain_row(None, None, 44, 1, None, 0) != 0 and b"null model" in lib.sbgm_last_error()
    assert lib.sbgm_randn_domain_rows(None, 1.0, 0, 0, None, None, 1, 32, 32, 32, 32, 1, None, 1, None) != 0
    assert b"randn_domain_rows" in lib.sbgm_last_error()
