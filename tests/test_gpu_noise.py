"""The in-kernel noise (csrc/philox.h and every kernel that draws from it) against the host Philox reference of philox_ref.py, draw by
draw: the contract is the table "Who draws what" of DESIGN.md §4.4.

(a) uniform bits of the loss time, exact                      (b) the attention dropout mask, exact
(c) normals of sbgm_randn_scaled against the reference        (d) every consumer draws what sbgm_randn_scaled returns, exact
(e) the seeded sampler runs (step graph and eager) equal runs on injected device draws 0 .. need-1, exact
(f) domain-keyed tile noise, pixel by pixel                   (g) the rank tie-break, exact

(c) is the one comparison that is not exact: the reference evaluates log, sqrt, sin and cos in float64 on the kernel's own float32
operands (uniforms, angle product, -2 ln u rounded to float32), so the difference is the device math library's error.  Budget per
element, in units of 2^-24 r (r = the pair's radius): logf and sqrtf at 1 ulp, the two float32 products, sincosf at 2 ulp of a value in
[0.5, 1) -- 6 to 8 units; the bound is 16.  A keying, lane or constant error is of order 1, i.e. ~1e7 units.
Measured on MI355X: (a), (b), (d), (e), (f: the two overlap checks), (g) exact as stated; (c) at most 3.94 units over the 12 (seed, draw)
cases (3.27 .. 3.94 per case, printed by the test); (f) 1.3e-7 of max |want| against the bound 1e-5.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import philox_ref as P  # noqa: E402
from util_models import build_pair, maxrel  # noqa: E402

import sbgm_danra_amd as S  # noqa: E402
from sbgm_danra_amd import _native as N  # noqa: E402
from sbgm_danra_amd import score_sampling as SS  # noqa: E402
from sbgm_danra_amd import verification as V  # noqa: E402

DEV = "cuda"
STD = (S.marginal_prob_std_fn, S.diffusion_coeff_fn)
UNIT = 2.0 ** -24


def L():
    return N.lib()


def device_draw(seed, draw, n, scale=1.0):
    """D_draw: what sbgm_randn_scaled writes for (seed, draw), flat [n]"""
    x = torch.empty(n, device=DEV)
    N.check(L().sbgm_randn_scaled(x.data_ptr(), scale, seed, draw, n, N.stream()))
    return x


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


def soft_mask(*shape):
    """0 / 1 / 0.5 in runs whose edges are no multiples of 4"""
    m = torch.zeros(shape)
    flat = m.view(-1)
    flat[3::7] = 1.0
    flat[5::11] = 0.5
    flat[: flat.numel() // 5] = 1.0
    flat[flat.numel() // 5: flat.numel() // 5 + 9] = 0.5
    return m.to(DEV)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- (a) uniform bits on the device -------------------------------------------------------------------------------------------------
def perturb(B, per, seed=0, pair=None, t_eps=0.0):
    """sbgm_dsm_perturb with in-kernel draws: seed by value (pair None), or a device (seed, offset) pair -> (t_out numpy, z_out)"""
    x = torch.zeros(B, per, device=DEV)
    xp, z = torch.empty_like(x), torch.empty_like(x)
    t, sd = torch.empty(B, device=DEV), torch.empty(B, device=DEV)
    state = None if pair is None else torch.tensor(list(pair), dtype=torch.int64, device=DEV)
    N.check(L().sbgm_dsm_perturb(x.data_ptr(), None, None, N.ptr(state), 0 if pair is not None else seed, t_eps, 25.0, xp.data_ptr(),
                                 z.data_ptr(), t.data_ptr(), sd.data_ptr(), B, per, N.stream()))
    return t.cpu().numpy(), z


def same_bits(got, want, what):
    bad = np.nonzero(bits(got) != bits(want))[0]
    if bad.size:
        # c >> 8 >= 2^23 <=> u >= 0.5: were every mismatch there, the emulation of the `+ 0.5f` rounding would be what differs
        raise AssertionError(f"{what}: {bad.size} of {got.size} differ, {int((np.asarray(want)[bad] >= 0.5).sum())} of them with "
                             f"c >> 8 >= 2^23; first at {bad[0]}: got {got[bad[0]]!r} want {want[bad[0]]!r}")


@pytest.mark.parametrize("seed", [0, 1234, 0x299f31d0a4093822])
def test_loss_time_is_the_first_uniform_of_stream_2off(seed):
    B = 257
    b = np.arange(B, dtype=np.uint64)
    t, _ = perturb(B, 4, seed=seed)
    same_bits(t, P.uniform4(seed, 0, b)[:, 0], f"seed {seed:#x} by value")
    if seed == 0:
        assert t[0] == np.float32((0x6627e8 + 0.5) * UNIT)                # the first Random123 known-answer vector
    for off in (0, 1, 5):
        t, _ = perturb(B, 4, pair=(seed, off))
        u = P.uniform4(seed, 2 * off, b)[:, 0]
        same_bits(t, u, f"device pair ({seed:#x}, {off})")
        assert t.min() >= 0.0 and t.max() <= 1.0
        # t_eps > 0: u (1 - eps) + eps in float32, the compiler free to fuse the multiply-add: within 1 ulp of the unfused value
        eps = np.float32(1e-3)
        te, _ = perturb(B, 4, pair=(seed, off), t_eps=1e-3)
        want = u * (np.float32(1.0) - eps) + eps
        assert want.dtype == np.float32
        assert (np.abs(te.astype(np.float64) - want.astype(np.float64)) <= np.spacing(want).astype(np.float64)).all()
        assert te.min() >= eps and te.max() <= 1.0


# ---- (b) dropout mask ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,S_,heads", [(2, 33, 3), (1, 64, 4)])
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("offset", [0, 7])
def test_dropout_mask_is_lane_e_and_3_of_quad_e_shift_2(B, S_, heads, p, offset):
    seed = (1 << 32) + 5
    total = B * heads * S_ * S_
    mask = torch.empty(total, device=DEV)
    N.check(L().sbgm_mha_dropout_mask(mask.data_ptr(), B, S_, heads, p, seed, offset, N.stream()))
    # element e = ((b heads + h) S + i) S + j is the flat index: lane e & 3 of quad e >> 2 is element e of the quads laid end to end
    u = P.uniform4(seed, offset, np.arange((total + 3) // 4, dtype=np.uint64)).reshape(-1)[:total]
    pf = np.float32(p)
    want = np.where(u < pf, np.float32(0.0), np.float32(1.0) / (np.float32(1.0) - pf)).astype(np.float32)
    got = mask.cpu().numpy()
    assert np.array_equal(bits(got), bits(want)), f"{int((bits(got) != bits(want)).sum())} of {total} mask entries differ"
    assert 0 < (want == 0).sum() < total


# ---- (c) normals ----------------------------------------------------------------------------------------------------------------------
SIZES = (4, 4 * 257, 4 * (2048 * 256 + 3))          # one quad; two blocks, the second partial; a second trip of the grid-stride loop


@pytest.mark.parametrize("seed", [0, 1234, (1 << 32) + 5, (1 << 63) + 11])
@pytest.mark.parametrize("draw", [0, 1, (1 << 32) + 3])
def test_normals_match_the_reference(seed, draw):
    """|device - reference| <= 16 * 2^-24 * r per element, for n in SIZES (quad i does not depend on n: one reference serves all)."""
    want, r = P.draw_with_radius(seed, draw, SIZES[-1])
    worst = 0.0
    for n in SIZES:
        got = device_draw(seed, draw, n).cpu().numpy().astype(np.float64)
        err = np.abs(got - want[:n])
        units = err / np.maximum(UNIT * r[:n], 1e-300)
        units[(r[:n] == 0) & (err == 0)] = 0.0
        worst = max(worst, float(units.max()))
        bad = np.nonzero(err > 16 * UNIT * r[:n])[0]
        assert bad.size == 0, (f"n={n}: {bad.size} elements beyond 16 units of 2^-24 r, max {units.max():.3g} units; first at {bad[0]}: "
                               f"got {got[bad[0]]!r} want {want[bad[0]]!r}")
    print(f"normals seed {seed:#x} draw {draw:#x}: max |device - reference| = {worst:.2f} units of 2^-24 r")


def test_scale_is_one_exact_multiply():
    n = SIZES[1]
    assert torch.equal(device_draw(1234, 3, n, scale=2.0), 2.0 * device_draw(1234, 3, n))


# ---- (d) consumers draw what sbgm_randn_scaled returns --------------------------------------------------------------------------------
N_D, DRAW = 4 * 257, 3
SEEDS_D = [1234, (1 << 63) + 11]


@pytest.mark.parametrize("seed", SEEDS_D)
def test_em_step_draws_D(seed):
    x0, s, D = rnd(N_D, seed=1) * 10, rnd(N_D, seed=2), device_draw(seed, DRAW, N_D)
    out = []
    for z in (None, D):
        x, xm = x0.clone(), torch.empty_like(x0)
        N.check(L().sbgm_em_step(x.data_ptr(), xm.data_ptr(), s.data_ptr(), N.ptr(z), 3.7, 1e-3, 0.06, seed, DRAW, N_D, N.stream()))
        out.append((x, xm))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert not torch.equal(out[0][0], out[0][1])                         # the draw did enter x


@pytest.mark.parametrize("seed", SEEDS_D)
def test_langevin_step_draws_D(seed):
    B = 3
    x0, s, D = rnd(B, N_D, seed=3) * 10, rnd(B, N_D, seed=4), device_draw(seed, DRAW, B * N_D)
    ws = torch.empty(B, dtype=torch.float64, device=DEV)
    out = []
    for z in (None, D):
        x = x0.clone()
        N.check(L().sbgm_langevin_step(x.data_ptr(), s.data_ptr(), N.ptr(z), 0.16 * math.sqrt(N_D), ws.data_ptr(), seed, DRAW, B, N_D,
                                       N.stream()))
        out.append(x)
    assert torch.equal(out[0], out[1]) and not torch.equal(out[0], x0)


@pytest.mark.parametrize("seed", SEEDS_D)
def test_edm_churn_draws_D(seed):
    x0, D = rnd(N_D, seed=5) * 10, device_draw(seed, DRAW, N_D)
    out = []
    for z in (None, D):
        x = x0.clone()
        N.check(L().sbgm_edm_churn(x.data_ptr(), N.ptr(z), 0.7, seed, DRAW, N_D, N.stream()))
        out.append(x)
    assert torch.equal(out[0], out[1]) and not torch.equal(out[0], x0)


@pytest.mark.parametrize("seed", SEEDS_D)
def test_hold_known_draws_D(seed):
    x0, xm0, known, mask, D = rnd(N_D, seed=6) * 10, rnd(N_D, seed=7), rnd(N_D, seed=8), soft_mask(N_D), device_draw(seed, DRAW, N_D)
    out = []
    for z in (None, D):
        x, xm = x0.clone(), xm0.clone()
        N.check(L().sbgm_hold_known(x.data_ptr(), xm.data_ptr(), known.data_ptr(), mask.data_ptr(), N.ptr(z), 1.3, seed, DRAW, N_D,
                                    N.stream()))
        out.append((x, xm))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert torch.equal(out[0][0][mask == 0], x0[mask == 0]) and not torch.equal(out[0][0][mask == 1], known[mask == 1])


@pytest.mark.parametrize("seed", [1234, 0x299f31d0a4093822])
def test_loss_noise_is_stream_2off_plus_1(seed):
    B, per = 3, 4 * 65
    for off in (0, 1, 5):
        _, z = perturb(B, per, pair=(seed, off), t_eps=1e-3)
        assert torch.equal(z.view(-1), device_draw(seed, 2 * off + 1, B * per)), off
    _, z = perturb(B, per, seed=seed, t_eps=1e-3)                        # seed by value: offset 0
    assert torch.equal(z.view(-1), device_draw(seed, 1, B * per))


# ---- (e) the seeded production path follows the documented draw schedule --------------------------------------------------------------
@pytest.fixture(scope="module")
def net():
    _, n, _ = build_pair(1)
    return n.eval()


KINDS = {"em": (S.Euler_Maruyama_sampler, N.SAMPLER_EM, {}, 5), "pc": (S.pc_sampler, N.SAMPLER_PC, {}, 9),
         "edm": (S.edm_heun_sampler, N.SAMPLER_EDM_HEUN, dict(s_churn=40.0), 5)}


@pytest.mark.parametrize("held", [False, True])
@pytest.mark.parametrize("kind", ["em", "pc", "edm"])
def test_seeded_run_equals_the_run_on_injected_device_draws(net, kind, held):
    sampler, code, kw, need = KINDS[kind]
    B, hw, steps, seed = 2, 32, 4, 1234 + (7 << 32)
    assert SS._counts(code, steps, bool(kw))[1] == need
    cond = rnd(B, 1, hw, hw, seed=11)
    if held:                                                              # EDM Heun: ties its recomputed draw0 to draw 0
        kw = dict(kw, known=rnd(B, 1, hw, hw, seed=12), known_mask=soft_mask(B, 1, hw, hw))
    run = lambda **how: sampler(net, *STD, batch_size=B, num_steps=steps, device=DEV, img_size=hw, cond_img=cond, **kw, **how)  # noqa: E731
    D = torch.stack([device_draw(seed, i, B * hw * hw).view(B, 1, hw, hw) for i in range(need)])
    want = run(noise=D)
    assert torch.isfinite(want).all()
    for graph in (True, False):
        got = run(seed=seed, use_graph=graph)
        assert torch.equal(got, want), (f"{kind} held={held} use_graph={graph}: seeded run differs from the run on draws 0..{need - 1}, "
                                        f"max-rel {maxrel(got, want):.3e}")
    if need > 2:                                                          # the schedule is observable: another order is another result
        assert not torch.equal(run(noise=D[[0, 2, 1] + list(range(3, need))]), want)


def test_rk45_seeded_start_is_std1_times_draw_0():
    _, plain, _ = build_pair(0)
    plain.eval()
    B, hw, seed, tol = 2, 32, 1234 + (7 << 32), 1e-3
    kw = dict(batch_size=B, img_size=hw, rtol=tol, atol=tol)
    D0 = device_draw(seed, 0, B * hw * hw).view(1, B, 1, hw, hw)
    seeded = S.rk45_sampler(plain, *STD, seed=seed, **kw)
    assert torch.equal(seeded, S.rk45_sampler(plain, *STD, noise=D0, **kw))             # both scaled by the engine's std(1)
    # the same start handed over as z: the scale is torch's std(1), an ulp from the engine's at most, and the two solves agree to the
    # solver's own tolerance (the bound test_gpu_rk45_sampler.py uses for this pair)
    via_z = S.rk45_sampler(plain, *STD, z=D0[0] * S.marginal_prob_std_fn(torch.ones(1, device=DEV)), **kw)
    assert maxrel(seeded, via_z) <= 20 * tol


# ---- (f) domain-keyed tile noise --------------------------------------------------------------------------------------------------------
def test_tile_noise_is_the_domain_draw_pixel_by_pixel():
    from sbgm_danra_amd.tiling import FullDomainTiler
    _, znet, _ = build_pair(1)
    znet.eval()
    fin = znet.decoder.final_layer.conv
    with torch.no_grad():                                                 # score == 0 exactly: the state is a sum of draws
        fin.weight.zero_()
        fin.bias.zero_()
    t = FullDomainTiler((70, 84), 32, 8)
    Hd, Wd = t.Hd, t.Wd_pad
    T, hw, seed, steps = len(t), 32, 21 + (3 << 32), 3
    assert Wd % 4 == 0 and any(x0 % 4 == 0 and x0 % 8 != 0 for _, x0 in t.origins) and any(y0 % 4 for y0, _ in t.origins)
    D = [device_draw(seed, i, Hd * Wd).view(Hd, Wd) for i in range(steps)]
    ref0, r0 = P.draw_with_radius(seed, 0, Hd * Wd)                       # ... and D_0 at this n is the reference's domain draw
    assert (np.abs(D[0].cpu().numpy().reshape(-1) - ref0) <= 16 * UNIT * r0).all()
    assert np.array_equal(ref0.reshape(Hd, Wd), P.domain_draw(seed, 0, Hd, Wd))
    cond = rnd(T, 1, hw, hw, seed=13)
    got = S.Euler_Maruyama_sampler(znet, *STD, batch_size=T, num_steps=steps, device=DEV, img_size=hw, cond_img=cond, seed=seed,
                                   tile_origins=t.origins_dev, domain_width=Wd)
    # the coefficients as the Python loop computes them: std(1), then g(t_i) sqrt(dt) of the steps whose draw reaches the last mean_x
    ones = torch.ones(T, device=DEV)
    ts = torch.linspace(1.0, 1e-3, steps, device=DEV)
    dt = float(ts[0] - ts[1])
    coef = [float(S.marginal_prob_std_fn(ones)[0])] + [math.sqrt(dt) * float(S.diffusion_coeff_fn(ones * tt)[0]) for tt in ts.tolist()[:-1]]
    dom = sum(c * d.double() for c, d in zip(coef, D))
    want = torch.stack([dom[y0:y0 + hw, x0:x0 + hw] for y0, x0 in t.origins]).view(T, 1, hw, hw)
    err = float((got.double() - want).abs().max() / want.abs().max())
    print(f"tile noise: max |got - want| / max |want| = {err:.2e} over {T} tiles of a {Hd} x {Wd} domain")
    assert err <= 1e-5
    # pixels that two tiles share: bit-equal, after the steps ...
    (ya, xa), (yb, xb) = t.origins[0], t.origins[1]
    assert ya == yb and xa < xb < xa + hw and xb % 8 != 0
    ov = xa + hw - xb
    assert torch.equal(got[0, 0, :, hw - ov:], got[1, 0, :, :ov])
    # ... and in the initial state, read through the ODE sampler: with a zero score its right-hand side is zero and the result is the
    # start, std(1) * D_0 on every tile's window
    x0 = S.rk45_sampler(znet, *STD, batch_size=T, device=DEV, img_size=hw, cond_img=cond, seed=seed, error_norm="sample",
                        tile_origins=t.origins_dev, domain_width=Wd)
    assert torch.equal(x0[0, 0, :, hw - ov:], x0[1, 0, :, :ov])
    win0 = torch.stack([D[0][y0:y0 + hw, x0_:x0_ + hw] for y0, x0_ in t.origins]).view(T, 1, hw, hw)
    assert maxrel(x0.double(), coef[0] * win0.double()) <= 1e-6           # one float32 multiply, the scale an ulp apart at most


# ---- (g) rank tie-break -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [11, 12])
def test_rank_tie_break_is_the_first_uniform_of_the_pixel(seed):
    M, shape = 7, (33, 5)
    ens, obs = torch.ones(M, *shape, device=DEV), torch.ones(*shape, device=DEV)
    rank = V.ensemble_scores(ens, obs, seed=seed)["rank"].cpu().numpy().reshape(-1)
    u = P.uniform4(seed, 0, np.arange(shape[0] * shape[1], dtype=np.uint64))[:, 0]
    prod = u * np.float32(M + 1)
    assert prod.dtype == np.float32
    want = np.minimum(M, np.floor(prod).astype(np.int64))
    assert np.array_equal(rank, want)
    assert len(set(want.tolist())) == M + 1                               # every rank 0..M occurs: the comparison is not vacuous
