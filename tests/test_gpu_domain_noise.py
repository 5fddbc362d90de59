"""The domain noise plan on the device: day-keyed, temporally correlated noise of tiled and joint full-domain runs.

(1) the op on geometry A, bit for bit against the float32 mix of temporal_noise_ref.py over sbgm_randn_scaled's flat draw
(2) the op on geometry B (one tile = the domain) against temporal_noise(rows=[R]), a row whose counter needs 64 bits included
(3) every consumer on A: tile t of a tiled run under a plan equals the untiled batch-of-one run of that tile on the op's draws, exact
(4) B: the tiled run under row R equals the untiled run under noise_rows=[R]; R = 0, K = 1 is the run without a plan, tiled and joint
(5) a joint run under a plan keeps the copies of a domain pixel bit-equal, and with a zero score is the weighted sum of the mixed draws
(6) FullDomainTiler.sample_series: extensible, independent of tiles_per_batch, correlated from day to day as acf[1]
(7) refusals leave the handle usable

Geometry A: domain 44 x 53, tile 32, halo 4: Wd_pad = 56, origins y in {0, 12}, x in {0, 24}, T = 4 (a padded width, overlaps on both
axes, a y origin that is no multiple of 4).  Geometry B: 32 x 32, one tile.

Everything is exact except the sum of (5), bound 1e-5 of max |want| (three float32 multiply-adds against their float64 sum, the bound of
the tile-noise and the row-noise tests), and the correlations of (6), within 5 / sqrt(n) of their expectation.

Premise of (3), established on the code without the plan: a tile of a tiled run equals the untiled batch-of-one run of that tile's
conditions on injected noise (the tile's windows of the plain domain draws) bit for bit; the test asserts it for every kind it uses
before it relies on it.
Measured on MI355X: every exact comparison holds as stated, predictor-corrector included; (5) 1.65e-07 of max |want| against 1e-5;
(6) lag-1 correlations 0.544 .. 0.560 against acf[1] = 0.548, three days apart -0.001 and -0.012, bound 0.073."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import temporal_noise_ref as R  # noqa: E402
from util_models import build_pair, maxrel  # noqa: E402

import sbgm_danra_amd as S  # noqa: E402
from sbgm_danra_amd import _native as N  # noqa: E402
from sbgm_danra_amd import score_sampling as SS  # noqa: E402
from sbgm_danra_amd.tiling import FullDomainTiler  # noqa: E402

DEV = "cuda"
STD = (S.marginal_prob_std_fn, S.diffusion_coeff_fn)
W3 = SS.temporal_noise_weights(0.6, 3)
HD, WD, WP, HW = 44, 53, 56, 32                                   # geometry A
ORIGINS = [(0, 0), (0, 24), (12, 0), (12, 24)]


def device_draw(seed, draw, n):
    """what sbgm_randn_scaled writes for (seed, draw): float32 numpy [n]"""
    x = torch.empty(n, device=DEV)
    N.check(N.lib().sbgm_randn_scaled(x.data_ptr(), 1.0, seed, draw, n, N.stream()))
    return x.cpu().numpy()


def mixed_domain(seed, draw, row, w, stride, hd=HD, wp=WP):
    """the definition: the float32 loop over the device's own white draws, reshaped [rows, hd, wp] -> numpy float32 [hd, wp]"""
    plain = device_draw(seed, draw, (row + 1) * hd * wp).reshape(row + 1, hd, wp)
    return R.mix([plain[row - k * stride] for k in range(len(w))], w)


def cut(dom, origins=ORIGINS, hw=HW):
    return np.stack([dom[y0:y0 + hw, x0:x0 + hw] for y0, x0 in origins])


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


@pytest.fixture(scope="module")
def net():
    _, n, _ = build_pair(1)
    return n.eval()


@pytest.fixture(scope="module")
def znet():
    """a network whose score is exactly zero: the state of a run is a sum of draws"""
    _, n, _ = build_pair(1)
    n.eval()
    fin = n.decoder.final_layer.conv
    with torch.no_grad():
        fin.weight.zero_()
        fin.bias.zero_()
    return n


@pytest.fixture(scope="module")
def A():
    """the tiler of geometry A, a random domain condition [1, 44, 53] and its tiles [4, 1, 32, 32]"""
    t = FullDomainTiler((HD, WD), HW, 4)
    assert t.origins == ORIGINS and t.Wd_pad == WP and len(t) == 4
    cond = rnd(1, HD, WD, seed=4)
    return t, cond, t.extract(cond)


# ---- (1) the op on geometry A --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1234, (1 << 32) + 5])
@pytest.mark.parametrize("draw", [0, (1 << 32) + 3])
def test_op_is_the_float32_mix_of_the_domain_draws(seed, draw):
    row, stride = 7, 2
    got = SS.temporal_noise_domain(seed, draw, row, ORIGINS, HW, (HD, WP), W3, stride)
    assert got.shape == (4, HW, HW) and got.dtype == torch.float32 and got.is_cuda
    g = got.cpu().numpy()
    want = cut(mixed_domain(seed, draw, row, W3, stride))
    assert np.array_equal(bits(g), bits(want)), f"{int((bits(g) != bits(want)).sum())} of {want.size} differ"
    plain = device_draw(seed, draw, HD * WP).reshape(HD, WP)
    assert not np.array_equal(want, cut(device_draw(seed, draw, 8 * HD * WP).reshape(8, HD, WP)[7]))     # the lags did enter
    # overlapping tiles agree on the pixels they share
    assert np.array_equal(bits(g[0][:, 24:]), bits(g[1][:, :8])) and np.array_equal(bits(g[0][12:]), bits(g[2][:20]))
    assert np.array_equal(bits(g[1][12:]), bits(g[3][:20])) and np.array_equal(bits(g[2][:, 24:]), bits(g[3][:, :8]))
    # row 0 with one lag of weight 1: today's tiled draw, the windows of the plain domain draw
    zero = SS.temporal_noise_domain(seed, draw, 0, ORIGINS, HW, (HD, WP)).cpu().numpy()
    assert np.array_equal(bits(zero), bits(cut(plain)))
    # the origins as a device tensor, and the scale as one exact multiply
    org = torch.tensor(ORIGINS, dtype=torch.int32, device=DEV)
    assert torch.equal(SS.temporal_noise_domain(seed, draw, row, org, HW, (HD, WP), W3, stride, scale=2.0), 2.0 * got)


# ---- (2) the op on geometry B ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", [9, (1 << 31) - 5])
def test_op_on_a_one_tile_domain_is_the_rows_op(row):
    seed, draw, stride = (3 << 32) + 11, (1 << 32) + 1, 3
    got = SS.temporal_noise_domain(seed, draw, row, [(0, 0)], HW, (HW, HW), W3, stride)
    want = SS.temporal_noise(seed, draw, [row], HW * HW, W3, stride).view(1, HW, HW)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert not torch.equal(got, SS.temporal_noise_domain(seed, draw, row - 1, [(0, 0)], HW, (HW, HW), W3, stride))


# ---- (3) every consumer on geometry A -------------------------------------------------------------------------------------------------
KINDS = {"em": (S.Euler_Maruyama_sampler, N.SAMPLER_EM, {}, 5), "pc": (S.pc_sampler, N.SAMPLER_PC, {}, 9),
         "edm": (S.edm_heun_sampler, N.SAMPLER_EDM_HEUN, dict(s_churn=40.0), 5),
         "dpm": (S.dpmpp_2m_sampler, N.SAMPLER_DPMPP_2M, dict(eta=1.0), 5)}


@pytest.mark.parametrize("held", [False, True])
@pytest.mark.parametrize("kind", list(KINDS))
def test_tile_of_a_run_under_a_plan_equals_its_untiled_run_on_the_ops_draws(net, A, kind, held):
    """Predictor-corrector is included: on a tile the Langevin step size uses the tile's own score norm, which is the batch-mean rule
    of the batch-of-one run, and the two were found bit-equal without a plan (the premise below)."""
    sampler, code, kw, need = KINDS[kind]
    t, _, tiles = A
    T, steps, seed, stride = len(t), 4, 1234 + (7 << 32), 3
    assert SS._counts(code, steps, True)[1] == need
    if held:
        kw = dict(kw, known=rnd(T, 1, HW, HW, seed=12), known_mask=soft_mask(T, 1, HW, HW))
    tiled = lambda **how: sampler(net, *STD, batch_size=T, num_steps=steps, device=DEV, img_size=HW, cond_img=tiles, seed=seed,  # noqa: E731
                                  tile_origins=t.origins_dev, domain_width=WP, **kw, **how)

    def untiled(i, D):                                     # tile i alone, on its windows of the draws D [need, T, 1, HW, HW]
        one = {k: (v[i:i + 1] if torch.is_tensor(v) else v) for k, v in kw.items()}
        return sampler(net, *STD, batch_size=1, num_steps=steps, device=DEV, img_size=HW, cond_img=tiles[i:i + 1],
                       noise=D[:, i:i + 1].contiguous(), **one)

    # the premise, without a plan: the tile's windows of the plain domain draws
    D0 = torch.stack([torch.from_numpy(cut(device_draw(seed, i, HD * WP).reshape(HD, WP))) for i in range(need)]).view(need, T, 1, HW, HW).to(DEV)
    plain = tiled()
    for i in range(T):
        assert torch.equal(plain[i:i + 1], untiled(i, D0)), f"{kind} held={held}: without a plan tile {i} differs from its untiled run"
    results = []
    for row in (9, 12):                                    # the second row: another value at the same device address
        D = torch.stack([SS.temporal_noise_domain(seed, i, row, ORIGINS, HW, (HD, WP), W3, stride) for i in range(need)]).view(need, T, 1, HW, HW)
        want = torch.cat([untiled(i, D) for i in range(T)])
        assert torch.isfinite(want).all()
        for graph in (True, False):
            got = tiled(use_graph=graph, noise_domain_row=row, domain_height=HD, noise_weights=W3, noise_row_stride=stride)
            assert torch.equal(got, want), (f"{kind} held={held} row={row} use_graph={graph}: the tiled run under the plan differs from the "
                                            f"untiled runs on the op's draws 0..{need - 1}, max-rel {maxrel(got, want):.3e}")
        results.append(want)
    assert not torch.equal(results[0], results[1]) and not torch.equal(results[0], plain)


# ---- (4) geometry B, and the plan that is no plan ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_one_tile_domain_is_the_rows_plan_and_row_zero_is_no_plan(net, A, kind):
    """Predictor-corrector is included (one tile: its own norm is the batch mean of the batch-of-one run)."""
    sampler, _, kw, _ = KINDS[kind]
    steps, seed, stride, row = 4, 99 + (2 << 32), 2, 11
    cond = rnd(1, 1, HW, HW, seed=21)
    org = torch.zeros(1, 2, dtype=torch.int32, device=DEV)
    run = lambda **how: sampler(net, *STD, batch_size=1, num_steps=steps, device=DEV, img_size=HW, cond_img=cond, seed=seed, **kw, **how)  # noqa: E731
    want = run(noise_rows=[row], noise_weights=W3, noise_row_stride=stride)
    got = run(tile_origins=org, domain_width=HW, noise_domain_row=row, domain_height=HW, noise_weights=W3, noise_row_stride=stride)
    assert torch.equal(got, want), f"{kind}: max-rel {maxrel(got, want):.3e}"
    one = dict(tile_origins=org, domain_width=HW)
    assert torch.equal(run(noise_domain_row=0, domain_height=HW, **one), run(**one))
    assert torch.equal(run(noise_domain_row=0, domain_height=HW, joint_tiles=(HW, 1), **one), run(joint_tiles=(HW, 1), **one))
    # the same on geometry A, tiled and joint
    t, _, tiles = A
    runA = lambda **how: sampler(net, *STD, batch_size=len(t), num_steps=steps, device=DEV, img_size=HW, cond_img=tiles, seed=seed,  # noqa: E731
                                 tile_origins=t.origins_dev, domain_width=WP, **kw, **how)
    assert torch.equal(runA(noise_domain_row=0, domain_height=HD, noise_weights=[1.0]), runA())
    joint = dict(joint_tiles=(HD, t.overlap))
    assert torch.equal(runA(noise_domain_row=0, **joint), runA(**joint))
    assert not torch.equal(runA(noise_domain_row=1, **joint), runA(**joint))


# ---- (5) a joint run under a plan ----------------------------------------------------------------------------------------------------------
def shared_rectangles(t):
    out = []
    for a, (ya, xa) in enumerate(t.origins):
        for b, (yb, xb) in enumerate(t.origins):
            y0, y1, x0, x1 = max(ya, yb), min(ya, yb) + t.tile, max(xa, xb), min(xa, xb) + t.tile
            if a < b and y0 < y1 and x0 < x1:
                out.append((a, b, (slice(y0 - ya, y1 - ya), slice(x0 - xa, x1 - xa)), (slice(y0 - yb, y1 - yb), slice(x0 - xb, x1 - xb))))
    return out


@pytest.mark.parametrize("kind", list(KINDS))
def test_joint_run_under_a_plan_keeps_copies_bit_equal(net, A, kind):
    sampler, _, kw, _ = KINDS[kind]
    t, _, tiles = A
    rects = shared_rectangles(t)
    assert len(rects) == 6
    got = sampler(net, *STD, batch_size=len(t), num_steps=3, device=DEV, img_size=HW, cond_img=tiles, seed=5 + (1 << 33),
                  tile_origins=t.origins_dev, domain_width=WP, joint_tiles=(HD, t.overlap), noise_domain_row=14, noise_weights=W3,
                  noise_row_stride=2, **kw)
    assert torch.isfinite(got).all()
    for a, b, wa, wb in rects:
        assert torch.equal(got[a, 0][wa], got[b, 0][wb]), f"{kind}: tiles {a} and {b} differ where they overlap"


def test_joint_zero_score_run_is_the_weighted_sum_of_the_mixed_domain_draws(znet, A):
    t, cond, _ = A
    seed, steps, row, stride = 21 + (3 << 32), 3, 8, 2
    dom = t.sample(znet, S.Euler_Maruyama_sampler, *STD, num_steps=steps, cond_img=cond, seed=seed, joint=True, noise_row=row,
                   noise_weights=W3, noise_row_stride=stride)
    assert dom.shape == (1, HD, WD)
    ones = torch.ones(1, device=DEV)
    ts = torch.linspace(1.0, 1e-3, steps, device=DEV)
    dt = float(ts[0] - ts[1])
    coef = [float(S.marginal_prob_std_fn(ones)[0])] + [math.sqrt(dt) * float(S.diffusion_coeff_fn(ones * tt)[0]) for tt in ts.tolist()[:-1]]
    want = sum(c * mixed_domain(seed, i, row, W3, stride).astype(np.float64) for i, c in enumerate(coef))[:, :WD]
    want = torch.from_numpy(want).view(1, HD, WD).to(DEV)
    err = float((dom.double() - want).abs().max() / want.abs().max())
    print(f"joint run under a domain plan: max |got - want| / max |want| = {err:.2e} over the {HD} x {WD} domain")
    assert err <= 1e-5


# ---- (6) the series --------------------------------------------------------------------------------------------------------------------------
def test_series_is_extensible_and_independent_of_the_batching(net, A):
    t, _, _ = A
    conds = rnd(4, 1, HD, WD, seed=31)
    seed = 20240229 + (1 << 34)
    series = lambda c, **how: t.sample_series(net, S.Euler_Maruyama_sampler, *STD, num_steps=3, cond_img=c, members=2, seed=seed,  # noqa: E731
                                              temporal_noise_weights=W3, **how)
    whole = series(conds)
    assert whole.shape == (4, 2, HD, WD) and whole.dtype == torch.float32 and torch.isfinite(whole).all()
    assert torch.equal(torch.cat([series(conds[:2]), series(conds[2:], first_day=2)]), whole)
    assert torch.equal(series(conds, tiles_per_batch=1), whole)
    assert (whole[:, 0] != whole[:, 1]).float().mean() > 0.99                                    # members differ
    # one day regenerated, jointly: the joint series is another series, and as extensible
    joint = series(conds, joint=True)
    assert torch.equal(series(conds[3:], first_day=3, joint=True), joint[3:]) and not torch.equal(joint, whole)
    # day d, member m is the tiler's sample under row (d + K - 1) M + m, stride M
    one = t.sample(net, S.Euler_Maruyama_sampler, *STD, num_steps=3, cond_img=conds[1], seed=seed, noise_row=(1 + 2) * 2 + 1,
                   noise_weights=W3, noise_row_stride=2)
    assert torch.equal(one[0], whole[1, 1])


def test_series_days_correlate_as_the_weights_say(znet, A):
    t, _, _ = A
    D, M, K = 5, 2, len(W3)
    out = t.sample_series(znet, S.Euler_Maruyama_sampler, *STD, num_steps=3, cond_img=rnd(D, 1, HD, WD, seed=32), members=M, seed=77,
                          temporal_noise_weights=W3)
    n = M * HD * WD
    flat = lambda d: out[d].reshape(-1).double()  # noqa: E731
    corr = lambda a, b: float(torch.corrcoef(torch.stack([a, b]))[0, 1])  # noqa: E731
    acf1 = float(SS.temporal_noise_acf(W3)[1])
    c1 = [corr(flat(d), flat(d + 1)) for d in range(D - 1)]
    cK = [corr(flat(d), flat(d + K)) for d in range(D - K)]
    cm = corr(out[:, 0].reshape(-1).double(), out[:, 1].reshape(-1).double())
    print(f"series: lag-1 correlations {c1} (acf[1] {acf1:.4f}), {K} days apart {cK}, members {cm:.4f}; bound {5 / math.sqrt(n):.4f}")
    assert all(abs(c - acf1) <= 5 / math.sqrt(n) for c in c1)
    assert all(abs(c) <= 5 / math.sqrt(n) for c in cK)                                           # no white row in common
    assert abs(cm) <= 5 / math.sqrt(D * HD * WD)                                                 # members are independent


# ---- (7) refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(net, A):
    t, cond, tiles = A
    T, steps, seed = len(t), 2, 5
    run = lambda **how: S.Euler_Maruyama_sampler(net, *STD, batch_size=T, num_steps=steps, device=DEV, img_size=HW, cond_img=tiles,  # noqa: E731
                                                 seed=seed, **how)
    tiled = dict(tile_origins=t.origins_dev, domain_width=WP)
    before, before_tiled = run(), run(**tiled)
    plan = dict(tiled, noise_domain_row=9, domain_height=HD, noise_weights=W3)
    under = run(**plan)
    for how in (dict(noise_domain_row=9, domain_height=HD), dict(plan, noise=torch.zeros(3, T, 1, HW, HW)), dict(plan, noise_rows=[4, 5, 6, 7]),
                dict(plan, noise_domain_row=1), dict(plan, domain_height=31), dict(tiled, noise_rows=[4, 5, 6, 7], noise_weights=W3)):
        with pytest.raises(ValueError):
            run(**how)
        assert torch.equal(run(), before)
    # the native call reads the tile table: a tile outside the plan's domain is refused (its counters would reach into the next row)
    for how in (dict(plan, domain_height=43), dict(plan, domain_width=52)):
        with pytest.raises(N.NativeError, match="domain"):
            run(**how)
        assert torch.equal(run(**tiled), before_tiled)
    lib = N.lib()
    out1, row1, w1 = torch.empty(1, HW, HW, device=DEV), torch.tensor([9], dtype=torch.int32, device=DEV), (N.C.c_float * 1)(1.0)
    for y0, x0 in ((16, 0), (0, 28), (0, 2), (-1, 0)):                       # the op reads the table as well
        far = torch.tensor([[y0, x0]], dtype=torch.int32, device=DEV)
        assert lib.sbgm_randn_domain_rows(out1.data_ptr(), 1.0, 1, 0, row1.data_ptr(), far.data_ptr(), 1, HW, HW, HD, WP, 1, w1, 1, N.stream()) != 0
        assert b"inside the 44 x 56 domain" in lib.sbgm_last_error()
    # the tiler names its own arguments
    for how, name in ((dict(noise_weights=W3), "noise_row"), (dict(noise_row=1, noise_weights=W3), "noise_row"),
                      (dict(noise_row=9, noise_weights=[0.6, 0.7]), "noise_weights"), (dict(noise_row=9, noise_row_stride=0), "noise_row_stride")):
        with pytest.raises(ValueError, match=name):
            t.sample(net, S.Euler_Maruyama_sampler, *STD, num_steps=steps, cond_img=cond, seed=seed, **how)
    with pytest.raises(ValueError, match="noise_row"):
        t.sample(net, S.rk45_sampler, *STD, num_steps=None, cond_img=cond, seed=seed, noise_row=9)
    for how, name in ((dict(members=0), "members"), (dict(first_day=-1), "first_day"), (dict(cond_img=cond), "cond_img"),
                      (dict(cond_img=None), "days"), (dict(first_day=(1 << 31)), "first_day")):
        with pytest.raises(ValueError, match=name):
            t.sample_series(net, S.Euler_Maruyama_sampler, *STD, num_steps=steps, **dict(dict(cond_img=cond[None]), **how))
    # the engine's own refusals (direct C calls): the plan stays with the handle until cleared, and the row is read from its address
    eng = net._engine(None, None, tiles)
    row = torch.tensor([9], dtype=torch.int32, device=DEV)
    rows = torch.tensor([4, 5, 6, 7], dtype=torch.int32, device=DEV)
    w = (N.C.c_float * 3)(*W3.tolist())
    for bad in ((row.data_ptr(), HD, 1, w, 33), (row.data_ptr(), HD, 0, w, 3), (row.data_ptr(), 0, 1, w, 3), (None, HD, 1, w, 2),
                (row.data_ptr(), HD, 1, None, 3)):
        assert lib.sbgm_sampler_set_noise_domain_row(eng.h, *bad) != 0
    N.check(lib.sbgm_sampler_set_noise_domain_row(eng.h, row.data_ptr(), HD, 1, w, 3))
    try:
        assert lib.sbgm_sampler_set_noise_rows(eng.h, rows.data_ptr(), 1, w, 3) != 0 and b"exclude" in lib.sbgm_last_error()
        with pytest.raises(N.NativeError, match="tile_origins"):
            run()                                                             # a domain row without tiles
        with pytest.raises(N.NativeError, match="injected noise"):
            run(noise=torch.zeros(3, T, 1, HW, HW))
        with pytest.raises(N.NativeError, match="ODE"):
            S.rk45_sampler(net, *STD, batch_size=T, device=DEV, img_size=HW, cond_img=tiles, seed=seed, error_norm="sample", **tiled)
        held_plan = run(**tiled)
        row.fill_(10)                                                         # another day at the same address: no new plan is set
        next_day = run(**tiled)
        row.fill_(1)                                                          # below (K - 1) stride: refused when the run reads it
        with pytest.raises(N.NativeError, match="row"):
            run(**tiled)
    finally:
        N.check(lib.sbgm_sampler_set_noise_domain_row(eng.h, None, 0, 1, None, 0))
    assert torch.equal(held_plan, under) and torch.equal(next_day, run(**dict(plan, noise_domain_row=10))) and not torch.equal(next_day, under)
    N.check(lib.sbgm_sampler_set_noise_rows(eng.h, rows.data_ptr(), 1, w, 3))
    try:
        assert lib.sbgm_sampler_set_noise_domain_row(eng.h, row.data_ptr(), HD, 1, w, 3) != 0 and b"exclude" in lib.sbgm_last_error()
        with pytest.raises(N.NativeError, match="tile_origins"):              # a rows plan with tiles stays refused
            run(**tiled)
    finally:
        N.check(lib.sbgm_sampler_set_noise_rows(eng.h, None, 1, None, 0))
    assert torch.equal(run(), before) and torch.equal(run(**tiled), before_tiled)
