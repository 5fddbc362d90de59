"""dpmpp_2m_sampler on the GPU (DPM-Solver++(2M), eta > 0: 2M SDE): the native loop (one captured step, evaluation + update, replayed N
times) and the Python loop (the update op around any score callable) against the host restatement of dpmpp_ref.py around the oracle
network; an analytic Gaussian score for the solver's order and the stochastic variant's spread; the history that must not be read on
the first step; graph replay against eager launches and the step-graph key; held pixels; joint tiles; the time rows; the CLI wiring.

Measured on MI355X (printed by the tests): see DESIGN.md 4.6."""
import math
import os

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu

from oracle import torch_ref as O  # noqa: E402
from util_models import build_pair, check_parity, maxrel  # noqa: E402

import constrained_ref as R  # noqa: E402
import dpmpp_ref as D  # noqa: E402
import joint_tiles_ref as J  # noqa: E402
import sbgm_danra_amd as S  # noqa: E402
from sbgm_danra_amd import _native as N  # noqa: E402
from sbgm_danra_amd import score_sampling as SS  # noqa: E402
from sbgm_danra_amd.tiling import FullDomainTiler  # noqa: E402
from util_step_runs import run_specs  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIG = 25.0
GUIDED = {"classifier_free_guidance": {"enabled": True, "guidance_scale": 2.5, "guidance_scale_max": 1.5}}
STD = (S.marginal_prob_std_fn, S.diffusion_coeff_fn)


@pytest.fixture(scope="module")
def pair():
    ora, net, _ = build_pair(1)
    return ora.eval(), net.eval()


def device_draw(seed, draw, shape):
    x = torch.empty(shape, device="cuda")
    N.check(N.lib().sbgm_randn_scaled(x.data_ptr(), 1.0, seed, draw, x.numel(), N.stream()))
    return x


# ---- 1. parity with the oracle network --------------------------------------------------------------------------------------
@pytest.mark.parametrize("eta", [0.0, 1.0])
def test_native_loop_matches_oracle_restatement(pair, eta):
    ora, net = pair
    g = torch.Generator().manual_seed(5)
    cond = torch.randn(2, 1, 64, 64, generator=g)
    noise = torch.randn(6, 2, 1, 64, 64, generator=g)
    with torch.no_grad():
        want = D.dpm_restatement(lambda x, t: ora(x, t, cond_img=cond), noise, 5, eta=eta)
        got = S.dpmpp_2m_sampler(net, *STD, batch_size=2, num_steps=5, device="cuda", img_size=64, cond_img=cond.cuda(), noise=noise,
                                 eta=eta)
    assert got.shape == (2, 1, 64, 64)
    check_parity(got.cpu(), want, 1e-4, f"dpmpp 2m N=5 eta={eta:g} vs oracle")


def test_guided_native_loop_matches_oracle_restatement():
    ora, net, _ = build_pair(1, 4)
    ora.eval(), net.eval()
    g = torch.Generator().manual_seed(6)
    cond = torch.randn(2, 1, 32, 32, generator=g)
    y = torch.tensor([1, 3])
    noise = torch.randn(5, 2, 1, 32, 32, generator=g)
    w = GUIDED["classifier_free_guidance"]["guidance_scale"]            # guidance_scale_max does not apply
    with torch.no_grad():
        want = D.dpm_restatement(lambda x, t: O.guided_score_fn(ora, x, t, y, cond, scale=w), noise, 4, eta=1.0)
        got = S.dpmpp_2m_sampler(net, *STD, batch_size=2, num_steps=4, device="cuda", img_size=32, y=y.cuda(), cond_img=cond.cuda(),
                                 cfg=GUIDED, noise=noise, eta=1.0)
    check_parity(got.cpu(), want, 1e-4, "guided dpmpp 2m N=4 vs oracle")


# ---- 2. analytic score: Gaussian data of variance s0^2, through the Python loop (the op kernel) ------------------------------------
@pytest.mark.parametrize("s0", [0.5, 1.0, 2.0])
def test_analytic_score_solver_order(s0):
    g = torch.Generator().manual_seed(int(s0 * 10))
    f = R.gaussian_score(s0)
    calls = [0]

    def counted(*a):
        calls[0] += 1
        return f(*a)
    err = {}
    for n in (8, 16, 32):
        noise = torch.randn(1, 4, 1, 16, 16, generator=g)
        calls[0] = 0
        got = S.dpmpp_2m_sampler(counted, *STD, batch_size=4, num_steps=n, device="cuda", img_size=16, noise=noise).cpu().double()
        assert calls[0] == n                                            # one evaluation per step
        sch = SS.dpmpp_2m_schedule(n, SIG)
        x0 = (noise[0] * float(np.float32(sch["sigma"][0]))).double()
        host = D.dpm_restatement(f, noise, n, dtype=torch.float64, x_init=x0)
        print(f"s0={s0} N={n}: device vs float64 host recurrence max-rel {maxrel(got, host):.2e}")
        assert maxrel(got, host) <= 2e-5, (s0, n, maxrel(got, host))
        err[n] = maxrel(got, D.gaussian_exact(x0, s0, sch))
    print(f"s0={s0}: error against the exact solution {err}")
    assert err[8] > err[16] > err[32]
    assert err[16] / err[32] >= 3.6, err                                # second order: the error falls ~4x per doubling


# ---- 3. the op: the history is not read when c_1 == 0 ---------------------------------------------------------------------------------
def test_step_op_does_not_read_the_history_without_a_second_order_term():
    g = torch.Generator().manual_seed(7)
    n = 4 * 1031                                                        # more than one block, no multiple of the block size
    x0, s, h0 = (torch.randn(n, generator=g) for _ in range(3))
    sigma, c_x, c_0, c_1 = (float(np.float32(v)) for v in (3.7, 0.55, 0.71, -0.26))

    def step(hist, c1, z=None, c_z=0.0):
        x, sc = x0.cuda(), s.cuda()
        N.check(N.lib().sbgm_dpmpp_2m_step(x.data_ptr(), sc.data_ptr(), hist.data_ptr(), N.ptr(z), sigma, c_x, c_0, c1, c_z, 3, 1, n,
                                           N.stream()))
        return x.cpu()
    d = x0 + (sigma * sigma) * s
    hist = torch.full((n,), float("nan"), device="cuda")
    got = step(hist, 0.0)
    assert torch.isfinite(got).all() and maxrel(got, c_x * x0 + c_0 * d) <= 1e-6
    assert torch.isfinite(hist).all() and maxrel(hist.cpu(), d) <= 1e-6       # the history now holds D
    hist = h0.cuda()
    assert maxrel(step(hist, c_1), c_x * x0 + c_0 * d + c_1 * h0) <= 1e-6
    assert maxrel(hist.cpu(), d) <= 1e-6
    z = torch.randn(n, generator=g)
    hist = h0.cuda()
    assert maxrel(step(hist, c_1, z.cuda(), 0.4), c_x * x0 + c_0 * d + c_1 * h0 + float(np.float32(0.4)) * z) <= 1e-6
    hist = h0.cuda()                                                    # z NULL, c_z != 0: the Philox draw (seed 3, draw 1)
    assert maxrel(step(hist, c_1, None, 0.4), c_x * x0 + c_0 * d + c_1 * h0 + float(np.float32(0.4)) * device_draw(3, 1, (n,)).cpu()) <= 1e-6


# ---- 4. Python loop == native loop; seeded == injected draws --------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(eta=0.0), dict(eta=0.7), dict(eta=0.7, sigma_min=0.002, sigma_max=80.0, rho=5.0, s_noise=1.003)])
def test_python_loop_equals_native_loop(pair, kw):
    net = pair[1]
    g = torch.Generator().manual_seed(3)
    cond = torch.randn(2, 1, 32, 32, generator=g).cuda()
    noise = torch.randn(7, 2, 1, 32, 32, generator=g)
    f = lambda x, t, y=None, c=None, l=None, tp=None: net(x, t, y, c, l, tp)  # noqa: E731  (a plain callable, not a ScoreNet)
    run = lambda m, **how: S.dpmpp_2m_sampler(m, *STD, batch_size=2, num_steps=6, device="cuda", img_size=32, cond_img=cond,  # noqa: E731
                                              **kw, **how)
    a, b = run(net, noise=noise), run(f, noise=noise)
    assert torch.isfinite(a).all()
    assert maxrel(a.cpu(), b.cpu()) <= 1e-4
    assert maxrel(run(net, seed=17).cpu(), run(f, seed=17).cpu()) <= 1e-4    # the same Philox numbers at the same draw indices
    with pytest.raises(N.NativeError):                                  # the Python loop has no tiles
        run(f, seed=17, tile_origins=torch.zeros(2, 2, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):                                     # one draw too few
        run(net, noise=noise[:6] if kw["eta"] > 0 else noise[:0])


@pytest.mark.parametrize("held", [False, True])
@pytest.mark.parametrize("eta", [0.0, 0.7])
def test_seeded_run_equals_the_run_on_injected_device_draws(pair, eta, held):
    net = pair[1]
    B, hw, steps, seed = 2, 32, 4, 1234 + (7 << 32)
    need = SS._counts(N.SAMPLER_DPMPP_2M, steps, eta > 0)[1]
    assert need == (5 if eta > 0 else 1)
    g = torch.Generator().manual_seed(11)
    cond = torch.randn(B, 1, hw, hw, generator=g).cuda()
    kw = dict(eta=eta)
    if held:                                                            # eta = 0: ties the recomputed draw 0 of the hold to draw 0
        kw.update(known=torch.randn(B, 1, hw, hw, generator=g).cuda(), known_mask=R.standard_mask(B, hw).cuda())
    run = lambda **how: S.dpmpp_2m_sampler(net, *STD, batch_size=B, num_steps=steps, device="cuda", img_size=hw, cond_img=cond,  # noqa: E731
                                           **kw, **how)
    draws = torch.stack([device_draw(seed, i, (B, 1, hw, hw)) for i in range(need)])
    want = run(noise=draws)
    assert torch.isfinite(want).all()
    for graph in (True, False):
        assert torch.equal(run(seed=seed, use_graph=graph), want), (eta, held, graph)
    if need > 2:
        assert not torch.equal(run(noise=draws[[0, 2, 1] + list(range(3, need))]), want)


# ---- 5. graph replay == eager, seeds, no graph shared ---------------------------------------------------------------------------------
@pytest.mark.parametrize("eta", [0.0, 1.0])
def test_graph_replay_equals_eager_bit_for_bit(pair, eta):
    net = pair[1]
    cond = torch.randn(2, 1, 64, 64, generator=torch.Generator().manual_seed(4)).cuda()
    kw = dict(batch_size=2, num_steps=6, device="cuda", img_size=64, cond_img=cond)
    dpm = lambda seed, graph, model=net, e=eta: S.dpmpp_2m_sampler(model, *STD, seed=seed, use_graph=graph, eta=e, **kw)  # noqa: E731
    a, b, a2 = dpm(77, True), dpm(77, False), dpm(77, True)
    assert torch.isfinite(a).all()
    assert torch.equal(a, b) and torch.equal(a, a2)
    assert not torch.equal(a, dpm(78, True))
    # directly after an EDM Heun run, and after a run of the other eta-mode, on the same handle: the fresh-handle result
    fresh = build_pair(1)[1].eval()
    want, want_other = dpm(77, True, fresh), dpm(77, True, build_pair(1)[1].eval(), 1.0 - eta)
    assert torch.equal(want, a)
    heun = S.edm_heun_sampler(net, *STD, seed=77, **kw)
    assert torch.equal(dpm(77, True), a)
    assert torch.equal(dpm(77, True, net, 1.0 - eta), want_other)
    assert torch.equal(dpm(77, True), a)
    assert torch.equal(S.edm_heun_sampler(net, *STD, seed=77, **kw), heun)
    assert not torch.equal(a, want_other) and not torch.equal(a, heun)


# ---- 6. constrained ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eta", [0.0, 1.0])
def test_held_pixels(pair, eta):
    ora, net = pair
    g = torch.Generator().manual_seed(11)
    cond, noise, known = torch.randn(2, 1, 32, 32, generator=g), torch.randn(6, 2, 1, 32, 32, generator=g), torch.randn(2, 1, 32, 32, generator=g)
    mask = R.standard_mask(2, 32)                                       # hard blocks plus a soft edge
    with torch.no_grad():
        want = D.dpm_restatement(lambda x, t: ora(x, t, cond_img=cond), noise, 5, known=known, mask=mask, eta=eta)
        got = S.dpmpp_2m_sampler(net, *STD, batch_size=2, num_steps=5, device="cuda", img_size=32, cond_img=cond.cuda(), noise=noise,
                                 known=known, known_mask=mask, eta=eta).cpu()
    assert torch.equal(got[mask == 1], known[mask == 1])
    check_parity(got, want, 1e-4, f"constrained dpmpp 2m N=5 eta={eta:g} vs oracle")
    # an all-zero mask: the run without the arguments, bit for bit, with NaN in `known`
    run = lambda graph=True, **kw: S.dpmpp_2m_sampler(net, *STD, batch_size=2, num_steps=5, device="cuda", img_size=32,  # noqa: E731
                                                      cond_img=cond.cuda(), seed=5, use_graph=graph, eta=eta, **kw)
    free = run()
    nan = torch.full((2, 1, 32, 32), float("nan"))
    for graph in (True, False):
        assert torch.equal(run(graph, known=nan, known_mask=torch.zeros(2, 1, 32, 32)), free)
    held = run(known=known, known_mask=mask)                            # in-kernel noise: exact on the mask, replay == eager
    on = (mask == 1).cuda()
    assert torch.isfinite(held).all() and torch.equal(held[on], known.cuda()[on]) and not torch.equal(held[~on], free[~on])
    assert torch.equal(run(False, known=known, known_mask=mask), held)
    f = lambda x, t, y=None, c=None, l=None, tp=None: net(x, t, y, c, l, tp)  # noqa: E731
    py = S.dpmpp_2m_sampler(f, *STD, batch_size=2, num_steps=5, device="cuda", img_size=32, cond_img=cond.cuda(), seed=5, eta=eta,
                            known=known, known_mask=mask)
    assert torch.equal(py[on], known.cuda()[on]) and maxrel(py.cpu(), held.cpu()) <= 1e-4


# ---- 7. joint tiles -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eta", [0.0, 1.0])
def test_joint_tiles(pair, eta):
    ora, net = pair
    t, geo = FullDomainTiler((32, 48), 32, 8), J.Geometry((32, 48), 32, 8)
    assert len(t) == 2 and t.origins == geo.origins and t.overlap == 16
    seed = 77 + (5 << 32)
    cond = torch.randn(1, 32, 48, generator=torch.Generator().manual_seed(4)).cuda()
    tiles = t.extract(cond)
    run = lambda **kw: S.dpmpp_2m_sampler(net, *STD, batch_size=2, num_steps=4, device="cuda", img_size=32, seed=seed,  # noqa: E731
                                          cond_img=tiles, tile_origins=t.origins_dev, domain_width=t.Wd_pad, eta=eta, **kw)
    got = run(joint_tiles=(t.Hd, t.overlap))
    assert torch.isfinite(got).all()
    (y0, x0), (y1, x1) = t.origins
    assert y0 == y1 and x1 - x0 == 16
    assert torch.equal(got[0, 0][:, 16:], got[1, 0][:, :16])            # every copy of a domain pixel
    plain = run()
    assert not torch.equal(plain[0, 0][:, 16:], plain[1, 0][:, :16])    # not vacuous
    assert torch.equal(run(joint_tiles=(t.Hd, t.overlap), use_graph=False), got)
    cond_h = tiles.cpu()
    with torch.no_grad():
        want = D.dpm_joint(lambda x, tt: ora(x, tt, cond_img=cond_h), seed, 4, geo, eta=eta)
    check_parity(t.stitch(got).cpu(), want, 1e-4, f"joint dpmpp 2m 32x48 N=4 eta={eta:g} vs restatement")
    dom = t.sample(net, S.dpmpp_2m_sampler, *STD, num_steps=4, cond_img=cond, seed=seed, joint=True, eta=eta)
    assert dom.shape == (1, 32, 48) and torch.equal(dom, t.stitch(got))
    tiled = t.sample(net, S.dpmpp_2m_sampler, *STD, num_steps=4, cond_img=cond, seed=seed, eta=eta)
    assert tiled.shape == (1, 32, 48) and torch.isfinite(tiled).all() and torch.equal(tiled, t.stitch(plain))


# ---- 8. the stochastic variant's spread -----------------------------------------------------------------------------------------------
def spread_target(s0):
    smin = SS.dpmpp_2m_schedule(32, SIG)["sigma_min"]
    return s0 ** 2 / math.sqrt(s0 ** 2 + smin ** 2)                     # x_N = D_{N-1} = x s0^2 / (s0^2 + smin^2), x ~ N(0, s0^2 + smin^2)


@pytest.mark.parametrize("s0", [0.5, 1.0, 2.0])
@pytest.mark.parametrize("eta", [0.5, 1.0])
def test_stochastic_spread_on_the_device(eta, s0):
    got = S.dpmpp_2m_sampler(R.gaussian_score(s0), *STD, batch_size=4, num_steps=32, device="cuda", img_size=64, seed=int(100 * eta + s0),
                             eta=eta)
    std = float(got.double().std())
    print(f"eta={eta} s0={s0}: sample std {std:.5f}, target {spread_target(s0):.5f} ({std / spread_target(s0) - 1:+.2%})")
    assert abs(std / spread_target(s0) - 1.0) <= 0.04


class SeededDraws:
    """noise[i] of a host run, drawn when it is asked for (33 draws of 480 x 64 x 64 float64 values are not kept at once)"""

    def __init__(self, seed, shape):
        self.seed, self.shape = seed, shape

    def __getitem__(self, i):
        return torch.randn(self.shape, generator=torch.Generator().manual_seed(self.seed * 64 + i), dtype=torch.float64)


@pytest.mark.parametrize("s0", [0.5, 1.0, 2.0])
@pytest.mark.parametrize("eta", [0.5, 1.0])
def test_stochastic_spread_of_the_host_recurrence(eta, s0):
    """120 seeded runs of B = 4 at 64 x 64 as one float64 batch of 480 samples.  The bound is on the recurrence's own bias, the standard
    deviation over the values of all 120 runs (the scatter of one run's 16384 values, 1 / sqrt(2 * 16384) = 0.55 %, comes on top of it
    and is what the 4 % of the device test leaves room for); a single run's deviation is printed."""
    noise = SeededDraws(int(1000 * eta + 10 * s0), (480, 1, 64, 64))
    f = D.gaussian_score_f64(s0)
    got = D.dpm_restatement(f, noise, 32, dtype=torch.float64, eta=eta)
    per_run = got.reshape(120, -1).std(dim=1) / spread_target(s0) - 1.0
    dev = float(got.std()) / spread_target(s0) - 1.0
    print(f"eta={eta} s0={s0}: host recurrence, 120 runs: sample std off by {dev:+.2%} (single runs {float(per_run.min()):+.2%} .. "
          f"{float(per_run.max()):+.2%})")
    assert abs(dev) <= 0.018
    off = float(D.dpm_restatement(f, noise, 32, dtype=torch.float64, eta=eta, drop_noise=True).std()) / spread_target(s0) - 1.0
    print(f"  without the noise term: {off:+.2%}")
    assert abs(off) > 0.55


# ---- 9. the time rows ------------------------------------------------------------------------------------------------------------------
SWITCHED = [
    dict(name="plain", B=2, N=5),
    dict(name="n2", B=2, N=2),                                          # the last (second) step clamps its row index
    dict(name="sde", B=2, N=4, eta=1.0),
    dict(name="guided", B=2, N=3, guided=True),                         # 2B rows are broadcast
    dict(name="held", B=2, N=3, held=True),
    dict(name="held_sde", B=2, N=3, held=True, eta=1.0),
    dict(name="joint", B=2, N=3, joint=True),
    dict(name="labels", B=2, N=3, classes=4, labels=True),              # labels: the route is off, both sides keep their launches
]
EXTRA = [dict(name="plain_eager", B=2, N=5, graph=False), dict(name="plain_n7", B=2, N=7), dict(name="plain_again", B=2, N=5)]


@pytest.fixture(scope="module")
def row_runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("dpmpp_time_rows")
    return {"rows": run_specs(SWITCHED + EXTRA, {}, d / "rows.npz"),
            "off": run_specs(SWITCHED, {"SBGM_NO_TIME_ROWS": "1"}, d / "off.npz")}


@pytest.mark.parametrize("name", [s["name"] for s in SWITCHED])
def test_run_with_time_rows_equals_the_per_step_launches(row_runs, name):
    got, want = row_runs["rows"][name], row_runs["off"][name]
    assert np.isfinite(got).all() and got.shape == want.shape
    assert np.array_equal(got, want), f"{name}: max |diff| {np.abs(got - want).max():.3e}"


def test_time_rows_are_rebuilt_on_every_call(row_runs):
    r = row_runs["rows"]
    assert np.array_equal(r["plain"], r["plain_eager"]) and np.array_equal(r["plain"], r["plain_again"])
    assert not np.array_equal(r["plain"], r["plain_n7"])


# ---- 10. CLI generation and the training preview --------------------------------------------------------------------------------------
@pytest.fixture()
def cfg_path(tmp_path, monkeypatch):
    for k in ("DATA_DIR", "CKPT_DIR", "SAMPLE_DIR", "STATS_LOAD_DIR"):
        monkeypatch.setenv(k, str(tmp_path / k.lower()))
    monkeypatch.setenv("SLURM_CPUS_PER_TASK", "2")
    raw = yaml.safe_load(open(os.path.join(ROOT, "sbgm_danra_amd", "config", "default_config.yaml")))
    raw["highres"]["data_size"] = [64, 64]
    raw["lowres"]["data_size"] = [64, 64]
    raw["lowres"]["condition_variables"] = ["temp", "prcp"]
    raw["stationary_conditions"]["geographic_conditions"]["sample_w_geo"] = True
    raw["stationary_conditions"]["seasonal_conditions"]["sample_w_cond_season"] = True
    raw["sampler"]["sampler_type"] = "dpmpp_2m_sampler"
    raw["sampler"]["n_timesteps"] = 6
    raw["dpm"] = {"sigma_min": 0.002, "sigma_max": 80, "rho": 7, "eta": 0.5}
    raw["constraint"] = {"enabled": True, "station_fraction": 0.05, "seed": 3}
    raw["evaluation"].update(batch_size=3, gen_type=["multiple", "single", "repeated"], n_repeats=2, transform_back=False)
    raw["training"]["batch_size"] = 2
    p = tmp_path / "run.yaml"
    p.write_text(yaml.safe_dump(raw))
    return str(p)


def test_cli_generate_and_training_preview_with_dpmpp_2m(cfg_path):
    from sbgm.cli import main_app
    from sbgm.score_unet import diffusion_coeff_fn, loss_fn, marginal_prob_std_fn
    from sbgm.training import TrainingPipeline_general
    from sbgm.training_utils import get_dataloader, get_model, get_optimizer
    from sbgm.utils import get_model_string, load_config
    cfg = load_config(cfg_path)
    ora = O.build_scorenet(6, num_classes=4)
    ckpt_dir = os.path.join(cfg.paths.path_save, cfg.paths.checkpoint_dir)
    os.makedirs(ckpt_dir, exist_ok=True)
    torch.save({"network_params": O.synth_state_dict(ora), "optimizer_params": {}}, os.path.join(ckpt_dir, get_model_string(cfg) + ".pth.tar"))
    main_app.main(["--config_path", cfg_path, "--mode", "generate"])
    out = os.path.join(cfg.paths.sample_dir, "generation", get_model_string(cfg), "generated_samples")
    load = lambda name: np.load(os.path.join(out, name))["arr_0"]  # noqa: E731
    for suffix, n in (("multi_n_3", 3), ("single", 1), ("repeated_n_2", 2)):
        gen, truth, mask = load(f"gen_samples_{suffix}.npz"), load(f"eval_samples_{suffix}.npz"), load(f"constraint_mask_{suffix}.npz")
        assert gen.shape == (n, 64, 64) and np.isfinite(gen).all(), suffix
        truth = np.broadcast_to(truth.reshape(-1, 64, 64), gen.shape)
        on = np.broadcast_to(mask == 1, gen.shape)
        assert on.any() and np.array_equal(gen[on], truth[on]), suffix      # the constraint: section is honoured
        assert not np.array_equal(gen[~on], truth[~on]), suffix
    torch.manual_seed(0)
    model, _, _ = get_model(cfg)
    pipe = TrainingPipeline_general(model, loss_fn, marginal_prob_std_fn, diffusion_coeff_fn, get_optimizer(cfg, model),
                                    torch.device("cuda"), None, cfg)
    _, _, gen_dl = get_dataloader(cfg)
    gen = pipe.generate_and_plot_samples(gen_dl, cfg=cfg, epoch=1)
    assert gen.dim() == 4 and gen.shape[1:] == (1, 64, 64) and torch.isfinite(gen).all()
