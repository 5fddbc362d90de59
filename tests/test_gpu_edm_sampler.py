"""EDM Heun sampler on the GPU: the native loop (one captured Heun step replayed N-1 times + an eager final Euler step) and the
Python loop (per-op churn / euler / heun kernels around any score callable) against a float32 CPU restatement around the
oracle network, an analytic Gaussian score that proves the solver's order, graph replay against eager launches, domain-keyed
noise on tiles, and the CLI / training-preview wiring of `sampler_type: edm_heun_sampler`."""
import math
import os

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu

from oracle import torch_ref as O  # noqa: E402
from util_models import build_pair, check_parity, maxrel  # noqa: E402

import sbgm_danra_amd as S  # noqa: E402
from sbgm_danra_amd import score_sampling as SS  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIG = 25.0
GUIDED = {"classifier_free_guidance": {"enabled": True, "guidance_scale": 2.5, "guidance_scale_max": 1.5}}


def heun_restatement(score, noise, n_steps, dtype=torch.float32, x_init=None, **sched):
    """the Heun recurrence of score_sampling.edm_heun_sampler written out on the host: `score(x, t)` gets fp32 times, the
    step scalars are rounded to `dtype`; the run starts from sigma_0 * noise[0], or from `x_init`"""
    sch = SS.edm_heun_schedule(n_steps, SIG, 1e-3, **sched)
    c = (lambda v: float(np.float32(v))) if dtype == torch.float32 else float
    B = noise[0].shape[0]
    x = noise[0].to(dtype) * c(sch["sigma"][0]) if x_init is None else x_init.to(dtype)
    for i in range(n_steps):
        sh, sn = c(sch["sigma_hat"][i]), c(sch["sigma"][i + 1])
        if sch["draws"] > 1:
            x = x + c(sch["churn_coef"][i]) * noise[1 + i].to(dtype)
        d = -sh * score(x, torch.full((B,), float(np.float32(sch["t_hat"][i]))))
        xp = x + (sn - sh) * d
        if i == n_steps - 1:
            return xp
        d2 = -sn * score(xp, torch.full((B,), float(np.float32(sch["t_next"][i]))))
        x = x + (sn - sh) * 0.5 * (d + d2)


# ---- 1. parity with the oracle network --------------------------------------------------------------------------------------
@pytest.mark.parametrize("s_churn", [0.0, 40.0])
def test_native_loop_matches_oracle_restatement(s_churn):
    ora, net, _ = build_pair(1)
    ora.eval(), net.eval()
    g = torch.Generator().manual_seed(5)
    cond = torch.randn(2, 1, 64, 64, generator=g)
    noise = torch.randn(6, 2, 1, 64, 64, generator=g)
    with torch.no_grad():
        want = heun_restatement(lambda x, t: ora(x, t, cond_img=cond), noise, 5, s_churn=s_churn)
        got = S.edm_heun_sampler(net, S.marginal_prob_std_fn, S.diffusion_coeff_fn, batch_size=2, num_steps=5, device="cuda",
                                 img_size=64, cond_img=cond.cuda(), noise=noise, s_churn=s_churn)
    assert got.shape == (2, 1, 64, 64)
    check_parity(got.cpu(), want, 1e-4, f"edm heun N=5 churn={s_churn:g} vs oracle")


def test_guided_native_loop_matches_oracle_restatement():
    ora, net, _ = build_pair(1, 4)
    ora.eval(), net.eval()
    g = torch.Generator().manual_seed(6)
    cond = torch.randn(2, 1, 32, 32, generator=g)
    y = torch.tensor([1, 3])
    noise = torch.randn(5, 2, 1, 32, 32, generator=g)
    w = GUIDED["classifier_free_guidance"]["guidance_scale"]            # both evaluations; guidance_scale_max does not apply
    with torch.no_grad():
        want = heun_restatement(lambda x, t: O.guided_score_fn(ora, x, t, y, cond, scale=w), noise, 4, s_churn=20.0)
        got = S.edm_heun_sampler(net, S.marginal_prob_std_fn, S.diffusion_coeff_fn, batch_size=2, num_steps=4, device="cuda",
                                 img_size=32, y=y.cuda(), cond_img=cond.cuda(), cfg=GUIDED, noise=noise, s_churn=20.0)
    check_parity(got.cpu(), want, 1e-4, "guided edm heun N=4 vs oracle")


# ---- 2. analytic score: Gaussian data of variance s0^2 --------------------------------------------------------------------------
def gaussian_score(s0):
    def f(x, t, y=None, c=None, l=None, tp=None):
        std = SS._ve_std(t.double().cpu().numpy(), SIG)
        var = torch.as_tensor(s0 ** 2 + std ** 2, device=x.device).view(-1, 1, 1, 1)
        return (-x.double() / var).to(x.dtype)
    return f


@pytest.mark.parametrize("s0", [0.5, 1.0, 2.0])
def test_analytic_score_solver_order(s0):
    g = torch.Generator().manual_seed(int(s0 * 10))
    err = {}
    for n in (8, 16, 32):
        noise = torch.randn(1, 4, 1, 16, 16, generator=g)
        got = S.edm_heun_sampler(gaussian_score(s0), S.marginal_prob_std_fn, S.diffusion_coeff_fn, batch_size=4, num_steps=n,
                                 device="cuda", img_size=16, noise=noise).cpu().double()
        x0 = (noise[0] * float(np.float32(SS.edm_heun_schedule(n, SIG)["sigma"][0]))).double()
        host = heun_restatement(gaussian_score(s0), noise, n, dtype=torch.float64, x_init=x0)
        assert maxrel(got, host) <= 2e-5, (s0, n, maxrel(got, host))
        sch = SS.edm_heun_schedule(n, SIG)
        smin, smax = sch["sigma_min"], sch["sigma_max"]
        exact = x0 * math.sqrt((s0 ** 2 + smin ** 2) / (s0 ** 2 + smax ** 2)) * s0 ** 2 / (s0 ** 2 + smin ** 2)
        err[n] = maxrel(got, exact)
    assert err[8] > err[16] > err[32]
    assert err[16] / err[32] >= 3.6, err                                # second order: the error falls ~4x per doubling


# ---- 3. native loop == Python loop -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(s_churn=0.0), dict(s_churn=30.0, s_tmin=0.05, s_tmax=5.0, s_noise=1.003),
                                dict(sigma_min=0.002, sigma_max=80.0, rho=5.0)])
def test_python_loop_equals_native_loop(kw):
    _, net, _ = build_pair(1)
    net.eval()
    g = torch.Generator().manual_seed(3)
    cond = torch.randn(2, 1, 32, 32, generator=g).cuda()
    noise = torch.randn(7, 2, 1, 32, 32, generator=g)
    f = lambda x, t, y=None, c=None, l=None, tp=None: net(x, t, y, c, l, tp)  # noqa: E731  (a plain callable, not a ScoreNet)
    run = lambda m: S.edm_heun_sampler(m, S.marginal_prob_std_fn, S.diffusion_coeff_fn, batch_size=2, num_steps=6,  # noqa: E731
                                       device="cuda", img_size=32, cond_img=cond, noise=noise, **kw)
    a, b = run(net), run(f)
    assert torch.isfinite(a).all()
    assert maxrel(a.cpu(), b.cpu()) <= 1e-4
    # in-kernel noise: the two loops draw the same Philox numbers at the same draw indices
    run2 = lambda m: S.edm_heun_sampler(m, S.marginal_prob_std_fn, S.diffusion_coeff_fn, batch_size=2, num_steps=6,  # noqa: E731
                                        device="cuda", img_size=32, cond_img=cond, seed=17, **kw)
    assert maxrel(run2(net).cpu(), run2(f).cpu()) <= 1e-4


# ---- 4. graph replay == eager, seeds, no graph shared between kinds ----------------------------------------------------------
@pytest.mark.parametrize("B,hw,n,s_churn", [(2, 64, 6, 0.0), (2, 64, 6, 25.0), (32, 128, 32, 0.0)])
def test_graph_replay_equals_eager_bit_for_bit(B, hw, n, s_churn):
    _, net, _ = build_pair(1)
    net.eval()
    cond = torch.randn(B, 1, hw, hw, generator=torch.Generator().manual_seed(4)).cuda()
    kw = dict(batch_size=B, num_steps=n, device="cuda", img_size=hw, cond_img=cond)
    edm = lambda seed, graph: S.edm_heun_sampler(net, S.marginal_prob_std_fn, S.diffusion_coeff_fn, seed=seed,  # noqa: E731
                                                 use_graph=graph, s_churn=s_churn, **kw)
    a, b, a2 = edm(77, True), edm(77, False), edm(77, True)
    assert torch.isfinite(a).all()
    assert torch.equal(a, b) and torch.equal(a, a2)
    assert not torch.equal(a, edm(78, True))
    # the EM / PC step graphs are their own: each still equals its eager run after (and before) an EDM capture
    kw_sde = dict(kw, num_steps=4, seed=5)
    for fn in (S.Euler_Maruyama_sampler, S.pc_sampler):
        g1 = fn(net, S.marginal_prob_std_fn, S.diffusion_coeff_fn, use_graph=True, **kw_sde)
        e1 = fn(net, S.marginal_prob_std_fn, S.diffusion_coeff_fn, use_graph=False, **kw_sde)
        assert torch.equal(g1, e1)
    assert torch.equal(edm(77, True), a)


# ---- 5. tiles ----------------------------------------------------------------------------------------------------------------------
def test_domain_keyed_noise_on_tiles():
    from sbgm_danra_amd.tiling import FullDomainTiler
    _, net, _ = build_pair(1)
    net.eval()
    t = FullDomainTiler((150, 172), 64, 8)
    cond = torch.randn(1, 150, 172, generator=torch.Generator().manual_seed(9)).cuda()
    tiles = t.extract(cond)
    kw = dict(num_steps=4, device="cuda", img_size=64, seed=21, domain_width=t.Wd_pad, s_churn=10.0)
    run = lambda idx: S.edm_heun_sampler(net, S.marginal_prob_std_fn, S.diffusion_coeff_fn, batch_size=len(idx),  # noqa: E731
                                         cond_img=tiles[idx], tile_origins=t.origins_dev[idx].contiguous(), **kw)
    full = run(list(range(len(t))))
    perm = list(range(len(t)))[::-1]
    assert maxrel(run(perm).flip(0).cpu(), full.cpu()) <= 1e-6
    a = S.edm_heun_sampler(net, S.marginal_prob_std_fn, S.diffusion_coeff_fn, batch_size=1, cond_img=tiles[:1],
                           tile_origins=t.origins_dev[:1].contiguous(), **kw)
    b = S.edm_heun_sampler(net, S.marginal_prob_std_fn, S.diffusion_coeff_fn, batch_size=1, cond_img=tiles[:1],
                           tile_origins=t.origins_dev[1:2].contiguous(), **kw)
    assert not torch.equal(a, b)
    with pytest.raises(S._native.NativeError):                          # domain-keyed noise needs the native loop
        S.edm_heun_sampler(lambda *a_: a_[0], S.marginal_prob_std_fn, S.diffusion_coeff_fn, batch_size=1, cond_img=tiles[:1],
                           tile_origins=t.origins_dev[:1].contiguous(), **kw)
    dom = t.sample(net, S.edm_heun_sampler, S.marginal_prob_std_fn, S.diffusion_coeff_fn, num_steps=4, cond_img=cond, seed=21,
                   tiles_per_batch=4)
    assert dom.shape == (1, 150, 172) and torch.isfinite(dom).all()
    dom2 = t.sample(net, S.edm_heun_sampler, S.marginal_prob_std_fn, S.diffusion_coeff_fn, num_steps=4, cond_img=cond, seed=21,
                    tiles_per_batch=4)
    assert torch.equal(dom, dom2)


# ---- 6. CLI generation and the training preview ----------------------------------------------------------------------------------
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
    raw["sampler"]["sampler_type"] = "edm_heun_sampler"
    raw["sampler"]["n_timesteps"] = 6
    raw["edm"] = {"enabled": True, "sigma_min": 0.002, "sigma_max": 80, "rho": 7}
    raw["evaluation"].update(batch_size=3, gen_type=["multiple", "single", "repeated"], n_repeats=2)
    raw["training"]["batch_size"] = 2
    p = tmp_path / "run.yaml"
    p.write_text(yaml.safe_dump(raw))
    return str(p)


def test_cli_generate_and_training_preview_with_edm_heun(cfg_path):
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
    shapes = {"gen_samples_multi_n_3.npz": (3, 64, 64), "gen_samples_single.npz": (1, 64, 64), "gen_samples_repeated_n_2.npz": (2, 64, 64)}
    for name, shape in shapes.items():
        g = np.load(os.path.join(out, name))["arr_0"]
        assert g.shape == shape and np.isfinite(g).all(), name
    torch.manual_seed(0)
    model, _, _ = get_model(cfg)
    pipe = TrainingPipeline_general(model, loss_fn, marginal_prob_std_fn, diffusion_coeff_fn, get_optimizer(cfg, model),
                                    torch.device("cuda"), None, cfg)
    _, _, gen_dl = get_dataloader(cfg)
    gen = pipe.generate_and_plot_samples(gen_dl, cfg=cfg, epoch=1)
    assert gen.dim() == 4 and gen.shape[1:] == (1, 64, 64) and torch.isfinite(gen).all()
