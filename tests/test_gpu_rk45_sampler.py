"""rk45_sampler on the GPU: the native loop (one captured attempt replayed until the device reports done) and the Python loop over the
same kernels, against the reference's RK45 golden, the scipy-driven `ode_sampler`, scipy on an analytic score, and `solve_ivp` around
native evaluations in the encoding direction; per-sample controllers, tiles, guidance and conditions, and the CLI / preview wiring.

Bounds.  An adaptive solver amplifies fp32-level differences of the right-hand side through its step decisions, so endpoints are held to
the project's policy for this solver (test_ode_sampler_matches_reference_golden): max-rel <= 20 x the solver tolerance and
evaluation counts within max(6, 2 %).  Where two runs launch the same kernels on the same data (graph against eager, native against
Python loop from a given start, one seed twice) they are bit-equal."""
import os

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu

from oracle import torch_ref as O  # noqa: E402
import util_models  # noqa: E402
from util_models import build_pair, check_parity, load_golden, maxrel  # noqa: E402

import sbgm_danra_amd as S  # noqa: E402
from sbgm_danra_amd import score_sampling as SS  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIG = 25.0
GUIDED = {"classifier_free_guidance": {"enabled": True, "guidance_scale": 2.5, "guidance_scale_max": 1.5}}
FNS = (S.marginal_prob_std_fn, S.diffusion_coeff_fn)


def note(label, got, want, tol, **counts):
    """max-rel of `got` against `want` held to `tol` by util_models.check_parity, which prints it with the element-wise figure (measured
    only: the policy for this solver bounds the global norm) and keeps both, and the run's `counts`, with the other samplers' measured
    parity figures"""
    if counts:
        print(f"measured[{label}]: " + ", ".join(f"{k} {v}" for k, v in counts.items()))
        util_models._MEASURED[label + "/counts"] = counts
    check_parity(got, want, tol, label, elem_tol=float("inf"))
    return util_models._MEASURED[label]["global"]


def nfev_close(a, b):
    return abs(int(a) - int(b)) <= max(6, 0.02 * int(b))


def as_callable(net):
    """the network as a plain callable (not a ScoreNet): rk45_sampler then runs its Python loop"""
    return lambda x, t, y=None, c=None, l=None, tp=None: net(x, t, y, c, l, tp)  # noqa: E731


@pytest.fixture(scope="module")
def plain():
    _, net, _ = build_pair(0)
    net.eval()
    return net


@pytest.fixture(scope="module")
def golden(golden_dir):
    return load_golden(os.path.join(golden_dir, "ode_b2_32.npz"))


# ---- 6. the reference's own RK45 run ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tol,tag", [(1e-3, "tol1e-3"), (1e-5, "tol1e-5")])
def test_native_loop_matches_reference_golden(plain, golden, tol, tag):
    """measured on MI355X: max-rel 7.2e-3 at 1e-3 (224 evaluations, golden 224), 5.2e-5 at 1e-5 (968, golden 974; scipy around the
    native network also takes 968)"""
    got, st = S.rk45_sampler(plain, *FNS, batch_size=2, z=golden["z"].cuda(), rtol=tol, atol=tol, return_stats=True)
    want, nref = golden[f"x_{tag}"], int(golden[f"nfev_{tag}"])
    note(f"rk45/golden/{tag}", got.double().cpu(), want, 20 * tol, nfev=int(st["nfev"]), nfev_golden=nref, accepted=st["n_accepted"],
         rejected=st["n_rejected"], surplus=st["surplus_attempts"])
    assert got.dtype == torch.float32 and got.shape == (2, 1, 32, 32)
    assert st["nfev"] == 2 + 6 * (st["n_accepted"] + st["n_rejected"]) and st["t_final"] == 1e-3 and st["surplus_attempts"] <= 1
    assert nfev_close(st["nfev"], nref)


# ---- 7. the scipy-driven sampler on the same model and start ------------------------------------------------------------------------------
@pytest.mark.parametrize("tol", [1e-3, 1e-5])
def test_native_loop_matches_scipy_driven_ode_sampler(plain, golden, tol):
    z = golden["z"].cuda()
    want, nref = S.ode_sampler(plain, *FNS, batch_size=2, device="cuda", z=z, atol=tol, rtol=tol, return_nfev=True)
    got, st = S.rk45_sampler(plain, *FNS, batch_size=2, z=z, rtol=tol, atol=tol, return_stats=True)
    note(f"rk45/ode_sampler/tol{tol:g}", got.double().cpu(), want.cpu(), 20 * tol, nfev=int(st["nfev"]), nfev_scipy=int(nref))
    assert nfev_close(st["nfev"], nref)


# ---- 8. Python loop == native loop; graph == eager; seeds; surplus attempts ----------------------------------------------------------------
@pytest.mark.parametrize("error_norm", ["batch", "sample"])
def test_python_loop_graph_and_eager_are_one_computation(plain, golden, error_norm):
    z = golden["z"].cuda()
    kw = dict(batch_size=2, rtol=1e-4, atol=1e-4, error_norm=error_norm, return_stats=True)
    a, sa = S.rk45_sampler(plain, *FNS, z=z, **kw)
    b, sb = S.rk45_sampler(plain, *FNS, z=z, use_graph=False, **kw)
    c, sc = S.rk45_sampler(as_callable(plain), *FNS, z=z, **kw)
    assert torch.isfinite(a).all()
    for s in (sa, sb, sc):
        assert np.all(np.asarray(s["t_final"]) == 1e-3) and s["surplus_attempts"] <= 1
    assert sc["surplus_attempts"] == 0
    for k in ("nfev", "n_accepted", "n_rejected", "t_final"):
        assert np.array_equal(sa[k], sb[k]) and np.array_equal(sa[k], sc[k]), (k, sa[k], sb[k], sc[k])
    assert torch.equal(a, b)                                            # graph replay == eager attempts, bit for bit
    note(f"rk45/python_vs_native/{error_norm}", c.cpu(), a.cpu(), 20 * 1e-4, bit_equal=bool(torch.equal(a, c)),
         nfev=np.asarray(sa["nfev"]).tolist())
    # seeded start: one seed twice is bit-equal, another seed is another sample, the two loops draw the same Philox numbers
    kw2 = dict(batch_size=2, img_size=32, rtol=1e-3, atol=1e-3, error_norm=error_norm)
    s1, s2, s3 = (S.rk45_sampler(plain, *FNS, seed=s, **kw2) for s in (11, 11, 12))
    assert torch.equal(s1, s2) and not torch.equal(s1, s3)
    p1 = S.rk45_sampler(as_callable(plain), *FNS, seed=11, **kw2)
    assert maxrel(p1.cpu(), s1.cpu()) <= 20 * 1e-3
    # injected noise is draw 0
    nz = torch.randn(1, 2, 1, 32, 32, generator=torch.Generator().manual_seed(2))
    n1 = S.rk45_sampler(plain, *FNS, noise=nz, **kw2)
    n2 = S.rk45_sampler(plain, *FNS, z=nz[0].cuda() * S.marginal_prob_std_fn(torch.ones(1, device="cuda")), **kw2)
    assert maxrel(n1.cpu(), n2.cpu()) <= 20 * 1e-3


def test_failures_are_raised_with_their_cause(plain, golden):
    z = golden["z"].cuda()
    for model in (plain, as_callable(plain)):
        with pytest.raises(SS.OdeSolverError, match=r"step budget \(max_steps=3\)"):
            S.rk45_sampler(model, *FNS, batch_size=2, z=z, max_steps=3)
    with pytest.raises(SS.OdeSolverError, match=r"sample \d\): the step budget"):
        S.rk45_sampler(plain, *FNS, batch_size=2, z=z, max_steps=3, error_norm="sample")
    calls = []

    def nan_score(x, t, y=None, c=None, l=None, tp=None):
        calls.append(1)
        return torch.full_like(x, float("nan")) if len(calls) > 3 else -x / 600.0
    with pytest.raises(SS.OdeSolverError, match="non-finite error norm"):
        S.rk45_sampler(nan_score, *FNS, batch_size=2, z=z)
    assert len(calls) == 8                                              # it stopped with the attempt that saw the NaN


# ---- 9. analytic score through the Python loop and the device kernels ----------------------------------------------------------------------
def gaussian_score(s0):
    def f(x, t, y=None, c=None, l=None, tp=None):
        std = SS._ve_std(t.double().cpu().numpy(), SIG)
        var = torch.as_tensor(s0 ** 2 + std ** 2, device=x.device).view(-1, 1, 1, 1)
        return (-x.double() / var).to(x.dtype)
    return f


def gaussian_rhs(s0):
    """the same right-hand side for scipy on the CPU, in the precision of ode_sampler's"""
    def f(t, x):
        tf = np.float32(t)
        g = np.float32(SIG) ** tf
        c = np.float32(-0.5) * np.float32(g * g)
        return np.float64(c) * (-x / (s0 ** 2 + SS._ve_std(float(tf), SIG) ** 2)).astype(np.float32).astype(np.float64)
    return f


@pytest.mark.parametrize("s0", [0.5, 1.0, 2.0])
@pytest.mark.parametrize("tol", [1e-3, 1e-5])
@pytest.mark.parametrize("error_norm", ["batch", "sample"])
def test_analytic_score_error_is_scipys(s0, tol, error_norm):
    """x(t) = x(1) sqrt((s0^2 + std(t)^2) / (s0^2 + std(1)^2)) solves the flow of Gaussian data exactly.  The device solver's error is
    held to 2 x the error scipy's RK45 makes on the same problem (same algorithm; only the fp32 rounding of the kernels' inputs and
    outputs differs) + 1e-6 max|x|, in the sampling direction and over the round trip 1 -> eps -> 1."""
    from scipy.integrate import solve_ivp
    eps = 1e-3
    v1, ve = s0 ** 2 + SS._ve_std(1.0, SIG) ** 2, s0 ** 2 + SS._ve_std(eps, SIG) ** 2
    x1 = (torch.randn(2, 1, 32, 32, generator=torch.Generator().manual_seed(int(10 * s0))) * np.sqrt(v1)).float()
    exact = x1.double() * np.sqrt(ve / v1)
    kw = dict(batch_size=2, rtol=tol, atol=tol, error_norm=error_norm, return_stats=True)
    got, st = S.rk45_sampler(gaussian_score(s0), *FNS, z=x1.cuda(), **kw)
    back, st2 = S.rk45_sampler(gaussian_score(s0), *FNS, z=got, t_span=(eps, 1.0), **kw)
    err = float((got.double().cpu() - exact).abs().max())
    err_rt = float((back.double().cpu() - x1.double()).abs().max())
    # scipy on the same problem; per sample when the controllers are per sample
    rows = x1.double().numpy().reshape(2, -1) if error_norm == "sample" else x1.double().numpy().reshape(1, -1)
    ref, ref_rt, nfev = 0.0, 0.0, []
    for r in rows:
        fwd = solve_ivp(gaussian_rhs(s0), (1.0, eps), r, method="RK45", rtol=tol, atol=tol)
        bwd = solve_ivp(gaussian_rhs(s0), (eps, 1.0), fwd.y[:, -1], method="RK45", rtol=tol, atol=tol)
        ref = max(ref, float(np.abs(fwd.y[:, -1] - r * np.sqrt(ve / v1)).max()))
        ref_rt = max(ref_rt, float(np.abs(bwd.y[:, -1] - r).max()))
        nfev.append((fwd.nfev, bwd.nfev))
    slack = 1e-6 * float(x1.abs().max())
    label = f"rk45/analytic/s0={s0:g}/tol{tol:g}/{error_norm}"           # the same two bounds, as max-rel: divided by max|exact|
    note(label, got.double().cpu(), exact, (2 * ref + slack) / float(exact.abs().max()), err=err, err_scipy=ref,
         nfev=np.asarray(st["nfev"]).tolist(), nfev_scipy=[n[0] for n in nfev])
    note(label + "/roundtrip", back.double().cpu(), x1.double(), (2 * ref_rt + slack) / float(x1.abs().max()), err=err_rt, err_scipy=ref_rt,
         nfev=np.asarray(st2["nfev"]).tolist(), nfev_scipy=[n[1] for n in nfev])
    assert err <= 2 * ref + slack
    assert err_rt <= 2 * ref_rt + slack
    assert all(nfev_close(a, n[0]) for a, n in zip(np.atleast_1d(st["nfev"]), nfev))
    assert np.all(np.asarray(st2["t_final"]) == 1.0)


# ---- 10. the encoding direction on the network, against solve_ivp around native evaluations -------------------------------------------------
@pytest.mark.parametrize("tol", [1e-3, 1e-5])
def test_encoding_matches_scipy_around_native_evaluations(plain, golden, tol):
    from scipy.integrate import solve_ivp
    data = golden["x_tol1e-5"].float().cuda()                            # a sample of this network: the data to encode
    shape = data.shape

    def rhs(t, xflat):                                                  # the right-hand side of ode_sampler, written out
        xs = torch.tensor(xflat, device="cuda", dtype=torch.float32).reshape(shape)
        tt = torch.tensor(np.ones((shape[0],)) * t, device="cuda", dtype=torch.float32)
        with torch.no_grad():
            s = plain(xs, tt)
        g = S.diffusion_coeff_fn(torch.tensor(t)).cpu().numpy()
        return -0.5 * (g ** 2) * s.cpu().numpy().reshape(-1).astype(np.float64)
    ref = solve_ivp(rhs, (1e-3, 1.0), data.reshape(-1).double().cpu().numpy(), rtol=tol, atol=tol, method="RK45")
    got, st = S.rk45_sampler(plain, *FNS, z=data, t_span=(1e-3, 1.0), rtol=tol, atol=tol, return_stats=True)
    note(f"rk45/encode/tol{tol:g}", got.double().cpu().reshape(-1), torch.from_numpy(ref.y[:, -1]), 20 * tol, nfev=int(st["nfev"]),
         nfev_scipy=int(ref.nfev), rejected=st["n_rejected"])
    assert ref.status == 0 and st["t_final"] == 1.0
    assert nfev_close(st["nfev"], ref.nfev)
    with pytest.raises(ValueError, match="pass it as z"):
        S.rk45_sampler(plain, *FNS, batch_size=2, img_size=32, t_span=(1e-3, 1.0))


# ---- 11. one controller per sample; tiles -----------------------------------------------------------------------------------------------------
def test_sample_mode_row_equals_its_own_run(plain):
    tol = 1e-4
    z = (torch.randn(4, 1, 32, 32, generator=torch.Generator().manual_seed(8)) * float(SS._ve_std(1.0, SIG))).cuda()
    kw = dict(rtol=tol, atol=tol, error_norm="sample", return_stats=True)
    full, st = S.rk45_sampler(plain, *FNS, z=z, **kw)
    assert st["nfev"].shape == (4,) and np.all(st["t_final"] == 1e-3)
    for b in range(4):
        one, s1 = S.rk45_sampler(plain, *FNS, z=z[b:b + 1], **kw)
        ref, nref = S.ode_sampler(plain, *FNS, batch_size=1, device="cuda", z=z[b:b + 1], atol=tol, rtol=tol, return_nfev=True)
        note(f"rk45/sample_mode/row{b}/own_run", full[b:b + 1].cpu(), one.cpu(), 20 * tol, nfev=int(st["nfev"][b]), nfev_own=int(s1["nfev"][0]))
        note(f"rk45/sample_mode/row{b}/scipy", full[b:b + 1].double().cpu(), ref.cpu(), 20 * tol, nfev=int(st["nfev"][b]), nfev_scipy=int(nref))
        assert nfev_close(st["nfev"][b], s1["nfev"][0]) and nfev_close(st["nfev"][b], nref)


def test_tiles_share_noise_and_do_not_couple():
    from sbgm_danra_amd.tiling import FullDomainTiler
    _, net, sd = build_pair(1)
    net.eval()
    t = FullDomainTiler((150, 172), 64, 8)
    cond = torch.randn(1, 150, 172, generator=torch.Generator().manual_seed(9)).cuda()
    tiles = t.extract(cond)
    tol = 1e-3
    kw = dict(device="cuda", img_size=64, seed=21, domain_width=t.Wd_pad, rtol=tol, atol=tol, error_norm="sample", return_stats=True)
    run = lambda model, idx: S.rk45_sampler(model, *FNS, batch_size=len(idx), cond_img=tiles[idx],  # noqa: E731
                                            tile_origins=t.origins_dev[idx].contiguous(), **kw)
    everything = list(range(len(t)))
    full, st = run(net, everything)
    assert torch.isfinite(full).all()
    # batch position: the same tiles in reverse order
    rev, sr = run(net, everything[::-1])
    for i in everything:
        note(f"rk45/tiles/reversed/tile{i}", rev.flip(0)[i:i + 1].cpu(), full[i:i + 1].cpu(), 20 * tol, accepted=int(st["n_accepted"][i]),
             rejected=int(st["n_rejected"][i]))
    assert np.array_equal(sr["n_accepted"][::-1], st["n_accepted"]) and np.array_equal(sr["n_rejected"][::-1], st["n_rejected"])
    # batch-mates: three of the tiles on their own
    some = [5, 0, 7]
    part, sp = run(net, some)
    for i, j in enumerate(some):
        note(f"rk45/tiles/subset/tile{j}", part[i:i + 1].cpu(), full[j:j + 1].cpu(), 20 * tol, accepted=int(sp["n_accepted"][i]),
             rejected=int(sp["n_rejected"][i]))
    assert np.array_equal(sp["n_accepted"], st["n_accepted"][some]) and np.array_equal(sp["n_rejected"], st["n_rejected"][some])
    # a shared step would couple tiles; the Python loop cannot key noise by domain position
    with pytest.raises(ValueError, match="error_norm='sample'"):
        S.rk45_sampler(net, *FNS, batch_size=1, cond_img=tiles[:1], tile_origins=t.origins_dev[:1].contiguous(), img_size=64)
    with pytest.raises(S._native.NativeError):
        run(as_callable(net), [0])
    # initial noise: with a score that is zero everywhere (final projection zeroed) the state never moves, so the result IS the start
    zero = {k: (torch.zeros_like(v) if k.startswith("decoder.final_layer.conv.") else v) for k, v in sd.items()}
    net.load_state_dict(zero)
    start, s0 = run(net, everything)
    assert np.all(s0["n_rejected"] == 0) and float(start.abs().max()) > 1.0
    shared = 0
    for i, (yi, xi) in enumerate(t.origins):
        for j, (yj, xj) in enumerate(t.origins):
            ya, yb, xa, xb = max(yi, yj), min(yi, yj) + 64, max(xi, xj), min(xi, xj) + 64
            if j <= i or ya >= yb or xa >= xb:
                continue
            shared += 1
            assert torch.equal(start[i, 0, ya - yi:yb - yi, xa - xi:xb - xi], start[j, 0, ya - yj:yb - yj, xa - xj:xb - xj]), (i, j)
    assert shared >= len(t)
    # the tiler drives it (no step count: num_steps=None)
    net.load_state_dict(sd)
    dom = t.sample(net, S.rk45_sampler, *FNS, None, cond_img=cond, seed=21, tiles_per_batch=4, rtol=1e-2, atol=1e-2, error_norm="sample")
    assert dom.shape == (1, 150, 172) and torch.isfinite(dom).all()


# ---- 12. guided and conditioned ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("error_norm", ["batch", "sample"])
def test_guided_conditioned_native_equals_python_loop(error_norm):
    _, net, _ = build_pair(1, 4)
    net.eval()
    g = torch.Generator().manual_seed(6)
    cond = torch.randn(2, 1, 32, 32, generator=g).cuda()
    y = torch.tensor([1, 3]).cuda()
    z = (torch.randn(2, 1, 32, 32, generator=g) * float(SS._ve_std(1.0, SIG))).cuda()
    tol = 1e-3
    kw = dict(z=z, rtol=tol, atol=tol, error_norm=error_norm, return_stats=True)
    a, sa = S.rk45_sampler(net, *FNS, y=y, cond_img=cond, cfg=GUIDED, **kw)
    b, sb = S.rk45_sampler(as_callable(net), *FNS, y=y, cond_img=cond, cfg=GUIDED, **kw)          # guided_score_fn per evaluation
    note(f"rk45/guided/{error_norm}", a.cpu(), b.cpu(), 20 * tol, nfev=np.asarray(sa["nfev"]).tolist(),
         nfev_python=np.asarray(sb["nfev"]).tolist())
    assert torch.isfinite(a).all()
    assert all(nfev_close(p, q) for p, q in zip(np.atleast_1d(sa["nfev"]), np.atleast_1d(sb["nfev"])))
    # guidance and every condition change the result
    plain_run = S.rk45_sampler(net, *FNS, y=y, cond_img=cond, **kw)[0]
    other_cond = S.rk45_sampler(net, *FNS, y=y, cond_img=cond.flip(0), cfg=GUIDED, **kw)[0]
    other_y = S.rk45_sampler(net, *FNS, y=torch.tensor([2, 2]).cuda(), cond_img=cond, cfg=GUIDED, **kw)[0]
    for other in (plain_run, other_cond, other_y):
        assert maxrel(other.cpu(), a.cpu()) > 20 * tol
    # unguided but conditioned: the two loops again
    c = S.rk45_sampler(as_callable(net), *FNS, y=y, cond_img=cond, **kw)[0]
    assert maxrel(c.cpu(), plain_run.cpu()) <= 20 * tol


# ---- 13. CLI generation and the training preview ----------------------------------------------------------------------------------------------
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
    raw["sampler"]["sampler_type"] = "rk45_sampler"
    raw["sampler"]["n_timesteps"] = 1000                                 # not read by this sampler
    raw["ode"] = {"rtol": 1e-2, "atol": 1e-2, "error_norm": "sample", "max_steps": 400}
    raw["evaluation"].update(batch_size=3, gen_type=["multiple", "single", "repeated"], n_repeats=2)
    raw["training"]["batch_size"] = 2
    p = tmp_path / "run.yaml"
    p.write_text(yaml.safe_dump(raw))
    return str(p)


def test_cli_generate_and_training_preview_with_rk45(cfg_path):
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
