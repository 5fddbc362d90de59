"""Constrained sampling on the GPU (known pixels held in Euler-Maruyama, predictor-corrector and EDM Heun runs): the
native loops against the host restatements of constrained_ref.py around the oracle network, the exactness of the hold (mask 1 is
`known`, mask 0 is the unconstrained run, NaN under a zero mask is never read), a pixel-independent score, the Python loops against the
native ones, step-graph reuse with and without a constraint, tiles, and `--mode generate` with a `constraint:` section."""
import os

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu

from oracle import torch_ref as O  # noqa: E402
from util_models import build_pair, check_parity, maxrel  # noqa: E402

import constrained_ref as R  # noqa: E402
import sbgm_danra_amd as S  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUIDED = {"classifier_free_guidance": {"enabled": True, "guidance_scale": 2.5, "guidance_scale_max": 1.5}}
SAMPLERS = {"em": S.Euler_Maruyama_sampler, "pc": S.pc_sampler, "edm": S.edm_heun_sampler}
STD = (S.marginal_prob_std_fn, S.diffusion_coeff_fn)


@pytest.fixture(scope="module")
def net():
    _, n, _ = build_pair(1)
    return n.eval()


def fields(B, hw, seed, draws=16):
    """cond, noise, known on the host and the standard mask"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, 1, hw, hw, generator=g), torch.randn(draws, B, 1, hw, hw, generator=g),
            torch.randn(B, 1, hw, hw, generator=g), R.standard_mask(B, hw))


# ---- 1. parity with the oracle network ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,hw,n,kw", [("em", 32, 5, {}), ("pc", 64, 4, {}), ("edm", 64, 5, dict(s_churn=0.0)),
                                          ("edm", 64, 5, dict(s_churn=40.0))])
def test_native_loop_matches_oracle_restatement(kind, hw, n, kw):
    ora, native, _ = build_pair(1)
    ora.eval(), native.eval()
    cond, noise, known, mask = fields(2, hw, 11)
    score = lambda x, t: ora(x, t, cond_img=cond)  # noqa: E731
    with torch.no_grad():
        want = {"em": R.em_restatement, "pc": R.pc_restatement, "edm": R.heun_restatement}[kind](score, noise, n, known, mask, **kw)
        got = SAMPLERS[kind](native, *STD, batch_size=2, num_steps=n, device="cuda", img_size=hw, cond_img=cond.cuda(), noise=noise,
                             known=known, known_mask=mask, **kw)
    assert got.shape == (2, 1, hw, hw)
    assert torch.equal(got.cpu()[mask == 1], known[mask == 1])
    check_parity(got.cpu(), want, 1e-4, f"constrained {kind} {hw}x{hw} N={n} {kw} vs oracle")


def test_guided_native_loop_matches_oracle_restatement():
    ora, native, _ = build_pair(1, 4)
    ora.eval(), native.eval()
    cond, noise, known, mask = fields(2, 32, 12)
    y = torch.tensor([1, 3])
    g = GUIDED["classifier_free_guidance"]
    pred = lambda x, t: O.guided_score_fn(ora, x, t, y, cond, scale=g["guidance_scale"])  # noqa: E731
    corr = lambda x, t: O.guided_score_fn(ora, x, t, y, cond, scale=g["guidance_scale_max"])  # noqa: E731  (the corrector's is clamped)
    with torch.no_grad():
        want = R.pc_restatement(pred, noise, 4, known, mask, score_corr=corr)
        got = S.pc_sampler(native, *STD, batch_size=2, num_steps=4, device="cuda", img_size=32, y=y.cuda(), cond_img=cond.cuda(),
                           cfg=GUIDED, noise=noise, known=known, known_mask=mask)
    check_parity(got.cpu(), want, 1e-4, "constrained guided pc N=4 vs oracle")


# ---- 2. exactness ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["em", "pc", "edm"])
def test_hold_is_exact(net, kind):
    cond, _, known, mask = fields(2, 32, 13)
    cond, known = cond.cuda(), known.cuda()
    run = lambda seed=5, graph=True, **kw: SAMPLERS[kind](net, *STD, batch_size=2, num_steps=4, device="cuda", img_size=32,  # noqa: E731
                                                          cond_img=cond, seed=seed, use_graph=graph, **kw)
    # mask == 1 everywhere: the output is `known`, whatever the seed
    for seed in (5, 6):
        assert torch.equal(run(seed, known=known, known_mask=torch.ones(32, 32)), known)
    # mask == 0 everywhere: the unconstrained run, bit for bit, replayed and eager
    free = run()
    for graph in (True, False):
        assert torch.equal(run(graph=graph, known=known, known_mask=torch.zeros(2, 1, 32, 32)), free)
    # binary mask: `known` on it, and the free pixels feel the held ones through the network
    binary = (mask >= 1).float()
    out = run(known=known, known_mask=binary)
    on = binary.bool().cuda()
    assert torch.isfinite(out).all() and torch.equal(out[on], known[on])
    assert not torch.equal(out[~on], free[~on])
    # NaN wherever the mask is 0: never read
    poisoned = torch.where(on, known, torch.full_like(known, float("nan")))
    zeroed = torch.where(on, known, torch.zeros_like(known))
    a, b = run(known=poisoned, known_mask=binary), run(known=zeroed, known_mask=binary)
    assert torch.isfinite(a).all() and torch.equal(a, b) and torch.equal(a, out)


# ---- 3. pixel-independent score through the Python loop -----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["em", "edm"])                         # not PC: its step size sees the whole sample
def test_pixel_independent_score_leaves_free_pixels_alone(kind):
    _, _, known, mask = fields(2, 32, 14)
    binary = (mask >= 1).float()
    run = lambda **kw: SAMPLERS[kind](R.gaussian_score(1.0), *STD, batch_size=2, num_steps=6, device="cuda", img_size=32,  # noqa: E731
                                      seed=9, **kw).cpu()
    free, held = run(), run(known=known, known_mask=binary)
    assert torch.equal(held[binary == 0], free[binary == 0])
    assert torch.equal(held[binary == 1], known[binary == 1])


# ---- 4. Python loop == native loop ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,kw", [("em", {}), ("pc", {}), ("edm", dict(s_churn=0.0)), ("edm", dict(s_churn=30.0))])
def test_python_loop_equals_native_loop(net, kind, kw):
    cond, noise, known, mask = fields(2, 32, 15)
    cond = cond.cuda()
    f = lambda x, t, y=None, c=None, l=None, tp=None: net(x, t, y, c, l, tp)  # noqa: E731  (a plain callable, not a ScoreNet)
    run = lambda m, **how: SAMPLERS[kind](m, *STD, batch_size=2, num_steps=5, device="cuda", img_size=32, cond_img=cond,  # noqa: E731
                                          known=known, known_mask=mask, **kw, **how).cpu()
    a, b = run(net, noise=noise), run(f, noise=noise)
    assert torch.isfinite(a).all() and torch.equal(a[mask == 1], known[mask == 1]) and torch.equal(b[mask == 1], known[mask == 1])
    assert maxrel(a, b) <= 1e-4
    a, b = run(net, seed=17), run(f, seed=17)           # in-kernel noise: the hold op reproduces the step's draw by (seed, draw index)
    assert torch.equal(b[mask == 1], known[mask == 1])
    assert maxrel(a, b) <= 1e-4


# ---- 5. graphs ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["em", "pc", "edm"])
def test_step_graph_with_and_without_a_constraint(net, kind):
    cond, _, known_h, mask = fields(2, 64, 16)
    cond, known, mask = cond.cuda(), known_h.cuda(), mask.cuda()
    run = lambda graph=True, **kw: SAMPLERS[kind](net, *STD, batch_size=2, num_steps=6, device="cuda", img_size=64,  # noqa: E731
                                                  cond_img=cond, seed=31, use_graph=graph, **kw)
    held = run(known=known, known_mask=mask)
    assert torch.isfinite(held).all()
    assert torch.equal(held, run(False, known=known, known_mask=mask))                 # replay == eager
    free = run()
    assert torch.equal(free, run(False)) and not torch.equal(free, held)
    assert torch.equal(run(known=known, known_mask=mask), held) and torch.equal(run(), free)    # held, unheld, held, unheld
    # new contents at the same address are read by the replays
    other = torch.randn(2, 1, 64, 64, generator=torch.Generator().manual_seed(99)).cuda()
    want_other = run(False, known=other.clone(), known_mask=mask)
    known.copy_(other)
    got_other = run(known=known, known_mask=mask)
    assert not torch.equal(got_other, held) and torch.equal(got_other, want_other)
    # a tensor at a new address: the result of an eager run on it
    moved = known_h.cuda()
    assert moved.data_ptr() != known.data_ptr()
    assert torch.equal(run(known=moved, known_mask=mask), held)


# ---- 6. tiles ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["pc", "edm"])
def test_tiles_hold_the_domain_fields(net, kind):
    from sbgm_danra_amd.tiling import FullDomainTiler
    t = FullDomainTiler((150, 170), 64, 8)
    assert t.Wd_pad == 172                                               # the padded path
    g = torch.Generator().manual_seed(17)
    cond, known = torch.randn(1, 150, 170, generator=g).cuda(), torch.randn(1, 150, 170, generator=g).cuda()
    mask = torch.zeros(1, 150, 170)
    mask[0, :9, :13] = 1.0                                               # a corner
    mask[0, 50:71, 37:139] = 1.0                                         # a block across tile seams
    mask[0, 71, 37:139] = 0.5
    mask[0, :, 167:] = 1.0                                               # the strip at the padded edge
    mask[0, 3::17, 5::11] = 1.0                                          # stations
    mask = mask.cuda()
    sampler = SAMPLERS[kind]
    sample = lambda: t.sample(net, sampler, *STD, num_steps=4, cond_img=cond, seed=21, tiles_per_batch=5, known=known,  # noqa: E731
                              known_mask=mask)
    dom = sample()
    assert dom.shape == (1, 150, 170) and torch.isfinite(dom).all()
    assert torch.equal(dom[mask == 1], known[mask == 1])
    assert not torch.equal(dom[mask == 0], known[mask == 0])
    assert torch.equal(sample(), dom)
    # a tile's result does not depend on its place in the batch
    tiles, kt, mt = t.extract(cond), t.extract(known), t.extract(mask)
    run = lambda idx: sampler(net, *STD, batch_size=len(idx), num_steps=4, device="cuda", img_size=64, seed=21,  # noqa: E731
                              domain_width=t.Wd_pad, cond_img=tiles[idx], tile_origins=t.origins_dev[idx].contiguous(),
                              known=kt[idx], known_mask=mt[idx])
    fwd = list(range(len(t)))
    full = run(fwd)
    assert maxrel(run(fwd[::-1]).flip(0).cpu(), full.cpu()) <= 1e-6
    assert torch.equal(full[mt == 1], kt[mt == 1])
    with pytest.raises(ValueError):                                      # a sampler that does not take the arguments
        t.sample(net, S.rk45_sampler, *STD, num_steps=None, cond_img=cond, known=known, known_mask=mask)


# ---- 7. CLI generation -------------------------------------------------------------------------------------------------------------
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
    raw["sampler"]["sampler_type"] = "pc_sampler"
    raw["sampler"]["n_timesteps"] = 4
    raw["constraint"] = {"enabled": True, "station_fraction": 0.05, "seed": 3}
    raw["evaluation"].update(batch_size=3, gen_type=["multiple", "single", "repeated"], n_repeats=2, transform_back=False)
    raw["training"]["batch_size"] = 2
    p = tmp_path / "run.yaml"
    p.write_text(yaml.safe_dump(raw))
    return str(p)


def test_cli_generate_holds_the_truth_on_the_station_mask(cfg_path):
    from sbgm.cli import main_app
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
        assert mask.shape == (64, 64) and set(np.unique(mask)) == {0.0, 1.0} and 0.02 < mask.mean() < 0.09
        truth = np.broadcast_to(truth.reshape(-1, 64, 64), gen.shape)
        on = np.broadcast_to(mask == 1, gen.shape)
        assert np.array_equal(gen[on], truth[on]), suffix
        assert not np.array_equal(gen[~on], truth[~on]), suffix
