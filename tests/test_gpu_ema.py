"""GPU suite: exponential moving average of the weights (training.with_ema) — the fused Adam/AdamW + EMA launch and the EMA-only
launch of csrc/optim.hip (sbgm_danra_amd.ema / optim), and the pipeline around them: captured and eager steps, validation and
sampling from the shadow, checkpoints, CLI generation with load_ema, two ranks."""
import logging
import os

import numpy as np
import pytest
import torch
import yaml

from sbgm_danra_amd import optim as O
from sbgm_danra_amd.ema import ModelEMA, decay_at

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1,), (7,), (33, 5), (64, 64, 3, 3), (4097,), (3, 1, 1, 1), (512, 256)]
DECAY = 0.45          # (1 + n) / (10 + n) passes it at n = 7: the 8-step runs cover the warm-up and the capped rate


class _Holder(torch.nn.Module):
    """parameters of SHAPES plus a misaligned one (a view 4 bytes into its storage: the scalar path of the kernel)"""

    def __init__(self, dev, bn=False):
        super().__init__()
        g = torch.Generator().manual_seed(5)
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(*s, generator=g).to(dev)) for s in SHAPES])
        base = torch.randn(1 + 1030, generator=g).to(dev)
        self.odd = torch.nn.Parameter(base[1:])
        self.bn = torch.nn.BatchNorm2d(6).to(dev) if bn else None

    def params(self):
        return list(self.ps) + [self.odd]


def _grads(step, params):
    g = torch.Generator().manual_seed(100 + step)
    return [(torch.randn(p.shape, generator=g) * (0.1 + step)).to(p.device) for p in params]


def _close(got, want64, tol=1e-6):
    got = got.detach().double().cpu()
    want64 = want64.cpu()
    return float((got - want64).abs().max()) <= tol * max(float(want64.abs().max()), 1e-30)


def _ref_update(ref, live, n, decay=DECAY):
    """float64 restatement of one update: ref[k] <- ref[k] + (1 - d_n) (live[k] - ref[k]); integer tensors copied"""
    d = decay_at(decay, n)
    for k, v in live.items():
        if v.dtype.is_floating_point:
            ref[k] = ref[k] + (1.0 - d) * (v.detach().double().cpu() - ref[k])
        else:
            ref[k] = v.detach().cpu().clone()


def _start_ref(model):
    return {k: (v.detach().double().cpu() if v.dtype.is_floating_point else v.detach().cpu().clone()) for k, v in model.state_dict().items()}


# 1. fused launch -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls,wd", [(O.Adam, 1e-2), (O.AdamW, 5e-2)])
def test_fused_step_keeps_the_optimizer_bit_exact_and_averages(cls, wd):
    plain, avg = _Holder("cuda"), _Holder("cuda")
    assert avg.odd.data_ptr() % 16 != 0
    o1 = cls(plain.params(), lr=3e-3, betas=(0.9, 0.995), eps=1e-8, weight_decay=wd)
    o2 = cls(avg.params(), lr=3e-3, betas=(0.9, 0.995), eps=1e-8, weight_decay=wd)
    ema = ModelEMA(avg, DECAY)
    ema.reset()
    o2.ema = ema
    ref = _start_ref(avg)
    for step in range(8):
        for p, q, g in zip(plain.params(), avg.params(), _grads(step, plain.params())):
            p.grad, q.grad = g.clone(), g.clone()
        if step == 4:
            o1.param_groups[0]["lr"] = o2.param_groups[0]["lr"] = 1e-3
        o1.step()
        o2.step()
        _ref_update(ref, avg.state_dict(), step + 1)
    for p, q in zip(plain.params(), avg.params()):
        assert torch.equal(p, q)
        assert torch.equal(o1.state[p]["exp_avg"], o2.state[q]["exp_avg"])
        assert torch.equal(o1.state[p]["exp_avg_sq"], o2.state[q]["exp_avg_sq"])
    assert ema.num_updates == 8
    for k, v in ema.shadow.state_dict().items():
        assert _close(v, ref[k]), k
    assert not torch.equal(ema.shadow.odd, avg.odd)       # the average lags the live weights


# 2. EMA-only mode ------------------------------------------------------------------------------------------------------------
def test_parameters_without_gradient_ride_on_the_fused_launch():
    plain, avg = _Holder("cuda", bn=True), _Holder("cuda", bn=True)
    o1 = O.Adam(plain.parameters(), lr=1e-3, weight_decay=1e-6)
    o2 = O.Adam(avg.parameters(), lr=1e-3, weight_decay=1e-6)
    ema = ModelEMA(avg, DECAY)
    ema.reset()
    o2.ema = ema
    ref = _start_ref(avg)
    for step in range(6):
        for i, (p, q, g) in enumerate(zip(plain.params(), avg.params(), _grads(step, plain.params()))):
            p.grad, q.grad = (None, None) if (i == 2 and step % 2) else (g.clone(), g.clone())
        for m in (plain.bn, avg.bn):                        # buffers move outside the optimizer (as a train-mode forward does)
            m.running_mean.add_(0.25 * (step + 1))
            m.running_var.mul_(1.5)
            m.num_batches_tracked += 1
        avg.bn.weight.grad = avg.bn.bias.grad = None        # BatchNorm affine parameters never get a gradient here
        o1.step()
        o2.step()
        _ref_update(ref, avg.state_dict(), step + 1)
    for p, q in zip(plain.params(), avg.params()):
        assert torch.equal(p, q)
    for k, v in ema.shadow.state_dict().items():
        if v.dtype.is_floating_point:
            assert _close(v, ref[k]), k
    assert int(ema.shadow.bn.num_batches_tracked) == 6 and ema.shadow.bn.num_batches_tracked.dtype == torch.int64


def test_ema_only_launch_after_sgd():
    m = _Holder("cuda", bn=True)
    opt = torch.optim.SGD(m.parameters(), lr=1e-2, momentum=0.9, weight_decay=1e-4)
    ema = ModelEMA(m, DECAY)
    ema.reset()
    ref = _start_ref(m)
    for step in range(8):
        for i, (q, g) in enumerate(zip(m.params(), _grads(step, m.params()))):
            q.grad = None if (i == 3 and step in (2, 5)) else g
        m.bn.running_mean.add_(0.5)
        m.bn.running_var.mul_(0.9)
        m.bn.num_batches_tracked += 3
        opt.step()
        ema.update()
        _ref_update(ref, m.state_dict(), step + 1)
    assert ema.num_updates == 8
    for k, v in ema.shadow.state_dict().items():
        if v.dtype.is_floating_point:
            assert _close(v, ref[k]), k
        else:
            assert torch.equal(v.cpu(), ref[k]), k
    assert int(ema.shadow.bn.num_batches_tracked) == 24


# pipeline fixtures (the 64x64 configuration of test_gpu_pipeline.py) ---------------------------------------------------------
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
    raw["sampler"]["n_timesteps"] = 4
    raw["evaluation"].update(batch_size=3, gen_type=["multiple"], n_repeats=2)
    raw["training"]["batch_size"] = 2
    p = tmp_path / "run.yaml"
    p.write_text(yaml.safe_dump(raw))
    return str(p)


def _pipe(cfg_path, **training_overrides):
    from sbgm.score_unet import diffusion_coeff_fn, loss_fn, marginal_prob_std_fn
    from sbgm.training import TrainingPipeline_general
    from sbgm.training_utils import get_model, get_optimizer
    from sbgm.utils import load_config
    cfg = load_config(cfg_path)
    cfg.training.use_hip_graph = True
    cfg.monitoring.extreme_prcp.enabled = False
    for k, v in training_overrides.items():
        setattr(cfg.training, k, v)
    torch.manual_seed(0)
    model, _, _ = get_model(cfg)
    pipe = TrainingPipeline_general(model, loss_fn, marginal_prob_std_fn, diffusion_coeff_fn, get_optimizer(cfg, model),
                                    torch.device("cuda"), None, cfg)
    return cfg, model, pipe


def _spy_steps(pipe, ref, decay):
    """after every optimizer step: advance the float64 restatement from the live state_dict"""
    orig, n = pipe.optimizer.step, [0]

    def step(*a, **k):
        r = orig(*a, **k)
        n[0] += 1
        _ref_update(ref, pipe.model.state_dict(), n[0], decay)
        return r
    pipe.optimizer.step = step
    return n


# 3. pipeline -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [True, False])
def test_pipeline_shadow_follows_the_rule(cfg_path, graph):
    from sbgm_danra_amd.score_unet import ScoreNet
    from sbgm_danra_amd.synthetic_data import synthetic_loader
    cfg, model, pipe = _pipe(cfg_path, with_ema=True, ema_decay=0.9, use_hip_graph=graph)
    dl = synthetic_loader(cfg, 2, n_items=8)
    ref = _start_ref(model)
    n = _spy_steps(pipe, ref, 0.9)
    pipe.train_batches(dl, epochs=2, current_epoch=1, verbose=False)
    pipe.train_batches(dl, epochs=2, current_epoch=2, verbose=False)
    assert n[0] == 8 and pipe.ema.num_updates == 8
    assert bool(getattr(pipe, "_graphs", None)) == graph
    shadow = pipe.ema_model
    assert isinstance(shadow, ScoreNet) and not shadow.training and shadow is not model
    assert not any(p.requires_grad for p in shadow.parameters()) and getattr(shadow, "_grad_arena", None) is None
    for k, v in shadow.state_dict().items():
        if v.dtype.is_floating_point:
            assert _close(v, ref[k], 2e-6), k
        else:
            assert torch.equal(v.cpu(), ref[k]), k
    assert int(shadow.encoder.bn1.num_batches_tracked) == int(model.encoder.bn1.num_batches_tracked) == 8
    v = pipe.validate_batches(dl, verbose=False)
    assert np.isfinite(v)


def test_ema_off_pipeline_is_unchanged(cfg_path):
    """with_ema false: no shadow, no EMA on the optimizer, the old checkpoint keys"""
    from sbgm_danra_amd.synthetic_data import synthetic_loader
    cfg, model, pipe = _pipe(cfg_path)
    pipe.train_batches(synthetic_loader(cfg, 2, n_items=4), epochs=1, current_epoch=1, verbose=False)
    assert pipe.ema_model is None and pipe.optimizer.ema is None
    pipe.save_model(pipe.checkpoint_dir, pipe.checkpoint_name)
    assert set(torch.load(pipe.checkpoint_path, weights_only=True)) == {"network_params", "optimizer_params"}


# 4. stale engine weights -----------------------------------------------------------------------------------------------------
def test_sampling_from_the_shadow_sees_every_update(cfg_path):
    from sbgm.training_utils import get_model
    from sbgm_danra_amd import score_sampling as SS
    from sbgm_danra_amd.score_unet import diffusion_coeff_fn, marginal_prob_std_fn
    from sbgm_danra_amd.synthetic_data import synthetic_loader
    from sbgm_danra_amd.utils import extract_samples
    cfg, model, pipe = _pipe(cfg_path, with_ema=True, ema_decay=0.9)
    dl = synthetic_loader(cfg, 2, n_items=4)
    _x, seasons, cond, _h, lsm, _s, topo, _a, _b = extract_samples(next(iter(dl)), "cuda")

    def sample(net):
        with torch.no_grad():
            return SS.pc_sampler(net, marginal_prob_std_fn, diffusion_coeff_fn, batch_size=2, num_steps=3, device="cuda", img_size=64,
                                 y=seasons, cond_img=cond, lsm_cond=lsm, topo_cond=topo, seed=1234).clone()
    pipe.train_batches(dl, epochs=2, current_epoch=1, verbose=False)
    first = sample(pipe.ema_model)                           # the shadow's engine uploads its weights here
    pipe.train_batches(dl, epochs=2, current_epoch=2, verbose=False)
    second = sample(pipe.ema_model)
    fresh, _, _ = get_model(cfg)
    fresh.load_state_dict(pipe.ema_model.state_dict())
    fresh.eval()
    want = sample(fresh)
    assert not torch.equal(first, second)
    assert torch.equal(second, want)


# 5. checkpoints --------------------------------------------------------------------------------------------------------------
def test_checkpoint_keys_load_ema_and_resume(cfg_path, caplog):
    from sbgm_danra_amd.synthetic_data import synthetic_loader
    cfg, model, pipe = _pipe(cfg_path, with_ema=True, ema_decay=0.9)
    dl = synthetic_loader(cfg, 2, n_items=6)
    pipe.train_batches(dl, epochs=1, current_epoch=1, verbose=False)
    pipe.save_model(pipe.checkpoint_dir, pipe.checkpoint_name)
    ck = torch.load(pipe.checkpoint_path, weights_only=True)
    assert set(ck) == {"network_params", "optimizer_params", "ema_network_params", "ema_num_updates"}
    assert ck["ema_num_updates"] == 3
    shadow_sd = {k: v.clone() for k, v in pipe.ema_model.state_dict().items()}
    assert all(torch.equal(ck["ema_network_params"][k], v) for k, v in shadow_sd.items())
    assert any(not torch.equal(ck["network_params"][k], v) for k, v in shadow_sd.items())
    # load_ema=True: the EMA weights go into the model; the shadow and its counter are restored too (resume)
    _, model2, pipe2 = _pipe(cfg_path, with_ema=True, ema_decay=0.9)
    pipe2.load_checkpoint(pipe.checkpoint_path, load_ema=True)
    assert all(torch.equal(model2.state_dict()[k], v) for k, v in shadow_sd.items())
    _, model3, pipe3 = _pipe(cfg_path, with_ema=True, ema_decay=0.9)
    pipe3.load_checkpoint(pipe.checkpoint_path)
    assert all(torch.equal(model3.state_dict()[k], v) for k, v in ck["network_params"].items())
    assert pipe3.ema.num_updates == 3 and all(torch.equal(pipe3.ema_model.state_dict()[k], v) for k, v in shadow_sd.items())
    pipe3.train_batches(dl, epochs=2, current_epoch=2, verbose=False)      # resumed: the average continues, it does not restart
    assert pipe3.ema.num_updates == 6
    # a checkpoint without EMA weights: load_ema warns and loads network_params
    _, _, plain = _pipe(cfg_path)
    plain.save_model(str(os.path.dirname(pipe.checkpoint_path)), "plain.pth.tar")
    _, model4, pipe4 = _pipe(cfg_path, with_ema=True)
    with torch.no_grad():
        model4.decoder.final_layer.conv.weight.mul_(0)
    with caplog.at_level(logging.WARNING):
        pipe4.load_checkpoint(os.path.join(os.path.dirname(pipe.checkpoint_path), "plain.pth.tar"), load_ema=True)
    assert "ema_network_params" in caplog.text
    want = torch.load(os.path.join(os.path.dirname(pipe.checkpoint_path), "plain.pth.tar"), weights_only=True)["network_params"]
    assert all(torch.equal(model4.state_dict()[k], v) for k, v in want.items())
    assert pipe4.ema_model is None                         # nothing to restore: the shadow starts with training


def test_preview_samples_from_the_shadow_of_the_best_checkpoint(cfg_path):
    from sbgm_danra_amd.synthetic_data import synthetic_loader
    cfg, model, pipe = _pipe(cfg_path, with_ema=True, ema_decay=0.9)
    dl = synthetic_loader(cfg, 2, n_items=4)
    pipe.train_batches(dl, epochs=1, current_epoch=1, verbose=False)
    pipe.save_model(pipe.checkpoint_dir, pipe.checkpoint_name)
    saved = torch.load(pipe.checkpoint_path, weights_only=True)
    pipe.train_batches(dl, epochs=2, current_epoch=2, verbose=False)
    gen = pipe.generate_and_plot_samples(synthetic_loader(cfg, 2, n_items=2), cfg=cfg, epoch=2)
    assert torch.isfinite(gen).all()
    assert all(torch.equal(pipe.ema_model.state_dict()[k], v) for k, v in saved["ema_network_params"].items())
    assert all(torch.equal(model.state_dict()[k], v) for k, v in saved["network_params"].items())
    assert pipe.ema.num_updates == saved["ema_num_updates"]


# 6. CLI generation -----------------------------------------------------------------------------------------------------------
def test_cli_generation_with_load_ema(cfg_path):
    from sbgm.training_utils import get_model
    from sbgm.utils import get_model_string, load_config
    from sbgm_danra_amd.evaluate_sbgm.generation_main import generation_main
    cfg = load_config(cfg_path)
    torch.manual_seed(0)
    live, _, _ = get_model(cfg)
    live_sd = {k: v.detach().cpu().clone() for k, v in live.state_dict().items()}
    ema_sd = {k: (v * 0.9 if v.dtype.is_floating_point else v) for k, v in live_sd.items()}
    ckpt_dir = os.path.join(cfg.paths.path_save, cfg.paths.checkpoint_dir)
    os.makedirs(ckpt_dir, exist_ok=True)
    path = os.path.join(ckpt_dir, get_model_string(cfg) + ".pth.tar")
    out = os.path.join(cfg.paths.sample_dir, "generation", get_model_string(cfg), "generated_samples", "gen_samples_multi_n_3.npz")

    def run(ck, load_ema):
        torch.save(ck, path)
        c = load_config(cfg_path)
        c.training.load_ema = load_ema
        generation_main(c)
        return np.load(out)["arr_0"]
    run({"network_params": live_sd, "optimizer_params": {}}, False)         # warm-up: every compared run below is a repeat
    got = run({"network_params": live_sd, "optimizer_params": {}, "ema_network_params": ema_sd, "ema_num_updates": 5}, True)
    manual = run({"network_params": ema_sd, "optimizer_params": {}}, False)
    plain = run({"network_params": live_sd, "optimizer_params": {}, "ema_network_params": ema_sd, "ema_num_updates": 5}, False)
    fallback = run({"network_params": live_sd, "optimizer_params": {}}, True)
    assert np.isfinite(got).all()
    assert np.array_equal(got, manual)
    assert not np.array_equal(got, plain)
    assert np.array_equal(fallback, plain)


# 7. two ranks ----------------------------------------------------------------------------------------------------------------
def test_two_ranks_keep_identical_shadows(cfg_path, tmp_path):
    """two ranks over gloo on this one GPU (the rehearsal of test_gpu_pipeline.py): every rank averages its own replica; parameters
    are bit-identical after the all-reduce, so the shadows' parameters are too (BatchNorm statistics are per replica)"""
    import socket
    import subprocess
    import sys
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    code = ("import sys, os, torch; sys.path.insert(0, %r); from sbgm.utils import load_config\n"
            "cfg = load_config(%r)\n"
            "from sbgm_danra_amd.training_main import train_main\n"
            "cfg.training.epochs = 1; cfg.training.with_ema = True; cfg.training.ema_decay = 0.9; cfg.monitoring.extreme_prcp.enabled = False\n"
            "import sbgm_danra_amd.training as TR\n"
            "orig = TR.TrainingPipeline_general.train_batches\n"
            "def spy(self, *a, **k):\n"
            "    r = orig(self, *a, **k)\n"
            "    torch.save({'sd': {k_: v.cpu() for k_, v in self.ema_model.state_dict().items()}, 'n': self.ema.num_updates,\n"
            "                'graphs': len(getattr(self, '_graphs', {}))}, os.path.join(%r, 'rank%%s.pt' %% os.environ.get('RANK', '0')))\n"
            "    return r\n"
            "TR.TrainingPipeline_general.train_batches = spy\n"
            "train_main(cfg)\n") % (ROOT, cfg_path, str(tmp_path))
    base = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    base["SBGM_DIST_BACKEND"] = "gloo"
    procs = [subprocess.Popen([sys.executable, "-c", code], env=dict(base, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2",
                                                                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port)),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = [p.communicate(timeout=900)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(o[-2000:] for o in outs)
    a, b = (torch.load(os.path.join(str(tmp_path), f"rank{r}.pt"), weights_only=True) for r in range(2))
    assert a["graphs"] >= 1 and b["graphs"] >= 1 and a["n"] == b["n"] > 0
    for k in a["sd"]:
        if "running_" in k or "num_batches" in k:
            continue
        assert torch.equal(a["sd"][k], b["sd"][k]), k
    assert all(torch.isfinite(v).all() for v in a["sd"].values() if v.dtype.is_floating_point)
