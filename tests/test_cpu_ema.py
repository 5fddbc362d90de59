"""Host-side logic of training.with_ema (sbgm_danra_amd/ema.py): the decay schedule, the config keys, the checkpoint keys on CPU
state_dicts, ScoreNet deep copies, and the C ABI of the EMA launches (symbols only; the kernels run in test_gpu_ema.py)."""
import copy
import logging
import os
import re

import pytest
import torch
import torch.nn as nn
import yaml

import sbgm_danra_amd as S
from sbgm_danra_amd import _native as N
from sbgm_danra_amd.ema import EMA_COUNT_KEY, EMA_KEY, ModelEMA, decay_at, pick_network_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _net():
    torch.manual_seed(0)
    enc = S.Encoder(1, 64, block_layers=[1, 1, 1, 1], n_heads=2)
    dec = S.Decoder(512, 1, 64, n_heads=2, norm="group", gn_groups=8, activation=nn.SiLU)
    return S.ScoreNet(S.marginal_prob_std_fn, enc, dec, device=torch.device("cpu"), debug_pre_sigma_div=False)


def test_decay_schedule_warms_up_then_caps():
    assert decay_at(0.9999, 1) == pytest.approx(2 / 11)
    assert decay_at(0.9999, 10) == pytest.approx(11 / 20)
    seq = [decay_at(0.9999, n) for n in range(1, 100000)]
    assert all(a <= b for a, b in zip(seq, seq[1:]))
    assert seq[-1] == 0.9999 and max(seq) == 0.9999
    assert decay_at(0.95, 200) == 0.95 and decay_at(0.95, 17) == pytest.approx(18 / 27)
    with pytest.raises(ValueError):
        ModelEMA(_net(), 1.5)


def test_config_defaults():
    raw = yaml.safe_load(open(os.path.join(ROOT, "sbgm_danra_amd", "config", "default_config.yaml")))
    t = raw["training"]
    assert t["with_ema"] is False and t["load_ema"] is False and t["ema_decay"] == 0.9999
    keys = list(t)
    assert keys.index("ema_decay") == keys.index("load_ema") + 1          # next to the other EMA switches


def test_checkpoint_key_selection(caplog):
    live, ema = {"w": torch.zeros(2)}, {"w": torch.ones(2)}
    ck = {"network_params": live, "optimizer_params": {}, EMA_KEY: ema, EMA_COUNT_KEY: 4}
    assert pick_network_params(ck, True) is ema
    assert pick_network_params(ck, False) is live
    old = {"network_params": live, "optimizer_params": {}}
    with caplog.at_level(logging.WARNING):
        assert pick_network_params(old, False) is live
        assert not caplog.records
        assert pick_network_params(old, True, "x.pth.tar") is live
    assert EMA_KEY in caplog.text and "x.pth.tar" in caplog.text


def test_ema_state_round_trip_on_cpu_state_dicts():
    net = _net()
    ema = ModelEMA(net, 0.99)
    sd = ema.state_dict()                                     # before training: the live weights, zero updates
    assert sd["num_updates"] == 0 and set(sd["network_params"]) == set(net.state_dict())
    other = {k: (v + 1 if v.dtype.is_floating_point else v + 7) for k, v in net.state_dict().items()}
    ema.load_state_dict({"network_params": other, "num_updates": 12})
    assert ema.num_updates == 12 and ema.loaded
    assert isinstance(ema.shadow, S.ScoreNet) and not ema.shadow.training
    assert not any(p.requires_grad for p in ema.shadow.parameters())
    assert all(torch.equal(ema.shadow.state_dict()[k], v) for k, v in other.items())
    assert not torch.equal(net.encoder.conv1.weight, ema.shadow.encoder.conv1.weight)
    ema.start()                                               # a restored average is kept when training starts
    assert ema.num_updates == 12 and torch.equal(ema.shadow.encoder.conv1.weight, other["encoder.conv1.weight"])
    assert ema.advance() == pytest.approx(1 - 14 / 23) and ema.num_updates == 13     # still in the warm-up
    fresh = ModelEMA(net, 0.99)
    fresh.start()                                             # no average yet: the shadow starts as the live weights
    assert all(torch.equal(fresh.shadow.state_dict()[k], v) for k, v in net.state_dict().items())
    assert all(a.data_ptr() != b.data_ptr() for a, b in zip(fresh.shadow.parameters(), net.parameters()))
    with pytest.raises(N.NativeError):                        # the update itself is native only
        fresh.update()


def test_scorenet_deepcopy_does_not_share_engines():
    net = _net()
    sentinel = object()
    net._engines[(0, 0, 0)] = sentinel
    object.__setattr__(net, "_grad_arena", sentinel)
    cp = copy.deepcopy(net)
    assert cp._engines == {} and cp._engines is not net._engines
    assert getattr(cp, "_grad_arena", None) is None
    assert net._engines[(0, 0, 0)] is sentinel and net._grad_arena is sentinel
    assert list(cp.state_dict()) == list(net.state_dict())
    assert all(torch.equal(a, b) and a.data_ptr() != b.data_ptr() for a, b in zip(cp.state_dict().values(), net.state_dict().values()))
    assert cp.encoder is not net.encoder and cp.marginal_prob_std is not None


def test_ema_entry_points_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "sbgm_hip.h")).read()
    for name in ("sbgm_adam_ema_step_batched", "sbgm_ema_update_batched"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in N.SIGNATURES
        assert hasattr(N.lib(), name)


def test_pipeline_checkpoint_keys_on_cpu(tmp_path, monkeypatch):
    from sbgm.score_unet import diffusion_coeff_fn, loss_fn, marginal_prob_std_fn
    from sbgm.training import TrainingPipeline_general
    from sbgm.utils import load_config
    for k in ("DATA_DIR", "CKPT_DIR", "SAMPLE_DIR", "STATS_LOAD_DIR"):
        monkeypatch.setenv(k, str(tmp_path / k.lower()))
    cfg = load_config(os.path.join(ROOT, "sbgm_danra_amd", "config", "default_config.yaml"))

    def pipe(with_ema):
        cfg.training.with_ema = with_ema
        net = _net()
        return net, TrainingPipeline_general(net, loss_fn, marginal_prob_std_fn, diffusion_coeff_fn,
                                             torch.optim.SGD(net.parameters(), lr=1e-3), torch.device("cpu"), None, cfg)
    net, off = pipe(False)
    assert off.ema is None and off.ema_model is None
    off.save_model(str(tmp_path), "off.pth")
    assert set(torch.load(tmp_path / "off.pth", weights_only=True)) == {"network_params", "optimizer_params"}
    net, on = pipe(True)
    assert on.ema.decay == 0.9999 and on.ema_model is None      # built when training starts, not in __init__
    on.save_model(str(tmp_path), "on.pth")
    ck = torch.load(tmp_path / "on.pth", weights_only=True)
    assert set(ck) == {"network_params", "optimizer_params", EMA_KEY, EMA_COUNT_KEY} and ck[EMA_COUNT_KEY] == 0
    ck[EMA_KEY] = {k: (v * 2 if v.dtype.is_floating_point else v) for k, v in ck[EMA_KEY].items()}
    ck[EMA_COUNT_KEY] = 9
    torch.save(ck, tmp_path / "on.pth")
    net2, on2 = pipe(True)
    on2.load_checkpoint(str(tmp_path / "on.pth"), load_ema=True)
    assert on2.ema.num_updates == 9
    assert all(torch.equal(net2.state_dict()[k], v) for k, v in ck[EMA_KEY].items())
    assert all(torch.equal(on2.ema_model.state_dict()[k], v) for k, v in ck[EMA_KEY].items())
    net3, off2 = pipe(False)
    off2.load_checkpoint(str(tmp_path / "on.pth"))             # EMA off: the extra keys are ignored
    assert off2.ema is None and all(torch.equal(net3.state_dict()[k], v) for k, v in ck["network_params"].items())
