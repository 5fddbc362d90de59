"""Row-keyed, temporally correlated in-kernel noise on the device, against the float32 mixing loop of
temporal_noise_ref.py over what sbgm_randn_scaled draws.

(5) the op, bit for bit                    (6) every consumer: a seeded run under a plan equals the run on injected mixed draws, exact
(7) the noise of a day does not depend on its batch, and is the sum of mixed draws     (8) refusals leave the handle usable
(9) `gen_type: series` with `evaluation.series.seed` / `temporal_noise`: reproducible, extensible, and as before without the keys;
    the same with a `constraint:` section, where the series seed must still reach the sampler

Everything is exact except the two sums of (7): the bound 1e-5 max|want| of the tile-noise test for three float32 multiply-adds against
their float64 sum, and 1e-6 relative for the one float32 multiply of the ODE start (its scale an ulp apart at most).
Measured on MI355X: every exact comparison holds as stated; (7) 1.56e-07 of max |want| against the bound 1e-5."""
import math
import os

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu

import temporal_noise_ref as R  # noqa: E402
from util_models import build_pair, maxrel  # noqa: E402

import sbgm_danra_amd as S  # noqa: E402
from sbgm_danra_amd import _native as N  # noqa: E402
from sbgm_danra_amd import score_sampling as SS  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
STD = (S.marginal_prob_std_fn, S.diffusion_coeff_fn)
W3 = SS.temporal_noise_weights(0.6, 3)


def device_draw(seed, draw, n):
    """what sbgm_randn_scaled writes for (seed, draw): float32 numpy [n]"""
    x = torch.empty(n, device=DEV)
    N.check(N.lib().sbgm_randn_scaled(x.data_ptr(), 1.0, seed, draw, n, N.stream()))
    return x.cpu().numpy()


def mixed(seed, draw, rows, per, w, stride):
    """the definition: the float32 loop over the device's own white draws -> numpy float32 [len(rows), per]"""
    return R.mix_rows(device_draw(seed, draw, (max(rows) + 1) * per), rows, per, w, stride)


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


# ---- (5) the op ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per", [8, 1024])
@pytest.mark.parametrize("seed", [1234, (1 << 32) + 5])
@pytest.mark.parametrize("draw", [0, (1 << 32) + 3])
def test_op_is_the_float32_mix_of_plain_draws(per, seed, draw):
    rows, stride = [7, 5, 12], 2
    got = SS.temporal_noise(seed, draw, rows, per, W3, stride)
    assert got.shape == (3, per) and got.dtype == torch.float32 and got.is_cuda
    plain = device_draw(seed, draw, 13 * per)
    want = R.mix_rows(plain, rows, per, W3, stride)
    assert np.array_equal(bits(got.cpu().numpy()), bits(want)), f"{int((bits(got.cpu().numpy()) != bits(want)).sum())} of {want.size} differ"
    assert not np.array_equal(want[0], plain[7 * per:8 * per])                           # the lags did enter
    # one lag of weight 1: the three slices of the plain draw; rows 0 .. B-1: the plain draw whole
    one = SS.temporal_noise(seed, draw, rows, per).cpu().numpy()
    assert np.array_equal(bits(one), bits(np.stack([plain[r * per:(r + 1) * per] for r in rows])))
    whole = SS.temporal_noise(seed, draw, torch.arange(13), per, [1.0], 1).cpu().numpy()
    assert np.array_equal(bits(whole.reshape(-1)), bits(plain))
    # the scale is one exact multiply
    assert torch.equal(SS.temporal_noise(seed, draw, rows, per, W3, stride, scale=2.0), 2.0 * got)


# ---- (6) every consumer ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net():
    _, n, _ = build_pair(1)
    return n.eval()


KINDS = {"em": (S.Euler_Maruyama_sampler, N.SAMPLER_EM, {}, 5), "pc": (S.pc_sampler, N.SAMPLER_PC, {}, 9),
         "edm": (S.edm_heun_sampler, N.SAMPLER_EDM_HEUN, dict(s_churn=40.0), 5),
         "dpm": (S.dpmpp_2m_sampler, N.SAMPLER_DPMPP_2M, dict(eta=1.0), 5)}


@pytest.mark.parametrize("held", [False, True])
@pytest.mark.parametrize("kind", list(KINDS))
def test_seeded_run_under_a_plan_equals_the_run_on_injected_mixed_draws(net, kind, held):
    sampler, code, kw, need = KINDS[kind]
    B, hw, steps, seed, stride = 2, 32, 4, 1234 + (7 << 32), 3
    per = hw * hw
    assert SS._counts(code, steps, True)[1] == need
    cond = rnd(B, 1, hw, hw, seed=11)
    if held:
        kw = dict(kw, known=rnd(B, 1, hw, hw, seed=12), known_mask=soft_mask(B, 1, hw, hw))
    run = lambda **how: sampler(net, *STD, batch_size=B, num_steps=steps, device=DEV, img_size=hw, cond_img=cond, **kw, **how)  # noqa: E731
    results = []
    for rows in ([9, 6], [12, 7]):                     # the second call: other contents at the same rows address
        D = torch.stack([torch.from_numpy(mixed(seed, i, rows, per, W3, stride)).view(B, 1, hw, hw) for i in range(need)]).to(DEV)
        want = run(noise=D)
        assert torch.isfinite(want).all()
        for graph in (True, False):
            got = run(seed=seed, use_graph=graph, noise_rows=rows, noise_weights=W3, noise_row_stride=stride)
            assert torch.equal(got, want), (f"{kind} held={held} rows={rows} use_graph={graph}: the run under the plan differs from the run "
                                            f"on the mixed draws 0..{need - 1}, max-rel {maxrel(got, want):.3e}")
        results.append(want)
    assert not torch.equal(results[0], results[1])
    # rows 0 .. B-1 with one lag of weight 1 draw what a run without a plan draws (and another graph serves it)
    plain = run(seed=seed)
    assert torch.equal(run(seed=seed, noise_rows=list(range(B)), noise_weights=[1.0]), plain)
    assert torch.equal(run(seed=seed, noise_rows=torch.arange(B), use_graph=False), plain)
    assert not torch.equal(plain, results[0])


# ---- (7) the noise of a day does not depend on its batch ---------------------------------------------------------------------------------
def test_noise_of_a_day_is_independent_of_its_batch_and_is_the_sum_of_mixed_draws():
    _, znet, _ = build_pair(1)
    znet.eval()
    fin = znet.decoder.final_layer.conv
    with torch.no_grad():                                                 # score == 0 exactly: the state is a sum of draws
        fin.weight.zero_()
        fin.bias.zero_()
    hw, seed, steps, K = 32, 21 + (3 << 32), 3, 3
    per = hw * hw
    rows = [d + K - 1 for d in range(4)]                                  # days 0..3, one member
    cond = rnd(4, 1, hw, hw, seed=13)
    run = lambda sl: S.Euler_Maruyama_sampler(znet, *STD, batch_size=len(rows[sl]), num_steps=steps, device=DEV, img_size=hw,  # noqa: E731
                                              cond_img=cond[sl], seed=seed, noise_rows=rows[sl], noise_weights=W3)
    one = run(slice(0, 4))
    two = torch.cat([run(slice(0, 2)), run(slice(2, 4))])
    assert torch.equal(one, two)
    # the coefficients as the Python loop computes them: std(1), then g(t_i) sqrt(dt) of the steps whose draw reaches the last mean_x
    ones = torch.ones(4, device=DEV)
    ts = torch.linspace(1.0, 1e-3, steps, device=DEV)
    dt = float(ts[0] - ts[1])
    coef = [float(S.marginal_prob_std_fn(ones)[0])] + [math.sqrt(dt) * float(S.diffusion_coeff_fn(ones * tt)[0]) for tt in ts.tolist()[:-1]]
    mixes = [mixed(seed, i, rows, per, W3, 1).astype(np.float64) for i in range(steps)]
    want = torch.from_numpy(sum(c * m for c, m in zip(coef, mixes))).view(4, 1, hw, hw).to(DEV)
    err = float((one.double() - want).abs().max() / want.abs().max())
    print(f"row-keyed noise: max |got - want| / max |want| = {err:.2e} over 4 days")
    assert err <= 1e-5
    # consecutive days share K - 1 white rows: their states are correlated, day 0 and day 3 (no row in common) are not
    c01 = float(torch.corrcoef(torch.stack([one[0].flatten(), one[1].flatten()]))[0, 1])
    c03 = float(torch.corrcoef(torch.stack([one[0].flatten(), one[3].flatten()]))[0, 1])
    acf1 = float(SS.temporal_noise_acf(W3)[1])
    assert abs(c01 - acf1) <= 5 * 1.5 / math.sqrt(per) and abs(c03) <= 5 / math.sqrt(per)
    # the initial state, read through the ODE sampler: with a zero score its right-hand side is zero and the result is the start
    x0 = S.rk45_sampler(znet, *STD, batch_size=4, device=DEV, img_size=hw, cond_img=cond, seed=seed, noise_rows=rows, noise_weights=W3)
    start = torch.from_numpy(mixes[0]).view(4, 1, hw, hw).to(DEV)
    assert maxrel(x0.double(), coef[0] * start) <= 1e-6


# ---- (8) refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(net):
    B, hw, steps, seed = 2, 32, 2, 5
    cond = rnd(B, 1, hw, hw, seed=14)
    run = lambda **how: S.Euler_Maruyama_sampler(net, *STD, batch_size=B, num_steps=steps, device=DEV, img_size=hw, cond_img=cond,  # noqa: E731
                                                 seed=seed, **how)
    before = run()
    origins = torch.tensor([[0, 0], [0, 24]], dtype=torch.int32, device=DEV)
    plan = dict(noise_rows=[4, 5], noise_weights=W3)
    for how in (dict(plan, tile_origins=origins, domain_width=56), dict(plan, tile_origins=origins, domain_width=56, joint_tiles=(32, 8)),
                dict(plan, noise=torch.zeros(3, B, 1, hw, hw)), dict(noise_rows=[4, 5], noise_weights=[0.6, 0.7]),
                dict(noise_rows=[40, 41], noise_weights=np.full(33, 33 ** -0.5)), dict(plan, noise_rows=[4, 1])):
        with pytest.raises(ValueError):
            run(**how)
        assert torch.equal(run(), before)
    # the engine's own refusals (a direct C call): the plan stays with the handle until cleared, and a cleared handle runs as before
    eng = net._engine(None, None, cond)
    lib, rows = N.lib(), torch.tensor([4, 5], dtype=torch.int32, device=DEV)
    w = (N.C.c_float * 3)(*W3.tolist())
    for bad in ((rows.data_ptr(), 1, w, 33), (rows.data_ptr(), 0, w, 3), (None, 1, w, 2)):
        assert lib.sbgm_sampler_set_noise_rows(eng.h, *bad) != 0
    N.check(lib.sbgm_sampler_set_noise_rows(eng.h, rows.data_ptr(), 1, w, 3))
    try:
        with pytest.raises(N.NativeError, match="injected noise"):
            run(noise=torch.zeros(3, B, 1, hw, hw))
        with pytest.raises(N.NativeError, match="tile_origins"):
            run(tile_origins=origins, domain_width=56)
        held_plan = run()
    finally:
        N.check(lib.sbgm_sampler_set_noise_rows(eng.h, None, 1, None, 0))
    assert torch.equal(held_plan, run(**plan)) and torch.equal(run(), before)


# ---- (9) the pipeline --------------------------------------------------------------------------------------------------------------------
def _run(tmp_path, monkeypatch, tag, constraint=None, **series):
    """generation_main, gen_type series, on a tiny model (64 x 64, 4 steps of dpmpp_2m_sampler) over two loader batches of two days;
    `constraint`: the top-level `constraint:` section (the truth is then held on its mask)"""
    from oracle import torch_ref as O
    from sbgm_danra_amd.config_loader import load_config
    from sbgm_danra_amd.evaluate_sbgm.generation_main import generation_main
    from sbgm_danra_amd.synthetic_data import synthetic_loader
    from sbgm_danra_amd.utils import get_model_string
    for k in ("DATA_DIR", "CKPT_DIR", "STATS_LOAD_DIR"):
        monkeypatch.setenv(k, str(tmp_path / k.lower()))
    monkeypatch.setenv("SAMPLE_DIR", str(tmp_path / f"samples_{tag}"))
    monkeypatch.setenv("SLURM_CPUS_PER_TASK", "2")
    raw = yaml.safe_load(open(os.path.join(ROOT, "sbgm_danra_amd", "config", "default_config.yaml")))
    raw["highres"]["data_size"] = [64, 64]
    raw["lowres"]["data_size"] = [64, 64]
    raw["lowres"]["condition_variables"] = ["temp", "prcp"]
    raw["stationary_conditions"]["geographic_conditions"]["sample_w_geo"] = True
    raw["stationary_conditions"]["seasonal_conditions"]["sample_w_cond_season"] = True
    raw["sampler"]["n_timesteps"] = 4
    raw["sampler"]["sampler_type"] = "dpmpp_2m_sampler"
    raw["paths"]["evaluation_dir"] = str(tmp_path / f"ev_{tag}")
    if constraint is not None:
        raw["constraint"] = constraint
    raw["evaluation"].update(batch_size=2, n_repeats=4, seed=11, gen_type=["series"], series=series)
    p = tmp_path / f"run_{tag}.yaml"
    p.write_text(yaml.safe_dump(raw))
    cfg = load_config(str(p))
    ckpt_dir = os.path.join(cfg.paths.path_save, cfg.paths.checkpoint_dir)
    os.makedirs(ckpt_dir, exist_ok=True)
    ckpt = os.path.join(ckpt_dir, get_model_string(cfg) + ".pth.tar")
    if not os.path.exists(ckpt):
        torch.save({"network_params": O.synth_state_dict(O.build_scorenet(6, num_classes=4)), "optimizer_params": {}}, ckpt)
    generation_main(cfg, dataloader=synthetic_loader(cfg, 2, n_items=4, seed=5))
    return os.path.join(cfg.paths.sample_dir, "generation", get_model_string(cfg), "generated_samples")


def _arr(folder, name):
    return np.load(os.path.join(folder, name))["arr_0"]


def test_series_generation_with_day_keyed_noise(tmp_path, monkeypatch):
    series = {"members": 2, "seed": 20240229, "temporal_noise": {"rho": 0.6, "lags": 4}}
    a = _run(tmp_path, monkeypatch, "a", **series)
    gen = _arr(a, "gen_samples_series_n_4.npz")
    assert gen.shape == (4, 2, 64, 64) and gen.dtype == np.float32 and np.isfinite(gen).all()
    assert _arr(a, "eval_samples_series_n_4.npz").shape == (4, 64, 64)
    index = dict(np.load(os.path.join(a, "series_index_series_n_4.npz")))
    w = SS.temporal_noise_weights(0.6, 4)
    assert int(index["members"]) == 2 and int(index["seed"]) == 20240229
    assert index["weights"].dtype == np.float32 and np.array_equal(index["weights"], w)
    assert index["acf"].dtype == np.float64 and np.array_equal(index["acf"], SS.temporal_noise_acf(w))
    for d in range(4):
        assert (gen[d, 0] != gen[d, 1]).mean() > 0.99                          # members differ
    b = _run(tmp_path, monkeypatch, "b", **series)                            # the series seed: the same bits
    np.testing.assert_array_equal(_arr(b, "gen_samples_series_n_4.npz").view(np.int32), gen.view(np.int32))
    c = _run(tmp_path, monkeypatch, "c", max_days=2, **series)                # a shorter series is the head of the longer one
    np.testing.assert_array_equal(_arr(c, "gen_samples_series_n_2.npz").view(np.int32), gen[:2].view(np.int32))
    d_ = _run(tmp_path, monkeypatch, "d", **dict(series, seed=20240301))      # another seed: another series
    assert (_arr(d_, "gen_samples_series_n_4.npz") != gen).mean() > 0.99
    e = _run(tmp_path, monkeypatch, "e", members=2)                           # without the two keys: the index file as it was
    assert set(np.load(os.path.join(e, "series_index_series_n_4.npz")).files) <= {"members", "hr_points"}
    assert _arr(e, "gen_samples_series_n_4.npz").shape == (4, 2, 64, 64)


def test_series_with_a_constraint_keeps_its_day_keyed_noise(tmp_path, monkeypatch):
    """the plan and the `constraint:` section compose: the truth is held on the mask AND the noise is the series seed's, keyed by day"""
    series = {"members": 2, "seed": 77, "temporal_noise": {"rho": 0.6, "lags": 4}}
    con = {"enabled": True, "station_fraction": 0.05, "seed": 3}
    a = _run(tmp_path, monkeypatch, "ca", constraint=con, **series)
    gen, truth, mask = _arr(a, "gen_samples_series_n_4.npz"), _arr(a, "eval_samples_series_n_4.npz"), _arr(a, "constraint_mask_series_n_4.npz")
    assert gen.shape == (4, 2, 64, 64) and np.isfinite(gen).all() and 0 < (mask == 1).sum() < mask.size
    held = np.broadcast_to(mask == 1, gen.shape)
    np.testing.assert_array_equal(gen[held], np.broadcast_to(truth[:, None], gen.shape)[held])        # held pixels: the truth itself
    assert int(np.load(os.path.join(a, "series_index_series_n_4.npz"))["seed"]) == 77
    b = _run(tmp_path, monkeypatch, "cb", constraint=con, **series)           # a second run reproduces the series
    np.testing.assert_array_equal(_arr(b, "gen_samples_series_n_4.npz").view(np.int32), gen.view(np.int32))
    c = _run(tmp_path, monkeypatch, "cc", constraint=con, max_days=2, **series)
    np.testing.assert_array_equal(_arr(c, "gen_samples_series_n_2.npz").view(np.int32), gen[:2].view(np.int32))
    # the series seed does reach the sampler: another seed gives other free pixels (the process seed, evaluation.seed, is the same)
    d_ = _arr(_run(tmp_path, monkeypatch, "cd", constraint=con, **dict(series, seed=78)), "gen_samples_series_n_4.npz")
    assert (d_[~held] != gen[~held]).mean() > 0.99
    np.testing.assert_array_equal(d_[held], gen[held])
