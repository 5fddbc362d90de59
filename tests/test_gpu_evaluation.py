"""Verification kernels (csrc/verify.hip) against float64 numpy restatements written here, their statistical behaviour on
calibrated and under-dispersed Gaussian ensembles, and `--mode evaluate` end to end from generated npz files."""
import json
import math
import os

import numpy as np
import pytest
import torch
import yaml

from sbgm_danra_amd import verification as V

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda")
SHAPES = [(37, 53), (589, 789)]
ALIGNED = (32, 48)                       # H*W % 4 == 0: the f32x4 / uchar4 loads of the error-statistics kernel


def _data(rng, n, shape, nan_frac=0.01, scale=2.0, offset=1.0):
    a = (rng.standard_normal((n, *shape)) * scale + offset).astype(np.float32)
    a[rng.random(a.shape) < nan_frac] = np.nan
    return a


def _valid(g, o, m):
    v = ~np.isnan(g) & ~np.isnan(np.broadcast_to(o, g.shape))
    if m is not None:
        v &= np.broadcast_to(m, g.shape)
    return v


def ref_error_stats(gen, obs, mask):
    g = gen.astype(np.float64)
    o = np.broadcast_to(obs, gen.shape).astype(np.float64)
    v = _valid(gen, obs, mask)
    d = np.where(v, g - o, 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        cnt = v.sum(0)
        pix = dict(count=cnt, mae=np.abs(d).sum(0) / cnt, rmse=np.sqrt((d * d).sum(0) / cnt),
                   bias=np.where(v, g, 0).sum(0) / cnt - np.where(v, o, 0).sum(0) / cnt)
        sc = v.sum((1, 2))
        smp = dict(sample_count=sc, sample_mae=np.abs(d).sum((1, 2)) / sc, sample_rmse=np.sqrt((d * d).sum((1, 2)) / sc))
    gv, ov = g[v], o[v]
    glob = [v.sum(), gv.mean(), ov.mean(), gv.mean() - ov.mean(), np.abs(gv - ov).mean(), np.sqrt(((gv - ov) ** 2).mean()),
            gv.min(), gv.max(), ov.min(), ov.max()]
    return pix, smp, np.array(glob)


@pytest.mark.parametrize("shape", SHAPES + [ALIGNED])
@pytest.mark.parametrize("n,no,nm,mdtype", [(5, 1, 1, "u8"), (3, 3, 3, "f32"), (4, 4, 0, None), (1, 1, 1, "bool")])
def test_error_stats_matches_numpy(shape, n, no, nm, mdtype):
    rng = np.random.default_rng(hash((shape, n, no, nm)) % 2**32)
    gen, obs = _data(rng, n, shape), _data(rng, no, shape)
    mask = None
    mt = None
    if mdtype is not None:
        mask = rng.random((nm, *shape)) < 0.7
        mt = torch.from_numpy(mask).to(DEV)
        mt = mt.to(torch.uint8) if mdtype == "u8" else (mt.float() if mdtype == "f32" else mt)
    got = V.error_stats(torch.from_numpy(gen).to(DEV), torch.from_numpy(obs).to(DEV), mt)
    pix, smp, glob = ref_error_stats(gen, obs, mask)
    np.testing.assert_array_equal(got["count"].cpu().numpy(), pix["count"])
    for k in ("mae", "rmse", "bias"):
        np.testing.assert_allclose(got[k].cpu().numpy(), pix[k], rtol=1e-6, atol=1e-6, equal_nan=True, err_msg=k)
    np.testing.assert_array_equal(got["sample_count"].cpu().numpy(), smp["sample_count"])
    for k in ("sample_mae", "sample_rmse"):
        np.testing.assert_allclose(got[k].cpu().numpy(), smp[k], rtol=1e-6, err_msg=k)
    g = got["global"].cpu().numpy()
    assert g[0] == glob[0]
    np.testing.assert_allclose(g[1:], glob[1:], rtol=1e-6, atol=1e-9)


def test_error_stats_all_invalid_pixel_is_nan():
    gen = torch.full((2, 37, 53), float("nan"), device=DEV)
    got = V.error_stats(gen, torch.zeros(1, 37, 53, device=DEV))
    assert int(got["count"].sum()) == 0 and torch.isnan(got["mae"]).all() and torch.isnan(got["global"][1:]).all()


def ref_histogram(x, bins, lo, hi, ref=None, mask=None, absdiff=False):
    v = ~np.isnan(x)
    if ref is not None:
        v = _valid(x, ref, mask)
        if absdiff:
            x = np.abs(x - np.broadcast_to(ref, x.shape)).astype(np.float32)
    elif mask is not None:
        v &= np.broadcast_to(mask, x.shape)
    xv = x[v].astype(np.float64)
    xv = xv[(xv >= lo) & (xv <= hi)]
    idx = np.minimum(np.floor((xv - lo) * bins / (hi - lo)).astype(np.int64), bins - 1)
    return np.bincount(idx, minlength=bins)


@pytest.mark.parametrize("shape", SHAPES + [ALIGNED])
def test_histogram_matches_numpy(shape):
    rng = np.random.default_rng(7)
    x, ref = _data(rng, 3, shape), _data(rng, 1, shape)
    mask = rng.random((3, *shape)) < 0.6
    xd, rd, md = (torch.from_numpy(a).to(DEV) for a in (x, ref, mask))
    for kw, want in [(dict(), ref_histogram(x, 150, -3.0, 4.5)),
                     (dict(ref=rd, mask=md), ref_histogram(x, 150, -3.0, 4.5, ref, mask)),
                     (dict(mask=md), ref_histogram(x, 150, -3.0, 4.5, mask=mask))]:
        np.testing.assert_array_equal(V.histogram(xd, 150, -3.0, 4.5, **kw).cpu().numpy(), want)
    got = V.histogram(xd, 70, 0.0, 6.0, ref=rd, absdiff=True).cpu().numpy()
    np.testing.assert_array_equal(got, ref_histogram(x, 70, 0.0, 6.0, ref, absdiff=True))


def test_histogram_bin_edges_and_closed_last_bin():
    """values exactly on the edges go to the bin they open; hi goes to the last bin; outside and NaN are dropped"""
    edges = np.linspace(-2.0, 2.0, 17)                  # multiples of 0.25: exact in fp32
    vals = np.concatenate([edges, [2.0, 2.0, -2.0, -2.0000002, 2.0000002, np.nan, 7.0]]).astype(np.float32)
    x = torch.from_numpy(vals).view(1, 1, -1).to(DEV)
    got = V.histogram(x, 16, -2.0, 2.0).cpu().numpy()
    want, _ = np.histogram(vals[~np.isnan(vals)], bins=16, range=(-2.0, 2.0))
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got, ref_histogram(vals.reshape(1, 1, -1), 16, -2.0, 2.0))
    assert got[-1] == 4 and got[0] == 2 and got.sum() == 17 + 3
    assert np.array_equal(V.histogram_edges(16, -2.0, 2.0).numpy(), edges)


def ref_ensemble(ens, obs, mask):
    e = ens.astype(np.float64).reshape(ens.shape[0], -1)
    y = obs.astype(np.float64).ravel()
    M = e.shape[0]
    valid = ~np.isnan(y) & ~np.isnan(e).any(0)
    if mask is not None:
        valid &= mask.ravel()
    s = np.sort(np.where(valid, e, 0.0), axis=0)
    i = np.arange(1, M + 1, dtype=np.float64)[:, None]
    pair = 2.0 * ((2 * i - M - 1) * s).sum(0)                  # sum_ij |x_i - x_j| (sorted form)
    t1 = np.abs(e - y).mean(0)
    fair, std = t1 - pair / (2 * M * (M - 1)), t1 - pair / (2 * M * M)
    mean, var = e.mean(0), e.var(0, ddof=1)
    lt, le = (e < y).sum(0), (e <= y).sum(0)
    nanv = np.full_like(y, np.nan)
    maps = dict(mean=np.where(valid, mean, nanv), var=np.where(valid, var, nanv), crps=np.where(valid, fair, nanv),
                lt=np.where(valid, lt, -1), le=np.where(valid, le, -1))
    skill = np.sqrt(((mean - y)[valid] ** 2).mean())
    spread = np.sqrt(var[valid].mean())
    scores = np.array([valid.sum(), fair[valid].mean(), std[valid].mean(), skill, spread, math.sqrt((M + 1) / M) * spread / skill])
    return maps, scores


@pytest.mark.parametrize("M,shape", [(2, (37, 53)), (3, (37, 53)), (17, (37, 53)), (64, (37, 53)), (257, (37, 53)),
                                     (1024, (37, 53)), (17, (589, 789))])
def test_ensemble_scores_match_numpy(M, shape):
    rng = np.random.default_rng(M)
    ens = _data(rng, M, shape, nan_frac=0.02 / M)
    obs = _data(rng, 1, shape, nan_frac=0.01)[0]
    mask = rng.random(shape) < 0.8
    got = V.ensemble_scores(torch.from_numpy(ens).to(DEV), torch.from_numpy(obs).to(DEV), torch.from_numpy(mask).to(DEV), seed=3)
    maps, scores = ref_ensemble(ens, obs, mask)
    for k in ("mean", "var", "crps"):
        np.testing.assert_allclose(got[k].cpu().numpy().ravel(), maps[k], rtol=1e-6, atol=1e-6, equal_nan=True, err_msg=k)
    rank = got["rank"].cpu().numpy().ravel()
    np.testing.assert_array_equal(rank, maps["lt"])            # continuous data: no ties, rank = #{x_i < y}
    np.testing.assert_array_equal(got["rank_hist"].cpu().numpy(), np.bincount(rank[rank >= 0], minlength=M + 1))
    s = got["scores"].cpu().numpy()
    assert s[0] == scores[0]
    np.testing.assert_allclose(s[1:], scores[1:], rtol=1e-6)


CHI2_CRIT_P1E3 = {8: 26.124, 32: 62.487}                       # chi-square quantiles at p = 1e-3


def _chi2(hist):
    e = hist.sum() / hist.size
    return float(((hist - e) ** 2 / e).sum())


def test_calibrated_gaussian_ensemble():
    g = torch.Generator(device=DEV).manual_seed(1234)
    mu, sigma, M = 3.0, 2.0, 32
    ens = mu + sigma * torch.randn(M, 256, 256, device=DEV, generator=g)
    obs = mu + sigma * torch.randn(256, 256, device=DEV, generator=g)
    r = V.ensemble_scores(ens, obs, seed=5)
    s = r["scores"].cpu().numpy()
    assert abs(s[1] / (sigma / math.sqrt(math.pi)) - 1.0) < 0.02, s
    h = r["rank_hist"].cpu().numpy()
    assert h.sum() == 256 * 256 and _chi2(h) < CHI2_CRIT_P1E3[32], h
    assert abs(s[5] - 1.0) < 0.05, s
    # under-dispersed: members with half the spread -> U-shaped rank histogram, spread/skill well below 1
    r2 = V.ensemble_scores(mu + 0.5 * (ens - mu), obs, seed=5)
    h2 = r2["rank_hist"].cpu().numpy()
    assert min(h2[0], h2[-1]) > 2 * h2[1:-1].mean(), h2
    assert r2["scores"][5].item() < 0.6


def test_ties_give_uniform_ranks():
    M = 8
    ens = torch.ones(M, 256, 256, device=DEV)
    r = V.ensemble_scores(ens, torch.ones(256, 256, device=DEV), seed=11)
    rank = r["rank"].cpu().numpy()
    assert rank.min() >= 0 and rank.max() <= M
    h = r["rank_hist"].cpu().numpy()
    assert _chi2(h) < CHI2_CRIT_P1E3[8], h
    assert float(r["crps"].abs().max()) == 0.0 and float(r["var"].abs().max()) == 0.0
    r2 = V.ensemble_scores(ens, torch.ones(256, 256, device=DEV), seed=12)
    assert not torch.equal(r["rank"], r2["rank"])              # another seed, other draws


def ref_rapsd_bins(power, H, W):
    L = max(H, W)
    fy, fx = np.fft.fftfreq(H), np.fft.fftfreq(W)
    k = np.rint(L * np.sqrt(fy[:, None] ** 2 + fx[None, :] ** 2)).astype(np.int64)
    keep = k <= L // 2
    tot = power.astype(np.float64).sum(0)
    s = np.bincount(k[keep], weights=tot[keep], minlength=L // 2 + 1)
    c = np.bincount(k[keep], minlength=L // 2 + 1)
    return s / (c * power.shape[0]), c


def test_rapsd_sinusoid_in_its_bin():
    H = W = 64
    x = torch.arange(W, dtype=torch.float64)
    f = torch.sin(2 * math.pi * 5 * x / W).expand(H, W).float().to(DEV)
    k, psd, skipped = V.rapsd(f[None])
    power = torch.fft.fft2(f - f.mean()).abs().square()
    _, cnt = ref_rapsd_bins(power[None].cpu().numpy(), H, W)
    tot = psd.cpu().numpy() * cnt
    assert int(skipped) == 0 and tot[5] / tot.sum() > 0.99


@pytest.mark.parametrize("shape", SHAPES)
def test_rapsd_random_fields_match_numpy(shape):
    H, W = shape
    rng = np.random.default_rng(H)
    fields = rng.standard_normal((3, H, W)).astype(np.float32)
    fields[1] = np.cumsum(fields[1], axis=1) * 0.1                    # a red spectrum next to white ones
    bad = fields.copy()
    bad[2, 5, 7] = np.nan
    t = torch.from_numpy(fields).to(DEV)
    k, psd, skipped = V.rapsd(t)
    # the binning, exactly, on the power the wrapper transforms
    x = t - t.mean(dim=(1, 2), keepdim=True)
    power = torch.fft.fft2(x).abs().square().float().cpu().numpy()
    want, _ = ref_rapsd_bins(power, H, W)
    np.testing.assert_allclose(psd.cpu().numpy(), want, rtol=1e-9)
    np.testing.assert_array_equal(k.cpu().numpy(), np.arange(max(H, W) // 2 + 1))
    # and against a float64 numpy FFT
    f64 = fields.astype(np.float64)
    p64 = np.abs(np.fft.fft2(f64 - f64.mean(axis=(1, 2), keepdims=True))) ** 2
    want64, _ = ref_rapsd_bins(p64, H, W)
    np.testing.assert_allclose(psd.cpu().numpy(), want64, rtol=2e-3, atol=1e-6 * want64.max())     # bin 0: mean removed, ~0
    # a field with a NaN is skipped and counted, never zero-filled into the mean
    _, psd_b, skipped_b = V.rapsd(torch.from_numpy(bad).to(DEV))
    _, psd_2, _ = V.rapsd(t[:2])
    assert int(skipped) == 0 and int(skipped_b) == 1
    assert torch.equal(psd_b, psd_2)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else (t.view(torch.int64) if t.dtype == torch.float64 else t)


def test_bitwise_reproducible():
    rng = np.random.default_rng(0)
    gen, obs = (torch.from_numpy(_data(rng, n, (589, 789))).to(DEV) for n in (8, 1))
    mask = torch.from_numpy(rng.random((589, 789)) < 0.7).to(DEV)
    calls = [lambda: V.error_stats(gen, obs, mask), lambda: {"h": V.histogram(gen, 150, -5, 7, ref=obs, mask=mask)},
             lambda: V.ensemble_scores(gen, obs[0], mask, seed=9), lambda: dict(zip("kps", V.rapsd(torch.nan_to_num(gen))))]
    for call in calls:
        a, b = call(), call()
        for key in a:
            assert torch.equal(_bits(a[key]), _bits(b[key])), key


def test_argument_checks_before_launch():
    x = torch.zeros(3, 8, 8, device=DEV)
    with pytest.raises(ValueError):
        V.error_stats(x, torch.zeros(2, 8, 8, device=DEV))
    with pytest.raises(ValueError):
        V.ensemble_scores(x[:1], x[0])
    with pytest.raises(ValueError):
        V.histogram(x, 10, 1.0, 1.0)
    with pytest.raises(ValueError):
        V.histogram(x, 10, 0.0, 1.0, absdiff=True)
    with pytest.raises(RuntimeError):
        V.error_stats(x.cpu(), x.cpu())


# ---- --mode evaluate end to end ---------------------------------------------------------------------------------------------

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
    raw["evaluation"].update(batch_size=3, gen_type=["multiple", "single", "repeated"], n_repeats=3, mask_stats=True,
                             save_stats=True, eval_stat_methods=["pixel_stats", "spatial_stats", "daily_stats", "spectral_stats"])
    raw["training"]["batch_size"] = 2
    p = tmp_path / "run.yaml"
    p.write_text(yaml.safe_dump(raw))
    return str(p)


def _checkpoint(cfg):
    from oracle import torch_ref as O
    from sbgm.utils import get_model_string
    ora = O.build_scorenet(6, num_classes=4)
    ckpt_dir = os.path.join(cfg.paths.path_save, cfg.paths.checkpoint_dir)
    os.makedirs(ckpt_dir, exist_ok=True)
    torch.save({"network_params": O.synth_state_dict(ora), "optimizer_params": {}}, os.path.join(ckpt_dir, get_model_string(cfg) + ".pth.tar"))


def _check_unit(stats, samples, label, suffix, ensemble):
    g = np.load(os.path.join(samples, f"gen_samples_{suffix}.npz"))["arr_0"].astype(np.float32)
    o = np.load(os.path.join(samples, f"eval_samples_{suffix}.npz"))["arr_0"][:, 0].astype(np.float32)
    m = np.load(os.path.join(samples, f"lsm_samples_{suffix}.npz"))["arr_0"][:, 0] > 0.5
    met = json.load(open(os.path.join(stats, f"{label}_metrics.json")))
    fld = np.load(os.path.join(stats, f"{label}_fields.npz"))
    pix, smp, glob = ref_error_stats(g, o, m)
    assert met["pixel_stats"]["count"] == glob[0] and met["mask_stats"] is True
    got = [met["pixel_stats"][k] for k in V.GLOBAL_KEYS[1:]]
    np.testing.assert_allclose(got, glob[1:], rtol=1e-6, atol=1e-9)
    np.testing.assert_array_equal(fld["spatial_count_per_pixel"], pix["count"])
    np.testing.assert_allclose(fld["spatial_rmse_per_pixel"], pix["rmse"], rtol=1e-6, atol=1e-7, equal_nan=True)
    np.testing.assert_allclose(fld["daily_mae"], smp["sample_mae"], rtol=1e-6, equal_nan=True)
    lo, hi = min(glob[6], glob[8]), max(glob[7], glob[9])
    np.testing.assert_array_equal(fld["pixel_hist_gen"], ref_histogram(g, 150, lo, hi, o, m))
    f64 = g.astype(np.float64)
    p64 = np.abs(np.fft.fft2(f64 - f64.mean(axis=(1, 2), keepdims=True))) ** 2
    want = ref_rapsd_bins(p64, 64, 64)[0]
    np.testing.assert_allclose(fld["spectral_psd_gen"], want, rtol=2e-3, atol=1e-6 * want.max())
    if ensemble:
        maps, scores = ref_ensemble(g, o[0], m[0])
        assert met["ensemble_stats"]["M"] == g.shape[0] and met["ensemble_stats"]["crps_map"] == "crps_fair"
        np.testing.assert_allclose([met["ensemble_stats"][k] for k in V.ENSEMBLE_KEYS[1:]], scores[1:], rtol=1e-6)
        assert fld["ensemble_rank_hist"].sum() == scores[0]


def test_cli_generate_then_evaluate(cfg_path):
    from sbgm.cli import main_app
    from sbgm.utils import get_model_string, load_config
    cfg = load_config(cfg_path)
    _checkpoint(cfg)
    main_app.main(["--config_path", cfg_path, "--mode", "generate"])
    main_app.main(["--config_path", cfg_path, "--mode", "evaluate"])
    samples = os.path.join(cfg.paths.sample_dir, "generation", get_model_string(cfg), "generated_samples")
    stats = os.path.join(cfg.paths.sample_dir, "evaluation", get_model_string(cfg), "statistics")
    for label, suffix in (("multiple", "multi_n_3"), ("single", "single"), ("repeated", "repeated_n_3")):
        _check_unit(stats, samples, label, suffix, ensemble=False)
    assert os.path.exists(os.path.join(stats, "n_samples_3_pixel_statistics.npz"))
    assert set(np.load(os.path.join(stats, "n_samples_3_RMSE_MAE_statistics.npz"))) == {"mae_all", "rmse_all"}
    # the ensemble scores of the repeated samples, through the config keys
    raw = yaml.safe_load(open(cfg_path))
    raw["evaluation"].update(eval_gen_type=["repeated"], eval_stat_methods=["pixel_stats", "spatial_stats", "daily_stats",
                                                                            "spectral_stats", "ensemble_stats"])
    open(cfg_path, "w").write(yaml.safe_dump(raw))
    main_app.main(["--config_path", cfg_path, "--mode", "evaluate"])
    _check_unit(stats, samples, "repeated", "repeated_n_3", ensemble=True)
    # full_pipeline without --skip_evaluation writes them too
    for f in os.listdir(stats):
        os.remove(os.path.join(stats, f))
    main_app.main(["--config_path", cfg_path, "--mode", "full_pipeline", "--skip_train"])
    _check_unit(stats, samples, "repeated", "repeated_n_3", ensemble=True)
