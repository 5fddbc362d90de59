"""GPU suite for `gen_type: [series]` under an `evaluation.full_domain` section: generation_main on a tiny seeded model over a
generation split written to a temporary .npz, against `FullDomainTiler.sample_series` called directly on conditions built with torch
from the same arrays; then `--mode evaluate` on what it wrote.

Geometry: domain 44 x 53, tile 32, halo 4 (Wd_pad = 56, 4 tiles: a padded width, overlaps on both axes); 4 days, 2 members, 3 steps;
two LR conditions, the land-sea mask and the topography as value||mask pairs, a class per day.  The fields are served raw
(transforms.scaling false: the transform programs are pinned by tests/test_gpu_domain_gather.py), so the conditions torch builds are the
loader's bit for bit, and every comparison below is exact."""
import json
import os

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HD, WD, WP, TILE, HALO, DAYS, MEMBERS, STEPS = 44, 53, 56, 32, 4, 4, 2, 3
SEED = 20240229 + (1 << 34)
SERIES = {"members": MEMBERS, "seed": SEED, "temporal_noise": {"rho": 0.6, "lags": 3}}
_CACHE = {}


def arrays():
    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[0:HD, 0:WD]
    return {"prcp_hr": rng.normal(0, 1, (DAYS, HD, WD)).astype(np.float32), "temp_lr": rng.normal(0, 1, (DAYS, HD, WD)).astype(np.float32),
            "prcp_lr": rng.normal(0, 1, (DAYS, HD, WD)).astype(np.float32),
            "lsm": np.where((yy + xx) % 7 == 0, 0.3, ((yy - 20) ** 2 + (xx - 30) ** 2 < 150)).astype(np.float32),
            "topo": rng.random((HD, WD), dtype=np.float32), "classifier": (np.arange(DAYS) % 4 + 1).astype(np.int64)}


def _config(tmp_path, monkeypatch, tag, full_domain, sampler=None, dpm=None, constraint=None, series=None, **evaluation):
    from sbgm_danra_amd.config_loader import load_config
    for k in ("DATA_DIR", "CKPT_DIR", "STATS_LOAD_DIR"):
        monkeypatch.setenv(k, str(tmp_path / k.lower()))
    monkeypatch.setenv("SAMPLE_DIR", str(tmp_path / f"samples_{tag}"))
    monkeypatch.setenv("SLURM_CPUS_PER_TASK", "2")
    npz = tmp_path / "gen.npz"
    if not npz.exists():
        np.savez(npz, **arrays())
    raw = yaml.safe_load(open(os.path.join(ROOT, "sbgm_danra_amd", "config", "default_config.yaml")))
    raw["highres"]["data_size"] = [TILE, TILE]                       # the training crop: the sampler's img_size, not the domain
    raw["lowres"]["data_size"] = [TILE, TILE]
    raw["lowres"]["condition_variables"] = ["temp", "prcp"]
    raw["transforms"]["scaling"] = False
    raw["stationary_conditions"]["geographic_conditions"].update(sample_w_geo=True, geo_variables=["lsm", "topo"])
    raw["stationary_conditions"]["seasonal_conditions"]["sample_w_cond_season"] = True
    raw["sampler"]["n_timesteps"] = STEPS
    raw["sampler"].update(sampler or {})
    raw.setdefault("data_handling", {})["resident_fields"] = {"gen": str(npz)}
    raw["paths"]["evaluation_dir"] = str(tmp_path / f"ev_{tag}")
    raw["evaluation"].update(dict(dict(batch_size=3, n_repeats=4, seed=11, gen_type=["series"], transform_back=False,
                                       series=dict(SERIES, **(series or {})), full_domain=full_domain), **evaluation))
    if constraint is not None:
        raw["constraint"] = constraint
    if dpm is not None:
        raw["dpm"] = dpm
    p = tmp_path / f"run_{tag}.yaml"
    p.write_text(yaml.safe_dump(raw))
    return load_config(str(p)), str(p)


def _state_dict():
    from oracle import torch_ref as O
    if "sd" not in _CACHE:
        _CACHE["sd"] = O.synth_state_dict(O.build_scorenet(6, num_classes=4))
    return _CACHE["sd"]


def _run(tmp_path, monkeypatch, tag, full_domain=None, **how):
    """one generation_main run into its own sample directory -> (folder, cfg, config path)"""
    from sbgm_danra_amd.evaluate_sbgm.generation_main import generation_main
    from sbgm_danra_amd.utils import get_model_string
    cfg, path = _config(tmp_path, monkeypatch, tag, full_domain or {"halo": HALO}, **how)
    ckpt_dir = os.path.join(cfg.paths.path_save, cfg.paths.checkpoint_dir)
    os.makedirs(ckpt_dir, exist_ok=True)
    ckpt = os.path.join(ckpt_dir, get_model_string(cfg) + ".pth.tar")
    if not os.path.exists(ckpt):
        torch.save({"network_params": _state_dict(), "optimizer_params": {}}, ckpt)
    generation_main(cfg)
    return os.path.join(cfg.paths.sample_dir, "generation", get_model_string(cfg), "generated_samples"), cfg, path


def _arr(folder, name, days=DAYS):
    return np.load(os.path.join(folder, f"{name}_series_n_{days}.npz"))["arr_0"]


def _model(cfg):
    from sbgm_danra_amd.training_utils import get_model
    model, _, _ = get_model(cfg)
    model = model.cuda()
    model.load_state_dict(_state_dict())
    return model.eval()


def conditions(pad):
    """what the loader and extract_any hand the tiler, rebuilt with torch: cond [D, 2, Hd, W] (sorted *_lr keys), lsm and topo as
    value||mask [2, Hd, W], the classes; W = Wd, or Wd_pad with the right edge replicated"""
    a = {k: torch.from_numpy(v).cuda() for k, v in arrays().items()}
    cond = torch.stack([a["prcp_lr"], a["temp_lr"]], dim=1)
    lsm = torch.stack([(a["lsm"] > 0.5).float(), torch.ones(HD, WD, device="cuda")])
    topo = torch.stack([a["topo"], torch.ones(HD, WD, device="cuda")])
    if pad:
        cond, lsm, topo = (torch.nn.functional.pad(t, (0, WP - WD, 0, 0), mode="replicate") for t in (cond, lsm[None], topo[None]))
        lsm, topo = lsm[0], topo[0]
    return cond, lsm, topo, a["classifier"].tolist(), a["prcp_hr"]


def direct(cfg, sampler, pad=False, **how):
    import sbgm_danra_amd as S
    from sbgm_danra_amd.score_sampling import temporal_noise_weights
    from sbgm_danra_amd.tiling import FullDomainTiler
    t = FullDomainTiler((HD, WD), TILE, HALO)
    assert t.Wd_pad == WP and len(t) == 4
    cond, lsm, topo, y, _ = conditions(pad)
    return t.sample_series(_model(cfg), sampler, S.marginal_prob_std_fn, S.diffusion_coeff_fn, STEPS, cond_img=cond, lsm_cond=lsm,
                           topo_cond=topo, y=y, members=MEMBERS, seed=SEED, temporal_noise_weights=temporal_noise_weights(0.6, 3), **how)


def base_run(tmp_path, monkeypatch):
    """the predictor-corrector series at evaluation.batch_size 3, once per session: (gen [4, 2, 44, 53], truth [4, 44, 53])"""
    if "base" not in _CACHE:
        folder, cfg, _ = _run(tmp_path, monkeypatch, "base")
        _CACHE["base"] = (_arr(folder, "gen_samples"), _arr(folder, "eval_samples"), sorted(os.listdir(folder)), cfg,
                          dict(np.load(os.path.join(folder, f"series_index_series_n_{DAYS}.npz"))), _arr(folder, "lsm_samples"),
                          _arr(folder, "seasons"))
    return _CACHE["base"]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_series_files_of_a_domain_run(tmp_path, monkeypatch):
    from sbgm_danra_amd.score_sampling import temporal_noise_acf, temporal_noise_weights
    gen, truth, files, _, index, lsm, seasons = base_run(tmp_path, monkeypatch)
    assert files == sorted(f"{p}_series_n_{DAYS}.npz" for p in ("gen_samples", "eval_samples", "lsm_samples", "seasons", "series_index"))
    assert gen.shape == (DAYS, MEMBERS, HD, WD) and gen.dtype == np.float32 and np.isfinite(gen).all()          # width 53: no pad in a file
    assert truth.shape == (DAYS, HD, WD) and np.array_equal(bits(truth), bits(arrays()["prcp_hr"]))
    assert lsm.shape == (1, 2, HD, WD) and np.array_equal(lsm[0, 0], (arrays()["lsm"] > 0.5).astype(np.float32))
    assert seasons.tolist() == arrays()["classifier"].tolist()
    w = temporal_noise_weights(0.6, 3)
    assert int(index["members"]) == MEMBERS and int(index["seed"]) == SEED and int(index["first_day"]) == 0
    assert np.array_equal(index["weights"], w) and np.array_equal(index["acf"], temporal_noise_acf(w))
    assert index["domain_hw"].tolist() == [HD, WD] and (int(index["tile"]), int(index["halo"]), bool(index["joint"])) == (TILE, HALO, False)
    assert index["tile_origins"].tolist() == [[0, 0], [0, 24], [12, 0], [12, 24]]
    for d in range(DAYS):
        assert (gen[d, 0] != gen[d, 1]).mean() > 0.99


@pytest.mark.parametrize("kind", ["pc", "dpm", "joint"])
def test_generate_series_equals_the_tiler_called_directly(tmp_path, monkeypatch, kind):
    import sbgm_danra_amd as S
    if kind == "pc":
        got, cfg = base_run(tmp_path, monkeypatch)[0], base_run(tmp_path, monkeypatch)[3]
        want = direct(cfg, S.pc_sampler)
    elif kind == "dpm":
        folder, cfg, _ = _run(tmp_path, monkeypatch, kind, sampler={"sampler_type": "dpmpp_2m_sampler"}, dpm={"eta": 1.0})
        got, want = _arr(folder, "gen_samples"), direct(cfg, S.dpmpp_2m_sampler, eta=1.0)
    else:
        folder, cfg, _ = _run(tmp_path, monkeypatch, kind, full_domain={"halo": HALO, "joint": True})
        got, want = _arr(folder, "gen_samples"), direct(cfg, S.pc_sampler, joint=True)
        assert not np.array_equal(got, base_run(tmp_path, monkeypatch)[0])
    want = want.cpu().numpy()
    assert np.isfinite(want).all()
    assert np.array_equal(bits(got), bits(want)), f"{kind}: {int((bits(got) != bits(want)).sum())} of {want.size} values differ"


@pytest.mark.parametrize("batch_size", [1, 4])
def test_series_does_not_depend_on_the_loaders_batching(tmp_path, monkeypatch, batch_size):
    gen, truth = base_run(tmp_path, monkeypatch)[:2]                 # evaluation.batch_size 3: a ragged last batch
    folder, _, _ = _run(tmp_path, monkeypatch, f"bs{batch_size}", batch_size=batch_size)
    assert np.array_equal(bits(_arr(folder, "gen_samples")), bits(gen)) and np.array_equal(bits(_arr(folder, "eval_samples")), bits(truth))


def test_first_day_keeps_the_absolute_rows(tmp_path, monkeypatch):
    gen, truth = base_run(tmp_path, monkeypatch)[:2]
    folder, _, _ = _run(tmp_path, monkeypatch, "late", full_domain={"halo": HALO, "first_day": 2}, series={"max_days": 2})
    assert np.array_equal(bits(_arr(folder, "gen_samples", 2)), bits(gen[2:])) and np.array_equal(bits(_arr(folder, "eval_samples", 2)), bits(truth[2:]))
    index = dict(np.load(os.path.join(folder, "series_index_series_n_2.npz")))
    assert int(index["first_day"]) == 2 and _arr(folder, "seasons", 2).tolist() == arrays()["classifier"][2:].tolist()
    folder, _, _ = _run(tmp_path, monkeypatch, "early", series={"max_days": 2})
    assert np.array_equal(bits(_arr(folder, "gen_samples", 2)), bits(gen[:2]))


def test_constraint_holds_the_days_truth_on_a_domain_mask(tmp_path, monkeypatch):
    mask = (np.random.default_rng(5).random((HD, WD)) < 0.2).astype(np.float32)
    np.save(tmp_path / "mask.npy", mask)
    folder, _, _ = _run(tmp_path, monkeypatch, "held", constraint={"enabled": True, "mask_file": str(tmp_path / "mask.npy")})
    gen, truth = _arr(folder, "gen_samples"), _arr(folder, "eval_samples")
    assert gen.shape == (DAYS, MEMBERS, HD, WD) and _arr(folder, "constraint_mask").shape == (HD, WD)
    held = mask > 0
    for m in range(MEMBERS):
        assert np.array_equal(bits(gen[:, m][:, held]), bits(truth[:, held]))
    assert (gen[:, 0][:, ~held] != truth[:, ~held]).mean() > 0.99
    np.save(tmp_path / "mask.npy", mask[:TILE, :TILE])              # a mask of the training crop is refused at start
    with pytest.raises(ValueError, match="constraint.mask_file"):
        _run(tmp_path, monkeypatch, "held_crop", constraint={"enabled": True, "mask_file": str(tmp_path / "mask.npy")})


def test_tiler_takes_prepadded_conditions(tmp_path, monkeypatch):
    import sbgm_danra_amd as S
    from sbgm_danra_amd.tiling import FullDomainTiler
    cfg = base_run(tmp_path, monkeypatch)[3]
    plain, padded = direct(cfg, S.pc_sampler), direct(cfg, S.pc_sampler, pad=True)
    assert padded.shape == (DAYS, MEMBERS, HD, WD) and torch.equal(plain, padded)
    t = FullDomainTiler((HD, WD), TILE, HALO)
    cond = conditions(False)[0][0]
    assert torch.equal(t.extract(cond), t.extract(torch.nn.functional.pad(cond[None], (0, WP - WD, 0, 0), mode="replicate")[0]))
    for bad in (WD + 1, WP + 4):
        with pytest.raises(ValueError, match="does not match the tiler"):
            t.extract(torch.zeros(1, HD, bad, device="cuda"))
    with pytest.raises(ValueError, match="known"):                   # known / known_mask stay [1, Hd, Wd]
        t.sample(_model(cfg), S.pc_sampler, S.marginal_prob_std_fn, S.diffusion_coeff_fn, STEPS, cond_img=conditions(False)[0][0],
                 lsm_cond=conditions(False)[1], topo_cond=conditions(False)[2], y=1, known=torch.zeros(1, HD, WP), known_mask=torch.zeros(1, HD, WP))


def test_evaluate_mode_runs_on_the_domain_files(tmp_path, monkeypatch):
    from sbgm_danra_amd.cli import main_app
    from sbgm_danra_amd.evaluate_sbgm.evaluation import statistics_dir
    folder, cfg, _ = _run(tmp_path, monkeypatch, "ev")
    gen, truth = _arr(folder, "gen_samples"), _arr(folder, "eval_samples")
    _, path = _config(tmp_path, monkeypatch, "ev", {"halo": HALO}, eval_gen_type=["series"],
                      eval_stat_methods=["pixel_stats", "spatial_stats", "daily_stats", "spectral_stats"],
                      climate_indices={"wet": 0.0, "quantiles": [0.5]}, series_scores={"thresholds": [0.0], "climatology": True},
                      spatial_scores={"thresholds": [0.0], "scales": [1, 5]}, object_scores={"thresholds": [0.5]})
    main_app.main(["--config_path", path, "--mode", "evaluate"])
    stats = statistics_dir(cfg)
    met = json.load(open(os.path.join(stats, "series_metrics.json")))
    assert met["shape"] == [HD, WD] and met["members"] == MEMBERS and met["n_samples"] == DAYS and met["gen_type"] == "series"
    for key in ("pixel_stats", "spatial_stats", "daily_stats", "climate", "series_ensemble"):
        assert key in met, sorted(met)
    f = dict(np.load(os.path.join(stats, "series_climate.npz")))
    assert f["gen_mean"].shape == (MEMBERS, HD, WD) and f["obs_mean"].shape == (HD, WD)
    assert (f["days"] == DAYS).all()
    np.testing.assert_array_equal(f["obs_mean"], (truth.astype(np.float64).cumsum(axis=0)[-1] / DAYS).astype(np.float32))
    fields = dict(np.load(os.path.join(stats, "series_fields.npz")))
    assert fields["spatial_mae_per_pixel"].shape == (HD, WD)
    s = dict(np.load(os.path.join(stats, "series_series_scores.npz")))
    assert any(v.shape[-2:] == (HD, WD) for v in s.values()) and not any(WP in v.shape for v in s.values()) and gen.shape[-2:] == (HD, WD)
