"""GPU suite for a series with a calendar: a generation split whose .npz carries `dates` keys its noise rows by date (crop series
and full-domain series, tiled and joint), so a file with a hole gives, on the dates it has, the fields of the gap-free file; the
noise across a hole correlates as the weights say for that many days; a second file continues a series under the first one's
origin; and `--mode evaluate` reads the dates back for the calendar-aware, grouped climate indices and the season groups of the
pooled scores.  Modelled on tests/test_gpu_domain_generation.py, whose tiny seeded model and geometry it shares (domain 44 x 53,
tile 32, halo 4, 3 steps, 2 members); the fields are served raw, so every comparison of fields is exact."""
import json
import math
import os

import numpy as np
import pytest
import torch
import yaml

import test_gpu_domain_generation as DG
from test_gpu_domain_generation import HALO, HD, MEMBERS, ROOT, SEED, STEPS, TILE, WD, bits

pytestmark = pytest.mark.gpu

D0 = int(np.datetime64("2020-02-27").astype(np.int64))        # 27 28 29 Feb | 1 2 Mar missing | 3 4 Mar: a leap day, two seasons
FULL, GAP, TAIL = [0, 1, 2, 3, 4, 5, 6], [0, 1, 2, 5, 6], [5, 6]
SERIES = {"members": MEMBERS, "seed": SEED, "temporal_noise": {"rho": 0.6, "lags": 5}}
CROP = [4, 36, 8, 40]
_CACHE = {}


def arrays(offsets):
    """the days D0 + offsets of one 7-day record: a date has the same fields in every file"""
    rng = np.random.default_rng(17)
    yy, xx = np.mgrid[0:HD, 0:WD]
    full = {"prcp_hr": rng.normal(0, 1, (7, HD, WD)).astype(np.float32), "temp_lr": rng.normal(0, 1, (7, HD, WD)).astype(np.float32),
            "prcp_lr": rng.normal(0, 1, (7, HD, WD)).astype(np.float32), "classifier": (np.arange(7) % 4 + 1).astype(np.int64)}
    out = {k: v[offsets] for k, v in full.items()}
    out.update(lsm=np.where((yy + xx) % 7 == 0, 0.3, ((yy - 20) ** 2 + (xx - 30) ** 2 < 150)).astype(np.float32),
               topo=rng.random((HD, WD), dtype=np.float32), dates=D0 + np.asarray(offsets, np.int64))
    return out


def _config(tmp_path, monkeypatch, tag, offsets, domain, series=None, dates=True, **evaluation):
    from sbgm_danra_amd.config_loader import load_config
    for k in ("DATA_DIR", "CKPT_DIR", "STATS_LOAD_DIR"):
        monkeypatch.setenv(k, str(tmp_path / k.lower()))
    monkeypatch.setenv("SAMPLE_DIR", str(tmp_path / f"samples_{tag}"))
    monkeypatch.setenv("SLURM_CPUS_PER_TASK", "2")
    npz = tmp_path / f"gen_{'_'.join(map(str, offsets))}_{int(dates)}.npz"
    if not npz.exists():
        a = arrays(offsets)
        if not dates:
            del a["dates"]
        np.savez(npz, **a)
    raw = yaml.safe_load(open(os.path.join(ROOT, "sbgm_danra_amd", "config", "default_config.yaml")))
    for sec in ("highres", "lowres"):
        raw[sec]["data_size"] = [TILE, TILE]
        raw[sec]["cutout_domains"] = CROP                          # the crop series: one fixed 32 x 32 rectangle
    raw["lowres"]["condition_variables"] = ["temp", "prcp"]
    raw["transforms"].update(scaling=False, sample_w_cutouts=False)
    raw["stationary_conditions"]["geographic_conditions"].update(sample_w_geo=True, geo_variables=["lsm", "topo"])
    raw["stationary_conditions"]["seasonal_conditions"]["sample_w_cond_season"] = True
    raw["sampler"]["n_timesteps"] = STEPS
    if domain is None:                                             # the crop series: the 2M SDE, which knows no batch-mates
        raw["sampler"]["sampler_type"] = "dpmpp_2m_sampler"
        raw["dpm"] = {"eta": 1.0}
    raw.setdefault("data_handling", {})["resident_fields"] = {"gen": str(npz)}
    raw["paths"]["evaluation_dir"] = str(tmp_path / f"ev_{tag}")
    # a crop series samples a batch of days in one call, and kernels chosen by the batch's shape round differently: one day a batch
    # gives a date the same call in every file; a domain series samples field by field whatever the batch is
    ev = dict(batch_size=1 if domain is None else 3, n_repeats=4, seed=11, gen_type=["series"], transform_back=False, series=dict(SERIES, **(series or {})))
    if domain is not None:
        ev["full_domain"] = domain
    raw["evaluation"].update(dict(ev, **evaluation))
    p = tmp_path / f"run_{tag}.yaml"
    p.write_text(yaml.safe_dump(raw))
    return load_config(str(p)), str(p)


def _run(tmp_path, monkeypatch, tag, offsets, domain, **how):
    """one generation_main run -> (gen [D, M, H, W], truth, index dict, folder, cfg); cached by tag"""
    if tag in _CACHE:
        return _CACHE[tag]
    from sbgm_danra_amd.evaluate_sbgm.generation_main import generation_main
    from sbgm_danra_amd.utils import get_model_string
    cfg, _ = _config(tmp_path, monkeypatch, tag, offsets, domain, **how)
    ckpt_dir = os.path.join(cfg.paths.path_save, cfg.paths.checkpoint_dir)
    os.makedirs(ckpt_dir, exist_ok=True)
    ckpt = os.path.join(ckpt_dir, get_model_string(cfg) + ".pth.tar")
    if not os.path.exists(ckpt):
        torch.save({"network_params": DG._state_dict(), "optimizer_params": {}}, ckpt)
    generation_main(cfg)
    folder = os.path.join(cfg.paths.sample_dir, "generation", get_model_string(cfg), "generated_samples")
    n = len(offsets)
    _CACHE[tag] = (DG._arr(folder, "gen_samples", n), DG._arr(folder, "eval_samples", n),
                   dict(np.load(os.path.join(folder, f"series_index_series_n_{n}.npz"))), folder, cfg)
    return _CACHE[tag]


KINDS = {"crop": None, "tiled": {"halo": HALO}, "joint": {"halo": HALO, "joint": True}}


@pytest.mark.parametrize("kind", list(KINDS))
def test_a_file_with_a_hole_gives_the_gap_free_files_fields_on_its_dates(tmp_path, monkeypatch, kind):
    full, truth_full, index_full = _run(tmp_path, monkeypatch, f"{kind}_full", FULL, KINDS[kind])[:3]
    gap, truth_gap, index = _run(tmp_path, monkeypatch, f"{kind}_gap", GAP, KINDS[kind])[:3]
    shape = (TILE, TILE) if kind == "crop" else (HD, WD)
    assert full.shape == (7, MEMBERS, *shape) and gap.shape == (5, MEMBERS, *shape) and np.isfinite(full).all()
    assert index["dates"].dtype == np.int64 and index["dates"].tolist() == [D0 + o for o in GAP] and int(index["calendar_origin"]) == D0
    assert index_full["dates"].tolist() == [D0 + o for o in FULL] and int(index_full["calendar_origin"]) == D0
    assert np.array_equal(bits(truth_gap), bits(truth_full[GAP]))
    print(f"{kind}: largest |gap - full| per date {np.abs(gap - full[GAP]).max(axis=(1, 2, 3)).tolist()}")
    assert np.array_equal(bits(gap), bits(full[GAP])), f"{int((bits(gap) != bits(full[GAP])).sum())} of {gap.size} values differ"
    for a, b in ((3, 5), (4, 6), (3, 4)):                                        # and the rows do select: other dates, other fields
        assert (full[a] != full[b]).mean() > 0.99


def test_without_dates_the_rows_count_positions(tmp_path, monkeypatch):
    """the same five days without `dates`: the series of file positions, bit for bit what the dated gap-free file gives on its first
    five positions' noise rows, and no calendar keys in the index"""
    bare, _, index = _run(tmp_path, monkeypatch, "bare", GAP, KINDS["tiled"], dates=False)[:3]
    assert "dates" not in index and "calendar_origin" not in index and int(index["first_day"]) == 0
    gap = _run(tmp_path, monkeypatch, "tiled_gap", GAP, KINDS["tiled"])[0]
    assert np.array_equal(bits(bare[:3]), bits(gap[:3])) and (bare[3:] != gap[3:]).mean() > 0.99


def test_a_second_file_continues_the_series_under_the_first_origin(tmp_path, monkeypatch):
    full = _run(tmp_path, monkeypatch, "tiled_full", FULL, KINDS["tiled"])[0]
    for origin in ("2020-02-27", D0):
        tail, _, index = _run(tmp_path, monkeypatch, f"tail_{origin}", TAIL, KINDS["tiled"], series={"calendar_origin": origin})[:3]
        assert int(index["calendar_origin"]) == D0 and index["dates"].tolist() == [D0 + 5, D0 + 6]
        assert np.array_equal(bits(tail), bits(full[TAIL]))
    own = _run(tmp_path, monkeypatch, "tail_own", TAIL, KINDS["tiled"])[0]         # its own first date as the origin: another series
    assert (own != full[TAIL]).mean() > 0.99
    with pytest.raises(ValueError, match="origin"):
        _run(tmp_path, monkeypatch, "tail_late", TAIL, KINDS["tiled"], series={"calendar_origin": D0 + 6})


def test_noise_across_a_hole_correlates_at_the_lag_of_the_hole():
    """zero score: a field is a sum of its draws.  Days 2 and 5 are three days apart, the other neighbours one; the tolerance is the
    5 / sqrt(n) of the domain-noise suite"""
    import sbgm_danra_amd as S
    from sbgm_danra_amd import score_sampling as SS
    from sbgm_danra_amd.tiling import FullDomainTiler
    from util_models import build_pair
    _, znet, _ = build_pair(1)
    znet.eval()
    with torch.no_grad():
        znet.decoder.final_layer.conv.weight.zero_()
        znet.decoder.final_layer.conv.bias.zero_()
    w = SS.temporal_noise_weights(0.6, 5)
    acf = SS.temporal_noise_acf(w)
    t = FullDomainTiler((HD, WD), TILE, HALO)
    cond = torch.randn(5, 1, HD, WD, generator=torch.Generator().manual_seed(32)).cuda()
    out = t.sample_series(znet, S.Euler_Maruyama_sampler, S.marginal_prob_std_fn, S.diffusion_coeff_fn, num_steps=3, cond_img=cond,
                          members=MEMBERS, seed=77, temporal_noise_weights=w, day_numbers=GAP)
    n = MEMBERS * HD * WD
    corr = lambda a, b: float(torch.corrcoef(torch.stack([out[a].reshape(-1).double(), out[b].reshape(-1).double()]))[0, 1])  # noqa: E731
    got = {(a, b): corr(a, b) for a, b in ((0, 1), (1, 2), (2, 3), (3, 4))}
    print(f"correlations {got}; acf[1] {acf[1]:.4f}, acf[3] {acf[3]:.4f}; bound {5 / math.sqrt(n):.4f}")
    assert float(acf[3]) > 0.1 and float(acf[1]) - float(acf[3]) > 10 / math.sqrt(n)                # the two lags can be told apart
    assert abs(got[(2, 3)] - float(acf[3])) <= 5 / math.sqrt(n)
    for pair in ((0, 1), (1, 2), (3, 4)):
        assert abs(got[pair] - float(acf[1])) <= 5 / math.sqrt(n)
    again = t.sample_series(znet, S.Euler_Maruyama_sampler, S.marginal_prob_std_fn, S.diffusion_coeff_fn, num_steps=3, cond_img=cond[3:],
                            members=MEMBERS, seed=77, temporal_noise_weights=w, day_numbers=TAIL)
    assert torch.equal(again, out[3:])                                           # a date's field depends on (seed, day, m) only


def test_evaluate_mode_groups_by_season_from_the_dates(tmp_path, monkeypatch):
    from sbgm_danra_amd import verification as V
    from sbgm_danra_amd.cli import main_app
    from sbgm_danra_amd.evaluate_sbgm.evaluation import statistics_dir
    gen, truth, index, folder, cfg = _run(tmp_path, monkeypatch, "ev", GAP, KINDS["tiled"])
    ids = [0, 0, 0, 1, 1]                                                        # 27 - 29 Feb: DJF; 3, 4 Mar: MAM
    section = {"wet": 0.0, "quantiles": [0.5], "wet_quantiles": [0.9], "groups": "season"}
    out = {}
    for tag, groups in (("season", "season"), ("list", ids + [])):
        _, path = _config(tmp_path, monkeypatch, "ev", GAP, KINDS["tiled"], eval_gen_type=["series"], eval_stat_methods=["daily_stats"],
                          climate_indices=section, series_scores={"thresholds": [0.0], "climatology": True, "groups": groups})
        main_app.main(["--config_path", path, "--mode", "evaluate"])
        stats = statistics_dir(cfg)
        out[tag] = (json.load(open(os.path.join(stats, "series_metrics.json"))), dict(np.load(os.path.join(stats, "series_series_scores.npz"))),
                    dict(np.load(os.path.join(stats, "series_climate.npz"))))
    met, scores, f = out["season"]
    # the climate file: every plain key, the dates, the groups and the group maps, equal to the device call made directly
    assert f["dates"].tolist() == index["dates"].tolist() and f["groups"].tolist() == ids and f["group_names"].tolist() == ["DJF", "MAM"]
    assert f["group_days"].shape == (2, HD, WD) and f["group_gen_mean"].shape == (MEMBERS, 2, HD, WD) and f["group_obs_quantiles"].shape == (2, 1, HD, WD)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()              # noqa: E731
    for m in range(MEMBERS):
        r = V.climate_indices(dev(gen[:, m]), dev(truth), 0.0, [0.5], [0.9], day_numbers=index["dates"], groups=ids)
        plain = V.climate_indices(dev(gen[:, m]), dev(truth), 0.0, [0.5], [0.9])
        np.testing.assert_array_equal(f["group_days"], r["group_days"].cpu().numpy())
        for k in V.CLIMATE_FLOAT_KEYS + V.CLIMATE_INT_KEYS:
            np.testing.assert_array_equal(bits32(f[f"gen_{k}"][m]), bits32(r[f"gen_{k}"]), err_msg=k)
            np.testing.assert_array_equal(bits32(f[f"obs_{k}"]), bits32(r[f"obs_{k}"]), err_msg=k)
            np.testing.assert_array_equal(bits32(f[f"group_gen_{k}"][m]), bits32(r[f"group_gen_{k}"]), err_msg=k)
            np.testing.assert_array_equal(bits32(f[f"group_obs_{k}"]), bits32(r[f"group_obs_{k}"]), err_msg=k)
        assert (r["gen_transitions"].sum(dim=0) == 3).all() and (plain["gen_transitions"].sum(dim=0) == 4).all()   # the hole is known
    cl = met["climate"]
    assert cl["calendar"] is True and cl["n_links_broken"] == 1 and [g["name"] for g in cl["groups"]] == ["DJF", "MAM"]
    assert [g["n_days"] for g in cl["groups"]] == [3, 2] and list(cl["groups"][0]["indices"]) == list(cl["indices"])
    assert cl["groups"][1]["indices"]["mean"]["per_member"][0]["pixels"] == HD * WD
    # the pooled scores: `season` is the same ids given as a list
    met_l, scores_l, _ = out["list"]
    assert scores["groups"].tolist() == ids and set(scores) == set(scores_l) and scores["scores"].shape[0] == 3
    for k in scores:
        np.testing.assert_array_equal(scores[k], scores_l[k], err_msg=k)
    assert json.dumps(met["series_ensemble"], sort_keys=True) == json.dumps(met_l["series_ensemble"], sort_keys=True)


def bits32(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.ascontiguousarray(a)
    return a.view(np.int32)
