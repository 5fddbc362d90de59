"""CPU suite for the evaluation stage: sample-file discovery, the config defaults of evaluation_main, and how main_app
dispatches `evaluate` / `full_pipeline` (no GPU: the launchers are replaced or the checks fire before any kernel)."""
import os

import numpy as np
import pytest
import torch

from sbgm_danra_amd.cli import main_app
from sbgm_danra_amd.config_loader import load_config, to_config
from sbgm_danra_amd.evaluate_sbgm import evaluation as E
from sbgm_danra_amd.evaluate_sbgm import evaluation_main as EM
from sbgm_danra_amd.utils import get_model_string

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "sbgm_danra_amd", "config", "default_config.yaml")


@pytest.fixture()
def cfg(tmp_path, monkeypatch):
    for k in ("DATA_DIR", "CKPT_DIR", "SAMPLE_DIR", "STATS_LOAD_DIR"):
        monkeypatch.setenv(k, str(tmp_path / k.lower()))
    monkeypatch.setenv("SLURM_CPUS_PER_TASK", "2")
    return load_config(CFG)


def _touch(d, names, rows=2):
    os.makedirs(d, exist_ok=True)
    for i, n in enumerate(names):
        np.savez_compressed(os.path.join(d, n), np.full((rows, 4, 5), float(i), np.float32))


def test_discovery_of_every_suffix_spelling(tmp_path):
    d = str(tmp_path)
    _touch(d, ["gen_samples_multi_n_4.npz", "eval_samples_multi_n_4.npz", "lsm_samples_multi_n_4.npz", "seasons_multi_n_4.npz",
               "gen_samples_single.npz", "eval_samples_single.npz",
               "gen_samples_repeated_n_3.npz", "eval_samples_repeated_n_3.npz"])
    [(r, f)] = E.sample_units(d, "multiple", 4)
    assert r is None and f == {p: [os.path.join(d, f"{p}_multi_n_4.npz")] for p in E.PREFIXES}
    [(r, f)] = E.sample_units(d, "single")
    assert r is None and set(f) == {"gen_samples", "eval_samples"}
    [(r, f)] = E.sample_units(d, "repeated", 3)
    assert f["gen_samples"] == [os.path.join(d, "gen_samples_repeated_n_3.npz")]
    d2 = str(tmp_path / "ref")
    _touch(d2, ["gen_samples_repeated_5.npz", "eval_samples_repeated_5.npz"])          # the reference's spelling
    [(r, f)] = E.sample_units(d2, "repeated", 5)
    assert f["eval_samples"] == [os.path.join(d2, "eval_samples_repeated_5.npz")]
    with pytest.raises(FileNotFoundError):
        E.sample_units(d2, "multiple")
    with pytest.raises(ValueError):
        E.sample_units(d2, "ensemble")


def test_discovery_of_rank_files(tmp_path):
    d = str(tmp_path)
    _touch(d, [f"{p}_multi_n_4_rank{r}.npz" for r in (1, 0, 2) for p in ("gen_samples", "eval_samples")] +
              [f"{p}_single_rank{r}.npz" for r in (0, 1) for p in ("gen_samples", "eval_samples")] +
              [f"{p}_repeated_n_4_rank{r}.npz" for r in (0, 1) for p in ("gen_samples", "eval_samples", "lsm_samples")])
    [(r, f)] = E.sample_units(d, "multiple", 4)                 # concatenated, in rank order
    assert r is None and f["gen_samples"] == [os.path.join(d, f"gen_samples_multi_n_4_rank{k}.npz") for k in (0, 1, 2)]
    assert "lsm_samples" not in f
    [(r, f)] = E.sample_units(d, "single")
    assert len(f["eval_samples"]) == 2
    units = E.sample_units(d, "repeated", 4)                    # one unit per rank
    assert [u[0] for u in units] == [0, 1]
    assert units[1][1]["lsm_samples"] == [os.path.join(d, "lsm_samples_repeated_n_4_rank1.npz")]
    # rank files whose size differs from the configured one are still found (a rank's shard may be smaller)
    assert len(E.sample_units(d, "multiple", 32)[0][1]["gen_samples"]) == 3


def test_discovery_size_choice_and_missing_truth(tmp_path):
    d = str(tmp_path)
    _touch(d, ["gen_samples_multi_n_4.npz", "eval_samples_multi_n_4.npz", "gen_samples_multi_n_8.npz", "eval_samples_multi_n_8.npz",
               "gen_samples_multi_n_2_rank0.npz", "eval_samples_multi_n_2_rank0.npz", "gen_samples_single.npz"])
    [(_, f)] = E.sample_units(d, "multiple", 8)                  # unranked files win; the configured size picks among them
    assert f["gen_samples"] == [os.path.join(d, "gen_samples_multi_n_8.npz")]
    with pytest.raises(ValueError):
        E.sample_units(d, "multiple", 16)
    with pytest.raises(FileNotFoundError):
        E.sample_units(d, "single")                              # no eval_samples_single


def test_statistics_dir_and_evaluation_on_loaded_files(cfg, tmp_path):
    assert E.statistics_dir(cfg) == os.path.join(cfg.paths.sample_dir, "evaluation", get_model_string(cfg), "statistics")
    cfg.paths.evaluation_dir = str(tmp_path / "ev")
    assert E.statistics_dir(cfg) == os.path.join(str(tmp_path / "ev"), get_model_string(cfg), "statistics")
    d = os.path.join(cfg.paths.sample_dir, "generation", get_model_string(cfg), "generated_samples")
    _touch(d, ["gen_samples_multi_n_4_rank0.npz", "eval_samples_multi_n_4_rank0.npz",
               "gen_samples_multi_n_4_rank1.npz", "eval_samples_multi_n_4_rank1.npz"], rows=4)
    ev = E.Evaluation(cfg, "multiple", 4, device=torch.device("cpu"))
    assert ev.gen_imgs.shape == (8, 4, 5) and ev.label == "multiple" and os.path.isdir(E.statistics_dir(cfg))
    with pytest.raises(ValueError, match="repeated"):             # an ensemble needs repeated samples
        ev.ensemble_statistics()
    cfg.evaluation.mask_stats = True
    with pytest.raises(FileNotFoundError, match="lsm_samples"):
        E.Evaluation(cfg, "multiple", 4, device=torch.device("cpu"))


def test_repeated_rank_units_need_a_rank(cfg):
    d = os.path.join(cfg.paths.sample_dir, "generation", get_model_string(cfg), "generated_samples")
    _touch(d, [f"{p}_repeated_n_4_rank{r}.npz" for r in (0, 1) for p in ("gen_samples", "eval_samples")])
    with pytest.raises(ValueError, match="rank"):
        E.Evaluation(cfg, "repeated", 4, device=torch.device("cpu"))
    ev = E.Evaluation(cfg, "repeated", 4, rank=1, device=torch.device("cpu"))
    assert ev.label == "repeated_rank1" and float(ev.gen_imgs[0, 0, 0]) == 2.0


def test_config_defaults():
    c = to_config({"evaluation": {"gen_type": ["single", "repeated"]}})
    assert EM.eval_gen_types(c) == ["single", "repeated"]
    assert EM.eval_gen_types(to_config({"evaluation": {}})) == ["multiple"]
    assert EM.eval_gen_types(to_config({"evaluation": {"gen_type": ["single"], "eval_gen_type": ["repeated"]}})) == ["repeated"]
    assert EM.eval_stat_methods(c) == ["pixel_stats", "spatial_stats"]
    m = ["daily_stats", "ensemble_stats", "spectral_stats"]
    assert EM.eval_stat_methods(to_config({"evaluation": {"eval_stat_methods": m}})) == m


def test_unknown_method_or_type_raises(cfg):
    cfg.evaluation.eval_stat_methods = ["pixel_stats", "morans_i"]
    with pytest.raises(ValueError, match="morans_i"):
        EM.evaluation_main(cfg)
    cfg.evaluation.eval_stat_methods = ["pixel_stats"]
    cfg.evaluation.eval_gen_type = ["ensemble"]
    with pytest.raises(ValueError, match="ensemble"):
        EM.evaluation_main(cfg)


@pytest.fixture()
def cfg_file(cfg, tmp_path):
    import yaml
    raw = yaml.safe_load(open(CFG))
    p = tmp_path / "run.yaml"
    p.write_text(yaml.safe_dump(raw))
    return str(p)


def test_evaluate_without_samples_raises(cfg_file):
    with pytest.raises(RuntimeError, match="Cannot evaluate: generated samples not found."):
        main_app.main(["--config_path", cfg_file, "--mode", "evaluate"])


@pytest.mark.parametrize("argv,want", [(["--mode", "evaluate"], ["eval"]),
                                       (["--mode", "full_pipeline"], ["train", "gen", "eval"]),
                                       (["--mode", "full_pipeline", "--skip_evaluation"], ["train", "gen"]),
                                       (["--mode", "full_pipeline", "--skip_train", "--skip_generation"], ["eval"]),
                                       (["--mode", "generate"], ["gen"]),
                                       (["--mode", "train"], ["train"])])
def test_main_app_dispatch(cfg_file, monkeypatch, argv, want):
    calls = []
    monkeypatch.setattr(main_app.launch_sbgm, "run", lambda cfg: calls.append("train"))
    monkeypatch.setattr(main_app.launch_generation, "run", lambda cfg: calls.append("gen"))
    monkeypatch.setattr(main_app.launch_evaluation, "run", lambda cfg: calls.append("eval"))
    monkeypatch.setattr(main_app, "check_model_exists", lambda cfg: True)
    monkeypatch.setattr(main_app, "check_generated_samples_exist", lambda cfg: True)
    main_app.main(["--config_path", cfg_file] + argv)
    assert calls == want


def test_data_splits_keeps_its_message(cfg_file):
    with pytest.raises(SystemExit, match="outside the accelerated hot path"):
        main_app.main(["--config_path", cfg_file, "--mode", "data_splits"])


def test_reference_module_paths_resolve():
    import sbgm
    from sbgm.cli import launch_evaluation
    from sbgm.evaluate_sbgm import evaluation, evaluation_main
    assert sbgm.cli.launch_evaluation is launch_evaluation
    assert evaluation.Evaluation is E.Evaluation and evaluation_main.evaluation_main is EM.evaluation_main


@pytest.mark.parametrize("rank", [0, 1])
def test_evaluation_runs_on_rank_zero_after_the_barrier(cfg_file, monkeypatch, rank):
    """under a 2-rank launch only rank 0 evaluates, and only after the barrier; the existence check is rank 0's, so a
    missing sample set cannot strand the other rank before the barrier"""
    from sbgm_danra_amd import parallel
    calls = []
    monkeypatch.setattr(parallel, "init_distributed", lambda *a, **k: (calls.append("init"), (rank, 2, 0))[1])
    monkeypatch.setattr(parallel, "barrier", lambda: calls.append("barrier"))
    monkeypatch.setattr(main_app.launch_evaluation, "run", lambda cfg: calls.append("eval"))
    monkeypatch.setattr(main_app, "check_generated_samples_exist", lambda cfg: (calls.append("check"), True)[1])
    main_app.main(["--config_path", cfg_file, "--mode", "evaluate"])
    assert calls == (["init", "barrier", "check", "eval"] if rank == 0 else ["init", "barrier"])
    calls.clear()
    monkeypatch.setattr(main_app, "check_generated_samples_exist", lambda cfg: (calls.append("check"), False)[1])
    if rank == 0:
        with pytest.raises(RuntimeError, match="Cannot evaluate: generated samples not found."):
            main_app.main(["--config_path", cfg_file, "--mode", "evaluate"])
        assert calls == ["init", "barrier", "check"]
    else:
        main_app.main(["--config_path", cfg_file, "--mode", "evaluate"])
        assert calls == ["init", "barrier"]


def test_unranked_files_next_to_rank_files_are_reported(tmp_path, caplog):
    d = str(tmp_path)
    _touch(d, ["gen_samples_multi_n_4.npz", "eval_samples_multi_n_4.npz",
               "gen_samples_multi_n_4_rank0.npz", "eval_samples_multi_n_4_rank0.npz"])
    with caplog.at_level("WARNING"):
        [(_, f)] = E.sample_units(d, "multiple", 4)
    assert f["gen_samples"] == [os.path.join(d, "gen_samples_multi_n_4.npz")]
    assert "rank files" in caplog.text
