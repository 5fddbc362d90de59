"""`python -m sbgm.cli.main_app --config_path X.yaml --mode {train,generate,evaluate,full_pipeline}` — the reference's
dispatcher (sbgm/cli/main_app.py:42-90).  `full_pipeline` runs evaluation unless --skip_evaluation is given; with several
ranks, evaluation runs on rank 0 after a barrier.  `data_splits` belongs to an out-of-scope subsystem
and exits with a message."""
import argparse
import os

import torch

from ..utils import get_model_string, load_config
from .. import parallel
from . import launch_evaluation, launch_generation, launch_sbgm


def check_model_exists(cfg) -> bool:
    d = os.path.join(cfg["paths"]["path_save"], cfg["paths"]["checkpoint_dir"])
    return os.path.exists(os.path.join(d, get_model_string(cfg) + ".pth.tar"))


def check_generated_samples_exist(cfg) -> bool:
    """reference main_app.py:35-38"""
    d = os.path.join(cfg["paths"]["sample_dir"], "generation", get_model_string(cfg), "generated_samples")
    return os.path.isdir(d) and any(f.startswith("gen_samples") for f in os.listdir(d))


def run_evaluation(cfg):
    """Evaluation runs once, on rank 0, after every rank has written its samples.  The process group is joined here
    (init_distributed is idempotent and creates none for a single process), because `--mode evaluate` alone never passes
    through the training or generation entry points that join it.  The barrier comes before the existence check, which
    only rank 0 makes: a rank that raised before the barrier would leave the others waiting in it."""
    rank, world, local = parallel.init_distributed()
    parallel.barrier()
    if rank != 0:
        return
    if world > 1 and torch.cuda.is_available():
        torch.cuda.set_device(local)
    if not check_generated_samples_exist(cfg):
        raise RuntimeError("Cannot evaluate: generated samples not found.")
    launch_evaluation.run(cfg)


def main(argv=None):
    ap = argparse.ArgumentParser(description="SBGM full pipeline launcher (MI355X-native hot path)")
    ap.add_argument("--config_path", required=True)
    ap.add_argument("--mode", choices=["train", "generate", "evaluate", "full_pipeline", "data_splits"], default="full_pipeline")
    ap.add_argument("--skip_train", action="store_true")
    ap.add_argument("--skip_generation", action="store_true")
    ap.add_argument("--skip_evaluation", action="store_true")
    a = ap.parse_args(argv)
    cfg = load_config(a.config_path)
    if a.mode == "data_splits":
        raise SystemExit(f"mode '{a.mode}' is outside the accelerated hot path (see DESIGN.md, out of scope)")
    if a.mode == "train" or (a.mode == "full_pipeline" and not a.skip_train):
        launch_sbgm.run(cfg)
    if a.mode == "generate" or (a.mode == "full_pipeline" and not a.skip_generation):
        if not check_model_exists(cfg):
            raise RuntimeError("Cannot generate: model checkpoint not found")
        launch_generation.run(cfg)
    if a.mode == "evaluate" or (a.mode == "full_pipeline" and not a.skip_evaluation):
        run_evaluation(cfg)
    print("\nPipeline finished successfully.")


if __name__ == "__main__":
    main()
