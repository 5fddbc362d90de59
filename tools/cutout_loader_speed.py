"""Speed probe of the device-resident cutout loader (sbgm_danra_amd/resident_data.py, csrc/cutout.hip) at the full DANRA domain:
589 x 789, N = 64 days, HR + two LR conditions + lsm + topo + SDF, the cutout rectangle of config/default_config.yaml, 128 x 128 crops at
batch 8 and 32.  One JSON line, per batch size:

    resident_ms_per_batch   draw + gather + SDF of the resident loader (median, min, max of six loops)
    host_ms_per_batch       the same batches by the host restatement tests/cutout_ref.py (numpy slicing, torch-CPU transforms,
                            scipy.ndimage.distance_transform_edt), including their copy to the device
    train_samples_per_s     TrainingPipeline_general.train_batches fed by the resident loader, by the synthetic loader (what
                            get_dataloader serves without `data_handling.resident_fields`) and by a list of batches that already sit
                            on the device (no loader at all), at the same shapes, six alternating loops each

Usage: python tools/cutout_loader_speed.py"""
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import yaml  # noqa: E402

import cutout_ref as R  # noqa: E402
from oracle import transforms_ref as TR  # noqa: E402
from sbgm_danra_amd import resident_data as RD  # noqa: E402
from sbgm_danra_amd.config_loader import to_config  # noqa: E402
from sbgm_danra_amd.score_unet import diffusion_coeff_fn, loss_fn, marginal_prob_std_fn  # noqa: E402
from sbgm_danra_amd.synthetic_data import synthetic_loader  # noqa: E402
from sbgm_danra_amd.training import TrainingPipeline_general  # noqa: E402
from sbgm_danra_amd.training_utils import get_model, get_optimizer  # noqa: E402

HD, WD, N_DAYS, CROP, LOOPS = 589, 789, 64, (128, 128), 6
STATS = {"prcp_hr": {"log_mean": -1.2345, "log_std": 2.0321, "log_min": -4.60517, "log_max": 5.7038},
         "temp_lr": {"mean": 8.7012, "std": 6.1923},
         "prcp_lr": {"log_mean": -0.5, "log_std": 1.75, "log_min": -4.60517, "log_max": 4.5}}


def make_arrays():
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:HD, 0:WD]
    lsm = (np.sin(yy / 23.0) + np.cos(xx / 31.0) + 0.3 * np.sin((yy + xx) / 7.0) > 0.2).astype(np.float32)      # coasts at several scales
    return {"prcp_hr": (rng.random((N_DAYS, HD, WD), dtype=np.float32) ** 4 * 60), "temp_lr": rng.normal(8, 6, (N_DAYS, HD, WD)).astype(np.float32),
            "prcp_lr": (rng.random((N_DAYS, HD, WD), dtype=np.float32) ** 4 * 40), "lsm": lsm,
            "topo": (rng.random((HD, WD), dtype=np.float32) * 900 - 5)}


def make_cfg(tmp, batch):
    raw = yaml.safe_load(open(os.path.join(ROOT, "sbgm_danra_amd", "config", "default_config.yaml")))
    raw["lowres"].update(condition_variables=["temp", "prcp"], scaling_methods=["zscore", "log_zscore"])
    raw["transforms"].update(sample_w_cutouts=True, scaling=True)
    raw["stationary_conditions"]["geographic_conditions"].update(sample_w_geo=True, sample_w_sdf=True)
    raw["training"].update(batch_size=batch, sdf_weighted_loss=True)
    raw["paths"] = {k: os.path.join(tmp, k) for k in ("data_dir", "checkpoint_dir", "sample_dir", "path_save", "stats_load_dir")}
    return to_config(raw)


def summary(values, digits=4):
    s = sorted(values)
    return {"median": round((s[len(s) // 2 - 1] + s[len(s) // 2]) / 2, digits), "min": round(s[0], digits), "max": round(s[-1], digits)}


def ref_transforms(arrays):
    log = lambda s: TR.PrcpLogTransform(scale_type="log_zscore", glob_mean_log=s["log_mean"], glob_std_log=s["log_std"],     # noqa: E731
                                        glob_min_log=s["log_min"], glob_max_log=s["log_max"], buffer_frac=0.5)
    return {"prcp_hr": log(STATS["prcp_hr"]), "prcp_lr": log(STATS["prcp_lr"]), "temp_lr": TR.ZScoreTransform(8.7012, 6.1923),
            "topo": TR.Scale(0.0, 1.0, float(arrays["topo"].min()), float(arrays["topo"].max()))}


def main():
    dev = torch.device("cuda")
    out = {"domain": [HD, WD], "days": N_DAYS, "crop": list(CROP), "loops": LOOPS, "device": torch.cuda.get_device_name(0), "batch": {}}
    arrays = make_arrays()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "train.npz")
        np.savez(path, **arrays)
        fields = RD.ResidentFields(path, "prcp", ["temp", "prcp"], device=dev)
        tr = ref_transforms(arrays)
        for batch in (8, 32):
            cfg = make_cfg(tmp, batch)
            dl = RD.ResidentCutoutLoader(fields, cfg, "train", batch, seed=1, stats=STATS)
            rect, row = dl.rect, {}
            for _ in dl:                                   # warm-up epoch
                pass
            torch.cuda.synchronize()
            res, host = [], []
            for loop in range(LOOPS):
                t0, n = time.perf_counter(), 0
                for _ in range(max(1, 64 // len(dl))):     # 64 batches a loop
                    for _b in dl:
                        n += 1
                torch.cuda.synchronize()
                res.append((time.perf_counter() - t0) * 1e3 / n)
                order = dl.item_order(loop)
                t0, n_host = time.perf_counter(), 2
                for i in range(n_host):
                    items = order[i * batch:(i + 1) * batch]
                    origins = R.draw_origins(1, R.draw_number("train", loop, i), batch, rect, CROP)
                    ref = R.batch_ref(arrays, "prcp_hr", ["temp_lr", "prcp_lr"], items, origins, CROP, tr)
                    moved = {k: torch.from_numpy(v).to(dev) for k, v in ref.items()}
                torch.cuda.synchronize()
                host.append((time.perf_counter() - t0) * 1e3 / n_host)
                del moved
            row["resident_ms_per_batch"], row["host_ms_per_batch"] = summary(res), summary(host, 2)
            # training: one pipeline, the loaders alternating; the first pass of each captures / tunes and is not timed
            torch.manual_seed(0)
            model, _, _ = get_model(cfg)
            model = model.to(dev)
            pipe = TrainingPipeline_general(model, loss_fn, marginal_prob_std_fn, diffusion_coeff_fn, get_optimizer(cfg, model), dev, None, cfg)
            syn = synthetic_loader(cfg, batch, n_items=N_DAYS, drop_last=True)
            dl.set_epoch(0)
            held = list(dl)                                # the same batches, cut once: what training costs with no loader at all
            rates = {"resident": [], "synthetic": [], "preloaded": []}
            for loop in range(LOOPS + 1):
                for name, loader in (("resident", dl), ("synthetic", syn), ("preloaded", held)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    epochs = 8 if batch == 8 else 16          # 64 and 32 steps a loop
                    for _ in range(epochs):
                        pipe.train_batches(loader, epochs=1, verbose=False)
                    torch.cuda.synchronize()
                    if loop:
                        rates[name].append(epochs * len(loader) * batch / (time.perf_counter() - t0))
            row["train_samples_per_s"] = {k: summary(v, 1) for k, v in rates.items()}
            r, s = row["train_samples_per_s"]["resident"], row["train_samples_per_s"]["synthetic"]
            row["resident_vs_synthetic_percent"] = round(100.0 * (r["median"] / s["median"] - 1.0), 2)
            row["synthetic_spread_percent"] = round(100.0 * (s["max"] - s["min"]) / s["median"], 2)
            h = row["train_samples_per_s"]["preloaded"]
            row["resident_vs_preloaded_percent"] = round(100.0 * (r["median"] / h["median"] - 1.0), 2)
            row["preloaded_spread_percent"] = round(100.0 * (h["max"] - h["min"]) / h["median"], 2)
            out["batch"][str(batch)] = row
            del pipe, model
            torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
