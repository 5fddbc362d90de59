"""Device-resident cutout batches on the GPU (csrc/cutout.hip, sbgm_danra_amd/resident_data.py) against the host restatement of
tests/cutout_ref.py: the exact distance transform and the normalised SDF, the origin draw, the one-launch gather with its transform
programs, the loader, and one training step fed by it.

Bounds.  d2, the draw, the crops, the affine programs, the mask and the points are integers or separately rounded fp32 ops: exact.  The
sdf is computed in fp64 and rounded once; the restatement's fp64 value can differ from the device's in its last bits only, which can at
most flip that rounding: 1 fp32 ulp.  Programs with exp / log: the 1e-6 max-rel of tests/test_gpu_postproc.py for the same cases."""
import ctypes as C
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch
import yaml

sys.path.insert(0, os.path.dirname(__file__))
import cutout_ref as R  # noqa: E402
from transform_cases import EXACT, cases  # noqa: E402
from util_models import load_golden, maxrel  # noqa: E402

from oracle import transforms_ref as TR  # noqa: E402
from sbgm_danra_amd import _native as N  # noqa: E402
from sbgm_danra_amd import resident_data as RD  # noqa: E402
from sbgm_danra_amd import special_transforms as ST  # noqa: E402
from sbgm_danra_amd.config_loader import to_config  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- SDF ----------------------------------------------------------------------------------------------------------------------
def run_sdf(mask, want_d2=True):
    B, h, w = mask.shape
    m = torch.from_numpy(np.ascontiguousarray(mask, dtype=np.float32)).cuda()
    sdf = torch.full((B, h, w), float("nan"), device="cuda")
    d2 = torch.full((B, h, w), -7, dtype=torch.int32, device="cuda") if want_d2 else None
    nbytes = N.lib().sbgm_sdf_workspace_bytes(B, h, w)
    assert nbytes > 0
    ws = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda")          # the op clears what it needs cleared
    N.check(N.lib().sbgm_sdf_from_mask(m.data_ptr(), sdf.data_ptr(), N.ptr(d2), ws.data_ptr(), B, h, w, N.stream()))
    return sdf.cpu().numpy(), None if d2 is None else d2.cpu().numpy()


def check_sdf(mask):
    sdf, d2 = run_sdf(mask)
    want_d2 = np.stack([R.edt_squared_scipy(m) for m in mask])
    want = np.stack([R.sdf_ref(m) for m in mask])
    ulps = R.ulp_distance_f32(sdf, want.astype(np.float32))
    print(f"sdf {mask.shape}: max ulp distance {int(ulps.max())}, d2 mismatches {int((d2 != want_d2).sum())}")
    assert np.array_equal(d2, want_d2)
    assert ulps.max() <= 1
    return sdf, d2


def random_masks(shape, land, seed):
    rng = np.random.default_rng(seed)
    m = (rng.random((3,) + shape) < land).astype(np.float32)
    for b in range(3):                                   # a mixed sample has a coast: at least one land and one sea pixel, when it can
        if not m[b].any():
            m[b].flat[rng.integers(m[b].size)] = 1.0
        if m[b].all() and m[b].size > 1:
            m[b].flat[rng.integers(m[b].size)] = 0.0
    return m


@pytest.mark.parametrize("shape,land", [((1, 7), 0.5), ((5, 1), 0.5), ((9, 13), 0.5), ((33, 20), 0.5), ((64, 64), 0.02), ((64, 64), 0.5),
                                        ((64, 64), 0.97), ((70, 300), 0.02)])
def test_sdf_matches_scipy(shape, land):
    check_sdf(random_masks(shape, land, seed=shape[0] * 1000 + shape[1] + int(land * 100)))


def test_sdf_single_land_pixel_in_a_corner():
    """the longest possible search: the nearest land pixel of the opposite corner is the whole diagonal away"""
    m = np.zeros((3, 128, 128), dtype=np.float32)
    m[0, 0, 0] = m[1, 127, 127] = m[2, 0, 127] = 1.0
    sdf, d2 = check_sdf(m)
    assert d2[0, 127, 127] == d2[1, 0, 0] == d2[2, 127, 0] == 2 * 127 ** 2
    assert sdf[0, 0, 0] == 1.0 and sdf[0, 127, 127] == 0.0


def test_sdf_without_a_coastline_and_repeatability():
    m = random_masks((33, 20), 0.5, seed=5)
    m[0] = 1.0                                           # all land: 1 (the reference: 0 / 0)
    m[1] = 0.0                                           # all sea: 0 (the reference: scipy on an input without background)
    sdf, d2 = check_sdf(m)
    assert (sdf[0] == 1.0).all() and (d2[0] == 0).all()
    assert (sdf[1] == 0.0).all() and (d2[1] == -1).all()
    assert sdf[2].min() == 0.0 and sdf[2].max() == 1.0
    again, d2_again = run_sdf(m)
    assert np.array_equal(sdf.view(np.int32), again.view(np.int32)) and np.array_equal(d2, d2_again)
    no_d2, _ = run_sdf(m, want_d2=False)                 # d2 is optional
    assert np.array_equal(sdf.view(np.int32), no_d2.view(np.int32))


def test_sdf_rejects_oversized_sides():
    x = torch.zeros(8, device="cuda")
    assert N.lib().sbgm_sdf_from_mask(x.data_ptr(), x.data_ptr(), None, x.data_ptr(), 1, 4097, 1, N.stream()) != 0


# ---- draw ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_off", [(0, 0), (1, 461), (52, 52)])
def test_draw_matches_reference(max_off):
    h, w, r0, c0 = 128, 128, 170, 40
    rect = [r0, r0 + h + max_off[0], c0, c0 + w + max_off[1]]
    for seed, draw in ((42, 0), (2 ** 40 + 3, R.draw_number("train", 7, 11, 1))):
        o = torch.full((64, 2), -1, dtype=torch.int32, device="cuda")
        N.check(N.lib().sbgm_cutout_draw(seed, draw, 64, (C.c_int * 4)(*rect), h, w, 589, 789, o.data_ptr(), N.stream()))
        assert np.array_equal(o.cpu().numpy(), R.draw_origins(seed, draw, 64, rect, (h, w)))


# ---- gather -------------------------------------------------------------------------------------------------------------------
def run_gather(fields, items, origins, crop, Hd, Wd):
    """fields: [(device tensor, n_items, is_mask, program)] -> list of [B, 1, h, w] cpu tensors; one launch"""
    lib, B, nf = N.lib(), len(items), len(fields)
    programs = RD.upload_programs([(is_mask, prog) for _s, _n, is_mask, prog in fields], "cuda")
    srcs, dsts, counts, outs = (N._vp * nf)(), (N._vp * nf)(), (C.c_int * nf)(), []
    for i, (src, n, _m, _p) in enumerate(fields):
        outs.append(torch.full((B, 1) + tuple(crop), 123.0, device="cuda"))
        srcs[i], dsts[i], counts[i] = src.data_ptr(), outs[-1].data_ptr(), n
    it = torch.tensor(items, dtype=torch.int32, device="cuda")
    og = torch.tensor(origins, dtype=torch.int32, device="cuda")
    N.check(lib.sbgm_cutout_gather(srcs, dsts, counts, nf, programs.data_ptr(), it.data_ptr(), og.data_ptr(), B, Hd, Wd, crop[0], crop[1],
                                   N.stream()))
    return [o.cpu() for o in outs]


@pytest.mark.parametrize("crop", [(16, 20), (16, 18), (1, 1)])
def test_gather_matches_slicing_and_transforms(golden_dir, crop):
    Hd, Wd, n, items = 37, 53, 5, [4, 0, 2]
    h, w = crop
    origins = [(3, 7), (0, 0), (Hd - h, Wd - w)]          # an odd x0, the first corner and the last one
    g = load_golden(os.path.join(golden_dir, "transforms.npz"))
    rng = np.random.default_rng(3)
    table = cases()
    names = sorted(table)                                 # 16 programs: every case of tests/transform_cases.py
    stacks = {key: np.resize(g[key].numpy().ravel(), (n, Hd, Wd)).astype(np.float32) for key in ("z", "phys")}
    lsm = rng.random((Hd, Wd), dtype=np.float32)           # not binary: the re-binarise after the crop has something to do
    lsm[0, 0], lsm[3, 7] = 0.5, np.nextafter(np.float32(0.5), np.float32(1))
    topo = (rng.random((Hd, Wd), dtype=np.float32) * 2400 - 12).astype(np.float32)
    dev = {k: torch.from_numpy(v).cuda() for k, v in stacks.items()}
    fields = [(dev["z"], n, 0, [])]                       # identity
    for name in names:
        mk, key, scale = table[name]
        assert scale in (1, 3)
        src = dev[key] if scale == 1 else dev.setdefault(key + "3", torch.from_numpy(stacks[key] * np.float32(scale)).cuda())
        fields.append((src, n, 0, mk(ST).program()))
    topo_scale = (-1.0, 1.0, float(topo.min()), float(topo.max()))
    fields.append((torch.from_numpy(lsm).cuda(), 0, 1, []))
    fields.append((torch.from_numpy(topo).cuda(), 0, 0, ST.Scale(*topo_scale).program()))
    assert len(fields) == 19                              # the most one launch takes: 17 stacks and 2 planes
    got = run_gather(fields, items, origins, crop, Hd, Wd)
    assert torch.equal(got[0], torch.from_numpy(R.crop_transform(stacks["z"], items, origins, crop)))
    for name, out in zip(names, got[1:17]):
        mk, key, scale = table[name]
        want = torch.from_numpy(R.crop_transform(stacks[key] * np.float32(scale), items, origins, crop, mk(TR)))
        if name in EXACT:
            assert torch.equal(out, want), name
        else:
            err = maxrel(out, want)
            print(f"gather {crop} {name}: max-rel {err:.3e}")
            assert err <= 1e-6, name
    want_lsm = torch.from_numpy(R.crop_transform(lsm, items, origins, crop, None, is_mask=True))
    assert torch.equal(got[17], want_lsm) and set(got[17].unique().tolist()) <= {0.0, 1.0}
    if crop != (1, 1):
        assert got[17][0, 0, 0, 0] == 1.0 and got[17][1, 0, 0, 0] == 0.0      # nextafter(0.5) is land, 0.5 itself is not
    assert torch.equal(got[18], torch.from_numpy(R.crop_transform(topo, items, origins, crop, TR.Scale(*topo_scale))))


def test_gather_guards_items_and_origins():
    """an item or an origin outside its stack is not read: the sample is NaN, its neighbours are untouched"""
    Hd, Wd, n = 12, 16, 2
    src = torch.arange(n * Hd * Wd, dtype=torch.float32, device="cuda").reshape(n, Hd, Wd)
    plane = torch.ones(Hd, Wd, device="cuda")
    for crop in ((8, 8), (8, 7)):
        h, w = crop
        got = run_gather([(src, n, 0, []), (plane, 0, 0, [])], [1, 2, -1, 0, 0, 0],
                         [(0, 0), (0, 0), (0, 0), (Hd - h + 1, 0), (0, Wd - w + 1), (-1, 0)], crop, Hd, Wd)
        assert torch.equal(got[0][0, 0], src[1, :h, :w].cpu())
        assert torch.isnan(got[0][1:]).all()
        assert (got[1][:3] == 1).all() and torch.isnan(got[1][3:]).all()       # a plane has no item to get wrong


# ---- loader -------------------------------------------------------------------------------------------------------------------
HD, WD, CROP, RECT = 40, 56, (32, 32), [2, 38, 4, 52]
STATS = {"prcp_hr": {"log_mean": -1.2345, "log_std": 2.0321, "log_min": -4.60517, "log_max": 5.7038},
         "temp_lr": {"mean": 8.7012, "std": 6.1923},
         "prcp_lr": {"log_mean": -0.5, "log_std": 1.75, "log_min": -4.60517, "log_max": 4.5}}


def make_arrays(n, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:HD, 0:WD]
    lsm = ((yy - 20) ** 2 + (xx - 30) ** 2 < 150).astype(np.float32)             # an island: every 32x32 crop of RECT has a coast
    return {"prcp_hr": (rng.random((n, HD, WD)) ** 4 * 60).astype(np.float32), "temp_lr": rng.normal(8, 6, (n, HD, WD)).astype(np.float32),
            "prcp_lr": (rng.random((n, HD, WD)) ** 4 * 40).astype(np.float32), "lsm": lsm,
            "topo": (rng.random((HD, WD)) * 900 - 5).astype(np.float32), "classifier": (np.arange(n) % 4 + 1).astype(np.int64)}


def make_cfg(tmp_path, zscore_only=False, **geo):
    raw = yaml.safe_load(open(os.path.join(ROOT, "sbgm_danra_amd", "config", "default_config.yaml")))
    for sec in ("highres", "lowres"):
        raw[sec].update(data_size=list(CROP), cutout_domains=list(RECT), full_domain_dims=[HD, WD])
    raw["highres"]["scaling_method"] = "zscore" if zscore_only else "log_zscore"
    raw["lowres"].update(condition_variables=["temp", "prcp"], scaling_methods=["zscore", "zscore" if zscore_only else "log_zscore"])
    raw["transforms"].update(sample_w_cutouts=True, scaling=True)
    raw["stationary_conditions"]["geographic_conditions"].update(sample_w_geo=True, sample_w_sdf=True, **geo)
    raw["stationary_conditions"]["seasonal_conditions"]["sample_w_cond_season"] = True
    raw["training"].update(batch_size=2, sdf_weighted_loss=True)
    raw["paths"] = {k: str(tmp_path / k) for k in ("data_dir", "checkpoint_dir", "sample_dir", "path_save", "stats_load_dir")}
    return to_config(raw)


def ref_transforms(arrays, zscore_only=False):
    log = lambda s: TR.PrcpLogTransform(scale_type="log_zscore", glob_mean_log=s["log_mean"], glob_std_log=s["log_std"],     # noqa: E731
                                        glob_min_log=s["log_min"], glob_max_log=s["log_max"], buffer_frac=0.5)
    z = lambda s: TR.ZScoreTransform(s["mean"], s["std"])                                                                    # noqa: E731
    t = {"temp_lr": z(STATS["temp_lr"]), "topo": TR.Scale(0.0, 1.0, float(arrays["topo"].min()), float(arrays["topo"].max()))}
    t["prcp_hr"], t["prcp_lr"] = (z(ZSTATS["prcp_hr"]), z(ZSTATS["prcp_lr"])) if zscore_only else (log(STATS["prcp_hr"]), log(STATS["prcp_lr"]))
    return t


ZSTATS = {"prcp_hr": {"mean": 3.5, "std": 7.25}, "prcp_lr": {"mean": 2.5, "std": 5.5}, "temp_lr": STATS["temp_lr"]}
EXACT_KEYS = ("temp_lr", "lsm", "lsm_hr", "topo", "classifier", "hr_points", "lr_points")


def compare_batch(batch, want, log_keys=("prcp_hr", "prcp_lr")):
    assert set(batch) == set(want), (sorted(batch), sorted(want))
    for k, v in batch.items():
        assert v.is_cuda and tuple(v.shape) == want[k].shape, k
        assert v.dtype == (torch.int64 if k in ("classifier", "hr_points", "lr_points") else torch.float32), k
        w = torch.from_numpy(want[k])
        if k == "sdf":
            ulps = R.ulp_distance_f32(v.cpu().numpy(), want[k])
            print(f"loader sdf: max ulp distance {int(ulps.max())}")
            assert ulps.max() <= 1
        elif k in log_keys:
            assert maxrel(v.cpu(), w) <= 1e-6, k
        else:
            assert torch.equal(v.cpu(), w), k


@pytest.fixture()
def split_files(tmp_path):
    paths = {}
    for split, n, seed in (("train", 6, 1), ("valid", 4, 2), ("gen", 3, 3)):
        paths[split] = str(tmp_path / f"{split}.npz")
        np.savez(paths[split], **make_arrays(n, seed))
    return paths


def test_loader_batches_match_reference(tmp_path, split_files):
    cfg = make_cfg(tmp_path)
    arrays = make_arrays(6, 1)
    fields = RD.ResidentFields(split_files["train"], "prcp", ["temp", "prcp"])
    assert (fields.n_items, fields.Hd, fields.Wd) == (6, HD, WD)
    dl = RD.ResidentCutoutLoader(fields, cfg, "train", 2, seed=11, stats=STATS)
    assert len(dl) == 3
    tr = ref_transforms(arrays)
    for epoch in (0, 1):
        dl.set_epoch(epoch)
        order = np.random.default_rng([11, epoch]).permutation(6)
        assert np.array_equal(dl.item_order(), order)
        batches = list(dl)
        assert len(batches) == 3
        for i, batch in enumerate(batches):
            items = order[2 * i:2 * i + 2]
            origins = R.draw_origins(11, R.draw_number("train", epoch, i), 2, RECT, CROP)
            want = R.batch_ref(arrays, "prcp_hr", ["temp_lr", "prcp_lr"], items, origins, CROP, tr, with_classes=True)
            compare_batch(batch, want)
            assert batch["lsm"].shape == (2, 1, 32, 32) and batch["hr_points"][:, 1].tolist() == (origins[:, 0] + 32).tolist()


def test_loader_epochs_shards_and_switches(tmp_path, split_files):
    cfg = make_cfg(tmp_path)
    fields = RD.ResidentFields(split_files["train"], "prcp", ["temp", "prcp"])
    mk = lambda **kw: RD.ResidentCutoutLoader(fields, cfg, kw.pop("split", "train"), 2, seed=11, stats=STATS, **kw)      # noqa: E731
    a, b = mk(), mk()
    ea0, eb0 = list(a), list(b)                           # two loaders, one seed: identical epochs
    for x, y in zip(ea0, eb0):
        assert set(x) == set(y) and all(torch.equal(x[k], y[k]) for k in x)
    assert a.epoch == 1                                   # a loop that never calls set_epoch still moves on
    ea1 = list(a)
    assert not torch.equal(torch.cat([x["hr_points"] for x in ea0]), torch.cat([x["hr_points"] for x in ea1]))
    b.set_epoch(0)
    assert all(torch.equal(x["prcp_hr"], y["prcp_hr"]) for x, y in zip(ea0, list(b)))
    v = mk(split="valid")
    assert len(v) == 3 and np.array_equal(v.item_order(), np.arange(6))
    v0 = list(v)
    v.set_epoch(5)
    v5 = list(v)
    assert all(torch.equal(x[k], y[k]) for x, y in zip(v0, v5) for k in x)           # a validation loss is comparable across epochs
    assert not torch.equal(v0[0]["hr_points"], ea0[0]["hr_points"]) or not torch.equal(v0[1]["hr_points"], ea0[1]["hr_points"])
    # shards: disjoint, and together every item; the classifier of this file is item % 4 + 1, the HR field identifies the item
    s0, s1 = mk(shard=(0, 2), drop_last=False), mk(shard=(1, 2), drop_last=False)
    o0, o1 = s0.item_order(), s1.item_order()
    assert not set(o0) & set(o1) and sorted(list(o0) + list(o1)) == list(range(6))
    assert len(s0) == 2 and len(mk(shard=(0, 2))) == 1     # 3 items a rank: the training loader drops the ragged last batch
    seen = torch.cat([x["classifier"] for x in s0] + [x["classifier"] for x in s1]).cpu().tolist()
    assert sorted(seen) == sorted((np.arange(6) % 4 + 1).tolist())
    assert s0.draw_number(0) != s1.draw_number(0)
    # switches
    cfg2 = make_cfg(tmp_path)
    cfg2.stationary_conditions.geographic_conditions.sample_w_sdf = False
    x = next(iter(RD.ResidentCutoutLoader(fields, cfg2, "valid", 2, seed=11, stats=STATS)))
    assert "sdf" not in x and "lsm" in x and "topo" in x
    cfg2.stationary_conditions.geographic_conditions.sample_w_geo = False
    cfg2.stationary_conditions.seasonal_conditions.sample_w_cond_season = False
    x = next(iter(RD.ResidentCutoutLoader(fields, cfg2, "valid", 2, seed=11, stats=STATS)))
    assert set(x) == {"prcp_hr", "temp_lr", "prcp_lr", "hr_points", "lr_points"}
    cfg2.stationary_conditions.geographic_conditions.sample_w_sdf = True            # the SDF alone still needs the mask
    x = next(iter(RD.ResidentCutoutLoader(fields, cfg2, "valid", 2, seed=11, stats=STATS)))
    assert set(x) == {"prcp_hr", "temp_lr", "prcp_lr", "hr_points", "lr_points", "lsm_hr", "sdf"}


def test_get_dataloader_switches_on_the_config_section(tmp_path, split_files):
    from torch.utils.data import DataLoader

    from sbgm_danra_amd.training_utils import get_dataloader, get_gen_dataloader
    cfg = make_cfg(tmp_path)
    assert all(isinstance(d, DataLoader) for d in get_dataloader(cfg)) and isinstance(get_gen_dataloader(cfg), DataLoader)
    for key, model, var in (("prcp_hr", "DANRA", "prcp"), ("temp_lr", "ERA5", "temp"), ("prcp_lr", "ERA5", "prcp")):
        d = tmp_path / "stats_load_dir" / model / var / "all"
        d.mkdir(parents=True)
        (d / f"global_stats__{model}__{HD}x{WD}__crop__2_38_4_52__{var}__all.json").write_text(json.dumps(STATS[key]))
    cfg.data_handling.resident_fields = split_files
    cfg.data_handling.n_gen_samples = 3
    cfg.training.seed = 11
    train, valid, gen = get_dataloader(cfg, shard=(0, 1))
    assert [type(d) for d in (train, valid, gen)] == [RD.ResidentCutoutLoader] * 3
    assert (len(train), len(valid), len(gen)) == (3, 2, 1) and (train.split, valid.split, gen.split) == ("train", "valid", "gen")
    direct = RD.ResidentCutoutLoader(RD.ResidentFields(split_files["train"], "prcp", ["temp", "prcp"]), cfg, "train", 2, seed=11, stats=STATS)
    x, y = next(iter(train)), next(iter(direct))
    assert set(x) == set(y) and all(torch.equal(x[k], y[k]) for k in x)              # the statistics files and the dicts agree
    ev = get_gen_dataloader(cfg)
    assert isinstance(ev, RD.ResidentCutoutLoader) and ev.batch_size == cfg.evaluation.batch_size and len(ev) == 1
    assert next(iter(ev))["prcp_hr"].shape == (3, 1, 32, 32)                        # the ragged only batch of a split that keeps it


# ---- one training step ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [False, "auto"])
def test_one_training_step_from_resident_batches(tmp_path, use_graph):
    from sbgm_danra_amd.score_unet import diffusion_coeff_fn, loss_fn, marginal_prob_std_fn
    from sbgm_danra_amd.training import TrainingPipeline_general
    from sbgm_danra_amd.training_utils import get_model, get_optimizer
    cfg = make_cfg(tmp_path, zscore_only=True)             # affine programs only: the two batches differ by the sdf's last bit at most
    cfg.training.use_hip_graph = use_graph
    arrays = make_arrays(2, 9)
    path = str(tmp_path / "train.npz")
    np.savez(path, **arrays)
    dl = RD.ResidentCutoutLoader(RD.ResidentFields(path, "prcp", ["temp", "prcp"]), cfg, "train", 2, seed=5, stats=ZSTATS)
    assert len(dl) == 1
    g = torch.Generator().manual_seed(3)
    noise = ((torch.rand(2, generator=g) * 0.9 + 0.05).cuda(), torch.randn(2, 1, 32, 32, generator=g).cuda())
    loss = functools.partial(loss_fn, noise=noise)

    def pipeline():
        torch.manual_seed(0)
        model, _, _ = get_model(cfg)
        model = model.cuda()
        return TrainingPipeline_general(model, loss, marginal_prob_std_fn, diffusion_coeff_fn, get_optimizer(cfg, model),
                                        torch.device("cuda"), None, cfg)
    pipe = pipeline()
    got = pipe.train_batches(dl, epochs=1, verbose=False)
    assert np.isfinite(got)
    items = np.random.default_rng([5, 0]).permutation(2)
    origins = R.draw_origins(5, R.draw_number("train", 0, 0), 2, RECT, CROP)
    ref = R.batch_ref(arrays, "prcp_hr", ["temp_lr", "prcp_lr"], items, origins, CROP, ref_transforms(arrays, zscore_only=True),
                      with_classes=True)
    ref_pipe = pipeline()
    ref_pipe.model.train()
    _, want = ref_pipe._loss({k: torch.from_numpy(v).cuda() for k, v in ref.items()})
    print(f"training step (use_hip_graph={use_graph}): loss {got:.8f}, from the rebuilt batch {float(want):.8f}")
    assert abs(got - float(want)) <= 1e-5 * abs(float(want))
