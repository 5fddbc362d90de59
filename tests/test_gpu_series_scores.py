"""GPU suite for the pooled ensemble verification of a series (verification.series_ensemble_scores; csrc/verify_series.hip,
DESIGN.md §11 K58 - K60) against the numpy restatement tests/series_scores_ref.py.

Bounds.  The integers (count, rank_hist, table) and the four maps are asserted bit-equal: the maps are the same IEEE fp64 ops in
the same order with contraction off, rounded to fp32 once.  clim_crps: 1 fp32 ulp — its fp64 pair sum is a sum of non-negative
exact terms, so any order agrees to n^2 2^-53 <= 2.5e-10 relative at n = 1500, far below half an fp32 ulp.  crpss map: the same bound
carried through the division, spacing(float32(|want|)) + 1e-9 |F / C|.  daily, scores, skill_scores: rtol 1e-9 — sums of at most
3e6 fp64 terms here, worst-case order effect 3e6 2^-53 = 3.3e-10; the pooled crpss is checked through its sum F and sum C, not the
cancelling difference.  exceedance: rtol 1e-12 against the formulas applied to the exact table.  The largest deviation per output
is printed before it is asserted."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

import series_scores_ref as R
from sbgm_danra_amd import verification as V

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
f32 = np.float32
MASKS = [None, ("hw", "uint8"), ("dhw", "bool"), ("hw", "float32"), ("dhw", "uint8"), ("hw", "bool"), ("dhw", "float32")]
THRESHOLDS = {0: [], 1: [1.0], 5: [0.25, 1.0, 2.0, 3.5, 5.0], 16: [0.25 * k for k in range(1, 17)]}
PLANTED = 8                                                               # columns of row 0 with a planted pixel
# (shape, D, M, T, G, kind, mask index): every D, M, T, G and mask kind of the issue appears; D = 1500 crosses every day chunk
CASES = [((37, 53), 1, 16, 5, 0, "grid", 0), ((32, 48), 2, 3, 1, 1, "rain", 1), ((37, 53), 3, 17, 16, 0, "grid", 2),
         ((32, 48), 17, 33, 5, 4, "rain", 3), ((37, 53), 65, 16, 16, 16, "grid", 4), ((32, 48), 65, 2, 0, 4, "rain", 5),
         ((37, 53), 366, 3, 5, 4, "rain", 6), ((32, 48), 366, 17, 1, 16, "grid", 0), ((32, 48), 1500, 2, 5, 4, "grid", 1)]
IDS = [f"{s[0]}x{s[1]}-D{D}-M{M}-T{T}-G{G}-{kind}-mask{mi}" for s, D, M, T, G, kind, mi in CASES]


def make_series(rng, kind, D, M, shape, groups):
    """grid: multiples of 0.25 in [0, 5] (ties, and values exactly on the thresholds); rain: max(3 z - 2, 0), more than half exact
    zeros, some values exactly 1.0.  About 2 % of the truth NaN, and about 2 % of the cells with one NaN member.
    Planted pixels of row 0: (0,0) no valid day; (0,1) one valid day; (0,2) two valid days; (0,3) constant truth; (0,4) one
    member NaN on day 0 only; (0,5) only two valid days in group 0; (0,6) truth below every member; (0,7) truth above."""
    def draw(size):
        if kind == "grid":
            return (rng.integers(0, 21, size=size) * 0.25).astype(f32)
        a = np.maximum(f32(3.0) * rng.standard_normal(size).astype(f32) - f32(2.0), f32(0.0))
        a[rng.random(size) < 0.05] = f32(1.0)
        return a
    ens, obs = draw((D, M, *shape)), draw((D, *shape))
    obs[rng.random(obs.shape) < 0.02] = np.nan
    hit = rng.random(obs.shape) < 0.02
    which = rng.integers(0, M, size=obs.shape)
    for m in range(M):
        ens[:, m][hit & (which == m)] = np.nan
    clean_e, clean_o = draw((D, M, PLANTED)), draw((D, PLANTED))          # the planted pixels start without NaN
    ens[:, :, 0, :PLANTED], obs[:, 0, :PLANTED] = clean_e, clean_o
    obs[:, 0, 0] = np.nan
    obs[1:, 0, 1] = np.nan
    obs[2:, 0, 2] = np.nan
    obs[:, 0, 3] = f32(1.0)
    ens[0, min(1, M - 1), 0, 4] = np.nan
    if groups is not None:
        days0 = np.flatnonzero(np.asarray(groups) == 0)
        obs[days0[2:], 0, 5] = np.nan
    obs[:, 0, 6], obs[:, 0, 7] = f32(-1.0), f32(100.0)
    return ens, obs


def make_groups(rng, G, D, kind):
    """None for G = 0; else every id 0..G-1 at least once: contiguous blocks (seasons) for rain, shuffled for grid"""
    if G == 0:
        return None
    g = (np.arange(D) * G // D).astype(np.int64) if D >= G else np.arange(D) % G
    return g if kind == "rain" else rng.permutation(g)


def make_mask(rng, spec, D, shape):
    if spec is None:
        return None
    layout, dtype = spec
    m = rng.random((D, *shape) if layout == "dhw" else shape) < 0.9
    m[..., 0, :PLANTED] = True                                               # the planted pixels stay admitted
    return m.astype(np.uint8) if dtype == "uint8" else m if dtype == "bool" else np.where(m, f32(0.75), f32(0.5)).astype(f32)


def assert_planted(want, D, M, G):
    """each special kind of pixel is present in the reference output, so no case passes by being empty"""
    n = want["count"]
    assert n[0, 0] == 0 and np.isnan(want["crps"][0, 0]) and n[0, 1] == 1 and not np.isnan(want["crps"][0, 1])
    assert np.isnan(want["clim_crps"][0, 1]) and n[0, 4] == D - 1 and n[0, 6] == n[0, 7] == D
    assert want["rank_hist"][0, 0] >= D and want["rank_hist"][0, M] >= D       # truth below / above every member
    if D >= 2:
        assert n[0, 2] == 2 and np.isnan(want["clim_crps"][0, 2]) and np.isnan(want["crpss"][0, 2])
    if D >= 3:
        assert n[0, 3] == D and want["clim_crps"][0, 3] == 0 and np.isnan(want["crpss"][0, 3]), "constant truth"
        assert (~np.isnan(want["crpss"])).any() and want["skill_scores"][0, 0] > 0
    if G >= 2 and D >= 17:
        assert want["_n"][1, 0, 5] == 2 and n[0, 5] >= 3 and np.isnan(want["_C"][1, 0, 5]), "a group with fewer than 3 valid days"


def to_dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def device_call(ens, obs, thresholds=(), groups=None, mask=None, seed=0, **kw):
    r = V.series_ensemble_scores(to_dev(ens), to_dev(obs), thresholds, groups=groups, mask=to_dev(mask), seed=seed, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


@functools.lru_cache(maxsize=None)
def _case(index):
    shape, D, M, T, G, kind, mi = CASES[index]
    rng = np.random.default_rng([index, D, M])
    groups = make_groups(rng, G, D, kind)
    ens, obs = make_series(rng, kind, D, M, shape, groups)
    mask = make_mask(rng, MASKS[mi], D, shape)
    want = R.series_ensemble_scores(ens, obs, THRESHOLDS[T], groups, mask, seed=index + 1)
    got = device_call(ens, obs, THRESHOLDS[T], None if groups is None else groups.tolist(), mask, seed=index + 1)
    return ens, obs, mask, groups, want, got


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def assert_bit_equal(got, want, keys=V.SERIES_KEYS, tag=""):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (tag, k, got[k].dtype, got[k].shape)
        if got[k].dtype.kind == "f":
            np.testing.assert_array_equal(np.isnan(got[k]), np.isnan(want[k]), err_msg=f"{tag} {k}: NaN positions")
            ok = ~np.isnan(want[k])
            view = np.int32 if got[k].dtype == np.float32 else np.int64
            np.testing.assert_array_equal(got[k][ok].view(view), want[k][ok].view(view), err_msg=f"{tag} {k}")
        else:
            np.testing.assert_array_equal(got[k], want[k], err_msg=f"{tag} {k}")


def rel_dev(got, want):
    both = ~np.isnan(got) & ~np.isnan(want) & (want != 0)
    return float((np.abs(got[both] - want[both]) / np.abs(want[both])).max()) if both.any() else 0.0


def assert_equal_to_reference(got, want, tag):
    assert set(got) == set(V.SERIES_KEYS), tag
    for k in V.SERIES_KEYS:
        assert got[k].shape == want[k].shape, (tag, k, got[k].shape, want[k].shape)
    ok3 = ~np.isnan(want["clim_crps"])
    ulp = np.spacing(np.maximum(np.abs(want["clim_crps"]), np.finfo(f32).tiny).astype(f32)).astype(np.float64)
    clim_dev = np.abs(got["clim_crps"].astype(np.float64) - want["clim_crps"])[ok3] / ulp[ok3]
    okc = ~np.isnan(want["crpss"])
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.abs(want["_F"][0] / want["_C"][0]) if "_F" in want else np.zeros(want["crpss"].shape)
    bound = np.spacing(np.abs(want["crpss"]).astype(f32)).astype(np.float64) + 1e-9 * ratio
    crpss_dev = np.abs(got["crpss"].astype(np.float64) - want["crpss"])
    print(f"{tag}: clim_crps {clim_dev.max() if clim_dev.size else 0:g} ulp; crpss {(crpss_dev[okc] / bound[okc]).max() if okc.any() else 0:g} "
          f"of its bound; relative: " + ", ".join(f"{k}={rel_dev(got[k], want[k]):.3g}" for k in ("daily", "scores", "skill_scores", "exceedance")))
    assert_bit_equal(got, want, ("count", "rank_hist", "table") + V.SERIES_MAP_KEYS, tag)
    assert got["count"].dtype == np.int32 and got["rank_hist"].dtype == np.int64 and got["clim_crps"].dtype == np.float32
    for k in V.SERIES_CLIM_MAP_KEYS:
        np.testing.assert_array_equal(np.isnan(got[k]), np.isnan(want[k]), err_msg=f"{tag} {k}: NaN positions")
    assert (clim_dev <= 1.0).all(), (tag, clim_dev.max())
    assert (crpss_dev[okc] <= bound[okc]).all(), tag
    for k in ("daily", "scores"):
        np.testing.assert_allclose(got[k], want[k], rtol=1e-9, atol=0, equal_nan=True, err_msg=f"{tag} {k}")
    gs, ws = got["skill_scores"], want["skill_scores"]
    np.testing.assert_array_equal(gs[:, 0], ws[:, 0], err_msg=f"{tag} skill cells")
    np.testing.assert_allclose(gs[:, 1:3], ws[:, 1:3], rtol=1e-9, atol=0, equal_nan=True, err_msg=f"{tag} skill means")
    np.testing.assert_allclose(gs[:, 1] * gs[:, 0], ws[:, 1] * ws[:, 0], rtol=1e-9, atol=0, equal_nan=True, err_msg=f"{tag} sum F")
    np.testing.assert_allclose(gs[:, 2] * gs[:, 0], ws[:, 2] * ws[:, 0], rtol=1e-9, atol=0, equal_nan=True, err_msg=f"{tag} sum C")
    np.testing.assert_array_equal(np.isnan(gs[:, 3]), np.isnan(ws[:, 3]), err_msg=f"{tag} pooled crpss: NaN rows")
    with np.errstate(invalid="ignore", divide="ignore"):
        own = 1.0 - gs[:, 1] / gs[:, 2]                                        # the device's crpss from the device's own sums
    sel = ~np.isnan(gs[:, 3])
    assert (np.abs(gs[sel, 3] - own[sel]) <= 1e-12 * (1.0 + np.abs(gs[sel, 1] / gs[sel, 2]))).all(), tag
    np.testing.assert_allclose(got["exceedance"], want["exceedance"], rtol=1e-12, atol=0, equal_nan=True, err_msg=f"{tag} exceedance")


@pytest.mark.parametrize("index", range(len(CASES)), ids=IDS)
def test_against_the_restatement(index):
    shape, D, M, T, G, kind, mi = CASES[index]
    ens, obs, mask, groups, want, got = _case(index)
    assert_planted(want, D, M, G)
    assert np.isnan(obs).mean() > 0.015 and 0.01 < np.isnan(ens).any(axis=1).mean() < 0.05
    if groups is not None:
        assert sorted(set(groups.tolist())) == list(range(G))
    if kind == "rain":
        assert (ens == 0).mean() > 0.5 and (obs == f32(1.0)).any()
    else:
        assert T == 0 or np.isin(obs[~np.isnan(obs)], np.asarray(THRESHOLDS[T], f32)).any()       # truths exactly on thresholds
    assert_equal_to_reference(got, want, IDS[index])


def test_every_setting_of_the_issue_appears_in_the_cases():
    assert {c[0] for c in CASES} == {(37, 53), (32, 48)} and {c[1] for c in CASES} == {1, 2, 3, 17, 65, 366, 1500}
    assert {c[2] for c in CASES} == {2, 3, 16, 17, 33} and {c[3] for c in CASES} == {0, 1, 5, 16} and {c[4] for c in CASES} == {0, 1, 4, 16}
    assert {c[5] for c in CASES} == {"grid", "rain"} and {c[6] for c in CASES} == set(range(len(MASKS)))
    assert [c for c in CASES if c[1] == 1500] == [((32, 48), 1500, 2, 5, 4, "grid", 1)]


def test_one_day_is_the_ensemble_and_exceedance_score():
    ens, obs, mask, _, _, got = _case(0)
    e, o = to_dev(ens[0]), to_dev(obs[0])
    es = V.ensemble_scores(e, o, seed=1)
    ex = V.exceedance_scores(e, o, THRESHOLDS[5])
    np.testing.assert_array_equal(got["rank_hist"][0], es["rank_hist"].cpu().numpy())
    np.testing.assert_array_equal(got["table"][0], ex["table"].cpu().numpy())
    np.testing.assert_array_equal(bits(got["crps"]), bits(es["crps"].cpu().numpy()))
    np.testing.assert_allclose(got["scores"][0], es["scores"].cpu().numpy(), rtol=1e-9, atol=0)
    np.testing.assert_allclose(got["daily"][0], es["scores"].cpu().numpy(), rtol=1e-9, atol=0)
    for j, k in enumerate(V.EXCEEDANCE_KEYS):
        np.testing.assert_array_equal(got["exceedance"][0, j].view(np.int64), ex[k].cpu().numpy().view(np.int64), err_msg=k)
    assert np.isnan(got["clim_crps"]).all() and got["skill_scores"][0, 0] == 0


def test_daily_rows_are_the_ensemble_scores_of_each_day():
    """on continuous data no rank needs a draw, so each day's histogram is that of ensemble_scores whatever block it draws from"""
    rng = np.random.default_rng(77)
    D, M, shape = 5, 16, (37, 53)
    ens, obs = rng.gamma(0.7, 3.0, size=(D, M, *shape)).astype(f32), rng.gamma(0.7, 3.0, size=(D, *shape)).astype(f32)
    obs[rng.random(obs.shape) < 0.02] = np.nan
    ens[:, 3][rng.random(obs.shape) < 0.02] = np.nan
    assert not (ens == obs[:, None]).any()
    got = device_call(ens, obs, seed=9)
    hist = np.zeros(M + 1, np.int64)
    for d in range(D):
        es = V.ensemble_scores(to_dev(ens[d]), to_dev(obs[d]), seed=9)
        np.testing.assert_allclose(got["daily"][d], es["scores"].cpu().numpy(), rtol=1e-9, atol=0, err_msg=f"day {d}")
        hist += es["rank_hist"].cpu().numpy()
    np.testing.assert_array_equal(hist, got["rank_hist"][0])
    assert hist.sum() == got["scores"][0, 0] == R.valid_cells(ens, obs).sum()


def test_rows_add_up_and_one_group_is_all_days():
    for index in (3, 4, 7):
        _, _, _, groups, _, got = _case(index)
        np.testing.assert_array_equal(got["rank_hist"][1:].sum(0), got["rank_hist"][0])
        np.testing.assert_array_equal(got["table"][1:].sum(0), got["table"][0])
        assert got["scores"][1:, 0].sum() == got["scores"][0, 0] == got["rank_hist"][0].sum() == got["count"].sum()
        if got["table"].shape[1]:
            assert (got["table"][0, :, :, 0].sum(1) == got["count"].sum()).all()
    ens, obs, mask, groups, _, got = _case(1)                                 # G = 1
    for k in ("scores", "rank_hist", "table", "exceedance", "skill_scores"):
        assert got[k].shape[0] == 2
        np.testing.assert_array_equal(got[k][1].view(np.int64), got[k][0].view(np.int64), err_msg=k)
    ens, obs, mask, groups, _, got = _case(4)
    one = device_call(ens, obs, THRESHOLDS[16], [0] * 65, mask, seed=5)
    for k in ("scores", "rank_hist", "table", "exceedance", "skill_scores"):
        np.testing.assert_array_equal(one[k][1].view(np.int64), one[k][0].view(np.int64), err_msg=k)
        np.testing.assert_array_equal(one[k][0].view(np.int64), got[k][0].view(np.int64), err_msg=k)


def test_layouts_chunking_repeat_and_climatology_switch():
    ens, obs, mask, groups, _, got = _case(6)                                 # rain, D = 366, M = 3, a float [D,H,W] mask
    thr, g, seed = THRESHOLDS[5], groups.tolist(), 7
    mdh = to_dev(np.ascontiguousarray(ens.transpose(1, 0, 2, 3)))             # [M, D, H, W], as Evaluation holds it
    view = mdh.permute(1, 0, 2, 3)
    assert not view.is_contiguous() and (view.stride(0), view.stride(1)) == (37 * 53, 366 * 37 * 53)
    o, m = to_dev(obs), to_dev(mask)

    def call(e, **kw):
        r = V.series_ensemble_scores(e, o, thr, groups=g, mask=m, seed=seed, **kw)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in r.items()}
    assert_bit_equal(call(view), got, tag="permuted view")
    assert_bit_equal(call(to_dev(ens)), got, tag="second call")
    lib = V.N.lib()
    query = lambda b: lib.sbgm_series_scores_workspace_bytes(366, 3, 37, 53, 5, 4, 1, b)      # noqa: E731
    middle = (query(0) + query(V.DEFAULT_WORKSPACE_BYTES)) // 2
    assert query(0) < query(middle) < query(V.DEFAULT_WORKSPACE_BYTES)        # three different day chunks: 32, some, all 366
    for b in (0, middle):
        assert_bit_equal(call(view, max_workspace_bytes=b), got, tag=f"max_workspace_bytes={b}")
    off = call(view, climatology=False)
    assert np.isnan(off["clim_crps"]).all() and np.isnan(off["crpss"]).all() and np.isnan(off["skill_scores"]).all()
    assert_bit_equal(off, got, ("count", "daily", "scores", "rank_hist", "table", "exceedance") + V.SERIES_MAP_KEYS, "climatology off")
    # a slice of the days of a longer tensor, and fp64 input, go through a copy and give the same
    longer = to_dev(np.concatenate([ens, ens[:3]]))
    assert_bit_equal({k: v.cpu().numpy() for k, v in
                      V.series_ensemble_scores(longer[:366].double(), o, thr, groups=g, mask=m, seed=seed).items()}, got, tag="fp64 slice")


def test_longest_record_and_most_members():
    """D = 4095 days on 2 x 8, and M = 4095 members with 16 thresholds (one threshold per workgroup of the counting kernel) on 2 x 3"""
    rng = np.random.default_rng(4095)
    ens, obs = make_series(rng, "grid", 4095, 2, (2, 8), None)
    want = R.series_ensemble_scores(ens, obs, [1.0], None, None, seed=1)
    assert_equal_to_reference(device_call(ens, obs, [1.0], seed=1), want, "D=4095")
    ens = (rng.integers(0, 21, size=(2, 4095, 2, 3)) * 0.25).astype(f32)
    obs = (rng.integers(0, 21, size=(2, 2, 3)) * 0.25).astype(f32)
    got = device_call(ens, obs, THRESHOLDS[16], [0, 1], seed=2)
    k = (ens[:, :, None] >= np.asarray(THRESHOLDS[16], f32)[None, None, :, None, None]).sum(1)          # [D, T, H, W]
    for t in range(16):
        np.testing.assert_array_equal(got["table"][0, t, :, 0], np.bincount(k[:, t].ravel(), minlength=4096), err_msg=f"t={t}")
    np.testing.assert_array_equal(got["table"][1:].sum(0), got["table"][0])
    assert got["rank_hist"][0].sum() == 12


# ---- --mode evaluate end to end -----------------------------------------------------------------------------------------------------

SECTION = {"thresholds": [1.0, 2.5], "climatology": True, "groups": [0, 0, 1, 1, 1], "seed": None}
BASE_METRICS = {"gen_type", "rank", "n_samples", "n_obs", "shape", "mask_stats", "pixel_stats", "spatial_stats", "daily_stats",
                "member", "members"}
BASE_FIELDS = ({f"pixel_{k}" for k in ("hist_gen", "hist_obs", "hist_value_edges", "hist_absdiff", "hist_absdiff_edges")} |
               {f"spatial_{k}_per_pixel" for k in ("count", "mae", "rmse", "bias")} | {f"daily_{k}" for k in ("count", "mae", "rmse")})
BASE_FILES = ["series_fields.npz", "series_metrics.json"]
ROW_KEYS = (set(V.ENSEMBLE_KEYS) | set(V.EXCEEDANCE_KEYS) |
            {"rank_reliability_index", "outside_fraction", "brier_skill", "climatology", "crpss"})


def _rainy(rng, shape):
    a = (rng.integers(0, 21, size=shape) * 0.25).astype(f32)
    a[rng.random(shape) < 0.02] = np.nan
    return a


def _evaluate(tmp_path, monkeypatch, tag, section):
    from sbgm_danra_amd.config_loader import load_config
    from sbgm_danra_amd.utils import get_model_string
    for k in ("DATA_DIR", "CKPT_DIR", "SAMPLE_DIR", "STATS_LOAD_DIR"):
        monkeypatch.setenv(k, str(tmp_path / k.lower()))
    monkeypatch.setenv("SLURM_CPUS_PER_TASK", "2")
    monkeypatch.setenv("PYTHONPATH", ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    raw = yaml.safe_load(open(os.path.join(ROOT, "sbgm_danra_amd", "config", "default_config.yaml")))
    raw["paths"]["evaluation_dir"] = str(tmp_path / f"ev_{tag}")
    raw["evaluation"].update(eval_gen_type=["series"], mask_stats=True, seed=11,
                             eval_stat_methods=["pixel_stats", "spatial_stats", "daily_stats"])
    if section is not None:
        raw["evaluation"]["series_scores"] = section
    cfg_path = tmp_path / f"run_{tag}.yaml"
    cfg_path.write_text(yaml.safe_dump(raw))
    name = get_model_string(load_config(str(cfg_path)))
    samples = tmp_path / "sample_dir" / "generation" / name / "generated_samples"
    if not samples.exists():
        samples.mkdir(parents=True)
        rng = np.random.default_rng(31)
        np.savez_compressed(samples / "gen_samples_series_n_5.npz", _rainy(rng, (5, 3, 16, 16)))
        np.savez_compressed(samples / "eval_samples_series_n_5.npz", _rainy(rng, (5, 16, 16)))
        np.savez_compressed(samples / "lsm_samples_series_n_5.npz", (rng.random((5, 1, 16, 16)) < 0.7).astype(f32))
        np.savez_compressed(samples / "series_index_series_n_5.npz", members=np.int64(3))
    subprocess.run([sys.executable, "-m", "sbgm_danra_amd.cli.main_app", "--config_path", str(cfg_path), "--mode", "evaluate"],
                   cwd=ROOT, check=True, capture_output=True, text=True, timeout=300)
    stats = tmp_path / f"ev_{tag}" / name / "statistics"
    return json.load(open(stats / "series_metrics.json")), dict(np.load(stats / "series_fields.npz")), samples, stats


def test_evaluate_mode_with_and_without_the_section(tmp_path, monkeypatch):
    met, fld, samples, stats_with = _evaluate(tmp_path, monkeypatch, "with", SECTION)
    met0, fld0, _, stats_without = _evaluate(tmp_path, monkeypatch, "without", None)
    assert sorted(os.listdir(stats_without)) == BASE_FILES
    assert sorted(os.listdir(stats_with)) == sorted(BASE_FILES + ["series_series_scores.npz"])
    assert set(met0) == BASE_METRICS and set(fld0) == BASE_FIELDS
    assert set(met) == BASE_METRICS | {"series_ensemble"} and set(fld) == BASE_FIELDS
    assert json.dumps({k: met[k] for k in met0}, sort_keys=True) == json.dumps(met0, sort_keys=True)
    for k in BASE_FIELDS:
        np.testing.assert_array_equal(fld[k], fld0[k], err_msg=k)
    gen = np.load(samples / "gen_samples_series_n_5.npz")["arr_0"]
    obs = np.load(samples / "eval_samples_series_n_5.npz")["arr_0"]
    lsm = (np.load(samples / "lsm_samples_series_n_5.npz")["arr_0"][:, 0] > 0.5).astype(np.uint8)      # 5 rows: a daily mask
    assert np.isnan(gen).any() and (lsm == 0).any()
    f = dict(np.load(stats_with / "series_series_scores.npz"))
    assert set(f) == set(V.SERIES_KEYS) | {"thresholds", "groups"}
    assert f["thresholds"].tolist() == SECTION["thresholds"] and f["groups"].tolist() == SECTION["groups"]
    r = device_call(gen, obs, SECTION["thresholds"], SECTION["groups"], lsm, seed=11)                  # seed: null = evaluation.seed
    assert_bit_equal(f, r, tag="evaluate mode")
    want = R.series_ensemble_scores(gen, obs, SECTION["thresholds"], SECTION["groups"], lsm, seed=11)
    assert_equal_to_reference(r, want, "evaluate mode")
    se = met["series_ensemble"]
    assert set(se) == {"M", "D", "thresholds", "climatology", "rank_seed", "n_groups", "pixels", "pooled", "groups", "crps_definitions",
                       "definition", "crpss"}
    assert (se["M"], se["D"], se["n_groups"], se["rank_seed"], se["thresholds"]) == (3, 5, 2, 11, SECTION["thresholds"])
    assert se["pixels"] == int((r["count"] > 0).sum()) > 0 and isinstance(se["definition"], str) and len(se["groups"]) == 2
    nan_eq = lambda a, b: np.testing.assert_allclose(np.asarray(a, np.float64), np.asarray(b, np.float64), rtol=1e-12, atol=0, equal_nan=True)  # noqa: E731
    for i, row in enumerate([se["pooled"]] + se["groups"]):
        assert set(row) == ROW_KEYS
        nan_eq([row[k] for k in V.ENSEMBLE_KEYS], r["scores"][i])
        assert row["count"] == int(r["rank_hist"][i].sum()) > 0
        h = r["rank_hist"][i].astype(np.float64)
        nan_eq(row["rank_reliability_index"], np.abs(h / h.sum() - 0.25).sum())
        nan_eq(row["outside_fraction"], (h[0] + h[3]) / h.sum())
        for j, k in enumerate(V.EXCEEDANCE_KEYS):
            nan_eq(row[k], r["exceedance"][i, j])
        nan_eq(row["brier_skill"], 1.0 - r["exceedance"][i, 0] / r["exceedance"][i, 3])
        nan_eq([row["climatology"][k] for k in V.SERIES_SKILL_KEYS], r["skill_scores"][i])
        nan_eq(row["crpss"], r["skill_scores"][i, 3])
    nan_eq(se["crpss"], r["skill_scores"][0, 3])
