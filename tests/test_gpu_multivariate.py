"""Energy scores (K53) and variogram scores (K54) of csrc/verify_multivariate.hip against the numpy float64 restatement in
tests/multivariate_ref.py, with bounds that come from the arithmetic and not from the kernels:

  dist2      rtol = count 2^-52.  Inputs are exact in fp64; either side sums `count` non-negative terms, each product rounded once
             (2^-53) and a sum of n non-negative terms in any order within (n - 1) 2^-53 of the exact one, so each side is
             within count 2^-53 and the two within count 2^-52.  The energy scalars: the same times 4.
  gamma_*    rtol = 2^-21: three fp32 roundings per non-negative term (difference, power, conversion), then fp64 sums.
  vs         within 2^-21 cond + 1e-12 |vs|, cond = sum w 2 |g_obs - g_ens| g_ens / sum w from the restatement.
  pairs, n_pairs, count: equal.

Also reproducibility, the invariances the scores must have, the limits, and `--mode evaluate` end to end with and without the
`evaluation.multivariate_scores` section."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multivariate_ref as R  # noqa: E402
from sbgm_danra_amd import verification as V  # noqa: E402
from sbgm_danra_amd._native import NativeError  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda")
U = 2.0 ** -52
# 5 x 7: smaller than the radius-8 disc; 33 x 65: crosses the 8 x 32 tile edges both ways; 32 x 48: aligned
SHAPES = [(5, 7), (33, 65), (32, 48)]
MEMBERS = [2, 3, 17, 64, 65]
MASKS = ("u8", "f32", "bool", None)


def _blur(z, width):
    """box blur of the last two axes, edges replicated"""
    if width == 1:
        return z
    pad = width // 2
    p = np.pad(z, [(0, 0)] * (z.ndim - 2) + [(pad, pad), (pad, pad)], mode="edge")
    out = np.zeros_like(z)
    for dy in range(width):
        for dx in range(width):
            out += p[..., dy:dy + z.shape[-2], dx:dx + z.shape[-1]]
    return out / (width * width)


@functools.lru_cache(maxsize=None)
def _case(M, shape_idx, kind, mask_kind):
    """(ens, obs, mask) as numpy: members from width-1 noise, the truth from width-3 box-blurred noise (another correlation
    length, so vs is no cancellation residue); about 1 % of the pixels get a NaN in one member; the mask drops about 15 %"""
    H, W = SHAPES[shape_idx]
    rng = np.random.default_rng([53, M, shape_idx, kind == "rain", MASKS.index(mask_kind)])
    z = rng.normal(size=(M, H, W))
    y = _blur(rng.normal(size=(H, W)), 3) * 3.0
    if kind == "rain":
        z, y = np.maximum(3 * z - 2, 0), np.maximum(3 * y - 2, 0)
    ens, obs = z.astype(np.float32), y.astype(np.float32)
    nan = rng.random((H, W)) < 0.01
    ens[rng.integers(0, M, size=(H, W))[nan], np.nonzero(nan)[0], np.nonzero(nan)[1]] = np.nan
    keep = rng.random((H, W)) < 0.85
    mask = {"u8": keep.astype(np.uint8) * 3, "f32": np.where(keep, 1.0, 0.25).astype(np.float32), "bool": keep, None: None}[mask_kind]
    for a in (ens, obs):
        a.setflags(write=False)
    return ens, obs, mask


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)          # a copy: the cached cases are read-only


@functools.lru_cache(maxsize=None)
def _energy_ref(M, shape_idx, kind, mask_kind):
    return R.energy_scores(*_case(M, shape_idx, kind, mask_kind))


def _check_energy(got, want, M):
    d2, s = got["dist2"].cpu().numpy(), got["scores"].cpu().numpy()
    count = int(want["scores"][0])
    assert s[0] == count
    err = np.abs(d2 - want["dist2"]) / np.maximum(want["dist2"], np.finfo(float).tiny)
    with np.errstate(invalid="ignore", divide="ignore"):
        serr = np.nanmax(np.abs(s[1:] / want["scores"][1:] - 1))
    print(f"energy M={M} count={count}: dist2 max rel err {err.max():.3e} (bound {count * U:.3e}); scores rel err {serr:.3e} "
          f"(bound {4 * count * U:.3e})")
    assert d2.shape == (M + 1, M + 1) and (np.diag(d2) == 0).all() and (d2 == d2.T).all()
    np.testing.assert_allclose(d2, want["dist2"], rtol=count * U, atol=0)
    np.testing.assert_allclose(s[1:], want["scores"][1:], rtol=4 * count * U, atol=0)


# ---- energy ------------------------------------------------------------------------------------------------------------------

CASES = [(M, si, kind, MASKS[(i + si + k) % 4]) for i, M in enumerate(MEMBERS) for si in range(3) for k, kind in enumerate(("normal", "rain"))]


@pytest.mark.parametrize("M,shape_idx,kind,mask_kind", CASES)
def test_energy_matches_restatement(M, shape_idx, kind, mask_kind):
    ens, obs, mask = _case(M, shape_idx, kind, mask_kind)
    _check_energy(V.energy_scores(_dev(ens), _dev(obs), mask=_dev(mask)), _energy_ref(M, shape_idx, kind, mask_kind), M)


def test_energy_many_members():
    """M = 1500: 94 x 94 tiles of 16 x 16 row pairs, the truth in the last one, one pixel segment per tile (the small cases
    above run 9 segments a tile).  The restatement of the whole matrix would take a minute on the host, so it is restated for
    26 rows — first and last tiles, tile edges, the truth — each against all 1501 columns; symmetry and the zero diagonal are
    checked on the whole matrix, and the scalars are restated from the device's own matrix, which checks the row and score
    kernels at this size."""
    H, W = SHAPES[1]
    rng = np.random.default_rng(1500)
    ens = rng.normal(size=(1500, H, W)).astype(np.float32)
    obs = rng.normal(size=(H, W)).astype(np.float32)
    ens[7, 3, 4] = np.nan
    r = V.energy_scores(_dev(ens), _dev(obs))
    d2, s = r["dist2"].cpu().numpy(), r["scores"].cpu().numpy()
    rows = sorted({0, 1, 7, 8, 9, 63, 64, 751, 752, 1495, 1496, 1497, 1498, 1499, 1500} | set(rng.integers(0, 1501, size=11).tolist()))
    want, count = R.energy_rows(ens, obs, rows=rows)
    assert count == H * W - 1 == s[0]
    assert (np.diag(d2) == 0).all() and (d2 == d2.T).all() and (d2[~np.eye(1501, dtype=bool)] > 0).all()
    print(f"energy M=1500: dist2 max rel err {np.abs(d2[rows] / np.where(want > 0, want, 1) - 1)[want > 0].max():.3e} (bound {count * U:.3e})")
    np.testing.assert_allclose(d2[rows], want, rtol=count * U, atol=0)
    np.testing.assert_allclose(s[1:], R.energy_scores_from_dist2(d2, count)[1:], rtol=4 * count * U, atol=0)


def test_duplicated_member_gives_an_exact_zero():
    ens, obs, mask = _case(17, 1, "normal", "u8")
    ens = ens.copy()
    ens[11] = ens[2]
    r = V.energy_scores(_dev(ens), _dev(obs), mask=_dev(mask))
    d2, s = r["dist2"].cpu().numpy(), r["scores"].cpu().numpy()
    assert d2[2, 11] == 0 and d2[11, 2] == 0 and s[5] == 0
    assert (d2[~np.eye(18, dtype=bool)] == 0).sum() == 2
    _check_energy(r, R.energy_scores(ens, obs, mask), 17)


# ---- variogram ---------------------------------------------------------------------------------------------------------------

def _check_variogram(got, want, tag):
    g = {k: v.cpu().numpy() for k, v in got.items()}
    s, ws = g["scores"], want["scores"]
    np.testing.assert_array_equal(g["offsets"], want["offsets"])
    np.testing.assert_array_equal(g["pairs"], want["pairs"])
    assert s[1] == ws[1] == want["pairs"].sum()
    has = want["pairs"] > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = max(np.nanmax(np.abs(g[k][has] / want[k][has] - 1), initial=0.0) for k in ("gamma_ens", "gamma_obs"))
    bound = 2.0 ** -21 * want["cond"] + 1e-12 * abs(ws[0])
    print(f"variogram {tag}: n_pairs={int(ws[1])} gamma max rel err {rel:.3e} (bound {2.0 ** -21:.3e}); |vs - ref| "
          f"{abs(s[0] - ws[0]):.3e} (bound {bound:.3e}, vs {ws[0]:.6e}, cond {want['cond']:.3e})")
    for k in ("gamma_ens", "gamma_obs"):
        assert np.isnan(g[k][~has]).all()
        np.testing.assert_allclose(g[k][has], want[k][has], rtol=2.0 ** -21, atol=0, err_msg=k)
    np.testing.assert_array_equal(np.isnan(g["vs_map"]), np.isnan(want["vs_map"]))
    if ws[1] == 0:
        assert np.isnan(s[0]) and np.isnan(s[3]) and s[2] == 0
        return
    assert abs(s[0] - ws[0]) <= bound
    np.testing.assert_allclose(s[2], ws[2], rtol=1e-12)
    # what the issue leaves open, by the same reasoning as its bound on vs: the unweighted score with the unweighted condition
    # number; the map, pixel by pixel, with the condition number of that pixel's own pairs (errors of both variograms) plus
    # the rounding of the fp64 sum to the fp32 map (2^-24) and of the fp64 sums themselves
    assert abs(s[3] - ws[3]) <= 2.0 ** -21 * want["cond_unweighted"] + 1e-12 * abs(ws[3])
    ok = ~np.isnan(want["vs_map"])
    assert (np.abs(g["vs_map"] - want["vs_map"])[ok] <= (2.0 ** -21 * want["map_cond"] + 2.0 ** -23 * want["vs_map"])[ok]).all()


VCASES = [(M, si, ("normal", "rain")[(i + j + si) % 2], MASKS[(i + si + j) % 4], radius, (0.5, 1.0, 2.0)[(i + j + si) % 3],
           V.VARIOGRAM_WEIGHTS[(i + si) % 2])
          for i, M in enumerate(MEMBERS) for si in range(3) for j, radius in enumerate((1, 3, 8))]


@pytest.mark.parametrize("M,shape_idx,kind,mask_kind,radius,order,weights", VCASES)
def test_variogram_matches_restatement(M, shape_idx, kind, mask_kind, radius, order, weights):
    ens, obs, mask = _case(M, shape_idx, kind, mask_kind)
    got = V.variogram_scores(_dev(ens), _dev(obs), radius=radius, order=order, weights=weights, mask=_dev(mask))
    want = R.variogram_scores(ens, obs, radius=radius, order=order, weights=weights, mask=mask)
    _check_variogram(got, want, f"M={M} {SHAPES[shape_idx]} {kind} r={radius} p={order} {weights}")


@pytest.mark.parametrize("order", [0.5, 1.0, 2.0])
@pytest.mark.parametrize("weights", V.VARIOGRAM_WEIGHTS)
def test_variogram_every_order_and_weighting_at_radius_8(order, weights):
    ens, obs, mask = _case(17, 1, "rain", "f32")
    got = V.variogram_scores(_dev(ens), _dev(obs), radius=8, order=order, weights=weights, mask=_dev(mask))
    _check_variogram(got, R.variogram_scores(ens, obs, radius=8, order=order, weights=weights, mask=mask), f"p={order} {weights}")


def test_variogram_many_members():
    H, W = SHAPES[1]
    rng = np.random.default_rng(1501)
    ens = rng.normal(size=(1500, H, W)).astype(np.float32)
    obs = (_blur(rng.normal(size=(H, W)), 3) * 3).astype(np.float32)
    got = V.variogram_scores(_dev(ens), _dev(obs), radius=4)
    _check_variogram(got, R.variogram_scores(ens, obs, radius=4), "M=1500")


# ---- invariances -------------------------------------------------------------------------------------------------------------

def _bits(r):
    return {k: v.cpu().numpy().tobytes() for k, v in r.items()}


def test_runs_are_bit_equal_and_counts_ignore_the_member_order():
    ens, obs, mask = _case(65, 1, "rain", "u8")
    e, o, m = _dev(ens), _dev(obs), _dev(mask)
    a, b = V.energy_scores(e, o, mask=m), V.energy_scores(e, o, mask=m)
    assert _bits(a) == _bits(b)
    va, vb = (V.variogram_scores(e, o, radius=8, mask=m) for _ in range(2))
    assert _bits(va) == _bits(vb)
    perm = torch.from_numpy(np.random.default_rng(6).permutation(65)).to(DEV)
    vp, ep = V.variogram_scores(e[perm], o, radius=8, mask=m), V.energy_scores(e[perm], o, mask=m)
    assert torch.equal(vp["pairs"], va["pairs"]) and vp["scores"][1] == va["scores"][1] and ep["scores"][0] == a["scores"][0]
    # the distance matrix is permuted with the members, entry by entry bit for bit: a pair's sum never depends on its tile
    idx = torch.cat([perm, torch.tensor([65], device=DEV)])
    assert torch.equal(ep["dist2"], a["dist2"][idx][:, idx])


def test_a_common_power_of_two_shift_leaves_the_variogram_unchanged():
    rng = np.random.default_rng(7)
    ens = (rng.integers(-40, 40, size=(17, 33, 65)) * 0.25).astype(np.float32)
    obs = (rng.integers(-40, 40, size=(33, 65)) * 0.25).astype(np.float32)
    mask = rng.random((33, 65)) < 0.9
    for order in (0.5, 1.0, 2.0):
        a = V.variogram_scores(_dev(ens), _dev(obs), radius=3, order=order, mask=_dev(mask))
        b = V.variogram_scores(_dev(ens + np.float32(256)), _dev(obs + np.float32(256)), radius=3, order=order, mask=_dev(mask))
        assert _bits(a) == _bits(b)
        assert a["scores"][0] > 0


def test_fully_masked_field():
    ens, obs, _ = _case(17, 2, "normal", None)
    for mask in (torch.zeros(32, 48, dtype=torch.uint8, device=DEV), torch.zeros(32, 48, device=DEV)):
        e = V.energy_scores(_dev(ens), _dev(obs), mask=mask)
        assert e["scores"][0] == 0 and torch.isnan(e["scores"][1:]).all() and (e["dist2"] == 0).all()
        v = V.variogram_scores(_dev(ens), _dev(obs), radius=3, mask=mask)
        assert (v["pairs"] == 0).all() and v["scores"][1] == 0 and v["scores"][2] == 0
        assert torch.isnan(v["scores"][[0, 3]]).all() and torch.isnan(v["vs_map"]).all() and torch.isnan(v["gamma_ens"]).all()
    nan_obs = torch.full((32, 48), float("nan"), device=DEV)
    assert V.energy_scores(_dev(ens), nan_obs)["scores"][0] == 0


def test_a_field_equals_itself_embedded_in_a_larger_masked_one():
    """dyadic data, 64 members, order 1, unit weights: every sum is exact, so the two runs agree bit for bit even though
    the embedded pixels fall into other tiles, lanes and segments"""
    rng = np.random.default_rng(8)
    H, W, y0, x0 = 19, 37, 9, 30
    ens = (rng.integers(-16, 16, size=(64, H, W)) * 0.25).astype(np.float32)
    obs = (rng.integers(-16, 16, size=(H, W)) * 0.25).astype(np.float32)
    big_e = rng.normal(size=(64, 40, 80)).astype(np.float32)
    big_o = rng.normal(size=(40, 80)).astype(np.float32)
    big_e[:, y0:y0 + H, x0:x0 + W], big_o[y0:y0 + H, x0:x0 + W] = ens, obs
    big_e[5, 0, 0] = np.nan
    mask = np.zeros((40, 80), np.uint8)
    mask[y0:y0 + H, x0:x0 + W] = 1
    a, b = V.energy_scores(_dev(ens), _dev(obs)), V.energy_scores(_dev(big_e), _dev(big_o), mask=_dev(mask))
    assert _bits(a) == _bits(b) and a["scores"][0] == H * W
    va = V.variogram_scores(_dev(ens), _dev(obs), radius=5, order=1.0, weights="unit")
    vb = V.variogram_scores(_dev(big_e), _dev(big_o), radius=5, order=1.0, weights="unit", mask=_dev(mask))
    for k in ("gamma_ens", "gamma_obs", "pairs", "scores", "offsets"):
        assert torch.equal(va[k], vb[k]), k
    assert torch.equal(va["vs_map"], vb["vs_map"][y0:y0 + H, x0:x0 + W])
    assert torch.isnan(vb["vs_map"]).sum() == 40 * 80 - H * W
    # and on arbitrary data with the square-root order, pixel by pixel: a pixel's own sum does not depend on where it lies
    ens2 = rng.normal(size=(17, H, W)).astype(np.float32)
    big_e2 = np.zeros((17, 40, 80), np.float32)
    big_e2[:, y0:y0 + H, x0:x0 + W] = ens2
    vc = V.variogram_scores(_dev(ens2), _dev(obs), radius=8)
    vd = V.variogram_scores(_dev(big_e2), _dev(big_o), radius=8, mask=_dev(mask))
    assert torch.equal(vc["vs_map"], vd["vs_map"][y0:y0 + H, x0:x0 + W]) and torch.equal(vc["pairs"], vd["pairs"])


# ---- limits ------------------------------------------------------------------------------------------------------------------

def test_limits_raise_before_any_launch():
    obs = torch.zeros(8, 9, device=DEV)
    ens = torch.zeros(3, 8, 9, device=DEV)
    for bad in (torch.zeros(1, 8, 9, device=DEV), torch.zeros(4096, 8, 9, device=DEV)):
        with pytest.raises(ValueError, match="members"):
            V.energy_scores(bad, obs)
        with pytest.raises(ValueError, match="members"):
            V.variogram_scores(bad, obs)
    for kw in (dict(radius=0), dict(radius=9), dict(order=0.7)):
        with pytest.raises(ValueError):
            V.variogram_scores(ens, obs, **kw)
    for fn in (V.energy_scores, V.variogram_scores):
        with pytest.raises(NativeError):
            fn(ens.cpu(), obs)
        with pytest.raises(NativeError):
            fn(ens, obs.cpu())
        with pytest.raises(NativeError):
            fn(ens, obs, mask=torch.ones(8, 9))


# ---- evaluate mode -----------------------------------------------------------------------------------------------------------

SECTION = {"energy": True, "variogram": {"radius": 3, "order": 0.5, "weights": "inverse_distance"}}


def _write_samples(samples):
    samples.mkdir(parents=True)
    rng = np.random.default_rng(26)
    for suffix, n, no in (("multi_n_3", 3, 3), ("repeated_n_4", 4, 1)):
        np.savez_compressed(samples / f"gen_samples_{suffix}.npz", rng.gamma(0.5, 2.0, size=(n, 1, 24, 40)).astype(np.float32))
        np.savez_compressed(samples / f"eval_samples_{suffix}.npz", rng.gamma(0.5, 2.0, size=(no, 1, 24, 40)).astype(np.float32))
        np.savez_compressed(samples / f"lsm_samples_{suffix}.npz", (rng.random((no, 1, 24, 40)) < 0.8).astype(np.float32))


def _evaluate(tmp_path, monkeypatch, tag, section):
    from sbgm_danra_amd.config_loader import load_config
    from sbgm_danra_amd.utils import get_model_string
    for k in ("DATA_DIR", "CKPT_DIR", "SAMPLE_DIR", "STATS_LOAD_DIR"):
        monkeypatch.setenv(k, str(tmp_path / k.lower()))
    monkeypatch.setenv("SLURM_CPUS_PER_TASK", "2")
    monkeypatch.setenv("PYTHONPATH", ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    raw = yaml.safe_load(open(os.path.join(ROOT, "sbgm_danra_amd", "config", "default_config.yaml")))
    assert "multivariate_scores" not in raw["evaluation"]
    raw["paths"]["evaluation_dir"] = str(tmp_path / f"ev_{tag}")
    raw["evaluation"].update(batch_size=3, n_repeats=4, eval_gen_type=["multiple", "repeated"], mask_stats=True,
                             eval_stat_methods=["pixel_stats", "spatial_stats"])
    if section is not None:
        raw["evaluation"]["multivariate_scores"] = section
    cfg_path = tmp_path / f"run_{tag}.yaml"
    cfg_path.write_text(yaml.safe_dump(raw))
    name = get_model_string(load_config(str(cfg_path)))
    samples = tmp_path / "sample_dir" / "generation" / name / "generated_samples"
    if not samples.exists():
        _write_samples(samples)
    subprocess.run([sys.executable, "-m", "sbgm_danra_amd.cli.main_app", "--config_path", str(cfg_path), "--mode", "evaluate"],
                   cwd=ROOT, check=True, capture_output=True, text=True, timeout=300)
    return tmp_path / f"ev_{tag}" / name / "statistics", samples


def test_evaluate_mode_with_and_without_the_section(tmp_path, monkeypatch):
    with_s, samples = _evaluate(tmp_path, monkeypatch, "with", SECTION)
    without, _ = _evaluate(tmp_path, monkeypatch, "without", None)
    # without the section: the files evaluate mode always wrote and no other; the section adds one file and one metrics entry
    assert sorted(p.name for p in without.iterdir()) == sorted(f"{label}_{kind}" for label in ("multiple", "repeated")
                                                               for kind in ("metrics.json", "fields.npz"))
    assert sorted(set(p.name for p in with_s.iterdir()) - set(p.name for p in without.iterdir())) == ["repeated_multivariate.npz"]
    # 'multiple' is skipped: its json is byte-equal (an npz carries the time it was written, so arrays are compared instead)
    assert (with_s / "multiple_metrics.json").read_bytes() == (without / "multiple_metrics.json").read_bytes()
    m1, m0 = np.load(with_s / "multiple_fields.npz"), np.load(without / "multiple_fields.npz")
    assert m1.files == m0.files and all(m1[k].dtype == m0[k].dtype and m1[k].tobytes() == m0[k].tobytes() for k in m0.files)
    f1, f0 = np.load(with_s / "repeated_fields.npz"), np.load(without / "repeated_fields.npz")
    assert f1.files == f0.files
    for k in f0.files:
        assert f1[k].dtype == f0[k].dtype and f1[k].tobytes() == f0[k].tobytes(), k
    met, met0 = json.load(open(with_s / "repeated_metrics.json")), json.load(open(without / "repeated_metrics.json"))
    assert set(met) == set(met0) | {"multivariate"}
    assert json.dumps({k: met[k] for k in met0}, sort_keys=True) == json.dumps(met0, sort_keys=True)
    # with it: the values of a direct call on the same files
    g = torch.from_numpy(np.load(samples / "gen_samples_repeated_n_4.npz")["arr_0"][:, 0]).to(DEV)
    o = torch.from_numpy(np.load(samples / "eval_samples_repeated_n_4.npz")["arr_0"][0, 0]).to(DEV)
    m = torch.from_numpy(np.load(samples / "lsm_samples_repeated_n_4.npz")["arr_0"][0, 0] > 0.5).to(DEV)
    e, v = V.energy_scores(g, o, mask=m), V.variogram_scores(g, o, mask=m, **SECTION["variogram"])
    npz = np.load(with_s / "repeated_multivariate.npz")
    assert sorted(npz.files) == sorted(["energy_dist2"] + [f"variogram_{k}" for k in ("vs_map", "gamma_ens", "gamma_obs", "offsets", "pairs")])
    np.testing.assert_array_equal(npz["energy_dist2"], e["dist2"].cpu().numpy())
    for k in ("vs_map", "gamma_ens", "gamma_obs", "offsets", "pairs"):
        np.testing.assert_array_equal(npz[f"variogram_{k}"], v[k].cpu().numpy(), err_msg=k)
    mv = met["multivariate"]
    assert mv["M"] == 4 and [mv["energy"][k] for k in V.ENERGY_KEYS] == e["scores"].tolist()
    assert [mv["variogram"][k] for k in V.VARIOGRAM_KEYS] == v["scores"].tolist()
    assert {k: mv["variogram"][k] for k in SECTION["variogram"]} == SECTION["variogram"]
    assert mv["energy"]["es_fair"] > 0 and mv["variogram"]["n_pairs"] > 0
