"""Host side of the device-resident cutout batches: the restatement the GPU tests compare against (tests/cutout_ref.py) checked against
scipy and against itself, the validation errors of ResidentFields and of the configuration, and the C ABI plumbing."""
import os
import re
import sys

import numpy as np
import pytest
import yaml

sys.path.insert(0, os.path.dirname(__file__))
import cutout_ref as R  # noqa: E402

from sbgm_danra_amd import _native as N  # noqa: E402
from sbgm_danra_amd import resident_data as RD  # noqa: E402
from sbgm_danra_amd.config_loader import to_config  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = ("sbgm_cutout_draw", "sbgm_cutout_gather", "sbgm_sdf_from_mask")


@pytest.mark.parametrize("shape", [(1, 7), (5, 1), (9, 13), (33, 20), (17, 40)])
@pytest.mark.parametrize("land", [0.02, 0.5, 0.97])
def test_separable_integer_transform_equals_scipy(shape, land):
    rng = np.random.default_rng(1000 * shape[0] + shape[1] + int(100 * land))
    mask = (rng.random(shape) < land).astype(np.float32)
    if not mask.any():
        mask[rng.integers(shape[0]), rng.integers(shape[1])] = 1.0
    want = R.edt_squared_scipy(mask)
    assert np.array_equal(R.edt_squared_separable(mask), want)
    # the reference hands scipy a [1, h, w] tensor: same distances as the 2-D call
    from scipy.ndimage import distance_transform_edt
    assert np.array_equal(distance_transform_edt(~(mask[None] > 0))[0], distance_transform_edt(~(mask > 0)))


def test_no_coastline_rules_and_normalisation():
    assert np.array_equal(R.sdf_ref(np.ones((4, 5))), np.ones((4, 5)))
    assert np.array_equal(R.sdf_ref(np.zeros((4, 5))), np.zeros((4, 5)))
    assert np.array_equal(R.edt_squared_separable(np.zeros((3, 3))), np.full((3, 3), -1))
    m = np.zeros((6, 9), dtype=np.float32)
    m[0, 0] = 1.0
    s = R.sdf_ref(m)
    assert s[0, 0] == 1.0 and s[5, 8] == 0.0 and s.min() == 0.0 and s.max() == 1.0
    with np.errstate(invalid="ignore"):
        assert np.isnan(R.normalize_sdf(R.generate_sdf(np.ones((3, 3))))).all()      # what the reference gives on an all-land crop


def test_draw_reaches_both_ends_and_stays_inside():
    lo, hi = np.float32(2.0 ** -25), np.float32(1.0)
    for max_off in (0, 1, 52, 461, 4095):
        assert R.offset_from_uniform(np.array([lo]), max_off)[0] == 0
        assert R.offset_from_uniform(np.array([hi]), max_off)[0] == max_off          # u = 1 would give max_off + 1 without the clamp
    rect, crop = [170, 350, 340, 520], (128, 19)
    o = R.draw_origins(7, 3, 4096, rect, crop)
    assert o.dtype == np.int32 and o.shape == (4096, 2)
    assert o[:, 0].min() >= 170 and o[:, 0].max() <= 350 - 128 and o[:, 1].min() >= 340 and o[:, 1].max() <= 520 - 19
    assert len(np.unique(o[:, 0])) == 350 - 128 - 170 + 1                           # every offset occurs in 4096 draws of 53 values
    assert np.array_equal(R.draw_origins(7, 3, 64, [5, 37, 9, 29], (32, 20)), np.tile(np.array([[5, 9]], dtype=np.int32), (64, 1)))
    assert not np.array_equal(R.draw_origins(7, 4, 4096, rect, crop), o)
    with pytest.raises(ValueError):
        R.draw_origins(7, 3, 4, rect, (181, 19))


def test_draw_numbers_agree_and_separate_the_splits():
    seen = set()
    for split in ("train", "valid", "gen"):
        for epoch in (0, 1, 2 ** 24 - 1):
            for batch in (0, 5, 2 ** 24 - 1):
                for rank in (0, 3):
                    d = RD.draw_number(split, epoch, batch, rank)
                    assert d == R.draw_number(split, epoch, batch, rank) and 0 <= d < 2 ** 64
                    seen.add(d)
    assert len(seen) == 3 * 3 * 2 + 2 * 3 * 2          # training separates its epochs; validation and generation do not
    with pytest.raises(ValueError):
        RD.draw_number("train", 2 ** 24, 0)


def _arrays(N_=3, Hd=12, Wd=14):
    rng = np.random.default_rng(0)
    return {"prcp_hr": rng.random((N_, Hd, Wd), dtype=np.float32), "temp_lr": rng.random((N_, Hd, Wd), dtype=np.float32),
            "lsm": (rng.random((Hd, Wd)) > 0.5).astype(np.float32), "topo": rng.random((Hd, Wd), dtype=np.float32),
            "classifier": np.arange(N_, dtype=np.int64) % 4 + 1}


@pytest.mark.parametrize("change,needle", [
    (lambda a: a.pop("prcp_hr"), "'prcp_hr' is missing"),
    (lambda a: a.pop("temp_lr"), "'temp_lr' is missing"),
    (lambda a: a.update(temp_lr=a["temp_lr"][:, :-1]), "'temp_lr' has shape"),
    (lambda a: a.update(prcp_hr=a["prcp_hr"][0]), "'prcp_hr' has shape"),
    (lambda a: a.update(prcp_hr=a["prcp_hr"].astype(np.int32)), "'prcp_hr' has dtype int32"),
    (lambda a: a.update(lsm=a["lsm"][:-1]), "'lsm' has shape"),
    (lambda a: a.pop("topo"), "'topo' is missing"),
    (lambda a: a.update(classifier=a["classifier"].astype(np.float32)), "'classifier' has shape"),
    (lambda a: a.update(classifier=a["classifier"][:-1]), "'classifier' has shape"),
])
def test_resident_fields_rejects_bad_files_before_any_upload(tmp_path, change, needle):
    a = _arrays()
    change(a)
    path = str(tmp_path / "fields.npz")
    np.savez(path, **a)
    # device="cpu" is itself refused, but only after validation: a bad file never reaches the upload
    with pytest.raises(ValueError, match=re.escape(needle)):
        RD.ResidentFields(path, "prcp", ["temp"], device="cpu", need=["lsm", "topo", "classifier"])


def test_resident_fields_has_no_host_path(tmp_path):
    path = str(tmp_path / "fields.npz")
    np.savez(path, **_arrays())
    with pytest.raises(N.NativeError, match="ROCm device"):
        RD.ResidentFields(path, "prcp", ["temp"], device="cpu")


def _cfg(**over):
    raw = yaml.safe_load(open(os.path.join(ROOT, "sbgm_danra_amd", "config", "default_config.yaml")))
    raw["highres"].update(data_size=[32, 32], cutout_domains=[2, 38, 4, 52])
    raw["lowres"].update(data_size=[32, 32], cutout_domains=[2, 38, 4, 52])
    raw["transforms"]["sample_w_cutouts"] = True
    for path, v in over.items():
        sec, key = path.split(".")
        raw[sec][key] = v
    return to_config(raw)


@pytest.mark.parametrize("over,needle", [
    ({"lowres.data_size": [16, 16]}, "lowres.data_size"),
    ({"lowres.cutout_domains": [0, 40, 0, 56]}, "lowres.cutout_domains"),
    ({"lowres.resize_factor": 2}, "resize_factor"),
    ({"highres.cutout_domains": [2, 41, 4, 52], "lowres.cutout_domains": [2, 41, 4, 52]}, "outside the 40x56 domain"),
    ({"highres.data_size": [37, 32], "lowres.data_size": [37, 32]}, "larger than the rectangle"),
])
def test_unsupported_configurations_say_so(over, needle):
    with pytest.raises(ValueError, match=re.escape(needle)):
        RD.cutout_geometry(_cfg(**over), 40, 56)


def test_geometry_with_and_without_cutouts():
    assert RD.cutout_geometry(_cfg(), 40, 56) == ([2, 38, 4, 52], (32, 32))
    c = _cfg(**{"highres.data_size": [36, 48], "lowres.data_size": [36, 48]})
    c.transforms.sample_w_cutouts = False
    assert RD.cutout_geometry(c, 40, 56) == ([2, 38, 4, 52], (36, 48))                 # the whole rectangle
    c = _cfg(**{"highres.data_size": [40, 56], "lowres.data_size": None, "highres.cutout_domains": None, "lowres.cutout_domains": None})
    c.transforms.sample_w_cutouts = False
    assert RD.cutout_geometry(c, 40, 56) == ([0, 40, 0, 56], (40, 56))                 # the whole domain
    c = _cfg()
    c.transforms.sample_w_cutouts = False
    with pytest.raises(ValueError, match="does not resize"):
        RD.cutout_geometry(c, 40, 56)


def test_per_element_statistics_are_refused():
    class F:
        hr_key, lr_keys, planes = "prcp_hr", [], {}
    c = _cfg(**{"lowres.condition_variables": []})
    c.highres.scaling_method = "zscore"
    with pytest.raises(ValueError, match="per-element"):
        RD.build_transforms(c, F, stats={"prcp_hr": {"mean": np.zeros((32, 32)), "std": 1.0}})
    tr = RD.build_transforms(c, F, stats={"prcp_hr": {"mean": 1.5, "std": 2.0}})
    assert [op for op, _ in tr["prcp_hr"].program()] == [0, 2]                         # ADD, DIV


def test_symbols_header_and_binding_agree():
    header = open(os.path.join(ROOT, "include", "sbgm_hip.h")).read()
    n_args = lambda name: len(re.search(name + r"\s*\(([^;]*)\);", header).group(1).split(","))  # noqa: E731
    for name, n in (("sbgm_cutout_draw", 10), ("sbgm_cutout_program_init", 5), ("sbgm_cutout_gather", 13), ("sbgm_sdf_workspace_bytes", 3),
                    ("sbgm_sdf_from_mask", 8)):
        assert re.search(r"\b(int|int64_t)\s+" + name + r"\s*\(", header), name
        assert name in N.SIGNATURES and n_args(name) == len(N.SIGNATURES[name][1]) == n, name
        assert hasattr(N.lib(), name)
    assert all(hasattr(N.lib(), name) for name in OPS)
    assert N.lib().sbgm_abi_version() == N.ABI_VERSION >= 7
    assert re.search(r"#define SBGM_CUTOUT_MAX_FIELDS \(1 \+ SBGM_ASSEMBLE_MAX_LR \+ 2\)", header) and N.CUTOUT_MAX_FIELDS == 1 + 16 + 2
    assert re.search(r"#define SBGM_CUTOUT_PROGRAM_WORDS \(2 \+ 2 \* SBGM_CHAIN_MAX_OPS\)", header) and N.CUTOUT_PROGRAM_WORDS == 2 + 2 * 12
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(name in doc for name in OPS) and "resident_fields" in doc


def test_host_side_validation_of_the_ops():
    """argument errors are raised on the host before any launch, so they need no device"""
    import ctypes as C
    lib = N.lib()
    rect = (C.c_int * 4)(170, 350, 340, 520)
    assert lib.sbgm_cutout_draw(1, 0, 4, rect, 181, 128, 589, 789, None, None) != 0
    assert lib.sbgm_cutout_draw(1, 0, 4, rect, 181, 128, 589, 789, 16, None) != 0 and b"larger than the rectangle" in lib.sbgm_last_error()
    assert lib.sbgm_cutout_draw(1, 0, 4, rect, 128, 128, 589, 500, 16, None) != 0 and b"outside" in lib.sbgm_last_error()
    assert lib.sbgm_sdf_workspace_bytes(2, 4097, 8) == -1 and lib.sbgm_sdf_workspace_bytes(2, 8, 4097) == -1
    assert lib.sbgm_sdf_workspace_bytes(3, 5, 7) == 32 + 3 * 5 * 7 * 4
    p = (C.c_int32 * N.CUTOUT_PROGRAM_WORDS)(*([-1] * N.CUTOUT_PROGRAM_WORDS))
    ops, cs = (C.c_int * 2)(0, 99), (C.c_float * 2)(1.0, 2.0)
    assert lib.sbgm_cutout_program_init(p, 2, ops, cs, 0) != 0 and b"unknown op code 99" in lib.sbgm_last_error()
    assert lib.sbgm_cutout_program_init(p, 13, ops, cs, 0) != 0 and list(p) == [-1] * N.CUTOUT_PROGRAM_WORDS
    ops[1] = 2
    assert lib.sbgm_cutout_program_init(p, 2, ops, cs, 5) == 0
    words = np.frombuffer(bytes(p), dtype=np.int32)
    assert words[:4].tolist() == [2, 1, 0, 2] and words[4:14].tolist() == [0] * 10           # n_ops, is_mask, ops
    assert words[14:].view(np.float32).tolist() == [1.0, 2.0] + [0.0] * 10                  # consts
    srcs, dsts, counts = (C.c_void_p * 1)(16), (C.c_void_p * 1)(16), (C.c_int * 1)(0)
    assert lib.sbgm_cutout_gather(srcs, dsts, counts, 20, 16, 16, 16, 1, 8, 8, 4, 4, None) != 0 and b"fields" in lib.sbgm_last_error()
    assert lib.sbgm_cutout_gather(srcs, dsts, counts, 1, 16, 16, 16, 1, 8, 8, 9, 4, None) != 0 and b"crop" in lib.sbgm_last_error()
