"""Host side of full-domain series generation: the restatement the GPU tests compare against (tests/domain_loader_ref.py) checked against
numpy's edge pad of the transformed field, the parsing and the refusals of evaluation.full_domain, the sections it must leave alone, and
the C ABI plumbing of sbgm_domain_gather.  Every comparison is exact."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import yaml

sys.path.insert(0, os.path.dirname(__file__))
import cutout_ref as R  # noqa: E402
import domain_loader_ref as DR  # noqa: E402

from oracle import transforms_ref as TR  # noqa: E402
from sbgm_danra_amd import _native as N  # noqa: E402
from sbgm_danra_amd import resident_data as RD  # noqa: E402
from sbgm_danra_amd.config_loader import to_config  # noqa: E402
from sbgm_danra_amd.evaluate_sbgm import generation as G  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULTS = os.path.join(ROOT, "sbgm_danra_amd", "config", "default_config.yaml")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the reference gather ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5, 7, 8), (6, 8, 8), (5, 9, 12), (4, 5, 12)])
def test_reference_gather_is_the_edge_pad_of_the_transformed_field(shape):
    Hd, Wd, Wp = shape
    rng = np.random.default_rng(Hd * 100 + Wd)
    stack = rng.normal(3, 5, (4, Hd, Wd)).astype(np.float32)
    plane = rng.random((Hd, Wd), dtype=np.float32)
    items = [2, 0, 2]
    z = TR.ZScoreTransform(1.25, 3.5)
    full = lambda a, tr=None, m=False: R.crop_transform(a, items, [(0, 0)] * 3, (Hd, Wd), tr, m)  # noqa: E731
    pad = lambda a: np.pad(a, ((0, 0), (0, 0), (0, 0), (0, Wp - Wd)), mode="edge")  # noqa: E731
    for got, want in ((DR.domain_gather(stack, items, Wp, z), pad(full(stack, z))), (DR.domain_gather(stack, items, Wp), pad(full(stack))),
                      (DR.domain_gather(plane, items, Wp, None, True), pad(full(plane, None, True)))):
        assert got.shape == (3, 1, Hd, Wp) and got.dtype == np.float32
        assert np.array_equal(bits(got), bits(want))
    got = DR.domain_gather(stack, [1, 4, -1], Wp, z)
    want = pad(R.crop_transform(stack, [1], [(0, 0)], (Hd, Wd), z))
    assert np.isnan(got[1:]).all() and np.array_equal(bits(got[0]), bits(want[0]))            # an item outside the stack: NaN, alone
    assert not np.isnan(DR.domain_gather(plane, [9], Wp)).any()                     # a plane has no item to get wrong
    with pytest.raises(ValueError):
        DR.domain_gather(stack, items, Wd - 1)


def test_reference_batch_has_the_loaders_keys():
    rng = np.random.default_rng(0)
    arrays = {"prcp_hr": rng.random((3, 5, 9), dtype=np.float32), "temp_lr": rng.random((3, 5, 9), dtype=np.float32),
              "lsm": rng.random((5, 9), dtype=np.float32), "topo": rng.random((5, 9), dtype=np.float32), "classifier": np.arange(3) + 1}
    b = DR.batch_ref(arrays, "prcp_hr", ["temp_lr"], [1, 2], 12, with_classes=True)
    assert set(b) == {"prcp_hr", "temp_lr", "lsm", "lsm_hr", "topo", "classifier", "hr_points", "lr_points", "domain_hw"}
    assert b["prcp_hr"].shape == (2, 1, 5, 12) and b["domain_hw"] == (5, 9) and b["hr_points"].tolist() == [[0, 5, 0, 9]] * 2
    assert set(np.unique(b["lsm"])) <= {0.0, 1.0} and b["classifier"].tolist() == [2, 3]
    assert np.array_equal(b["topo"][:, :, :, 9:], np.repeat(b["topo"][:, :, :, 8:9], 3, axis=3))


# ---- the section ---------------------------------------------------------------------------------------------------------------------
def _cfg(full_domain="absent", gen_type=("series",), resident=True, **over):
    raw = yaml.safe_load(open(DEFAULTS))
    raw["highres"]["data_size"] = [32, 32]
    raw["lowres"]["data_size"] = [32, 32]
    raw["evaluation"]["gen_type"] = list(gen_type)
    if full_domain != "absent":
        raw["evaluation"]["full_domain"] = full_domain
    if resident:
        raw.setdefault("data_handling", {})["resident_fields"] = {"gen": "/nonexistent/gen.npz"}
    for path, v in over.items():
        sec, key = path.split(".")
        raw[sec][key] = v
    return to_config(raw)


def test_shipped_defaults_do_not_opt_in():
    raw = yaml.safe_load(open(DEFAULTS))
    assert "full_domain" not in raw["evaluation"]
    assert RD.full_domain_config(to_config(raw)) is None and G.full_domain_config is RD.full_domain_config
    assert RD.full_domain_config(_cfg()) is None


def test_section_parses_with_its_defaults():
    got = RD.full_domain_config(_cfg({"halo": 4}))
    assert got == {"tile": 32, "halo": 4, "joint": False, "tiles_per_batch": None, "first_day": 0}     # tile: highres.data_size[0]
    got = RD.full_domain_config(_cfg({"tile": 64, "halo": 16, "joint": True, "tiles_per_batch": 2, "first_day": 3}))
    assert got == {"tile": 64, "halo": 16, "joint": True, "tiles_per_batch": 2, "first_day": 3}
    got = RD.full_domain_config(_cfg({"tile": None, "halo": 4, "tiles_per_batch": None}), domain_hw=(44, 53))
    assert got["tile"] == 32
    assert RD.full_domain_config(_cfg({"tile": 256}))["halo"] == 32                                       # the documented default halo


@pytest.mark.parametrize("section,needle", [
    ({"halo": 4, "tiles": 2}, "takes the keys"),
    ([32, 4], "takes the keys"),
    ({"halo": 16}, "evaluation.full_domain.halo"),                    # 2 * halo = tile: axis_origins' "overlap must be in [0, tile)"
    ({"halo": -1}, "evaluation.full_domain.halo"),
    ({"halo": 4.0}, "evaluation.full_domain.halo"),
    ({"tile": 0, "halo": 0}, "evaluation.full_domain.tile"),
    ({"tile": True, "halo": 0}, "evaluation.full_domain.tile"),
    ({"halo": 4, "joint": 1}, "evaluation.full_domain.joint"),
    ({"halo": 4, "tiles_per_batch": 0}, "evaluation.full_domain.tiles_per_batch"),
    ({"halo": 4, "first_day": -1}, "evaluation.full_domain.first_day"),
    ({"halo": 4, "first_day": 1.5}, "evaluation.full_domain.first_day"),
])
def test_malformed_sections_are_refused_by_key(section, needle):
    with pytest.raises(ValueError, match=re.escape(needle)):
        RD.full_domain_config(_cfg(section))


def test_geometry_the_tile_table_refuses():
    from sbgm_danra_amd.tiling import axis_origins, padded_width
    assert padded_width(53, 32) == 56 and padded_width(789, 256) == 792 and padded_width(56, 32) == 56
    with pytest.raises(ValueError, match="larger than the domain"):
        axis_origins(30, 32, 8)
    with pytest.raises(ValueError, match=re.escape("evaluation.full_domain: tile 32, halo 4 on the 30x53 domain")):
        RD.full_domain_config(_cfg({"halo": 4}), domain_hw=(30, 53))
    with pytest.raises(ValueError, match="evaluation.full_domain: tile 32"):
        RD.full_domain_config(_cfg({"halo": 4}), domain_hw=(44, 20))
    assert RD.full_domain_config(_cfg({"halo": 4}), domain_hw=(32, 32))["tile"] == 32                    # one tile


def test_what_a_domain_series_does_not_do_is_refused_at_start(tmp_path, monkeypatch):
    with pytest.raises(ValueError, match="rk45_sampler"):
        RD.full_domain_config(_cfg({"halo": 4}, **{"sampler.sampler_type": "rk45_sampler"}))
    for kinds in (["series", "multiple"], ["multiple"], []):
        with pytest.raises(ValueError, match=re.escape("evaluation.gen_type")):
            RD.full_domain_config(_cfg({"halo": 4}, gen_type=kinds))
    with pytest.raises(ValueError, match=re.escape("data_handling.resident_fields.gen")):
        RD.full_domain_config(_cfg({"halo": 4}, resident=False))
    c = _cfg({"halo": 4})
    c.data_handling.resident_fields = {"train": "/nonexistent/train.npz"}
    with pytest.raises(ValueError, match=re.escape("data_handling.resident_fields.gen")):
        RD.full_domain_config(c)
    # the generator and the loader factory refuse the same things before a model or a file is touched
    from sbgm_danra_amd import parallel
    from sbgm_danra_amd.training_utils import get_gen_dataloader
    with pytest.raises(ValueError, match=re.escape("data_handling.resident_fields.gen")):
        get_gen_dataloader(_cfg({"halo": 4}, resident=False))
    with pytest.raises(ValueError, match="one rank"):
        RD.resident_domain_loader(_cfg({"halo": 4}), shard=(1, 2))
    from sbgm_danra_amd.evaluate_sbgm.generation_main import generation_main
    for k in ("DATA_DIR", "CKPT_DIR", "STATS_LOAD_DIR", "SAMPLE_DIR"):
        monkeypatch.setenv(k, str(tmp_path / k.lower()))
    bad = _cfg({"halo": 4}, **{"sampler.sampler_type": "rk45_sampler"})
    bad.paths.sample_dir = str(tmp_path / "samples")
    with pytest.raises(ValueError, match="evaluation.full_domain"):
        generation_main(bad)
    ok = _cfg({"halo": 4})
    ok.paths.sample_dir = str(tmp_path / "samples")
    monkeypatch.setattr(parallel, "world", lambda: (0, 2))
    with pytest.raises(ValueError, match="evaluation.full_domain runs on one rank"):
        generation_main(ok)


def test_series_sections_are_unchanged():
    for fd in ("absent", {"halo": 4}):
        c = _cfg(fd)
        assert G.series_config(c) == (1, None) and G.series_noise_config(c) == (None, None)
        c = _cfg(fd, **{"evaluation.series": {"members": 3, "max_days": 5, "seed": 7, "temporal_noise": {"rho": 0.6, "lags": 3}}})
        assert G.series_config(c) == (3, 5)
        seed, w = G.series_noise_config(c)
        from sbgm_danra_amd.score_sampling import temporal_noise_weights
        assert seed == 7 and np.array_equal(w, temporal_noise_weights(0.6, 3))
        with pytest.raises(ValueError, match="evaluation.series takes the keys"):
            G.series_config(_cfg(fd, **{"evaluation.series": {"members": 1, "first_day": 2}}))
    from sbgm_danra_amd.evaluate_sbgm import evaluation as E
    assert E.GEN_TYPES == ("multiple", "single", "repeated", "series") and E.TIME_AXIS_TYPES == ("multiple", "series")


def test_constraint_mask_takes_the_domain_shape():
    c = _cfg({"halo": 4})
    c.constraint = to_config({"enabled": True, "station_fraction": 0.2, "seed": 3})
    m = G.constraint_mask(c, (44, 53))
    assert m.shape == (44, 53) and m.dtype == np.float32 and 0 < m.mean() < 0.5


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------------
def test_symbol_header_and_binding_agree():
    header = open(os.path.join(ROOT, "include", "sbgm_hip.h")).read()
    args = re.search(r"\bint\s+sbgm_domain_gather\s*\(([^;]*)\);", header).group(1).split(",")
    assert "sbgm_domain_gather" in N.SIGNATURES and len(args) == len(N.SIGNATURES["sbgm_domain_gather"][1]) == 11
    lib = N.lib()
    assert hasattr(lib, "sbgm_domain_gather") and lib.sbgm_abi_version() == N.ABI_VERSION >= 18
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "sbgm_domain_gather" in doc and "full_domain" in doc


def test_host_side_validation_of_the_op():
    """argument errors are raised on the host before any launch, so they need no device"""
    lib = N.lib()
    srcs, dsts, counts = (C.c_void_p * 1)(16), (C.c_void_p * 1)(16), (C.c_int * 1)(0)
    call = lambda nf, B, Hd, Wd, Wp: lib.sbgm_domain_gather(srcs, dsts, counts, nf, 16, 16, B, Hd, Wd, Wp, None)  # noqa: E731
    assert call(20, 1, 8, 8, 8) != 0 and b"fields" in lib.sbgm_last_error()
    assert call(1, 0, 8, 8, 8) != 0 and b"domain" in lib.sbgm_last_error()
    assert call(1, 1, 0, 8, 8) != 0 and call(1, 1, 8, 0, 8) != 0
    assert call(1, 1, 8, 9, 8) != 0 and b"padded width" in lib.sbgm_last_error()           # Wp < Wd
    assert call(1, 1, 8, 7, 10) != 0 and b"padded width" in lib.sbgm_last_error()          # Wp % 4
    dsts[0] = 20
    assert call(1, 1, 8, 7, 8) != 0 and b"16-byte aligned" in lib.sbgm_last_error()
    counts[0] = -1
    assert call(1, 1, 8, 7, 8) != 0 and b"negative item count" in lib.sbgm_last_error()
