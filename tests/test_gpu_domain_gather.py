"""`sbgm_domain_gather` on the GPU (csrc/cutout.hip), bit for bit against the numpy restatement of tests/domain_loader_ref.py and against
`sbgm_cutout_gather` at full extent followed by a replicate pad, and `ResidentDomainLoader` against the restated batch.

Every program here is affine (separately rounded fp32 adds, multiplies and divides), the mask is a comparison and the pad a copy: every
comparison is exact.  Shapes (Hd, Wd, Wp): (5, 7, 8) one pad column, (6, 8, 8) no pad, (5, 9, 12) a row that ends inside a quad and
(4, 5, 12) a pad wider than a quad (a whole quad of clamped columns)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import yaml

sys.path.insert(0, os.path.dirname(__file__))
import domain_loader_ref as DR  # noqa: E402

from oracle import transforms_ref as TR  # noqa: E402
from sbgm_danra_amd import _native as N  # noqa: E402
from sbgm_danra_amd import resident_data as RD  # noqa: E402
from sbgm_danra_amd.config_loader import to_config  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(5, 7, 8), (6, 8, 8), (5, 9, 12), (4, 5, 12)]
ADD, MUL, DIV = 0, 1, 2
PROGRAM3 = [(ADD, -2.75), (MUL, 1.7), (DIV, 3.3)]                     # three steps, each rounded to fp32 on its own
N_ITEMS = 4


def program3(t):
    """PROGRAM3 on a float32 CPU tensor: one rounding per step, as the device chain does"""
    return ((t + np.float32(-2.75)) * np.float32(1.7)) / np.float32(3.3)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def host_fields(Hd, Wd):
    rng = np.random.default_rng(Hd * 1000 + Wd)
    lsm = rng.random((Hd, Wd), dtype=np.float32)                        # not binary: the binarisation has something to do
    lsm[0, 0], lsm[Hd - 1, Wd - 1] = 0.5, np.nextafter(np.float32(0.5), np.float32(1))
    return {"a": rng.normal(2, 9, (N_ITEMS, Hd, Wd)).astype(np.float32), "b": rng.normal(0, 1, (N_ITEMS, Hd, Wd)).astype(np.float32),
            "plane": (rng.random((Hd, Wd), dtype=np.float32) * 900 - 5).astype(np.float32), "lsm": lsm}


def device_fields(host):
    """[(key, device tensor, n_items, is_mask, program, reference transform)]; stack `a` starts 4 bytes into its allocation, so its
    rows have every alignment but the allocation's"""
    n, Hd, Wd = host["a"].shape
    big = torch.empty(n * Hd * Wd + 1, device="cuda")
    a = big[1:].view(n, Hd, Wd)
    a.copy_(torch.from_numpy(host["a"]))
    assert a.data_ptr() % 16 == 4
    up = lambda k: torch.from_numpy(host[k]).cuda()  # noqa: E731
    return [("a", a, n, 0, PROGRAM3, program3), ("b", up("b"), n, 0, [], None), ("plane", up("plane"), 0, 0, [], None),
            ("lsm", up("lsm"), 0, 1, [], None)], big


def run_domain_gather(fields, items, Hd, Wd, Wp):
    """one launch -> list of [B, 1, Hd, Wp] cpu tensors"""
    B, nf = len(items), len(fields)
    programs = RD.upload_programs([(m, p) for _k, _s, _n, m, p, _t in fields], "cuda")
    srcs, dsts, counts, outs = (N._vp * nf)(), (N._vp * nf)(), (C.c_int * nf)(), []
    for i, (_k, src, n, _m, _p, _t) in enumerate(fields):
        outs.append(torch.full((B, 1, Hd, Wp), 123.0, device="cuda"))
        srcs[i], dsts[i], counts[i] = src.data_ptr(), outs[-1].data_ptr(), n
    it = torch.tensor(items, dtype=torch.int32, device="cuda")
    N.check(N.lib().sbgm_domain_gather(srcs, dsts, counts, nf, programs.data_ptr(), it.data_ptr(), B, Hd, Wd, Wp, N.stream()))
    return [o.cpu() for o in outs]


def run_cutout_gather_and_pad(fields, items, Hd, Wd, Wp):
    """sbgm_cutout_gather at full extent (crop = the domain, origin 0), then F.pad(replicate)"""
    B, nf = len(items), len(fields)
    programs = RD.upload_programs([(m, p) for _k, _s, _n, m, p, _t in fields], "cuda")
    srcs, dsts, counts, outs = (N._vp * nf)(), (N._vp * nf)(), (C.c_int * nf)(), []
    for i, (_k, src, n, _m, _p, _t) in enumerate(fields):
        outs.append(torch.full((B, 1, Hd, Wd), 123.0, device="cuda"))
        srcs[i], dsts[i], counts[i] = src.data_ptr(), outs[-1].data_ptr(), n
    it = torch.tensor(items, dtype=torch.int32, device="cuda")
    og = torch.zeros(B, 2, dtype=torch.int32, device="cuda")
    N.check(N.lib().sbgm_cutout_gather(srcs, dsts, counts, nf, programs.data_ptr(), it.data_ptr(), og.data_ptr(), B, Hd, Wd, Hd, Wd, N.stream()))
    return [torch.nn.functional.pad(o, (0, Wp - Wd, 0, 0), mode="replicate").cpu() if Wp > Wd else o.cpu() for o in outs]


@pytest.mark.parametrize("items", [[2], [3, 0, 3]], ids=["B1", "B3_repeated"])
@pytest.mark.parametrize("shape", SHAPES)
def test_gather_matches_the_reference_and_the_padded_cutout(shape, items):
    Hd, Wd, Wp = shape
    host = host_fields(Hd, Wd)
    fields, _keep = device_fields(host)
    got = run_domain_gather(fields, items, Hd, Wd, Wp)
    other = run_cutout_gather_and_pad(fields, items, Hd, Wd, Wp)
    for (key, _s, _n, is_mask, _p, tr), g, o in zip(fields, got, other):
        want = DR.domain_gather(host[key], items, Wp, tr, bool(is_mask))
        assert g.shape == (len(items), 1, Hd, Wp) and g.dtype == torch.float32
        assert np.array_equal(bits(g.numpy()), bits(want)), f"{key} {shape}: {int((bits(g.numpy()) != bits(want)).sum())} of {want.size} differ"
        assert np.array_equal(bits(g.numpy()), bits(o.numpy())), f"{key} {shape}: differs from the padded cutout gather"
        for x in range(Wd, Wp):                                          # the pad is the last real column, after the program
            assert torch.equal(g[..., x], g[..., Wd - 1])
    assert set(got[3].unique().tolist()) <= {0.0, 1.0}
    assert got[3][0, 0, 0, 0] == 0.0 and got[3][0, 0, Hd - 1, Wd - 1] == 1.0        # 0.5 itself is sea, nextafter(0.5) is land
    assert not torch.equal(got[0], torch.from_numpy(DR.domain_gather(host["a"], items, Wp)))     # the program did run


@pytest.mark.parametrize("shape", SHAPES)
def test_items_outside_their_stack_give_nan_and_leave_the_others_alone(shape):
    Hd, Wd, Wp = shape
    host = host_fields(Hd, Wd)
    fields, _keep = device_fields(host)
    items = [1, N_ITEMS, -1]
    got = run_domain_gather(fields, items, Hd, Wd, Wp)
    clean = run_domain_gather(fields, [1], Hd, Wd, Wp)
    for (key, _s, n, is_mask, _p, tr), g, c in zip(fields, got, clean):
        want = DR.domain_gather(host[key], items, Wp, tr, bool(is_mask))
        assert np.array_equal(bits(g.numpy()), bits(want)), key
        assert torch.equal(g[0], c[0]), key
        assert torch.isnan(g[1:]).all() if n else not torch.isnan(g).any(), key      # a plane has no item to get wrong


def test_the_op_refuses_what_the_header_says():
    x = torch.arange(64, dtype=torch.float32, device="cuda")
    lib = N.lib()
    p = RD.upload_programs([(0, [])], "cuda")
    srcs, dsts, counts = (N._vp * 1)(x.data_ptr()), (N._vp * 1)(x.data_ptr()), (C.c_int * 1)(0)
    it = torch.zeros(1, dtype=torch.int32, device="cuda")
    call = lambda Wd, Wp: lib.sbgm_domain_gather(srcs, dsts, counts, 1, p.data_ptr(), it.data_ptr(), 1, 4, Wd, Wp, N.stream())  # noqa: E731
    assert call(9, 8) != 0 and b"padded width" in lib.sbgm_last_error()
    assert call(5, 6) != 0 and b"padded width" in lib.sbgm_last_error()
    dsts[0] = x.data_ptr() + 4
    assert call(5, 8) != 0 and b"16-byte aligned" in lib.sbgm_last_error()
    dsts[0] = x.data_ptr() + 128                                            # Wp - Wd >= 4 is accepted
    assert call(3, 8) == 0
    cols = torch.tensor([0, 1, 2, 2, 2, 2, 2, 2])
    assert torch.equal(x[32:].cpu().view(4, 8), (3 * torch.arange(4)[:, None] + cols[None]).float())
    assert torch.equal(x[:32].cpu(), torch.arange(32, dtype=torch.float32))


# ---- the loader ------------------------------------------------------------------------------------------------------------------------
HD, WD, TILE, WP = 44, 53, 32, 56
ZSTATS = {"prcp_hr": {"mean": 3.5, "std": 7.25}, "prcp_lr": {"mean": 2.5, "std": 5.5}, "temp_lr": {"mean": 8.7012, "std": 6.1923}}


def make_arrays(n, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:HD, 0:WD]
    return {"prcp_hr": (rng.random((n, HD, WD)) ** 4 * 60).astype(np.float32), "temp_lr": rng.normal(8, 6, (n, HD, WD)).astype(np.float32),
            "prcp_lr": (rng.random((n, HD, WD)) ** 4 * 40).astype(np.float32),
            "lsm": np.where((yy + xx) % 7 == 0, 0.3, ((yy - 20) ** 2 + (xx - 30) ** 2 < 150)).astype(np.float32),   # 0, 0.3 and 1
            "topo": (rng.random((HD, WD)) * 900 - 5).astype(np.float32), "classifier": (np.arange(n) % 4 + 1).astype(np.int64)}


def make_cfg(tmp_path):
    raw = yaml.safe_load(open(os.path.join(ROOT, "sbgm_danra_amd", "config", "default_config.yaml")))
    for sec in ("highres", "lowres"):
        raw[sec].update(data_size=[TILE, TILE], cutout_domains=[2, 38, 4, 52], full_domain_dims=[HD, WD])     # the training crop: ignored
    raw["highres"]["scaling_method"] = "zscore"
    raw["lowres"].update(condition_variables=["temp", "prcp"], scaling_methods=["zscore", "zscore"])
    raw["transforms"].update(sample_w_cutouts=True, scaling=True)
    raw["stationary_conditions"]["geographic_conditions"].update(sample_w_geo=True, sample_w_sdf=True)
    raw["stationary_conditions"]["seasonal_conditions"]["sample_w_cond_season"] = True
    raw["paths"] = {k: str(tmp_path / k) for k in ("data_dir", "checkpoint_dir", "sample_dir", "path_save", "stats_load_dir")}
    return to_config(raw)


def test_loader_serves_the_padded_domain_in_file_order(tmp_path):
    from sbgm_danra_amd.tiling import FullDomainTiler, padded_width
    from sbgm_danra_amd.utils import extract_any
    arrays = make_arrays(5, 3)
    path = str(tmp_path / "gen.npz")
    np.savez(path, **arrays)
    cfg = make_cfg(tmp_path)
    fields = RD.ResidentFields(path, "prcp", ["temp", "prcp"])
    assert padded_width(WD, TILE) == WP == FullDomainTiler((HD, WD), TILE, 4).Wd_pad
    z = lambda s: TR.ZScoreTransform(s["mean"], s["std"])  # noqa: E731
    tr = {k: z(ZSTATS[k]) for k in ZSTATS}
    tr["topo"] = TR.Scale(0.0, 1.0, float(arrays["topo"].min()), float(arrays["topo"].max()))
    for batch_size, first in ((2, 0), (3, 1), (5, 4)):
        dl = RD.ResidentDomainLoader(fields, cfg, WP, batch_size, first_day=first, stats=ZSTATS)
        assert dl.n_days == 5 - first and len(dl) == -(-(5 - first) // batch_size) and dl.domain_hw == (HD, WD)
        day = first
        for batch in dl:
            items = list(range(day, min(day + batch_size, 5)))
            want = DR.batch_ref(arrays, "prcp_hr", ["temp_lr", "prcp_lr"], items, WP, tr, with_classes=True)
            assert set(batch) == set(want), (sorted(batch), sorted(want))
            for k, v in batch.items():
                if k == "domain_hw":
                    assert v == (HD, WD)
                    continue
                assert v.is_cuda and tuple(v.shape) == want[k].shape, k
                assert torch.equal(v.cpu(), torch.from_numpy(want[k])), k
            assert batch["prcp_hr"].shape == (len(items), 1, HD, WP) and batch["prcp_hr"].data_ptr() % 16 == 0
            x, y, lr, _lsm_hr, lsm, sdf, topo, _hp, _lp = extract_any(batch, torch.device("cuda"))          # Hd * Wp % 4 == 0: as it is
            assert lr.shape == (len(items), 2, HD, WP) and lsm.shape == topo.shape == (len(items), 2, HD, WP) and sdf is None
            assert torch.equal(lr[:, 1:2], batch["temp_lr"]) and torch.equal(lsm[:, :1], batch["lsm"]) and y.tolist() == [i % 4 + 1 for i in items]
            day += len(items)
        assert day == 5
    for bad in (dict(padded_width=52), dict(padded_width=54), dict(padded_width=WP, first_day=5), dict(padded_width=WP, batch_size=0)):
        with pytest.raises(ValueError, match="ResidentDomainLoader"):
            RD.ResidentDomainLoader(fields, cfg, **dict(dict(batch_size=2, stats=ZSTATS), **bad))
