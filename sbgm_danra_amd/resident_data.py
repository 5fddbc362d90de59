"""Device-resident data: the fields of a split live in HBM and every batch is cut, transformed and given its signed-distance field by
three native ops (csrc/cutout.hip) — what the reference's `DANRA_Dataset_cutouts_ERA5_Zarr.__getitem__` does per sample on the host
(data_modules.py:727-997: `find_rand_points` :184-223, the crops, the scalar transforms, `generate_sdf` / `normalize_sdf` :93-118).

    ResidentFields        one .npz per split, validated and uploaded once
    ResidentCutoutLoader  iterable of the reference's batch dicts, as device tensors
    ResidentDomainLoader  iterable of whole days of a split, right-padded for `tiling.FullDomainTiler` (one `sbgm_domain_gather` per batch):
                          what `get_gen_dataloader` returns with an `evaluation.full_domain` section (`full_domain_config`)
    resident_loaders / resident_gen_loader   what `training_utils.get_dataloader` / `get_gen_dataloader` return when the config has
                          `data_handling.resident_fields: {train: <npz>, valid: <npz>, gen: <npz>}`

npz layout: `<hr_var>_hr` [N, Hd, Wd]; `<cond>_lr` [N, Hd, Wd] per condition variable, already on the HR grid; `lsm`, `topo` [Hd, Wd]
(optional); `classifier` [N] integer (optional); `dates` [N] (optional): integer days since 1970-01-01 or datetime64[D], strictly increasing.  Resizing is out of scope: the LR cutout must be the HR cutout and `resize_factor` 1.

Two deliberate differences from the reference, both on crops without a coastline (include/sbgm_hip.h, sbgm_sdf_from_mask): an all-land
crop gets sdf = 1 (reference: 0/0 = NaN, which poisons the loss) and an all-sea crop gets sdf = 0 (reference: scipy's transform of an
input without background, not a distance to anything).

Draw numbers: batch `i` of epoch `e` draws its origins from Philox offset
`draw_number(split, e, i, rank) = ((split_id * 4096 + rank) * 2^24 + e) * 2^24 + i`, split_id = 0 train, 1 valid, 2 gen; validation and
generation always use e = 0, so their cutouts — and a validation loss — are the same in every epoch.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _native as N
from .calendar import day_numbers
from .special_transforms import Scale, _Chain, get_transforms_from_stats

SPLIT_IDS = {"train": 0, "valid": 1, "gen": 2}
MAX_LR = 16


def draw_number(split: str, epoch: int, batch: int, rank: int = 0) -> int:
    if not (0 <= epoch < 1 << 24 and 0 <= batch < 1 << 24 and 0 <= rank < 4096):
        raise ValueError(f"draw_number: epoch={epoch}, batch={batch} (each < 2^24), rank={rank} (< 4096)")
    e = epoch if split == "train" else 0
    return (((SPLIT_IDS[split] * 4096 + rank) << 24 | e) << 24) | batch


class ResidentFields:
    """The fields of one split on the device.  `stacks`: key -> fp32 [N, Hd, Wd]; `planes`: 'lsm' / 'topo' -> fp32 [Hd, Wd];
    `classifier`: int64 [N] or None; `dates`: HOST int64 day numbers [N] or None; `topo_range`: (min, max) of the topography plane, taken on the host before the upload."""

    def __init__(self, path, hr_var, lr_vars=(), device="cuda", need=()):
        lr_vars = list(lr_vars or [])
        if len(lr_vars) > MAX_LR:
            raise ValueError(f"{len(lr_vars)} condition variables (max {MAX_LR})")
        with np.load(path) as z:
            arrays = {k: z[k] for k in z.files}
        stack_keys = [f"{hr_var}_hr"] + [f"{v}_lr" for v in lr_vars]
        shape = None
        for k in stack_keys:
            a = self._floating(arrays, k, path)
            if a.ndim != 3 or a.shape[0] < 1:
                raise ValueError(f"{path}: '{k}' has shape {a.shape}, expected [N, Hd, Wd]")
            if shape is None:
                shape = a.shape
            elif a.shape != shape:
                raise ValueError(f"{path}: '{k}' has shape {a.shape}, but '{stack_keys[0]}' has {shape}")
        self.n_items, self.Hd, self.Wd = (int(s) for s in shape)
        for k in ("lsm", "topo"):
            if k not in arrays:
                if k in need:
                    raise ValueError(f"{path}: key '{k}' is missing (the configuration asks for it)")
                continue
            a = self._floating(arrays, k, path)
            if a.shape != shape[1:]:
                raise ValueError(f"{path}: '{k}' has shape {a.shape}, expected the domain {tuple(shape[1:])}")
        cls = arrays.get("classifier")
        if cls is None and "classifier" in need:
            raise ValueError(f"{path}: key 'classifier' is missing (the configuration asks for it)")
        if cls is not None and (cls.shape != (self.n_items,) or not np.issubdtype(cls.dtype, np.integer)):
            raise ValueError(f"{path}: 'classifier' has shape {cls.shape} and dtype {cls.dtype}, expected [{self.n_items}] integers")
        dev = torch.device(device)
        if dev.type != "cuda":
            raise N.NativeError(f"ResidentFields keeps its fields on a ROCm device, got device={device!r}")
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)       # noqa: E731
        self.path, self.device, self.hr_key, self.lr_keys = path, dev, stack_keys[0], stack_keys[1:]
        self.topo_range = (float(arrays["topo"].min()), float(arrays["topo"].max())) if "topo" in arrays else None
        self.lsm_range = (float(arrays["lsm"].min()), float(arrays["lsm"].max())) if "lsm" in arrays else None
        self.stacks = {k: up(arrays[k]) for k in stack_keys}
        self.planes = {k: up(arrays[k]) for k in ("lsm", "topo") if k in arrays}
        self.classifier = None if cls is None else torch.from_numpy(cls.astype(np.int64)).to(dev)
        self.dates = None                                   # host int64 day numbers [N] (calendar.day_numbers), or None
        if "dates" in arrays:
            try:
                self.dates = day_numbers(arrays["dates"])
            except ValueError as e:
                raise ValueError(f"{path}: {e}") from None
            if self.dates.shape != (self.n_items,):
                raise ValueError(f"{path}: 'dates' holds {self.dates.shape[0]} days, the fields {self.n_items}")

    @staticmethod
    def _floating(arrays, key, path):
        if key not in arrays:
            raise ValueError(f"{path}: key '{key}' is missing")
        a = arrays[key]
        if not np.issubdtype(a.dtype, np.floating):
            raise ValueError(f"{path}: '{key}' has dtype {a.dtype}, expected a floating-point field")
        return a


def _scalar_stats(stats, key):
    for name, v in (stats or {}).items():
        if v is not None and np.ndim(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v) != 0 and np.size(v) != 1:
            raise ValueError(f"'{key}': the statistic '{name}' has shape {np.shape(v)}; per-element statistics are not supported "
                             f"by the resident loader (scalar statistics only)")


def cutout_geometry(cfg, Hd, Wd):
    """-> (rect [r0, r1, c0, c1], (h, w)) from the config; ValueError for what the resident loader does not do."""
    hr, lr = cfg["highres"], cfg["lowres"]
    rf = lr.get("resize_factor", 1)
    if rf not in (None, 1):
        raise ValueError(f"lowres.resize_factor = {rf}: the resident loader does not resize (only resize_factor 1 is supported)")
    for key in ("data_size", "cutout_domains"):
        a, b = lr.get(key), hr.get(key)
        if a is not None and (b is None or list(a) != list(b)):
            raise ValueError(f"lowres.{key} = {list(a)} differs from highres.{key} = {None if b is None else list(b)}: the resident loader "
                             f"cuts LR and HR at the same rectangle (resizing is not supported)")
    dom = hr.get("cutout_domains")
    rect = [int(v) for v in dom] if dom is not None else [0, Hd, 0, Wd]
    if len(rect) != 4 or not (0 <= rect[0] < rect[1] <= Hd and 0 <= rect[2] < rect[3] <= Wd):
        raise ValueError(f"highres.cutout_domains = {rect} lies outside the {Hd}x{Wd} domain of the fields")
    size = hr.get("data_size")
    if (cfg.get("transforms", {}) or {}).get("sample_w_cutouts", False):
        if size is None:
            raise ValueError("transforms.sample_w_cutouts needs highres.data_size")
        h, w = int(size[0]), int(size[1])
        if h > rect[1] - rect[0] or w > rect[3] - rect[2]:
            raise ValueError(f"Crop size {h}x{w} is larger than the rectangle dimensions {rect[1] - rect[0]}x{rect[3] - rect[2]}.")
    else:
        h, w = rect[1] - rect[0], rect[3] - rect[2]
        if size is not None and (int(size[0]), int(size[1])) != (h, w):
            raise ValueError(f"without transforms.sample_w_cutouts a sample is the whole {h}x{w} rectangle, but highres.data_size is "
                             f"{list(size)}: the resident loader does not resize")
    return rect, (h, w)


def build_transforms(cfg, fields, stats=None):
    """key -> transform (`_Chain`) or None, for every field the loader gathers: the reference's choice per variable
    (data_modules.py:568-640 through get_transforms_from_stats, statistics files named as training._build_back_transforms names them) and,
    for `topo`, the min-max scaling of reference training_utils.py:146-162.  `stats`: key -> statistics dict, instead of the files."""
    out = {k: None for k in [fields.hr_key] + fields.lr_keys}
    if not (cfg.get("transforms", {}) or {}).get("scaling", False):
        return out
    hr, lr = cfg["highres"], cfg["lowres"]
    dims = lambda d: f"{d[0]}x{d[1]}" if d is not None else "full_domain"                 # noqa: E731
    crop = lambda c: "_".join(map(str, c)) if c is not None else "no_crop"               # noqa: E731
    jobs = [(fields.hr_key, hr["variable"], hr["model"], hr, hr["scaling_method"])]
    jobs += [(k, v, lr["model"], lr, m) for k, v, m in zip(fields.lr_keys, lr["condition_variables"] or [], lr["scaling_methods"])]
    for key, var, model, sec, method in jobs:
        st = (stats or {}).get(key)
        _scalar_stats(st, key)
        out[key] = get_transforms_from_stats(variable=var, model=model, domain_str=dims(sec.get("full_domain_dims")),
                                             crop_region_str=crop(sec.get("cutout_domains")), split="all", transform_type=method,
                                             buffer_frac=sec.get("buffer_frac", 0.5), stats=st,
                                             stats_file_path="" if st else cfg["paths"]["stats_load_dir"])
    geo = cfg["stationary_conditions"]["geographic_conditions"]
    if "topo" in fields.planes:
        g = lambda k, d: d if geo.get(k) is None else geo[k]                              # noqa: E731
        t_min, t_max = g("topo_min", fields.topo_range[0]), g("topo_max", fields.topo_range[1])
        lsm_rng = fields.lsm_range or (0.0, 1.0)
        out["topo"] = Scale(g("norm_min", lsm_rng[0]), g("norm_max", lsm_rng[1]), t_min, t_max)
    return out


def upload_programs(fields, device) -> torch.Tensor:
    """[(is_mask, transform or program or None)] -> the device table sbgm_cutout_gather reads: int32 [n][CUTOUT_PROGRAM_WORDS]"""
    W = N.CUTOUT_PROGRAM_WORDS
    host = (C.c_int32 * (W * len(fields)))()
    for i, (is_mask, tr) in enumerate(fields):
        prog = [] if tr is None else list(tr.program() if isinstance(tr, _Chain) else tr)
        ops = (C.c_int * max(1, len(prog)))(*[int(o) for o, _ in prog])
        cs = (C.c_float * max(1, len(prog)))(*[float(c) for _, c in prog])
        row = C.cast(C.byref(host, 4 * W * i), C.POINTER(C.c_int32))
        N.check(N.lib().sbgm_cutout_program_init(row, len(prog), ops, cs, int(is_mask)))
    return torch.frombuffer(bytearray(bytes(host)), dtype=torch.int32).reshape(len(fields), W).to(device)


class ResidentCutoutLoader:
    """Iterable of batch dicts cut from `fields` on the device: one origin draw, one gather over every field and, with
    `sample_w_sdf`, one signed-distance transform per batch.  Keys: `<hr_var>_hr`, `<cond>_lr`, raw 1-channel `lsm` / `topo`
    (`training._extract` then assembles the mask channel and the CFG dropout on the device), `lsm_hr`, `sdf`, `classifier`,
    `hr_points` / `lr_points` (int64 [B, 4] rows [r0, r1, c0, c1]).  Training shuffles with a host permutation per epoch from
    (seed, epoch), uploaded once per epoch; `shard=(rank, world)` takes every world-th item of it from `rank`."""

    def __init__(self, fields: ResidentFields, cfg, split="train", batch_size=None, seed=0, shard=None, drop_last=None, stats=None):
        if split not in SPLIT_IDS:
            raise ValueError(f"split = {split!r}: one of {sorted(SPLIT_IDS)}")
        self.fields, self.cfg, self.split, self.seed = fields, cfg, split, int(seed)
        self.batch_size = int(batch_size if batch_size is not None else cfg["training"]["batch_size"])
        self.rank, self.world = (int(shard[0]), int(shard[1])) if shard else (0, 1)
        self.shuffle = split == "train"
        self.drop_last = (split == "train") if drop_last is None else bool(drop_last)
        self.epoch = 0
        self.rect, (self.h, self.w) = cutout_geometry(cfg, fields.Hd, fields.Wd)
        geo = cfg["stationary_conditions"]["geographic_conditions"]
        self.with_sdf = bool(geo.get("sample_w_sdf", False))
        geo_vars = list(geo.get("geo_variables") or []) if geo.get("sample_w_geo", False) else []
        self.with_classes = bool(cfg["stationary_conditions"]["seasonal_conditions"].get("sample_w_cond_season", False))
        if self.with_classes and fields.classifier is None:
            raise ValueError(f"{fields.path}: key 'classifier' is missing, but seasonal_conditions.sample_w_cond_season is set")
        for k in geo_vars + (["lsm"] if self.with_sdf else []):
            if k in ("lsm", "topo") and k not in fields.planes:
                raise ValueError(f"{fields.path}: key '{k}' is missing, but the geographic conditions ask for it")
        transforms = build_transforms(cfg, fields, stats)
        # (batch key, source tensor, n_items, is_mask, program)
        plan = [(k, fields.stacks[k], fields.n_items, 0, transforms[k]) for k in [fields.hr_key] + fields.lr_keys]
        self.yield_lsm, self.yield_topo = "lsm" in geo_vars, "topo" in geo_vars
        if self.yield_lsm or self.with_sdf:
            plan.append(("lsm", fields.planes["lsm"], 0, 1, None))
        if self.yield_topo:
            plan.append(("topo", fields.planes["topo"], 0, 0, transforms.get("topo")))
        self.plan = plan
        lib = N.lib()
        self.programs = upload_programs([(is_mask, tr) for _k, _s, _n, is_mask, tr in plan], fields.device)   # once, not per batch
        self._rect = (C.c_int * 4)(*self.rect)
        self._extent = torch.tensor([0, self.h, 0, self.w], dtype=torch.int64, device=fields.device)
        self._cols = torch.tensor([0, 0, 1, 1], dtype=torch.int64, device=fields.device)
        self._sdf_ws = None
        if self.with_sdf:
            nbytes = lib.sbgm_sdf_workspace_bytes(self.batch_size, self.h, self.w)
            if nbytes < 0:
                N.check(1)
            self._sdf_ws = torch.empty(nbytes, dtype=torch.uint8, device=fields.device)
        self._items, self._items_epoch = None, None

    # ---- item order -----------------------------------------------------------------------------------------------------------
    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)

    def item_order(self, epoch=None) -> np.ndarray:
        """the items this rank visits in `epoch`, in order (host int64)"""
        e = self.epoch if epoch is None else int(epoch)
        n = self.fields.n_items
        order = np.random.default_rng([self.seed, e]).permutation(n) if self.shuffle else np.arange(n)
        if self.world > 1:
            if self.drop_last:
                order = order[: n // self.world * self.world]      # every rank runs the same number of steps
            order = order[self.rank::self.world]
        return order.astype(np.int64)

    def __len__(self):
        n = len(self.item_order(0))
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def draw_number(self, batch: int) -> int:
        return draw_number(self.split, self.epoch, batch, self.rank)

    # ---- one batch ------------------------------------------------------------------------------------------------------------
    def cut(self, items: torch.Tensor, origins: torch.Tensor, items_host=None) -> dict:
        """the batch for given device tensors items int32 [B] and origins int32 [B, 2] (what __iter__ calls after its draw).
        `items_host`: the same items as a host array, for `batch["dates"]`; without it a split with dates copies `items` to the
        host, which synchronises (__iter__ passes its own host order, so its batches never do)"""
        F, dev, lib = self.fields, self.fields.device, N.lib()
        B = items.shape[0]
        nf = len(self.plan)
        srcs, dsts, counts, outs = (N._vp * nf)(), (N._vp * nf)(), (C.c_int * nf)(), {}
        block = torch.empty(nf, B, 1, self.h, self.w, device=dev)          # one allocation; the batch holds views of it
        for i, (key, src, n, _m, _t) in enumerate(self.plan):
            outs[key] = block[i]
            srcs[i], dsts[i], counts[i] = src.data_ptr(), outs[key].data_ptr(), n
        N.check(lib.sbgm_cutout_gather(srcs, dsts, counts, nf, self.programs.data_ptr(), items.data_ptr(), origins.data_ptr(), B, F.Hd, F.Wd,
                                       self.h, self.w, N.stream()))
        batch = {k: outs[k] for k in [F.hr_key] + F.lr_keys}
        if "lsm" in outs:
            batch["lsm_hr"] = outs["lsm"]
            if self.yield_lsm:
                batch["lsm"] = outs["lsm"]
        if self.yield_topo:
            batch["topo"] = outs["topo"]
        if self.with_sdf:
            ws = self._sdf_ws
            if B != self.batch_size:                                # ragged last batch of a split that keeps it
                ws = torch.empty(lib.sbgm_sdf_workspace_bytes(B, self.h, self.w), dtype=torch.uint8, device=dev)
            batch["sdf"] = torch.empty(B, 1, self.h, self.w, device=dev)
            N.check(lib.sbgm_sdf_from_mask(outs["lsm"].data_ptr(), batch["sdf"].data_ptr(), None, ws.data_ptr(), B, self.h, self.w, N.stream()))
        if self.with_classes:
            batch["classifier"] = F.classifier.index_select(0, items.long())
        pts = origins.long().index_select(1, self._cols) + self._extent             # rows [r0, r1, c0, c1]
        batch["hr_points"], batch["lr_points"] = pts, pts.clone()
        if F.dates is not None:
            batch["dates"] = F.dates[items.cpu().numpy() if items_host is None else np.asarray(items_host, np.int64)]   # host int64 [B]
        return batch

    def draw_origins(self, batch: int, B: int) -> torch.Tensor:
        origins = torch.empty(B, 2, dtype=torch.int32, device=self.fields.device)
        N.check(N.lib().sbgm_cutout_draw(self.seed, self.draw_number(batch), B, self._rect, self.h, self.w, self.fields.Hd, self.fields.Wd,
                                         origins.data_ptr(), N.stream()))
        return origins

    def __iter__(self):
        if self._items is None or self._items_epoch != self.epoch or self.shuffle:
            self._items_host = self.item_order()
            self._items = torch.from_numpy(self._items_host.astype(np.int32)).to(self.fields.device)     # once per epoch
            self._items_epoch = self.epoch
        items_all, host_all = self._items, self._items_host
        for i in range(len(self)):
            items = items_all[i * self.batch_size:(i + 1) * self.batch_size]
            yield self.cut(items, self.draw_origins(i, items.shape[0]), host_all[i * self.batch_size:(i + 1) * self.batch_size])
        if self.shuffle:
            self.epoch += 1          # a loop that never calls set_epoch still sees a new order and new cutouts every epoch


FULL_DOMAIN_KEYS = ("tile", "halo", "joint", "tiles_per_batch", "first_day")


def full_domain_config(cfg, domain_hw=None):
    """The optional evaluation.full_domain section as {tile, halo, joint, tiles_per_batch, first_day}, or None without it.  With the
    section `gen_type: [series]` downscales the whole domain of `data_handling.resident_fields.gen` through `FullDomainTiler`
    (`SampleGenerator.generate_series`).  `tile` (default highres.data_size[0]) and `halo` (default 32) are the tiler's, `joint` and
    `tiles_per_batch` (default: all tiles of a rank in one batch) those of `FullDomainTiler.sample`; `first_day` >= 0 skips that many
    days of the split and keeps their absolute noise rows.  Every refusal is a ValueError that names its key: an unknown key, a value of
    the wrong type, `rk45_sampler`, a `gen_type` beside `series`, a configuration without the generation split's file and — with
    `domain_hw` = (Hd, Wd), once the file is open — a tile or halo the tile table (`tiling.axis_origins`) refuses for that domain."""
    ev = cfg["evaluation"]
    sec = ev.get("full_domain") if hasattr(ev, "get") else None
    if sec is None:
        return None
    if not hasattr(sec, "keys") or not set(sec.keys()) <= set(FULL_DOMAIN_KEYS):
        raise ValueError(f"evaluation.full_domain takes the keys {list(FULL_DOMAIN_KEYS)} only, got {sec!r}")
    integer = lambda v: isinstance(v, int) and not isinstance(v, bool)                    # noqa: E731
    size = cfg["highres"].get("data_size")
    tile = sec.get("tile") if sec.get("tile") is not None else (None if size is None else int(size[0]))
    halo, joint, per, first = sec.get("halo", 32), sec.get("joint", False), sec.get("tiles_per_batch"), sec.get("first_day", 0)
    if not integer(tile) or tile < 1:
        raise ValueError(f"evaluation.full_domain.tile must be an integer >= 1 (default: highres.data_size[0]), got {tile!r}")
    if not integer(halo) or not 0 <= 2 * halo < tile:
        raise ValueError(f"evaluation.full_domain.halo must be an integer with 0 <= 2 * halo < tile = {tile}, got {halo!r}")
    if not isinstance(joint, bool):
        raise ValueError(f"evaluation.full_domain.joint must be true or false, got {joint!r}")
    if per is not None and (not integer(per) or per < 1):
        raise ValueError(f"evaluation.full_domain.tiles_per_batch must be null or an integer >= 1, got {per!r}")
    if not integer(first) or first < 0:
        raise ValueError(f"evaluation.full_domain.first_day must be an integer >= 0, got {first!r}")
    if cfg["sampler"].get("sampler_type") == "rk45_sampler":
        raise ValueError("evaluation.full_domain: sampler.sampler_type rk45_sampler does not take a domain noise plan (use pc_sampler, "
                         "edm_heun_sampler or dpmpp_2m_sampler)")
    kinds = list(ev.get("gen_type") or [])
    if kinds != ["series"]:
        raise ValueError(f"evaluation.full_domain serves evaluation.gen_type ['series'] alone, got {kinds}: the other types draw crops "
                         "of highres.data_size from another loader")
    paths = (cfg.get("data_handling", {}) or {}).get("resident_fields") or {}
    if not (hasattr(paths, "get") and paths.get("gen")):
        raise ValueError("evaluation.full_domain needs data_handling.resident_fields.gen, the .npz of the generation split")
    if domain_hw is not None:
        from .tiling import axis_origins, padded_width
        try:
            axis_origins(int(domain_hw[0]), tile, 2 * halo)
            axis_origins(padded_width(domain_hw[1], tile), tile, 2 * halo, align=4)
        except ValueError as e:
            raise ValueError(f"evaluation.full_domain: tile {tile}, halo {halo} on the {domain_hw[0]}x{domain_hw[1]} domain: {e}") from None
    return {"tile": tile, "halo": halo, "joint": joint, "tiles_per_batch": per, "first_day": first}


class ResidentDomainLoader:
    """Iterable over the days of `fields` in file order, `batch_size` days at a time from `first_day` on, each batch the WHOLE domain,
    right-padded to `padded_width` (the `Wd_pad` of the `FullDomainTiler` it feeds, `tiling.padded_width`): one `sbgm_domain_gather`
    over every field per batch, no origin draw and no shuffle.  Keys as `ResidentCutoutLoader` (`<hr_var>_hr`, `<cond>_lr`, raw
    1-channel `lsm` / `topo`, `lsm_hr`, `classifier`, `hr_points` / `lr_points` = [0, Hd, 0, Wd]) with every field [B, 1, Hd, Wp], plus
    `domain_hw` = (Hd, Wd).  No `sdf`: it weights the training loss.  The rectangle is the domain of the file, whatever
    highres.data_size and cutout_domains say (they describe the training crop); the transforms are `build_transforms`'."""

    def __init__(self, fields: ResidentFields, cfg, padded_width, batch_size=None, first_day=0, stats=None):
        rf = cfg["lowres"].get("resize_factor", 1)
        if rf not in (None, 1):
            raise ValueError(f"lowres.resize_factor = {rf}: the resident loader does not resize (only resize_factor 1 is supported)")
        self.fields, self.cfg = fields, cfg
        self.batch_size = int(batch_size if batch_size is not None else cfg["evaluation"]["batch_size"])
        self.first_day, self.Wp = int(first_day), int(padded_width)
        self.domain_hw = (fields.Hd, fields.Wd)
        if self.batch_size < 1 or not 0 <= self.first_day < fields.n_items:
            raise ValueError(f"ResidentDomainLoader: batch_size={self.batch_size} (>= 1), first_day={self.first_day} of the "
                             f"{fields.n_items} days of {fields.path}")
        if self.Wp < fields.Wd or self.Wp % 4:
            raise ValueError(f"ResidentDomainLoader: padded_width={self.Wp} must be a multiple of 4 and at least the domain width {fields.Wd}")
        geo = cfg["stationary_conditions"]["geographic_conditions"]
        geo_vars = list(geo.get("geo_variables") or []) if geo.get("sample_w_geo", False) else []
        self.with_classes = bool(cfg["stationary_conditions"]["seasonal_conditions"].get("sample_w_cond_season", False))
        if self.with_classes and fields.classifier is None:
            raise ValueError(f"{fields.path}: key 'classifier' is missing, but seasonal_conditions.sample_w_cond_season is set")
        for k in geo_vars:
            if k in ("lsm", "topo") and k not in fields.planes:
                raise ValueError(f"{fields.path}: key '{k}' is missing, but the geographic conditions ask for it")
        transforms = build_transforms(cfg, fields, stats)
        plan = [(k, fields.stacks[k], fields.n_items, 0, transforms[k]) for k in [fields.hr_key] + fields.lr_keys]
        self.yield_lsm, self.yield_topo = "lsm" in geo_vars, "topo" in geo_vars
        if self.yield_lsm:
            plan.append(("lsm", fields.planes["lsm"], 0, 1, None))
        if self.yield_topo:
            plan.append(("topo", fields.planes["topo"], 0, 0, transforms.get("topo")))
        self.plan = plan
        self.programs = upload_programs([(is_mask, tr) for _k, _s, _n, is_mask, tr in plan], fields.device)   # once, not per batch
        self._items = torch.arange(fields.n_items, dtype=torch.int32, device=fields.device)
        self._points = torch.tensor([0, fields.Hd, 0, fields.Wd], dtype=torch.int64, device=fields.device)

    @property
    def n_days(self):
        """the days the loader serves: those of the split from `first_day` on"""
        return self.fields.n_items - self.first_day

    def __len__(self):
        return -(-self.n_days // self.batch_size)

    def gather(self, items: torch.Tensor, items_host=None) -> dict:
        """the batch of the days `items` (device int32 [B]; what __iter__ calls, with the same days as a host array for
        `batch["dates"]`: without `items_host` a split with dates copies `items` to the host, which synchronises)"""
        F, dev = self.fields, self.fields.device
        B, nf = items.shape[0], len(self.plan)
        srcs, dsts, counts, outs = (N._vp * nf)(), (N._vp * nf)(), (C.c_int * nf)(), {}
        block = torch.empty(nf, B, 1, F.Hd, self.Wp, device=dev)           # one allocation; the batch holds views of it
        for i, (key, src, n, _m, _t) in enumerate(self.plan):
            outs[key] = block[i]
            srcs[i], dsts[i], counts[i] = src.data_ptr(), outs[key].data_ptr(), n
        N.check(N.lib().sbgm_domain_gather(srcs, dsts, counts, nf, self.programs.data_ptr(), items.data_ptr(), B, F.Hd, F.Wd, self.Wp,
                                           N.stream()))
        batch = {k: outs[k] for k in [F.hr_key] + F.lr_keys}
        if self.yield_lsm:
            batch["lsm"] = batch["lsm_hr"] = outs["lsm"]
        if self.yield_topo:
            batch["topo"] = outs["topo"]
        if self.with_classes:
            batch["classifier"] = F.classifier.index_select(0, items.long())
        pts = self._points.expand(B, 4).contiguous()
        batch["hr_points"], batch["lr_points"], batch["domain_hw"] = pts, pts.clone(), self.domain_hw
        if F.dates is not None:
            batch["dates"] = F.dates[items.cpu().numpy() if items_host is None else np.asarray(items_host, np.int64)]   # host int64 [B]
        return batch

    def __iter__(self):
        for d in range(self.first_day, self.fields.n_items, self.batch_size):
            yield self.gather(self._items[d:d + self.batch_size], np.arange(d, min(d + self.batch_size, self.fields.n_items)))


def _split_fields(cfg, split, device):
    paths = cfg["data_handling"]["resident_fields"]
    if split not in paths or not paths[split]:
        raise ValueError(f"data_handling.resident_fields has no '{split}' file")
    geo = cfg["stationary_conditions"]["geographic_conditions"]
    need = list(geo.get("geo_variables") or []) if geo.get("sample_w_geo", False) else []
    need += ["lsm"] if geo.get("sample_w_sdf", False) else []
    need += ["classifier"] if cfg["stationary_conditions"]["seasonal_conditions"].get("sample_w_cond_season", False) else []
    return ResidentFields(paths[split], cfg["highres"]["variable"], cfg["lowres"]["condition_variables"], device=device, need=need)


def _device(cfg):
    if not torch.cuda.is_available():
        raise N.NativeError("data_handling.resident_fields keeps the fields on a ROCm device and none is present")
    return torch.device("cuda", torch.cuda.current_device())       # the rank's device (parallel.init_distributed selects it)


def resident_loaders(cfg, shard=None):
    """(train, valid, gen) resident loaders; same roles, batch sizes and sharding as the synthetic ones of get_dataloader"""
    bs, seed = cfg["training"]["batch_size"], int(cfg["training"].get("seed", 0) or 0)
    n_gen = max(1, int(cfg["data_handling"].get("n_gen_samples", 1) or 1))
    dev = _device(cfg)
    return (ResidentCutoutLoader(_split_fields(cfg, "train", dev), cfg, "train", bs, seed, shard=shard, drop_last=True),
            ResidentCutoutLoader(_split_fields(cfg, "valid", dev), cfg, "valid", bs, seed),
            ResidentCutoutLoader(_split_fields(cfg, "gen", dev), cfg, "gen", n_gen, seed))


def resident_domain_loader(cfg, shard=None):
    """the `ResidentDomainLoader` of a configuration with an evaluation.full_domain section: evaluation.batch_size days a batch, padded
    for the section's tile; one rank only (the days of a series keep the file's order)"""
    from .tiling import padded_width
    fd = full_domain_config(cfg)
    if fd is None:
        raise ValueError("resident_domain_loader: the configuration has no evaluation.full_domain section")
    if shard is not None and shard[1] > 1:
        raise ValueError(f"evaluation.full_domain runs on one rank, got {shard[1]}: sharded days would break the day order of the series")
    fields = _split_fields(cfg, "gen", _device(cfg))
    fd = full_domain_config(cfg, (fields.Hd, fields.Wd))
    return ResidentDomainLoader(fields, cfg, padded_width(fields.Wd, fd["tile"]), int(cfg["evaluation"]["batch_size"]), fd["first_day"])


def resident_gen_loader(cfg, shard=None):
    bs, seed = int(cfg["evaluation"]["batch_size"]), int(cfg["evaluation"].get("seed", 0) or 0)
    world = shard[1] if shard is not None else 1
    return ResidentCutoutLoader(_split_fields(cfg, "gen", _device(cfg)), cfg, "gen", bs, seed, shard=shard if world > 1 else None)
