"""Host restatement of the device-resident cutout path (csrc/cutout.hip, sbgm_danra_amd/resident_data.py), in numpy + scipy + the
PyTorch-CPU transform oracle.  TEST INFRASTRUCTURE ONLY.

    draw_origins         find_rand_points (reference data_modules.py:184-223) with the kernel's Philox draw: the uniforms of
                         tests/philox_ref.uniform4 and the fp32 expression y0 = r0 + min(max_off, (int)floorf(u * (float)(max_off + 1)))
    crop_transform       numpy slicing, then an oracle.transforms_ref transform, then the mask re-binarise (:874, :909)
    generate_sdf / normalize_sdf / sdf_ref   reference :93-118 around scipy.ndimage.distance_transform_edt, in float64, with the two
                         no-coastline rules of the device path (all land -> 1, all sea -> 0; the reference gives NaN / scipy's
                         transform of an input without background there)
    edt_squared_scipy    rint(scipy^2): the exact squared distances as integers (-1 throughout a mask with no land)
    edt_squared_separable   a plain separable integer transform (column distances, then a full row minimum), as a second opinion
    batch_ref            the whole batch dict of ResidentCutoutLoader for given items and origins
"""
import numpy as np
import torch
from scipy.ndimage import distance_transform_edt

import philox_ref

SPLIT_IDS = {"train": 0, "valid": 1, "gen": 2}


def offset_from_uniform(u, max_off):
    """the fp32 expression of the draw kernel for uniforms u (float32 array) and one max_off"""
    u = np.asarray(u, dtype=np.float32)
    prod = (u * np.float32(max_off + 1)).astype(np.float32)          # one fp32 product
    return np.minimum(np.int64(max_off), np.floor(prod).astype(np.int64))


def draw_origins(seed, draw, B, rect, crop):
    """int32 [B, 2] = (y0, x0); rect = [r0, r1, c0, c1], crop = (h, w)"""
    r0, r1, c0, c1 = rect
    h, w = crop
    if h > r1 - r0 or w > c1 - c0:
        raise ValueError("Crop size is larger than the rectangle dimensions.")
    u = philox_ref.uniform4(seed, draw, np.arange(B, dtype=np.uint64))
    y0 = r0 + offset_from_uniform(u[:, 0], r1 - r0 - h)
    x0 = c0 + offset_from_uniform(u[:, 1], c1 - c0 - w)
    return np.stack([y0, x0], axis=1).astype(np.int32)


def draw_number(split, epoch, batch, rank=0):
    e = epoch if split == "train" else 0
    return ((SPLIT_IDS[split] * 4096 + rank) * 2 ** 24 + e) * 2 ** 24 + batch


def crop_transform(stack, items, origins, crop, transform=None, is_mask=False):
    """float32 [B, 1, h, w]: stack [N, Hd, Wd] (items index it) or a plane [Hd, Wd] (items ignored)"""
    h, w = crop
    out = []
    for b, (y0, x0) in enumerate(np.asarray(origins)):
        plane = stack[int(items[b])] if stack.ndim == 3 else stack
        t = torch.from_numpy(np.ascontiguousarray(plane[y0:y0 + h, x0:x0 + w], dtype=np.float32))
        if transform is not None:
            t = transform(t)
        if is_mask:
            t = (t > 0.5).to(t.dtype)
        out.append(t.numpy())
    return np.stack(out)[:, None]


def generate_sdf(mask):                                             # data_modules.py:93-103, float64
    land = np.asarray(mask) > 0
    return 10.0 * land.astype(np.float64) - distance_transform_edt(~land)


def normalize_sdf(sdf):                                             # :105-118
    return (sdf - sdf.min()) / (sdf.max() - sdf.min())


def sdf_ref(mask):
    """float64 [h, w] of one sample, with the device path's two no-coastline rules"""
    land = np.asarray(mask) > 0
    if land.all():
        return np.ones(land.shape, dtype=np.float64)
    if not land.any():
        return np.zeros(land.shape, dtype=np.float64)
    return normalize_sdf(generate_sdf(mask))


def edt_squared_scipy(mask):
    land = np.asarray(mask) > 0
    if not land.any():
        return np.full(land.shape, -1, dtype=np.int64)
    d = distance_transform_edt(~land)
    return np.rint(d * d).astype(np.int64)


def edt_squared_separable(mask):
    """exact squared distance to the nearest land pixel by two separable integer passes; a column without land carries a sentinel whose
    square exceeds every true distance and does not overflow.  A mask with no land gives -1."""
    land = np.asarray(mask) > 0
    h, w = land.shape
    if not land.any():
        return np.full((h, w), -1, dtype=np.int64)
    far = 4 * (h + w)
    g = np.full((h, w), far, dtype=np.int64)
    for x in range(w):
        d = far
        for y in range(h):
            d = 0 if land[y, x] else min(d + 1, far)
            g[y, x] = d
        d = far
        for y in range(h - 1, -1, -1):
            d = 0 if land[y, x] else min(d + 1, far)
            g[y, x] = min(g[y, x], d)
    xs = np.arange(w, dtype=np.int64)
    dx2 = (xs[:, None] - xs[None, :]) ** 2                           # [x, x']
    return (dx2[None] + (g ** 2)[:, None, :]).min(axis=2)


def ulp_distance_f32(a, b):
    """|a - b| in units of the last place of float32, elementwise, through the order-preserving integer image"""
    def key(v):
        i = np.ascontiguousarray(v, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def batch_ref(arrays, hr_key, lr_keys, items, origins, crop, transforms=None, geo=("lsm", "topo"), with_sdf=True, with_classes=False):
    """the ResidentCutoutLoader batch for host `arrays` (the npz contents): dict of numpy arrays"""
    transforms = transforms or {}
    h, w = crop
    out = {k: crop_transform(arrays[k], items, origins, crop, transforms.get(k)) for k in [hr_key] + list(lr_keys)}
    if "lsm" in geo or with_sdf:
        lsm = crop_transform(arrays["lsm"], items, origins, crop, None, is_mask=True)
        out["lsm_hr"] = lsm
        if "lsm" in geo:
            out["lsm"] = lsm
        if with_sdf:
            out["sdf"] = np.stack([sdf_ref(m[0]) for m in lsm])[:, None].astype(np.float32)
    if "topo" in geo:
        out["topo"] = crop_transform(arrays["topo"], items, origins, crop, transforms.get("topo"))
    if with_classes:
        out["classifier"] = np.asarray(arrays["classifier"])[np.asarray(items)].astype(np.int64)
    o = np.asarray(origins, dtype=np.int64)
    out["hr_points"] = np.stack([o[:, 0], o[:, 0] + h, o[:, 1], o[:, 1] + w], axis=1)
    out["lr_points"] = out["hr_points"].copy()
    return out
