"""Host restatement of the full-domain gather (csrc/cutout.hip `sbgm_domain_gather`, resident_data.ResidentDomainLoader), in numpy on top of
the cutout restatement of tests/cutout_ref.py.  TEST INFRASTRUCTURE ONLY.

    domain_gather    out[b][0][y][x] = program(src[item_b][y][min(x, Wd - 1)]): the column is clamped first, then the transform chain of
                     cutout_ref.crop_transform runs on the padded plane (the order the kernel uses); an item outside its stack gives NaN
    batch_ref        the whole batch dict of ResidentDomainLoader for given days
"""
import numpy as np

import cutout_ref as R


def domain_gather(stack, items, Wp, transform=None, is_mask=False):
    """float32 [B, 1, Hd, Wp]: stack [N, Hd, Wd] (items index it) or a plane [Hd, Wd] (items ignored)"""
    stack = np.asarray(stack, dtype=np.float32)
    Hd, Wd = stack.shape[-2:]
    if Wp < Wd:
        raise ValueError(f"padded width {Wp} below the domain width {Wd}")
    cols = np.minimum(np.arange(Wp), Wd - 1)
    padded = np.ascontiguousarray(stack[..., cols])                  # [.., Hd, Wp]: clamp first
    out = np.full((len(items), 1, Hd, Wp), np.nan, dtype=np.float32)
    for b, item in enumerate(items):
        if stack.ndim == 3 and not 0 <= int(item) < stack.shape[0]:
            continue
        out[b] = R.crop_transform(padded, [int(item)], [(0, 0)], (Hd, Wp), transform, is_mask)[0]
    return out


def batch_ref(arrays, hr_key, lr_keys, items, Wp, transforms=None, geo=("lsm", "topo"), with_classes=False):
    """the ResidentDomainLoader batch for host `arrays` (the npz contents): dict of numpy arrays (and the `domain_hw` tuple)"""
    transforms = transforms or {}
    Hd, Wd = arrays[hr_key].shape[-2:]
    out = {k: domain_gather(arrays[k], items, Wp, transforms.get(k)) for k in [hr_key] + list(lr_keys)}
    if "lsm" in geo:
        out["lsm"] = out["lsm_hr"] = domain_gather(arrays["lsm"], items, Wp, None, is_mask=True)
    if "topo" in geo:
        out["topo"] = domain_gather(arrays["topo"], items, Wp, transforms.get("topo"))
    if with_classes:
        out["classifier"] = np.asarray(arrays["classifier"])[np.asarray(items)].astype(np.int64)
    out["hr_points"] = np.tile(np.asarray([0, Hd, 0, Wd], dtype=np.int64), (len(items), 1))
    out["lr_points"] = out["hr_points"].copy()
    out["domain_hw"] = (Hd, Wd)
    return out
