"""numpy / scipy.ndimage restatement of the object-based verification (sbgm_danra_amd.verification.object_labels and
object_scores), shared by test_cpu_objects.py and test_gpu_objects.py.  It states the contract, not the
kernel: the objects come from scipy.ndimage.label (the kernel is a union-find), every sum is a plain fp64 sum of the fp32
values (the kernel adds fixed-point integers) and the order statistics of the relative threshold come from np.sort (the kernel
never sorts).  scipy numbers the components in raster order of their first pixel, which is the rank order of the canonical
labels 1 + min(row * W + col), so partitions compare exactly once scipy's numbers are replaced by the canonical ones."""
import numpy as np
from scipy import ndimage

AREA_BINS = 21
STRUCTURES = {4: np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], bool), 8: np.ones((3, 3), bool)}


def valid_pixels(gen, obs, mask=None):
    """[N,H,W] bool: gen and obs are not NaN and the mask admits the pixel (bool / uint8 != 0, float > 0.5)"""
    gen, obs = np.asarray(gen), np.asarray(obs)
    ok = ~np.isnan(gen) & ~np.isnan(np.broadcast_to(obs, gen.shape))
    if mask is not None:
        mask = np.asarray(mask)
        ok &= np.broadcast_to((mask > 0.5) if mask.dtype.kind == "f" else (mask != 0), gen.shape)
    return ok


def label(objects, connectivity=8):
    """int32 [H,W] canonical labels of a bool image: 1 + the smallest linear index of the pixel's component, 0 for background"""
    objects = np.asarray(objects, bool)
    lab, n = ndimage.label(objects, structure=STRUCTURES[connectivity])
    out = np.zeros(objects.shape, np.int32)
    if n:
        first = np.full(n + 1, objects.size, np.int64)
        np.minimum.at(first, lab.ravel(), np.arange(objects.size))
        out[objects] = (first[lab[objects]] + 1).astype(np.int32)
    return out


def object_labels(fields, threshold, mask=None, connectivity=8):
    """int32 [N,H,W] canonical labels of the valid pixels with fields >= threshold (compared in fp32)"""
    fields = np.asarray(fields, np.float32)
    ok = valid_pixels(fields, fields, mask)
    with np.errstate(invalid="ignore"):
        obj = ok & (fields >= np.float32(threshold))
    return np.stack([label(o, connectivity) for o in obj])


def type7(values, q):
    """Hyndman-Fan type 7 quantile of a 1-D fp32 array as ensemble_products defines it: exact order statistics, h = q (n - 1),
    lo = floor(h), g = h - lo in fp64; x_(lo) when g == 0 or x_(lo) == x_(lo+1), else one fp64 lerp rounded to fp32"""
    srt = np.sort(np.asarray(values, np.float32))
    n = srt.size
    h = np.float64(q) * np.float64(n - 1)
    lo = int(np.floor(h))
    g = np.float64(h - np.floor(h))
    a, b = srt[lo], srt[min(lo + 1, n - 1)]
    if g == 0.0 or a == b:
        return np.float32(a)
    return np.float32(np.float64(a) + g * (np.float64(b) - np.float64(a)))


def relative_threshold(values, factor, quantile, wet):
    """fp32 R* = factor * R^quantile over the values >= wet (fp32 comparison); NaN when there is none"""
    values = np.asarray(values, np.float32)
    wetv = values[values >= np.float32(wet)]
    if wetv.size == 0:
        return np.float32(np.nan)
    return np.float32(np.float64(factor) * np.float64(type7(wetv, quantile)))


def field_objects(F, ok, thr, connectivity=8):
    """the objects of one side of one field.  F fp32 [H,W], ok bool [H,W], thr fp32 (NaN: none).  Returns a dict: labels (int32
    [H,W], canonical) and per object, in ascending label order, area (int64), R, Rmax, row, col (fp64)"""
    F64 = np.where(ok, F, 0).astype(np.float64)
    with np.errstate(invalid="ignore"):
        obj = ok & (F >= np.float32(thr))
    lab = label(obj, connectivity)
    ids, inv = np.unique(lab[obj], return_inverse=True)
    n = ids.size
    rows, cols = np.nonzero(obj)
    v = F64[obj]
    R = np.bincount(inv, weights=v, minlength=n)
    with np.errstate(invalid="ignore", divide="ignore"):
        row = np.bincount(inv, weights=v * rows, minlength=n) / R
        col = np.bincount(inv, weights=v * cols, minlength=n) / R
    Rmax = np.full(n, -np.inf)
    np.maximum.at(Rmax, inv, v)
    return dict(labels=lab, area=np.bincount(inv, minlength=n).astype(np.int64), R=R, Rmax=Rmax, row=row, col=col)


def _ratio(num, den):
    """num / den in fp64, NaN where den is 0"""
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(den == 0, np.nan, np.asarray(num, np.float64) / np.where(den == 0, 1.0, den))


def object_scores(gen, obs, thresholds=(), relative=None, mask=None, connectivity=8):
    """the dict verification.object_scores returns (without `status`), as numpy arrays"""
    gen = np.asarray(gen, np.float32)
    obs = np.broadcast_to(np.asarray(obs, np.float32), gen.shape)
    N, H, W = gen.shape
    fixed = [np.float32(t) for t in thresholds]
    T = len(fixed) + (relative is not None)
    ok = valid_pixels(gen, obs, mask)
    rr, cc = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    d = np.sqrt(np.float64((H - 1) ** 2 + (W - 1) ** 2))
    out = dict(threshold=np.zeros((2, N, T), np.float32), n_objects=np.zeros((2, N, T), np.int64), area=np.zeros((2, N, T), np.int64),
               mass=np.zeros((2, N, T)), V=np.full((2, N, T), np.nan), r=np.full((2, N, T), np.nan), domain_mean=np.full((2, N), np.nan),
               com=np.full((2, N, 2), np.nan), valid=ok.reshape(N, -1).sum(axis=1).astype(np.int64),
               area_hist=np.zeros((2, T, AREA_BINS), np.int64))
    total = np.zeros((2, N))
    for side, fields in enumerate((gen, obs)):
        for f in range(N):
            F, k = fields[f], ok[f]
            F64 = np.where(k, F, 0).astype(np.float64)
            nv = int(k.sum())
            s = F64.sum()
            total[side, f] = s
            if nv:
                out["domain_mean"][side, f] = s / nv
            if nv and s != 0:
                out["com"][side, f] = (F64 * rr).sum() / s, (F64 * cc).sum() / s
            thr = list(fixed)
            if relative is not None:
                thr.append(relative_threshold(F[k], relative["factor"], relative["quantile"], relative["wet"]))
            for t, th in enumerate(thr):
                out["threshold"][side, f, t] = th
                o = field_objects(F, k, th, connectivity)
                n = o["area"].size
                out["n_objects"][side, f, t] = n
                out["area"][side, f, t] = o["area"].sum()
                if not n:
                    continue
                m = o["R"].sum()
                out["mass"][side, f, t] = m
                with np.errstate(invalid="ignore", divide="ignore"):
                    dist = np.sqrt((out["com"][side, f, 0] - o["row"]) ** 2 + (out["com"][side, f, 1] - o["col"]) ** 2)
                    out["V"][side, f, t] = (o["R"] * (o["R"] / o["Rmax"])).sum() / m
                    out["r"][side, f, t] = (o["R"] * dist).sum() / m
                np.add.at(out["area_hist"][side, t], np.floor(np.log2(o["area"])).astype(int), 1)
    Dg, Do = out["domain_mean"]
    field_ok = (out["valid"] > 0) & (total[0] != 0) & (total[1] != 0)
    out["A"] = np.where(field_ok, _ratio(Dg - Do, 0.5 * (Dg + Do)), np.nan)
    out["L1"] = np.where(field_ok, np.sqrt(((out["com"][0] - out["com"][1]) ** 2).sum(axis=1)) / d, np.nan)
    both = (out["n_objects"][0] > 0) & (out["n_objects"][1] > 0)
    Vg, Vo = out["V"]
    out["S"] = np.where(both, _ratio(Vg - Vo, 0.5 * (Vg + Vo)), np.nan)
    out["L2"] = np.where(both, 2.0 * np.abs(out["r"][0] - out["r"][1]) / d, np.nan)
    out["L"] = out["L1"][:, None] + out["L2"]
    return out
