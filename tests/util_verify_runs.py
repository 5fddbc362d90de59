"""Every public function of sbgm_danra_amd/verification.py, and the quantile path of the post-processing kernels
(special_transforms.sample_extremes), on small seeded inputs that reach every branch of the kernels: `run_all()` returns
{key: numpy array} of all outputs, `workspace_sizes()` the five chunked / planned `*_workspace_bytes` queries on a shape table
(host arithmetic, no device).  The outputs are documented as bit-reproducible, so a refactor of the kernels' helpers must
leave every one of them unchanged: tests/golden/verify_parent.npz holds them as the parent commit of that refactor computed
them, and tests/test_gpu_verify_parent.py compares bit for bit.

`python tests/util_verify_runs.py ROOT OUT [COMMIT]` writes that fixture from the package under ROOT: it runs every case twice
and records only the keys whose two runs agree bit for bit (any other is printed with both values and listed under
`unstable_keys`), the workspace sizes under `ws/...`, and COMMIT under `commit`."""
import json
import os
import sys

import numpy as np

N_FIELDS = 3
FIELD_SHAPES = ((5, 7), (8, 12))                  # the scalar tail path (HW % 4 != 0) and the vector path
THRESHOLDS = (-0.4, 0.1, 0.7)
WIDTHS = (1, 3, 15)
WS_SHAPES = ((3, 5, 7), (3, 9, 293), (2, 9, 11), (2, 6, 300), (64, 589, 789), (1000, 589, 789))
WS_CAPS = (256 << 20, 0, 1 << 20, 40 << 20)


def _gen(seed):
    import torch
    return torch.Generator().manual_seed(seed)


def _paired(H, W, seed, n=N_FIELDS):
    """gen [n,H,W] and obs [n,H,W] with NaNs in gen, in obs and one whole gen field of NaN (the last)"""
    import torch
    g = _gen(seed)
    gen, obs = torch.randn(n, H, W, generator=g), torch.randn(n, H, W, generator=g)
    gen[0, 1, 2] = float("nan")
    obs[0, H - 1, W - 1] = float("nan")
    obs[1, 0, 0] = float("nan")
    gen[n - 1] = float("nan")
    return gen, obs


def _masks(n, H, W, seed):
    """the three mask kinds: absent, uint8 per field, one float field"""
    import torch
    g = _gen(seed)
    return {"nomask": None, "u8": (torch.rand(n, H, W, generator=g) < 0.8).to(torch.uint8), "f32": (torch.rand(H, W, generator=g) < 0.8).float()}


def _ensemble(M, H, W, seed, ties=False):
    import torch
    g = _gen(seed)
    ens, obs = torch.randn(M, H, W, generator=g), torch.randn(H, W, generator=g)
    if ties:                                      # one decimal: many members tie with each other and with the truth
        ens, obs = (ens * 2).round() / 2, (obs * 2).round() / 2
    ens[1, 0, 1] = float("nan")
    obs[H - 1, 0] = float("nan")
    mask = (torch.rand(H, W, generator=g) < 0.85).to(torch.uint8)
    return ens, obs, mask


def _precip(n, H, W, seed):
    """non-negative fields with dry background and a few cells, a NaN and exact ties"""
    import torch
    g = _gen(seed)
    x = torch.randn(n, 1, H, W, generator=g)
    x = torch.nn.functional.avg_pool2d(x, 3, stride=1, padding=1)[:, 0]
    x = ((x * 8).clamp_min(0.0) * 4).round() / 4
    x[0, 0, 0] = float("nan")
    return x


def _dev(t):
    return None if t is None else t.cuda()


def _put(out, prefix, res):
    import torch
    if isinstance(res, dict):
        items = res.items()
    elif isinstance(res, (tuple, list)):
        items = ((str(i), r) for i, r in enumerate(res))
    else:
        items = (("out", res),)
    for k, v in items:
        out[f"{prefix}/{k}"] = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


def run_all():
    import torch
    from sbgm_danra_amd import verification as V
    from sbgm_danra_amd.special_transforms import sample_extremes

    out = {}
    # paired fields: error_stats, histogram
    for H, W in FIELD_SHAPES:
        gen, obs = _paired(H, W, 11 * H + W)
        for no in (1, N_FIELDS):
            for mk, mask in _masks(N_FIELDS, H, W, 5).items():
                tag = f"{H}x{W}_obs{no}_{mk}"
                g, o, m = _dev(gen), _dev(obs[:no]), _dev(mask)
                _put(out, f"error_stats/{tag}", V.error_stats(g, o, m))
                _put(out, f"histogram/{tag}", V.histogram(g, 9, -2.0, 2.0, mask=m))
                _put(out, f"histogram_ref/{tag}", V.histogram(g, 9, -2.0, 2.0, ref=o, mask=m))
                _put(out, f"histogram_absdiff/{tag}", V.histogram(g, 300, 0.0, 3.0, ref=o, mask=m, absdiff=True))
    # ensemble_scores: one and two register passes of the pairwise loop, ties broken by the seeded draw
    for M in (5, 19):
        for H, W in FIELD_SHAPES:
            ens, obs, mask = _ensemble(M, H, W, 100 + M, ties=True)
            _put(out, f"ensemble_scores/M{M}_{H}x{W}", V.ensemble_scores(_dev(ens), _dev(obs), _dev(mask), seed=1406))
            _put(out, f"ensemble_scores/M{M}_{H}x{W}_nomask", V.ensemble_scores(_dev(ens), _dev(obs), seed=7))
    # rapsd: three fields, one holding a NaN
    f = torch.randn(3, 8, 12, generator=_gen(3))
    f[1, 2, 3] = float("nan")
    _put(out, "rapsd/8x12", V.rapsd(_dev(f)))
    # neighbourhood_scores: one strip and two strips, every chunking
    T, S = len(THRESHOLDS), len(WIDTHS)
    for H, W in ((5, 7), (9, V.neighbourhood_strip_columns() + 37)):
        gen, obs = _paired(H, W, 7 * H + W)
        one_field = int(N_lib().sbgm_neighbourhood_scores_workspace_bytes(1, H, W, T, S, 1 << 40))
        masks = _masks(N_FIELDS, H, W, 9)
        for (cap_name, cap), no, mk in zip((("default", None), ("zero", 0), ("one_field", one_field)), (N_FIELDS, 1, N_FIELDS),
                                           ("u8", "f32", "nomask")):
            kw = {} if cap is None else {"max_workspace_bytes": cap}
            _put(out, f"neighbourhood_scores/{H}x{W}_{cap_name}_obs{no}_{mk}",
                 V.neighbourhood_scores(_dev(gen), _dev(obs[:no]), THRESHOLDS, WIDTHS, mask=_dev(masks[mk]), **kw))
    # exceedance_scores: all thresholds in one workgroup, and thresholds split over workgroups
    for M in (5, 1500):
        ens, obs, mask = _ensemble(M, 5, 7, 200 + M)
        _put(out, f"exceedance_scores/M{M}", V.exceedance_scores(_dev(ens), _dev(obs), THRESHOLDS, mask=_dev(mask)))
        _put(out, f"exceedance_scores/M{M}_nomask", V.exceedance_scores(_dev(ens), _dev(obs), THRESHOLDS))
    # ensemble_products: one and two quantile launches; members holding both zeros
    for M in (5, 33):
        for qname, qs in (("Q3", (0.0, 0.5, 1.0)), ("Q9", tuple(i / 8 for i in range(9)))):
            for H, W in FIELD_SHAPES:
                ens, _, mask = _ensemble(M, H, W, 300 + M, ties=True)
                ens[0, 2, :] = 0.0
                ens[2, 2, :] = -0.0
                ens[:, 3, 1] = -0.0                   # every member -0
                ens[:, 3, 2] = ens[:, 3, 2].abs().neg()
                ens[M - 1, 3, 2] = -0.0               # -0 is the maximum
                ens[:, 3, 3] = ens[:, 3, 3].abs()
                ens[0, 3, 3] = -0.0                   # -0 is the minimum
                _put(out, f"ensemble_products/M{M}_{qname}_{H}x{W}", V.ensemble_products(_dev(ens), qs, THRESHOLDS, mask=_dev(mask)))
        ens, _, _ = _ensemble(M, 5, 7, 300 + M)
        _put(out, f"ensemble_products/M{M}_noQ", V.ensemble_products(_dev(ens), (), THRESHOLDS))
        _put(out, f"ensemble_products/M{M}_noT", V.ensemble_products(_dev(ens), (0.25,), ()))
    # objects
    for H, W in ((9, 11), (6, 300)):
        x = _precip(2, H, W, 17 * H + W)
        masks = _masks(2, H, W, 13)
        for conn in (4, 8):
            for mk in ("nomask", "u8", "f32"):
                _put(out, f"object_labels/{H}x{W}_c{conn}_{mk}",
                     V.object_labels(_dev(x), 0.5, mask=_dev(masks[mk]), connectivity=conn, return_status=True))
        obs = _precip(2, H, W, 19 * H + W)
        rel = {"factor": 1.0 / 15.0, "quantile": 0.95, "wet": 0.1}
        for cap_name, kw in (("default", {}), ("zero", {"max_workspace_bytes": 0})):
            for no, mk, conn in ((2, "u8", 8), (1, "f32", 4), (2, "nomask", 8)):
                _put(out, f"object_scores/{H}x{W}_{cap_name}_obs{no}_{mk}_c{conn}",
                     V.object_scores(_dev(x), _dev(obs[:no]), (0.5, 2.0), relative=rel, mask=_dev(masks[mk]), connectivity=conn, **kw))
        _put(out, f"object_scores/{H}x{W}_relative_only", V.object_scores(_dev(x), _dev(obs), (), relative=rel))
    # multivariate
    for M in (5, 20):
        for H, W in ((9, 11), (40, 40)):
            ens, obs, mask = _ensemble(M, H, W, 400 + M + H)
            ens[3] = ens[2]                           # duplicated members: an exact 0 distance
            _put(out, f"energy_scores/M{M}_{H}x{W}", V.energy_scores(_dev(ens), _dev(obs), mask=_dev(mask)))
            _put(out, f"energy_scores/M{M}_{H}x{W}_nomask", V.energy_scores(_dev(ens), _dev(obs)))
    for H, W in ((9, 11), (20, 70)):
        ens, obs, mask = _ensemble(5, H, W, 500 + H)
        for radius in (1, 8):
            for i, order in enumerate(V.VARIOGRAM_ORDERS):
                # the weighting only changes the host-built table: both on the small field, alternating on the larger one
                for weights in (V.VARIOGRAM_WEIGHTS if H == 9 else V.VARIOGRAM_WEIGHTS[(i + radius) % 2:][:1]):
                    _put(out, f"variogram_scores/{H}x{W}_r{radius}_p{order}_{weights}",
                         V.variogram_scores(_dev(ens), _dev(obs), radius=radius, order=order, weights=weights, mask=_dev(mask)))
    out["variogram_offsets/r3"] = np.asarray(V.variogram_offsets(3))
    # the post-processing quantile path: radix select on the order-preserving keys, both zeros, a NaN row
    for per in (35, 96, 3000):
        x = (torch.randn(4, per, generator=_gen(per)) * 4).round() / 4
        x[1, : per // 2] = -0.0
        x[1, per // 2:] = 0.0
        x[2, 5] = float("nan")
        for q in (0.5, 0.999, 1.0):
            _put(out, f"sample_extremes/per{per}_q{q}", sample_extremes(_dev(x), q))
    torch.cuda.synchronize()
    return out


def N_lib():
    from sbgm_danra_amd import _native
    return _native.lib()


def workspace_sizes():
    """{key: int64} of the five shape-dependent workspace queries over WS_SHAPES x WS_CAPS (no device needed)"""
    lib, out = N_lib(), {}
    T, S = len(THRESHOLDS), len(WIDTHS)
    for n, H, W in WS_SHAPES:
        for cap in WS_CAPS:
            out[f"ws/neighbourhood/{n}x{H}x{W}_cap{cap}"] = lib.sbgm_neighbourhood_scores_workspace_bytes(n, H, W, T, S, cap)
            for t in (1, T, 17):
                out[f"ws/object/{n}x{H}x{W}_T{t}_cap{cap}"] = lib.sbgm_object_scores_workspace_bytes(n, H, W, t, cap)
        out[f"ws/exceedance/{n}x{H}x{W}"] = lib.sbgm_exceedance_scores_workspace_bytes(n, H * W, T)
        out[f"ws/energy/{n}x{H}x{W}"] = lib.sbgm_energy_scores_workspace_bytes(max(n, 2), H * W)
        for radius in (1, 8):
            out[f"ws/variogram/{n}x{H}x{W}_r{radius}"] = lib.sbgm_variogram_scores_workspace_bytes(max(n, 2), H, W, radius)
    # beyond the limits every query answers 0
    out["ws/neighbourhood/too_large"] = lib.sbgm_neighbourhood_scores_workspace_bytes(1, 2049, 4, T, S, 1 << 30)
    out["ws/object/too_large"] = lib.sbgm_object_scores_workspace_bytes(1, 1024, 1025, 1, 1 << 30)
    out["ws/energy/too_many"] = lib.sbgm_energy_scores_workspace_bytes(4096, 35)
    return {k: np.int64(v) for k, v in out.items()}


def same_bits(a, b):
    """np.array_equal with NaNs (and the sign of zero) compared by bit pattern"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind == "f":
        u = np.dtype(f"u{a.dtype.itemsize}")
        a, b = a.reshape(-1).view(u), b.reshape(-1).view(u)
    return bool(np.array_equal(a, b))


def _pack(arrays):
    """{key: array} -> (index, blob): several hundred small arrays as one byte string, so the archive pays for one entry"""
    index, parts, off = {}, [], 0
    for k, v in arrays.items():
        v = np.asarray(v)
        index[k] = [v.dtype.str, list(v.shape), off]
        parts.append(v.tobytes())                     # C order
        off += v.nbytes
    return json.dumps(index), np.frombuffer(b"".join(parts), dtype=np.uint8)


def load_fixture(path=None):
    """the recorded {key: array}, and the `commit` and `unstable_keys` of the recording"""
    path = path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "verify_parent.npz")
    with np.load(path) as z:
        index, blob = json.loads(str(z["index"])), z["blob"].tobytes()
        meta = {"commit": str(z["commit"]), "unstable_keys": [str(k) for k in z["unstable_keys"]]}
    out = {}
    for k, (dtype, shape, off) in index.items():
        dt = np.dtype(dtype)
        out[k] = np.frombuffer(blob, dtype=dt, count=int(np.prod(shape, dtype=np.int64)), offset=off).reshape(shape)
    return out, meta


def _record(out_path, commit):
    first, second = run_all(), run_all()
    assert first.keys() == second.keys()
    keep, unstable = {}, []
    for k in first:
        if same_bits(first[k], second[k]):
            keep[k] = first[k]
        else:
            unstable.append(k)
            print(f"UNSTABLE {k}:\n  run 1 {first[k]!r}\n  run 2 {second[k]!r}")
    keep.update(workspace_sizes())
    index, blob = _pack(keep)
    np.savez_compressed(out_path, index=np.array(index), blob=blob, unstable_keys=np.array(unstable, dtype=str), commit=np.array(commit))
    print(f"recorded {len(keep)} keys, {len(unstable)} unstable, {os.path.getsize(out_path)} bytes")


if __name__ == "__main__":
    sys.path.insert(0, sys.argv[1])
    _record(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else "")
