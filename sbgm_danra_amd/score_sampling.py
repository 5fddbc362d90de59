"""Drop-in mirror of the reference's `sbgm/score_sampling.py`: same function names, positional/keyword
signatures and return values; the loops run on the device through libsbgm_hip.so.

* `score_model` is a native `ScoreNet` and classifier-free guidance is off (the only configuration the
  reference CLI reaches): the whole loop — network evaluations, Langevin / Euler-Maruyama
  updates, in-kernel Philox noise — is enqueued by one C call (`sbgm_sampler_run`), optionally as a replayed
  hipGraph of one SDE step.
* otherwise (guidance on, or an arbitrary callable as `score_model`): a Python loop drives the same fused update
  kernels (`sbgm_em_step`, `sbgm_langevin_step`, `sbgm_cfg_combine`) around `score_model` calls.

Extra keyword-only arguments (not in the reference): `noise` — pre-drawn N(0,1) tensors consumed in the
reference's RNG order (init, then per step [corrector,] predictor) for parity runs; `use_graph`; `seed`.
Deviation kept explicit: the reference's Euler-Maruyama sampler ignores `img_size` and always starts from
32x32 (score_sampling.py:94); here `img_size` is honoured (pass 32 to reproduce the reference literally).

Constrained sampling (imputation, Song et al. 2021 App. I.2): `Euler_Maruyama_sampler`, `pc_sampler` and
`edm_heun_sampler` take keyword-only `known` / `known_mask` and hold the masked pixels at `known`, re-noised after every state update to
the level the state is at, in the epilogue of the update kernels; `sde_hold_levels` is the host definition of those levels.

Beyond the reference: `edm_heun_sampler`, a deterministic few-step Heun solver of the probability-flow ODE on the Karras
sigma ladder (Karras et al. 2022, Alg. 2) for the same VE-trained network; `edm_heun_schedule` is its one host definition.
`dpmpp_2m_sampler`, DPM-Solver++(2M) (Lu et al. 2022) on the same ladder: second order at ONE evaluation per step (the previous step's
denoised estimate is the second-order term), with `eta > 0` its SDE variant; `dpmpp_2m_schedule` is its one host definition.
`rk45_sampler`, the adaptive probability-flow ODE solver on the device (Dormand-Prince 5(4) with scipy's RK45 step controller):
conditioned, guided, tileable, in both directions of the flow, with one controller per batch or per sample; `rk45_host_solve` is
its definition in numpy.

Row-keyed, temporally correlated noise: the five samplers above take keyword-only `noise_rows` / `noise_weights` /
`noise_row_stride` (see `pc_sampler`); `temporal_noise_weights`, `temporal_noise_acf` and `temporal_noise` are its host helpers.
"""
from __future__ import annotations

import ctypes as C
import logging
import math

import numpy as np
import torch

from . import _native as N
from .score_unet import ScoreNet, _sigma_of

logger = logging.getLogger(__name__)

signal_to_noise_ratio = 0.16      # reference score_sampling.py:132
error_tolerance = 1e-5            # reference score_sampling.py:238


def _fresh_seed() -> int:
    """64-bit seed drawn from torch's default CPU generator, so torch.manual_seed() makes runs repeatable"""
    return int(torch.empty((), dtype=torch.int64).random_().item()) & 0x7FFFFFFFFFFFFFFF


fresh_seed = _fresh_seed          # for callers outside this module that fix one seed for several sampler calls (generate_series)


def _cfg_enabled(cfg) -> bool:
    return bool((cfg or {}).get("classifier_free_guidance", {}).get("enabled", False))


def guided_score_fn(score_model, x, t, y=None, cond_img=None, lsm_cond=None, topo_cond=None, null_token: int = 0,
                    scale: float = 2.0):
    """Classifier-free guidance (reference score_sampling.py:10-56): (1+w)*s_cond - w*s_uncond, where the
    unconditional branch zeroes cond_img, zeroes only the MASK channel of 2-channel geo conditions and uses the
    null class token.  The two evaluations run through `score_model`; the combine is one fused kernel."""
    def strip_mask(c):
        if c is None or c.shape[1] != 2:
            return c
        c = c.clone()
        c[:, 1, :, :] = 0.0
        return c
    s_c = score_model(x, t, y, cond_img, lsm_cond, topo_cond)
    s_u = score_model(x, t, None if y is None else torch.full_like(y, null_token),
                      None if cond_img is None else torch.zeros_like(cond_img), strip_mask(lsm_cond), strip_mask(topo_cond))
    N.require_device(s_c, s_u)
    s_c, s_u = N.f32c(s_c), N.f32c(s_u)
    out = torch.empty_like(s_c)
    N.check(N.lib().sbgm_cfg_combine(out.data_ptr(), s_c.data_ptr(), s_u.data_ptr(), float(scale), out.numel(), N.stream()))
    return out


def _score(score_model, cfg, x, t, y, cond_img, lsm_cond, topo_cond, clamp=False):
    if _cfg_enabled(cfg):
        g = cfg["classifier_free_guidance"]
        scale = g.get("guidance_scale", 2.0)
        if clamp and g.get("guidance_scale_max") is not None and scale > g["guidance_scale_max"]:
            scale = g["guidance_scale_max"]                                            # reference :184-186
        return guided_score_fn(score_model, x, t, y, cond_img, lsm_cond, topo_cond, scale=scale)
    return score_model(x, t, y, cond_img, lsm_cond, topo_cond)


def _guidance(cfg):
    """(enabled, predictor scale, corrector scale): the reference clamps only the corrector's scale to
    guidance_scale_max (score_sampling.py:184-186 vs :213)."""
    if not _cfg_enabled(cfg):
        return 0, 0.0, 0.0
    g = cfg["classifier_free_guidance"]
    scale = float(g.get("guidance_scale", 2.0))
    corr = scale
    if g.get("guidance_scale_max") is not None and corr > g["guidance_scale_max"]:
        corr = float(g["guidance_scale_max"])
    return 1, scale, corr


def _counts(kind, num_steps, churn=False):
    """(network evaluations per step, noise draws of a run) of a sampler kind: draw 0 is the initial state; then one draw per
    evaluation of an SDE step (PC: corrector and predictor), or one per EDM Heun step with churn / per 2M step with eta > 0 (`churn`)"""
    if kind == N.SAMPLER_EDM_HEUN:
        return 2, 1 + (int(num_steps) if churn else 0)
    if kind == N.SAMPLER_DPMPP_2M:
        return 1, 1 + (int(num_steps) if churn else 0)
    if kind == N.SAMPLER_RK45:                                # six evaluations per attempt; the only draw is the start
        return 6, 1
    per_step = 2 if kind == N.SAMPLER_PC else 1
    return per_step, 1 + int(num_steps) * per_step


def _prep_known(known, known_mask, batch_size, hw, device, who):
    """(known, known_mask) as contiguous fp32 [B,1,H,W] device tensors, or (None, None).  known: [B,1,H,W] or [B,H,W]; known_mask also
    [H,W] or [1,1,H,W] (one mask for the whole batch).  Shapes are checked, values are not (no device sync): the kernels clamp the mask."""
    if known is None and known_mask is None:
        return None, None
    if known is None or known_mask is None:
        raise ValueError(f"{who}: known and known_mask must be given together")
    B, full = int(batch_size), (int(batch_size), 1, int(hw), int(hw))
    dev = torch.device(device) if not isinstance(device, torch.device) else device

    def view_of(t, name, shared):                          # the shape to view `t` as before it is expanded over the batch
        ok = {full: full, (B, hw, hw): full}
        if shared:
            ok.update({(hw, hw): (1, 1, hw, hw), (1, 1, hw, hw): (1, 1, hw, hw)})
        if tuple(t.shape) not in ok:
            raise ValueError(f"{who}: {name} has shape {tuple(t.shape)}, expected one of {sorted(ok, key=len)}")
        return ok[tuple(t.shape)]
    known, known_mask = torch.as_tensor(known), torch.as_tensor(known_mask)
    views = view_of(known, "known", False), view_of(known_mask, "known_mask", True)        # both checked before anything moves
    return tuple(N.f32c(t.to(dev).reshape(v).expand(full)) for t, v in zip((known, known_mask), views))


def _held_start(x, known, mask):
    """x0 = scale z0 + m known of a constrained run (the native loop's init kernel), for the Python loops"""
    m = mask.clamp(0.0, 1.0)
    return torch.where(m > 0, x + m * known, x)


def sde_hold_levels(kind, num_steps, sigma_sde=25.0, eps=1e-3):
    """Noise levels a constrained Euler-Maruyama (`kind="em"`) or predictor-corrector (`kind="pc"`) run re-noises its held pixels to,
    as the engine builds them beside its step table: `t` [N] the table's fp32 times (torch.linspace in fp32 for EM, np.linspace in
    float64 rounded to fp32 for PC), `s_cur` [N] = fp32(marginal_prob_std(t_i)) evaluated in float64 (floored at 1e-5 like the model's) --
    the corrector's level -- and `s_next` [N] = s_cur shifted by one step with a final 0 -- the predictor's level."""
    if kind in ("em", N.SAMPLER_EM):
        t = torch.linspace(1.0, eps, int(num_steps)).numpy().astype(np.float64)
    elif kind in ("pc", N.SAMPLER_PC):
        t = np.linspace(1.0, eps, int(num_steps)).astype(np.float32).astype(np.float64)
    else:
        raise ValueError(f"sde_hold_levels: kind={kind!r} must be 'em' or 'pc'")
    s_cur = np.maximum(_ve_std(t, sigma_sde), 1e-5).astype(np.float32)
    return {"t": t, "s_cur": s_cur, "s_next": np.append(s_cur[1:], np.float32(0.0))}


def _prep_joint(joint_tiles, tile_origins, noise, who):
    """`joint_tiles` as (domain_height, ramp_len) ints, or None; the argument checks of a joint run that need no device"""
    if joint_tiles is None:
        return None
    try:
        domain_height, ramp_len = (int(v) for v in joint_tiles)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: joint_tiles must be (domain_height, ramp_len), got {joint_tiles!r}") from None
    if tile_origins is None:
        raise ValueError(f"{who}: joint_tiles needs tile_origins (the batch must be all tiles of one domain)")
    if noise is not None:
        raise ValueError(f"{who}: joint_tiles draws domain-keyed in-kernel noise; it cannot be combined with injected noise")
    if domain_height < 1 or ramp_len < 1:
        raise ValueError(f"{who}: joint_tiles = (domain_height, ramp_len) = ({domain_height}, {ramp_len}) must both be >= 1")
    return domain_height, ramp_len


NOISE_MAX_LAGS = 32               # include/sbgm_hip.h: sbgm_sampler_set_noise_rows


def temporal_noise_weights(rho, lags):
    """float32 [lags] weights w_k proportional to rho^k with sum w_k^2 = 1 (normalised in float64): the moving average that makes the
    noise of consecutive rows correlated like a truncated AR(1) of coefficient `rho`.  -1 < rho < 1, 1 <= lags <= 32; rho = 0 or
    lags = 1 gives [1.0], white noise."""
    rho, lags = float(rho), int(lags)
    if not -1.0 < rho < 1.0:
        raise ValueError(f"temporal_noise_weights: rho={rho!r} must lie in (-1, 1)")
    if not 1 <= lags <= NOISE_MAX_LAGS:
        raise ValueError(f"temporal_noise_weights: lags={lags!r} must lie in 1..{NOISE_MAX_LAGS}")
    w = rho ** np.arange(lags, dtype=np.float64)
    return (w / np.sqrt((w * w).sum())).astype(np.float32)


def temporal_noise_acf(weights):
    """float64 [K]: acf[j] = sum_k w_k w_{k+j}, the lag-j autocorrelation of every draw under the weights (acf[0] = sum w^2)"""
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    return np.array([float(np.dot(w[:w.size - j], w[j:])) for j in range(w.size)], dtype=np.float64)


def noise_weights_f32(weights, who="noise_weights"):
    """`weights` as the float32 [K] array a noise plan carries, checked: 1 <= K <= 32 and |sum w^2 - 1| <= 1e-5 in float64 on the float32
    values.  `who` names the argument or config key in the ValueError.  The one definition for the samplers and the series config."""
    try:
        w64 = np.asarray([float(v) for v in np.asarray(weights).reshape(-1)], dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{who} must be a list of numbers, got {weights!r}") from None
    if not 1 <= w64.size <= NOISE_MAX_LAGS:
        raise ValueError(f"{who} holds {w64.size} lags, must be 1..{NOISE_MAX_LAGS}")
    w = w64.astype(np.float32)
    ss = float((w.astype(np.float64) ** 2).sum())
    if not abs(ss - 1.0) <= 1e-5:
        raise ValueError(f"{who} must have sum of squares 1 (every draw stays N(0,1)), got {ss!r}")
    return w


def _prep_noise_rows(noise_rows, noise_weights, noise_row_stride, batch_size, who, noise=None, tile_origins=None, joint_tiles=None):
    """The noise plan of a run as (rows int64 numpy [B], stride, weights float32 numpy [K]), or None; every check needs the host only."""
    if noise_rows is None:
        if noise_weights is not None and [float(v) for v in np.asarray(noise_weights).reshape(-1)] != [1.0]:
            raise ValueError(f"{who}: noise_weights needs noise_rows (the rows the weights mix)")
        if int(noise_row_stride) != 1:
            raise ValueError(f"{who}: noise_row_stride needs noise_rows")
        return None
    for other, name in ((noise, "noise"), (tile_origins, "tile_origins"), (joint_tiles, "joint_tiles")):
        if other is not None:
            raise ValueError(f"{who}: noise_rows keys and mixes the in-kernel noise; it cannot be combined with {name}")
    w = noise_weights_f32([1.0] if noise_weights is None else noise_weights, f"{who}: noise_weights")
    stride = int(noise_row_stride)
    if stride < 1:
        raise ValueError(f"{who}: noise_row_stride={noise_row_stride!r} must be >= 1")
    rows = noise_rows.detach().cpu().numpy() if torch.is_tensor(noise_rows) else np.asarray(noise_rows)
    if rows.ndim != 1 or rows.shape[0] != int(batch_size) or rows.dtype.kind not in "iu":
        raise ValueError(f"{who}: noise_rows must be {int(batch_size)} integers (one row per sample), got shape {tuple(rows.shape)} "
                         f"of {rows.dtype}")
    rows = rows.astype(np.int64)
    if (rows < 0).any():
        raise ValueError(f"{who}: noise_rows must be >= 0, got {int(rows.min())}")
    if (rows < (w.size - 1) * stride).any():
        raise ValueError(f"{who}: noise_rows must be >= (lags - 1) * noise_row_stride = {(w.size - 1) * stride} (row {int(rows.min())} "
                         f"would reach below row 0)")
    if (rows > 0x7FFFFFFF).any():
        raise ValueError(f"{who}: noise_rows must fit int32, got {int(rows.max())}")
    return rows, stride, w


def _prep_noise_domain(noise_domain_row, domain_height, noise_weights, noise_row_stride, img_size, who, noise=None, tile_origins=None,
                       joint_tiles=None, noise_rows=None):
    """The domain noise plan of a tiled run as (row, stride, weights float32 numpy [K], domain_height), or None; every check needs the host
    only (that the tiles lie inside the domain is checked by the native call, which reads the tile table)."""
    if noise_domain_row is None:
        if domain_height is not None:
            raise ValueError(f"{who}: domain_height needs noise_domain_row (it is the height the domain noise row is drawn over)")
        return None
    if noise_rows is not None:
        raise ValueError(f"{who}: noise_domain_row (one row for all tiles of a domain) and noise_rows (one row per sample) exclude each other")
    if noise is not None:
        raise ValueError(f"{who}: noise_domain_row keys and mixes the in-kernel noise; it cannot be combined with noise")
    if tile_origins is None:
        raise ValueError(f"{who}: noise_domain_row needs tile_origins (it is the noise row of all tiles of one domain)")
    if isinstance(noise_domain_row, (bool, float)) or not isinstance(noise_domain_row, (int, np.integer)):
        raise ValueError(f"{who}: noise_domain_row must be one integer (the row of the whole batch), got {noise_domain_row!r}")
    row = int(noise_domain_row)
    if domain_height is None and joint_tiles is not None:
        domain_height = joint_tiles[0]
    if domain_height is None or isinstance(domain_height, (bool, float)) or not isinstance(domain_height, (int, np.integer)):
        raise ValueError(f"{who}: domain_height must be given with noise_domain_row as an integer (rows of the domain), got {domain_height!r}")
    domain_height = int(domain_height)
    if domain_height < int(img_size):
        raise ValueError(f"{who}: domain_height={domain_height} must be >= img_size={int(img_size)} (every tile lies inside the domain)")
    if joint_tiles is not None and int(joint_tiles[0]) != domain_height:
        raise ValueError(f"{who}: domain_height={domain_height} differs from the joint run's domain height {int(joint_tiles[0])}")
    w = noise_weights_f32([1.0] if noise_weights is None else noise_weights, f"{who}: noise_weights")
    stride = int(noise_row_stride)
    if stride < 1:
        raise ValueError(f"{who}: noise_row_stride={noise_row_stride!r} must be >= 1")
    if row < 0:
        raise ValueError(f"{who}: noise_domain_row must be >= 0, got {row}")
    if row < (w.size - 1) * stride:
        raise ValueError(f"{who}: noise_domain_row must be >= (lags - 1) * noise_row_stride = {(w.size - 1) * stride} (row {row} would "
                         f"reach below row 0)")
    if row > 0x7FFFFFFF:
        raise ValueError(f"{who}: noise_domain_row must fit int32, got {row}")
    return row, stride, w, domain_height


def _prep_noise_plan(noise_rows, noise_weights, noise_row_stride, batch_size, who, noise, tile_origins, joint_tiles, noise_domain_row,
                     domain_height, img_size):
    """The run's noise plan: the rows plan of `_prep_noise_rows` (3 entries), the domain plan of `_prep_noise_domain` (4), or None"""
    domain = _prep_noise_domain(noise_domain_row, domain_height, noise_weights, noise_row_stride, img_size, who, noise, tile_origins,
                                joint_tiles, noise_rows)
    if domain is not None:
        return domain
    return _prep_noise_rows(noise_rows, noise_weights, noise_row_stride, batch_size, who, noise, tile_origins, joint_tiles)


def _weights_arg(w):
    return (C.c_float * len(w))(*[float(v) for v in w])


def temporal_noise_domain(seed, draw, row, origins, tile, domain_hw, weights=(1.0,), stride=1, scale=1.0, device="cuda"):
    """scale * the mixed draw `draw` of the stream `seed` for the domain noise row `row`, cut into tiles: fp32 [T, tile, tile] on the
    device, what a tiled sampler run with `tile_origins=origins, domain_width=domain_hw[1], noise_domain_row=row, domain_height=
    domain_hw[0], noise_weights=weights, noise_row_stride=stride` uses as its draw `draw` (`sbgm_randn_domain_rows`).  `origins`:
    T pairs (y0, x0), x0 % 4 == 0 (a sequence, or an int tensor [T, 2]); `domain_hw`: (height, padded width)."""
    org = origins.detach().cpu().numpy() if torch.is_tensor(origins) else np.asarray(origins)
    if org.ndim != 2 or org.shape[1] != 2 or org.shape[0] < 1 or org.dtype.kind not in "iu":
        raise ValueError(f"temporal_noise_domain: origins must be T >= 1 integer pairs (y0, x0), got shape {tuple(org.shape)} of {org.dtype}")
    org = org.astype(np.int64)
    tile = int(tile)
    if tile < 4 or tile % 4:
        raise ValueError(f"temporal_noise_domain: tile={tile} must be a positive multiple of 4")
    try:
        dom_h, dom_w = (int(v) for v in domain_hw)
    except (TypeError, ValueError):
        raise ValueError(f"temporal_noise_domain: domain_hw must be (domain_height, domain_width), got {domain_hw!r}") from None
    if dom_h < tile or dom_w < tile:
        raise ValueError(f"temporal_noise_domain: domain_hw=({dom_h}, {dom_w}) must hold a tile of {tile} x {tile}")
    if (org < 0).any() or (org[:, 1] % 4).any() or (org[:, 0] + tile > dom_h).any() or (org[:, 1] + tile > dom_w).any():
        raise ValueError(f"temporal_noise_domain: origins must lie quad-aligned (x0 % 4 == 0) with their tiles inside the {dom_h} x {dom_w} "
                         f"domain, got {org.tolist()}")
    row, stride, w, _ = _prep_noise_domain(row, dom_h, weights, stride, tile, "temporal_noise_domain", tile_origins=org)
    dev = torch.device(device) if not isinstance(device, torch.device) else device
    if dev.type != "cuda":
        raise N.NativeError(f"temporal_noise_domain runs on a ROCm device, got device={device!r}")
    with torch.cuda.device(dev):
        r_dev = torch.tensor([row], dtype=torch.int32, device=dev)
        o_dev = torch.from_numpy(org.astype(np.int32)).to(dev).contiguous()
        x = torch.empty(org.shape[0], tile, tile, device=dev)
        N.check(N.lib().sbgm_randn_domain_rows(x.data_ptr(), float(scale), int(seed), int(draw), r_dev.data_ptr(), o_dev.data_ptr(),
                                               org.shape[0], tile, tile, dom_h, dom_w, stride, _weights_arg(w), len(w), N.stream()))
    return x


def temporal_noise(seed, draw, rows, per_sample, weights=(1.0,), stride=1, device="cuda", scale=1.0):
    """scale * the mixed draw `draw` of the stream `seed` for the noise rows `rows`: fp32 [len(rows), per_sample] on the device, what a
    sampler with `noise_rows=rows, noise_weights=weights, noise_row_stride=stride` uses as its draw `draw` (`sbgm_randn_rows`)."""
    n_rows = int(rows.shape[0]) if hasattr(rows, "shape") else len(rows)
    plan = _prep_noise_rows(rows, weights, stride, n_rows, "temporal_noise")
    per_sample = int(per_sample)
    if per_sample < 4 or per_sample % 4:
        raise ValueError(f"temporal_noise: per_sample={per_sample} must be a positive multiple of 4")
    dev = torch.device(device) if not isinstance(device, torch.device) else device
    if dev.type != "cuda":
        raise N.NativeError(f"temporal_noise runs on a ROCm device, got device={device!r}")
    r, stride, w = plan
    with torch.cuda.device(dev):
        r_dev = torch.from_numpy(r.astype(np.int32)).to(dev)
        x = torch.empty(n_rows, per_sample, device=dev)
        N.check(N.lib().sbgm_randn_rows(x.data_ptr(), float(scale), int(seed), int(draw), r_dev.data_ptr(), n_rows, per_sample, stride,
                                        _weights_arg(w), len(w), N.stream()))
    return x


class _noise_plan:
    """The handle's noise plan around ONE native sampler call: set from `plan` (None: nothing to do) and cleared again whatever happens.
    The rows live in a device buffer the engine keeps per batch size, so the captured step's key sees one address from call to call."""
    def __init__(self, eng, plan, dev):
        self.eng, self.plan, self.dev = eng, plan, dev

    def __enter__(self):
        if self.plan is None:
            return self
        bufs = getattr(self.eng, "_noise_rows", None)
        if bufs is None:
            bufs = self.eng._noise_rows = {}
        index = self.dev.index if self.dev.index is not None else torch.cuda.current_device()     # "cuda" is the current device
        if len(self.plan) == 4:                          # the domain plan: ONE row at one address, whatever the day and the batch
            row, stride, w, domain_h = self.plan
            buf = bufs.get((index, "domain"))
            if buf is None:
                buf = bufs[(index, "domain")] = torch.empty(1, dtype=torch.int32, device=torch.device("cuda", index))
            buf.copy_(torch.tensor([row], dtype=torch.int32))
            N.check(self.eng.lib.sbgm_sampler_set_noise_domain_row(self.eng.h, buf.data_ptr(), domain_h, stride, _weights_arg(w), len(w)))
            return self
        rows, stride, w = self.plan
        buf = bufs.get((index, rows.size))
        if buf is None:
            buf = bufs[(index, rows.size)] = torch.empty(rows.size, dtype=torch.int32, device=torch.device("cuda", index))
        buf.copy_(torch.from_numpy(rows.astype(np.int32)))
        N.check(self.eng.lib.sbgm_sampler_set_noise_rows(self.eng.h, buf.data_ptr(), stride, _weights_arg(w), len(w)))
        return self

    def __exit__(self, *exc):
        if self.plan is not None:
            N.check(self.eng.lib.sbgm_sampler_set_noise_rows(self.eng.h, None, 1, None, 0))
        return False


def _native_run(kind, score_model: ScoreNet, batch_size, num_steps, snr, eps, hw, y, cond_img, lsm_cond, topo_cond,
                noise, use_graph, seed, device, cfg=None, tile_origins=None, domain_width=0, edm_args=None, held=(None, None),
                joint=None, dpm_args=None, plan=None):
    dev = torch.device(device) if not isinstance(device, torch.device) else device
    if dev.type != "cuda":
        raise N.NativeError(f"the native samplers run on a ROCm device, got device={device!r}")
    x_dummy = torch.empty(batch_size, 1, hw, hw, device=dev)
    t_dummy = torch.empty(batch_size, device=dev)
    _, _, y, cond_img, lsm_cond, topo_cond = score_model._prep(x_dummy, t_dummy, y, cond_img, lsm_cond, topo_cond)
    eng = score_model._engine(lsm_cond, topo_cond, cond_img)
    out = torch.empty(batch_size, 1, hw, hw, device=dev)
    nz = None
    if noise is not None:
        nz = noise if torch.is_tensor(noise) else torch.stack(list(noise))
        stochastic = edm_args[3] > 0 if edm_args is not None else dpm_args is not None and dpm_args[3] > 0   # s_churn / eta
        need = _counts(kind, num_steps, stochastic)[1]
        if nz.shape[0] < need:
            raise ValueError(f"noise holds {nz.shape[0]} draws, the sampler consumes {need}")
        nz = N.f32c(nz.to(dev))
    a = N.SamplerArgs(kind, batch_size, hw, hw, int(num_steps), float(eps), float(snr), int(seed), int(bool(use_graph)),
                      int(score_model.training), N.ptr(y), N.ptr(cond_img), N.ptr(lsm_cond), N.ptr(topo_cond), N.ptr(nz),
                      out.data_ptr(), *_guidance(cfg), N.ptr(tile_origins), int(domain_width or 0))
    if tile_origins is not None:
        N.require_device(tile_origins)
        if tile_origins.dtype != torch.int32 or tuple(tile_origins.shape) != (batch_size, 2) or not tile_origins.is_contiguous():
            raise ValueError("tile_origins must be a contiguous int32 [batch, 2] device tensor of (y0, x0)")
        if noise is not None:
            raise ValueError("tile_origins keys the in-kernel noise; it cannot be combined with injected noise")
    known, mask = held
    with _noise_plan(eng, plan, dev):                      # set and cleared around the one native call
        if dpm_args is not None:                           # one entry point: the constraint and the joint blend are optional arguments
            N.check(eng.lib.sbgm_sampler_run_dpmpp(eng.h, C.byref(a), *dpm_args, N.ptr(known), N.ptr(mask), *(joint or (0, 0)), N.stream()))
            return out
        if joint is not None:                              # one diffusion over the domain: the tiles' scores are blended at every step
            if edm_args is not None:
                N.check(eng.lib.sbgm_sampler_run_edm_joint(eng.h, C.byref(a), *edm_args, *joint, N.ptr(known), N.ptr(mask), N.stream()))
            else:
                N.check(eng.lib.sbgm_sampler_run_joint(eng.h, C.byref(a), *joint, N.ptr(known), N.ptr(mask), N.stream()))
            return out
        if edm_args is not None:
            if known is not None:
                N.check(eng.lib.sbgm_sampler_run_edm_held(eng.h, C.byref(a), *edm_args, known.data_ptr(), mask.data_ptr(), N.stream()))
            else:
                N.check(eng.lib.sbgm_sampler_run_edm(eng.h, C.byref(a), *edm_args, N.stream()))
            return out
        if known is not None:
            N.check(eng.lib.sbgm_sampler_run_held(eng.h, C.byref(a), known.data_ptr(), mask.data_ptr(), N.stream()))
        else:
            N.check(eng.lib.sbgm_sampler_run(eng.h, C.byref(a), N.stream()))
    if score_model.training:
        eng.download_bn_stats(score_model, n_forwards=int(num_steps) * _counts(kind, num_steps)[0])
    return out


def _host_start(kind, batch_size, num_steps, img_size, device, noise, seed, scale, tile_origins, churn=False, joint=None, plan=None):
    """Setup of the host-driven loops: refuses `tile_origins` and `joint_tiles`, checks that `noise` holds the run's draws, and returns the initial
    x = scale * (draw 0) and z(i), the i-th noise draw (None: the kernels draw in-kernel Philox noise)."""
    if joint is not None:
        raise N.NativeError("joint tiled sampling (joint_tiles) needs the native sampler loop (a ScoreNet in eval mode)")
    if tile_origins is not None:
        raise N.NativeError("domain-keyed noise (tile_origins) needs the native sampler loop (a ScoreNet in eval mode)")
    if plan is not None:
        raise N.NativeError("row-keyed noise (noise_rows) needs the native sampler loop (a ScoreNet in eval mode)")
    if noise is not None:
        noise = noise if torch.is_tensor(noise) else list(noise)
        need = _counts(kind, num_steps, churn)[1]
        if len(noise) < need:
            raise ValueError(f"noise holds {len(noise)} draws, the sampler consumes {need}")
    x = torch.empty(batch_size, 1, img_size, img_size, device=device)
    if noise is None:
        N.check(N.lib().sbgm_randn_scaled(x.data_ptr(), scale, seed, 0, x.numel(), N.stream()))
    else:
        x.copy_(noise[0].to(x) * scale)
    return x, lambda i: None if noise is None else N.f32c(noise[i].to(x))


def Euler_Maruyama_sampler(score_model, marginal_prob_std, diffusion_coeff, batch_size=64, num_steps=500, device="cuda",
                           eps=1e-3, img_size=64, y=None, cond_img=None, lsm_cond=None, topo_cond=None, cfg=None, *,
                           noise=None, use_graph=True, seed=None, tile_origins=None, domain_width=0, known=None, known_mask=None,
                           joint_tiles=None, noise_rows=None, noise_weights=None, noise_row_stride=1, noise_domain_row=None,
                           domain_height=None):
    """Euler-Maruyama reverse-SDE sampler (reference score_sampling.py:63-127).  Returns the last `mean_x`.
    `known` / `known_mask` (not in the reference): hold the masked pixels at `known`, see `pc_sampler`; `joint_tiles`: see `pc_sampler`;
    `noise_rows` / `noise_weights` / `noise_row_stride` (row-keyed, temporally correlated noise) and `noise_domain_row` /
    `domain_height` (the same for tiled runs): see `pc_sampler`."""
    seed = _fresh_seed() if seed is None else seed
    joint = _prep_joint(joint_tiles, tile_origins, noise, "Euler_Maruyama_sampler")
    plan = _prep_noise_plan(noise_rows, noise_weights, noise_row_stride, batch_size, "Euler_Maruyama_sampler", noise, tile_origins, joint_tiles,
                            noise_domain_row, domain_height, img_size)
    known, known_mask = _prep_known(known, known_mask, batch_size, img_size, device, "Euler_Maruyama_sampler")
    if isinstance(score_model, ScoreNet) and not (_cfg_enabled(cfg) and score_model.training):
        return _native_run(N.SAMPLER_EM, score_model, batch_size, num_steps, 0.0, eps, img_size, y, cond_img, lsm_cond,
                           topo_cond, noise, use_graph, seed, device, cfg, tile_origins, domain_width, held=(known, known_mask),
                           joint=joint, plan=plan)
    lib, st = N.lib(), N.stream
    ones = torch.ones(batch_size, device=device)
    x, z = _host_start(N.SAMPLER_EM, batch_size, num_steps, img_size, device, noise, seed, float(marginal_prob_std(ones)[0]),
                       tile_origins, joint=joint, plan=plan)
    time_steps = torch.linspace(1.0, eps, num_steps, device=device)
    step_size = float(time_steps[0] - time_steps[1])
    mean_x = torch.empty_like(x)
    if known is not None:
        x = _held_start(x, known, known_mask)
        s_next = sde_hold_levels("em", num_steps, _sigma_of(marginal_prob_std), eps)["s_next"]
    with torch.no_grad():
        for draw, ts in enumerate(time_steps.tolist(), 1):
            bt = ones * ts
            g = float(diffusion_coeff(bt)[0])
            score = N.f32c(_score(score_model, cfg, x, bt, y, cond_img, lsm_cond, topo_cond))
            N.check(lib.sbgm_em_step(x.data_ptr(), mean_x.data_ptr(), score.data_ptr(), N.ptr(z(draw)), g * g, step_size,
                                     math.sqrt(step_size) * g, seed, draw, x.numel(), st()))
            if known is not None:
                N.check(lib.sbgm_hold_known(x.data_ptr(), mean_x.data_ptr(), known.data_ptr(), known_mask.data_ptr(), N.ptr(z(draw)),
                                            float(s_next[draw - 1]), seed, draw, x.numel(), st()))
    return mean_x


def pc_sampler(score_model, marginal_prob_std, diffusion_coeff, batch_size=64, num_steps=800, snr=signal_to_noise_ratio,
               device="cuda", eps=1e-3, img_size=64, y=None, cond_img=None, lsm_cond=None, topo_cond=None, cfg=None, *,
               noise=None, use_graph=True, seed=None, tile_origins=None, domain_width=0, known=None, known_mask=None,
               joint_tiles=None, noise_rows=None, noise_weights=None, noise_row_stride=1, noise_domain_row=None, domain_height=None):
    """Predictor-corrector sampler: Langevin corrector with the batch-mean gradient norm, then an Euler-Maruyama
    predictor (reference score_sampling.py:136-230).  Returns the last `x_mean`.

    Constrained sampling (not in the reference; Song et al. 2021, App. I.2): `known` [B,1,H,W] or [B,H,W], model space, and `known_mask`
    of the same shape, or [H,W] / [1,1,H,W] for one mask shared by the batch, values in [0,1] (clamped on the device; CPU tensors are
    moved).  Pixels with mask 1 are held: after every state update they are overwritten with `known` plus noise of the level the state
    is at (reusing that update's own draw: no extra draw, `noise=` keeps its layout), so the result equals `known` there bit for bit and
    the free pixels are sampled consistently with them.  Mask 0 leaves a pixel exactly as without the arguments (`known` may be NaN
    there); values in between blend.  Both or neither must be given (ValueError).

    Joint full-domain sampling (not in the reference; Mixture of Diffusers / MultiDiffusion): `joint_tiles=(domain_height, ramp_len)` with
    `tile_origins` and `domain_width` declares the batch to be ALL tiles of one domain and runs ONE diffusion over it: wherever an update
    reads a tile's score it reads the stitch-weighted blend of every tile's score at that domain pixel (ramps of `ramp_len` pixels, as
    `FullDomainTiler.stitch`), and the corrector's step size is the batch-mean rule over the tiles.  All copies of a domain pixel then
    stay bit-equal through the run, so stitching the result averages nothing.  Needs the native loop and in-kernel noise; composes with
    `known` / `known_mask` and guidance.  `FullDomainTiler.sample(..., joint=True)` sets it up.

    Row-keyed, temporally correlated noise (not in the reference): `noise_rows` (sequence or int tensor [batch_size])
    gives sample b the noise row r_b, and every in-kernel draw of the run becomes z = sum_k w_k xi(r_b - k * noise_row_stride) over the K
    `noise_weights` (default [1.0]; their squares must sum to 1 within 1e-5, K <= 32, every r_b >= (K-1) * noise_row_stride), xi(r) the
    white draw of row r, i.e. what a run without the arguments draws for its sample r.  Every draw a sample sees is still N(0,1),
    independent across pixels and steps, so each sample is a sample of this sampler as it is; samples whose rows are j strides apart are
    correlated with `temporal_noise_acf(noise_weights)[j]`, and a sample's noise depends on (seed, row) only, not on its place in the
    batch (this sampler's Langevin step size still uses the batch-mean score norm).  Rows 0..B-1 with the default weights reproduce the
    run without the arguments bit for bit.  Needs the native loop; refused (ValueError) with `noise`, `tile_origins` or `joint_tiles`;
    composes with `known` / `known_mask` and guidance.  `temporal_noise_weights(rho, lags)` makes AR(1)-like weights.

    The same for a tiled or joint run: `noise_domain_row=R` (one int: all tiles of the batch are one field on one
    day) with `domain_height`, `tile_origins`, `domain_width` and the same `noise_weights` / `noise_row_stride`.  The white draw of lag k
    at domain row Y, quad column X4 has the counter (R - k stride) Q + Y dom_w4 + X4, Q = domain_height * ceil(domain_width / 4): R = 0
    with the default weights is the tiled run without the arguments bit for bit, one tile that covers the domain draws what
    `noise_rows=[R]` draws, and the copies of a domain pixel still share their draw.  Every tile must lie inside domain_height x
    domain_width (checked by the native call).  Refused (ValueError) with `noise_rows`, `noise`, or without `tile_origins`;
    `FullDomainTiler.sample(noise_row=...)` and `.sample_series` set it up; `temporal_noise_domain` is the draw itself."""
    seed = _fresh_seed() if seed is None else seed
    joint = _prep_joint(joint_tiles, tile_origins, noise, "pc_sampler")
    plan = _prep_noise_plan(noise_rows, noise_weights, noise_row_stride, batch_size, "pc_sampler", noise, tile_origins, joint_tiles,
                            noise_domain_row, domain_height, img_size)
    known, known_mask = _prep_known(known, known_mask, batch_size, img_size, device, "pc_sampler")
    if isinstance(score_model, ScoreNet) and not (_cfg_enabled(cfg) and score_model.training):
        return _native_run(N.SAMPLER_PC, score_model, batch_size, num_steps, snr, eps, img_size, y, cond_img, lsm_cond,
                           topo_cond, noise, use_graph, seed, device, cfg, tile_origins, domain_width, held=(known, known_mask),
                           joint=joint, plan=plan)
    lib, st = N.lib(), N.stream
    ones = torch.ones(batch_size, device=device)
    x, z = _host_start(N.SAMPLER_PC, batch_size, num_steps, img_size, device, noise, seed, float(marginal_prob_std(ones)[0]),
                       tile_origins, joint=joint, plan=plan)
    time_steps = np.linspace(1.0, eps, num_steps)
    step_size = float(time_steps[0] - time_steps[1])
    x_mean = torch.empty_like(x)
    sumsq = torch.empty(batch_size, dtype=torch.float64, device=device)
    per = x[0].numel()
    snr_nn = float(snr * np.sqrt(per))
    if known is not None:
        x = _held_start(x, known, known_mask)
        lv = sde_hold_levels("pc", num_steps, _sigma_of(marginal_prob_std), eps)

    def hold(x_mean_ptr, level, i, draw):                  # after a step op, with that op's draw
        if known is not None:
            N.check(lib.sbgm_hold_known(x.data_ptr(), x_mean_ptr, known.data_ptr(), known_mask.data_ptr(), N.ptr(z(draw)),
                                        float(lv[level][i]), seed, draw, x.numel(), st()))
    with torch.no_grad():
        for i, ts in enumerate(time_steps):
            bt = ones * ts
            grad = N.f32c(_score(score_model, cfg, x, bt, y, cond_img, lsm_cond, topo_cond, clamp=True))
            N.check(lib.sbgm_langevin_step(x.data_ptr(), grad.data_ptr(), N.ptr(z(1 + 2 * i)), snr_nn, sumsq.data_ptr(), seed,
                                           1 + 2 * i, batch_size, per, st()))
            hold(None, "s_cur", i, 1 + 2 * i)
            g = float(diffusion_coeff(bt)[0])
            score = N.f32c(_score(score_model, cfg, x, bt, y, cond_img, lsm_cond, topo_cond))
            N.check(lib.sbgm_em_step(x.data_ptr(), x_mean.data_ptr(), score.data_ptr(), N.ptr(z(2 + 2 * i)), g * g, step_size,
                                     math.sqrt(g * g * step_size), seed, 2 + 2 * i, x.numel(), st()))
            hold(x_mean.data_ptr(), "s_next", i, 2 + 2 * i)
    return x_mean


def ode_sampler(score_model, marginal_prob_std, diffusion_coeff, num_steps=100, batch_size=64, atol=error_tolerance,
                rtol=error_tolerance, device="cuda", z=None, eps=1e-3, img_size=64, y=None, cond_img=None, lsm_cond=None,
                topo_cond=None, cfg=None, *, return_nfev=False):
    """Probability-flow ODE via scipy RK45 (reference score_sampling.py:239-300).  Host-driven by construction
    (the solver lives in scipy); every right-hand-side evaluation is one native network evaluation.  Like the
    reference it conditions on nothing but (x, t) (:290) and starts from 32x32 unless `z` is given (:279-283).  The
    right-hand side keeps the reference's precision: t goes to the network in fp32, g(t)^2 is squared in fp32 (:296) and
    multiplies the float64 score.  Keyword-only `return_nfev` (not in the reference, which only logs the count) also
    returns the number of right-hand-side evaluations."""
    from scipy import integrate
    ones = torch.ones(batch_size, device=device)
    if z is None:
        init_x = torch.randn(batch_size, 1, 32, 32, device=device) * marginal_prob_std(ones)[:, None, None, None]
    else:
        init_x = z
    shape = init_x.shape

    def rhs(t, xflat):
        xs = torch.tensor(xflat, device=device, dtype=torch.float32).reshape(shape)
        tt = torch.tensor(np.ones((shape[0],)) * t, device=device, dtype=torch.float32)
        with torch.no_grad():
            s = score_model(xs, tt)
        g = diffusion_coeff(torch.tensor(t)).cpu().numpy()          # fp32 0-d array, as in the reference
        return -0.5 * (g ** 2) * s.cpu().numpy().reshape(-1).astype(np.float64)

    res = integrate.solve_ivp(rhs, (1.0, eps), init_x.reshape(-1).cpu().numpy(), rtol=rtol, atol=atol, method="RK45")
    logger.info(f"Number of function evaluations: {res.nfev}")
    x = torch.tensor(res.y[:, -1], device=device).reshape(shape)
    return (x, res.nfev) if return_nfev else x


def edm_sigma_schedule(n_steps, sigma_min=0.002, sigma_max=80, rho=7.0, device="cuda"):
    """Karras sigma ladder (reference score_sampling.py:304-307; unused by the CLI)."""
    i = torch.linspace(0, 1, n_steps, device=device)
    return (sigma_max ** (1 / rho) + i * (sigma_min ** (1 / rho) - sigma_max ** (1 / rho))) ** rho


def _ve_std(t, sigma_sde):
    """marginal_prob_std in float64 (no floor): sqrt((sigma^2t - 1) / (2 ln sigma))"""
    ls = math.log(sigma_sde)
    return np.sqrt(np.expm1(2.0 * np.asarray(t, dtype=np.float64) * ls) / (2.0 * ls))


def edm_heun_schedule(num_steps, sigma_sde=25.0, eps=1e-3, sigma_min=None, sigma_max=None, rho=7.0, s_churn=0.0, s_tmin=0.0,
                      s_tmax=float("inf"), s_noise=1.0):
    """Step table of `edm_heun_sampler` (Karras et al. 2022, Alg. 2 on the VE SDE), in float64.  The engine builds the same
    table (stored as fp32) for its native loop.  Returns a dict of numpy arrays and counts:

    sigma [N+1]       Karras ladder sigma_i = (smax^(1/rho) + i/(N-1) (smin^(1/rho) - smax^(1/rho)))^rho, sigma_N = 0
    gamma, sigma_hat  churn gamma_i = min(s_churn/N, sqrt2-1) inside [s_tmin, s_tmax], capped so sigma_hat <= sigma_0
    t_hat, t_next     t(sigma_hat_i), t(sigma_{i+1}) with t(s) = log1p(2 ln sigma_sde s^2) / (2 ln sigma_sde), clamped to [eps, 1]
    churn_coef        s_noise sqrt(sigma_hat^2 - sigma_i^2)
    nfe, draws        2N - 1 network evaluations; 1 noise draw (+N when s_churn > 0)
    sigma_min/max     the ladder's ends after clipping

    sigma_min / sigma_max default to the trained range [std(eps), std(1)]; other values are clipped to it, with one warning."""
    if not s_churn >= 0:
        raise ValueError(f"edm_heun_sampler: s_churn={s_churn} must be >= 0")
    N_, sigma, t_of, smin, smax = _karras_ladder("edm_heun_sampler", num_steps, sigma_sde, eps, sigma_min, sigma_max, rho, s_noise)
    s = sigma[:N_]
    gamma = np.where((s_tmin <= s) & (s <= s_tmax), min(s_churn / N_, math.sqrt(2.0) - 1.0), 0.0)
    gamma = np.minimum(gamma, sigma[0] / s - 1.0)
    sigma_hat = s * (1.0 + gamma)
    return {"sigma": sigma, "gamma": gamma, "sigma_hat": sigma_hat, "t_hat": t_of(sigma_hat), "t_next": t_of(sigma[1:]),
            "churn_coef": s_noise * np.sqrt(np.maximum(0.0, sigma_hat ** 2 - s ** 2)), "nfe": 2 * N_ - 1,
            "draws": _counts(N.SAMPLER_EDM_HEUN, N_, s_churn > 0)[1], "sigma_min": smin, "sigma_max": smax}


def _karras_ladder(who, num_steps, sigma_sde, eps, sigma_min, sigma_max, rho, s_noise):
    """what the few-step schedules share: the checked arguments, the Karras ladder sigma [N+1] (sigma_N = 0) clipped to the trained range
    with one warning, and t(sigma).  Returns (N, sigma, t_of, sigma_min, sigma_max)."""
    N_ = int(num_steps)
    if N_ < 2:
        raise ValueError(f"{who}: num_steps={num_steps} must be >= 2")
    if not rho > 0:
        raise ValueError(f"{who}: rho={rho} must be > 0")
    if not s_noise >= 0:
        raise ValueError(f"{who}: s_noise={s_noise} must be >= 0")
    ls = math.log(sigma_sde)
    lo, hi = float(_ve_std(eps, sigma_sde)), float(_ve_std(1.0, sigma_sde))
    smin = lo if sigma_min is None else float(sigma_min)
    smax = hi if sigma_max is None else float(sigma_max)
    clipped_min, clipped_max = min(hi, max(lo, smin)), min(hi, max(lo, smax))
    if (clipped_min, clipped_max) != (smin, smax):
        logger.warning(f"{who}: sigma range [{smin:g}, {smax:g}] clipped to the trained range [{lo:.6g}, {hi:.6g}] "
                       f"(std(eps), std(1) of the VE SDE with sigma={sigma_sde:g})")
    smin, smax = clipped_min, clipped_max
    if not smin < smax:
        raise ValueError(f"{who}: sigma_min={smin:g} must be below sigma_max={smax:g}")
    a0, a1 = smax ** (1.0 / rho), smin ** (1.0 / rho)
    sigma = np.zeros(N_ + 1)
    sigma[:N_] = (a0 + np.arange(N_, dtype=np.float64) / (N_ - 1) * (a1 - a0)) ** rho
    sigma[0], sigma[N_ - 1] = smax, smin                   # the ends exactly (the power round trip is off by an ulp)

    def t_of(v):                                           # clamped in sigma too: sigma >= std(1) is t = 1 exactly
        t = np.clip(np.log1p(2.0 * ls * np.square(v)) / (2.0 * ls), eps, 1.0)
        return np.where(v >= hi, 1.0, np.where(v <= lo, eps, t))
    return N_, sigma, t_of, smin, smax


def edm_sampler_kwargs(cfg) -> dict:
    """keyword arguments of `edm_heun_sampler` from the optional `edm:` section of a config (sigma_min, sigma_max, rho and
    s_churn, s_tmin, s_tmax, s_noise); a missing section or key keeps the sampler's default.  `edm.enabled` is not read:
    `sampler.sampler_type` selects the sampler."""
    sec = (cfg or {}).get("edm") or {}
    return {k: float(sec[k]) for k in ("sigma_min", "sigma_max", "rho", "s_churn", "s_tmin", "s_tmax", "s_noise")
            if sec.get(k) is not None}


def edm_heun_sampler(score_model, marginal_prob_std, diffusion_coeff, batch_size=64, num_steps=32, device="cuda", eps=1e-3,
                     img_size=64, y=None, cond_img=None, lsm_cond=None, topo_cond=None, cfg=None, *, sigma_min=None, sigma_max=None,
                     rho=7.0, s_churn=0.0, s_tmin=0.0, s_tmax=float("inf"), s_noise=1.0, noise=None, use_graph=True, seed=None,
                     tile_origins=None, domain_width=0, known=None, known_mask=None, joint_tiles=None, noise_rows=None,
                     noise_weights=None, noise_row_stride=1, noise_domain_row=None, domain_height=None):
    """Heun (2nd-order) solver of the probability-flow ODE dx/dsigma = -sigma * score on the Karras sigma ladder, with optional
    stochastic churn (Karras et al. 2022, Alg. 2); works with the VE-SDE score network as trained.  `num_steps` N costs 2N-1
    network evaluations (18-64 is the intended range).  Conditions, guidance (`cfg`: both evaluations of a step use
    guidance_scale), `noise` (draw 0 = initial state, draw 1+i = churn of step i when s_churn > 0), `seed`, `use_graph` and
    `tile_origins` behave as in `pc_sampler`.  `diffusion_coeff` is accepted for signature compatibility and unused.
    `known` / `known_mask` as in `pc_sampler`; here a held pixel follows known + sigma * (draw 0), the exact trajectory of a point mass,
    so the sampler stays deterministic in its seed.  `joint_tiles` as in `pc_sampler`: both slopes of a step use the blended score.
    `noise_rows` / `noise_weights` / `noise_row_stride` as in `pc_sampler`: the start, the churn and the held pixels' draw 0 are mixed;
    `noise_domain_row` / `domain_height` (the plan of a tiled run) as in `pc_sampler`.
    Returns x after the last step, [B,1,H,W] (no noise added at the end).  Sample quality against `pc_sampler` at 1000 steps
    has not been measured."""
    sig = float(score_model.sigma) if isinstance(score_model, ScoreNet) else _sigma_of(marginal_prob_std)
    sch = edm_heun_schedule(num_steps, sig, eps, sigma_min, sigma_max, rho, s_churn, s_tmin, s_tmax, s_noise)
    seed = _fresh_seed() if seed is None else seed
    known, known_mask = _prep_known(known, known_mask, batch_size, img_size, device, "edm_heun_sampler")
    joint = _prep_joint(joint_tiles, tile_origins, noise, "edm_heun_sampler")
    plan = _prep_noise_plan(noise_rows, noise_weights, noise_row_stride, batch_size, "edm_heun_sampler", noise, tile_origins, joint_tiles,
                            noise_domain_row, domain_height, img_size)
    if isinstance(score_model, ScoreNet) and not score_model.training:
        edm_args = (0.0 if sigma_min is None else sch["sigma_min"], 0.0 if sigma_max is None else sch["sigma_max"], float(rho),
                    float(s_churn), float(s_tmin), float(s_tmax), float(s_noise))
        return _native_run(N.SAMPLER_EDM_HEUN, score_model, batch_size, num_steps, 0.0, eps, img_size, y, cond_img, lsm_cond,
                           topo_cond, noise, use_graph, seed, device, cfg, tile_origins, domain_width, edm_args=edm_args,
                           held=(known, known_mask), joint=joint, plan=plan)
    lib, st = N.lib(), N.stream
    churn = s_churn > 0
    x, z = _host_start(N.SAMPLER_EDM_HEUN, batch_size, num_steps, img_size, device, noise, seed, float(np.float32(sch["sigma"][0])),
                       tile_origins, churn, joint=joint, plan=plan)
    n = x.numel()
    xp, d, out = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    ones = torch.ones(batch_size, device=device)
    if known is not None:
        x = _held_start(x, known, known_mask)

    def hold(v, level):                                    # held pixels: known + sigma_{i+1} * (draw 0)
        if known is not None:
            N.check(lib.sbgm_hold_known(v.data_ptr(), None, known.data_ptr(), known_mask.data_ptr(), N.ptr(z(0)), level, seed, 0, n, st()))
    with torch.no_grad():
        for i in range(int(num_steps)):
            sh, sn = float(sch["sigma_hat"][i]), float(sch["sigma"][i + 1])
            if churn:
                N.check(lib.sbgm_edm_churn(x.data_ptr(), N.ptr(z(1 + i)), float(sch["churn_coef"][i]), seed, 1 + i, n, st()))
            s1 = N.f32c(_score(score_model, cfg, x, ones * float(np.float32(sch["t_hat"][i])), y, cond_img, lsm_cond, topo_cond))
            last = i == int(num_steps) - 1
            N.check(lib.sbgm_edm_euler(x.data_ptr(), s1.data_ptr(), d.data_ptr(), (out if last else xp).data_ptr(), sh, sn, n, st()))
            hold(out if last else xp, sn)
            if last:
                break
            s2 = N.f32c(_score(score_model, cfg, xp, ones * float(np.float32(sch["t_next"][i])), y, cond_img, lsm_cond, topo_cond))
            N.check(lib.sbgm_edm_heun(x.data_ptr(), d.data_ptr(), s2.data_ptr(), sh, sn, n, st()))
            hold(x, sn)
    return out


def dpmpp_2m_schedule(num_steps, sigma_sde=25.0, eps=1e-3, sigma_min=None, sigma_max=None, rho=7.0, eta=0.0, s_noise=1.0):
    """Step table of `dpmpp_2m_sampler` (DPM-Solver++(2M), Lu et al. 2022, on the VE SDE: alpha = 1, sigma = marginal_prob_std; eta > 0 is
    its SDE variant in midpoint form), in float64.  The engine builds the same table (stored as fp32) for its native loop.  With
    D_i = x_i + sigma_i^2 score(x_i, t_i) step i is x_{i+1} = c_x x_i + c_0 D_i + c_1 D_{i-1} + c_z z_i.  Returns a dict of numpy arrays
    and counts:

    sigma [N+1]       the Karras ladder of `edm_heun_schedule` (same defaults, same clipping with one warning), sigma_N = 0
    t [N]             t(sigma_i), the evaluation times, clamped to [eps, 1]
    c_x, c_0, c_1     with h_i = ln(sigma_i / sigma_{i+1}), a_i = -expm1(-(1 + eta) h_i): c_x = (sigma_{i+1} / sigma_i) exp(-eta h_i);
                      c_0 = a_i, c_1 = 0 at i = 0; c_0 = a_i (1 + 1/(2r)), c_1 = -a_i / (2r), r = h_{i-1} / h_i at i >= 1
    c_z               s_noise sigma_{i+1} sqrt(-expm1(-2 eta h_i))
                      the last row is (c_x, c_0, c_1, c_z) = (0, 1, 0, 0): x_N = D_{N-1}
    nfe, draws        N network evaluations; 1 noise draw (+N when eta > 0: draw 1+i belongs to step i)
    sigma_min/max     the ladder's ends after clipping"""
    if not eta >= 0:
        raise ValueError(f"dpmpp_2m_sampler: eta={eta} must be >= 0")
    N_, sigma, t_of, smin, smax = _karras_ladder("dpmpp_2m_sampler", num_steps, sigma_sde, eps, sigma_min, sigma_max, rho, s_noise)
    c_x, c_0, c_1, c_z = np.zeros(N_), np.ones(N_), np.zeros(N_), np.zeros(N_)
    h = np.log(sigma[:N_ - 1] / sigma[1:N_])
    a = -np.expm1(-(1.0 + eta) * h)
    c_x[:-1] = sigma[1:N_] / sigma[:N_ - 1] * np.exp(-eta * h)
    c_0[:-1] = a
    r = h[:-1] / h[1:]                                     # r_i = h_{i-1} / h_i of the steps 1 .. N-2
    c_0[1:-1] = a[1:] * (1.0 + 1.0 / (2.0 * r))
    c_1[1:-1] = -a[1:] / (2.0 * r)
    c_z[:-1] = s_noise * sigma[1:N_] * np.sqrt(np.maximum(0.0, -np.expm1(-2.0 * eta * h)))
    return {"sigma": sigma, "t": t_of(sigma[:N_]), "c_x": c_x, "c_0": c_0, "c_1": c_1, "c_z": c_z, "nfe": N_,
            "draws": _counts(N.SAMPLER_DPMPP_2M, N_, eta > 0)[1], "sigma_min": smin, "sigma_max": smax}


def dpm_sampler_kwargs(cfg) -> dict:
    """keyword arguments of `dpmpp_2m_sampler` from the optional `dpm:` section of a config (sigma_min, sigma_max, rho, eta, s_noise); a
    missing section or key keeps the sampler's default.  `sampler.sampler_type: dpmpp_2m_sampler` selects the sampler."""
    sec = (cfg or {}).get("dpm") or {}
    return {k: float(sec[k]) for k in ("sigma_min", "sigma_max", "rho", "eta", "s_noise") if sec.get(k) is not None}


def dpmpp_2m_sampler(score_model, marginal_prob_std, diffusion_coeff, batch_size=64, num_steps=32, device="cuda", eps=1e-3,
                     img_size=64, y=None, cond_img=None, lsm_cond=None, topo_cond=None, cfg=None, *, sigma_min=None, sigma_max=None,
                     rho=7.0, eta=0.0, s_noise=1.0, noise=None, use_graph=True, seed=None, tile_origins=None, domain_width=0,
                     known=None, known_mask=None, joint_tiles=None, noise_rows=None, noise_weights=None, noise_row_stride=1,
                     noise_domain_row=None, domain_height=None):
    """DPM-Solver++(2M) (Lu et al. 2022) on the Karras sigma ladder of `edm_heun_sampler`: a second-order multistep solver that reuses the
    previous step's denoised estimate, so `num_steps` N costs exactly N network evaluations (EDM Heun: 2N-1).  `eta = 0` is the
    deterministic solver of the probability-flow ODE; `eta > 0` is the SDE variant ("2M SDE", midpoint form), which adds noise of weight
    `s_noise` in every step.  `dpmpp_2m_schedule` is the table.  Conditions, guidance (`cfg`: the evaluation uses guidance_scale), `seed`,
    `use_graph`, `tile_origins` and `joint_tiles` behave as in `pc_sampler`; `noise`: draw 0 = initial state, and with eta > 0 draw 1+i =
    step i.  `diffusion_coeff` is accepted for signature compatibility and unused.
    `known` / `known_mask` as in `pc_sampler`: after every step the held pixels are known + sigma_{i+1} z, with z the run's draw 0 when
    eta = 0 (the trajectory of a point mass, as in `edm_heun_sampler`: deterministic in the seed) and the step's own draw when eta > 0.
    `noise_rows` / `noise_weights` / `noise_row_stride` as in `pc_sampler` (the start, and with eta > 0 every step's draw);
    `noise_domain_row` / `domain_height` (the plan of a tiled run) as in `pc_sampler`.
    An eval-mode ScoreNet runs the native loop (`sbgm_sampler_run_dpmpp`); any other callable runs a Python loop over the same update
    kernel.  Returns x after the last step, [B,1,H,W].  On the analytic Gaussian problem it has the error of EDM Heun at the same N;
    sample quality on a trained checkpoint has not been measured."""
    sig = float(score_model.sigma) if isinstance(score_model, ScoreNet) else _sigma_of(marginal_prob_std)
    sch = dpmpp_2m_schedule(num_steps, sig, eps, sigma_min, sigma_max, rho, eta, s_noise)
    seed = _fresh_seed() if seed is None else seed
    known, known_mask = _prep_known(known, known_mask, batch_size, img_size, device, "dpmpp_2m_sampler")
    joint = _prep_joint(joint_tiles, tile_origins, noise, "dpmpp_2m_sampler")
    plan = _prep_noise_plan(noise_rows, noise_weights, noise_row_stride, batch_size, "dpmpp_2m_sampler", noise, tile_origins, joint_tiles,
                            noise_domain_row, domain_height, img_size)
    if isinstance(score_model, ScoreNet) and not score_model.training:
        dpm_args = (0.0 if sigma_min is None else sch["sigma_min"], 0.0 if sigma_max is None else sch["sigma_max"], float(rho),
                    float(eta), float(s_noise))
        return _native_run(N.SAMPLER_DPMPP_2M, score_model, batch_size, num_steps, 0.0, eps, img_size, y, cond_img, lsm_cond,
                           topo_cond, noise, use_graph, seed, device, cfg, tile_origins, domain_width, held=(known, known_mask),
                           joint=joint, dpm_args=dpm_args, plan=plan)
    lib, st = N.lib(), N.stream
    sde = eta > 0
    f32 = lambda v: float(np.float32(v))  # noqa: E731
    x, z = _host_start(N.SAMPLER_DPMPP_2M, batch_size, num_steps, img_size, device, noise, seed, f32(sch["sigma"][0]), tile_origins, sde,
                       joint=joint, plan=plan)
    n = x.numel()
    hist = torch.empty_like(x)
    ones = torch.ones(batch_size, device=device)
    if known is not None:
        x = _held_start(x, known, known_mask)
    with torch.no_grad():
        for i in range(int(num_steps)):
            draw = 1 + i if sde else 0                     # the draw a held pixel is re-noised with
            score = N.f32c(_score(score_model, cfg, x, ones * f32(sch["t"][i]), y, cond_img, lsm_cond, topo_cond))
            N.check(lib.sbgm_dpmpp_2m_step(x.data_ptr(), score.data_ptr(), hist.data_ptr(), N.ptr(z(draw)) if sde else None,
                                           f32(sch["sigma"][i]), f32(sch["c_x"][i]), f32(sch["c_0"][i]), f32(sch["c_1"][i]),
                                           f32(sch["c_z"][i]), seed, draw, n, st()))
            if known is not None:
                N.check(lib.sbgm_hold_known(x.data_ptr(), None, known.data_ptr(), known_mask.data_ptr(), N.ptr(z(draw)),
                                            f32(sch["sigma"][i + 1]), seed, draw, n, st()))
    return x


# ---- rk45_sampler: Dormand-Prince 5(4) with the step controller of scipy.integrate.RK45 -------------------------------------------
_RK_C = np.array([0, 1 / 5, 3 / 10, 4 / 5, 8 / 9, 1])
_RK_A = np.array([[0, 0, 0, 0, 0], [1 / 5, 0, 0, 0, 0], [3 / 40, 9 / 40, 0, 0, 0], [44 / 45, -56 / 15, 32 / 9, 0, 0],
                  [19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729, 0],
                  [9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656]])
_RK_B = np.array([35 / 384, 0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84])
_RK_E = np.array([-71 / 57600, 0, 71 / 16695, -71 / 1920, 17253 / 339200, -22 / 525, 1 / 40])
_RK_SAFETY, _RK_MIN_FACTOR, _RK_MAX_FACTOR = 0.9, 0.2, 10.0
_ODE_FAILURES = {N.ODE_TOO_SMALL_STEP: "the step size fell below the minimal step (10 ulp of t) after a rejection",
                 N.ODE_NONFINITE: "non-finite error norm (the right-hand side returned NaN or inf)",
                 N.ODE_MAX_STEPS: "the step budget (max_steps={max_steps}) was used up before t reached the end of t_span"}


class OdeSolverError(RuntimeError):
    """the adaptive solver stopped before the end of its time span; the message names the cause"""


def _rms(x):
    return np.linalg.norm(x) / x.size ** 0.5


def _check_tolerances(rtol, atol, error_norm, max_steps):
    if error_norm not in ("batch", "sample"):
        raise ValueError(f"rk45: error_norm={error_norm!r} must be 'batch' or 'sample'")
    if not rtol > 0:
        raise ValueError(f"rk45: rtol={rtol} must be > 0")
    if not atol >= 0:
        raise ValueError(f"rk45: atol={atol} must be >= 0")
    if not int(max_steps) >= 1:
        raise ValueError(f"rk45: max_steps={max_steps} must be >= 1")


def rk45_host_solve(f, t0, t_bound, y0, rtol, atol, error_norm="batch", batch=None, max_steps=10000):
    """The solver of `rk45_sampler`, restated in numpy: Dormand-Prince 5(4) with FSAL, `select_initial_step` and the step
    controller of scipy.integrate.RK45 (scipy 1.15), float64 throughout.  The stage sums are the same `np.dot` expressions as
    scipy's, so for `error_norm="batch"` the endpoint and the evaluation count equal `solve_ivp(f, (t0, t_bound), y0,
    method="RK45", rtol=rtol, atol=atol)` (rtol is not raised to 100 eps here; rtol <= 0 is an error).

    error_norm="batch": `y0` is one vector, `f(t, y)` with a float `t`; one controller, scipy's semantics.
    error_norm="sample": `y0` is [batch, m] (or flat, with `batch` given) and `f(t, y)` takes t [batch] and y [batch, m], row b being
    a function of (t[b], y[b]) alone.  Every row has its own controller (t, h, error norm over its m values, initial step, accept /
    reject, counters); a finished row is frozen: `f` still sees it, at its final (t, y), and the result is ignored.

    Returns (y, stats); stats holds nfev, n_accepted, n_rejected and t_final (ints / a float, or arrays of `batch` in sample mode).
    Raises OdeSolverError, naming the cause, on a non-finite error norm (at once), when a controller has used `max_steps` attempts,
    or when the step falls below 10 ulp of t after a rejection."""
    _check_tolerances(rtol, atol, error_norm, max_steps)
    per_sample = error_norm == "sample"
    y0 = np.asarray(y0, dtype=np.float64)
    shape = y0.shape
    if per_sample:
        G = int(batch) if batch is not None else int(shape[0])
        ys = [np.ascontiguousarray(r) for r in y0.reshape(G, -1)]
    else:
        G = 1
        ys = [y0.reshape(-1).copy()]
    t0, t_bound = float(t0), float(t_bound)
    if t0 == t_bound:
        raise ValueError("rk45: t0 and t_bound must differ")
    direction = float(np.sign(t_bound - t0))
    m = ys[0].size
    ts = [t0] * G

    def call(tt, yy):                                  # one evaluation of every row, frozen ones included
        if per_sample:
            return list(np.asarray(f(np.asarray(tt, dtype=np.float64), np.stack(yy)), dtype=np.float64).reshape(G, m))
        return [np.asarray(f(tt[0], yy[0]), dtype=np.float64).reshape(m)]

    def fail(code, g):
        who = f" (sample {g})" if per_sample else ""
        raise OdeSolverError("rk45" + who + ": " + _ODE_FAILURES[code].format(max_steps=max_steps))

    def finite(v, g):
        if not np.isfinite(v):
            fail(N.ODE_NONFINITE, g)

    # ---- select_initial_step (order 4) --------------------------------------------------------------------------------------------
    K = [np.empty((7, m)) for _ in range(G)]
    fs = call(ts, ys)
    nfev = np.full(G, 2, dtype=np.int64)
    h0s, d1s, scales = [0.0] * G, [0.0] * G, [None] * G
    interval = abs(t_bound - t0)
    for g in range(G):
        scales[g] = atol + np.abs(ys[g]) * rtol
        d0, d1 = _rms(ys[g] / scales[g]), _rms(fs[g] / scales[g])
        finite(d0, g), finite(d1, g)
        h0s[g] = min(1e-6 if d0 < 1e-5 or d1 < 1e-5 else 0.01 * d0 / d1, interval)
        d1s[g] = d1
    f1s = call([t0 + h0s[g] * direction for g in range(G)], [ys[g] + h0s[g] * direction * fs[g] for g in range(G)])
    h_abs = [0.0] * G
    for g in range(G):
        d2 = _rms((f1s[g] - fs[g]) / scales[g]) / h0s[g]
        finite(d2, g)
        h1 = max(1e-6, h0s[g] * 1e-3) if d1s[g] <= 1e-15 and d2 <= 1e-15 else (0.01 / max(d1s[g], d2)) ** (1 / 5)
        h_abs[g] = min(100 * h0s[g], h1, interval)
    # ---- the attempts -------------------------------------------------------------------------------------------------------------
    running = [True] * G
    rejected = [False] * G
    n_acc, n_rej = np.zeros(G, dtype=np.int64), np.zeros(G, dtype=np.int64)
    hs, t_news = [0.0] * G, [0.0] * G
    while any(running):
        live = [g for g in range(G) if running[g]]
        for g in live:
            t = ts[g]
            min_step = 10 * np.abs(np.nextafter(t, direction * np.inf) - t)
            if not rejected[g]:
                h_abs[g] = max(h_abs[g], min_step)
            elif h_abs[g] < min_step:
                fail(N.ODE_TOO_SMALL_STEP, g)
            h = h_abs[g] * direction
            t_new = t + h
            if direction * (t_new - t_bound) > 0:
                t_new = t_bound
            hs[g], t_news[g] = t_new - t, t_new
            h_abs[g] = np.abs(hs[g])
            K[g][0] = fs[g]
        y_new = list(ys)
        for s in range(1, 7):
            tt, yy = list(ts), list(ys)
            for g in live:
                if s < 6:
                    yy[g] = ys[g] + np.dot(K[g][:s].T, _RK_A[s, :s]) * hs[g]
                    tt[g] = ts[g] + _RK_C[s] * hs[g]
                else:
                    yy[g] = y_new[g] = ys[g] + hs[g] * np.dot(K[g][:-1].T, _RK_B)
                    tt[g] = ts[g] + hs[g]
            out = call(tt, yy)
            for g in live:
                K[g][s] = out[g]
        for g in live:
            nfev[g] += 6
            scale = atol + np.maximum(np.abs(ys[g]), np.abs(y_new[g])) * rtol
            err = _rms(np.dot(K[g].T, _RK_E) * hs[g] / scale)
            finite(err, g)
            if err < 1:
                factor = _RK_MAX_FACTOR if err == 0 else min(_RK_MAX_FACTOR, _RK_SAFETY * err ** -0.2)
                if rejected[g]:
                    factor = min(1, factor)
                h_abs[g] *= factor
                ts[g] = t_news[g]
                ys[g], fs[g] = y_new[g], K[g][6].copy()
                rejected[g] = False
                n_acc[g] += 1
                if direction * (ts[g] - t_bound) >= 0:
                    running[g] = False
            else:
                h_abs[g] *= max(_RK_MIN_FACTOR, _RK_SAFETY * err ** -0.2)
                rejected[g] = True
                n_rej[g] += 1
            if running[g] and n_acc[g] + n_rej[g] >= int(max_steps):
                fail(N.ODE_MAX_STEPS, g)
    if per_sample:
        return np.stack(ys).reshape(shape), {"nfev": nfev, "n_accepted": n_acc, "n_rejected": n_rej, "t_final": np.asarray(ts)}
    return ys[0].reshape(shape), {"nfev": int(nfev[0]), "n_accepted": int(n_acc[0]), "n_rejected": int(n_rej[0]), "t_final": ts[0]}


def ode_sampler_kwargs(cfg) -> dict:
    """keyword arguments of `rk45_sampler` from the optional `ode:` section of a config (rtol, atol, error_norm, max_steps); a
    missing section or key keeps the sampler's default.  `sampler.sampler_type: rk45_sampler` selects the sampler; `n_timesteps`
    is not read by it (the tolerances decide the number of steps)."""
    sec = (cfg or {}).get("ode") or {}
    kw = {k: float(sec[k]) for k in ("rtol", "atol") if sec.get(k) is not None}
    if sec.get("error_norm") is not None:
        kw["error_norm"] = str(sec["error_norm"])
    if sec.get("max_steps") is not None:
        kw["max_steps"] = int(sec["max_steps"])
    return kw


def _ode_stats(raw_i, raw_d, G, per_sample, max_steps, surplus):
    """statistics dict of a run from the solver's read-back; raises OdeSolverError when a controller did not finish"""
    grp = raw_i[:4 * G].reshape(G, 4)
    for g in range(G):
        code = int(grp[g, 3])
        if code != N.ODE_FINISHED:
            who = f" (sample {g})" if per_sample else ""
            why = _ODE_FAILURES.get(code, f"controller status {code}").format(max_steps=max_steps)
            raise OdeSolverError(f"rk45_sampler{who}: {why}; stopped at t = {raw_d[g]:.6g} after {int(grp[g, 1])} accepted and "
                                 f"{int(grp[g, 2])} rejected steps")
    one = (lambda a: a.copy()) if per_sample else (lambda a: a[0].item())
    return {"nfev": one(grp[:, 0]), "n_accepted": one(grp[:, 1]), "n_rejected": one(grp[:, 2]), "t_final": one(raw_d[:G]),
            "surplus_attempts": int(surplus)}


def rk45_sampler(score_model, marginal_prob_std, diffusion_coeff, batch_size=64, device="cuda", eps=1e-3, img_size=64, y=None,
                 cond_img=None, lsm_cond=None, topo_cond=None, cfg=None, *, rtol=1e-5, atol=1e-5, error_norm="batch", t_span=None,
                 z=None, noise=None, seed=None, use_graph=True, max_steps=10000, tile_origins=None, domain_width=0,
                 return_stats=False, noise_rows=None, noise_weights=None, noise_row_stride=1):
    """Adaptive solver of the probability-flow ODE dx/dt = -1/2 g(t)^2 score(x, t) on the device: Dormand-Prince 5(4) with FSAL and
    the step controller of scipy.integrate.RK45 (`rk45_host_solve` is the definition), with the right-hand side in the precision of
    `ode_sampler` (network input and time in fp32, g(t)^2 squared in fp32, state and stage sums in float64).  `rtol` / `atol` take
    the place of a step count.  Unlike `ode_sampler` it is conditioned (`y`, `cond_img`, `lsm_cond`, `topo_cond`), guided (`cfg`:
    every evaluation uses guidance_scale) and tileable, and it honours `img_size`.

    t_span      (t0, t1), both in [eps, 1]; None is (1.0, eps), i.e. sampling.  (eps, 1.0) encodes data into the latent and needs `z`.
    z           start state [B,1,H,W] (its shape then sets the batch and image size).  Without it the run starts from
                marginal_prob_std(t0) times draw 0 of the run's Philox stream (`seed`), or times `noise[0]` when `noise` is given.
    error_norm  "batch": one step size and error norm over the whole batch (scipy's semantics).  "sample": one controller per sample,
                so a sample's trajectory does not depend on its batch-mates; required with `tile_origins`.
    max_steps   attempts (accepted + rejected) a controller may use; OdeSolverError when they run out, on a non-finite error norm, or
                when the step size underflows.
    `noise_rows` / `noise_weights` / `noise_row_stride` as in `pc_sampler`: they key and mix the start draw (the solver draws nothing
    else), so they are refused with `z`.
    `seed`, `use_graph`, `tile_origins`, `domain_width` as in `edm_heun_sampler`; `diffusion_coeff` is accepted for signature
    compatibility and unused (g(t) = sigma^t of the model).  An eval-mode ScoreNet runs the native loop (`sbgm_sampler_run_ode`:
    one captured attempt replayed until the device reports done); any other callable, or a train-mode model, runs a Python loop over
    the same kernels.  Returns fp32 [B,1,H,W]; with `return_stats` also a dict with nfev (network evaluations that counted, the two of
    the initial step included), n_accepted, n_rejected, t_final (arrays per sample with error_norm="sample") and surplus_attempts
    (attempts enqueued after the run was done: at most 1 for the native loop, 0 for the Python loop)."""
    _check_tolerances(rtol, atol, error_norm, max_steps)
    per_sample = error_norm == "sample"
    t0, t1 = (1.0, float(eps)) if t_span is None else (float(t_span[0]), float(t_span[1]))
    if not (eps <= t0 <= 1.0 and eps <= t1 <= 1.0) or t0 == t1:
        raise ValueError(f"rk45_sampler: t_span=({t0:g}, {t1:g}) must be two different times in [eps, 1] = [{eps:g}, 1]")
    if t0 < t1 and z is None:
        raise ValueError("rk45_sampler: encoding (t_span[0] < t_span[1]) starts from data: pass it as z")
    if z is not None and noise is not None:
        raise ValueError("rk45_sampler: pass either z (the start state) or noise (its N(0,1) draw), not both")
    if tile_origins is not None and not per_sample:
        raise ValueError("rk45_sampler: tile_origins needs error_norm='sample' (a step size shared by the batch would couple the tiles)")
    if z is not None:
        if z.dim() != 4 or z.shape[1] != 1 or z.shape[2] != z.shape[3]:
            raise ValueError(f"rk45_sampler: z must be [B, 1, H, H], got {tuple(z.shape)}")
        batch_size, img_size = int(z.shape[0]), int(z.shape[-1])
    B, hw = int(batch_size), int(img_size)
    plan = _prep_noise_rows(noise_rows, noise_weights, noise_row_stride, B, "rk45_sampler", noise, tile_origins)
    if plan is not None and z is not None:
        raise ValueError("rk45_sampler: noise_rows keys the start draw; it cannot be combined with z")
    G = B if per_sample else 1
    sig = float(score_model.sigma) if isinstance(score_model, ScoreNet) else _sigma_of(marginal_prob_std)
    seed = _fresh_seed() if seed is None else seed
    dev = torch.device(device) if not isinstance(device, torch.device) else device
    raw_i, raw_d = np.zeros(4 * G + 2, dtype=np.int64), np.zeros(G, dtype=np.float64)

    if isinstance(score_model, ScoreNet) and not score_model.training:
        if dev.type != "cuda":
            raise N.NativeError(f"the native samplers run on a ROCm device, got device={device!r}")
        x_dummy, t_dummy = torch.empty(B, 1, hw, hw, device=dev), torch.empty(B, device=dev)
        _, _, y, cond_img, lsm_cond, topo_cond = score_model._prep(x_dummy, t_dummy, y, cond_img, lsm_cond, topo_cond)
        eng = score_model._engine(lsm_cond, topo_cond, cond_img)
        out = torch.empty(B, 1, hw, hw, device=dev)
        x0 = None if z is None else N.f32c(z.to(dev))
        nz = None
        if noise is not None:
            nz = N.f32c((noise if torch.is_tensor(noise) else torch.stack(list(noise)))[0].to(dev))
            if tuple(nz.shape) != (B, 1, hw, hw):
                raise ValueError(f"noise[0] must be [{B}, 1, {hw}, {hw}], got {tuple(nz.shape)}")
        if tile_origins is not None:
            N.require_device(tile_origins)
            if tile_origins.dtype != torch.int32 or tuple(tile_origins.shape) != (B, 2) or not tile_origins.is_contiguous():
                raise ValueError("tile_origins must be a contiguous int32 [batch, 2] device tensor of (y0, x0)")
            if noise is not None or z is not None:
                raise ValueError("tile_origins keys the in-kernel noise; it cannot be combined with z or injected noise")
        a = N.SamplerArgs(N.SAMPLER_RK45, B, hw, hw, 0, float(eps), 0.0, int(seed), int(bool(use_graph)), 0, N.ptr(y), N.ptr(cond_img),
                          N.ptr(lsm_cond), N.ptr(topo_cond), N.ptr(nz), out.data_ptr(), *_guidance(cfg), N.ptr(tile_origins),
                          int(domain_width or 0))
        with _noise_plan(eng, plan, dev):
            N.check(eng.lib.sbgm_sampler_run_ode(eng.h, C.byref(a), t0, t1, float(rtol), float(atol), int(per_sample), int(max_steps),
                                                 N.ptr(x0), raw_i.ctypes.data, raw_d.ctypes.data, N.stream()))
        stats = _ode_stats(raw_i, raw_d, G, per_sample, max_steps, raw_i[4 * G])
        return (out, stats) if return_stats else out

    # ---- Python loop over the same kernels (any callable, or a train-mode model): also the definition the native loop is tested against
    lib, st = N.lib(), N.stream
    if z is not None:
        if tile_origins is not None:
            raise N.NativeError("domain-keyed noise (tile_origins) needs the native sampler loop (a ScoreNet in eval mode)")
        x = N.f32c(z.to(dev)).clone()
    else:
        std0 = float(marginal_prob_std(torch.full((B,), t0, device=dev))[0])
        x, _ = _host_start(N.SAMPLER_RK45, B, 0, hw, dev, noise, seed, std0, tile_origins, plan=plan)
    N.require_device(x)
    per, n = hw * hw, B * hw * hw
    state = torch.empty(int(lib.sbgm_rk45_state_bytes(G)), dtype=torch.uint8, device=dev)
    partials = torch.empty(int(lib.sbgm_rk45_partials_bytes(B, per)) // 8, dtype=torch.float64, device=dev)
    K = torch.empty(7, n, device=dev)
    yy, y_new = torch.empty(n, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.float64, device=dev)
    xs, t_dev = torch.empty(B, 1, hw, hw, device=dev), torch.empty(B, device=dev)
    ptrs = (yy.data_ptr(), y_new.data_ptr(), K.data_ptr(), n)

    def evaluate(phase, slot):
        N.check(lib.sbgm_rk45_stage(state.data_ptr(), phase, *ptrs, xs.data_ptr(), t_dev.data_ptr(), B, per, int(per_sample), st()))
        K[slot].copy_(N.f32c(_score(score_model, cfg, xs, t_dev, y, cond_img, lsm_cond, topo_cond)).reshape(-1))

    def control(what):
        N.check(lib.sbgm_rk45_control(state.data_ptr(), what, *ptrs, partials.data_ptr(), B, per, int(per_sample), st()))

    def done():
        N.check(lib.sbgm_rk45_read(state.data_ptr(), G, raw_i.ctypes.data, raw_d.ctypes.data, st()))
        return bool(raw_i[4 * G])

    with torch.no_grad():
        N.check(lib.sbgm_rk45_init(state.data_ptr(), G, t0, t1, float(rtol), float(atol), sig, int(max_steps), st()))
        N.check(lib.sbgm_rk45_load(yy.data_ptr(), x.data_ptr(), n, st()))
        evaluate(N.ODE_PHASE_F0, 0)
        control(0)
        evaluate(N.ODE_PHASE_F1, 1)
        control(1)
        while not done():
            for s in range(1, 7):
                evaluate(s, s)
            control(2)
            N.check(lib.sbgm_rk45_commit(state.data_ptr(), *ptrs, B, per, int(per_sample), st()))
        out = torch.empty(B, 1, hw, hw, device=dev)
        N.check(lib.sbgm_rk45_store(out.data_ptr(), yy.data_ptr(), n, st()))
    stats = _ode_stats(raw_i, raw_d, G, per_sample, max_steps, 0)
    return (out, stats) if return_stats else out
