"""Host restatement of `dpmpp_2m_sampler` (DPM-Solver++(2M) and its SDE variant) around any `score(x, t)`, written out in torch on the
CPU with injected noise, and the Heun recurrence next to it for the analytic comparison.  Modelled on `heun_restatement` of
test_gpu_edm_sampler.py / constrained_ref.py: `score` gets fp32 times, the step scalars are rounded to fp32 unless dtype is float64."""
import math

import numpy as np
import torch

from constrained_ref import hold, start
from sbgm_danra_amd import score_sampling as SS

SIG = 25.0


def dpm_restatement(score, noise, n_steps, dtype=torch.float32, x_init=None, known=None, mask=None, drop_noise=False, **sched):
    """x_{i+1} = c_x x_i + c_0 D_i + c_1 D_{i-1} + c_z z_i with D_i = x_i + sigma_i^2 score(x_i, t_i); the run starts from
    sigma_0 * noise[0] (+ m known), or from `x_init`.  eta > 0: noise[1 + i] is step i's draw.  Held pixels: known + sigma_{i+1} z with
    z = noise[0] at eta = 0 and the step's own draw at eta > 0; the history is not held.  `drop_noise`: leave the c_z z term out."""
    sch = SS.dpmpp_2m_schedule(n_steps, SIG, 1e-3, **sched)
    c = (lambda v: float(np.float32(v))) if dtype == torch.float32 else float
    B = noise[0].shape[0]
    sde = sch["draws"] > 1
    z0 = noise[0].to(dtype)
    x = start(z0, c(sch["sigma"][0]), known, mask) if x_init is None else x_init.to(dtype)
    d_prev = None
    for i in range(n_steps):
        sg = c(sch["sigma"][i])
        d = x + (sg * sg) * score(x, torch.full((B,), float(np.float32(sch["t"][i]))))
        z = noise[1 + i].to(dtype) if sde else z0
        v = c(sch["c_x"][i]) * x + c(sch["c_0"][i]) * d
        if sch["c_1"][i] != 0:
            v = v + c(sch["c_1"][i]) * d_prev
        if sde and not drop_noise:
            v = v + c(sch["c_z"][i]) * z
        if known is not None:
            v = hold(v, known + c(sch["sigma"][i + 1]) * z, mask)
        x, d_prev = v, d
    return x


def heun_f64(score, x0, n_steps, **sched):
    """the deterministic Heun recurrence of edm_heun_sampler in float64, from x0"""
    sch = SS.edm_heun_schedule(n_steps, SIG, 1e-3, **sched)
    B = x0.shape[0]
    x = x0.double()
    for i in range(n_steps):
        sh, sn = float(sch["sigma_hat"][i]), float(sch["sigma"][i + 1])
        d = -sh * score(x, torch.full((B,), float(sch["t_hat"][i]), dtype=torch.float64))
        xp = x + (sn - sh) * d
        if i == n_steps - 1:
            return xp
        d2 = -sn * score(xp, torch.full((B,), float(sch["t_next"][i]), dtype=torch.float64))
        x = x + (sn - sh) * 0.5 * (d + d2)


def gaussian_score_f64(s0):
    """score of Gaussian data of variance s0^2 under the VE SDE, in the precision of its arguments' times (float64 on the host)"""
    def f(x, t, y=None, c=None, l=None, tp=None):
        std = SS._ve_std(t.double().cpu().numpy(), SIG)
        var = torch.as_tensor(s0 ** 2 + std ** 2, device=x.device).view(-1, 1, 1, 1)
        return (-x.double() / var).to(x.dtype)
    return f


def gaussian_exact(x0, s0, sch):
    """the exact solution of the probability-flow ODE from x0 at sigma_max, denoised at sigma_min (test_analytic_score_solver_order)"""
    smin, smax = sch["sigma_min"], sch["sigma_max"]
    return x0 * math.sqrt((s0 ** 2 + smin ** 2) / (s0 ** 2 + smax ** 2)) * s0 ** 2 / (s0 ** 2 + smin ** 2)


def dpm_joint(score, seed, n_steps, geo, known=None, mask=None, **sched):
    """dpm_restatement on the domain of joint_tiles_ref.Geometry `geo`: the score is the stitch-weighted blend of the tiles' scores,
    the noise the domain draws 0 and (eta > 0) 1 + i; `known` / `mask` are domain fields [1, 1, Hd, Wd_pad]"""
    import joint_tiles_ref as J
    sch = SS.dpmpp_2m_schedule(n_steps, SIG, 1e-3, **sched)
    c = lambda v: float(np.float32(v))  # noqa: E731
    sde = sch["draws"] > 1
    z0 = J.domain_noise(seed, 0, geo)
    x = start(z0, c(sch["sigma"][0]), known, mask)
    d_prev = None
    for i in range(n_steps):
        sg = c(sch["sigma"][i])
        d = x + (sg * sg) * J.blended_score(score, x, c(sch["t"][i]), geo)[0]
        z = J.domain_noise(seed, 1 + i, geo) if sde else z0
        v = c(sch["c_x"][i]) * x + c(sch["c_0"][i]) * d
        if sch["c_1"][i] != 0:
            v = v + c(sch["c_1"][i]) * d_prev
        if sde:
            v = v + c(sch["c_z"][i]) * z
        if known is not None:
            v = hold(v, known + c(sch["sigma"][i + 1]) * z, mask)
        x, d_prev = v, d
    return J.crop(x, geo)
