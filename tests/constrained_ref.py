"""Host restatements of constrained sampling around any `score(x, t)`: the Euler-Maruyama, predictor-corrector and
EDM Heun recurrences with known pixels held, written out in torch on the CPU with injected noise and fp32-rounded step scalars (modelled on
`heun_restatement` of test_gpu_edm_sampler.py and on the oracle's EM / PC loops).  With `known=None` they are the unconstrained loops."""
import numpy as np
import torch

from oracle import torch_ref as O
from sbgm_danra_amd import score_sampling as SS

SIG = 25.0


def hold(v, target, m):
    """select with a soft edge: m == 0 -> v, m == 1 -> target (both bit-exactly), else (1-m) v + m target"""
    m = m.clamp(0.0, 1.0)
    return torch.where(m <= 0, v, torch.where(m >= 1, target, (1.0 - m) * v + m * target))


def start(z0, scale, known, mask):
    x = z0 * scale
    if known is None:
        return x
    m = mask.clamp(0.0, 1.0)
    return torch.where(m > 0, x + m * known, x)


def standard_mask(B, hw):
    """differs per sample, x edges that are no multiples of 4, touches the corner (0, 0), one feathered row of 0.25 / 0.5"""
    m = torch.zeros(B, 1, hw, hw)
    for b in range(B):
        m[b, 0, 0:5 + b, 0:7 + 2 * b] = 1.0
        m[b, 0, 10 + b:17, 5 + b:hw - 3] = 1.0
        m[b, 0, 17, 5 + b:hw - 3:2] = 0.25
        m[b, 0, 17, 6 + b:hw - 3:2] = 0.5
    return m


def em_restatement(score, noise, n_steps, known=None, mask=None, eps=1e-3):
    """oracle.Euler_Maruyama_sampler (torch.linspace times, fp32) with the hold after the start and after every update"""
    B = noise[0].shape[0]
    ones = torch.ones(B)
    lv = SS.sde_hold_levels("em", n_steps, SIG, eps)
    x = start(noise[0].float(), O.marginal_prob_std(ones)[:, None, None, None], known, mask)
    ts = torch.linspace(1.0, eps, n_steps)
    dt = ts[0] - ts[1]
    mean_x = x
    for i, tt in enumerate(ts):
        bt = ones * tt
        g = O.diffusion_coeff(bt)
        z = noise[1 + i].float()
        mean = x + (g ** 2)[:, None, None, None] * score(x, bt) * dt
        x = mean + torch.sqrt(dt) * g[:, None, None, None] * z
        mean_x = mean
        if known is not None:
            mean_x = hold(mean, known, mask)
            x = hold(x, known + float(lv["s_next"][i]) * z, mask)
    return mean_x


def pc_restatement(score, noise, n_steps, known=None, mask=None, snr=0.16, eps=1e-3, score_corr=None):
    """oracle.pc_sampler (np.linspace float64 scalars on fp32 tensors, batch-mean score norm) with the hold after the start, the
    corrector (level std(t_i)) and the predictor (level std(t_{i+1}), 0 at the end); `score_corr`: the corrector's evaluation"""
    B = noise[0].shape[0]
    ones = torch.ones(B)
    lv = SS.sde_hold_levels("pc", n_steps, SIG, eps)
    x = start(noise[0].float(), O.marginal_prob_std(ones)[:, None, None, None], known, mask)
    ts = np.linspace(1.0, eps, n_steps)
    dt = ts[0] - ts[1]
    x_mean = x
    for i, tt in enumerate(ts):
        bt = ones * tt
        grad = (score_corr or score)(x, bt)
        gnorm = torch.norm(grad.reshape(B, -1), dim=-1).mean()
        lstep = 2 * (snr * np.sqrt(np.prod(x.shape[1:])) / gnorm) ** 2
        z = noise[1 + 2 * i].float()
        x = x + lstep * grad + torch.sqrt(2 * lstep) * z
        if known is not None:
            x = hold(x, known + float(lv["s_cur"][i]) * z, mask)
        g = O.diffusion_coeff(bt)
        z = noise[2 + 2 * i].float()
        mean = x + (g ** 2)[:, None, None, None] * score(x, bt) * dt
        x = mean + torch.sqrt(g ** 2 * dt)[:, None, None, None] * z
        x_mean = mean
        if known is not None:
            x_mean = hold(mean, known, mask)
            x = hold(x, known + float(lv["s_next"][i]) * z, mask)
    return x_mean


def heun_restatement(score, noise, n_steps, known=None, mask=None, **sched):
    """the Heun recurrence of edm_heun_sampler; held pixels follow known + sigma * noise[0] (the churn is not constrained)"""
    sch = SS.edm_heun_schedule(n_steps, SIG, 1e-3, **sched)
    c = lambda v: float(np.float32(v))  # noqa: E731
    B = noise[0].shape[0]
    z0 = noise[0].float()
    x = start(z0, c(sch["sigma"][0]), known, mask)
    for i in range(n_steps):
        sh, sn = c(sch["sigma_hat"][i]), c(sch["sigma"][i + 1])
        if sch["draws"] > 1:
            x = x + c(sch["churn_coef"][i]) * noise[1 + i].float()
        d = -sh * score(x, torch.full((B,), c(sch["t_hat"][i])))
        xp = x + (sn - sh) * d
        if known is not None:
            xp = hold(xp, known + sn * z0, mask)
        if i == n_steps - 1:
            return xp
        d2 = -sn * score(xp, torch.full((B,), c(sch["t_next"][i])))
        x = x + (sn - sh) * 0.5 * (d + d2)
        if known is not None:
            x = hold(x, known + sn * z0, mask)


def gaussian_score(s0):
    """score of Gaussian data of variance s0^2 under the VE SDE: pixel-independent, so free pixels cannot see held ones"""
    def f(x, t, y=None, c=None, l=None, tp=None):
        std = SS._ve_std(t.double().cpu().numpy(), SIG)
        var = torch.as_tensor(s0 ** 2 + std ** 2, device=x.device).view(-1, 1, 1, 1)
        return (-x.double() / var).to(x.dtype)
    return f
