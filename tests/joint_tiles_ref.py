"""Host restatements of joint full-domain sampling around any `score(tiles, t)`: ONE Euler-Maruyama, predictor-corrector
or EDM Heun recurrence over a DOMAIN state X [1, 1, Hd, Wd_pad] whose score is, at every evaluation, the stitch-weighted blend of the
tiles' scores: cut tiles (`oracle.tiler_ref.extract`), evaluate, blend (`oracle.tiler_ref.stitch`).  Noise is the domain draw of
`philox_ref.domain_draw` at the offsets of DESIGN.md §4.4; the step scalars and the order of operations are those of constrained_ref.py, so a
one-tile domain reproduces the plain recurrences bit for bit.  `known` / `mask` are domain fields [1, 1, Hd, Wd_pad]."""
import numpy as np
import torch

from oracle import tiler_ref as OT
from oracle import torch_ref as O
from sbgm_danra_amd import score_sampling as SS
from sbgm_danra_amd.tiling import axis_origins

import constrained_ref as R
import philox_ref as P

SIG = R.SIG


class Geometry:
    """the tile table of FullDomainTiler(domain_hw, tile, halo), computed without a device"""

    def __init__(self, domain_hw, tile, halo):
        self.Hd, self.Wd, self.tile, self.overlap = int(domain_hw[0]), int(domain_hw[1]), int(tile), 2 * int(halo)
        self.Wd_pad = self.Wd + (-(self.Wd - self.tile)) % 4
        self.R = max(1, self.overlap)
        ys = axis_origins(self.Hd, self.tile, self.overlap)
        xs = axis_origins(self.Wd_pad, self.tile, self.overlap, align=4)
        self.origins = [(y, x) for y in ys for x in xs]

    def __len__(self):
        return len(self.origins)

    def pad(self, dom):
        """[..., Hd, Wd] -> [..., Hd, Wd_pad], right edge replicated (FullDomainTiler._pad)"""
        return dom if self.Wd_pad == self.Wd else torch.cat([dom, dom[..., -1:].expand(*dom.shape[:-1], self.Wd_pad - self.Wd)], -1)

    def extract(self, dom):
        """torch [C, Hd, Wd_pad] -> [T, C, tile, tile]"""
        return torch.from_numpy(OT.extract(dom.numpy(), self.origins, self.tile))

    def stitch(self, tiles):
        """torch [T, C, tile, tile] -> [C, Hd, Wd_pad]"""
        return torch.from_numpy(OT.stitch(tiles.numpy(), self.origins, self.Hd, self.Wd_pad, self.R))

    def coverage(self):
        """[Hd, Wd_pad] int: how many tiles cover each domain pixel"""
        n = np.zeros((self.Hd, self.Wd_pad), np.int64)
        for y, x in self.origins:
            n[y:y + self.tile, x:x + self.tile] += 1
        return n


def domain_noise(seed, offset, geo):
    """draw `offset` of a tiled run as a float32 [1, 1, Hd, Wd_pad] tensor"""
    return torch.from_numpy(P.domain_draw(seed, offset, geo.Hd, geo.Wd_pad)).float()[None, None]


def tile_noise(seed, n_draws, geo):
    """[n_draws, T, 1, tile, tile]: what the tiles of a tiled run see of draws 0 .. n_draws-1 (the `noise=` of an independent-tile
    restatement with the same domain-keyed noise)"""
    return torch.stack([geo.extract(domain_noise(seed, d, geo)[0]) for d in range(n_draws)])


def blended_score(score, X, t, geo):
    """(s* [1, 1, Hd, Wd_pad], raw tile scores [T, 1, tile, tile]) of the domain state X at time t"""
    tiles = geo.extract(X[0])
    raw = score(tiles, torch.full((len(geo),), float(t)))
    return geo.stitch(raw.float())[None], raw


def crop(X, geo):
    return X[0, :, :, :geo.Wd].contiguous()


def em_joint(score, seed, n_steps, geo, known=None, mask=None, eps=1e-3):
    """constrained_ref.em_restatement on the domain, with the blended score; draws 0, 1 + i"""
    ones = torch.ones(1)
    lv = SS.sde_hold_levels("em", n_steps, SIG, eps)
    x = R.start(domain_noise(seed, 0, geo), O.marginal_prob_std(ones)[:, None, None, None], known, mask)
    ts = torch.linspace(1.0, eps, n_steps)
    dt = ts[0] - ts[1]
    mean_x = x
    for i, tt in enumerate(ts):
        g = O.diffusion_coeff(ones * tt)
        z = domain_noise(seed, 1 + i, geo)
        mean = x + (g ** 2)[:, None, None, None] * blended_score(score, x, tt, geo)[0] * dt
        x = mean + torch.sqrt(dt) * g[:, None, None, None] * z
        mean_x = mean
        if known is not None:
            mean_x = R.hold(mean, known, mask)
            x = R.hold(x, known + float(lv["s_next"][i]) * z, mask)
    return crop(mean_x, geo)


def pc_joint(score, seed, n_steps, geo, known=None, mask=None, snr=0.16, eps=1e-3):
    """constrained_ref.pc_restatement on the domain: the corrector's step size is the batch-mean rule over the RAW tile scores with
    prod(x.shape[1:]) = tile^2, its update uses the blended score; draws 0, 1 + 2i (corrector), 2 + 2i (predictor)"""
    ones = torch.ones(1)
    T = len(geo)
    lv = SS.sde_hold_levels("pc", n_steps, SIG, eps)
    x = R.start(domain_noise(seed, 0, geo), O.marginal_prob_std(ones)[:, None, None, None], known, mask)
    ts = np.linspace(1.0, eps, n_steps)
    dt = ts[0] - ts[1]
    x_mean = x
    for i, tt in enumerate(ts):
        bt = ones * tt
        grad, raw = blended_score(score, x, tt, geo)
        gnorm = torch.norm(raw.reshape(T, -1), dim=-1).mean()
        lstep = 2 * (snr * np.sqrt(np.prod(raw.shape[1:])) / gnorm) ** 2
        z = domain_noise(seed, 1 + 2 * i, geo)
        x = x + lstep * grad + torch.sqrt(2 * lstep) * z
        if known is not None:
            x = R.hold(x, known + float(lv["s_cur"][i]) * z, mask)
        g = O.diffusion_coeff(bt)
        z = domain_noise(seed, 2 + 2 * i, geo)
        mean = x + (g ** 2)[:, None, None, None] * blended_score(score, x, tt, geo)[0] * dt
        x = mean + torch.sqrt(g ** 2 * dt)[:, None, None, None] * z
        x_mean = mean
        if known is not None:
            x_mean = R.hold(mean, known, mask)
            x = R.hold(x, known + float(lv["s_next"][i]) * z, mask)
    return crop(x_mean, geo)


def heun_joint(score, seed, n_steps, geo, known=None, mask=None, **sched):
    """constrained_ref.heun_restatement on the domain: both slopes from the blended score; draw 0, churn draws 1 + i"""
    sch = SS.edm_heun_schedule(n_steps, SIG, 1e-3, **sched)
    c = lambda v: float(np.float32(v))  # noqa: E731
    z0 = domain_noise(seed, 0, geo)
    x = R.start(z0, c(sch["sigma"][0]), known, mask)
    for i in range(n_steps):
        sh, sn = c(sch["sigma_hat"][i]), c(sch["sigma"][i + 1])
        if sch["draws"] > 1:
            x = x + c(sch["churn_coef"][i]) * domain_noise(seed, 1 + i, geo)
        d = -sh * blended_score(score, x, c(sch["t_hat"][i]), geo)[0]
        xp = x + (sn - sh) * d
        if known is not None:
            xp = R.hold(xp, known + sn * z0, mask)
        if i == n_steps - 1:
            return crop(xp, geo)
        d2 = -sn * blended_score(score, xp, c(sch["t_next"][i]), geo)[0]
        x = x + (sn - sh) * 0.5 * (d + d2)
        if known is not None:
            x = R.hold(x, known + sn * z0, mask)
