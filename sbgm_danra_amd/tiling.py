"""Full-domain sampling by overlapping tiles (BASELINE config 5: a 589x789 DANRA field as 256x256
tiles with halo).  The reference holds only the domain dimensions (config/full_run_config_new.yaml:26,28) — no tiling,
halo or stitching code exists there, so this module has no reference counterpart; its specification is DESIGN.md §9:

* tile origins: per axis n = ceil((L - overlap) / (tile - overlap)) tiles, first at 0, last flush with the domain edge,
  the rest evenly spread (x origins rounded down to multiples of 4: the in-kernel noise is drawn in quads);
* conditioning fields are cut into tiles on the device (`sbgm_extract_tiles`), the tiles are one sampler batch;
* the sampler's in-kernel noise is keyed by DOMAIN position (`tile_origins` of `sbgm_sampler_run`), so the pixels two tiles
  share see identical noise in both and differ only through their receptive-field context;
* `sbgm_stitch_tiles` blends the tiles with linear ramps over the overlap, normalised per pixel (a partition of unity).

Multi-GPU: tiles are independent units -> rank r samples tiles r::world with no collective during sampling; one
all-reduce of the finished tiles (every tile is written by exactly one rank, the others hold zeros) precedes the stitch.
The result does NOT depend on the world size or on `tiles_per_batch`: with `tile_origins` the Langevin step size of a
tile uses that tile's own score norm (csrc/sampler.hip; the reference's batch-mean rule, score_sampling.py:201, is for
batches of independent samples), the noise is keyed by domain position and everything else in the network is per
sample in eval mode.

Joint sampling (`sample(..., joint=True)`): ONE diffusion over the domain instead of T that share their noise.  All
tiles run as one batch and every update kernel reads the stitch-weighted blend of the tiles' scores (`joint_tiles` of the samplers),
so all copies of a domain pixel stay bit-equal through the run and the stitch has nothing left to average: no band of smoother
texture over the overlaps.  One rank, one batch; `pc_sampler` then uses the batch-mean Langevin step size over the tiles.

Series (`sample(..., noise_row=)`, `sample_series`): the domain noise plan keys the domain-keyed noise by a noise
row as well (one row for all tiles: they are one field on one day) and mixes it over the preceding rows, so the fields of consecutive
days are correlated as the weights say and a day's field depends on (seed, day, member) alone.
"""
from __future__ import annotations

import math

import torch

from . import _native as N
from . import parallel


def axis_origins(length: int, tile: int, overlap: int, align: int = 1):
    if tile >= length:
        if tile > length:
            raise ValueError(f"tile {tile} larger than the domain extent {length}")
        return [0]
    if not 0 <= overlap < tile:
        raise ValueError(f"overlap {overlap} must be in [0, tile)")
    n = max(2, math.ceil((length - overlap) / (tile - overlap)))
    last = length - tile
    out = []
    for i in range(n):
        o = round(i * last / (n - 1))
        if 0 < i < n - 1 or align > 1:
            o = (o // align) * align
        out.append(o)
    if align > 1 and out[-1] != last:          # keep the domain covered: add a final tile flush with the edge when rounding fell short
        if last % align == 0:
            out[-1] = last
        else:
            raise ValueError(f"domain extent {length} - tile {tile} = {last} is not a multiple of {align}; pad the domain")
    return out


def padded_width(Wd: int, tile: int) -> int:
    """the width the tile table works on: Wd padded on the right until Wd_pad - tile is a multiple of 4 (the x origins are noise quads)"""
    return int(Wd) + (-(int(Wd) - int(tile))) % 4


class FullDomainTiler:
    """Tile table + device gather/blend kernels for one (domain, tile, halo) geometry."""

    def __init__(self, domain_hw, tile: int = 256, halo: int = 32, device="cuda"):
        self.Hd, self.Wd = int(domain_hw[0]), int(domain_hw[1])
        self.tile, self.halo, self.overlap = int(tile), int(halo), 2 * int(halo)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise N.NativeError(f"FullDomainTiler runs on a ROCm device, got device={device!r}")
        ys = axis_origins(self.Hd, self.tile, self.overlap)
        xs = self._x_origins()
        self.origins = [(y, x) for y in ys for x in xs]
        self.origins_dev = torch.tensor(self.origins, dtype=torch.int32, device=self.device).contiguous()
        self._origin_tables = {}

    def _x_origins(self):
        # x origins must be multiples of 4 (noise quads).  The last tile has to end at the domain edge, so when
        # Wd - tile is not a multiple of 4 the tile table works on a domain padded on the right to the next multiple.
        self.Wd_pad = padded_width(self.Wd, self.tile)
        return axis_origins(self.Wd_pad, self.tile, self.overlap, align=4)

    def __len__(self):
        return len(self.origins)

    def _origins_of(self, idx):
        """the origins of the tiles `idx` as one device table, kept per batch: the captured step's key holds its address, so the days of
        a series replay one step instead of capturing one each"""
        key = tuple(int(i) for i in idx)
        if key not in self._origin_tables:
            self._origin_tables[key] = self.origins_dev[list(key)].contiguous()
        return self._origin_tables[key]

    def _pad(self, dom):
        """[C, Hd, Wd] -> [C, Hd, Wd_pad], right edge replicated (only when Wd - tile is not a multiple of 4)"""
        if self.Wd_pad == self.Wd:
            return dom
        return torch.nn.functional.pad(dom, (0, self.Wd_pad - self.Wd), mode="replicate")

    def extract(self, domain: torch.Tensor, which=None) -> torch.Tensor:
        """domain [C, Hd, Wd] (device) -> tiles [T, C, tile, tile]; `which` = tile indices (default all).  A domain that is already
        [C, Hd, Wd_pad] (right edge replicated by its producer, `sbgm_domain_gather`) is cut as it is, without the pad's copy."""
        N.require_device(domain)
        if domain.dim() != 3 or domain.shape[1] != self.Hd or domain.shape[2] not in (self.Wd, self.Wd_pad):
            raise ValueError(f"domain tensor {tuple(domain.shape)} does not match the tiler's [C, {self.Hd}, {self.Wd}]"
                             + ("" if self.Wd_pad == self.Wd else f" or its padded [C, {self.Hd}, {self.Wd_pad}]"))
        dom = N.f32c(domain.float() if domain.shape[2] == self.Wd_pad else self._pad(domain.float()))
        C = dom.shape[0]
        org = self.origins_dev if which is None else self.origins_dev[list(which)].contiguous()
        T = org.shape[0]
        tiles = torch.empty(T, C, self.tile, self.tile, device=dom.device)
        N.check(N.lib().sbgm_extract_tiles(dom.data_ptr(), org.data_ptr(), tiles.data_ptr(), T, C, self.Hd, self.Wd_pad, self.tile,
                                           self.tile, N.stream()))
        return tiles

    def stitch(self, tiles: torch.Tensor) -> torch.Tensor:
        """tiles [T, C, tile, tile] (all tiles, table order) -> domain [C, Hd, Wd]"""
        N.require_device(tiles)
        tiles = N.f32c(tiles)
        T, C = tiles.shape[:2]
        if T != len(self.origins) or tiles.shape[2] != self.tile or tiles.shape[3] != self.tile:
            raise ValueError(f"expected {len(self.origins)} tiles of {self.tile}x{self.tile}, got {tuple(tiles.shape)}")
        dom = torch.empty(C, self.Hd, self.Wd_pad, device=tiles.device)
        N.check(N.lib().sbgm_stitch_tiles(tiles.data_ptr(), self.origins_dev.data_ptr(), dom.data_ptr(), T, C, self.Hd, self.Wd_pad,
                                          self.tile, self.tile, max(1, self.overlap), N.stream()))
        return dom[:, :, : self.Wd].contiguous() if self.Wd_pad != self.Wd else dom

    def sample(self, score_model, sampler, marginal_prob_std, diffusion_coeff, num_steps, cond_img=None, lsm_cond=None,
               topo_cond=None, y=None, seed=None, tiles_per_batch=None, known=None, known_mask=None, joint=False,
               noise_row=None, noise_weights=None, noise_row_stride=1, **sampler_kw) -> torch.Tensor:
        """Sample the whole domain: cond_img [C,Hd,Wd] / lsm_cond, topo_cond [2,Hd,Wd] / y scalar class -> [1,Hd,Wd].
        Each condition may instead come pre-padded, [.., Hd, Wd_pad] (`extract`; what `ResidentDomainLoader` serves); `known`,
        `known_mask` and the result are always Wd wide.  Tiles are sharded over the ranks of the process group (if any) and, per rank, run in batches of
        `tiles_per_batch`; every batch shares `seed`, so the domain-keyed noise is identical wherever tiles overlap.
        `known`, `known_mask` [1,Hd,Wd] (constrained sampling, see `pc_sampler`): cut into tiles like the conditions and passed to
        the sampler; after the stitch the hold is applied once more against the domain fields, so the result equals `known` on the
        mask bit for bit and not just to the rounding of the blend.
        `joint=True`: one diffusion over the domain (the sampler's `joint_tiles`): all tiles in one batch on one rank, the tiles'
        scores blended at every step, so the tiles agree bit for bit wherever they overlap and the stitch only assembles them.
        `noise_row` (int), `noise_weights`, `noise_row_stride`: the domain noise plan (the samplers' `noise_domain_row` with
        `domain_height = Hd`): the field is drawn as noise row `noise_row` of the stream `seed`, mixed over the rows
        `noise_row - k * noise_row_stride` with the weights, whatever `tiles_per_batch` and `joint` are.  `sample_series` uses it."""
        import inspect
        from .score_sampling import _fresh_seed, _prep_noise_domain
        _, world = parallel.world()
        if noise_row is None:
            if noise_weights is not None or int(noise_row_stride) != 1:
                raise ValueError("FullDomainTiler.sample: noise_weights and noise_row_stride need noise_row (the row they mix)")
        else:
            if "noise_domain_row" not in inspect.signature(sampler).parameters:
                raise ValueError(f"FullDomainTiler.sample: {getattr(sampler, '__name__', sampler)} does not take noise_row (a domain noise "
                                 "plan is served by the step samplers)")
            try:                                         # every host check before the first batch, under the tiler's argument name
                _prep_noise_domain(noise_row, self.Hd, noise_weights, noise_row_stride, self.tile, "FullDomainTiler.sample", tile_origins=True)
            except ValueError as e:
                raise ValueError(str(e).replace("noise_domain_row", "noise_row")) from None
            sampler_kw = dict(sampler_kw, noise_domain_row=int(noise_row), domain_height=self.Hd, noise_weights=noise_weights,
                              noise_row_stride=noise_row_stride)
        if joint:
            if "joint_tiles" not in inspect.signature(sampler).parameters:
                raise ValueError(f"FullDomainTiler.sample: {getattr(sampler, '__name__', sampler)} does not take joint_tiles (the per-sample "
                                 "step controllers of the adaptive samplers would let the copies of a pixel drift)")
            if tiles_per_batch is not None and tiles_per_batch < len(self):
                raise ValueError(f"FullDomainTiler.sample: a joint run needs all {len(self)} tiles in one batch, got tiles_per_batch="
                                 f"{tiles_per_batch}")
            if world > 1:
                raise ValueError("FullDomainTiler.sample: a joint run blends the scores of all tiles at every step and cannot be split "
                                 f"over {world} ranks; let each rank sample whole domains instead")
            sampler_kw = dict(sampler_kw, joint_tiles=(self.Hd, max(1, self.overlap)))
        if (known is None) != (known_mask is None):
            raise ValueError("FullDomainTiler.sample: known and known_mask must be given together")
        held = {}
        if known is not None:
            if "known" not in inspect.signature(sampler).parameters:
                raise ValueError(f"FullDomainTiler.sample: {getattr(sampler, '__name__', sampler)} does not take known / known_mask")
            known, known_mask = (N.f32c(torch.as_tensor(f).to(self.device)) for f in (known, known_mask))
            for f, name in ((known, "known"), (known_mask, "known_mask")):
                if tuple(f.shape) != (1, self.Hd, self.Wd):
                    raise ValueError(f"FullDomainTiler.sample: {name} {tuple(f.shape)} must be [1, {self.Hd}, {self.Wd}]")
            held = {"known": known, "known_mask": known_mask}
        seed = _fresh_seed() if seed is None else seed
        if world > 1:                                  # one seed for the whole domain
            import torch.distributed as dist
            s = torch.tensor([seed], dtype=torch.int64, device=self.device)
            dist.broadcast(s, 0)
            seed = int(s.item())
        def run_batch(idx):
            cut = lambda f: None if f is None else self.extract(f, idx)   # noqa: E731
            yb = None if y is None else torch.full((len(idx),), int(y), dtype=torch.int64, device=self.device)
            steps = {} if num_steps is None else {"num_steps": num_steps}      # None: an adaptive sampler (rk45_sampler) has no step count
            return sampler(score_model, marginal_prob_std, diffusion_coeff, batch_size=len(idx), **steps,
                           device=self.device, img_size=self.tile, y=yb, cond_img=cut(cond_img), lsm_cond=cut(lsm_cond),
                           topo_cond=cut(topo_cond), seed=seed, tile_origins=self._origins_of(idx),
                           domain_width=self.Wd_pad, **{k: cut(f) for k, f in held.items()}, **sampler_kw)
        out = sample_tiles_sharded(len(self), run_batch, (1, self.tile, self.tile), self.device, tiles_per_batch)
        dom = self.stitch(out)
        if known is not None:                          # hold(dom, known, m): a select where m is 0 or 1
            m = known_mask.clamp(0.0, 1.0)
            dom = torch.where(m <= 0, dom, torch.where(m >= 1, known, (1.0 - m) * dom + m * known))
        return dom

    def sample_series(self, score_model, sampler, marginal_prob_std, diffusion_coeff, num_steps, cond_img=None, lsm_cond=None,
                      topo_cond=None, y=None, members=1, seed=None, temporal_noise_weights=None, first_day=None, days=None,
                      tiles_per_batch=None, known=None, known_mask=None, joint=False, day_numbers=None, **sampler_kw) -> torch.Tensor:
        """A series of full-domain fields: cond_img [D,C,Hd,Wd] (one condition per day; or None with `days=D`) -> [D, members, Hd, Wd].
        The whole series runs under ONE `seed`, and member m of day d is drawn as the domain noise row (first_day + d + K - 1) * members
        + m with stride `members` (K = len(temporal_noise_weights), default [1.0]: white in time), the row convention of the cutout
        series (`generate_series`): consecutive days of a member share K - 1 white rows and correlate with `temporal_noise_acf(w)[1]`,
        members are independent, and a day's field depends on (seed, first_day + d, m) only, not on the call that made it, so a series
        can be extended (`first_day`) or one day regenerated.  `day_numbers` (instead of `first_day`; giving both is an error): a list
        of `days` non-negative ints, the absolute day of each field, e.g. its date minus the calendar origin of the series; day d is
        then drawn as row (day_numbers[d] + K - 1) * members + m, so the day after a gap of g days correlates with the day before
        it at `temporal_noise_acf(w)[g]`.  `lsm_cond`, `topo_cond` [2,Hd,Wd] and a scalar `y` are shared by the
        days; `y` may also hold D classes, `known` / `known_mask` [1,Hd,Wd] are shared or [D,1,Hd,Wd] per day; `joint`,
        `tiles_per_batch` and the sampler's keywords act as in `sample`."""
        from .score_sampling import _fresh_seed, noise_weights_f32
        if first_day is not None and day_numbers is not None:
            raise ValueError("FullDomainTiler.sample_series: give first_day or day_numbers, not both")
        members, first_day = int(members), int(first_day or 0)
        if members < 1:
            raise ValueError(f"FullDomainTiler.sample_series: members={members} must be >= 1")
        if first_day < 0:
            raise ValueError(f"FullDomainTiler.sample_series: first_day={first_day} must be >= 0")
        if cond_img is not None:
            if cond_img.dim() != 4 or (days is not None and int(days) != cond_img.shape[0]):
                raise ValueError(f"FullDomainTiler.sample_series: cond_img {tuple(cond_img.shape)} must be [days, C, {self.Hd}, {self.Wd}]"
                                 + ("" if days is None else f" with days={days}"))
            days = cond_img.shape[0]
        if days is None or int(days) < 1:
            raise ValueError(f"FullDomainTiler.sample_series: days={days!r} must be >= 1 (or given through cond_img [days, C, Hd, Wd])")
        days = int(days)
        w = noise_weights_f32([1.0] if temporal_noise_weights is None else temporal_noise_weights,
                              "FullDomainTiler.sample_series: temporal_noise_weights")
        what = f"day_numbers up to {max(day_numbers)}" if day_numbers is not None and len(day_numbers) else f"first_day={first_day}"
        if day_numbers is None:
            day_numbers = range(first_day, first_day + days)
        day_numbers = [int(n) for n in day_numbers]
        if len(day_numbers) != days or min(day_numbers) < 0:
            raise ValueError(f"FullDomainTiler.sample_series: day_numbers must hold {days} non-negative integers, got {day_numbers}")
        last = (max(day_numbers) + w.size - 1) * members + members - 1
        if last > 0x7FFFFFFF:
            raise ValueError(f"FullDomainTiler.sample_series: {what} puts the last noise row at {last}, beyond int32")
        known, known_mask = (None if f is None else torch.as_tensor(f) for f in (known, known_mask))
        per_day = lambda f, d, lead: None if f is None else (f[d] if f.dim() == lead + 1 else f)   # noqa: E731
        if y is not None and not isinstance(y, int) and len(y) != days:
            raise ValueError(f"FullDomainTiler.sample_series: y must be one class or {days} classes, got {len(y)}")
        seed = _fresh_seed() if seed is None else seed
        out = torch.empty(days, members, self.Hd, self.Wd, device=self.device)
        for d in range(days):
            for m in range(members):
                out[d, m] = self.sample(score_model, sampler, marginal_prob_std, diffusion_coeff, num_steps,
                                        cond_img=None if cond_img is None else cond_img[d], lsm_cond=lsm_cond, topo_cond=topo_cond,
                                        y=y if y is None or isinstance(y, int) else int(y[d]), seed=seed, tiles_per_batch=tiles_per_batch,
                                        known=per_day(known, d, 3), known_mask=per_day(known_mask, d, 3), joint=joint,
                                        noise_row=(day_numbers[d] + w.size - 1) * members + m, noise_weights=w, noise_row_stride=members,
                                        **sampler_kw)[0]
        return out


def sample_tiles_sharded(n_tiles: int, run_batch, tile_shape, device, tiles_per_batch=None) -> torch.Tensor:
    """Deal `n_tiles` independent tiles round-robin over the ranks of the process group (rank r owns tiles r::world), run this
    rank's tiles through `run_batch(list of tile indices) -> [len, *tile_shape]` in batches of `tiles_per_batch`, and merge:
    every tile is written by exactly one rank, the others hold zeros, so ONE sum all-reduce leaves all tiles on every rank.
    No collective runs while the tiles are being sampled."""
    rank, world = parallel.world()
    mine = list(range(n_tiles))[rank::world]
    per = tiles_per_batch or max(1, len(mine))
    out = torch.zeros(n_tiles, *tile_shape, device=device)
    for i in range(0, len(mine), per):
        idx = mine[i:i + per]
        out[idx] = run_batch(idx)
    if world > 1:
        import torch.distributed as dist
        dist.all_reduce(out)
    return out
