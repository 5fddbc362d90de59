"""`SampleGenerator` — reference sbgm/evaluate_sbgm/generation.py:40-314 (its live part): draws a batch, runs
`pc_sampler` with the reference's kwargs, squeezes / moves to CPU exactly like `_run_sampler` (:56-83) and saves
`gen_samples_* / eval_samples_* / lsm_samples_* / seasons_*` npz files.  Plotting and the stats-file back-transforms
are out of scope.  With an `evaluation.ensemble_products` section, `generate_repeated` also writes
`ens_products_*`: the per-pixel mean, spread, envelope, quantile and exceedance-probability maps of its members, computed on
the device (verification.ensemble_products).  `generate_series` (no reference counterpart) downscales the whole generation
split in loader order, `evaluation.series.members` samples per day, into `*_series_n_<D>` files; with an `evaluation.full_domain`
section the days are whole domains, sampled through `tiling.FullDomainTiler.sample_series` (`_generate_domain_series`).

Deliberate deviation: the reference writes `self.model.eval` without calling it, so its generation
runs BatchNorm in training mode.  Here `eval()` IS called; pass `literal_reference_bn=True` to reproduce the
reference's behaviour (the engine supports train-mode BatchNorm in the sampler)."""
from __future__ import annotations

import logging
import os

import numpy as np
import torch

from .. import calendar, parallel
from .. import verification as V
from ..resident_data import full_domain_config
from ..score_sampling import (NOISE_MAX_LAGS, dpm_sampler_kwargs, dpmpp_2m_sampler, edm_heun_sampler, edm_sampler_kwargs, fresh_seed,
                              noise_weights_f32, ode_sampler_kwargs, pc_sampler, rk45_sampler, temporal_noise_acf, temporal_noise_weights)
from ..score_unet import diffusion_coeff_fn, marginal_prob_std_fn
from ..utils import extract_any, get_model_string
from .evaluation import ensemble_products_config

logger = logging.getLogger(__name__)


def constraint_mask(cfg, hw):
    """The [H,W] float32 mask of the optional top-level `constraint:` section, or None when it is absent or `enabled` is false.
    `mask_file`: an .npy file of shape [H,W] (values in [0,1]); else `station_fraction` (default 0.01) with `seed` (default 0): a
    seeded Bernoulli mask, the same for every sample of a run.  The batch's true high-resolution field is held where it is set."""
    sec = (cfg.get("constraint") if hasattr(cfg, "get") else None) or {}
    if not sec.get("enabled", False):
        return None
    if cfg["sampler"].get("sampler_type") == "rk45_sampler":
        raise ValueError("constraint.enabled: rk45_sampler does not take known pixels (use pc_sampler, edm_heun_sampler or dpmpp_2m_sampler)")
    H, W = int(hw[0]), int(hw[1])
    if sec.get("mask_file"):
        mask = np.load(sec["mask_file"]).astype(np.float32)
        if mask.shape != (H, W):
            raise ValueError(f"constraint.mask_file holds {mask.shape}, the samples are {(H, W)}")
        return mask
    frac = float(sec.get("station_fraction", 0.01))
    if not 0.0 <= frac <= 1.0:
        raise ValueError(f"constraint.station_fraction={frac} must be in [0, 1]")
    return (np.random.default_rng(int(sec.get("seed", 0))).random((H, W)) < frac).astype(np.float32)


def series_config(cfg):
    """(members, max_days) of the optional evaluation.series section: `members` >= 1 samples per day (default 1), `max_days` >= 1
    or null (default: the whole generation split).  The section's other two keys, `seed` and `temporal_noise`, are read by
    `series_noise_config`, `calendar_origin` by `series_calendar`."""
    sec = cfg["evaluation"].get("series") or {}
    if not hasattr(sec, "keys") or not set(sec.keys()) <= {"members", "max_days", "seed", "temporal_noise", "calendar_origin"}:
        raise ValueError(f"evaluation.series takes the keys 'members', 'max_days', 'seed', 'temporal_noise' and 'calendar_origin' only, "
                         f"got {sec!r}")
    members, max_days = sec.get("members", 1), sec.get("max_days")
    if isinstance(members, bool) or not isinstance(members, int) or members < 1:
        raise ValueError(f"evaluation.series.members must be an integer >= 1, got {members!r}")
    if max_days is not None and (isinstance(max_days, bool) or not isinstance(max_days, int) or max_days < 1):
        raise ValueError(f"evaluation.series.max_days must be null or an integer >= 1, got {max_days!r}")
    return members, max_days


def series_noise_config(cfg):
    """(seed, weights) of the optional keys `seed` and `temporal_noise` of evaluation.series, (None, None) when neither is there.
    `seed`: an integer in [0, 2^63), the one Philox seed of the whole series (None here: `generate_series` draws one).
    `temporal_noise`: {rho, lags} (weights proportional to rho^k, `score_sampling.temporal_noise_weights`) or {weights: [...]} (1..32
    numbers whose squares sum to 1 within 1e-5); without it the weights are [1.0], white noise keyed by day."""
    sec = cfg["evaluation"].get("series") or {}
    if not hasattr(sec, "keys") or ("seed" not in sec.keys() and "temporal_noise" not in sec.keys()):
        return None, None
    seed = sec.get("seed")
    if seed is not None and (isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 63):
        raise ValueError(f"evaluation.series.seed must be null or an integer in [0, 2^63), got {seed!r}")
    tn = sec.get("temporal_noise")
    if tn is None:
        return seed, np.ones(1, dtype=np.float32)
    if not hasattr(tn, "keys") or set(tn.keys()) not in ({"rho", "lags"}, {"weights"}):
        raise ValueError(f"evaluation.series.temporal_noise takes either the keys 'rho' and 'lags' or the key 'weights', got {tn!r}")
    if "weights" in tn.keys():
        return seed, noise_weights_f32(tn["weights"], "evaluation.series.temporal_noise.weights")
    rho, lags = tn["rho"], tn["lags"]
    if isinstance(rho, bool) or not isinstance(rho, (int, float)) or not -1.0 < rho < 1.0:
        raise ValueError(f"evaluation.series.temporal_noise.rho must be a number in (-1, 1), got {rho!r}")
    if isinstance(lags, bool) or not isinstance(lags, int) or not 1 <= lags <= NOISE_MAX_LAGS:
        raise ValueError(f"evaluation.series.temporal_noise.lags must be an integer in 1..{NOISE_MAX_LAGS}, got {lags!r}")
    return seed, temporal_noise_weights(rho, lags)


def series_calendar(cfg, dataloader):
    """the calendar origin (an int day number) of a series whose generation split has dates, else None: the optional
    evaluation.series.calendar_origin (an int day number or "YYYY-MM-DD"), by default the first date of the split's file.  The key
    without dates in the file is refused."""
    sec = cfg["evaluation"].get("series") or {}
    origin = sec.get("calendar_origin") if hasattr(sec, "get") else None
    origin = None if origin is None else calendar.parse_origin(origin)
    dates = getattr(getattr(dataloader, "fields", None), "dates", None)
    if dates is None:
        if origin is not None:
            raise ValueError("evaluation.series.calendar_origin is set, but the generation split's file has no `dates`")
        return None
    return int(dates[0]) if origin is None else origin


class _SeriesDates:
    """the dates of the batches of a series, in the order served: absolute days for the noise rows, strictly increasing dates"""

    def __init__(self, origin):
        self.origin, self.dates = origin, []

    def days(self, batch_dates):
        """int64 [B] absolute days n_d = date - origin of one batch"""
        dates = np.asarray(batch_dates, np.int64)
        n = calendar.series_days(np.concatenate([self.dates[-1][-1:], dates]) if self.dates else dates, self.origin)
        self.dates.append(dates)
        return n[1:] if len(self.dates) > 1 else n

    def index(self):
        return {"dates": np.concatenate(self.dates), "calendar_origin": np.int64(self.origin)}


def maybe_inverse_transform(k, arr, back_transforms):
    """reference generation.py:26-35"""
    if back_transforms and k in back_transforms:
        return back_transforms[k](arr)
    return arr


class SampleGenerator:
    def __init__(self, cfg, model, dataloader, back_transforms, device, literal_reference_bn: bool = False):
        self.cfg, self.model, self.dataloader, self.back_transforms, self.device = cfg, model, dataloader, back_transforms, device
        self.model.train() if literal_reference_bn else self.model.eval()
        self.model_name_str = get_model_string(cfg)
        self.output_dir = os.path.join(cfg["paths"]["sample_dir"], "generation", self.model_name_str)
        self.sample_path = os.path.join(self.output_dir, "generated_samples")
        os.makedirs(self.sample_path, exist_ok=True)
        self.full_domain = full_domain_config(cfg)                   # raises here, at start, on what a domain series does not do
        hw = cfg["highres"]["data_size"]
        hw = (hw[0], hw[0])
        if self.full_domain is not None:                             # the samples are whole domains: the mask has the domain's shape
            if parallel.world()[1] > 1:
                raise ValueError(f"evaluation.full_domain runs on one rank, got {parallel.world()[1]}: sharded days would break the "
                                 "day order of the series")
            hw = getattr(dataloader, "domain_hw", None)
            if hw is None:
                raise ValueError("evaluation.full_domain needs the loader of whole days (resident_data.ResidentDomainLoader, what "
                                 f"get_gen_dataloader builds for the section), got {type(dataloader).__name__}")
            self.full_domain = full_domain_config(cfg, hw)
        self.constraint = constraint_mask(cfg, hw)                   # raises here, at start, on a sampler that cannot hold pixels
        self.products = ensemble_products_config(cfg)                # likewise on a malformed evaluation.ensemble_products section

    def _sample_device(self, batch_size, y, cond_img, lsm_cond, topo_cond, known=None, noise_plan=None):
        """the sampler output as [B,H,W] still on the device (what _run_sampler returns after .cpu()).  pc_sampler, as in the
        reference, unless cfg.sampler.sampler_type is "edm_heun_sampler": then n_timesteps is its Heun step count N (2N-1
        network evaluations; 18-64 is the intended range) and the optional `edm:` section sets the sigma ladder; "dpmpp_2m_sampler":
        n_timesteps is its step count N (N evaluations) and the optional `dpm:` section sets the ladder, eta and s_noise; or "rk45_sampler":
        the adaptive ODE solver, which ignores n_timesteps and reads its tolerances from the optional `ode:` section.
        With a `constraint:` section, `known` (the batch's true field, model space) is held on the section's mask.
        `noise_plan`: the seed and noise-row arguments of a series (`generate_series`), passed to the sampler as they are."""
        held = dict(noise_plan or {})                      # the plan and the constraint compose: both go to the sampler
        if self.constraint is not None and known is not None:
            held.update(known=known.reshape(-1, 1, *known.shape[-2:]).expand(batch_size, -1, -1, -1),
                        known_mask=torch.from_numpy(self.constraint))
        if self.cfg["sampler"].get("sampler_type") == "edm_heun_sampler":
            gen = edm_heun_sampler(score_model=self.model, marginal_prob_std=marginal_prob_std_fn, diffusion_coeff=diffusion_coeff_fn,
                                   batch_size=batch_size, num_steps=self.cfg["sampler"]["n_timesteps"], device=self.device,
                                   img_size=self.cfg["highres"]["data_size"][0], y=y, cond_img=cond_img, lsm_cond=lsm_cond,
                                   topo_cond=topo_cond, **edm_sampler_kwargs(self.cfg), **held)
        elif self.cfg["sampler"].get("sampler_type") == "dpmpp_2m_sampler":
            gen = dpmpp_2m_sampler(score_model=self.model, marginal_prob_std=marginal_prob_std_fn, diffusion_coeff=diffusion_coeff_fn,
                                   batch_size=batch_size, num_steps=self.cfg["sampler"]["n_timesteps"], device=self.device,
                                   img_size=self.cfg["highres"]["data_size"][0], y=y, cond_img=cond_img, lsm_cond=lsm_cond,
                                   topo_cond=topo_cond, **dpm_sampler_kwargs(self.cfg), **held)
        elif self.cfg["sampler"].get("sampler_type") == "rk45_sampler":
            gen = rk45_sampler(score_model=self.model, marginal_prob_std=marginal_prob_std_fn, diffusion_coeff=diffusion_coeff_fn,
                               batch_size=batch_size, device=self.device, img_size=self.cfg["highres"]["data_size"][0], y=y,
                               cond_img=cond_img, lsm_cond=lsm_cond, topo_cond=topo_cond, **ode_sampler_kwargs(self.cfg), **(noise_plan or {}))
        else:
            gen = pc_sampler(score_model=self.model, marginal_prob_std=marginal_prob_std_fn, diffusion_coeff=diffusion_coeff_fn,
                             batch_size=batch_size, num_steps=self.cfg["sampler"]["n_timesteps"], device=self.device,
                             img_size=self.cfg["highres"]["data_size"][0], y=y, cond_img=cond_img, lsm_cond=lsm_cond,
                             topo_cond=topo_cond, **held)
        gen = gen.squeeze().detach()
        if gen.ndim == 4:
            gen = gen.squeeze(1)
        elif gen.ndim == 2:
            gen = gen.unsqueeze(0)
        elif gen.ndim != 3:
            raise ValueError(f"Unknown generated sample shape: {gen.shape}")
        return gen

    def _run_sampler(self, batch_size, y, cond_img, lsm_cond, topo_cond):
        """reference generation.py:56-83: [B,H,W] on the host"""
        return self._sample_device(batch_size, y, cond_img, lsm_cond, topo_cond).cpu()

    def _apply_backtransforms(self, x, generated, cond_images, seasons=None):
        """reference generation.py:85-107, on the device: the transforms are elementwise, so one launch per key covers the
        whole batch (the reference loops over samples and stacks).  cond_images comes back as the reference's nested list
        [sample][variable] of [H,W] tensors."""
        hr_key = self.cfg["highres"]["variable"] + "_hr"
        if generated.ndim == 2:
            generated = generated.unsqueeze(0)
        x = maybe_inverse_transform(hr_key, x, self.back_transforms)
        generated = maybe_inverse_transform(hr_key, generated, self.back_transforms)
        if cond_images is not None:
            keys = self.cfg["lowres"]["condition_variables"] or []
            per_var = [maybe_inverse_transform(k + "_lr", cond_images[:, i], self.back_transforms) for i, k in enumerate(keys)]
            cond_images = [[v[b] for v in per_var] for b in range(cond_images.shape[0])]
        return x, generated, cond_images

    def _generate(self, x, seasons, cond, lsm, topo, suffix, batch=None, products=None):
        gen = self._sample_device(x.shape[0] if batch is None else batch, seasons, cond, lsm, topo, known=x)
        cond_out = cond
        if self.cfg["evaluation"].get("transform_back", False):
            x, gen, cond_out = self._apply_backtransforms(x, gen, cond, seasons)
        if products is not None:
            self._save_products(gen, products, suffix)
        gen = gen.cpu()
        self._save_npz({"gen_samples": gen, "eval_samples": x, "lsm_samples": lsm, "seasons": seasons,
                        "constraint_mask": self.constraint}, suffix)
        if cond_out is not None and isinstance(cond_out, list):
            for i, k in enumerate(self.cfg["lowres"]["condition_variables"] or []):
                self._save_npz({f"cond_samples_{k}": torch.stack([im[i] for im in cond_out])}, suffix)
        return gen

    def _save_products(self, gen, products, suffix):
        """ens_products_<suffix>.npz: the products of the members gen [M,H,W] (on the device, in the units of the gen_samples
        file), without a mask"""
        quantiles, thresholds = products
        r = V.ensemble_products(gen, quantiles, thresholds)
        arrays = {k: r[k].cpu().numpy() for k in ("mean", "std", "min", "max", "quantiles", "exceed_prob")}
        np.savez_compressed(os.path.join(self.sample_path, f"ens_products_{suffix}.npz"), **arrays,
                            quantile_levels=np.asarray(quantiles, dtype=np.float64),
                            thresholds=np.asarray(thresholds, dtype=np.float64), members=np.int64(gen.shape[0]))

    def _save_npz(self, data, suffix):
        for k, v in data.items():
            if v is not None:
                np.savez_compressed(os.path.join(self.sample_path, f"{k}_{suffix}.npz"), v.cpu().numpy() if torch.is_tensor(v) else v)

    def _batch(self, first_only=False):
        x, seasons, cond, _lsm_hr, lsm, _sdf, topo, _hp, _lp = extract_any(next(iter(self.dataloader)), self.device)
        if first_only:
            x, seasons, cond, lsm, topo = [None if t is None else t[:1] for t in (x, seasons, cond, lsm, topo)]
        return x, seasons, cond, lsm, topo

    @staticmethod
    def _rank_suffix():
        """with several ranks every rank owns whole batches and writes its own files (two ranks writing one path would race)"""
        rank, world = parallel.world()
        return f"_rank{rank}" if world > 1 else ""

    def generate_multiple(self):
        x, seasons, cond, lsm, topo = self._batch()
        return self._generate(x, seasons, cond, lsm, topo, f"multi_n_{x.shape[0]}" + self._rank_suffix())

    def generate_single(self):
        x, seasons, cond, lsm, topo = self._batch(first_only=True)
        return self._generate(x, seasons, cond, lsm, topo, "single" + self._rank_suffix())

    def generate_series(self):
        """the whole generation split, day by day: every batch of the loader in loader order, M = evaluation.series.members
        (default 1) samples per day, up to evaluation.series.max_days days (default: all).  A batch of B days is one sampler
        call with B * M rows — each day's conditions repeated M times, independent noise per row — through _sample_device, so
        the sampler type, guidance and the `constraint:` section act as for `multiple`.  Writes gen_samples_series_n_<D>
        [D, M, H, W], eval_samples_series_n_<D> [D, H, W], lsm_samples_ / seasons_ as for `multiple`, and series_index_series_n_<D>
        with `members` and, when the batches carry them, `hr_points`.  The days keep the loader's order; several ranks would
        interleave it, so they are refused.

        With `evaluation.series.seed` or `.temporal_noise` (`series_noise_config`) the noise is keyed by day instead of by batch: every
        batch runs under the ONE series seed with `noise_rows = (d + K - 1) M + m` for member m of the absolute day d (counted over
        the loader), `noise_row_stride = M` and the K weights, so the draws of member m on day d are the moving average of the white
        draws of days d .. d-K+1 (lag-j autocorrelation `temporal_noise_acf(weights)[j]`, members mutually independent), each still
        N(0,1).  A day's noise then does not depend on the loader's batch size or on `max_days`, and a series can be reproduced or
        extended; `seed`, `weights` and `acf` go into the index file.  When the generation split's file has `dates`, d is the day's
        date minus the calendar origin (`series_calendar`) instead of its position: the day after a gap of g days is coupled to the
        day before it at acf[g], a date's noise depends on (seed, origin, date, m) only, and `dates` and `calendar_origin` go into
        the index file; the dates served must be strictly increasing.  With or without dates the rows come from `calendar.noise_rows`, which
        refuses a row beyond int32 here, before the sampler would.  Rows are keyed by position in the crop: the coupling means
        something for a fixed crop (`sample_w_cutouts: false`) on consecutive days.  `pc_sampler`'s Langevin step still uses the
        batch-mean score norm, so its result, unlike its noise, depends on a day's batch-mates.  Without the two keys nothing changes."""
        if self.full_domain is not None:
            return self._generate_domain_series()
        members, max_days = series_config(self.cfg)
        seed, weights = series_noise_config(self.cfg)
        if weights is not None and seed is None:
            seed = fresh_seed()                            # one seed for the whole series, written to the index file
        if parallel.world()[1] > 1:
            raise ValueError("gen_type 'series' runs on one rank: sharded days would interleave in the rank files and break the "
                             "day order")
        origin = series_calendar(self.cfg, self.dataloader)
        cal = None if origin is None else _SeriesDates(origin)
        gens, truths, lsms, seas, points, days = [], [], [], [], [], 0
        rep = lambda t: None if t is None else t.repeat_interleave(members, dim=0)   # noqa: E731
        for batch in self.dataloader:
            if max_days is not None and days >= max_days:
                break
            x, seasons, cond, _lsm_hr, lsm, _sdf, topo, hp, _lp = extract_any(batch, self.device)
            if max_days is not None and days + x.shape[0] > max_days:
                keep = max_days - days
                x, seasons, cond, lsm, topo, hp = [None if t is None else t[:keep] for t in (x, seasons, cond, lsm, topo, hp)]
            B = x.shape[0]
            plan = None
            absolute = np.arange(days, days + B) if cal is None else cal.days(batch["dates"][:B])
            if weights is not None:
                plan = {"seed": seed, "noise_rows": calendar.noise_rows(absolute, len(weights), members), "noise_row_stride": members,
                        "noise_weights": weights}
            gen = self._sample_device(B * members, rep(seasons), rep(cond), rep(lsm), rep(topo), known=rep(x), noise_plan=plan)
            if self.cfg["evaluation"].get("transform_back", False):
                x, gen, _ = self._apply_backtransforms(x, gen, None, seasons)
            gens.append(gen.reshape(B, members, *gen.shape[-2:]).cpu())
            truths.append(x.reshape(B, *x.shape[-2:]).cpu())
            for store, t in ((lsms, lsm), (seas, seasons), (points, hp)):
                if t is not None:
                    store.append(t.cpu() if torch.is_tensor(t) else torch.as_tensor(np.asarray(t)))
            days += B
        if not days:
            raise ValueError("gen_type 'series': the generation loader gave no day")
        cat = lambda parts: torch.cat(parts) if parts else None   # noqa: E731
        suffix = f"series_n_{days}"
        gen = torch.cat(gens)
        self._save_npz({"gen_samples": gen, "eval_samples": cat(truths), "lsm_samples": cat(lsms), "seasons": cat(seas),
                        "constraint_mask": self.constraint}, suffix)
        index = {"members": np.int64(members)}
        if weights is not None:
            index.update(seed=np.int64(seed), weights=np.asarray(weights, dtype=np.float32), acf=temporal_noise_acf(weights))
        if len(points) == len(gens):
            index["hr_points"] = cat(points).numpy()
        if cal is not None:
            index.update(cal.index())
        np.savez_compressed(os.path.join(self.sample_path, f"series_index_{suffix}.npz"), **index)
        return gen

    def _domain_sampler(self):
        """(sampler, its keywords) of a domain series: the dispatch of `_sample_device` without rk45_sampler (refused at start)"""
        kind = self.cfg["sampler"].get("sampler_type")
        if kind == "edm_heun_sampler":
            return edm_heun_sampler, edm_sampler_kwargs(self.cfg)
        if kind == "dpmpp_2m_sampler":
            return dpmpp_2m_sampler, dpm_sampler_kwargs(self.cfg)
        return pc_sampler, {}

    def _generate_domain_series(self):
        """`generate_series` with an evaluation.full_domain section: the loader (`ResidentDomainLoader`) serves whole days of the
        generation split, already padded for the tiler, and every batch of days runs through `FullDomainTiler.sample_series`: M =
        evaluation.series.members fields per day, tiled or joint as the section says.  A domain series is always keyed by day: the ONE
        seed and the weights are those of `series_noise_config` (a fresh seed and [1.0] without the keys), and a batch passes the absolute
        index of its first day, so member m of day d is drawn as noise row (d + K - 1) M + m whatever evaluation.batch_size, `first_day`
        and `max_days` are; when the split's file has `dates`, d is the date minus the calendar origin (`series_calendar`) and `dates` and
        `calendar_origin` go into the index file.  With a `constraint:` section the day's truth is held on the [Hd, Wd] mask.  The host arrays are allocated
        once and filled batch by batch; the files hold the Wd real columns, the pad never leaves the device.  lsm_samples holds the one
        static plane, [1, 2, Hd, Wd]."""
        from ..tiling import FullDomainTiler
        fd, loader = self.full_domain, self.dataloader
        members, max_days = series_config(self.cfg)
        seed, weights = series_noise_config(self.cfg)
        weights = np.ones(1, dtype=np.float32) if weights is None else weights
        seed = fresh_seed() if seed is None else seed
        Hd, Wd = loader.domain_hw
        tiler = FullDomainTiler((Hd, Wd), fd["tile"], fd["halo"], device=self.device)
        if tiler.Wd_pad != loader.Wp or loader.first_day != fd["first_day"]:
            raise ValueError(f"evaluation.full_domain: the loader serves width {loader.Wp} from day {loader.first_day}, the section's "
                             f"tiler works on {tiler.Wd_pad} from day {fd['first_day']}")
        D = loader.n_days if max_days is None else min(loader.n_days, max_days)
        origin = series_calendar(self.cfg, loader)
        cal = None if origin is None else _SeriesDates(origin)
        sampler, kw = self._domain_sampler()
        back = self.cfg["evaluation"].get("transform_back", False)
        hr_key = self.cfg["highres"]["variable"] + "_hr"
        mask = None if self.constraint is None else torch.from_numpy(self.constraint).to(self.device)[None]
        gen, truth = torch.empty(D, members, Hd, Wd), torch.empty(D, Hd, Wd)      # the series is held once, on the host
        lsm_plane, seas, done = None, [], 0
        for batch in loader:
            if done >= D:
                break
            x, seasons, cond, _lsm_hr, lsm, _sdf, topo, _hp, _lp = extract_any(batch, self.device)
            B = min(x.shape[0], D - done)
            x = x[:B, 0, :, :Wd].contiguous()                                      # the truth, without the pad
            when = (dict(first_day=fd["first_day"] + done) if cal is None
                    else dict(day_numbers=cal.days(batch["dates"][:B]).tolist()))   # by position, or by date
            out = tiler.sample_series(self.model, sampler, marginal_prob_std_fn, diffusion_coeff_fn, self.cfg["sampler"]["n_timesteps"],
                                      cond_img=None if cond is None else cond[:B], lsm_cond=None if lsm is None else lsm[0],
                                      topo_cond=None if topo is None else topo[0], y=None if seasons is None else seasons[:B].tolist(),
                                      members=members, seed=seed, temporal_noise_weights=weights, days=B, **when,
                                      tiles_per_batch=fd["tiles_per_batch"], known=None if mask is None else x[:, None],
                                      known_mask=mask, joint=fd["joint"], **kw)
            if back:
                x, out = (maybe_inverse_transform(hr_key, t, self.back_transforms) for t in (x, out))
            gen[done:done + B].copy_(out)
            truth[done:done + B].copy_(x)
            if seasons is not None:
                seas.append(seasons[:B].cpu())
            if lsm is not None and lsm_plane is None:
                lsm_plane = lsm[:1, :, :, :Wd].cpu()
            done += B
        if done != D:
            raise ValueError(f"gen_type 'series': the generation loader gave {done} of {D} days")
        suffix = f"series_n_{D}"
        self._save_npz({"gen_samples": gen, "eval_samples": truth, "lsm_samples": lsm_plane, "seasons": torch.cat(seas) if seas else None,
                        "constraint_mask": self.constraint}, suffix)
        index = {"members": np.int64(members), "seed": np.int64(seed), "weights": np.asarray(weights, dtype=np.float32),
                 "acf": temporal_noise_acf(weights), "first_day": np.int64(fd["first_day"]), "domain_hw": np.asarray([Hd, Wd], dtype=np.int64),
                 "tile": np.int64(fd["tile"]), "halo": np.int64(fd["halo"]), "joint": np.bool_(fd["joint"]),
                 "tile_origins": np.asarray(tiler.origins, dtype=np.int64),
                 "hr_points": np.tile(np.asarray([0, Hd, 0, Wd], dtype=np.int64), (D, 1))}
        if cal is not None:
            index.update(cal.index())
        np.savez_compressed(os.path.join(self.sample_path, f"series_index_{suffix}.npz"), **index)
        return gen

    def generate_repeated(self):
        """cfg.evaluation.n_repeats samples from ONE conditioning sample, drawn as one batch (independent noise per
        row); with several ranks the repeats are independent units and are sharded, no collective.  With an
        evaluation.ensemble_products section every rank also writes the products of its own members (at least 2)."""
        products = self.products
        x, seasons, cond, lsm, topo = self._batch(first_only=True)
        n = int(self.cfg["evaluation"]["n_repeats"])
        rank, world = parallel.world()
        mine = len(parallel.shard_range(n, rank, world))
        if products is not None and mine == 1:
            raise ValueError(f"evaluation.ensemble_products needs at least 2 members per rank; rank {rank} of {world} draws 1 of "
                             f"n_repeats={n}")
        rep = lambda t: None if t is None else t.repeat(mine, *([1] * (t.dim() - 1)))   # noqa: E731
        if not mine:
            return None
        return self._generate(x, rep(seasons), rep(cond), rep(lsm), rep(topo),
                              f"repeated_n_{n}" + (f"_rank{rank}" if world > 1 else ""), batch=mine, products=products)
