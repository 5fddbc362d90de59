"""Exponential moving average of a ScoreNet's weights (`training.with_ema`, `training.ema_decay`).

After optimizer step n = 1, 2, ... every floating-point parameter and buffer e of the shadow model moves towards its live
counterpart p,
    e <- e + (1 - d_n) (p - e),      d_n = min(ema_decay, (1 + n) / (10 + n))
(the warm-up of score_sde's ExponentialMovingAverage: a short run's average does not stay near the random initialisation), and
integer buffers (`num_batches_tracked`) are copied.  n counts on the host and d_n goes to the kernel by value.

The update is csrc/optim.hip: for the native Adam / AdamW step it is an epilogue of the optimizer's one launch
(optim._NativeStep reads `optimizer.ema`), and the tensors that launch does not cover (buffers, parameters without a gradient this
step) ride on it as EMA-only descriptors.  Any other optimizer takes one EMA-only launch after its step (`update()`).
The shadow is a ScoreNet of its own (own native engines, no gradient arena), always in eval mode, with requires_grad off."""
from __future__ import annotations

import copy
import logging

import torch

from . import _native as N

logger = logging.getLogger(__name__)

# checkpoint keys next to the reference's {"network_params", "optimizer_params"}; written only with training.with_ema
EMA_KEY, EMA_COUNT_KEY = "ema_network_params", "ema_num_updates"


def pick_network_params(ckpt: dict, load_ema: bool, where: str = "checkpoint"):
    """the state_dict a model loads from checkpoint dict `ckpt`: the EMA weights when `load_ema` and the file has them, else
    `network_params` (with a warning when EMA weights were asked for)"""
    if load_ema:
        if EMA_KEY in ckpt:
            return ckpt[EMA_KEY]
        logger.warning(f"load_ema is set but {where} has no '{EMA_KEY}' (trained without training.with_ema?): loading 'network_params'")
    return ckpt["network_params"]


def decay_at(decay: float, n: int) -> float:
    """d_n of update n (1-based)"""
    return min(float(decay), (1.0 + n) / (10.0 + n))


class ModelEMA:
    def __init__(self, model, decay: float = 0.9999):
        if not 0.0 <= float(decay) <= 1.0:
            raise ValueError(f"ema_decay must lie in [0, 1], got {decay}")
        self.model, self.decay = model, float(decay)
        self.shadow = None
        self.num_updates = 0
        self.loaded = False            # state came from a checkpoint: training must not re-initialise it from the live weights
        self._pairs = None             # [(live, shadow, is_float)] over state_dict order, one entry per storage
        self._tables = {}

    # -- shadow -----------------------------------------------------------------------------------------------------
    def _make_shadow(self):
        self.shadow = copy.deepcopy(self.model)       # ScoreNet.__deepcopy__: no engines, no gradient arena
        for p in self.shadow.parameters():
            p.requires_grad_(False)
        self.shadow.eval()
        self._bind()

    def _bind(self):
        live, sh = self.model.state_dict(keep_vars=True), self.shadow.state_dict(keep_vars=True)
        if list(live) != list(sh):
            raise ValueError("EMA shadow and live model have different state_dict keys")
        pairs, seen = [], set()
        for k, p in live.items():
            if p.data_ptr() in seen:
                continue
            seen.add(p.data_ptr())
            pairs.append((p, sh[k], p.dtype.is_floating_point))
        self._pairs = pairs
        self._tables.clear()

    def reset(self):
        """shadow := the live weights, counter 0 (training start without a restored average)"""
        if self.shadow is None:
            self._make_shadow()
        else:
            with torch.no_grad():
                self.shadow.load_state_dict(self.model.state_dict())
            self._bind()
        self.num_updates, self.loaded = 0, False

    def start(self):
        """called when training (re)starts: initialise from the live weights unless an average exists already"""
        if self.shadow is None or (self.num_updates == 0 and not self.loaded):
            self.reset()
        else:
            self._bind()               # the live model's tensors may have moved since (load_state_dict(assign=True), .to())

    def state_dict(self):
        return {"network_params": self.shadow.state_dict() if self.shadow is not None else self.model.state_dict(),
                "num_updates": int(self.num_updates)}

    def load_state_dict(self, sd):
        if self.shadow is None:
            self._make_shadow()
        with torch.no_grad():
            self.shadow.load_state_dict(sd["network_params"])
        self.shadow.eval()
        self.num_updates, self.loaded = int(sd.get("num_updates", 0)), True
        self._bind()

    # -- the update ---------------------------------------------------------------------------------------------------
    def advance(self) -> float:
        """n += 1; returns 1 - d_n, the rate of this step's update"""
        self.num_updates += 1
        return 1.0 - decay_at(self.decay, self.num_updates)

    def shadow_ptr(self, p) -> int:
        """shadow storage of live parameter `p`"""
        sh = self._shadow_by_ptr().get(p.data_ptr())
        if sh is None:
            raise ValueError("a parameter the optimizer steps is not part of the model the EMA follows")
        return sh.data_ptr()

    def _shadow_by_ptr(self):
        m = self.__dict__.get("_by_ptr")
        if m is None or m[0] is not self._pairs:
            m = self._by_ptr = (self._pairs, {p.data_ptr(): e for p, e, _ in self._pairs})
        return m[1]

    def rest_rows(self, covered=frozenset()):
        """EMA-only descriptor rows (p, g=None, m=None, v=None, e, numel, mode) for every tensor whose live storage is not in
        `covered` (data pointers the optimizer launch averages itself).  mode 1: bit copy of an integer buffer (32-bit words)."""
        rows = []
        for p, e, is_float in self._pairs:
            if p.data_ptr() in covered:
                continue
            N.require_device(p, e)
            if not (p.is_contiguous() and e.is_contiguous()):
                raise N.NativeError("EMA needs contiguous parameters and buffers")
            if is_float:
                if p.dtype != torch.float32 or e.dtype != torch.float32:
                    raise N.NativeError(f"the native EMA averages fp32 tensors; got {p.dtype}")
                rows.append((p.data_ptr(), None, None, None, e.data_ptr(), p.numel(), 0))
            else:
                nbytes = p.numel() * p.element_size()
                if nbytes % 4 or e.dtype != p.dtype:
                    raise N.NativeError(f"EMA bit copy of a {p.dtype} buffer of {nbytes} bytes")
                rows.append((p.data_ptr(), None, None, None, e.data_ptr(), nbytes // 4, 1))
        return rows

    def table(self, cache_key, rows, dev):
        """(desc_dev, ema_dev, n, total_blocks) for descriptor rows; cached while the pointers stay the same"""
        key = tuple(rows)
        tab = self._tables.get(cache_key)
        if tab is None or tab[0] != key:
            lib, blk, descs = N.lib(), 0, []
            for p, g, m, v, _e, n, mode in rows:
                descs.append(N.AdamDesc(p, g, m, v, n, blk, mode))
                blk += lib.sbgm_adam_step_blocks(n)
            raw = (N.AdamDesc * len(descs))(*descs)
            d_dev = torch.frombuffer(bytearray(bytes(raw)), dtype=torch.uint8).to(dev)
            e_dev = torch.tensor([r[4] for r in rows], dtype=torch.int64).to(dev)
            tab = self._tables[cache_key] = (key, d_dev, e_dev, len(rows), blk)
        return tab[1:]

    def launch_rest(self, rate: float, covered=frozenset()):
        """EMA-only launch over everything not in `covered`"""
        rows = self.rest_rows(covered)
        if rows:
            d_dev, e_dev, n, blk = self.table("rest", rows, self.shadow_device())
            N.check(N.lib().sbgm_ema_update_batched(d_dev.data_ptr(), e_dev.data_ptr(), n, blk, float(rate), N.stream()))
        N.bump_generation()            # the shadow was written through raw pointers (no version-counter bump)

    def shadow_device(self):
        return self._pairs[0][1].device

    @torch.no_grad()
    def update(self):
        """one EMA update after an optimizer step that did not average anything itself (SGD, torch's own Adam step)"""
        if self.shadow is None:
            self.reset()
        self.launch_rest(self.advance())
