"""Training path: the ScoreNet forward as a graph of native ops with hand-written HIP backward kernels.

Inference and sampling run the whole network inside the C++ engine (`sbgm_model_forward`).  Training needs every
intermediate for `loss.backward()` (reference training.py:403-405), so here the same launch sequence is issued op by
op through the per-op C ABI, each op wrapped in a `torch.autograd.Function` whose forward AND backward are HIP
kernels from libsbgm_hip.so (conv data-gradient = the forward implicit-GEMM kernel on transposed/flipped weights,
conv weight-gradient = MFMA GEMM over pixels, norm / attention / upsample / time-embedding backward kernels in
csrc/backward.hip).  PyTorch contributes the autograd tape, tensor storage and `torch.optim`; no torch.nn op is called.

Activations are NHWC fp32 tensors `[B, H, W, C]`; parameters stay in the reference layouts (OIHW etc.) and are
repacked per step (they change every optimizer step).  Semantics follow the reference in train mode: BatchNorm uses
batch statistics and updates `running_mean/var/num_batches_tracked` (momentum 0.1, unbiased variance).
"""
from __future__ import annotations

import ctypes as C
import weakref

import torch

from . import _native as N

_L = N.lib
_ACT = {"ReLU": N.RELU, "SiLU": N.SILU, "GELU": N.GELU, "Identity": N.NONE}


def _st():
    return N.stream()


def _pad_c(c):
    return 4 if c <= 4 else 8 if c <= 8 else (c + 15) // 16 * 16


_TILES = {}            # conv geometry -> (tile_co, tile_px, splits, waves_per_tile, winograd bits), found by sbgm_conv2d_tune
_SPLITK = {}           # device -> split-K scratch (16 Mi floats), shared by every convolution (stream-ordered)
_SPLITK_FLOATS = 16 << 20

# debugging switches
_USE_ARENA = [True]    # False = every gradient in a fresh tensor (the pre-arena behaviour)
_USE_SLOTS = [True]    # False = every fork summed by autograd (the pre-slot behaviour)
_USE_WINO = [True]     # False = the training convolutions never use the Winograd kernels
_BATCH_WGRAD = [True]  # queue the small weight-gradient GEMMs of a backward sweep for one batched launch (sbgm_wgrad_defer bit 1)
_DEFER_UNPACK = [True]  # queue the slab -> OIHW layout passes of a backward sweep for one launch at its end (sbgm_wgrad_defer bit 0)


def _zero_(t):
    """t.zero_() with the library's own kernel (no at::native fill on the hot path; capture-safe); host tensors: t.zero_()"""
    if not t.is_cuda:
        return t.zero_()
    if t.numel():
        N.check(_L().sbgm_fill_zero(t.data_ptr(), t.numel() * t.element_size(), _st()))
    return t


def _splitk_ws(dev):
    ws = _SPLITK.get(dev)
    if ws is None:
        ws = _SPLITK[dev] = torch.empty(_SPLITK_FLOATS, device=dev)
    return ws


# ---- per-step pools --------------------------------------------------------------------------------------------------------
# Backward scratch that is accumulated with atomics (weight-gradient slabs, norm-backward sums) comes out of ONE buffer that
# is zeroed once per step; slices are handed out sequentially and never reused before the next forward, so every
# slice is still zero when its kernel runs (a second backward through the same graph simply takes fresh slices).
# Only the part that was handed out is re-zeroed: everything past the step's offset is still zero from the allocation.  Under
# stream capture the zeroing is recorded with a fixed extent (the high-water mark of earlier steps); slices past it come from
# fresh tensors, so a replay never sees a stale slab.
# Gradients that are accumulated with atomics and RETURNED to autograd (conv biases, LayerNorm gamma/beta, time-bias sums, the
# weights of 1x1 convolutions / linears) are slices of a second pool: a fresh zeroed tensor per step, so a slice that lives on as
# some parameter's .grad is never touched by a later step (unlike the scratch pool, which is re-zeroed in place).
_ZERO_FLOATS = 32 << 20
_GRAD_FLOATS = 4 << 20


class _Pool:
    """bump allocator over one zeroed fp32 tensor, slices aligned to 64 floats"""
    __slots__ = ("buf", "off", "high_water", "extent", "replayed")

    def __init__(self, buf):
        self.buf, self.off, self.high_water, self.extent, self.replayed = buf, 0, 0, buf.numel(), False

    def take(self, n):
        """n zeroed floats: (a slice of the pool, True -> the launcher may skip its own memset) or (a fresh tensor, False)"""
        end = self.off + (n + 63) // 64 * 64
        if end > self.extent:
            return torch.zeros(n, device=self.buf.device), False
        out = self.buf[self.off: self.off + n]
        self.off = end
        if end > self.high_water:
            self.high_water = end
        return out, True

    def rezero(self, capturing):
        """the scratch pool's step: same buffer (captured steps hold its address), dirty prefix zeroed in place"""
        self.replayed = self.replayed or capturing      # replays of captured steps dirty the pool behind Python's back: from then on
        dirty = self.high_water if self.replayed else self.off      # the whole high-water prefix is re-zeroed, not just the last step's
        if dirty:
            _zero_(self.buf[:dirty])
        self.extent = self.high_water if capturing else self.buf.numel()
        self.off = 0

    def renew(self):
        """the returned-gradient pool's step: a new zeroed tensor (slices of the old one may live on as .grad)"""
        self.buf, self.off = _zero_(torch.empty_like(self.buf)), 0


# ---- gradient arena ------------------------------------------------------------------------------------------------------
# Every parameter gradient of a model lives in ONE flat fp32 tensor: the backward kernels write (or atomically accumulate) a
# parameter's gradient straight into its slice, `p.grad` ends up as a view of that slice, so the data-parallel exchange is ONE
# all-reduce over the flat tensor with no gather / scatter copies (parallel.GradientBucket adopts it) and the native Adam step
# reads the same memory.  The arena is zeroed once per step by _Step.begin.  It is used when every `p.grad` is None at the start
# of the step (`optimizer.zero_grad()` default); with live gradients (accumulation over several backward calls) the kernels
# write fresh tensors and autograd adds them, exactly as before.
class GradArena:
    def __init__(self, net):
        self.params = [p for p in net.parameters() if p.requires_grad]
        self.index, off = {}, 0
        for p in self.params:
            self.index[p.data_ptr()] = (off, p.numel())
            off += (p.numel() + 63) // 64 * 64
        self.numel = off
        self.flat = torch.zeros(off, dtype=torch.float32, device=self.params[0].device)
        self.sig = self.signature(net)
        self.claimed = set()

    @staticmethod
    def signature(net):
        return tuple(p.data_ptr() for p in net.parameters() if p.requires_grad)

    def begin_step(self):
        _zero_(self.flat)
        self.claimed.clear()

    def view(self, t):
        """slice for parameter tensor `t` (the parameter itself or a same-size view of it), once per step; else None"""
        e = self.index.get(t.data_ptr())
        if e is None or e[1] != t.numel() or e[0] in self.claimed:
            return None
        self.claimed.add(e[0])
        return self.flat[e[0]: e[0] + e[1]].view(t.shape)

    def grad_of(self, p):
        off, n = self.index[p.data_ptr()]
        return self.flat[off: off + n].view(p.shape)


_WGRAD_LOG = [None]             # bench.py: when a list, ConvFn.backward appends the geometry of every weight gradient it launches


def arena_for(net, create=True):
    """the model's gradient arena (rebuilt when a parameter moved: .to(), load_state_dict(assign=True))"""
    a = getattr(net, "_grad_arena", None)
    if a is not None and a.sig != GradArena.signature(net):
        a = None
    if a is None and create:
        a = GradArena(net)
        object.__setattr__(net, "_grad_arena", a)
    return a


def _in_arena(arena, t):
    if arena is None or t is None:
        return False
    a = arena.flat.data_ptr()
    return a <= t.data_ptr() < a + arena.flat.numel() * 4


def _pgrad(arena, like, zeroed):
    """storage for the gradient of parameter tensor `like`: (tensor shaped like it, True if it is known to be zero).
    From the arena when one is active and the slice was not handed out yet this step, else a pooled / fresh tensor."""
    if arena is not None:
        v = arena.view(like)
        if v is not None:
            return v, True
    if zeroed:
        g, z = _STEP.zeros(like.numel(), like.device, True)
        return g.view(like.shape), z
    return torch.empty_like(like), False


# Test instrumentation: when a list, every BatchNorm(+ReLU) forward appends the ReLU decision its backward will use
# (relu output > 0, [B, H, W, C] bool).  tests/test_gpu_configs.py evaluates its float64 reference under the SAME decisions: a
# pre-activation within rounding distance of zero otherwise routes its gradient differently in two arithmetics, and one such flip
# moves an encoder weight gradient by ~1e-2.
_RELU_TRACE = [None]

# ---- gradient slots ------------------------------------------------------------------------------------------------------
# A forward tensor with several consumers (the residual forks of the BasicBlocks and attention half-blocks, the feature maps that
# feed both the next encoder layer and a decoder skip) receives the SUM of its consumers' gradients.  Left to autograd that is one
# at::native add launch per fork (20 per training step, ~5 us each at batch 8).  A slot lets the consumers sum inside their own
# backward kernels: every consumer's backward takes the partial sum collected so far, folds it into its own kernel (the data
# gradient convolution adds it in its epilogue as a residual, LayerNorm's backward takes it as dx_add) and either parks the new
# partial sum in the slot (returning None to autograd) or, when it is the last consumer, returns the total.  Consumers may run in
# any order; an incomplete slot at the end of the backward pass raises.
class _GradSlot:
    __slots__ = ("n", "left", "acc")

    def __init__(self, n):
        self.n, self.left, self.acc = n, n, None

    def take(self, like=None):
        a, self.acc = self.acc, None
        return a if (a is None or like is None) else a.view(like.shape)

    def give(self, g):
        _STEP.at_backward_end()                              # the incomplete-slot check
        self.left -= 1
        if self.left > 0:
            self.acc = g
            return None
        self.left = self.n                                   # re-armed: a second backward over a retained graph works the same way
        return g


def _slot(n):
    if not _USE_SLOTS[0] or n < 2:
        return None
    sl = _GradSlot(n)
    _STEP.slots.append(sl)
    return sl


def _fold(slot, g):
    """hand gradient `g` of a slotted input to the slot, from a consumer whose kernel has no fused-add path"""
    if slot is None:
        return g
    extra = slot.take(g)
    if extra is not None:
        g = g + extra                                        # ran late: one torch add
    return slot.give(g)


# SyncBatchNorm: statistics summed over the ranks of the process group, see BNTrainFn
_SYNC_BN = [False]


def set_sync_batchnorm(on: bool):
    prev = _SYNC_BN[0]
    _SYNC_BN[0] = bool(on)
    return prev


def _sync_world():
    import torch.distributed as dist
    if _SYNC_BN[0] and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        return dist
    return None


# ---- the step ------------------------------------------------------------------------------------------------------------
class _Step:
    """Everything that lives for one forward + backward.  `begin` is the only place that resets it; forward_train, the stand-alone
    sub-module calls and tests that drive single ops all start there.  Deliberately older than a step: the scratch pool's buffer
    (captured steps hold its address), a model's _PackPlan and GradArena, the tile cache _TILES and the split-K scratch."""

    def __init__(self):
        self.pools = {}            # device -> (scratch pool, returned-gradient pool)
        self.arena = None          # the GradArena the gradients of this step go to, or None
        self.plan = None           # the _PackPlan whose images this step's convolutions read, or None
        self.slots = []            # every _GradSlot of this step
        self.queued = False        # the end-of-backward callback is queued
        self.keep = []             # (dy, x) of the weight-gradient GEMMs queued for the batched launch: alive until the flush has enqueued them
        self.nbt = []              # num_batches_tracked of every train-mode BatchNorm of the forward: one increment at its end, not 20
        self.sync_count = None     # SyncBatchNorm: total batch size over the ranks (a python int)

    def begin(self, dev, net=None):
        """start a step on `dev`; net: the model whose whole forward this is (its plan and, when every p.grad is None, its arena
        become active), None: a stand-alone call, neither"""
        if _L().sbgm_wgrad_flush_pending():           # a backward pass that raised before its end-of-pass callback: its queued layout
            _L().sbgm_wgrad_discard()                 # passes point at gradient tensors that may be freed by now -- drop them unrun
        self.slots.clear()
        self.keep.clear()
        self.nbt.clear()
        self.queued = False                           # (autograd drops the queued callback of a backward pass that raised)
        self.plan = self.arena = self.sync_count = None
        pools = self.pools.get(dev)
        if pools is None:
            pools = self.pools[dev] = (_Pool(torch.zeros(_ZERO_FLOATS, device=dev)), _Pool(torch.empty(_GRAD_FLOATS, device=dev)))
        pools[0].rezero(dev.type == "cuda" and torch.cuda.is_current_stream_capturing())
        pools[1].renew()
        if net is not None:
            self.plan = _plan_for(net)
            if _USE_ARENA[0] and all(p.grad is None for p in net.parameters()):      # fresh step: gradients go straight into the model's flat arena
                self.arena = arena_for(net)
                self.arena.begin_step()

    def zeros(self, n, dev, returned=False):
        """n zeroed floats of backward scratch, or (returned) for a gradient that is handed to autograd; see _Pool.take"""
        pools = self.pools.get(dev)
        return pools[returned].take(n) if pools is not None else (torch.zeros(n, device=dev), False)

    def bump_nbt(self):
        if self.nbt:
            with torch.no_grad():
                torch._foreach_add_(list(self.nbt), 1)
            self.nbt.clear()

    def flush_wgrad(self):
        """run the weight-gradient work queued so far (also called mid-pass by _BucketBoundary)"""
        try:
            if _L().sbgm_wgrad_flush_pending():
                N.check(_L().sbgm_wgrad_flush(_st()))
        finally:
            self.keep.clear()

    def at_backward_end(self):
        """queue the end-of-backward work (once per pass)"""
        if not self.queued:
            try:
                torch.autograd.Variable._execution_engine.queue_callback(self._backward_end)
                self.queued = True
            except RuntimeError:                             # not inside a backward pass (a direct .backward() call on the Function):
                self.flush_wgrad()                           # nothing to wait for, and no pass whose slots could be checked

    def _backward_end(self):
        self.queued = False
        self.flush_wgrad()
        bad = [sl for sl in self.slots if sl.left != sl.n]   # untouched (no consumer needed the gradient) or completed: fine
        for sl in bad:
            sl.left, sl.acc = sl.n, None
        if bad:
            raise RuntimeError(f"{len(bad)} gradient slot(s) were left incomplete by the backward pass: a consumer of a shared tensor did not "
                               f"run its backward (partial graph?); set train_graph._USE_SLOTS[0] = False")


_STEP = _Step()
_zero_reset = _STEP.begin      # the name tests that drive single ops know for "begin a stand-alone step on `dev`"


# Slab -> OIHW layout passes of the weight gradients are queued during a backward pass and run as one launch at its end
# (autograd's end-of-pass callback).  Only slabs from the step's pool are queued: they stay alive and untouched until the next
# forward.  Until the callback has run, the affected `.grad` views hold zeros (gradient hooks on conv weights would see that).
class _deferred_unpack:
    """`on`: the slab -> OIHW pass of this call may wait for the end of the backward sweep; `gemm`: so may the weight-gradient GEMM itself
    (sbgm_wgrad_defer bit 1: the small per-tap GEMMs of a sweep run as one batched launch) — `keep` = the tensors it reads, held until then"""
    def __init__(self, on, gemm=False, keep=()):
        self.mask = ((1 if on else 0) | (2 if gemm else 0)) if _DEFER_UNPACK[0] else 0
        self.on = self.mask != 0
        self.keep = keep if (self.mask & 2) else ()

    def __enter__(self):
        if self.on:
            self.prev = _L().sbgm_wgrad_defer(self.mask)
            if self.keep:
                _STEP.keep.append(self.keep)

    def __exit__(self, *exc):
        if self.on:
            _L().sbgm_wgrad_defer(self.prev)
            if not _STEP.queued and _L().sbgm_wgrad_flush_pending():
                _STEP.at_backward_end()


class _prezeroed:
    """`with _prezeroed(flag):` tells the backward launchers that their scratch arrives zeroed (skips ~75 memsets per step)"""
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.prev = _L().sbgm_set_scratch_prezeroed(1) if self.on else None

    def __exit__(self, *exc):
        if self.on:
            _L().sbgm_set_scratch_prezeroed(self.prev)


# Conv / linear weights change every optimizer step and are needed twice per step (forward operator and data-gradient
# operator).  The first forward records which weights are used and how; from then on ONE batched launch at the start of
# forward_train packs all of them (sbgm_conv_pack_weights_batched) instead of ~90 single-weight launches.
class _PackPlan:
    def __init__(self):
        self.entries = {}          # (data_ptr, cs) -> dict(w_shape, cs, dgrad, fwd=tensor, bwd=tensor|None)
        self.desc = None           # device descriptor table
        self.keep = []             # superseded tables (still referenced by captured steps)
        self.dirty = False         # entries / layouts were added since the table was built
        self.sig = None
        self.blocks = 0
        self.fresh = False
        self.owner = lambda: None

    def note(self, w, cs, dgrad, layout):
        """layout 'g' / 'w' / 'd': the tuned forward kernel of this call read the implicit-GEMM / the Winograd F(2,3) / the Winograd
        F(2x2,3x3) weight image.  One weight
        may be needed in both (two batch shapes whose tuned tiles differ): every layout ever used is packed from then on."""
        key = (w.data_ptr(), cs)
        e = self.entries.get(key)
        if e is None:
            base = w._base if w._base is not None else w
            e = self.entries[key] = dict(shape=tuple(w.shape), cs=cs, dgrad=False, ref=weakref.ref(base), need=set(),
                                         img={(r_, l_): None for r_ in ("fwd", "bwd") for l_ in ("g", "w", "d")})
            self.dirty = True
        if dgrad and not e["dgrad"]:
            e["dgrad"] = True
            self.dirty = True
        if ("fwd", layout) not in e["need"]:
            e["need"].add(("fwd", layout))
            self.dirty = True

    def note_bwd(self, w, cs, layout):
        e = self.entries.get((w.data_ptr(), cs))
        if e is not None and ("bwd", layout) not in e["need"]:
            e["need"].add(("bwd", layout))
            e["dgrad"] = True
            self.dirty = True

    def lookup(self, w, cs):
        e = self.entries.get((w.data_ptr(), cs)) if self.fresh else None
        return e if e is not None and e.get("packed") and e["shape"] == tuple(w.shape) else None

    def build(self, dev):
        descs, blk = [], 0
        for (ptr, cs), e in self.entries.items():
            cout, cin, k, _ = e["shape"]
            cso = (cout + 15) // 16 * 16
            jobs = []
            for (role, layout) in sorted(e["need"]):
                co_, ci_, cs_ = (cout, cin, cs) if role == "fwd" else (cin, cout, cso)
                n = (_L().sbgm_conv_wino_packed_numel(co_, cs_) if layout == "w" else
                     _L().sbgm_conv_wino2d_packed_numel(co_, cs_) if layout == "d" else _L().sbgm_conv_packed_numel(co_, k, k, cs_))
                if e["img"][(role, layout)] is None:         # never re-allocated: a captured step keeps reading the image it saw
                    e["img"][(role, layout)] = torch.empty(n, device=dev)
                jobs.append((e["img"][(role, layout)], co_, ci_, cs_,
                             (1 if role == "bwd" else 0) | (2 if layout == "w" else 0) | (4 if layout == "d" else 0)))
            e["packed"] = True
            for dst, co_, ci_, cs_, tr in jobs:
                nsteps = dst.numel() // (co_ * 16)
                descs.append(N.PackDesc(ptr, dst.data_ptr(), co_, ci_, k, k, cs_, nsteps, tr, blk))
                blk += _L().sbgm_conv_pack_weights_batched_blocks(co_, k, k, cs_)
        raw = (N.PackDesc * len(descs))(*descs)
        host = torch.frombuffer(bytearray(bytes(raw)), dtype=torch.uint8)
        if self.desc is not None:
            self.keep.append(self.desc)                      # an earlier capture replays its pack launch from this table
        self.desc, self.n, self.blocks = host.to(dev), len(descs), blk

    def run(self, dev):
        """pack everything recorded so far (no-op until the first forward has recorded the weights)"""
        self.fresh = False
        # a recorded weight whose parameter died or moved (model deleted, .to(), load with assign) must never be read again
        stale = [k for k, e in self.entries.items() if e["ref"]() is None or e["ref"]().data_ptr() != k[0]]
        if stale and not torch.cuda.is_current_stream_capturing():
            for k in stale:
                del self.entries[k]
            self.dirty = True
        capturing = torch.cuda.is_current_stream_capturing()
        if not self.entries or capturing and self.desc is None:
            return
        if (self.desc is None or self.dirty) and not capturing:      # (a capture replays the table it was recorded with)
            self.build(dev)
            self.dirty = False
        N.check(_L().sbgm_conv_pack_weights_batched(self.desc.data_ptr(), self.n, self.blocks, _st()))
        self.fresh = True


_PLANS = {}            # id(net) -> _PackPlan


def _plan_for(net):
    plan = _PLANS.get(id(net))
    if plan is None or plan.owner() is not net:           # ids are recycled: a plan belongs to one live model object
        plan = _PLANS[id(net)] = _PackPlan()
        plan.owner = weakref.ref(net)
        for k in [k for k, v in _PLANS.items() if v.owner() is None]:
            del _PLANS[k]
    return plan


def _wino_ok(k, stride, pad, in_dil, cs, cout, W):
    """geometries the Winograd F(2,3) kernels take (3x3 / stride 1 / pad 1, channels in 16s, even width)"""
    return k == 3 and stride == 1 and pad == 1 and not in_dil and cs % 16 == 0 and cout % 32 == 0 and W % 2 == 0


def _w2d_ok(k, stride, pad, in_dil, cs, cout, H, W):
    """geometries the 2-D Winograd F(2x2,3x3) kernels take (conv_w2d.hip: 16-pixel-wide tiles, 2x2 output blocks)"""
    return k == 3 and stride == 1 and pad == 1 and not in_dil and cs % 16 == 0 and cout % 32 == 0 and W % 16 == 0 and H % 2 == 0


class _MissingImage(Exception):
    """the geometry's tuned tile reads a weight image ('g' implicit GEMM / 'w' Winograd F(2,3) / 'd' F(2x2,3x3)) the caller did not
    bring"""


def _tile_from_tune(t6):
    """sbgm_conv2d_tune's tile[6] -> (tile_co, tile_px, splits, waves_per_tile, winograd bits) of sbgm_conv_args"""
    if t6[4] == 2:                                           # F(2x2,3x3): bit 3; bit 4 = persistent form, bit 2 = two stage buffers
        return (t6[0], 0, 0, t6[3], 8 | (16 if t6[5] == 3 else (4 if t6[5] == 2 else 0)))
    return (t6[0], t6[1], t6[2], t6[3], t6[4] | (2 if t6[5] else 0) | (4 if t6[5] == 2 else 0))


def _tile_layout(tile):
    return "d" if tile[4] & 8 else ("w" if tile[4] & 1 else "g")


def _conv_launch(x, packed, out, cs, cout, k, stride, pad, bias=None, res=None, tbias=None, in_dil=0, out_hw=(0, 0), wino=None,
                 w2d=None, on_missing="default"):
    """One convolution through the per-op C ABI.  The first time a geometry is seen (outside graph capture) the library
    times its kernel / tile / split-K candidates on these very operands and the winner is reused from then on.
    packed / wino / w2d: the implicit-GEMM, the Winograd F(2,3) and the Winograd F(2x2,3x3) weight image; any may be None when the
    geometry's tile is known to read another.  Returns the layout the launch read: 'g', 'w' or 'd'."""
    B, H, W, _ = x.shape
    # the key says which Winograd candidates take part for this geometry: first-step calls then bring every image, so the
    # cached tile never depends on which caller tuned it
    wk = _USE_WINO[0] and _wino_ok(k, stride, pad, in_dil, cs, cout, W)
    dk = _USE_WINO[0] and _w2d_ok(k, stride, pad, in_dil, cs, cout, H, W)
    key = (B, H, W, cs, cout, k, stride, pad, in_dil, out_hw, bias is not None, res is not None, tbias is not None, wk, dk)
    ws = _splitk_ws(x.device)
    first = packed if packed is not None else (wino if wino is not None else w2d)
    a = N.ConvArgs(x.data_ptr(), first.data_ptr(), out.data_ptr(), None, N.ptr(bias), N.ptr(tbias),
                   N.ptr(res), B, H, W, cs, cout, k, k, stride, pad, N.NONE, 0, 0, 0, 0, 0, 0, in_dil, out_hw[0], out_hw[1],
                   ws.data_ptr(), _SPLITK_FLOATS, 0, None, None, 0, N.ptr(wino) if wk else None, N.ptr(w2d) if dk else None)
    have = {"g": packed is not None, "w": wino is not None, "d": w2d is not None}
    tile = _TILES.get(key)
    if tile is None and cout % 32 == 0 and not torch.cuda.is_current_stream_capturing() and packed is not None \
            and (wino is not None or not wk) and (w2d is not None or not dk):
        t6 = (C.c_int * 6)()
        N.check(_L().sbgm_conv2d_tune(C.byref(a), t6, _st()))
        tile = _TILES[key] = _tile_from_tune(t6)
    if tile is not None and not have[_tile_layout(tile)]:
        if on_missing == "raise":
            raise _MissingImage(_tile_layout(tile))
        tile = None                                        # the tuned choice reads an image this call does not have: default tile
    if tile is not None:
        a.tile_co, a.tile_px, a.splits, a.waves_per_tile, a.winograd = tile
    elif packed is None:
        raise _MissingImage("g")
    N.check(_L().sbgm_conv2d_fwd(C.byref(a), _st()))
    return _tile_layout(tile) if tile is not None else "g"


def _pack_single(w, cout, cin, k, cs, flags):
    """one weight through the batched pack entry (flags: bit 0 data-gradient operator, bit 1 Winograd F(2,3) image, bit 2 F(2x2,3x3)
    image); first step only"""
    dst = torch.empty(_L().sbgm_conv_wino_packed_numel(cout, cs) if flags & 2 else
                      _L().sbgm_conv_wino2d_packed_numel(cout, cs) if flags & 4 else _L().sbgm_conv_packed_numel(cout, k, k, cs), device=w.device)
    d = N.PackDesc(w.data_ptr(), dst.data_ptr(), cout, cin, k, k, cs, dst.numel() // (cout * 16), flags, 0)
    dev = torch.frombuffer(bytearray(bytes(d)), dtype=torch.uint8).to(w.device)
    N.check(_L().sbgm_conv_pack_weights_batched(dev.data_ptr(), 1, _L().sbgm_conv_pack_weights_batched_blocks(cout, k, k, cs), _st()))
    return dst


def _conv_with_images(x, w, out, imgs, dgrad, cs, cout, k, stride, pad, **epilogue):
    """One convolution with whatever images weight `w` has.  dgrad False: the forward operator (w is [cout, cin <= cs, k, k]);
    True: the data-gradient operator (w is [cs, cout, k, k], read transposed and flipped).  imgs: the plan's ('g', 'w', 'd') images
    for this role, or None.  When they do not hold what the geometry's tile reads (first step; another batch shape of the same weight
    wants another layout) the implicit-GEMM image and every Winograd image the geometry admits are packed on the spot.
    Returns (layout read, True if packed here): the caller tells its plan."""
    if imgs is not None and any(im is not None for im in imgs):
        try:
            return _conv_launch(x, imgs[0], out, cs, cout, k, stride, pad, wino=imgs[1], w2d=imgs[2], on_missing="raise", **epilogue), False
        except _MissingImage:
            pass
    packed = torch.empty(_L().sbgm_conv_packed_numel(cout, k, k, cs), device=x.device)
    if dgrad:
        N.check(_L().sbgm_conv_pack_weight_dgrad(w.data_ptr(), packed.data_ptr(), cs, cout, k, k, _st()))
    else:
        N.check(_L().sbgm_conv_pack_weight(w.data_ptr(), packed.data_ptr(), cout, w.shape[1], k, k, cs, _st()))
    pw = pd = None
    if _USE_WINO[0] and not torch.cuda.is_current_stream_capturing():
        cin, in_dil = w.shape[0 if dgrad else 1], epilogue.get("in_dil", 0)
        if _wino_ok(k, stride, pad, in_dil, cs, cout, x.shape[2]):
            pw = _pack_single(w, cout, cin, k, cs, 2 | dgrad)
        if _w2d_ok(k, stride, pad, in_dil, cs, cout, x.shape[1], x.shape[2]):
            pd = _pack_single(w, cout, cin, k, cs, 4 | dgrad)
    return _conv_launch(x, packed, out, cs, cout, k, stride, pad, wino=pw, w2d=pd, **epilogue), True


def _samplesum(dy, B, Cc):
    """gradient of a per-sample bias [B, Cc] broadcast over the pixels of dy"""
    dtb, zeroed = _STEP.zeros(B * Cc, dy.device, True)
    with _prezeroed(zeroed):
        N.check(_L().sbgm_samplesum(dy.data_ptr(), dtb.data_ptr(), B, dy.numel() // (B * Cc), Cc, _st()))
    return dtb.view(B, Cc)


class ConvFn(torch.autograd.Function):
    """y = conv2d(x, w, stride, pad) [+ bias] [+ tbias[b] broadcast over pixels] [+ res]   (NHWC x, OIHW w).
    Also serves nn.Linear as a 1x1 conv."""

    @staticmethod
    def forward(ctx, x, w, bias, res, tbias, stride, pad, xslot=None, rslot=None):
        B, H, W, cs = x.shape
        cout, cin, k, _ = w.shape
        plan = _STEP.plan
        e = plan.lookup(w, cs) if plan is not None else None
        fwd_imgs = ctx.packed_bwd = None
        if e is not None:                                    # packed by the step's batched launch, in the layout(s) its tiles read
            fwd_imgs, ctx.packed_bwd = (tuple(e["img"][(role, l)] for l in "gwd") for role in ("fwd", "bwd"))
        oh, ow = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        y = torch.empty(B, oh, ow, cout, device=x.device)
        used, packed_here = _conv_with_images(x, w, y, fwd_imgs, False, cs, cout, k, stride, pad, bias=bias, res=res, tbias=tbias)
        base = w._base if w._base is not None else w
        if packed_here and plan is not None and base.is_leaf and base.data_ptr() == w.data_ptr() and base.numel() == w.numel():
            # a parameter or a reshaped view of one (nn.Linear weights), not a derived tensor: batch-pack it from the next step on
            plan.note(w, cs, dgrad=x.requires_grad and cs == cin and cs % 32 == 0, layout=used)
        ctx.save_for_backward(x, w, bias)
        ctx.geom = (stride, pad, bias is not None, res is not None, tbias is not None)
        ctx.slots = (xslot, rslot)
        ctx.plan = plan
        ctx.arena = _STEP.arena
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, bias = ctx.saved_tensors
        arena = ctx.arena
        stride, pad, has_bias, has_res, has_tb = ctx.geom
        dy = dy.contiguous()
        B, H, W, cs = x.shape
        cout, cin, k, _ = w.shape
        dx = dw = db = None
        xslot, rslot = ctx.slots
        extra = xslot.take(x) if (xslot is not None and ctx.needs_input_grad[0]) else None      # partial sum from x's other consumers
        fused = False
        if ctx.needs_input_grad[0] and k == 8 and stride == 2 and pad == 3 and cs == cin and cin % 16 == 0 and cout % 16 == 0 \
                and H % 2 == 0 and W % 2 == 0:
            # stem conv2: phase-decomposed data gradient (5x5 / stride 1 over dy to 4*Cin phase-major channels + depth->space)
            # instead of an 8x8 convolution over the zero-inserted dy (75 % of whose MACs multiply zeros)
            wph = torch.empty(4 * cin, cout, 5, 5, device=x.device)
            N.check(_L().sbgm_conv8x8s2_dgrad_phase_weight(w.data_ptr(), wph.data_ptr(), cout, cin, _st()))
            pk = torch.empty(_L().sbgm_conv_packed_numel(4 * cin, 5, 5, cout), device=x.device)
            N.check(_L().sbgm_conv_pack_weight(wph.data_ptr(), pk.data_ptr(), 4 * cin, cout, 5, 5, cout, _st()))
            ph = torch.empty(B, H // 2, W // 2, 4 * cin, device=x.device)
            _conv_launch(dy, pk, ph, cout, 4 * cin, 5, 1, 2)
            dx = torch.empty_like(x)
            N.check(_L().sbgm_depth_to_space2(ph.data_ptr(), dx.data_ptr(), B, H // 2, W // 2, cin, _st()))
        elif ctx.needs_input_grad[0]:
            if cs != cin or cs % 32:
                raise NotImplementedError("data gradient w.r.t. a channel-padded input is not needed on this path")
            dx = torch.empty_like(x)
            used, packed_here = _conv_with_images(dy, w, dx, ctx.packed_bwd, True, cout, cin, k, 1, k - 1 - pad, res=extra,
                                                  in_dil=2 if stride == 2 else 0, out_hw=(H, W))
            if packed_here and ctx.plan is not None:
                ctx.plan.note_bwd(w, cs, used)
            fused = True                                         # the convolution's epilogue added the pending partial sum
        want_db = has_bias and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1]:
            if _WGRAD_LOG[0] is not None:
                _WGRAD_LOG[0].append((B, H, W, cs, cin, cout, k, stride, pad))
            if k == 1 and cs == cin and cs % 64 == 0 and cout % 64 == 0:
                # 1x1 / linear: the partial-sum slab has the OIHW layout, so the (zeroed) gradient itself is the workspace
                dw, pooled = _pgrad(arena, w, True)
                ws, defer = dw, False
            else:
                dw, in_arena = _pgrad(arena, w, False)
                ws, pooled = _STEP.zeros(k * k * cout * cs, x.device)
                # the layout pass may run at the end of the backward sweep only when nothing consumes dw before that: an arena
                # slice becomes p.grad as it is; a fresh tensor may be added to a live .grad by AccumulateGrad right away
                defer = pooled and in_arena
            # the GEMM itself may join the sweep's batched launch when its results land in the arena (nothing reads them before the flush)
            gemm_defer = _BATCH_WGRAD[0] and pooled and _in_arena(arena, dw) and torch.is_grad_enabled() is False
            if want_db and pooled:                               # bias gradient as a by-product of the weight-gradient sweep
                db, _ = _pgrad(arena, bias, True)                # a returned gradient: never a slice of the re-zeroed scratch pool
                with _prezeroed(True), _deferred_unpack(ws is not dw and defer, gemm_defer and _in_arena(arena, db), (dy, x)):
                    N.check(_L().sbgm_conv2d_wgrad_bias(dy.data_ptr(), x.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), B, H, W,
                                                        cs, cin, cout, k, k, stride, pad, _st()))
                want_db = False
            else:
                with _prezeroed(pooled), _deferred_unpack(ws is not dw and defer, gemm_defer, (dy, x)):
                    N.check(_L().sbgm_conv2d_wgrad(dy.data_ptr(), x.data_ptr(), dw.data_ptr(), ws.data_ptr(), B, H, W, cs, cin, cout, k, k,
                                                   stride, pad, _st()))
        if want_db:
            db, _ = _pgrad(arena, bias, False)
            N.check(_L().sbgm_colsum(dy.data_ptr(), None, db.data_ptr(), dy.numel() // cout, cout, _st()))
        dtb = _samplesum(dy, B, cout) if has_tb and ctx.needs_input_grad[4] else None
        if xslot is not None and ctx.needs_input_grad[0]:
            if not fused and extra is not None:
                dx = dx + extra                                  # stem convolution (phase-decomposed data gradient): no residual epilogue
            dx = xslot.give(dx)
        dres = dy if has_res and ctx.needs_input_grad[3] else None
        if dres is not None:
            dres = _fold(rslot, dres)
        return dx, dw, db, dres, dtb, None, None, None, None


def linear(x2d, w, b, res=None, rslot=None):
    """nn.Linear over tokens [M, C] (+ residual) on the conv kernel"""
    M, Cc = x2d.shape
    y = ConvFn.apply(x2d.view(1, 1, M, Cc), w.view(w.shape[0], w.shape[1], 1, 1), b,
                     None if res is None else res.view(1, 1, M, -1), None, 1, 0, None, rslot)
    return y.view(M, -1)


class BNTrainFn(torch.autograd.Function):
    """y = relu?(BatchNorm_train(x) [+ res]) [+ tbias_after]; updates running statistics in place.
    With set_sync_batchnorm(True) and a process group of more than one rank the statistics (forward: sum x, sum x^2; backward:
    sum g, sum g*xhat) are summed over the ranks — one small all-reduce each way — so the step equals the reference's
    single-device step on the GLOBAL batch (reference score_unet.py:323 sees the whole batch on one device)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, rm, rv, res, tb_after, relu, eps, momentum, rslot=None):
        B, H, W, Cc = x.shape
        ctx.rslot = rslot
        y = torch.empty_like(x)
        mr = torch.empty(Cc, 2, device=x.device)         # (mean, rstd) per channel, kept for the backward
        sums, pooled = _STEP.zeros(4 * Cc, x.device)          # 2C fp64 sums: scratch of this launch only
        dist = _sync_world()
        n_total = None
        with _prezeroed(pooled):
            if dist is None:
                N.check(_L().sbgm_batchnorm_train_fwd(x.data_ptr(), y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(),
                                                      rv.data_ptr(), N.ptr(res), N.ptr(tb_after), int(relu), B, H * W, Cc, eps, momentum,
                                                      sums.data_ptr(), mr.data_ptr(), _st()))
            else:
                n_total = float(_STEP.sync_count * H * W)
                N.check(_L().sbgm_batchnorm_train_stats(x.data_ptr(), B, H * W, Cc, sums.data_ptr(), _st()))
                dist.all_reduce(sums.view(torch.float64))
                N.check(_L().sbgm_batchnorm_train_apply(x.data_ptr(), y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(),
                                                        rv.data_ptr(), N.ptr(res), N.ptr(tb_after), int(relu), B, H * W, Cc, eps, momentum,
                                                        sums.data_ptr(), n_total, mr.data_ptr(), _st()))
        if relu and _RELU_TRACE[0] is not None:
            _RELU_TRACE[0].append(((y - tb_after.view(B, 1, 1, Cc)) if tb_after is not None else y) > 0)
        ctx.save_for_backward(x, y, gamma, beta, tb_after, mr)
        ctx.cfg = (relu, res is not None, tb_after is not None, n_total)
        ctx.arena = _STEP.arena
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, gamma, beta, tb_after, mr = ctx.saved_tensors
        relu, has_res, has_tb, n_total = ctx.cfg
        dy = dy.contiguous()
        B, H, W, Cc = x.shape
        dx, dres = torch.empty_like(x), (torch.empty_like(x) if has_res else None)
        dg, _ = _pgrad(ctx.arena, gamma, False)
        db, _ = _pgrad(ctx.arena, beta, False)
        s12, pooled = _STEP.zeros(B * Cc * 2, x.device)
        with _prezeroed(pooled):
            if n_total is None:
                N.check(_L().sbgm_batchnorm_bwd(x.data_ptr(), dy.data_ptr(), y.data_ptr(), gamma.data_ptr(), N.ptr(tb_after), mr.data_ptr(),
                                                int(relu), dx.data_ptr(), N.ptr(dres), dg.data_ptr(), db.data_ptr(), s12.data_ptr(), B, H * W,
                                                Cc, _st()))
            else:
                dist = _sync_world()
                if dist is None:
                    raise RuntimeError("SyncBatchNorm backward without the process group its forward ran in")
                N.check(_L().sbgm_batchnorm_bwd_reduce(x.data_ptr(), dy.data_ptr(), y.data_ptr(), N.ptr(tb_after), mr.data_ptr(), int(relu),
                                                       s12.data_ptr(), B, H * W, Cc, _st()))
                tot = s12.view(B, Cc * 2).sum(0)
                dist.all_reduce(tot)
                N.check(_L().sbgm_batchnorm_bwd_apply(x.data_ptr(), dy.data_ptr(), y.data_ptr(), gamma.data_ptr(), N.ptr(tb_after),
                                                      mr.data_ptr(), int(relu), dx.data_ptr(), N.ptr(dres), dg.data_ptr(), db.data_ptr(),
                                                      s12.data_ptr(), tot.data_ptr(), n_total, B, H * W, Cc, _st()))
        dtb = _samplesum(dy, B, Cc) if has_tb else None
        return dx, dg, db, None, None, (_fold(ctx.rslot, dres) if dres is not None else None), dtb, None, None, None, None


class GroupNormFn(torch.autograd.Function):
    """y = act(GroupNorm(x) [+ skip] [+ tbias])   (gamma/beta None = InstanceNorm2d without affine)"""

    @staticmethod
    def forward(ctx, x, gamma, beta, skip, tbias, act, G, eps, sslot=None):
        B, H, W, Cc = x.shape
        ctx.sslot = sslot
        y = torch.empty_like(x)
        ws = torch.empty(1024 * B * G, dtype=torch.uint8, device=x.device)
        mr = torch.empty(B * G * 2, device=x.device)
        N.check(_L().sbgm_groupnorm_fwd(x.data_ptr(), y.data_ptr(), N.ptr(gamma), N.ptr(beta), N.ptr(skip), N.ptr(tbias), act, B, H * W,
                                        Cc, G, eps, ws.data_ptr(), mr.data_ptr(), _st()))
        ctx.save_for_backward(x, gamma, beta, skip, tbias, mr)
        ctx.cfg = (act, G)
        ctx.arena = _STEP.arena
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, beta, skip, tbias, mr = ctx.saved_tensors
        act, G = ctx.cfg
        dy = dy.contiguous()
        B, H, W, Cc = x.shape
        dev = x.device
        dx = torch.empty_like(x)
        dskip = torch.empty_like(x) if skip is not None else None
        dg = _pgrad(ctx.arena, gamma, False)[0] if gamma is not None else None
        db = _pgrad(ctx.arena, beta, False)[0] if gamma is not None else None
        dtb = torch.empty(B, Cc, device=dev) if tbias is not None else None
        s12, pooled = _STEP.zeros(B * Cc * 2, dev)
        with _prezeroed(pooled):
            N.check(_L().sbgm_groupnorm_bwd(x.data_ptr(), dy.data_ptr(), N.ptr(gamma), N.ptr(beta), N.ptr(skip), N.ptr(tbias), mr.data_ptr(),
                                            act, dx.data_ptr(), N.ptr(dskip), N.ptr(dg), N.ptr(db), N.ptr(dtb), s12.data_ptr(), B, H * W, Cc,
                                            G, _st()))
        return dx, dg, db, (_fold(ctx.sslot, dskip) if dskip is not None else None), dtb, None, None, None, None


class LayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, eps, xslot=None):
        M, Cc = x.shape
        y = torch.empty_like(x)
        N.check(_L().sbgm_layernorm_fwd(x.data_ptr(), y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), M, Cc, eps, _st()))
        ctx.save_for_backward(x, gamma, beta)
        ctx.xslot = xslot
        ctx.eps = eps
        ctx.arena = _STEP.arena
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, beta = ctx.saved_tensors
        dy = dy.contiguous()
        M, Cc = x.shape
        dx = torch.empty_like(x)
        dg, z1 = _pgrad(ctx.arena, gamma, True)
        db, z2 = _pgrad(ctx.arena, beta, True)
        zeroed = z1 and z2
        if not zeroed:                                   # adjacent: the launcher zeroes both with one memset
            dgb = torch.empty(2 * Cc, device=x.device)
            dg, db = dgb[:Cc], dgb[Cc:]
        extra = ctx.xslot.take(x) if ctx.xslot is not None else None
        with _prezeroed(zeroed):
            N.check(_L().sbgm_layernorm_bwd(x.data_ptr(), dy.data_ptr(), gamma.data_ptr(), dx.data_ptr(), dg.data_ptr(), db.data_ptr(), M,
                                            Cc, ctx.eps, N.ptr(None if extra is None else extra.contiguous()), _st()))
        if ctx.xslot is not None:
            dx = ctx.xslot.give(dx)
        return dx, dg, db, None, None


class MHACoreFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, B, S, Cc, heads):
        out = torch.empty(B * S, Cc, device=qkv.device)
        N.check(_L().sbgm_mha_core_fwd(qkv.data_ptr(), out.data_ptr(), B, S, Cc, heads, _st()))
        ctx.save_for_backward(qkv)
        ctx.dims = (B, S, Cc, heads)
        return out

    @staticmethod
    def backward(ctx, dout):
        (qkv,) = ctx.saved_tensors
        B, S, Cc, heads = ctx.dims
        dout = dout.contiguous()
        dqkv, zeroed = _STEP.zeros(qkv.numel(), qkv.device, True)       # dK / dV are accumulated with atomics: a slice of the step's zeroed pool
        dqkv = dqkv.view(qkv.shape)                              # saves the launcher's own memset (4 per step)
        with _prezeroed(zeroed):
            N.check(_L().sbgm_mha_core_bwd(qkv.data_ptr(), dout.data_ptr(), dqkv.data_ptr(), B, S, Cc, heads, _st()))
        return dqkv, None, None, None, None


class MHACoreDropoutFn(torch.autograd.Function):
    """the attention core with train-mode dropout on the softmax probabilities (nn.MultiheadAttention(dropout=p)): the mask is a Philox
    stream keyed by `seed`, regenerated in the backward pass (csrc/attention_dropout.hip)"""
    @staticmethod
    def forward(ctx, qkv, B, S, Cc, heads, p, seed):
        out = torch.empty(B * S, Cc, device=qkv.device)
        N.check(_L().sbgm_mha_core_dropout_fwd(qkv.data_ptr(), out.data_ptr(), B, S, Cc, heads, float(p), int(seed), 0, _st()))
        ctx.save_for_backward(qkv)
        ctx.dims = (B, S, Cc, heads, float(p), int(seed))
        return out

    @staticmethod
    def backward(ctx, dout):
        (qkv,) = ctx.saved_tensors
        B, S, Cc, heads, p, seed = ctx.dims
        dout = dout.contiguous()
        dqkv, zeroed = _STEP.zeros(qkv.numel(), qkv.device, True)
        dqkv = dqkv.view(qkv.shape)
        with _prezeroed(zeroed):
            N.check(_L().sbgm_mha_core_dropout_bwd(qkv.data_ptr(), dout.data_ptr(), dqkv.data_ptr(), B, S, Cc, heads, p, seed, 0, _st()))
        return dqkv, None, None, None, None, None, None


class UpsampleFn(torch.autograd.Function):
    """nn.Upsample(scale_factor=scale, bilinear, align_corners=False) over NHWC; scale 2 (every block of the Decoder) has its own kernels"""
    @staticmethod
    def forward(ctx, x, scale=2):
        B, H, W, Cc = x.shape
        y = torch.empty(B, scale * H, scale * W, Cc, device=x.device)
        if scale == 2:
            N.check(_L().sbgm_upsample2x_fwd(x.data_ptr(), y.data_ptr(), B, H, W, Cc, _st()))
        else:
            N.check(_L().sbgm_upsample_bilinear_fwd(x.data_ptr(), y.data_ptr(), B, H, W, Cc, scale, _st()))
        ctx.dims = (B, H, W, Cc, scale)
        return y

    @staticmethod
    def backward(ctx, dy):
        B, H, W, Cc, scale = ctx.dims
        dy = dy.contiguous()
        dx = torch.empty(B, H, W, Cc, device=dy.device)
        if scale == 2:
            N.check(_L().sbgm_upsample2x_bwd(dy.data_ptr(), dx.data_ptr(), B, H, W, Cc, _st()))
        else:
            N.check(_L().sbgm_upsample_bilinear_bwd(dy.data_ptr(), dx.data_ptr(), B, H, W, Cc, scale, _st()))
        return dx, None


class DepthToSpaceFn(torch.autograd.Function):
    """[B,H,W,s*s*C] (phase-major channels) -> [B,sH,sW,C]; backward is the inverse permutation (s = 2: the Decoder's own kernels)"""
    @staticmethod
    def forward(ctx, x, s=2):
        B, H, W, Cd = x.shape
        Cc = Cd // (s * s)
        y = torch.empty(B, s * H, s * W, Cc, device=x.device)
        if s == 2:
            N.check(_L().sbgm_depth_to_space2(x.data_ptr(), y.data_ptr(), B, H, W, Cc, _st()))
        else:
            N.check(_L().sbgm_depth_to_space(x.data_ptr(), y.data_ptr(), B, H, W, Cc, s, _st()))
        ctx.dims = (B, H, W, Cd, s)
        return y

    @staticmethod
    def backward(ctx, dy):
        B, H, W, Cd, s = ctx.dims
        dy = dy.contiguous()
        dx = torch.empty(B, H, W, Cd, device=dy.device)
        if s == 2:
            N.check(_L().sbgm_space_to_depth2(dy.data_ptr(), dx.data_ptr(), B, H, W, Cd // 4, _st()))
        else:
            N.check(_L().sbgm_space_to_depth(dy.data_ptr(), dx.data_ptr(), B, H, W, Cd // (s * s), s, _st()))
        return dx, None


def conv_transpose2x(x, mod):
    """nn.ConvTranspose2d(C, C, s, stride=s) (reference score_unet.py:472-475, :589; s = 2 in the Decoder) = 1x1 conv to s*s*C phase-major
    channels + depth->space.  The weight/bias rearrangement is plain autograd-tracked tensor indexing on the parameters."""
    ci, co = mod.weight.shape[0], mod.weight.shape[1]
    s = int(mod.weight.shape[2])
    w1 = mod.weight.permute(2, 3, 1, 0).reshape(s * s * co, ci, 1, 1).contiguous()       # [(dy,dx,co), ci]
    bs = None if mod.bias is None else mod.bias.repeat(s * s)
    return DepthToSpaceFn.apply(ConvFn.apply(x, w1, bs, None, None, 1, 0), s)


class ActFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, act):
        y = torch.empty_like(x)
        N.check(_L().sbgm_act_fwd(x.data_ptr(), y.data_ptr(), x.numel(), act, _st()))
        ctx.save_for_backward(x)
        ctx.act = act
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        N.check(_L().sbgm_act_bwd(x.data_ptr(), dy.data_ptr(), dx.data_ptr(), x.numel(), ctx.act, _st()))
        return dx, None


class TimeProjFn(torch.autograd.Function):
    """SinusoidalEmbedding(t) [+ label_emb(y)] -> SiLU -> Linear : [B] -> [B, ch]"""

    @staticmethod
    def forward(ctx, t, y, table, freqs, weight, bias):
        B, (ch, D) = t.numel(), weight.shape
        out, semb, raw = torch.empty(B, ch, device=t.device), torch.empty(B, D, device=t.device), torch.empty(B, D, device=t.device)
        N.check(_L().sbgm_time_proj_fwd(t.data_ptr(), N.ptr(y), N.ptr(table) if y is not None else None, freqs.data_ptr(),
                                        weight.data_ptr(), bias.data_ptr(), out.data_ptr(), semb.data_ptr(), raw.data_ptr(), B, D, ch,
                                        _st()))
        ctx.save_for_backward(weight, bias, semb, raw, y if y is not None else torch.empty(0), table if table is not None else torch.empty(0))
        ctx.has_y = y is not None
        ctx.arena = _STEP.arena
        return out

    @staticmethod
    def backward(ctx, dout):
        weight, bias, semb, raw, y, table = ctx.saved_tensors
        dout = dout.contiguous()
        B, (ch, D) = dout.shape[0], weight.shape
        dW, db = _pgrad(ctx.arena, weight, False)[0], _pgrad(ctx.arena, bias, False)[0]
        demb = torch.zeros(B, D, device=dout.device) if ctx.has_y else None
        N.check(_L().sbgm_time_proj_bwd(dout.data_ptr(), weight.data_ptr(), semb.data_ptr(), raw.data_ptr(), dW.data_ptr(), db.data_ptr(),
                                        N.ptr(demb), B, D, ch, _st()))
        dtable = None
        if ctx.has_y:
            dtable, was_zero = _pgrad(ctx.arena, table, True)
            if not was_zero:
                dtable.zero_()
            N.check(_L().sbgm_label_emb_bwd(demb.data_ptr(), y.data_ptr(), dtable.data_ptr(), B, D, _st()))
        return None, None, dtable, None, dW, db


class TimeProjMultiFn(torch.autograd.Function):
    """n_proj projections of n_emb time embeddings in one launch pair (instead of one pair per projection):
    apply(t, y, table, emb_index (tuple), n_emb, *freqs[n_emb], *weights[n_proj], *biases[n_proj]) -> n_proj tensors [B, ch_i]"""

    @staticmethod
    def forward(ctx, t, y, table, emb_index, n_emb, *rest):
        n_proj = len(emb_index)
        freqs, weights, biases = rest[:n_emb], rest[n_emb:n_emb + n_proj], rest[n_emb + n_proj:]
        B, D = t.numel(), weights[0].shape[1]
        dev = t.device
        outs = [torch.empty(B, w.shape[0], device=dev) for w in weights]
        semb, raw = torch.empty(n_emb, B, D, device=dev), torch.empty(n_emb, B, D, device=dev)
        arr = lambda ts: (C.c_void_p * len(ts))(*[x.data_ptr() for x in ts])                 # noqa: E731
        N.check(_L().sbgm_time_proj_multi_fwd(t.data_ptr(), N.ptr(y), N.ptr(table) if y is not None else None, arr(freqs), n_emb,
                                              arr(weights), arr(biases), arr(outs), (C.c_int * n_proj)(*[w.shape[0] for w in weights]),
                                              (C.c_int * n_proj)(*emb_index), n_proj, semb.data_ptr(), raw.data_ptr(), B, D, _st()))
        ctx.save_for_backward(semb, raw, y if y is not None else torch.empty(0), table if table is not None else torch.empty(0),
                              *weights, *biases)
        ctx.meta = (tuple(emb_index), n_emb, n_proj, y is not None)
        ctx.arena = _STEP.arena
        return tuple(outs)

    @staticmethod
    def backward(ctx, *douts):
        emb_index, n_emb, n_proj, has_y = ctx.meta
        semb, raw, y, table = ctx.saved_tensors[:4]
        weights, biases = ctx.saved_tensors[4:4 + n_proj], ctx.saved_tensors[4 + n_proj:]
        B, D = semb.shape[1], semb.shape[2]
        demb = torch.zeros(B, D, device=semb.device) if has_y else None          # only embedding 0 carries the label embedding
        dWs, dbs = [None] * n_proj, [None] * n_proj
        live = [i for i, d in enumerate(douts) if d is not None]
        dcs = {i: douts[i].contiguous() for i in live}
        for i in live:
            dWs[i], dbs[i] = _pgrad(ctx.arena, weights[i], False)[0], _pgrad(ctx.arena, biases[i], False)[0]
        if live:                                             # every weight / bias gradient of the group in one launch
            arr = lambda ts: (C.c_void_p * len(ts))(*[x.data_ptr() for x in ts])             # noqa: E731
            N.check(_L().sbgm_time_proj_multi_bwd(arr([dcs[i] for i in live]), arr([semb[emb_index[i]] for i in live]),
                                                  arr([dWs[i] for i in live]), arr([dbs[i] for i in live]),
                                                  (C.c_int * len(live))(*[weights[i].shape[0] for i in live]), len(live), B, D, _st()))
        if has_y:                                            # label-embedding gradient: embedding 0's projections only
            for i in live:
                if emb_index[i] == 0:
                    tmpW, tmpb = torch.empty_like(weights[i]), torch.empty_like(biases[i])
                    N.check(_L().sbgm_time_proj_bwd(dcs[i].data_ptr(), weights[i].data_ptr(), semb[0].data_ptr(), raw[0].data_ptr(),
                                                    tmpW.data_ptr(), tmpb.data_ptr(), demb.data_ptr(), B, D, weights[i].shape[0], _st()))
        dtable = None
        if has_y:
            dtable, was_zero = _pgrad(ctx.arena, table, True)
            if not was_zero:
                dtable.zero_()
            N.check(_L().sbgm_label_emb_bwd(demb.data_ptr(), y.data_ptr(), dtable.data_ptr(), B, D, _st()))
        return (None, None, dtable, None, None) + (None,) * n_emb + tuple(dWs) + tuple(dbs)


class Cout1Fn(torch.autograd.Function):
    """final_layer.conv (3x3, C -> 1) followed by the division by sigma(t) (t None: no division): NHWC a -> NCHW [B,1,H,W]"""

    @staticmethod
    def forward(ctx, a, w, bias, t, sigma):
        B, H, W, Cc = a.shape
        wp = torch.empty(9 * Cc, device=a.device)
        N.check(_L().sbgm_cout1_pack_weight(w.data_ptr(), wp.data_ptr(), Cc, _st()))
        out = torch.empty(B, 1, H, W, device=a.device)
        N.check(_L().sbgm_conv3x3_cout1_fwd(a.data_ptr(), wp.data_ptr(), bias.data_ptr(), N.ptr(t), sigma, out.data_ptr(), B, H, W, Cc,
                                            _st()))
        ctx.save_for_backward(a, wp, t, w, bias)
        ctx.sigma = sigma
        ctx.arena = _STEP.arena
        return out

    @staticmethod
    def backward(ctx, dout):
        a, wp, t, w, bias = ctx.saved_tensors
        dout = dout.contiguous()
        B, H, W, Cc = a.shape
        da, dwp, db = torch.empty_like(a), torch.empty(9 * Cc, device=a.device), _pgrad(ctx.arena, bias, False)[0]
        N.check(_L().sbgm_conv3x3_cout1_bwd(dout.data_ptr(), a.data_ptr(), wp.data_ptr(), N.ptr(t), ctx.sigma, da.data_ptr(),
                                            dwp.data_ptr(), db.data_ptr(), B, H, W, Cc, _st()))
        dw, _ = _pgrad(ctx.arena, w, False)
        dw.view(Cc, 9).copy_(dwp.view(9, Cc).t())                                        # [tap][c] -> OIHW
        return da, dw, db, None, None


# ----------------------------------------------------------------------------------------------------------------------
# the network (train mode), same order as Encoder.forward / DecoderBlock.forward / Decoder.forward of the reference
# ----------------------------------------------------------------------------------------------------------------------
def _pack_inputs(x, lsm, topo, cond, cs):
    srcs = [s for s in (x, lsm, topo, cond) if s is not None]
    B, _, H, W = x.shape
    out = torch.empty(B, H, W, cs, device=x.device)
    ptrs = (C.c_void_p * len(srcs))(*[s.data_ptr() for s in srcs])
    chs = (C.c_int * len(srcs))(*[s.shape[1] for s in srcs])
    N.check(_L().sbgm_pack_input(ptrs, chs, len(srcs), out.data_ptr(), B, H, W, cs, _st()))
    return out


def _bn(x, bn, res=None, tb_after=None, relu=True, rslot=None):
    if not bn.training:
        return _bn_eval(x, bn, res, tb_after, relu, rslot)
    y = BNTrainFn.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, res, tb_after, relu, bn.eps, bn.momentum, rslot)
    _STEP.nbt.append(bn.num_batches_tracked)
    return y


class BNEvalFn(torch.autograd.Function):
    """y = relu?(BatchNorm_eval(x) [+ res]) [+ tbias_after] with the RUNNING statistics (module.eval()), differentiable: the
    reference's ScoreNet.forward builds an autograd graph in any mode (score_unet.py:829-879).  Forward = the apply half of the
    train-mode kernel fed sums that reproduce (running_mean, running_var) exactly; the running statistics stay untouched.
    Backward = the SyncBatchNorm backward halves with zero batch-mean terms: dx = gamma * rstd * g (no dependence of the statistics
    on x), dgamma = sum g * xhat, dbeta = sum g."""

    @staticmethod
    def forward(ctx, x, gamma, beta, rm, rv, res, tb_after, relu, eps, rslot=None):
        B, H, W, Cc = x.shape
        ctx.rslot = rslot
        n = float(B * H * W)
        rmd, rvd = rm.double(), rv.double()
        ws = torch.empty(3 * Cc, dtype=torch.float64, device=x.device)              # (sum x, sum x^2) pairs + room for (mean, rstd)
        ws[:2 * Cc] = torch.stack([rmd * n, (rvd + rmd * rmd) * n], 1).reshape(-1)
        y = torch.empty_like(x)
        mr = torch.empty(Cc, 2, device=x.device)
        N.check(_L().sbgm_batchnorm_train_apply(x.data_ptr(), y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), None, None, N.ptr(res),
                                                N.ptr(tb_after), int(relu), B, H * W, Cc, eps, 0.0, ws.data_ptr(), n, mr.data_ptr(), _st()))
        if relu and _RELU_TRACE[0] is not None:
            _RELU_TRACE[0].append(((y - tb_after.view(B, 1, 1, Cc)) if tb_after is not None else y) > 0)
        ctx.save_for_backward(x, y, gamma, beta, tb_after, mr)
        ctx.cfg = (relu, res is not None, tb_after is not None)
        ctx.arena = _STEP.arena
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, gamma, beta, tb_after, mr = ctx.saved_tensors
        relu, has_res, has_tb = ctx.cfg
        dy = dy.contiguous()
        B, H, W, Cc = x.shape
        dx, dres = torch.empty_like(x), (torch.empty_like(x) if has_res else None)
        dg, _ = _pgrad(ctx.arena, gamma, False)
        db, _ = _pgrad(ctx.arena, beta, False)
        s12, pooled = _STEP.zeros(B * Cc * 2, x.device)
        with _prezeroed(pooled):
            N.check(_L().sbgm_batchnorm_bwd_reduce(x.data_ptr(), dy.data_ptr(), y.data_ptr(), N.ptr(tb_after), mr.data_ptr(), int(relu),
                                                   s12.data_ptr(), B, H * W, Cc, _st()))
        zero = torch.zeros(2 * Cc, device=x.device)                                   # batch-mean terms: none in eval mode
        N.check(_L().sbgm_batchnorm_bwd_apply(x.data_ptr(), dy.data_ptr(), y.data_ptr(), gamma.data_ptr(), N.ptr(tb_after), mr.data_ptr(),
                                              int(relu), dx.data_ptr(), N.ptr(dres), dg.data_ptr(), db.data_ptr(), s12.data_ptr(),
                                              zero.data_ptr(), float(B * H * W), B, H * W, Cc, _st()))
        dtb = _samplesum(dy, B, Cc) if has_tb else None
        return dx, dg, db, None, None, (_fold(ctx.rslot, dres) if dres is not None else None), dtb, None, None, None


def _bn_eval(x, bn, res, tb_after, relu, rslot=None):
    """BatchNorm2d with running statistics (module.eval())"""
    return BNEvalFn.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, res, tb_after, relu, bn.eps, rslot)


def _attention(mod, x):                               # x: [B, H, W, C] -> same (reference score_unet.py:136-148)
    B, H, W, Cc = x.shape
    drop = float(getattr(mod, "dropout", 0.0)) if mod.training else 0.0
    if drop > 0 and x.is_cuda and torch.cuda.is_current_stream_capturing():
        # the mask's seed is a by-value kernel argument: a captured step would replay ONE mask for ever
        raise RuntimeError("train-mode attention dropout draws a fresh seed per call and cannot be captured into a hipGraph: "
                           "set training.use_hip_graph: false (auto does this by itself)")
    tok = x.reshape(B * H * W, Cc)
    grad = torch.is_grad_enabled() and tok.requires_grad
    s1 = _slot(2) if grad else None                          # tok feeds ln1 and the residual of out_proj
    n1 = LayerNormFn.apply(tok, mod.ln1.weight, mod.ln1.bias, mod.ln1.eps, s1)
    qkv = linear(n1, mod.mha.in_proj_weight, mod.mha.in_proj_bias)
    if drop > 0:
        from .score_sampling import _fresh_seed          # torch's CPU generator: torch.manual_seed makes the masks repeatable
        att = MHACoreDropoutFn.apply(qkv, B, H * W, Cc, mod.n_heads, drop, _fresh_seed())
    else:
        att = MHACoreFn.apply(qkv, B, H * W, Cc, mod.n_heads)
    h = linear(att, mod.mha.out_proj.weight, mod.mha.out_proj.bias, res=tok, rslot=s1)
    s2 = _slot(2) if grad else None                          # h feeds ln2 and the residual of ff[2]
    n2 = LayerNormFn.apply(h, mod.ln2.weight, mod.ln2.bias, mod.ln2.eps, s2)
    f = ActFn.apply(linear(n2, mod.ff[0].weight, mod.ff[0].bias), N.GELU)
    return linear(f, mod.ff[2].weight, mod.ff[2].bias, res=h, rslot=s2).view(B, H, W, Cc)


def forward_train(net, x, t, y, cond, lsm, topo):
    _STEP.begin(x.device, net)
    try:
        dist = _sync_world()
        if dist is not None:                                # SyncBatchNorm: total batch over the ranks (ragged last batches allowed)
            cnt = torch.tensor([float(x.shape[0])], device=x.device)
            dist.all_reduce(cnt)
            _STEP.sync_count = int(round(float(cnt.item())))
        _STEP.plan.run(x.device)
        skip_slots = []
        fmaps = encoder_forward(net.encoder, x, t, y, cond, lsm, topo, skip_slots)
        a = decoder_forward(net.decoder, fmaps, t, skip_slots)
        fin = net.decoder.final_layer
        _STEP.bump_nbt()
        return Cout1Fn.apply(a, fin.conv.weight, fin.conv.bias, t, float(net.sigma))
    finally:
        _STEP.plan = _STEP.arena = None                     # active while the forward records its ops, not for single ops run after it


def _tproj(t, y, tlabel, freq_mod, seq):
    return TimeProjFn.apply(t, y, tlabel, freq_mod.W, seq[1].weight, seq[1].bias)


def encoder_forward(enc, x, t, y, cond, lsm, topo, skip_slots=None):
    """Encoder.forward (reference score_unet.py:247-364) on NCHW inputs -> the 5 feature maps, NHWC.
    skip_slots: a list that receives one gradient slot (or None) per feature map 0..3 when the CALLER will consume each map exactly
    once more (the decoder's skip connections in forward_train); None: the maps' gradients are summed by autograd."""
    tlabel = enc.label_emb.weight if (y is not None and enc.num_classes is not None) else None
    if y is not None and tlabel is None:
        raise ValueError("y given but the model has no label embedding")
    x0 = _pack_inputs(x, lsm, topo, cond, _pad_c(enc.input_channels))
    seqs = [enc.time_projection_layers[i][1] for i in range(5)]               # one embedding, five SiLU -> Linear heads (:301-308)
    tb = TimeProjMultiFn.apply(t, y if tlabel is not None else None, tlabel, (0,) * 5, 1, enc.sinusoidal_embedding.W,
                               *[q.weight for q in seqs], *[q.bias for q in seqs])
    grad = torch.is_grad_enabled()
    shared = grad and skip_slots is not None
    f1 = ConvFn.apply(x0, enc.conv1.weight, None, None, tb[0], 2, 3)                    # conv1 + time bias (:312-316)
    s_f1 = _slot(2) if shared else None                                                 # f1 feeds conv2 and the last decoder skip
    h = _bn(ConvFn.apply(f1, enc.conv2.weight, None, None, None, 2, 3, s_f1), enc.bn1)
    fmaps, slots = [f1], [s_f1]
    hs = None                                # slot of `h` when it is a feature map the decoder consumes as well
    for li in range(1, 5):
        layer = getattr(enc, f"layer{li}")
        for bi, blk in enumerate(layer):
            # h feeds conv1 and either the shortcut convolution or the residual add (and, as a feature map, a decoder skip)
            sx = hs if hs is not None else (_slot(2) if grad else None)
            hs = None
            y1 = _bn(ConvFn.apply(h, blk.conv1.weight, None, None, None, blk.stride, 1, sx), blk.bn1)
            idn, rs = h, sx
            if blk.downsample is not None:
                idn = _bn(ConvFn.apply(h, blk.downsample[0].weight, None, None, None, blk.stride, 0, sx), blk.downsample[1], relu=False)
                rs = None
            last = bi == len(layer) - 1
            h = _bn(ConvFn.apply(y1, blk.conv2.weight, None, None, None, 1, 1), blk.bn2, res=idn, tb_after=tb[li] if last else None,
                    rslot=rs)
        if not isinstance(enc.attention_layers[li], torch.nn.Identity):
            h = _attention(enc.attention_layers[li], h)
        fmaps.append(h)
        if li < 4:
            hs = _slot(3) if shared else None
            slots.append(hs)
    if skip_slots is not None:
        skip_slots[:] = slots
    return fmaps


def _upsampled(blk, h):           # (A) of DecoderBlock: resize-conv (default) or the ConvTranspose2d ablation path
    if blk.use_resize_conv:
        return ConvFn.apply(UpsampleFn.apply(h, int(blk.upsample_scale)), blk.conv_up.weight, blk.conv_up.bias, None, None, 1, 1)
    return conv_transpose2x(h, blk.transpose)


def decoder_block_forward(blk, cur, skip, t, tbd=None, sslot=None):
    """DecoderBlock.forward (reference score_unet.py:559-627) for a block WITH norms: NHWC in, NHWC out.  tbd: the block's time
    projection when the caller already computed it (decoder_forward batches the four blocks' projections)"""
    group = blk.norm_kind == "group"
    G1 = max(1, min(blk.gn_groups, blk.input_channels)) if group else blk.input_channels
    G2 = max(1, min(blk.gn_groups, blk.output_channels)) if group else blk.output_channels
    g = lambda n: (n.weight, n.bias) if group else (None, None)   # noqa: E731
    act = _ACT.get(type(blk.activation).__name__)
    if act is None:
        raise NotImplementedError(f"decoder activation {type(blk.activation).__name__} not implemented natively")
    up = _upsampled(blk, cur)
    if skip is not None:                                         # reference :596-597 (every block asserts this, also inside Decoder.forward)
        want = (up.shape[0], up.shape[1], up.shape[2], blk.output_channels)
        assert tuple(skip.shape) == want, f"prev_fmap shape {tuple(skip.shape)} (NHWC) must match output shape {want}"
    a = GroupNormFn.apply(up, *g(blk.norm1), None, None, N.NONE, G1, 1e-5)
    c2 = ConvFn.apply(a, blk.conv.weight, blk.conv.bias, None, None, 1, 1)
    if tbd is None and t is not None:
        tbd = _tproj(t, None, None, blk.sinusoidal_embedding, blk.time_projection_layer)
    out = GroupNormFn.apply(c2, *g(blk.norm2), skip, tbd, act, G2, 1e-5, sslot)
    if blk.compute_attn:
        out = _attention(blk.attention, out)
    return out


# Data-parallel overlap (parallel.GradientBucket): backward runs the decoder before the encoder, so the moment the gradient of the
# bottleneck feature map is delivered every decoder gradient is final.  An identity node there flushes the queued weight-gradient
# layout passes and starts the asynchronous all-reduce of the decoder's slice of the arena; it then runs beside the encoder's backward.
_OVERLAP_BUCKET = [None]


def set_overlap_bucket(bucket):
    """the GradientBucket whose decoder slice is all-reduced from inside backward (None: off); returns the previous one"""
    prev = _OVERLAP_BUCKET[0]
    _OVERLAP_BUCKET[0] = bucket
    return prev


class _BucketBoundary(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, dec, bucket):
        ctx.dec, ctx.bucket = dec, bucket
        return x.view_as(x)

    @staticmethod
    def backward(ctx, dy):
        if not (dy.is_cuda and torch.cuda.is_current_stream_capturing()):      # a captured step exchanges after the replay
            _STEP.flush_wgrad()                              # decoder weight gradients: slab -> OIHW slices of the arena, now
            ctx.bucket.begin_early([p for p in ctx.dec.parameters() if p.requires_grad])
        return dy, None, None


def decoder_forward(dec, fmaps, t, skip_slots=None):
    """Decoder.forward up to (not including) final_layer.conv: the 4 residual blocks and the final block's upsampling convolution"""
    cur = fmaps[4]
    if _OVERLAP_BUCKET[0] is not None and torch.is_grad_enabled() and cur.requires_grad:
        cur = _BucketBoundary.apply(cur, dec, _OVERLAP_BUCKET[0])
    blocks = list(dec.residual_layers)
    tbs = [None] * len(blocks)
    if t is not None and len(blocks) <= 8:                   # every block has its own embedding + projection (:606-609)
        n = len(blocks)
        tbs = TimeProjMultiFn.apply(t, None, None, tuple(range(n)), n, *[b.sinusoidal_embedding.W for b in blocks],
                                    *[b.time_projection_layer[1].weight for b in blocks], *[b.time_projection_layer[1].bias for b in blocks])
    for i, blk in enumerate(blocks):
        cur = decoder_block_forward(blk, cur, fmaps[3 - i], t, tbs[i], skip_slots[3 - i] if skip_slots else None)
    return _upsampled(dec.final_layer, cur)


# ---- stand-alone sub-module calls (reference score_unet.py: Encoder.forward :247-364, DecoderBlock.forward :559-627,
# Decoder.forward :733-758): NCHW tensors at the boundary like the reference, native ops inside ------------------------------------
def _nhwc(x):
    B, Cc, H, W = x.shape
    out = torch.empty(B, H, W, Cc, device=x.device)
    N.check(_L().sbgm_nchw_to_nhwc(N.f32c(x).data_ptr(), out.data_ptr(), B, H, W, Cc, _st()))
    return out


class _ToNCHW(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        B, H, W, Cc = x.shape
        out = torch.empty(B, Cc, H, W, device=x.device)
        N.check(_L().sbgm_nhwc_to_nchw(x.data_ptr(), out.data_ptr(), B, H, W, Cc, _st()))
        return out

    @staticmethod
    def backward(ctx, dy):
        return _ToNHWC.apply(dy.contiguous())


class _ToNHWC(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return _nhwc(x)

    @staticmethod
    def backward(ctx, dy):
        return _ToNCHW.apply(dy.contiguous())


def _standalone(dev, fn, *a):
    """run `fn` as a step of its own on `dev`: no plan, no arena"""
    _STEP.begin(dev)
    out = fn(*a)
    _STEP.bump_nbt()
    return out


def encoder_call(enc, x, t, y=None, cond_img=None, lsm_cond=None, topo_cond=None):
    N.require_device(x)
    for name, c in (("lsm_cond", lsm_cond), ("topo_cond", topo_cond)):
        if c is not None and c.shape[0] != x.shape[0]:
            raise ValueError(f"Batch mismatch: x= {x.shape[0]}, {name}={c.shape[0]}.")                  # reference :275,:280
    f = lambda v: None if v is None else N.f32c(v.to(x.device))   # noqa: E731
    t = N.f32c(t.to(x.device).view(-1))
    yl = None if y is None else y.to(x.device).long().contiguous()
    fm = _standalone(x.device, encoder_forward, enc, f(x), t, yl, f(cond_img), f(lsm_cond), f(topo_cond))
    return tuple(_ToNCHW.apply(v) for v in fm)


def decoder_block_call(blk, fmap, prev_fmap=None, t=None):
    N.require_device(fmap)
    if prev_fmap is not None and torch.is_tensor(prev_fmap):
        want = (fmap.shape[0], blk.output_channels, fmap.shape[2] * blk.upsample_scale, fmap.shape[3] * blk.upsample_scale)
        assert tuple(prev_fmap.shape) == want, f"prev_fmap shape {tuple(prev_fmap.shape)} must match output shape {want}"   # reference :596-597
    else:
        prev_fmap = None
    # the reference accepts raw timesteps [B] or a PRECOMPUTED embedding [B, time_dim] (score_unet.py:604-609): the latter skips the
    # block's SinusoidalEmbedding and goes straight through time_projection_layer = SiLU -> Linear
    t_emb = None
    if t is not None and t.dim() == 2 and t.shape[-1] == blk.time_embedding:
        t_emb, t = N.f32c(t.to(fmap.device)), None
    tt = None if t is None else N.f32c(t.to(fmap.device).view(-1))

    def run():
        cur, skip = _ToNHWC.apply(N.f32c(fmap)), (None if prev_fmap is None else _ToNHWC.apply(N.f32c(prev_fmap)))
        tbd = None
        if t_emb is not None:
            lin = blk.time_projection_layer[1]
            tbd = linear(ActFn.apply(t_emb, N.SILU), lin.weight, lin.bias)
        if isinstance(blk.norm1, torch.nn.Identity) and isinstance(blk.norm2, torch.nn.Identity):
            a = _upsampled(blk, cur)
            if blk.output_channels == 1 and skip is None and tt is None and tbd is None and isinstance(blk.activation, torch.nn.Identity):
                # the Decoder's final block: no norms, no skip, no time, identity activation (:726-730)
                return Cout1Fn.apply(a, blk.conv.weight, blk.conv.bias, None, 0.0)              # already NCHW [B,1,H,W]
            # any other block whose norms were replaced by Identity (what Decoder does to its final layer, applied elsewhere):
            # conv + skip + time projection ride on the convolution's epilogue, the activation and the attention follow
            if blk.output_channels % 32:
                raise NotImplementedError("a norm-free DecoderBlock needs output_channels % 32 == 0 (or the final layer's C -> 1 form)")
            act = _ACT.get(type(blk.activation).__name__)
            if act is None:
                raise NotImplementedError(f"decoder activation {type(blk.activation).__name__} not implemented natively")
            if tbd is None and tt is not None:
                tbd = _tproj(tt, None, None, blk.sinusoidal_embedding, blk.time_projection_layer)
            out = ConvFn.apply(a, blk.conv.weight, blk.conv.bias, skip, tbd, 1, 1)
            if act != N.NONE:
                out = ActFn.apply(out, act)
            if blk.compute_attn:
                out = _attention(blk.attention, out)
            return _ToNCHW.apply(out)
        return _ToNCHW.apply(decoder_block_forward(blk, cur, skip, tt, tbd))
    return _standalone(fmap.device, run)


def decoder_call(dec, *fmaps, t=None):
    assert len(fmaps) == len(dec.residual_layers) + 1
    N.require_device(*fmaps)
    tt = None if t is None else N.f32c(t.to(fmaps[0].device).view(-1))

    def run():
        nh = [_ToNHWC.apply(N.f32c(f)) for f in fmaps]
        a = decoder_forward(dec, nh, tt)
        fin = dec.final_layer
        return Cout1Fn.apply(a, fin.conv.weight, fin.conv.bias, None, 0.0)
    return _standalone(fmaps[0].device, run)
