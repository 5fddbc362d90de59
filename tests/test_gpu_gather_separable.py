"""The two-pass gather of a small-map decoder block (csrc/conv_uplow.hip) through sbgm_up_lowres_fwd against the fp64 CPU chain
group_norm(conv_up(interpolate(x))): either side of every boundary of the kernel's LDS plan, small and ragged maps, every
register-resident item count and the read-back form, maps with more columns than a workgroup has threads, one-hot inputs at the corners
and an edge, and run-to-run / graph-replay determinism.  Output and workspace start as NaN, so an element that is read but never written
shows.

The plan, per workgroup (a sample's slice of CW channels; CW = C / groups with GroupNorm, 16 without), in bytes per low-res pixel:
  Z with all 9 taps beside R: 60 CW, one staging;  else Z one tap row at a time beside R: 36 CW, three stagings;  else row chunks of the
  latter with partial statistics.  The LDS holds 160 KiB - 512 = 163328 bytes, so with CW = 64 (C = 64 in one group) a map of 42 pixels
  is the last single staging (161280 bytes), 70 pixels the last single workgroup (161280 bytes), 72 pixels the first in chunks.
A workgroup has 1024 threads; a thread keeps one of the 2 w CW / 4 (column, channel quad) pairs and walks rows r0, r0 + rpp, ..,
rpp = 1024 / pairs, so it owns ceil(2 h / rpp) output values: kept in registers across the statistics barrier in the instantiations for
1, 2, 4 and 8 values.  More pairs than threads takes the general form that reads its own stores back; a map that fits one workgroup's
LDS never has more than 8 values per thread otherwise (h w CW <= 4537 floats of a tap, and 2 h > 8 rpp needs more)."""
import pytest
import torch
import torch.nn.functional as F

from sbgm_danra_amd import _native as N

pytestmark = pytest.mark.gpu

DEV = "cuda"
BOUND = 2e-5            # the project's bound for a kernel against fp64 (test_gpu_up_lowres.py)
EPS = 1e-5
THREADS = 1024          # conv_uplow.hip: up_threads()


def relerr(got, want):
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-30))


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return torch.randn(*shape, generator=g) * scale


def chain(x, w, b, groups=0, gamma=None, beta=None):
    """group_norm(conv_up(interpolate(x))) in fp64 on the CPU"""
    up = F.interpolate(x.double(), scale_factor=2, mode="bilinear", align_corners=False)
    out = F.conv2d(up, w.double(), b.double(), padding=1)
    if groups:
        out = F.group_norm(out, groups, None if gamma is None else gamma.double(), None if beta is None else beta.double(), eps=EPS)
    return out.float()


class Block:
    """conv_up's weight and bias, norm1's affine, and the mix's packed 1x1 weight on the device"""

    def __init__(self, c, seed=1):
        self.c = c
        self.w, self.b = rnd(c, c, 3, 3, seed=seed, scale=(9 * c) ** -0.5), rnd(c, seed=seed + 1, scale=0.5)
        self.gamma, self.beta = rnd(c, seed=seed + 2).abs() + 0.5, rnd(c, seed=seed + 3)
        lib, n = N.lib(), N.lib().sbgm_up_lowres_weight_numel(c)
        taps = torch.full((n,), float("nan"), device=DEV)
        self.packed = torch.full((n,), float("nan"), device=DEV)
        N.check(lib.sbgm_up_lowres_pack(self.w.contiguous().to(DEV).data_ptr(), taps.data_ptr(), self.packed.data_ptr(), c, N.stream()))
        torch.cuda.synchronize()

    def operands(self, x, b, groups, gamma, beta):
        B, c, h, w = x.shape
        dev = lambda t: None if t is None else t.contiguous().to(DEV)  # noqa: E731
        ws = torch.full((N.lib().sbgm_up_lowres_ws_numel(B, 2 * h, 2 * w, c, groups),), float("nan"), device=DEV)
        out = torch.full((B, 2 * h, 2 * w, c), float("nan"), device=DEV)
        return x.permute(0, 2, 3, 1).contiguous().to(DEV), dev(b), dev(gamma), dev(beta), ws, out

    def launch(self, ops, groups):
        xd, bd, gd, btd, ws, out = ops
        B, H, W, c = out.shape
        N.check(N.lib().sbgm_up_lowres_fwd(xd.data_ptr(), self.packed.data_ptr(), bd.data_ptr(), N.ptr(gd), N.ptr(btd), groups, EPS,
                                           out.data_ptr(), ws.data_ptr(), ws.numel(), B, H, W, c, N.stream()))

    def run(self, x, groups=0, affine=True, b=None):
        """x: low-resolution NCHW (CPU) -> the block's output NCHW [B,C,2h,2w] (CPU)"""
        b = self.b if b is None else b
        ops = self.operands(x, b, groups, self.gamma if groups and affine else None, self.beta if groups and affine else None)
        self.launch(ops, groups)
        torch.cuda.synchronize()
        return ops[-1].permute(0, 3, 1, 2).cpu()

    def want(self, x, groups=0, affine=True, b=None):
        b = self.b if b is None else b
        return chain(x, self.w, b, groups, self.gamma if groups and affine else None, self.beta if groups and affine else None)


@pytest.fixture(scope="module")
def blocks():
    return {c: Block(c) for c in (32, 64)}


def values_per_thread(h, w, cw):
    """-> the kernel's register-resident instantiation for a whole (sample, group) in one workgroup, 0: the read-back form"""
    pairs = 2 * w * cw // 4
    if pairs > THREADS:
        return 0
    n = -(-2 * h // (THREADS // pairs))
    return next((k for k in (1, 2, 4, 8) if n <= k), 0)


def check(blk, hw, groups, seed=2):
    x = rnd(2, blk.c, *hw, seed=seed)
    want, got = blk.want(x, groups), blk.run(x, groups)
    assert got.shape == want.shape and torch.isfinite(got).all()
    err = relerr(got, want)
    print(f"two-pass gather {hw} C={blk.c} groups={groups}: max-rel {err:.2e} against the fp64 chain (bound {BOUND:.0e})")
    assert err < BOUND


# C = 64 in ONE group (a 64-channel slice, the widest of the network): either side of the two boundaries of the LDS plan.
#   6x7  = 42 px: the last single staging;           12 rows over 4 per sweep: 3 values, the 4-value instantiation
#   8x8  = 64 px: a tap row at a time (C4's slice);   16 rows over 4 per sweep: the 4-value instantiation, full
#   7x10 = 70 px: the last single workgroup;          14 rows over 3 per sweep: 5 values, the 8-value instantiation
#   8x9  = 72 px: row chunks and partial statistics, finished by groupnorm_apply
PLAN = [(6, 7), (8, 8), (7, 10), (8, 9)]


@pytest.mark.parametrize("hw", PLAN, ids=lambda v: "x".join(map(str, v)))
@pytest.mark.parametrize("norm", [False, True], ids=["raw", "groupnorm"])
def test_lds_plan_boundaries(blocks, hw, norm):
    lds_max, px = 160 * 1024 - 512, hw[0] * hw[1]
    assert {(6, 7): px * 60 * 64 <= lds_max < (px + 1) * 60 * 64, (8, 8): px * 60 * 64 > lds_max >= px * 36 * 64,
            (7, 10): px * 36 * 64 <= lds_max < (px + 1) * 36 * 64, (8, 9): px * 36 * 64 > lds_max}[hw]
    if hw != (8, 9):                                   # one workgroup per (sample, group)
        assert values_per_thread(*hw, 64) == {(6, 7): 4, (8, 8): 4, (7, 10): 8}[hw]
    check(blocks[64], hw, 1 if norm else 0)


# Small and ragged maps: raw in 16-channel slices, C = 32 and C = 64 in 8 groups (4- and 8-channel slices): one value per thread.  The raw
# case runs at C = 32, not 16: sbgm_up_lowres_fwd's tap mix is the implicit-GEMM convolution, whose smallest tile has 32 output rows, and
# 9 * 16 = 144 is no multiple of that.  The gather cuts a raw map into 16-channel slices whatever C is, so this is the same slice, twice.
@pytest.mark.parametrize("hw", [(1, 1), (2, 3), (3, 5)], ids=lambda v: "x".join(map(str, v)))
@pytest.mark.parametrize("c,groups", [(32, 0), (32, 8), (64, 8)])
def test_small_and_ragged_maps(blocks, hw, c, groups):
    if groups:
        assert values_per_thread(*hw, c // groups) == 1
    check(blocks[c], hw, groups, seed=3)


# Every register-resident instantiation and the read-back form, C = 64 in one group (pairs = 32 w):
#   1x1: 32 pairs, 32 rows per sweep, 2 rows -> 1;   3x7: 224 pairs, 4 per sweep, 6 rows -> 2;   5x7: 10 rows -> 3: the 4-value instantiation
#   with a row to spare;   9x7: 18 rows -> 5: the 8-value instantiation (a tap row at a time);
#   2x33: 1056 pairs, more than the workgroup has threads: the general form with two columns per thread, and read-back
ITEMS = [((1, 1), 1), ((3, 7), 2), ((5, 7), 4), ((9, 7), 8), ((2, 33), 0)]


@pytest.mark.parametrize("hw,ni", ITEMS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"ni{v}")
@pytest.mark.parametrize("affine", [True, False], ids=["affine", "plain"])
def test_item_count_instantiations(blocks, hw, ni, affine):
    assert values_per_thread(*hw, 64) == ni
    blk = blocks[64]
    x = rnd(2, 64, *hw, seed=4)
    err = relerr(blk.run(x, 1, affine), blk.want(x, 1, affine))
    print(f"two-pass gather {hw}, {ni or 'read-back'} values per thread, affine={affine}: max-rel {err:.2e}")
    assert err < BOUND


def test_raw_map_with_more_columns_than_threads(blocks):
    """raw 16-channel slices of a 1x130 map: 2 * 130 * 4 = 1040 (column, quad) pairs for 1024 threads"""
    check(blocks[32], (1, 130), 0, seed=5)


@pytest.mark.parametrize("groups", [0, 1, 8], ids=["raw", "one-group", "eight-groups"])
def test_one_hot_inputs(blocks, groups):
    """single low-resolution pixels of a 3x5 map: the four corners and an edge midpoint.  A wrong clamp, shift or padding test shows as
    a misplaced or missing copy of the filter"""
    blk, h, w = blocks[64], 3, 5
    pts = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 2), (h // 2, 0)]
    x = torch.zeros(len(pts), 64, h, w)
    for i, (py, px) in enumerate(pts):
        x[i, (7 * i) % 64, py, px] = 1.0
    zb = torch.zeros(64)
    want, got = blk.want(x, groups, b=zb), blk.run(x, groups, b=zb)
    assert torch.isfinite(got).all()
    for i in range(len(pts)):
        assert relerr(got[i], want[i]) < BOUND, pts[i]


@pytest.mark.parametrize("hw,groups", [((8, 8), 1), ((5, 7), 8), ((8, 9), 1), ((5, 7), 0)], ids=["tap-rows", "registers", "chunks", "raw"])
def test_same_call_twice_and_graph_replay_are_bitwise_equal(blocks, hw, groups):
    blk = blocks[64]
    x = rnd(2, 64, *hw, seed=6)
    ops = blk.operands(x, blk.b, groups, blk.gamma if groups else None, blk.beta if groups else None)
    out = ops[-1]
    blk.launch(ops, groups)
    torch.cuda.synchronize()
    eager = out.clone()
    assert torch.isfinite(eager).all()
    out.fill_(float("nan"))
    blk.launch(ops, groups)
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        blk.launch(ops, groups)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        blk.launch(ops, groups)
    for _ in range(3):
        out.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
