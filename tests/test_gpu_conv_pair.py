"""A BasicBlock's 3x3 / stride 2 convolution and its 1x1 / stride 2 shortcut in one launch (conv_igemm_pair_kernel): both kernels' bodies
are one device function, so sbgm_conv2d_pair_fwd must give the bits of two sbgm_conv2d_fwd calls with the same tiles; a combination
outside the instantiated set, or one with grid split-K, runs as two launches with the same result.  Network level: the forward and an
EM run against SBGM_NO_CONV_PAIR=1 in fresh interpreters (the switch is read once per process).

Shapes: B = 3, a 10 x 10 input -> 5 x 5 outputs, M = 75: a ragged last pixel tile for 16-, 32- and 64-pixel tiles.  Output channels are
one channel tile for one member and three for the other (a channel tile is 32 or 64 wide, so 48 channels are not a case: 32 against
96, 64 against 192), so an odd tile count leaves the last workgroup's last tile slot empty; the main problem's 2 to 9 workgroups are never a multiple
of 8, so the aux workgroups always start behind idle padding workgroups."""
import ctypes as C

import numpy as np
import pytest
import torch

from sbgm_danra_amd import _native as N
from util_step_runs import run_specs

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, HW = 3, 10

# (main tile, aux tile) = (channel fragments, pixel fragments, waves per tile): main with 2 and 4 waves per tile against aux with 1, 2, 4
SERVED = [((2, 2, 4), (2, 1, 4)), ((2, 2, 2), (2, 1, 2)), ((4, 2, 4), (2, 1, 1)), ((4, 2, 2), (4, 1, 1)), ((4, 2, 4), (4, 1, 4)),
          ((4, 2, 4), (2, 2, 2)), ((2, 2, 4), (2, 2, 4)), ((2, 1, 4), (2, 1, 4)), ((4, 4, 4), (4, 2, 2)), ((4, 2, 4), (4, 2, 4)),
          ((2, 1, 4), (2, 1, 2)), ((4, 2, 4), (2, 1, 2)), ((2, 2, 2), (4, 1, 2)), ((4, 2, 2), (2, 1, 4))]
NOT_SERVED = [((2, 2, 1), (2, 1, 1)), ((4, 4, 2), (2, 1, 4))]


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


class Conv:
    """one member: packed weight, folded-BatchNorm scale / bias, its output buffer and its arguments"""

    def __init__(self, x, cin, cout, k, pad, tile, relu, ws, splits=1, seed=0):
        lib = N.lib()
        w = rnd(cout, cin, k, k, seed=seed, scale=(k * k * cin) ** -0.5)
        self.packed = torch.empty(lib.sbgm_conv_packed_numel(cout, k, k, cin), device=DEV)
        N.check(lib.sbgm_conv_pack_weight(w.data_ptr(), self.packed.data_ptr(), cout, cin, k, k, cin, N.stream()))
        self.scale, self.bias = rnd(cout, seed=seed + 1).abs() + 0.5, rnd(cout, seed=seed + 2)
        self.shape = (B, HW // 2, HW // 2, cout)
        self.keep = (x, ws)
        self.args = lambda out: N.ConvArgs(x.data_ptr(), self.packed.data_ptr(), out.data_ptr(), self.scale.data_ptr(), self.bias.data_ptr(),
                                           None, None, B, HW, HW, cin, cout, k, k, 2, pad, N.RELU if relu else N.NONE, 1, tile[0], tile[1],
                                           splits, tile[2], 0, 0, 0, 0, ws.data_ptr(), ws.numel())

    def out(self):
        return torch.full(self.shape, float("nan"), device=DEV)


def run_both(tm, ta, cin, cm, ca, splits=1):
    """-> (paired flag, [main, aux] through the pair entry, [main, aux] through two single calls)"""
    lib = N.lib()
    x = rnd(B, HW, HW, cin, seed=3)
    ws = torch.zeros(8 * B * 25 * max(cm, ca), device=DEV)
    main = Conv(x, cin, cm, 3, 1, tm, True, ws, splits, seed=10)
    aux = Conv(x, cin, ca, 1, 0, ta, False, ws, 1, seed=20)
    pair, single = [main.out(), aux.out()], [main.out(), aux.out()]
    paired = C.c_int(-1)
    am, aa = main.args(pair[0]), aux.args(pair[1])
    N.check(lib.sbgm_conv2d_pair_fwd(C.byref(am), C.byref(aa), C.byref(paired), N.stream()))
    for conv, o in zip((main, aux), single):
        a = conv.args(o)
        N.check(lib.sbgm_conv2d_fwd(C.byref(a), N.stream()))
    torch.cuda.synchronize()
    return paired.value, [t.cpu() for t in pair], [t.cpu() for t in single]


def channels(tm, ta, wide_main):
    """one channel tile for one member, three for the other"""
    return (16 * tm[0] * (3 if wide_main else 1), 16 * ta[0] * (1 if wide_main else 3))


@pytest.mark.parametrize("wide_main", [False, True], ids=["aux-3-co-tiles", "main-3-co-tiles"])
@pytest.mark.parametrize("tm,ta", SERVED, ids=lambda t: "x".join(map(str, t)))
def test_pair_launch_equals_two_launches(tm, ta, wide_main):
    cm, ca = channels(tm, ta, wide_main)
    paired, pair, single = run_both(tm, ta, 16, cm, ca)
    assert paired == 1
    for got, want in zip(pair, single):
        assert torch.isfinite(want).all() and torch.equal(got, want)


def test_pair_launch_with_more_k_steps():
    """32 input channels: the shortcut has 2 K steps (its 4 waves per tile get 1, 1, 0, 0), the 3x3 has 18"""
    paired, pair, single = run_both((2, 2, 4), (2, 1, 4), 32, 32, 96)
    assert paired == 1 and all(torch.equal(g, w) for g, w in zip(pair, single))


@pytest.mark.parametrize("tm,ta", NOT_SERVED, ids=lambda t: "x".join(map(str, t)))
def test_other_tiles_fall_back_to_two_launches(tm, ta):
    paired, pair, single = run_both(tm, ta, 16, 64, 64)
    assert paired == 0 and all(torch.isfinite(w).all() and torch.equal(g, w) for g, w in zip(pair, single))


def test_grid_split_k_falls_back_to_two_launches():
    paired, pair, single = run_both((2, 2, 4), (2, 1, 4), 32, 32, 32, splits=2)
    assert paired == 0 and all(torch.isfinite(w).all() and torch.equal(g, w) for g, w in zip(pair, single))


# B = 33 at 32 x 32: layer2's pair (an 8 x 8 map, M = 528) is the first the static plan runs without grid split-K, as one launch
NETWORK = [dict(name="forward", kind="forward", B=33, N=0), dict(name="em", kind="em", B=33, N=3)]


def test_network_equals_the_two_launches(tmp_path):
    pair = run_specs(NETWORK, {}, tmp_path / "pair.npz")
    two = run_specs(NETWORK, {"SBGM_NO_CONV_PAIR": "1"}, tmp_path / "two.npz")
    for name in ("forward", "em"):
        assert np.isfinite(pair[name]).all() and np.array_equal(pair[name], two[name]), name
