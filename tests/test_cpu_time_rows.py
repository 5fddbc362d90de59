"""Host-side contract of an EM / PC run's time rows, without a device: where the nine time-bias vectors lie in a row, and
which row a run evaluates at after k completed steps."""
import ctypes as C

import pytest

from sbgm_danra_amd import _native as N

ENCODER = [64, 64, 128, 256, 512]                                  # the encoder's five maps (score_unet.py:198)


def layout(widths):
    off = (C.c_int * (len(widths) + 1))(*([-7] * (len(widths) + 1)))
    tb = N.lib().sbgm_time_row_layout((C.c_int * len(widths))(*widths), len(widths), off)
    return tb, list(off)


@pytest.mark.parametrize("decoder", [[256, 128, 64, 64], [512, 256, 128, 64], [128, 64, 32, 16], [4, 8, 12, 20]],
                         ids=["default", "wide", "narrow", "odd-quads"])
def test_row_layout_is_the_concatenation_in_forward_order(decoder):
    widths = ENCODER + decoder
    tb, off = layout(widths)
    assert tb == sum(widths) == off[-1] and off[0] == 0
    assert [b - a for a, b in zip(off, off[1:])] == widths         # vector i starts where vector i - 1 ends
    assert all(o % 4 == 0 for o in off)                            # the broadcast copies 16-byte quads


def test_default_row_length():
    assert layout(ENCODER + [256, 128, 64, 64])[0] == 1536


@pytest.mark.parametrize("widths", [[], [64] * 17, [64, 6], [64, 0], [64, -4]], ids=["none", "17", "not-a-quad", "zero", "negative"])
def test_row_layout_refuses_what_a_row_cannot_hold(widths):
    if widths:
        assert layout(widths)[0] == -1
    else:
        assert N.lib().sbgm_time_row_layout(None, 0, None) == -1


@pytest.mark.parametrize("n", [2, 3, 5, 500])
def test_row_index_after_k_advances(n):
    idx = N.lib().sbgm_time_row_index
    for k in [0, 1, 2, n - 2, n - 1, n, n + 3]:
        assert idx(k, n) == min(k, n - 1), (k, n)
