"""Host statements of the skip the final mix forms in place (csrc/conv_final.hip, skip_from_x), shared by test_cpu_skip_mix.py and
test_gpu_skip_mix.py: the packed image of conv1's x-channel weights, the (k step, lane quarter) -> tap order of its 16 products, and
the fp64 chain of the block behind it."""
import torch
import torch.nn.functional as F

K_STEPS, QUARTERS, CO = 16, 4, 64


def pack_w1x(w1):
    """conv1.weight OIHW [64][Cin][8][8] -> the A operand [k step s][co][kq]: tap 4 s + kq = 8 v + u of input channel 0"""
    taps = w1[:, 0].reshape(CO, 64)                                  # [co][8 v + u]
    return taps.reshape(CO, K_STEPS, QUARTERS).permute(1, 0, 2).contiguous()


def tap_of(s, kq):
    """(v, u) of the filter tap that k step s, lane quarter kq multiplies"""
    tap = 4 * s + kq
    return tap >> 3, tap & 7


def conv1_x_by_steps(img, x):
    """what the kernel's 16 products per 16-channel fragment sum, in their order, from the packed image: x [B][1][H][W] ->
    [B][64][H/2][W/2]; a tap outside the image reads zero through a row mask and a column mask (never a linear index)"""
    B, _, H, W = x.shape
    h, w = H // 2, W // 2
    out = torch.zeros(B, CO, h, w, dtype=x.dtype)
    ly, lx = torch.arange(h), torch.arange(w)
    for s in range(K_STEPS):
        for kq in range(QUARTERS):
            v, u = tap_of(s, kq)
            iy, ix = 2 * ly + v - 3, 2 * lx + u - 3
            rows, cols = (iy >= 0) & (iy < H), (ix >= 0) & (ix < W)
            b = torch.zeros(B, h, w, dtype=x.dtype)
            b[:, rows.nonzero()[:, None, 0], cols.nonzero()[None, :, 0]] = x[:, 0][:, iy[rows]][:, :, ix[cols]]
            out += img[s, :, kq].to(x.dtype)[None, :, None, None] * b[:, None]
    return out


def conv1(w1, inp):
    """the encoder's stem convolution: 8x8, stride 2, padding 3, no bias"""
    return F.conv2d(inp, w1, stride=2, padding=3)


def skip_parts(w1, x, cond, tb0):
    """fp64: (conv1(x || cond) + tb0, conv1_x(x), conv1(0 || cond)) with x [B][1][H][W], cond [B][Cin-1][H][W] or None, tb0 [B][64]"""
    w1, x, tb0 = w1.double(), x.double(), tb0.double()
    full = torch.cat([x, cond.double()], dim=1) if cond is not None else x
    whole = conv1(w1, full) + tb0[:, :, None, None]
    xpart = conv1(w1[:, :1], x)
    cpart = conv1(w1, torch.cat([torch.zeros_like(x), cond.double()], dim=1)) if cond is not None else None
    return whole, xpart, cpart


def chain(raw, scale, shift, skip, fw1, fb1, fw2, fb2):
    """conv(conv_up(up(SiLU(raw * scale + shift + skip)))) in fp64: raw, skip [B][64][h][w], scale / shift [B][64]"""
    v = raw.double() * scale.double()[:, :, None, None] + shift.double()[:, :, None, None] + skip.double()
    up = F.interpolate(F.silu(v), scale_factor=2, mode="bilinear", align_corners=False)
    return F.conv2d(F.conv2d(up, fw1.double(), fb1.double(), padding=1), fw2.double(), fb2.double(), padding=1)
