"""Plain references, input builders and the row-wise error for the attention kernels (tests only, CPU, no device).

References (any dtype; the tests use float64 as the truth and float32 as the yardstick of what fp32 arithmetic can give):
  mha_core       softmax(q k^T / sqrt(d)) v per (sample, head) on a packed qkv [B, S, 3C]
  mha_core_grad  its autograd gradient with respect to qkv
  attn_in        LayerNorm1 + in_proj;  attn_tail: out_proj + residual + LayerNorm2 + FF + residual

Row-wise error: max|got - want| over one row of one head divided by max|want| over the same row.  A whole-tensor norm
hides a mis-masked ragged key, a lost rescale in one wave's partial, or one bad query row out of thousands; this does not.
head_error measures the same rows on the scale of their (sample, head), for the cases where a row's own scale is lost in fp32.

Input builders, all derived from one seed: plain, offset, late spike, gather (see each function), and Poisoned, which puts
a tensor inside a larger NaN-filled allocation.
"""
import math

import torch
import torch.nn.functional as F

SEED = 20240611
ULP = 2.0 ** -23                      # spacing of fp32 at 1
FLOOR = 8 * ULP                       # no tolerance below 8 ulp of fp32
GATHER_MASS = 1e-6                    # a gather row keeps more than 1 - GATHER_MASS of its mass on its key


def gen(*salt):
    """a generator derived from the one seed and the case (shape, kind)"""
    s = SEED
    for v in salt:
        s = (s * 1000003 + int(v)) % (2 ** 62)
    return torch.Generator().manual_seed(s)


# ---------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------
def split_heads(qkv, heads):
    """qkv [B, S, 3C] -> q, k, v [B, heads, S, d]"""
    B, S, C3 = qkv.shape
    C = C3 // 3
    return [t.reshape(B, S, heads, C // heads).transpose(1, 2) for t in qkv.split(C, dim=-1)]


def probabilities(qkv, heads, dtype=torch.float64):
    q, k, _ = split_heads(qkv.to(dtype), heads)
    return torch.softmax((q @ k.transpose(-1, -2)) / math.sqrt(q.shape[-1]), -1)


def mha_core(qkv, heads, dtype=torch.float64):
    """[B, S, 3C] -> [B, S, C], every operation in `dtype`"""
    B, S, C3 = qkv.shape
    _, _, v = split_heads(qkv.to(dtype), heads)
    return (probabilities(qkv, heads, dtype) @ v).transpose(1, 2).reshape(B, S, C3 // 3)


def mha_core_grad(qkv, dout, heads, dtype=torch.float64):
    """d(sum(mha_core(qkv) * dout)) / d qkv by autograd, in `dtype`"""
    x = qkv.to(dtype).clone().requires_grad_(True)
    mha_core(x, heads, dtype).backward(dout.to(dtype))
    return x.grad


def attn_in(x, g, b, w, bias, dtype=torch.float64, eps=1e-5):
    x, g, b, w, bias = [t.to(dtype) for t in (x, g, b, w, bias)]
    return F.linear(F.layer_norm(x, (x.shape[-1],), g, b, eps), w, bias)


def attn_tail(att, x, wo, bo, g, b, w1, b1, w2, b2, dtype=torch.float64, eps=1e-5):
    att, x, wo, bo, g, b, w1, b1, w2, b2 = [t.to(dtype) for t in (att, x, wo, bo, g, b, w1, b1, w2, b2)]
    h = x + F.linear(att, wo, bo)
    return h + F.linear(F.gelu(F.linear(F.layer_norm(h, (x.shape[-1],), g, b, eps), w1, b1)), w2, b2)


# ---------------------------------------------------------------------------------------------------------------------
# row-wise error
# ---------------------------------------------------------------------------------------------------------------------
def row_error(got, want, heads=1):
    """got, want [B, S, heads * d] -> [B, heads, S]: max|got - want| / max|want| over the d elements of each (b, h, row).
    A row with a NaN or an infinity in `got` gets an infinite error."""
    B, S, C = want.shape
    g = got.double().reshape(B, S, heads, C // heads)
    w = want.double().reshape(B, S, heads, C // heads)
    err = (g - w).abs().amax(-1) / w.abs().amax(-1).clamp_min(1e-300)
    err = torch.where(torch.isfinite(g).all(-1), err, torch.full_like(err, float("inf")))
    return err.transpose(1, 2)


def head_error(got, want, heads=1):
    """[B, heads, S]: max|got - want| over one row of one head divided by max|want| over ALL rows of that (sample, head).
    The companion of row_error for rows whose true values nearly vanish (the dQ row of a query whose softmax is saturated on
    one key): there fp32 keeps no digit of the row itself, row_error of any fp32 evaluation is of order one, and a tolerance
    drawn from it says nothing about the other rows.  On the scale of the head such a row is held to the same few ulp as
    every other row, and a wrong row of ordinary size stands out just the same."""
    B, S, C = want.shape
    g = got.double().reshape(B, S, heads, C // heads)
    w = want.double().reshape(B, S, heads, C // heads)
    err = (g - w).abs().amax(-1) / w.abs().amax(dim=(1, 3)).clamp_min(1e-300)[:, None, :]
    err = torch.where(torch.isfinite(g).all(-1), err, torch.full_like(err, float("inf")))
    return err.transpose(1, 2)


def worst_row(err):
    """[B, heads, S] -> (value, (b, h, row))"""
    i = int(torch.argmax(err))
    _, H, S = err.shape
    return float(err.reshape(-1)[i]), (i // (H * S), i // S % H, i % S)


def tolerance(fp32_err, factor=4.0):
    """what a kernel row may be off by: `factor` x the largest row error of the same expression evaluated in fp32 on the
    CPU for this case, never tighter than 8 ulp of fp32"""
    return max(factor * float(fp32_err.max()), FLOOR)


# ---------------------------------------------------------------------------------------------------------------------
# input builders
# ---------------------------------------------------------------------------------------------------------------------
def plain(B, S, C, heads, salt=0):
    """N(0, 1) * 0.7"""
    return torch.randn(B, S, 3 * C, generator=gen(B, S, C, heads, salt)) * 0.7


OFFSET_LOGIT = 120.0                  # the common term of every logit of a query, far above log(FLT_MAX) = 88.7


def offset(B, S, C, heads):
    """q, k, v with mean 3, and a constant vector added to every key of a head, sized so that all logits of a query share a
    term of about OFFSET_LOGIT: exp() of a logit overflows fp32, only the subtraction of the row maximum keeps it finite."""
    d = C // heads
    x = plain(B, S, C, heads, 1) + 3.0
    x[..., C:2 * C] += OFFSET_LOGIT / (3.0 * math.sqrt(d))          # q . c / sqrt(d) ~ 3 a d / sqrt(d) = OFFSET_LOGIT
    return x


SPIKE = 25.0


def spike_positions(S):
    """keys at which the running maximum of an online softmax must jump late, deduplicated, ascending: a key of the
    fourth of four key blocks dealt round-robin to the waves (48 .. 63), the first key of the second 128-key chunk, the
    first key of the last key block, and key S - 1"""
    cand = [50, 128, (S - 1) // 16 * 16, S - 1]
    return sorted({p for p in cand if 0 < p < S})


def late_spike(B, S, C, heads, pos):
    """plain, with key `pos` of every (sample, head) scaled by SPIKE: the queries aligned with it meet their maximum there"""
    x = plain(B, S, C, heads, 2)
    x[:, pos, C:2 * C] *= SPIKE
    return x


def gather(B, S, C, heads):
    """-> (qkv, pi [B, heads, S], v [B, heads, S, d]).  Unit keys, q_i = alpha * k_pi(i) with alpha sized from the smallest
    gap between a key's self product and its product with any other key, so that row i keeps more than 1 - GATHER_MASS of its
    float64 softmax mass on key pi(i); pi is a random permutation per (sample, head) (so every key, 0, 15, 16, 127, 128 and
    S - 1 among them, is some row's target) with pi(0) = S - 1 and pi(S - 1) = 0.  v[j][e] = +-(j + 1 + e / 512) encodes
    the key and the element exactly in fp32, the sign alternating with the (sample, head): the output row must be v[pi(i)]."""
    d = C // heads
    g = gen(B, S, C, heads, 3)
    k = torch.randn(B, heads, S, d, generator=g, dtype=torch.float64)
    k = (k / k.norm(dim=-1, keepdim=True)).float()
    pi = torch.argsort(torch.rand(B, heads, S, generator=g), dim=-1)
    if S > 1:
        for t, want in ((0, S - 1), (S - 1, 0)):                    # swap so that pi stays a permutation
            at = (pi == want).nonzero()[:, 2].reshape(B, heads, 1)
            pi.scatter_(2, at, pi[:, :, t:t + 1].clone())
            pi[:, :, t] = want
    kk = k.double() @ k.double().transpose(-1, -2)                  # [B, heads, S, S]
    self_prod = kk.diagonal(dim1=-2, dim2=-1)
    others = kk - torch.diag_embed(torch.full((S,), float("inf"), dtype=torch.float64))
    gap = float((self_prod - others.amax(-1)).min()) if S > 1 else 1.0
    margin = math.log(max(S - 1, 1) / GATHER_MASS) + 2.0            # (S - 1) e^-margin < GATHER_MASS, with room for fp32 rounding of q
    alpha = margin * math.sqrt(d) / gap
    q = (alpha * torch.gather(k.double(), 2, pi[..., None].expand(-1, -1, -1, d))).float()
    sign = 1.0 - 2.0 * (torch.arange(B * heads).reshape(B, heads, 1, 1) % 2)
    v = (sign * (torch.arange(1, S + 1).reshape(1, 1, S, 1) + torch.arange(d).reshape(1, 1, 1, d) / 512.0)).float().expand(B, heads, S, d)
    qkv = torch.cat([t.transpose(1, 2).reshape(B, S, C) for t in (q, k, v)], -1).contiguous()
    return qkv, pi, v


def gather_expected(pi, v):
    """the rows v[pi(i)] as [B, S, C]"""
    B, H, S, d = v.shape
    return torch.gather(v, 2, pi[..., None].expand(-1, -1, -1, d)).transpose(1, 2).reshape(B, S, H * d)


def ulp_of(x):
    """spacing of fp32 at |x| (elementwise, float64 result)"""
    _, e = torch.frexp(x.double().abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(x, dtype=torch.float64), e - 24)


def gather_bound(qkv, heads, expected):
    """[B, S, C] absolute bound per element: the leakage of the other keys into the row, computed in float64, plus 8 ulp"""
    leak = (mha_core(qkv, heads) - expected.double()).abs()
    B, S, C = leak.shape
    leak = leak.reshape(B, S, heads, C // heads).amax(-1, keepdim=True).expand(-1, -1, -1, C // heads).reshape(B, S, C)
    return leak + 8 * ulp_of(expected)


class Poisoned:
    """A tensor that lives inside a larger allocation whose other elements are NaN: PAD floats directly before its first
    element and PAD after its last.  All of it is allocated memory, so an access past the tensor cannot fault; a read that is
    only "masked" by a multiplication with zero turns into a NaN in the result, and a write shows in check()."""
    PAD = 256                          # floats; a multiple of 4 keeps the tensor 16-byte aligned like any allocation

    def __init__(self, shape, device, value=None):
        n = math.prod(shape)
        self.buf = torch.full((n + 2 * self.PAD,), float("nan"), device=device)
        self.t = self.buf[self.PAD:self.PAD + n].view(*shape)
        if value is not None:
            self.t.copy_(value)
        self.before = self._surround().clone()

    def _surround(self):
        return torch.cat([self.buf[:self.PAD], self.buf[-self.PAD:]]).view(torch.int32)

    def ptr(self):
        return self.t.data_ptr()

    def surround_unchanged(self):
        return torch.equal(self._surround(), self.before)
