"""float64 statements of a LayerNorm folded into the linear after it (sbgm_ln_fold_pack / sbgm_ln_linear_fwd) and the inputs the
tests of the fold share.

    LN(x) = r diag(gamma) (I - 11^T/C) x + beta,   r = 1/sqrt(var(x) + eps)
    linear(LN(x)) = r W'' x + h,   W'' = W diag(gamma) (I - 11^T/C),   h = b + W beta
"""
import functools
import math

import numpy as np

EPS = 1e-5
M_MAX = 2048
FAMILIES = ("centred", "relu", "shift4", "shift16", "shift64", "constant")


def fold64(w, b, gamma, beta):
    """W'' and h in float64 from float64 views of the fp32 operands"""
    w, b, gamma, beta = (np.asarray(a, np.float64) for a in (w, b, gamma, beta))
    wg = w * gamma[None, :]
    return wg - wg.sum(1, keepdims=True) / w.shape[1], b + w @ beta


def pack_host(w, b, gamma, beta):
    """The ABI's pack restated on the host: float64 sums, each result rounded to fp32 once; the image is [C/16][Cout][16]"""
    w2, h = fold64(w, b, gamma, beta)
    w2f, hf = w2.astype(np.float32), h.astype(np.float32)
    cout, c = w2f.shape
    image = np.ascontiguousarray(w2f.reshape(cout, c // 16, 16).transpose(1, 0, 2)).reshape(-1)
    return w2f, hf, image


def inv_sigma(x, eps=EPS):
    """r per row, two-pass in float64"""
    x = np.asarray(x, np.float64)
    d = x - x.mean(1, keepdims=True)
    return 1.0 / np.sqrt((d * d).mean(1) + eps)


def layernorm_linear(x, w, b, gamma, beta, eps=EPS):
    """the chain the fold replaces, in float64: Linear(LayerNorm(x))"""
    x, w, b, gamma, beta = (np.asarray(a, np.float64) for a in (x, w, b, gamma, beta))
    d = x - x.mean(1, keepdims=True)
    n = d * inv_sigma(x, eps)[:, None] * gamma[None, :] + beta[None, :]
    return n @ w.T + b[None, :]


def gelu(v):
    import torch            # float64 erf over a whole array (the GPU tests only)
    t = torch.from_numpy(np.ascontiguousarray(v, np.float64))
    return (0.5 * t * (1.0 + torch.erf(t / math.sqrt(2.0)))).numpy()


def rows(C, m=M_MAX, seed=0):
    """fp32 rows [m][C]: row i is of family FAMILIES[i % 6], except that row 5 alone is constant (the later rows of that slot are
    centred), so the first 16 rows hold every family: centred normal; ReLU of a normal (|mean|/sigma ~ 0.8); a unit normal shifted to
    |mean|/sigma = 4, 16 and 64 (sign alternating); one constant row.  A constant row has sigma = 0, so what plays the part of
    |mean|/sigma in the fold is |c| / sqrt(eps); its value 13/64 puts that at 64.2, the conditioning of the most shifted rows"""
    g = np.random.default_rng(1000 + C + seed)
    x = g.standard_normal((m, C))
    fam = np.arange(m) % 6
    x[fam == 1] = np.maximum(x[fam == 1], 0.0)
    for k, shift in ((2, 4.0), (3, 16.0), (4, 64.0)):
        idx = np.nonzero(fam == k)[0]
        z = x[idx]
        z = (z - z.mean(1, keepdims=True)) / z.std(1, keepdims=True)
        x[idx] = (z + shift * np.where(idx % 4 < 2, 1.0, -1.0)[:, None]) * 0.7
    x[5] = 13.0 / 64.0
    return x.astype(np.float32)


def row_family(i):
    return "constant" if i == 5 else "centred" if i % 6 == 5 else FAMILIES[i % 6]


@functools.lru_cache(maxsize=None)
def case(C, Cout):
    """Operands and float64 results of one (C, Cout), computed once for M_MAX rows and left unchanged; the rows of every quantity are
    independent of each other, so the case of M rows is its first M rows.
    want: Linear(LayerNorm(x)); bracket: r sum_k |W''[co][k]| |x_k|; res: a residual; want_act: GELU(want + res), pre = want + res"""
    g = np.random.default_rng(7 * C + Cout)
    x = rows(C)
    w = (g.standard_normal((Cout, C)) / math.sqrt(C)).astype(np.float32)
    b = (g.standard_normal(Cout) * 0.1).astype(np.float32)
    gamma = (g.standard_normal(C) * 0.2 + 1.0).astype(np.float32)
    beta = (g.standard_normal(C) * 0.2).astype(np.float32)
    res = g.standard_normal((M_MAX, Cout)).astype(np.float32)
    w2, h = fold64(w, b, gamma, beta)
    want = layernorm_linear(x, w, b, gamma, beta)
    bracket = inv_sigma(x)[:, None] * (np.abs(x.astype(np.float64)) @ np.abs(w2).T)
    pre = want + res
    return dict(x=x, w=w, b=b, gamma=gamma, beta=beta, res=res, w2=w2, h=h, want=want, bracket=bracket, pre=pre, want_act=gelu(pre))
