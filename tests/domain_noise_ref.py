"""Host restatement of the domain noise plan ("domain rows"): the Philox counter of a domain quad under a noise row and
the float32 mix over the lags, on the host Philox of philox_ref.py.

    dom_w4 = ceil(domain_width / 4),  Q = domain_height * dom_w4
    counter(R, k; Y, X4) = (R - k stride) Q + Y dom_w4 + X4          (64-bit unsigned)
    z = w_0 xi_0;  z = z + w_k xi_k  in ascending k, float32 products and sums (temporal_noise_ref.mix)."""
import numpy as np

import philox_ref as P
import temporal_noise_ref as R


def counters(row, lag, stride, domain_h, domain_w):
    """uint64 [domain_h, dom_w4]: the counter of every domain quad for the white draw of lag `lag` under the noise row `row`"""
    dom_w4 = (int(domain_w) + 3) // 4
    Q = int(domain_h) * dom_w4
    base = (int(row) - int(lag) * int(stride)) * Q
    assert 0 <= base and base + Q <= (1 << 64)
    Y, X4 = np.meshgrid(np.arange(domain_h, dtype=np.uint64), np.arange(dom_w4, dtype=np.uint64), indexing="ij")
    return np.uint64(base) + Y * np.uint64(dom_w4) + X4


def white(seed, offset, row, lag, stride, domain_h, domain_w):
    """float32 [domain_h, 4 dom_w4]: the white draw of lag `lag`; pixel (Y, X) is lane X % 4 of the quad (Y, X // 4)"""
    z, _ = P.normal4(seed, offset, counters(row, lag, stride, domain_h, domain_w))
    return z.reshape(int(domain_h), -1).astype(np.float32)


def domain_draw(seed, offset, row, domain_h, domain_w, w, stride=1):
    """float32 [domain_h, 4 dom_w4]: the mixed draw of the domain under the noise row `row`"""
    return R.mix([white(seed, offset, row, k, stride, domain_h, domain_w) for k in range(len(w))], w)


def cut(dom, origins, tile):
    """[T, tile, tile]: the windows of a domain field at the tile origins"""
    return np.stack([dom[y0:y0 + tile, x0:x0 + tile] for y0, x0 in origins])
