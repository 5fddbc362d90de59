"""Host definition of the row-keyed, temporally correlated noise: the weights, their autocorrelation in closed form, and
the float32 mixing loop z = w_0 xi_0; z = z + w_k xi_k (k ascending) over white draws, every product and sum rounded to float32."""
import numpy as np


def weights(rho, lags):
    """float32 [lags]: rho^k normalised to unit sum of squares in float64"""
    w = np.array([float(rho) ** k for k in range(int(lags))], dtype=np.float64)
    return (w / np.sqrt(np.sum(w * w))).astype(np.float32)


def acf_closed(rho, lags):
    """float64 [lags]: rho^j (1 - rho^(2(K-j))) / (1 - rho^(2K)), the lag-j autocorrelation of the exact weights; rho = 0: (1, 0, ...)"""
    K = int(lags)
    if rho == 0:
        return np.array([1.0] + [0.0] * (K - 1))
    return np.array([rho ** j * (1.0 - rho ** (2 * (K - j))) / (1.0 - rho ** (2 * K)) for j in range(K)], dtype=np.float64)


def mix(white, w):
    """white: K arrays (lag 0 first) of equal shape -> float32 array of that shape.  numpy multiplies and adds float32 arrays in float32,
    one rounding each: the definition's arithmetic."""
    w = np.asarray(w, dtype=np.float32)
    z = w[0] * np.asarray(white[0], dtype=np.float32)
    for k in range(1, len(w)):
        z = z + w[k] * np.asarray(white[k], dtype=np.float32)
    assert z.dtype == np.float32
    return z


def mix_rows(plain, rows, per, w, stride=1):
    """plain: flat white draw (what a run without a plan draws at that stream offset), long enough to hold row max(rows) -> float32
    [len(rows), per]: row r mixes plain[(r - k stride) per : (r - k stride + 1) per], k = 0 .. K-1"""
    plain = np.asarray(plain, dtype=np.float32).reshape(-1)
    out = []
    for r in rows:
        lagged = [plain[(int(r) - k * stride) * per:(int(r) - k * stride + 1) * per] for k in range(len(w))]
        assert all(int(r) - k * stride >= 0 for k in range(len(w))) and all(a.size == per for a in lagged)
        out.append(mix(lagged, w))
    return np.stack(out)
