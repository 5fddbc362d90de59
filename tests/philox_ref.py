"""Host reference of the in-kernel noise (csrc/philox.h): Philox4x32-10 (Salmon et al. 2011, the Random123 generator) plus
Box-Muller, in numpy only, vectorised over the element index.

Keying, as the kernels key it: counter = (idx lo, idx hi, offset lo, offset hi), key = (seed lo, seed hi), all 64-bit values split
into 32-bit words.  `uniform4` is a bit-exact emulation of the kernel's float32 expression; `normal4` feeds those exact float32
uniforms, the float32 angle product and the float32-rounded -2 ln u into float64 transcendentals, so what remains between it and the
device is the error of the device's logf / sqrtf / sincosf alone (see test_gpu_noise.py for the bound).
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57                # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85                # key schedule (Weyl) increments
MASK32 = np.uint64(0xFFFFFFFF)
TWO_PI_F32 = np.float32(6.283185307179586)
MASK64 = (1 << 64) - 1


def philox4x32_10(counter, key):
    """counter: 4 words, key: 2 words (Python ints or arrays of a common shape, values < 2^32) -> uint32 array [..., 4]"""
    c = [np.asarray(w, dtype=np.uint64) & MASK32 for w in counter]
    shape = np.broadcast(*c).shape
    c = [np.broadcast_to(w, shape).copy() for w in c]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]               # 32 x 32 -> 64 bits: exact in uint64
        p1 = np.uint64(M1) * c[2]
        n0 = (p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0)
        n2 = (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1)
        c = [n0, p1 & MASK32, n2, p0 & MASK32]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack(c, axis=-1).astype(np.uint32)


def counter_key(seed, offset, idx):
    """the kernels' keying: ((idx lo, idx hi, offset lo, offset hi), (seed lo, seed hi)); idx may be an array"""
    seed, offset = int(seed) & MASK64, int(offset) & MASK64
    idx = np.asarray(idx, dtype=np.uint64)
    return ((idx & MASK32, idx >> np.uint64(32), offset & 0xFFFFFFFF, offset >> 32), (seed & 0xFFFFFFFF, seed >> 32))


def uniform_from_bits(c):
    """uint32 words -> the kernel's float32 uniform ((float)(c >> 8) + 0.5f) * 2^-24, every step in float32.  c >> 8 + 0.5 is not
    representable from 2^23 on and rounds to even, so the interval is [2^-25, 1]: never 0, exactly 1 for c >> 8 == 2^24 - 1."""
    v = (np.asarray(c, dtype=np.uint32) >> np.uint32(8)).astype(np.float32)        # < 2^24: exact
    return (v + np.float32(0.5)) * np.float32(1.0 / 16777216.0)


def uniform4(seed, offset, idx):
    """float32 [..., 4]: the four uniforms of counter block (seed, offset, idx)"""
    return uniform_from_bits(philox4x32_10(*counter_key(seed, offset, idx)))


def box_muller(u):
    """float32 uniforms [..., 4] -> (z, r) float64 [..., 4]: lanes (r0 cos a0, r0 sin a0, r1 cos a1, r1 sin a1) with r0, a0 from
    (u0, u1) and r1, a1 from (u2, u3); r repeats the pair's radius on both of its lanes.  The float32 roundings of the kernel that do
    not depend on a math library are emulated: the angle is the float32 product 2pi_f32 * u, and -2 ln u is rounded to float32."""
    u = np.asarray(u, dtype=np.float32)
    m = (-2.0 * np.log(u[..., 0::2].astype(np.float64))).astype(np.float32)        # [..., 2]
    r = np.sqrt(np.maximum(m.astype(np.float64), 0.0))                            # max: -0.0 at u == 1
    a = (TWO_PI_F32 * u[..., 1::2]).astype(np.float64)                            # float32 product, then widened
    z = np.stack([r[..., 0] * np.cos(a[..., 0]), r[..., 0] * np.sin(a[..., 0]),
                  r[..., 1] * np.cos(a[..., 1]), r[..., 1] * np.sin(a[..., 1])], axis=-1)
    return z, np.repeat(r, 2, axis=-1)


def normal4(seed, offset, idx):
    """(z, r) float64 [..., 4] of counter block (seed, offset, idx)"""
    return box_muller(uniform4(seed, offset, idx))


def draw_with_radius(seed, offset, n):
    """(z, r) flat float64 [n]: quad i is normal4(seed, offset, i); n a multiple of 4"""
    assert n % 4 == 0
    z, r = normal4(seed, offset, np.arange(n // 4, dtype=np.uint64))
    return z.reshape(-1), r.reshape(-1)


def draw(seed, offset, n):
    """what sbgm_randn_scaled(x, 1.0, seed, offset, n) draws: flat float64 [n]"""
    return draw_with_radius(seed, offset, n)[0]


def domain_draw(seed, offset, Hd, Wd_pad):
    """draw `offset` of a tiled run over a domain of Hd x Wd_pad pixels (Wd_pad a multiple of 4), float64 [Hd, Wd_pad]: pixel (Y, X) is
    lane X % 4 of quad Y * Wd_pad/4 + X/4, whatever tile it is seen through"""
    assert Wd_pad % 4 == 0
    return draw(seed, offset, Hd * Wd_pad).reshape(Hd, Wd_pad)
