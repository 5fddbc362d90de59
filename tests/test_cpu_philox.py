"""The host reference of the in-kernel noise (philox_ref.py) against the published generator and against its own claims: the Random123
known-answer vectors of philox4x32-10, the float32 uniform conversion at its rounding edges (interval [2^-25, 1], ties to even), the
64-bit keying, the moments of a draw, and the distance between the float32-emulating Box-Muller and a pure float64 one."""
import numpy as np
import pytest

import philox_ref as P

KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.mark.parametrize("counter,key,want", KAT)
def test_known_answer_vectors(counter, key, want):
    assert tuple(int(v) for v in P.philox4x32_10(counter, key)) == want


def test_known_answer_vectors_through_the_keying_and_vectorised():
    # the same three blocks addressed as (seed, offset, idx), and all three counters of one key in one vectorised call
    for (c0, c1, c2, c3), (k0, k1), want in KAT:
        ck = P.counter_key(k0 | (k1 << 32), c2 | (c3 << 32), c0 | (c1 << 32))
        assert tuple(int(v) for v in P.philox4x32_10(*ck)) == want
    cs = np.array([k[0] for k in KAT], dtype=np.uint64)
    out = P.philox4x32_10(tuple(cs[:, i] for i in range(4)), (0, 0))
    assert out.shape == (3, 4) and tuple(int(v) for v in out[0]) == KAT[0][2]


def test_uniform_conversion_edges():
    v = np.array([0, 1, 2**23 - 1, 2**23, 2**23 + 1, 2**24 - 2, 2**24 - 1], dtype=np.uint32)
    # v + 0.5 in float32: exact below 2^23, then a tie between two integers that goes to the even one
    rounded = np.array([0.5, 1.5, 2**23 - 0.5, 2**23, 2**23 + 2, 2**24 - 2, 2**24], dtype=np.float64)
    for low_bits in (0, 0xFF):                                           # the low 8 bits are discarded
        u = P.uniform_from_bits((v << np.uint32(8)) | np.uint32(low_bits))
        assert u.dtype == np.float32
        assert np.array_equal(u.astype(np.float64), rounded * 2.0**-24)
    assert u[0] == np.float32(2.0**-25) and u[-1] == np.float32(1.0)      # the interval is [2^-25, 1]
    z, r = P.box_muller(np.array([1.0, 0.25, 2.0**-25, 1.0], dtype=np.float32))
    assert r[0] == 0 and z[0] == 0 and z[1] == 0                          # u == 1: radius 0
    assert abs(r[2] - np.sqrt(50 * np.log(2.0))) < 1e-6                   # the largest radius, 5.887
    assert np.isfinite(z).all()


def test_high_words_enter_the_counter_and_the_key():
    base = P.counter_key(7, 3, 5)
    for kw, where, word in ((dict(idx=5 + (9 << 32)), 0, 1), (dict(offset=3 + (9 << 32)), 0, 3), (dict(seed=7 + (9 << 32)), 1, 1)):
        args = dict(seed=7, offset=3, idx=5)
        args.update(kw)
        ck = P.counter_key(**args)
        flat = lambda t: [int(w) for w in t[0]] + [int(w) for w in t[1]]  # noqa: E731
        diff = [i for i, (a, b) in enumerate(zip(flat(base), flat(ck))) if a != b]
        assert diff == [4 * where + word] and flat(ck)[diff[0]] == 9      # only that word moves, and it holds the high half
        assert not np.array_equal(P.uniform4(**args), P.uniform4(7, 3, 5))
    assert [int(w) for w in base[0]] == [5, 0, 3, 0] and list(base[1]) == [7, 0]
    # idx as an array crossing 2^32
    idx = np.array([2**32 - 1, 2**32, 2**32 + 1], dtype=np.uint64)
    u = P.uniform4(1, 0, idx)
    assert np.array_equal(u[1], P.uniform4(1, 0, 2**32)) and not np.array_equal(u[1], P.uniform4(1, 0, 0))


def test_moments_of_a_draw():
    n = 1 << 20
    a, b = 2.0 * P.draw(1234, 0, n), 2.0 * P.draw(1234, 1, n)            # scale 2: the device test's bounds as they stand
    print(f"host draw(1234, 0, 2^20): mean {a.mean() / 2:.2e} std {a.std() / 2:.5f} fourth moment {((a / 2) ** 4).mean():.4f}")
    assert abs(a.mean()) < 0.01 and abs(a.std() - 2.0) < 0.01
    assert abs(((a / 2) ** 4).mean() - 3.0) < 0.05
    assert abs((a * b).mean()) < 0.02 and not np.array_equal(a, b)
    assert np.array_equal(P.draw(1234, 0, 64), a[:64] / 2)                # a prefix of the same stream


def test_domain_draw_is_the_flat_draw_reshaped():
    d = P.domain_draw(21, 2, 6, 12)
    z, _ = P.normal4(21, 2, 4 * 3 + 1)                                    # row 4, quad 1 of 3
    assert np.array_equal(d[4, 4:8], z)


def test_emulated_box_muller_against_pure_float64():
    """|emulated - float64| <= r * (angle error) + (radius error): the float32 angle product is off by at most 2^-24 of an angle below
    2 pi (half an ulp), the float32 constant 2pi_f32 by |2pi_f32 - 2 pi| = 1.75e-7 (times u <= 1), and rounding -2 ln u to float32
    moves the radius by at most 2^-25 of itself.  A comparison with the device that ignored the float32 angle would need this much
    slack, about 10 units of 2^-24 r, on top of the math functions' error; the emulated form needs none of it."""
    u = P.uniform4(99, 0, np.arange(1 << 18, dtype=np.uint64))
    z, r = P.box_muller(u)
    u64 = u.astype(np.float64)
    r64 = np.repeat(np.sqrt(-2.0 * np.log(u64[:, 0::2])), 2, axis=-1)
    a64 = np.repeat(2.0 * np.pi * u64[:, 1::2], 2, axis=-1)
    trig = np.stack([np.cos(a64[:, 0]), np.sin(a64[:, 1]), np.cos(a64[:, 2]), np.sin(a64[:, 3])], axis=-1)
    diff = np.abs(z - r64 * trig)
    angle_err = 2.0 * np.pi * 2.0**-24 + abs(float(P.TWO_PI_F32) - 2.0 * np.pi)
    bound = r * (angle_err + 2.0**-25) + 1e-12
    print(f"emulated vs float64 Box-Muller over 2^18 quads: max |diff| {diff.max():.2e}, max diff / bound {(diff / bound).max():.3f}")
    assert (diff <= bound).all()
    assert diff.max() > 1e-7                                              # the two do differ: the emulation is not a no-op
