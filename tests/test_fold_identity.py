"""The two identities behind the folded mirrored stage (yaman_stage_mirrored, FOLD), in float32 and
float64, against exact integer arithmetic:

  (1)  fma(x, y, RN(y*x)) == 2 * RN(x*y)      for EVERY finite x, y: signed zeros, subnormal and overflowing products included;
  (2)  RN((2e) * m) == RN(e * (2m))           whenever both doublings are exact, i.e. neither 2e nor 2m overflows -- the one
                                              edge the stage's comment names (a doubling that overflows is not a scaling).

A value is held as n * 2**q with Python integers, a product or a sum of such values is exact, and RN rounds it once to the
format (nearest, ties to even, gradual underflow, overflow to infinity).  NumPy's own multiplication is tied to that model
in every case, so the right-hand sides may be formed by NumPy in the format itself."""
import math

import numpy as np
import pytest

FORMATS = {np.float32: dict(p=24, qmin=-149, emax=127, bits=np.uint32), np.float64: dict(p=53, qmin=-1074, emax=1023, bits=np.uint64)}
N_RANDOM = 100_000


def exact(v):
    """finite float -> (n, q) with v == n * 2**q"""
    m, e = math.frexp(float(v))
    return int(m * (1 << 53)), e - 53


def mul(a, b):
    return a[0] * b[0], a[1] + b[1]


def add(a, b):
    q = min(a[1], b[1])
    return (a[0] << (a[1] - q)) + (b[0] << (b[1] - q)), q


def rn(v, negative_zero, p, qmin, emax, **_):
    """(n, q) rounded once to the format, as a Python float; an exact zero takes the sign the operation gives it"""
    n, q = v
    if n == 0:
        return -0.0 if negative_zero else 0.0
    sign, a = (-1.0 if n < 0 else 1.0), abs(n)
    ulp = max(q + a.bit_length() - p, qmin)        # exponent of the result's last place
    shift = ulp - q
    if shift <= 0:
        mant = a << -shift
    else:
        mant, rem, half = a >> shift, a & ((1 << shift) - 1), 1 << (shift - 1)
        if rem > half or (rem == half and (mant & 1)):
            mant += 1
    if mant.bit_length() + ulp > emax + 1:
        return sign * math.inf
    return sign * math.ldexp(mant, ulp)


def same_bits(a, b, dtype):
    t = FORMATS[dtype]["bits"]
    return np.array_equal(np.asarray(a, dtype=dtype).view(t), np.asarray(b, dtype=dtype).view(t))


def check_case(x, y, e, dtype):
    """both identities for one (x, y) and the phase factor component e -> which of them were checked"""
    fmt = FORMATS[dtype]
    x, y, e = dtype(x), dtype(y), dtype(e)
    neg = bool(np.signbit(x) ^ np.signbit(y))
    xy = mul(exact(x), exact(y))
    m = rn(xy, neg, **fmt)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        m_np, two_m, two_e = x * y, (x * y) + (x * y), e + e
        assert same_bits(m_np, m, dtype), (x, y)                      # NumPy's product is the model's
        # (1): the exact sum x*y + m, rounded once, is 2m
        fused = math.copysign(math.inf, m) if math.isinf(m) else rn(add(xy, exact(m)), neg, **fmt)
        assert same_bits(fused, two_m, dtype), ("fma(x, y, y*x) != 2*RN(x*y)", x, y, fused, two_m)
        # (2): needs exact doublings
        if not (np.isfinite(two_m) and np.isfinite(two_e)):
            return 1
        neg2 = bool(np.signbit(e)) ^ neg
        lhs = rn(mul(exact(two_e), exact(m)), neg2, **fmt)
        rhs = rn(mul(exact(e), exact(two_m)), neg2, **fmt)
        assert same_bits(lhs, rhs, dtype), ("RN(2e * m) != RN(e * 2m)", x, y, e)
        assert same_bits(two_e * m_np, lhs, dtype) and same_bits(e * two_m, rhs, dtype), (x, y, e)
    return 2


def random_finite(rng, n, dtype):
    """uniform over the bit patterns of the finite values: every exponent, subnormals and both signs alike"""
    t = FORMATS[dtype]["bits"]
    v = rng.integers(0, np.iinfo(t).max, size=2 * n + 64, dtype=t, endpoint=True).view(dtype)
    return v[np.isfinite(v)][:n]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_random_cases_over_the_whole_exponent_range(dtype):
    """half of the cases take y from the whole range too (most products overflow or underflow), half place the product's
    exponent uniformly over the format's range, subnormal results included"""
    fmt = FORMATS[dtype]
    rng = np.random.default_rng(20261018)
    x, e = random_finite(rng, N_RANDOM, dtype), random_finite(rng, N_RANDOM, dtype)
    y = random_finite(rng, N_RANDOM, dtype)
    half = N_RANDOM // 2
    ex = np.frexp(x[half:].astype(np.float64))[1]
    target = rng.integers(fmt["qmin"] - 2, fmt["emax"] + 3, size=N_RANDOM - half)       # exponent of the product
    with np.errstate(over="ignore", under="ignore"):
        y[half:] = np.ldexp(rng.uniform(0.5, 1.0, N_RANDOM - half) * rng.choice([-1.0, 1.0], N_RANDOM - half),
                            target - ex).astype(dtype)
    y = np.where(np.isfinite(y), y, dtype(1.5))
    both = sum(check_case(a, b, c, dtype) == 2 for a, b, c in zip(x, y, e))
    assert both > N_RANDOM // 2                                       # identity (2) was not skipped wholesale


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_hand_picked_cases(dtype):
    fmt = FORMATS[dtype]
    p, emax, qmin = fmt["p"], fmt["emax"], fmt["qmin"]
    eps, tiny, big = dtype(2.0) ** (1 - p), dtype(np.ldexp(1.0, qmin)), np.finfo(dtype).max
    one = dtype(1.0)
    cases = []
    # products one ulp either side of a power of two, and the ties between: (1 + a eps)(1 - b eps), x * y just off 2^k
    for a in (1, 2, 3):
        for b in (1, 2, 3):
            for k in (0, 7, -9, emax - 1, qmin + p + 3):
                s = dtype(np.ldexp(1.0, k // 2))
                cases += [((one + a * eps) * s, (one - b * eps / 2) * s), ((one + a * eps) * s, (one + b * eps) * s),
                          ((one - a * eps / 2) * s, (one - b * eps / 2) * s), ((dtype(2) - a * eps) * s, (one + b * eps) * s)]
    # subnormal products: exact, inexact, ties at half the subnormal quantum, the smallest normal from both sides
    for fx in (1.0, 1.5, 1.25, 1.75, 1.0 + float(eps), 2.0 - float(eps)):
        for k in (0, 1, 2, 3, p - 2, p - 1, p, p + 1):
            cases += [(dtype(fx), dtype(np.ldexp(1.0, qmin + k - 1))), (dtype(np.ldexp(fx, qmin // 2)), dtype(np.ldexp(1.5, qmin - qmin // 2 + k - 2)))]
    cases += [(tiny, dtype(0.5)), (tiny, dtype(0.75)), (tiny, dtype(0.25)), (tiny, tiny), (dtype(3) * tiny, dtype(0.5))]
    # signed zeros
    for zx in (dtype(0.0), dtype(-0.0)):
        for other in (dtype(0.0), dtype(-0.0), dtype(0.7), dtype(-0.7), big, tiny):
            cases += [(zx, other), (other, zx)]
    # a finite product that overflows when doubled, one that overflows itself, the largest that survives doubling
    cases += [(dtype(np.ldexp(1.5, emax // 2)), dtype(np.ldexp(1.25, emax - emax // 2))), (big, one), (big, dtype(0.75)),
              (big, dtype(2.0)), (big, big), (dtype(np.ldexp(1.0, emax // 2)), dtype(np.ldexp(1.0, emax - emax // 2 - 1))),
              (big, dtype(0.5)), (dtype(np.ldexp(1.0 - float(eps) / 2, emax // 2 + 1)), dtype(np.ldexp(1.0 - float(eps) / 2, emax - emax // 2)))]
    factors = (dtype(0.023), dtype(-0.0115), dtype(0.0), dtype(-0.0), tiny, dtype(3) * tiny, big, dtype(np.ldexp(1.0, emax)))
    checked = [0, 0, 0]
    with np.errstate(over="ignore", under="ignore"):
        for x, y in cases:
            for sx in (one, -one):
                for e in factors:
                    checked[check_case(sx * x, y, e, dtype)] += 1
    assert checked[1] > 0 and checked[2] > checked[1]                 # overflowing doublings are there, beside the rest
