"""The crosswise four-wave stage (yaman_stage with CROSS, yaman_stage_mirrored) restated in
Python, against the pairwise stage it replaces in the RK4 sweeps:

  (1)  both forms give the same dA/dz to rounding: they are the same three complex multiplications in another order;
  (2)  the crosswise expression list is symmetric: exchanging (A1 <-> A2, A3 <-> A4) permutes the eight outputs and changes
       no bit -- every pair of members is one expression with the partner's operands exchanged;
  (3)  on mirrored inputs (A2 == A1, A4 == A3 bit for bit) the eight outputs of the general stage are the four of the
       mirrored stage, pairwise, in every bit: signed zeros, subnormal products and overflowing products included.

(2) and (3) are statements about bits, so they are evaluated with an FMA that rounds once: math.fma where Python has it,
else exact rational arithmetic rounded once.  (1) is a statement about rounding noise and runs vectorised in NumPy."""
import math
from fractions import Fraction

import numpy as np

N_RANDOM = 10_000
EPS = float(np.finfo(np.float64).eps)


def _fma_exact(a, b, c):
    """a*b + c rounded once, for Python floats (IEEE binary64)"""
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c                          # an inf or NaN operand: no rounding is involved, the sum's rules decide
    r = Fraction(a) * Fraction(b) + Fraction(c)
    if r == 0:
        if a == 0.0 or b == 0.0:                  # an exactly zero product keeps its sign into the sum of two zeros
            return math.copysign(0.0, a) * math.copysign(1.0, b) + c
        return 0.0                                # exact cancellation of non-zero terms: +0 in round-to-nearest
    try:
        return float(r)                           # int / int true division: correctly rounded, gradual underflow
    except OverflowError:
        return math.inf if r > 0 else -math.inf


fma = getattr(math, "fma", _fma_exact)


def test_the_rational_fma_is_an_fma():
    """the fallback against hand-checked single roundings (and against math.fma where there is one)"""
    tiny = math.ldexp(1.0, -1074)
    cases = [(1.0 + EPS, 1.0 - EPS, -1.0, -EPS * EPS), (0.1, 10.0, -1.0, math.ldexp(1.0, -54)), (3.0, tiny, tiny, 4 * tiny),
             (0.5, tiny, 0.0, 0.0), (1.5, tiny, 0.0, 2 * tiny), (1e200, 1e200, -1e300, math.inf), (-1e200, 1e200, 1e300, -math.inf),
             (2.0, 3.0, -6.0, 0.0), (-0.0, 3.0, -0.0, -0.0), (-0.0, 3.0, 0.0, 0.0), (0.0, -3.0, -0.0, -0.0)]
    for a, b, c, want in cases:
        got = _fma_exact(a, b, c)
        assert got == want and math.copysign(1.0, got) == math.copysign(1.0, want), (a, b, c, got, want)
    if hasattr(math, "fma"):
        rng = np.random.default_rng(3)
        for a, b, c in rng.standard_normal((2000, 3)) * 10.0 ** rng.integers(-160, 160, (2000, 3)):
            a, b, c = float(a), float(b), float(c)
            try:
                want = math.fma(a, b, c)
            except OverflowError:
                continue
            assert _fma_exact(a, b, c) == want, (a, b, c)


# ---- the stages, operation for operation as in csrc/psa_rk4_kernel.inc.h (FUSED, LOSS) -------------------------------------
def _link(gsig, v, ha, a_c, base_c):
    return fma(gsig, v, fma(ha, a_c, base_c))


def stage_crosswise(a, base, Er, Ei, g, tg, ha):
    x1, y1, x2, y2, x3, y3, x4, y4 = a
    p = [fma(a[2 * j], a[2 * j], a[2 * j + 1] * a[2 * j + 1]) for j in range(4)]
    gs = tg * ((p[0] + p[1]) + (p[2] + p[3]))
    gj = [fma(-g, pj, gs) for pj in p]
    b23r, b23i = fma(x2, x3, y2 * y3), fma(x2, y3, -(y2 * x3))
    b14r, b14i = fma(x1, x4, y1 * y4), fma(x1, y4, -(y1 * x4))
    h23r, h23i = fma(Er, b23r, -(Ei * b23i)), fma(Er, b23i, Ei * b23r)
    h14r, h14i = fma(Er, b14r, -(Ei * b14i)), fma(Er, b14i, Ei * b14r)
    lk = lambda gsig, v, c: _link(gsig, v, ha, a[c], base[c])   # noqa: E731
    return [fma(-y4, h23r, fma(-x4, h23i, lk(-gj[0], y1, 0))), fma(x4, h23r, fma(-y4, h23i, lk(gj[0], x1, 1))),
            fma(-y3, h14r, fma(-x3, h14i, lk(-gj[1], y2, 2))), fma(x3, h14r, fma(-y3, h14i, lk(gj[1], x2, 3))),
            fma(-y2, h14r, fma(x2, h14i, lk(-gj[2], y3, 4))), fma(x2, h14r, fma(y2, h14i, lk(gj[2], x3, 5))),
            fma(-y1, h23r, fma(x1, h23i, lk(-gj[3], y4, 6))), fma(x1, h23r, fma(y1, h23i, lk(gj[3], x4, 7)))]


def stage_mirrored(a, base, Er, Ei, g, sg, ha):
    x1, y1, xs, ys = a
    p0, p2 = fma(x1, x1, y1 * y1), fma(xs, xs, ys * ys)
    gs = sg * (p0 + p2)
    g1, g3 = fma(-g, p0, gs), fma(-g, p2, gs)
    br, bi = fma(x1, xs, y1 * ys), fma(x1, ys, -(y1 * xs))
    hr, hi = fma(Er, br, -(Ei * bi)), fma(Er, bi, Ei * br)
    lk = lambda gsig, v, c: _link(gsig, v, ha, a[c], base[c])   # noqa: E731
    return [fma(-ys, hr, fma(-xs, hi, lk(-g1, y1, 0))), fma(xs, hr, fma(-ys, hi, lk(g1, x1, 1))),
            fma(-y1, hr, fma(x1, hi, lk(-g3, ys, 2))), fma(x1, hr, fma(y1, hi, lk(g3, xs, 3)))]


def same_bits(a, b):
    """bit patterns equal; two NaNs match (a payload is not part of the claim)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and bool(np.all(nan | (a.view(np.uint64) == b.view(np.uint64))))


def _random_inputs(rng, n):
    """amplitudes of the sweeps' kind (pumps ~1, sidebands 1e-4..1e-1, any phase), stage constants of the headline step"""
    amp = np.column_stack([rng.uniform(0.3, 1.0, (n, 2)), 10.0 ** rng.uniform(-4, -1, (n, 2))])
    A = amp * np.exp(1j * rng.uniform(-np.pi, np.pi, (n, 4)))
    B = A * (1.0 + 1e-3 * rng.standard_normal((n, 4)))          # the chain's base: a state nearby
    g = rng.uniform(5e-3, 2e-2, n) * 0.05                       # d * gamma
    ha = -0.5 * rng.uniform(0.0, 3e-4, n) * 0.05                # -d * alpha / 2
    ph = rng.uniform(-np.pi, np.pi, n)
    return A, B, 2 * g * np.cos(ph), 2 * g * np.sin(ph), g, 2 * g, ha


# ---- (1) the two forms agree to rounding ------------------------------------------------------------------------------------
def test_crosswise_and_pairwise_forms_agree_to_rounding():
    """dA/dz (un-fused) of both forms in complex NumPy arithmetic on 10 000 random sets.  Each output is a sum of three terms,
    (ha + i g_j) A_j (two) and the triple product; a form evaluates the triple product with three complex multiplications
    (relative error below 3 * sqrt(8) u, u = eps / 2) and adds three terms (two more roundings on a sum bounded by the sum
    of the moduli).  With L the sum of the three terms' moduli, each form is within (3 * sqrt(8) + 2) u L < 11 u L of the
    exact value and the two within 22 u L = 11 eps L of each other; the orders of operation differ between NumPy and the
    kernel's FMA chains, not the bound's kind.  Asserted: 11 eps L, component-wise on the modulus."""
    rng = np.random.default_rng(20261018)
    A, _, Er, Ei, g, tg, ha = _random_inputs(rng, N_RANDOM)
    E = Er + 1j * Ei
    A1, A2, A3, A4 = A.T
    P = np.abs(A) ** 2
    gj = (tg * P.sum(axis=1))[:, None] - g[:, None] * P
    lin = (ha[:, None] + 1j * gj) * A
    q12, q34 = A1 * A2, A3 * A4
    Fp, Fs = E * q34, np.conj(E) * q12
    pair = lin + 1j * np.column_stack([np.conj(A2) * Fp, np.conj(A1) * Fp, np.conj(A4) * Fs, np.conj(A3) * Fs])
    H23, H14 = E * (np.conj(A2) * A3), E * (np.conj(A1) * A4)
    cross = lin + 1j * np.column_stack([H23 * A4, H14 * A3, np.conj(H14) * A2, np.conj(H23) * A1])
    partners = np.abs(np.column_stack([A2 * A3 * A4, A1 * A3 * A4, A4 * A1 * A2, A3 * A1 * A2]))
    L = (np.abs(ha)[:, None] + np.abs(gj)) * np.abs(A) + np.abs(E)[:, None] * partners
    ratio = np.abs(cross - pair) / (EPS * L)
    print(f"largest |cross - pair| = {ratio.max():.2f} eps * L")
    assert ratio.max() < 11.0
    # and the Python restatement of the kernel's FMA chains is the same function (same bound against the NumPy value)
    for k in range(0, N_RANDOM, 100):
        a = A[k].view(np.float64).tolist()
        out = stage_crosswise(a, [0.0] * 8, float(Er[k]), float(Ei[k]), float(g[k]), float(tg[k]), float(ha[k]))
        got = np.array(out).view(np.complex128)
        assert np.all(np.abs(got - cross[k]) < 11.0 * EPS * L[k]), k


# ---- (2) exchange symmetry, in bits -----------------------------------------------------------------------------------------
EXCHANGE = [2, 3, 0, 1, 6, 7, 4, 5]          # components after A1 <-> A2, A3 <-> A4


def _hand_picked():
    """amplitude components that make signed zeros, subnormal products and overflowing products inside the stage"""
    tiny, sub, big = math.ldexp(1.0, -1074), math.ldexp(1.5, -540), 1.2e154
    return [[0.0, 0.7, -0.0, 0.7, 1e-3, 0.0, 1e-3, -0.0], [-0.0, -0.0, 0.0, 0.0, 0.3, -0.2, 0.1, 0.4], [0.7, 0.0, 0.7, -0.0, 0.0, 0.0, -0.0, -0.0],
            [sub, -sub, 0.5 * sub, sub, sub, sub, -sub, 3 * sub],            # every pair product is subnormal or underflows
            [1.0, -1.0, 0.5, 0.25, tiny, -tiny, 3 * tiny, tiny], [1e-160, 1e-160, -1e-161, 2e-160, 1e-150, -1e-152, 1e-151, 1e-150],
            [big, 0.5 * big, -big, big, big, -big, 0.9 * big, big],          # x*x + y*y and the pair products overflow
            [1e200, 1.0, 1.0, 1e200, 1e120, -1e120, 1e-5, 1e120], [1e154, 1e154, 1e154, -1e154, 1e-3, 1e-3, 1e-3, 1e-3]]


def _cases(rng, n, mirrored):
    A, B, Er, Ei, g, tg, ha = _random_inputs(rng, n)
    if mirrored:
        A[:, 1], A[:, 3], B[:, 1], B[:, 3] = A[:, 0], A[:, 2], B[:, 0], B[:, 2]
    out = [(A[k].view(np.float64).tolist(), B[k].view(np.float64).tolist(), float(Er[k]), float(Ei[k]), float(g[k]), float(tg[k]),
            float(ha[k])) for k in range(n)]
    for a in _hand_picked():
        if mirrored:
            a = a[0:2] + a[0:2] + a[4:6] + a[4:6]
        for er, ei in ((1.1e-3, -0.4e-3), (0.0, -0.0), (-0.0, 1e-3)):
            out.append((a, [0.5 * v for v in a], er, ei, 5.75e-4, 1.15e-3, -2.9e-6))
            out.append((a, a, er, ei, 5.75e-4, 1.15e-3, 0.0))
    return out


N_BITS = 10_000 if hasattr(math, "fma") else 1_000     # the rational FMA is a hundred times slower


def test_exchanging_the_partners_permutes_the_outputs_bit_for_bit():
    rng = np.random.default_rng(7)
    for a, base, Er, Ei, g, tg, ha in _cases(rng, N_BITS, mirrored=False):
        with np.errstate(all="ignore"):
            out = stage_crosswise(a, base, Er, Ei, g, tg, ha)
            swapped = stage_crosswise([a[c] for c in EXCHANGE], [base[c] for c in EXCHANGE], Er, Ei, g, tg, ha)
        assert same_bits([out[c] for c in EXCHANGE], swapped), a


# ---- (3) the mirrored stage is the general stage with the duplicates removed -------------------------------------------------
def test_mirrored_inputs_give_the_mirrored_stage_pairwise_in_every_bit():
    """The one liberty of the mirrored stage is gs = (2 tg) * (p0 + p2) for tg * ((p0 + p0) + (p2 + p2)): the same number
    unless 2 * (p0 + p2) overflows while p0 + p2 does not, where both stages end non-finite in the same components.  The
    overflowing cases here overflow p0 + p2 itself (or x*x + y*y), so even their inf / NaN patterns must agree."""
    rng = np.random.default_rng(11)
    n_special = 0
    for a, base, Er, Ei, g, tg, ha in _cases(rng, N_BITS, mirrored=True):
        assert a[0:2] == a[2:4] and a[4:6] == a[6:8]
        with np.errstate(all="ignore"):
            full = stage_crosswise(a, base, Er, Ei, g, tg, ha)
            half = stage_mirrored(a[0:2] + a[4:6], base[0:2] + base[4:6], Er, Ei, g, tg + tg, ha)
        assert same_bits(full[0:2], half[0:2]) and same_bits(full[2:4], half[0:2]), a
        assert same_bits(full[4:6], half[2:4]) and same_bits(full[6:8], half[2:4]), a
        n_special += not all(math.isfinite(v) and v != 0.0 for v in full)
    assert n_special >= 6                       # zeros and non-finite results were among the cases
