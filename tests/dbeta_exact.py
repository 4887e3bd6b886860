"""An exact yardstick for the phase mismatch, the forward bound of the kernel's operation list, a float64 restatement of
that list in which defects can be planted, and the input sets that tests/test_dbeta_exact_host.py and
tests/test_gpu_dbeta_exact.py share.  Standard library and NumPy only; nothing is taken from the package but the equations.

Every float64 is a rational number and the formulas are polynomials, so ``fractions.Fraction`` evaluates them without any
rounding.  The one division by an input, omega = 2*pi*c / lambda, is rational too: ``two_pi_c`` is the float64 the model carries.

Two references:

* ``staged_*``: the exact value of the formula AT the float64 plan values the host forms (omega_d, Omega for the symmetric
  closed form; w1..w4 and omega_ref for the Taylor sum).  Against it only the evaluation's own roundings are left.
* ``from_wavelengths``: the exact mismatch of the three float64 wavelengths, omega_4 and Omega formed with nothing rounded
  in between.  Against it the plan stage's roundings show as well (Omega = w3 - omega_c is a difference of two numbers of
  1.2e15: up to ~1e-12 relative, the reference scheme's own conditioning).

The forward bound (first order in u = 2^-53; the tests allow 2 B for the second-order terms).

Symmetric closed form with k orders, term n: t_n = ((beta_n * (Omega^n - omega_d^n)) * 2) / n!,
m_n = |beta_n| (|Omega|^n + |omega_d|^n) 2 / n!  (>= |t_n|):
    Omega^n, omega_d^n    each rounded once (x*x, or a double-double product rounded once):  u (|Omega|^n + |omega_d|^n)
                          on the difference                                                  -> 1 u m_n
    the difference        one rounding, u |Omega^n - omega_d^n|                              -> 1 u m_n
    beta_n * (...)        one rounding                                                       -> 1 u m_n
    * 2                   exact
    / n!                  one rounding (n! <= 40320 is exact)                                -> 1 u m_n
    acc + t_n             the first addition is 0 + t, exact; k - 1 more, each u |partial sum| <= u sum_n m_n
                                                                                             -> (k - 1) u sum_n m_n
    B = (k + 3) u sum_n m_n.     (An order with beta_n = 0 is skipped by every statement and leaves the bound slack.)

Taylor sum of order P at w_j, dw_j = w_j - omega_ref, term n: (beta_n * dw^n) / n!,  M_j = sum_n |beta_n| |dw_j|^n / n!:
    dw = w - omega_ref    one rounding, relative u on dw, hence n u on dw^n                  -> n u |term|   (<= P u)
    dw^n                  rounded once                                                       -> 1 u |term|
    beta_n * dw^n         one rounding                                                       -> 1 u |term|
    / n!                  one rounding                                                       -> 1 u |term|
    acc + term            the first is exact; up to P more, each u |partial sum| <= u M_j    -> P u M_j
    so beta(w_j) carries (2P + 3) u M_j; then the four-wave combination (b3 + b4) - (b1 + b2):
    b3 + b4, b1 + b2, and the final difference: three roundings, each <= u sum_j M_j         -> 3 u sum_j M_j
    B = (2P + 6) u sum_j M_j.

``scale`` is sum_n m_n (symmetric) or sum_j M_j (Taylor): the unit of the per-point figure e = |got - staged| / scale.
"""
from fractions import Fraction
from math import factorial

import numpy as np

U = Fraction(1, 2 ** 53)
C_LIGHT = 299792458.0
TWO_PI_C = 2.0 * np.pi * C_LIGHT          # the float64 the model carries, (2*pi)*c
MAX_ORDER = 8

# The aggregate bar of the GPU test: median(e_device) <= FACTOR_MEDIAN * median(e_host_scalar) and max(e_device) <= FACTOR_MAX *
# max(e_host_scalar) over a set.  The factors are three times the spread between the package's two HOST statements (the scalar
# reference-faithful path and the array path), rounded up to the next integer -- as DESIGN section 4 set its 4 and 8 from a
# measured 1.3 and 2.4.  Measured on the CPU over every valid-only input set below (tests/test_dbeta_exact_host.py prints and
# re-checks it): medians within SPREAD_MEDIAN of each other, maxima within SPREAD_MAX.
SPREAD_MEDIAN = 1.02       # measured 1.0129 on "taylor 6 beta2,3,4,6 alone" (1.0040 on sym (8,)): NumPy's array pow against libm's
SPREAD_MAX = 1.09          # measured 1.0870 on sym (8,).  On the other sets the two host statements are the same bits: 1.0000
FACTOR_MEDIAN = 4.0        # 3 * 1.02 = 3.06
FACTOR_MAX = 4.0           # 3 * 1.09 = 3.27


def _fr(x) -> Fraction:
    return Fraction(float(x))


# ---- the exact formulas ------------------------------------------------------------------------------------------------------
def _sym_exact(beta, orders, od: Fraction, Om: Fraction):
    """-> (sum_n beta_n (Om^n - od^n) 2/n!,  sum_n |beta_n| (|Om|^n + |od|^n) 2/n!), exact."""
    total, scale = Fraction(0), Fraction(0)
    for n in orders:
        bn = _fr(beta[n])
        if bn != 0:
            total += bn * (Om ** n - od ** n) * 2 / factorial(n)
            scale += abs(bn) * (abs(Om) ** n + abs(od) ** n) * 2 / factorial(n)
    return total, scale


def _taylor_exact(beta, max_order, dw: Fraction):
    """-> (sum_{n <= P} beta_n dw^n / n!, sum_n |beta_n| |dw|^n / n!), exact."""
    total, scale, p = Fraction(0), Fraction(0), Fraction(1)
    for n in range(max_order + 1):
        bn = _fr(beta[n])
        if bn != 0:
            total += bn * p / factorial(n)
            scale += abs(bn * p) / factorial(n)
        p *= dw
    return total, scale


def staged_symmetric(beta, orders, od, Om):
    """The exact closed form at the float64 (omega_d, Omega).  -> (value, scale, B) as Fractions."""
    value, scale = _sym_exact(beta, orders, _fr(od), _fr(Om))
    return value, scale, (len(orders) + 3) * U * scale


def staged_taylor(beta, max_order, omega_ref, w):
    """The exact (beta(w3) + beta(w4)) - (beta(w1) + beta(w2)) at the float64 w = (w1, w2, w3, w4) and omega_ref.
    -> (value, scale, B) as Fractions."""
    b, scale = [], Fraction(0)
    for wj in w:
        v, s = _taylor_exact(beta, max_order, _fr(wj) - _fr(omega_ref))
        b.append(v)
        scale += s
    return (b[2] + b[3]) - (b[0] + b[1]), scale, (2 * max_order + 6) * U * scale


def staged(case, plan):
    """``plan``: what the host formed in float64 -- dict(w=(w1, w2, w3, w4), od=, Om=).  -> (value, scale, B)."""
    if case["method"] == "symmetric":
        return staged_symmetric(case["beta"], case["orders"], plan["od"], plan["Om"])
    return staged_taylor(case["beta"], case["max_order"], case["omega_ref"], plan["w"])


def from_wavelengths(case, l1, l2, l3) -> Fraction:
    """The exact mismatch of three float64 wavelengths: w_j = two_pi_c / lambda_j, w4 = w1 + w2 - w3, omega_c = (w1 + w2) / 2,
    omega_d = (w1 - w2) / 2, Omega = w3 - omega_c, all as rationals."""
    k = _fr(TWO_PI_C)
    w1, w2, w3 = k / _fr(l1), k / _fr(l2), k / _fr(l3)
    w4 = w1 + w2 - w3
    if case["method"] == "symmetric":
        return _sym_exact(case["beta"], case["orders"], (w1 - w2) / 2, w3 - (w1 + w2) / 2)[0]
    ref = _fr(case["omega_ref"])
    b = [_taylor_exact(case["beta"], case["max_order"], w - ref)[0] for w in (w1, w2, w3, w4)]
    return (b[2] + b[3]) - (b[0] + b[1])


# ---- the kernel's operation list in float64, restated (Python floats are IEEE doubles, one rounding per operation) -----------
def pow_once(x: float, n: int) -> float:
    """x**n rounded once: what the kernel's double-double product delivers (its error before the last rounding is ~2^-100)."""
    return float(Fraction(x) ** n)


def twin_symmetric(beta, orders, od: float, Om: float) -> float:
    acc = 0.0
    for n in orders:
        bn = float(beta[n])
        if bn != 0.0:
            acc = acc + bn * (pow_once(Om, n) - pow_once(od, n)) * 2.0 / float(factorial(n))
    return acc


def twin_taylor(beta, max_order, omega_ref: float, w: float) -> float:
    dw = w - omega_ref
    acc = 0.0
    for n in range(max_order + 1):
        bn = float(beta[n])
        if bn != 0.0:
            acc = acc + bn * pow_once(dw, n) / float(factorial(n))
    return acc


def split_exact(i: int, n3: int):
    """Row and column of flat index i with Python integers."""
    return i // n3, i % n3


def split_int32(i: int, n3: int):
    """PLANTED DEFECT: the flat index held in 32 bits (what `int i = first + t` would do)."""
    i32 = (int(i) + 2 ** 31) % 2 ** 32 - 2 ** 31
    q = abs(i32) // n3 * (1 if i32 >= 0 else -1)      # C's division truncates towards zero
    return q, i32 - q * n3


def _isclose(lhs, rhs, atol, rtol):
    return abs(lhs - rhs) <= (atol + rtol * abs(rhs))


def twin_point(case, l1: float, l2: float, l3: float, *, omega_from_idler: bool = False):
    """One point of dbeta_grid_kernel, rule by rule.  -> (dbeta or NaN, valid).  ``omega_from_idler``: PLANTED DEFECT, Omega
    taken as omega_c - w4 instead of w3 - omega_c."""
    fin = np.isfinite
    nan = float("nan")
    with np.errstate(all="ignore"):
        l1, l2, l3 = np.float64(l1), np.float64(l2), np.float64(l3)
        ok = bool(fin(l1) and fin(l2) and fin(l3) and l1 > 0.0 and l2 > 0.0 and l3 > 0.0)
        k = np.float64(TWO_PI_C)
        w1, w2, w3 = k / l1, k / l2, k / l3
        w4 = w1 + w2 - w3
        ok = ok and bool(fin(w4) and w4 > 0.0)
        ok = ok and bool(_isclose(w1 + w2, w3 + w4, 0.0, 1e-12))
        ok = ok and bool(fin(w1) and fin(w2) and fin(w3) and w1 > 0.0 and w2 > 0.0 and w3 > 0.0)
        ok = ok and bool(_isclose(w1 + w2, w3 + w4, case["atol"], case["rtol"]))
        if not ok:                       # everything below is arithmetic on values that no longer matter
            return nan, False
        w1, w2, w3, w4 = float(w1), float(w2), float(w3), float(w4)
        if case["method"] == "taylor":
            b = [twin_taylor(case["beta"], case["max_order"], case["omega_ref"], w) for w in (w1, w2, w3, w4)]
            db = (b[2] + b[3]) - (b[0] + b[1])
        else:
            oc, od = 0.5 * (w1 + w2), 0.5 * (w1 - w2)
            Om = oc - w4 if omega_from_idler else w3 - oc
            ok = bool(fin(oc) and fin(od) and fin(Om) and oc > 0.0 and abs(od) < oc)
            r1, r2, r3, r4 = oc + od, oc - od, oc + Om, oc - Om
            ok = ok and r1 > 0.0 and r2 > 0.0 and r3 > 0.0 and r4 > 0.0
            ok = ok and bool(_isclose(r1 + r2, r3 + r4, 0.0, 1e-12))
            ok = ok and bool(_isclose(r4, w4, case["atol"], case["rtol"]))
            if not ok:
                return nan, False
            db = twin_symmetric(case["beta"], case["orders"], od, Om)
    return (db, True) if np.isfinite(db) else (nan, False)


def twin_grid(case, l1, ax2, ax3, first: int = 0, n_points=None, *, split=split_exact, omega_from_idler: bool = False):
    """Points [first, first + n_points) of the flattened ax2 x ax3 grid.  -> (dbeta[n], valid[n])."""
    n3 = len(ax3)
    n = len(ax2) * n3 - first if n_points is None else n_points
    out, valid = np.empty(n), np.empty(n, dtype=bool)
    for t in range(n):
        r, c = split(first + t, n3)
        out[t], valid[t] = twin_point(case, l1, ax2[r], ax3[c], omega_from_idler=omega_from_idler)
    return out, valid


# ---- the input sets ----------------------------------------------------------------------------------------------------------
LAMBDA1 = 1550e-9
N2, N3 = 7, 43                       # 301 points: a block of 256 and a ragged one; n3 odd, so rows change inside a wave
OMEGA_REF = TWO_PI_C / 1552e-9
# beta_0 .. beta_8 (s^n / m): the even coefficients of tools/dbeta_fuzz.py with a beta_8, beta_0 = n omega / c and beta_1 = 1 / v_g of
# silica at 1550 nm, and odd coefficients of the size a dispersion slope gives
BETA = (5.8e6, 4.9e-9, -2.3e-28, 4.1e-41, -3.0e-55, 2.0e-69, 1.0e-84, -3.0e-98, 5.0e-114)
BETA_EVEN = tuple(b if n % 2 == 0 and n >= 2 else 0.0 for n, b in enumerate(BETA))


def _case(name, method, *, orders=(), max_order=0, beta=BETA, omega_ref=OMEGA_REF, atol=0.0, rtol=1e-12, grid="band"):
    return dict(name=name, method=method, orders=tuple(orders), max_order=max_order, beta=tuple(beta), omega_ref=omega_ref,
                atol=atol, rtol=rtol, grid=grid)


def _zeroed(beta, *orders):
    return tuple(0.0 if n in orders else b for n, b in enumerate(beta))


# the sets on which every plan is valid
CASES = (
    _case("sym (2,)", "symmetric", orders=(2,)),
    _case("sym (2,4)", "symmetric", orders=(2, 4)),
    _case("sym (2,4,6)", "symmetric", orders=(2, 4, 6)),
    _case("sym (2,4,6,8)", "symmetric", orders=(2, 4, 6, 8)),
    _case("sym (8,)", "symmetric", orders=(8,)),
    _case("taylor 2", "taylor", max_order=2),
    _case("taylor 4", "taylor", max_order=4),
    _case("taylor 6", "taylor", max_order=6),
    _case("taylor 8", "taylor", max_order=8),
    _case("sym (2,4,6) beta4=0", "symmetric", orders=(2, 4, 6), beta=_zeroed(BETA, 4)),
    _case("taylor 6 beta3=beta4=0", "taylor", max_order=6, beta=_zeroed(BETA, 3, 4)),
    _case("taylor 6 ref +10%", "taylor", max_order=6, omega_ref=1.1 * OMEGA_REF),
    _case("taylor 6 beta2,3,4,6 alone", "taylor", max_order=6, beta=_zeroed(BETA, 0, 1, 5, 7, 8)),     # tools/dbeta_fuzz.py's model
    # default tolerances on the grid of tolerance_axes: signal wavelengths out to 22 um and more, where w4 and Omega are ROUNDED
    _case("sym (2,4) long lambda3", "symmetric", orders=(2, 4), grid="tolerance"),
    _case("sym (8,) long lambda3", "symmetric", orders=(8,), grid="tolerance"),
    _case("taylor 4 long lambda3", "taylor", max_order=4, grid="tolerance"),
)
# the sets whose tolerances decide, on a grid of their own (tolerance_axes).  At rtol = atol = 0 conservation holds only where
# the float64 sums w1 + w2 and w3 + w4 are the same number, and the symmetric form's r4 must be w4 bit for bit.  With
# atol = 0.125, rtol = 1.63e-16 the threshold 0.125 + 1.63e-16 |w4| crosses 0.5 -- one ulp of w4 from 2^51 up, i.e. for lambda_3
# beyond 10.5 um -- at w4 = 2.30e15, lambda_3 = 14 um: r4 one ulp off w4 is refused between 10.5 and 14 um and admitted on
# either side (below 10.5 um one ulp is 0.25).  Both numbers decide.
CASES_TOLERANCE = (
    _case("sym (2,4) rtol=0", "symmetric", orders=(2, 4), atol=0.0, rtol=0.0, grid="tolerance"),
    _case("taylor 4 rtol=0", "taylor", max_order=4, atol=0.0, rtol=0.0, grid="tolerance"),
    _case("sym (2,4) atol=0.125 rtol=1.63e-16", "symmetric", orders=(2, 4), atol=0.125, rtol=1.63e-16, grid="tolerance"),
    _case("taylor 4 atol=0.125 rtol=1.63e-16", "taylor", max_order=4, atol=0.125, rtol=1.63e-16, grid="tolerance"),
)
ORDERS_LE_2 = ("sym (2,)", "taylor 2")     # only squares enter: every statement is the same bits


def axes():
    """(lambda_p2[N2], lambda_3[N3]) in the band of tools/dbeta_fuzz.py, fixed seed."""
    rng = np.random.default_rng(20240531)
    return np.sort(rng.uniform(1545e-9, 1570e-9, N2)), np.sort(rng.uniform(1500e-9, 1620e-9, N3))


def conservation_breakers(pumps, count: int, seed: int = 20240605):
    """-> (l2, lambda_3[count]): the first l2 of ``pumps`` that has them, and signal wavelengths at which
    fl(w3 + fl(fl(w1 + w2) - w3)) is not fl(w1 + w2) for the pumps (LAMBDA1, l2).  The sum can miss only through a tie that
    rounds away: w4 at or above 2^51 (ulp 0.5), w3 an odd multiple of 0.25 -- lambda_3 beyond about 10.5 um, one candidate in
    sixteen -- and the last bit of fl(w1 + w2) odd, which half the pumps have."""
    rng = np.random.default_rng(seed)
    cand = rng.uniform(11e-6, 40e-6, 4000)
    w3 = TWO_PI_C / cand
    for l2 in pumps:
        s12 = TWO_PI_C / LAMBDA1 + TWO_PI_C / float(l2)
        hits = cand[(w3 + (s12 - w3)) != s12]
        if hits.size >= count:
            return float(l2), hits[:count]
    raise AssertionError("no pump among the candidates has an odd sum")


def tolerance_axes():
    """The grid of CASES_TOLERANCE.  While lambda_3 stays within about four times the pumps' wavelength every difference of the
    plan stage is exact (w4 and Omega have no more bits than their operands) and no tolerance can decide; beyond 6.4 um w3 has two
    bits below the ulp of w4 and Omega, and r4 = omega_c - Omega and w4 = (w1 + w2) - w3 round apart at about one point in five.
    So 13 signal wavelengths lie in the band, 27 between 6.5 and 22 um, and 3 are conservation_breakers of one of the pumps."""
    rng = np.random.default_rng(20240604)
    l2 = np.sort(rng.uniform(1545e-9, 1570e-9, N2))
    l3 = np.concatenate([rng.uniform(1500e-9, 1620e-9, 13), rng.uniform(6.5e-6, 22e-6, N3 - 16), conservation_breakers(l2, 3)[1]])
    return l2, np.sort(l3)


def axes_of(case):
    return tolerance_axes() if case["grid"] == "tolerance" else axes()


def grid_points(ax2, ax3):
    """The flattened grid's (l2, l3), row-major."""
    return [(float(a), float(b)) for a in ax2 for b in ax3]


# the six-wave pair grid: two Omega axes with negative entries and Omega = 0
PAIR_OMEGA_D = 0.5 * (TWO_PI_C / 1550e-9 - TWO_PI_C / 1558e-9)
PAIR_ORDER_SETS = ((2, 4), (2, 4, 6, 8))


def pair_axes():
    rng = np.random.default_rng(20240601)
    o1 = rng.uniform(-3e13, 3e13, N2)
    o2 = rng.uniform(-3e13, 3e13, N3)
    o1[3] = 0.0
    o2[[0, 20]] = 0.0
    o2[41] = -o2[40]
    return o1, o2


def wide_axes(n: int = 64):
    """An n x n cut of the wide grid of tools/dbeta_fuzz.py: wavelengths far outside the band and the special values."""
    rng = np.random.default_rng(2)
    l2 = np.concatenate([np.sort(rng.uniform(0.4e-6, 4e-6, n - 4)), [0.0, -1e-6, np.nan, np.inf]])
    l3 = np.concatenate([np.sort(rng.uniform(0.3e-6, 6e-6, n - 3)), [0.0, -2e-6, np.nan]])
    return l2, l3


# ---- the validity rules, one point each ---------------------------------------------------------------------------------------
CASE_SYM = CASES[1]
CASE_TAYLOR = CASES[6]
CASE_SYM_RTOL0 = CASES_TOLERANCE[0]
CASE_TAYLOR_RTOL0 = CASES_TOLERANCE[1]
CASE_SYM_OVERFLOW = _case("sym (2,4) beta2=1e300", "symmetric", orders=(2, 4), beta=(0.0, 0.0, 1e300) + BETA[3:])
CASE_TAYLOR_OVERFLOW = _case("taylor 4 beta2=1e300", "taylor", max_order=4, beta=BETA[:2] + (1e300,) + BETA[3:])


def r4_breaker(l2: float, seed: int = 20240606) -> float:
    """A signal wavelength at which w1 + w2 == w3 + w4 holds in float64 and omega_c - Omega is not w4: the r4-against-w4 rule
    alone at rtol = atol = 0."""
    rng = np.random.default_rng(seed)
    k = TWO_PI_C
    w1, w2 = k / LAMBDA1, k / l2
    for l3 in rng.uniform(7e-6, 40e-6, 1000):
        w3 = k / l3
        s12 = w1 + w2
        w4 = s12 - w3
        oc = 0.5 * s12
        if w3 + w4 == s12 and oc - (w3 - oc) != w4:
            return float(l3)
    raise AssertionError("no such wavelength among the candidates")


def rule_points():
    """[(label, case, l1, l2, l3, what the scalar path's message must contain, the case under which the same point is valid
    or None)]: every rule of dbeta_grid_kernel that finite or non-finite inputs can trip, tripped alone.

    Rules that NO input trips alone, with the reason:
      * conserves(w1 + w2, w3 + w4, 0, 1e-12), the plan's own check: w4 = fl(fl(w1 + w2) - w3) puts w3 + w4 within two ulp of
        w1 + w2 whenever w4 is finite, 2e-16 relative.
      * w1, w2, w3 finite and positive: 2 pi c / lambda is positive for a finite positive lambda, cannot underflow to zero
        (lambda <= 1.8e308 leaves 1e-299), and where it overflows (lambda < 1.1e-299) w4 is non-finite as well: the omega_4
        rule trips first.
      * omega_c, omega_d, Omega finite and omega_c > 0: sums and differences of finite positive numbers of 1e15.
      * r1, r2, r4 > 0: r1 = fl(omega_c + omega_d) and r2 are w1 and w2 to within an ulp; r4 = omega_c - Omega is w4 to within an
        ulp of omega_c, and where w4 is that small every difference is exact and r4 IS w4.
      * conserves(r1 + r2, r3 + r4, 0, 1e-12): both sums are 2 omega_c to within two ulp.
    Two rules the wavelengths of a laboratory cannot trip and absurd finite ones can (both are in the list):
      * |omega_d| < omega_c: lambda_p2 = 1e12 m makes w2 vanish beside w1, and fl(w1 - w2) = fl(w1 + w2).
      * r3 > 0: lambda_3 = 1e12 m makes Omega = fl(w3 - omega_c) = -omega_c, r3 = 0."""
    ax2, ax3 = axes()
    l2, l3 = float(ax2[2]), float(ax3[7])
    out = []
    for bad, what in ((float("nan"), "not finite"), (float("inf"), "not finite"), (0.0, "needs a positive"), (-1.5e-6, "needs a positive")):
        for case in (CASE_SYM, CASE_TAYLOR):
            out.append((f"lambda1 = {bad}", case, bad, l2, l3, "lambda1_m: " + what, None))
            out.append((f"lambda2 = {bad}", case, LAMBDA1, bad, l3, "lambda2_m: " + what, None))
            out.append((f"lambda3 = {bad}", case, LAMBDA1, l2, bad, "lambda3_m: " + what, None))
    for case in (CASE_SYM, CASE_TAYLOR):
        out.append(("omega4 <= 0", case, LAMBDA1, l2, 0.7e-6, "omega4(inferred): needs a positive", None))
        out.append(("omega4 non-finite", case, LAMBDA1, l2, 1e-300, "omega4(inferred): not finite", None))
    l2c, l3c = conservation_breakers(ax2, 1)
    out.append(("conservation at rtol = 0", CASE_SYM_RTOL0, LAMBDA1, l2c, float(l3c[0]), "photon energy is not conserved", CASE_SYM))
    out.append(("conservation at rtol = 0", CASE_TAYLOR_RTOL0, LAMBDA1, l2c, float(l3c[0]), "photon energy is not conserved", CASE_TAYLOR))
    out.append(("r4 against w4", CASE_SYM_RTOL0, LAMBDA1, l2, r4_breaker(l2), "symmetric form gives w4", CASE_SYM))
    out.append(("|omega_d| < omega_c", CASE_SYM, LAMBDA1, 1e12, float(ax3[-1]), ">= omega_c", CASE_TAYLOR))     # lambda_3 > lambda_1: w4 > 0
    out.append(("r3 > 0", CASE_SYM, LAMBDA1, l2, 1e12, "signal/idler frequency <= 0", CASE_TAYLOR))
    out.append(("non-finite dbeta", CASE_SYM_OVERFLOW, LAMBDA1, l2, l3, "non-finite dbeta", CASE_SYM))
    out.append(("non-finite dbeta", CASE_TAYLOR_OVERFLOW, LAMBDA1, l2, l3, "non-finite dbeta", CASE_TAYLOR))
    return out


# the large grids: 70 001 x 70 001 = 4.9e9 points, of which only the axes exist
BIG_N = 70_001
BIG_POINTS = 300
BIG_FIRSTS = (2 ** 31 - 150, 2 ** 32 - 150, (2 ** 32 // BIG_N + 2) * BIG_N - 120)    # the last: a row boundary above 2^32


def big_axes():
    rng = np.random.default_rng(20240602)
    return rng.uniform(1545e-9, 1570e-9, BIG_N), rng.uniform(1500e-9, 1620e-9, BIG_N)


def big_pair_axes():
    rng = np.random.default_rng(20240603)
    return rng.uniform(-3e13, 3e13, BIG_N), rng.uniform(-3e13, 3e13, BIG_N)


def small_grid_of(first: int, n_points: int, n3: int):
    """The rows a block [first, first + n_points) of a grid with n3 columns touches, and the block's first index in the grid
    made of those rows alone; Python integers throughout.  -> (rows, first_in_small_grid)."""
    r0, r1 = first // n3, (first + n_points - 1) // n3
    return list(range(r0, r1 + 1)), first - r0 * n3


# ---- the aggregate figure ----------------------------------------------------------------------------------------------------
def unit_errors(values, refs):
    """e = |got - staged| / scale per point, as float64.  refs: [(value, scale, B)]."""
    return np.array([float(abs(_fr(v) - r[0]) / r[1]) for v, r in zip(values, refs)])


def worst_over_bound(values, refs) -> float:
    """max |got - staged| / B over the points."""
    return max(float(abs(_fr(v) - r[0]) / r[2]) for v, r in zip(values, refs))
