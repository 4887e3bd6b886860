"""The exact yardstick of tests/dbeta_exact.py pinned against mpmath, the package's two host statements of the phase mismatch
held to it, the spread between them that sets the aggregate factor of tests/test_gpu_dbeta_exact.py, the two planted defects
against the bars of that file, and the validity rules one by one.  CPU only.

Every bar here is the GPU file's: a point lies within 2 B of the staged value (B: the derived first-order bound), a set's median
and maximum of e = |got - staged| / scale stay within FACTOR_* of the scalar path's, masks are equal, a block of a large grid
is the same bits as the small-grid evaluation of the same (l2, l3) pairs.
"""
import math
from fractions import Fraction

import numpy as np
import pytest

import dbeta_exact as X
import dbeta_hosts as H

ALL_CASES = X.CASES + X.CASES_TOLERANCE
_ids = [c["name"] for c in ALL_CASES]


# ---- the bars, as the GPU file applies them --------------------------------------------------------------------------------
def within_2B(values, refs):
    """|got - staged| <= 2 B at every point, exactly.  The factor 2 covers the second-order terms of a first-order bound."""
    return all(abs(Fraction(float(v)) - r[0]) <= 2 * r[2] for v, r in zip(values, refs))


def aggregate_ok(e_got, e_twin):
    return (np.median(e_got) <= X.FACTOR_MEDIAN * np.median(e_twin)) and (e_got.max() <= X.FACTOR_MAX * e_twin.max())


def large_grid_ok(producer, ax2, ax3, first):
    """``producer(ax2, ax3, first, n)`` -> n numbers.  The block [first, first + BIG_POINTS) of the whole grid against the same
    producer on the grid made of the block's rows alone, where every index is small."""
    rows, first_small = X.small_grid_of(first, X.BIG_POINTS, len(ax3))
    want = producer(ax2[rows], ax3, first_small, X.BIG_POINTS)
    return np.array_equal(producer(ax2, ax3, first, X.BIG_POINTS), want, equal_nan=True)


# ---- the yardstick itself ----------------------------------------------------------------------------------------------------
def test_the_model_constant_is_the_packages():
    import psa_amd._native as nat
    from psa_amd import constants
    assert constants.c == X.C_LIGHT
    assert nat.dbeta_model(*H.disp_cfg(X.CASE_SYM))["two_pi_c"] == X.TWO_PI_C
    assert nat.DBETA_MAX_ORDER == X.MAX_ORDER


@pytest.mark.parametrize("case", X.CASES, ids=[c["name"] for c in X.CASES])
def test_yardstick_against_mpmath_at_50_digits(case):
    """Five points of every method and order set: the staged value at the host's plan and the function of the wavelengths, written
    again in mpmath from the equations.  50 digits leave ~1e-49 of the largest term; the Fractions are exact."""
    import mpmath as mp
    mp.mp.dps = 50
    ev = H.evaluated(case["name"])
    F = lambda x: mp.mpf(float(x))                                              # noqa: E731  (a float64 is exact in mpf)
    Q = lambda q: mp.mpf(q.numerator) / mp.mpf(q.denominator)                   # noqa: E731
    beta = [F(b) for b in case["beta"]]

    def sym(od, Om):
        return mp.fsum(beta[n] * (Om ** n - od ** n) * 2 / mp.factorial(n) for n in case["orders"])

    def taylor(w):
        dw = w - F(case["omega_ref"])
        return mp.fsum(beta[n] * dw ** n / mp.factorial(n) for n in range(case["max_order"] + 1))

    for k in (0, 1, 150, 255, 300):
        i = ev["idx"][k]
        plan, (value, scale, B) = ev["plans"][i], ev["refs"][k]
        l2, l3 = ev["points"][i]
        w = [F(X.TWO_PI_C) / F(l) for l in (X.LAMBDA1, l2, l3)]
        w.append(w[0] + w[1] - w[2])
        if case["method"] == "symmetric":
            st = sym(F(plan["od"]), F(plan["Om"]))
            ex = sym((w[0] - w[1]) / 2, w[2] - (w[0] + w[1]) / 2)
        else:
            b = [taylor(F(x)) for x in plan["w"]]
            st = (b[2] + b[3]) - (b[0] + b[1])
            b = [taylor(x) for x in w]
            ex = (b[2] + b[3]) - (b[0] + b[1])
        assert abs(st - Q(value)) <= mp.mpf(10) ** -45 * Q(scale), (case["name"], k)
        assert abs(ex - Q(ev["exact"][k])) <= mp.mpf(10) ** -45 * Q(scale), (case["name"], k)
        assert 0 < B == (len(case["orders"]) + 3 if case["method"] == "symmetric" else 2 * case["max_order"] + 6) * X.U * scale


# ---- the two host statements -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL_CASES, ids=_ids)
def test_host_statements_lie_inside_the_bound(case):
    """The scalar path, the array path and the restated operation list: same validity, same plan bits, every valid point within
    the FIRST-ORDER bound B of the staged value (the GPU file allows the kernel 2 B)."""
    ev = H.evaluated(case["name"])
    idx, refs = ev["idx"], ev["refs"]
    twin, ok_twin = X.twin_grid(case, X.LAMBDA1, ev["ax2"], ev["ax3"])
    assert np.array_equal(ev["valid_array"], ev["valid"]) and np.array_equal(ok_twin, ev["valid"])
    assert np.array_equal(np.isnan(ev["array"]), ~ev["valid"]) and np.array_equal(np.isnan(twin), ~ev["valid"])
    assert np.array_equal(ev["omega_array"][idx], np.array([ev["plans"][i]["w"] for i in idx]))      # the plan stage, bit for bit
    e_scalar = X.unit_errors(ev["scalar"][idx], refs)
    for label, values in (("host scalar", ev["scalar"]), ("host array", ev["array"]), ("restated list", twin)):
        worst = X.worst_over_bound(values[idx], refs)
        H.line(label, case["name"], X.unit_errors(values[idx], refs), e_scalar, worst)
        assert worst <= 1.0, (label, worst)
    if case["name"] in X.ORDERS_LE_2:
        assert np.array_equal(ev["array"], ev["scalar"], equal_nan=True) and np.array_equal(twin, ev["scalar"], equal_nan=True)
    rel = np.array([float(abs(Fraction(v) - e) / abs(e)) for v, e in zip(ev["scalar"][idx], ev["exact"])])
    print(f"\ndbeta | host scalar against the exact function of the wavelengths | {case['name']} | relative median {np.median(rel):.1e} "
          f"max {rel.max():.1e}")
    if case["grid"] == "tolerance" and case["rtol"] != 1e-12:       # conditions on the inputs: the tolerances decide
        n_bad = int((~ev["valid"]).sum())
        print(f"\ndbeta | {case['name']} | {n_bad} of {ev['valid'].size} plans invalid")
        assert n_bad <= ev["valid"].size - 100
        if case["rtol"] == 0.0:
            assert n_bad >= 3                                         # the planted conservation breakers at the least
        else:                                                         # the non-default pair admits what rtol = atol = 0 refuses
            assert not np.array_equal(ev["valid"], H.evaluated(case["name"].split(" atol")[0] + " rtol=0")["valid"])
            assert n_bad >= 1 or case["method"] == "taylor"           # ... and, in the symmetric form, refuses what the default admits


@pytest.mark.parametrize("orders", X.PAIR_ORDER_SETS, ids=str)
def test_pair_grid_host_statements_lie_inside_the_bound(orders):
    ev = H.evaluated_pairs(orders)
    for key in ("axis1", "axis2"):
        a = ev[key]
        twin = np.array([X.twin_symmetric(ev["case"]["beta"], orders, ev["od"], float(Om)) for Om in a["axis"]])
        e_scalar = X.unit_errors(a["scalar"], a["refs"])
        for label, values in (("host scalar", a["scalar"]), ("host array", a["array"]), ("restated list", twin)):
            worst = X.worst_over_bound(values, a["refs"])
            H.line(label, f"pairs {orders} {key}", X.unit_errors(values, a["refs"]), e_scalar, worst)
            assert worst <= 1.0, (label, key, worst)
        assert (a["axis"] == 0.0).any() and (a["axis"] < 0.0).any()


def test_the_spread_between_the_host_statements_sets_the_factors():
    """The measurement behind FACTOR_MEDIAN and FACTOR_MAX: over every set, how far apart are the two host statements' median
    and maximum of e?  Three times that, rounded up to the next integer, is the factor -- measured here, never on the kernel."""
    spread_med = spread_max = 1.0
    for case in ALL_CASES:
        ev = H.evaluated(case["name"])
        es, ea = (X.unit_errors(ev[k][ev["idx"]], ev["refs"]) for k in ("scalar", "array"))
        r_med = max(np.median(es) / np.median(ea), np.median(ea) / np.median(es))
        r_max = max(es.max() / ea.max(), ea.max() / es.max())
        print(f"\ndbeta | spread scalar/array | {case['name']} | median {r_med:.4f} max {r_max:.4f}")
        spread_med, spread_max = max(spread_med, r_med), max(spread_max, r_max)
    print(f"\ndbeta | spread over the sets | median {spread_med:.4f} max {spread_max:.4f}")
    assert spread_med <= X.SPREAD_MEDIAN and spread_max <= X.SPREAD_MAX
    assert X.FACTOR_MEDIAN == math.ceil(3 * X.SPREAD_MEDIAN) and X.FACTOR_MAX == math.ceil(3 * X.SPREAD_MAX)


# ---- the planted defects -----------------------------------------------------------------------------------------------------
def _twin_producer(case, **defect):
    return lambda ax2, ax3, first, n: X.twin_grid(case, X.LAMBDA1, ax2, ax3, first, n, **defect)[0]


def test_planted_defect_omega_from_the_idler():
    """Omega taken as omega_c - w4 instead of w3 - omega_c.

    Where w4 = fl(fl(w1 + w2) - w3) is exact -- every signal wavelength within about four times the pumps', the whole band --
    both differences are the SAME real number rounded once, and the planted change moves no bit: shown first, on every in-band
    symmetric set.  It is a defect where w4 is rounded (the grid of tolerance_axes, lambda_3 of 6.5 um and more), by one ulp of w4 in
    Omega ~ 1e15.  There it misses the per-point bound on order 8 (8 ulp of Omega on one term against 2 B = 8 u), misses the
    aggregate bar there, and changes the validity mask at rtol = 0, where r4 = omega_c - Omega is compared with w4 bit for
    bit.  On (2,4) its 2 ulp stay inside 2 B = 10 u: the bound has no room to spare, and none to give.  It passes the large grid."""
    for case in X.CASES:
        if case["method"] == "symmetric" and case["grid"] == "band":
            ev = H.evaluated(case["name"])
            got, ok = X.twin_grid(case, X.LAMBDA1, ev["ax2"], ev["ax3"], omega_from_idler=True)
            clean, _ = X.twin_grid(case, X.LAMBDA1, ev["ax2"], ev["ax3"])
            assert np.array_equal(got, clean) and ok.all(), case["name"]
    ev = H.evaluated("sym (8,) long lambda3")
    got, ok = X.twin_grid(ev["case"], X.LAMBDA1, ev["ax2"], ev["ax3"], omega_from_idler=True)
    clean, _ = X.twin_grid(ev["case"], X.LAMBDA1, ev["ax2"], ev["ax3"])
    assert ok.all() and ev["valid"].all()
    e_scalar = X.unit_errors(ev["scalar"], ev["refs"])
    H.line("planted: Omega from the idler", ev["case"]["name"], X.unit_errors(got, ev["refs"]), e_scalar, X.worst_over_bound(got, ev["refs"]))
    assert within_2B(clean, ev["refs"]) and not within_2B(got, ev["refs"])
    assert aggregate_ok(X.unit_errors(clean, ev["refs"]), e_scalar) and not aggregate_ok(X.unit_errors(got, ev["refs"]), e_scalar)
    ev = H.evaluated("sym (2,4) rtol=0")
    _, ok = X.twin_grid(ev["case"], X.LAMBDA1, ev["ax2"], ev["ax3"], omega_from_idler=True)
    assert not np.array_equal(ok, ev["valid"])
    print(f"\ndbeta | planted: Omega from the idler | {ev['case']['name']} | {int((ok != ev['valid']).sum())} of {ok.size} mask entries differ")
    ax2, ax3 = X.big_axes()
    for first in X.BIG_FIRSTS:
        assert large_grid_ok(_twin_producer(X.CASE_SYM, omega_from_idler=True), ax2, ax3, first)


def test_planted_defect_flat_index_split_in_32_bits():
    """The flat index held in an int: every block of the small sets is untouched (same bits as the clean list, inside every
    bar), every block of the large grid is other points."""
    for case in (X.CASE_SYM, X.CASE_TAYLOR):
        ev = H.evaluated(case["name"])
        got, ok = X.twin_grid(case, X.LAMBDA1, ev["ax2"], ev["ax3"], split=X.split_int32)
        assert ok.all() and within_2B(got, ev["refs"])
        assert aggregate_ok(X.unit_errors(got, ev["refs"]), X.unit_errors(ev["scalar"], ev["refs"]))
        ax2, ax3 = X.big_axes()
        for first in X.BIG_FIRSTS:
            assert large_grid_ok(_twin_producer(case), ax2, ax3, first)
            assert not large_grid_ok(_twin_producer(case, split=X.split_int32), ax2, ax3, first), first


def test_large_grid_blocks_are_where_the_issue_puts_them():
    n = X.BIG_N
    assert n * n > 2 ** 32 and all(f + X.BIG_POINTS <= n * n for f in X.BIG_FIRSTS)
    a, b, c = X.BIG_FIRSTS
    assert a < 2 ** 31 < a + X.BIG_POINTS and b < 2 ** 32 < b + X.BIG_POINTS and c > 2 ** 32
    assert c // n != (c + X.BIG_POINTS - 1) // n and (c + 255) // n != c // n          # a row boundary inside the first block of 256
    rows, first_small = X.small_grid_of(c, X.BIG_POINTS, n)
    assert len(rows) == 2 and first_small == n - 120


# ---- validity ----------------------------------------------------------------------------------------------------------------
def test_every_validity_rule_tripped_alone():
    """Each point of rule_points() is invalid on the scalar path FOR THE STATED REASON (the message of what it raises names the
    rule), valid under the neighbouring case where one is given (so nothing else is wrong with it), and the array path and the
    restated operation list agree.  The rules nothing can trip alone are listed, with reasons, in rule_points' docstring."""
    seen = set()
    for label, case, l1, l2, l3, fragment, valid_under in X.rule_points():
        db, ok, _, msg = H.scalar_point(case, l1, l2, l3)
        assert not ok and np.isnan(db) and fragment in msg, (label, case["name"], msg)
        with np.errstate(all="ignore"):
            a_db, a_ok, _ = H.array_grid(case, l1, [l2], [l3])
        t_db, t_ok = X.twin_point(case, l1, l2, l3)
        assert not a_ok[0] and np.isnan(a_db[0]) and not t_ok and np.isnan(t_db), (label, case["name"])
        if valid_under is not None:
            assert H.scalar_point(valid_under, l1, l2, l3)[1] and X.twin_point(valid_under, l1, l2, l3)[1], (label, case["name"])
        seen.add(label.split(" = ")[0])
    assert seen >= {"lambda1", "lambda2", "lambda3", "omega4 <= 0", "omega4 non-finite", "conservation at rtol", "r4 against w4",
                    "|omega_d| < omega_c", "r3 > 0", "non-finite dbeta"}


def test_wide_grid_has_both_kinds_of_plan():
    """The 64 x 64 cut of the wide grid the GPU file compares masks on: at least a tenth of its plans invalid and at least a
    third valid on the scalar path, and the array path and the restated list give the same mask."""
    l2, l3 = X.wide_axes()
    for case in (X.CASE_SYM, X.CASE_TAYLOR):
        _, valid, _ = H.scalar_grid(case, X.LAMBDA1, X.grid_points(l2, l3))
        share = valid.mean()
        print(f"\ndbeta | wide grid | {case['name']} | {int(valid.sum())} of {valid.size} plans valid")
        assert 1 / 3 <= share <= 0.9
        with np.errstate(all="ignore"):
            assert np.array_equal(H.array_grid(case, X.LAMBDA1, l2, l3)[1], valid)
        assert np.array_equal(X.twin_grid(case, X.LAMBDA1, l2, l3)[1], valid)
