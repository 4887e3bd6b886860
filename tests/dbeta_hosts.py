"""The package's two host statements of the phase mismatch on the input sets of tests/dbeta_exact.py, each point with its
exact references, computed once per process and shared by tests/test_dbeta_exact_host.py and tests/test_gpu_dbeta_exact.py.

scalar: frequency_plan.plan_from_wavelengths + phase_matching.compute_phase_mismatch, the reference-faithful path that raises;
        a point is valid where it does not raise and its dbeta is finite (the drivers' rule).
array:  plan_from_wavelengths_batch + compute_phase_mismatch_batch, what feeds the sweeps.
"""
import functools

import numpy as np

import dbeta_exact as X
from psa_amd import dispersion, frequency_plan, phase_matching


def disp_cfg(case):
    """The package's (DispersionParams, PhaseMatchingConfig) of a case."""
    b = case["beta"]
    d = dispersion.DispersionParams(omega_ref=case["omega_ref"], beta0=b[0], beta1=b[1], beta2=b[2], beta3=b[3], beta4=b[4],
                                    extra={n: b[n] for n in range(5, X.MAX_ORDER + 1)})
    if case["method"] == "symmetric":
        cfg = phase_matching.PhaseMatchingConfig(method="symmetric_even", even_orders=case["orders"], atol=case["atol"],
                                                 rtol=case["rtol"])
    else:
        cfg = phase_matching.PhaseMatchingConfig(method="general_taylor", max_order=case["max_order"], atol=case["atol"],
                                                 rtol=case["rtol"])
    return d, cfg


def scalar_point(case, l1, l2, l3, d_cfg=None):
    """-> (dbeta or NaN, valid, plan or None, the message of what the scalar path raised or None)."""
    d, cfg = d_cfg or disp_cfg(case)
    with np.errstate(all="ignore"):
        try:
            om = frequency_plan.plan_from_wavelengths(l1, l2, l3)
            res = phase_matching.compute_phase_mismatch(om, d, cfg)
        except (ValueError, TypeError, OverflowError) as exc:
            return float("nan"), False, None, str(exc)
    db = float(res.delta_beta)
    if not np.isfinite(db):
        return float("nan"), False, None, "non-finite dbeta"
    plan = dict(w=tuple(float(w) for w in om))
    if res.symmetric is not None:
        plan.update(od=float(res.symmetric.omega_d), Om=float(res.symmetric.Omega))
    return db, True, plan, None


def scalar_grid(case, l1, points):
    """The scalar path over [(l2, l3)].  -> (dbeta[n] with NaN, valid[n], plans[n])."""
    d_cfg = disp_cfg(case)
    got = [scalar_point(case, l1, l2, l3, d_cfg) for l2, l3 in points]
    return np.array([g[0] for g in got]), np.array([g[1] for g in got], dtype=bool), [g[2] for g in got]


def array_grid(case, l1, ax2, ax3):
    """The array path over the flattened ax2 x ax3 grid.  -> (dbeta[n] with NaN, valid[n], omega[n, 4])."""
    d, cfg = disp_cfg(case)
    L2, L3 = np.meshgrid(np.asarray(ax2, dtype=float), np.asarray(ax3, dtype=float), indexing="ij")
    om, ok = frequency_plan.plan_from_wavelengths_batch(l1, L2.ravel(), L3.ravel())
    db, ok2 = phase_matching.compute_phase_mismatch_batch(om, d, cfg)
    good = ok & ok2
    return np.where(good, db, np.nan), good, om


@functools.lru_cache(maxsize=None)
def evaluated(name):
    """A case of X.CASES / X.CASES_TOLERANCE on its grid (X.axes_of): the two host statements, and for every valid point the
    staged reference (value, scale, B) and the exact function of the wavelengths."""
    case = next(c for c in X.CASES + X.CASES_TOLERANCE if c["name"] == name)
    ax2, ax3 = X.axes_of(case)
    points = X.grid_points(ax2, ax3)
    scalar, valid, plans = scalar_grid(case, X.LAMBDA1, points)
    array, valid_a, om = array_grid(case, X.LAMBDA1, ax2, ax3)
    idx = np.flatnonzero(valid)
    refs = [X.staged(case, plans[i]) for i in idx]
    exact = [X.from_wavelengths(case, X.LAMBDA1, *points[i]) for i in idx]
    return dict(case=case, ax2=ax2, ax3=ax3, points=points, scalar=scalar, valid=valid, plans=plans, array=array,
                valid_array=valid_a, omega_array=om, idx=idx, refs=refs, exact=exact)


@functools.lru_cache(maxsize=None)
def evaluated_pairs(orders):
    """The six-wave pair grid for one order set: per axis the scalar statement (dispersion.delta_beta_symmetric), the array
    statement and the staged references."""
    case = X._case(f"pairs {orders}", "symmetric", orders=orders, beta=X.BETA_EVEN)
    d, _ = disp_cfg(case)
    out = dict(case=case, od=X.PAIR_OMEGA_D)
    for key, axis in zip(("axis1", "axis2"), X.pair_axes()):
        scalar = np.array([dispersion.delta_beta_symmetric(1.2e15, X.PAIR_OMEGA_D, float(Om), d, even_orders=orders) for Om in axis])
        array = dispersion.delta_beta_symmetric_array(X.PAIR_OMEGA_D, axis, d, even_orders=orders)
        refs = [X.staged_symmetric(case["beta"], orders, X.PAIR_OMEGA_D, float(Om)) for Om in axis]
        out[key] = dict(axis=axis, scalar=scalar, array=array, refs=refs)
    return out


def line(label, name, e_got, e_twin, worst):
    """One line of the record (profiles/dbeta_errors.txt)."""
    med, mx, tmed, tmx = float(np.median(e_got)), float(e_got.max()), float(np.median(e_twin)), float(e_twin.max())
    r_med = med / tmed if tmed > 0 else (1.0 if med == 0 else float("inf"))
    r_max = mx / tmx if tmx > 0 else (1.0 if mx == 0 else float("inf"))
    print(f"\ndbeta | {label} | {name} | {med:.3e} {mx:.3e} | twin {tmed:.3e} {tmx:.3e} | ratio {r_med:.2f} {r_max:.2f} | "
          f"worst/B {worst:.3f}")
    return r_med, r_max
