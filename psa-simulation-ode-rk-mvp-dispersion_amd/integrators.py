"""Fixed-step RK4 integration -- the operator API of the reference's integrators.py
(``RHSFunction`` :18, ``rk4_step`` :25-61, ``integrate_fixed_step`` :68-142, ``integrate_interval`` :150-204).

Dispatch
--------
* ``f`` is a NATIVE operator handle (``f.native_kind == "yaman4"``, i.e. ``yaman_model.rhs_yaman_simplified``):
  the whole z-loop -- four RHS evaluations per step, save stride, per-step NaN test -- runs inside ONE launch of
  the HIP kernel ``psa_rk4_sweep_f64`` with N = 1 and the trajectory output enabled.  No Python code runs per
  step.  If ``libpsa_hip.so`` or a GPU is missing this raises; it never degrades to a host loop.
* ``f`` is an arbitrary Python callable (what the reference's own tests pass: ``lambda z, y, p: y``): the callback
  has to execute on the host by definition, so the stepping loop around it does too (``_step_callable`` below).
  This is the reference's generic-operator contract, not a fallback for the Yaman path.

Semantics kept from the reference: n = int(round(z_max/dz)) and the grid np.linspace(0, z_max, n+1) (R7);
rows only at multiples of ``save_every`` plus z = 0, ``n_saved = n // save_every + 1`` (R8); ValueError for
bad z_max / dz / save_every / z_grid.ndim; FloatingPointError("NaN or Inf detected at step {i}, z = {z}")
when ``check_nan`` and the state after step i is not finite; silent NaNs otherwise.
"""
from __future__ import annotations

from typing import Callable, Tuple

import numpy as np

from . import _native

RHSFunction = Callable[[float, np.ndarray, object], np.ndarray]

__all__ = ["RHSFunction", "rk4_step", "integrate_fixed_step", "integrate_interval", "integrate_adaptive"]


def _is_native(f) -> bool:
    return getattr(f, "native_kind", None) == "yaman4"


def rk4_step(f: RHSFunction, z: float, y: np.ndarray, dz: float, params: object) -> np.ndarray:
    """One classic RK4 step; ``f`` may be a Python callable or the native RHS handle (4 batched-kernel calls)."""
    half = 0.5 * dz
    k1 = f(z, y, params)
    k2 = f(z + half, y + half * k1, params)
    k3 = f(z + half, y + half * k2, params)
    k4 = f(z + dz, y + dz * k3, params)
    return y + (dz / 6.0) * (k1 + 2.0 * k2 + 2.0 * k3 + k4)


def _step_callable(f, z_grid, y0, params, save_every, check_nan):
    """Host stepping loop for user-supplied Python right-hand sides (see module docstring)."""
    n = len(z_grid) - 1
    rows = n // save_every + 1
    z_out = np.empty(rows, dtype=float)
    y_out = np.empty((rows, y0.size), dtype=y0.dtype)
    y = y0.copy()
    z_out[0], y_out[0] = z_grid[0], y
    r = 1
    for i in range(n):
        y = rk4_step(f, z_grid[i], y, z_grid[i + 1] - z_grid[i], params)
        if check_nan and not np.all(np.isfinite(y)):
            raise FloatingPointError(f"NaN or Inf detected at step {i}, z = {z_grid[i]}")
        if (i + 1) % save_every == 0:
            z_out[r], y_out[r] = z_grid[i + 1], y
            r += 1
    return z_out[:r], y_out[:r]


def _run_native(f, z_max: float, n_steps: int, y0, params, save_every: int, check_nan: bool):
    """N = 1 launch of the sweep kernel with every saved row written out."""
    from .yaman_model import extract_gamma_alpha_dbeta
    gamma, alpha, dbeta = extract_gamma_alpha_dbeta(params)
    a0 = np.asarray(y0)
    if a0.shape != (4,):
        raise ValueError("a_arr must have shape (4,)")
    res = _native.sweep_host(np.array([dbeta]), n_steps=n_steps, z_max=z_max, save_every=save_every, gamma=gamma,
                             alpha=alpha, a0=a0.astype(np.complex128), check_nan=check_nan, exact_step=True,
                             want_traj=True)
    z_grid = np.linspace(0.0, z_max, n_steps + 1)
    bad = int(res["first_bad_step"][0])
    if check_nan and bad >= 0:
        raise FloatingPointError(f"NaN or Inf detected at step {bad}, z = {z_grid[bad]}")
    rows = res["traj"][0]
    z_out = z_grid[::save_every][: rows.shape[0]].copy()
    if not np.iscomplexobj(a0):  # the reference stores into an array of y0's dtype
        rows = rows.astype(a0.dtype)
    return z_out, rows


def _uniform_from_zero(z_grid: np.ndarray) -> bool:
    n = len(z_grid) - 1
    return n >= 1 and z_grid[0] == 0.0 and z_grid[-1] > 0.0 and \
        np.array_equal(z_grid, np.linspace(0.0, z_grid[-1], n + 1))


def integrate_fixed_step(f: RHSFunction, z_grid: np.ndarray, y0: np.ndarray, params: object, *,
                         save_every: int = 1, check_nan: bool = True) -> Tuple[np.ndarray, np.ndarray]:
    """RK4 over a given monotone grid -> (z_out[n_saved], y_out[n_saved, state_dim])."""
    z_grid = np.asarray(z_grid, dtype=float)
    if z_grid.ndim != 1:
        raise ValueError("z_grid must be a one-dimensional array")
    if save_every <= 0:
        raise ValueError("save_every must be a positive integer")
    y0 = np.asarray(y0)
    if _is_native(f) and _uniform_from_zero(z_grid):
        return _run_native(f, float(z_grid[-1]), len(z_grid) - 1, y0, params, int(save_every), bool(check_nan))
    # arbitrary grids / arbitrary callables: the callback contract (for the native handle each stage is one
    # call of the batched HIP RHS kernel)
    return _step_callable(f, z_grid, y0, params, int(save_every), bool(check_nan))


def integrate_interval(f: RHSFunction, z_max: float, dz: float, y0: np.ndarray, params: object, *,
                       save_every: int = 1, check_nan: bool = True) -> Tuple[np.ndarray, np.ndarray]:
    """RK4 on [0, z_max] with nominal step dz (effective step z_max / round(z_max/dz))."""
    if z_max <= 0.0:
        raise ValueError("z_max must be positive")
    if dz <= 0.0:
        raise ValueError("dz must be positive")
    if save_every <= 0:
        raise ValueError("save_every must be a positive integer")
    n_steps = int(round(z_max / dz))
    if _is_native(f):
        if n_steps < 1:
            return np.zeros(1), np.asarray(y0)[None, :].copy()
        return _run_native(f, float(z_max), n_steps, np.asarray(y0), params, int(save_every), bool(check_nan))
    return integrate_fixed_step(f, np.linspace(0.0, z_max, n_steps + 1), np.asarray(y0), params,
                                save_every=save_every, check_nan=check_nan)


# ---- adaptive integration: embedded Dormand-Prince 5(4), scipy.integrate.RK45 step for step ----------------------------
# (tableau, controller and dense output of scipy 1.15 _ivp/rk.py; initial step of _ivp/common.py select_initial_step)
_RK45_C = (0.0, 1 / 5, 3 / 10, 4 / 5, 8 / 9, 1.0)
_RK45_A = ((), (1 / 5,), (3 / 40, 9 / 40), (44 / 45, -56 / 15, 32 / 9),
           (19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729),
           (9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656))
_RK45_B = np.array([35 / 384, 0.0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84])
_RK45_E = np.array([-71 / 57600, 0.0, 71 / 16695, -71 / 1920, 17253 / 339200, -22 / 525, 1 / 40])
_RK45_P = np.array([
    [1, -8048581381 / 2820520608, 8663915743 / 2820520608, -12715105075 / 11282082432],
    [0, 0, 0, 0],
    [0, 131558114200 / 32700410799, -68118460800 / 10900136933, 87487479700 / 32700410799],
    [0, -1754552775 / 470086768, 14199869525 / 1410260304, -10690763975 / 1880347072],
    [0, 127303824393 / 49829197408, -318862633887 / 49829197408, 701980252875 / 199316789632],
    [0, -282668133 / 205662961, 2019193451 / 616988883, -1453857185 / 822651844],
    [0, 40617522 / 29380423, -110615467 / 29380423, 69997945 / 29380423]])


def _rms(x) -> float:
    return float(np.linalg.norm(x) / x.size ** 0.5)


def _rk45_callable(f, z_max: float, y0: np.ndarray, params, tol, n_out: int):
    """Host loop for user-supplied Python right-hand sides: the algorithm of the kernel, one point."""
    rtol, atol, h_max, max_steps = float(tol.rtol), float(tol.atol), float(tol.h_max), int(tol.max_steps)
    cdt = np.result_type(y0.dtype, np.float64)
    y = np.array(y0, dtype=cdt)
    t_eval = np.linspace(0.0, z_max, n_out + 1)
    rows = np.full((n_out + 1, y.size), np.nan, dtype=cdt)
    rows[0] = y
    nxt, z, n_acc, n_rej = 1, 0.0, 0, 0
    fun = lambda t, v: np.asarray(f(t, v, params), dtype=cdt)  # noqa: E731
    if not np.all(np.isfinite(y)):
        return rows, dict(status=1, z_end=0.0, n_accepted=0, n_rejected=0, y_end=y)
    fz = fun(0.0, y)
    if tol.first_step > 0.0:
        h_abs = float(tol.first_step)
    else:
        scale = atol + np.abs(y) * rtol
        d0, d1 = _rms(y / scale), _rms(fz / scale)
        h0 = 1e-6 if (d0 < 1e-5 or d1 < 1e-5) else 0.01 * d0 / d1
        h0 = min(h0, z_max)
        d2 = _rms((fun(h0, y + h0 * fz) - fz) / scale) / h0
        h1 = max(1e-6, h0 * 1e-3) if (d1 <= 1e-15 and d2 <= 1e-15) else (0.01 / max(d1, d2)) ** (1 / 5)
        h_abs = min(100 * h0, h1, z_max, h_max)
    status = None
    K = np.empty((7, y.size), dtype=cdt)
    with np.errstate(all="ignore"):
        while status is None:
            min_step = 10 * np.abs(np.nextafter(z, np.inf) - z)
            h_abs = h_max if h_abs > h_max else (min_step if h_abs < min_step else h_abs)
            rejected = False
            while True:
                if h_abs < min_step:
                    status = 1
                    break
                if n_acc + n_rej >= max_steps:
                    status = 2
                    break
                t_new = min(z + h_abs, z_max)
                h = t_new - z
                h_abs = abs(h)
                K[0] = fz
                for s in range(1, 6):
                    K[s] = fun(z + _RK45_C[s] * h, y + np.dot(K[:s].T, _RK45_A[s]) * h)
                y_new = y + h * np.dot(K[:-1].T, _RK45_B)
                K[6] = fun(z + h, y_new)
                scale = atol + np.maximum(np.abs(y), np.abs(y_new)) * rtol
                en = _rms(np.dot(K.T, _RK45_E) * h / scale)
                if en < 1:
                    fac = 10.0 if en == 0 else min(10.0, 0.9 * en ** -0.2)
                    h_abs *= min(1.0, fac) if rejected else fac
                    break
                h_abs *= max(0.2, 0.9 * en ** -0.2)
                rejected = True
                n_rej += 1
            if status is not None:
                break
            Q = K.T.dot(_RK45_P)
            while nxt <= n_out and t_eval[nxt] <= t_new:
                rows[nxt] = h * np.dot(Q, np.cumprod(np.full(4, (t_eval[nxt] - z) / h))) + y
                nxt += 1
            y, fz, z = y_new, K[6].copy(), t_new
            n_acc += 1
            if z >= z_max:
                status = 0
    return rows, dict(status=status, z_end=z, n_accepted=n_acc, n_rejected=n_rej, y_end=y)


def integrate_adaptive(f: RHSFunction, z_max: float, y0: np.ndarray, params: object, *, tol, n_out: int):
    """Adaptive RK45 on [0, z_max] to the tolerance ``tol`` (config.AdaptiveConfig) -> (z_out, y_out, info).

    Rows are the dense output at z_out = np.linspace(0, z_max, n_out + 1) (row 0 is y0; rows past the end of a failed
    run are NaN); info = dict(status, z_end, n_accepted, n_rejected, y_end) with the status codes of psa_rk45_sweep_f64.
    The native handle (rhs_yaman_simplified) runs one N = 1 launch of the adaptive kernel; any other callable runs the
    same algorithm in a host loop around the callback."""
    from .config import AdaptiveConfig
    if not isinstance(tol, AdaptiveConfig):
        raise TypeError("tol must be an AdaptiveConfig")
    tol.validate()
    z_max = float(z_max)
    if not (np.isfinite(z_max) and z_max > 0.0):
        raise ValueError("z_max must be positive")
    n_out = int(n_out)
    if n_out < 0:
        raise ValueError("n_out must be >= 0")
    y0 = np.asarray(y0)
    z_out = np.linspace(0.0, z_max, n_out + 1)
    if _is_native(f):
        from .yaman_model import extract_gamma_alpha_dbeta
        if y0.shape != (4,):
            raise ValueError("a_arr must have shape (4,)")
        gamma, alpha, dbeta = extract_gamma_alpha_dbeta(params)
        r = _native.rk45_sweep_host(np.array([dbeta]), z_max=z_max, rtol=tol.rtol, atol=tol.atol, h_max=tol.h_max,
                                    first_step=tol.first_step, max_steps=int(tol.max_steps), n_out=n_out, gamma=gamma,
                                    alpha=alpha, a0=y0.astype(np.complex128))
        rows = r["traj"][0] if n_out > 0 else y0.astype(np.complex128)[None, :]
        info = dict(status=int(r["status"][0]), z_end=float(r["z_end"][0]), n_accepted=int(r["n_accepted"][0]),
                    n_rejected=int(r["n_rejected"][0]), y_end=r["a_end"][0])
        return z_out, rows, info
    rows, info = _rk45_callable(f, z_max, y0, params, tol, n_out)
    return z_out, rows, info
