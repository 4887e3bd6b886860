"""NumPy restatement of the adaptive sweep (psa_rk45_sweep_f64), vectorised over sweep points.

scipy.integrate.RK45 (scipy 1.15: _ivp/rk.py, _ivp/common.py) step for step, with a step size, a z and a step count of
its own for every point, plus what the kernel adds: the max_steps cap (status 2), the per-point summary and the dense
rows at np.linspace(0, z_max, n_out + 1).  Test infrastructure: no scipy, not imported by the package.  The right-hand
sides are the oracle's NumPy statements (oracle.np_rhs, oracle.np_rhs6).

    rk45(rhs, y0, z_max, rtol=..., atol=...) -> dict(a_end, p_end, p_max, status, z_end, n_accepted, n_rejected, traj, steps)

rhs(z[m], y[n, m], idx[m]) -> dy/dz [n, m] for the points idx (m of them); y0 is (n, N) complex.  steps: the accepted
(z, h) pairs of the point ``record``, or None.
"""
from __future__ import annotations

import numpy as np

C = [0.0, 1 / 5, 3 / 10, 4 / 5, 8 / 9, 1.0]
A = [[], [1 / 5], [3 / 40, 9 / 40], [44 / 45, -56 / 15, 32 / 9],
     [19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729],
     [9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656]]
B = [35 / 384, 0.0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84]
E = [-71 / 57600, 0.0, 71 / 16695, -71 / 1920, 17253 / 339200, -22 / 525, 1 / 40]
P = np.array([
    [1, -8048581381 / 2820520608, 8663915743 / 2820520608, -12715105075 / 11282082432],
    [0, 0, 0, 0],
    [0, 131558114200 / 32700410799, -68118460800 / 10900136933, 87487479700 / 32700410799],
    [0, -1754552775 / 470086768, 14199869525 / 1410260304, -10690763975 / 1880347072],
    [0, 127303824393 / 49829197408, -318862633887 / 49829197408, 701980252875 / 199316789632],
    [0, -282668133 / 205662961, 2019193451 / 616988883, -1453857185 / 822651844],
    [0, 40617522 / 29380423, -110615467 / 29380423, 69997945 / 29380423]])
SAFETY, MIN_FACTOR, MAX_FACTOR, ERR_EXP = 0.9, 0.2, 10.0, -1 / 5


def _norm(x):
    """common.norm per column: np.linalg.norm of a complex vector / sqrt(size)."""
    return np.sqrt((x.real * x.real).sum(0) + (x.imag * x.imag).sum(0)) / x.shape[0] ** 0.5


def _comb(K, w):
    s = K[0] * w[0]
    for k in range(1, len(w)):
        s = s + K[k] * w[k]
    return s


def _alpha_of(alpha):
    """alpha one scalar for all points (0.0 keeps the oracle's lossless branch) or (N,) -> idx -> the points' alpha."""
    if np.ndim(alpha) == 0:
        return lambda idx: float(alpha)
    alpha = np.asarray(alpha, dtype=float)
    return lambda idx: alpha[idx]


def rhs4(dbeta, gamma, alpha):
    """Four waves: oracle.np_rhs on (4, m) columns; alpha a scalar or per point."""
    import oracle as O
    dbeta = np.asarray(dbeta, dtype=float)
    gamma = np.broadcast_to(np.asarray(gamma, dtype=float), dbeta.shape)
    al = _alpha_of(alpha)
    return lambda z, y, idx: O.np_rhs(z, y, gamma[idx], al(idx), dbeta[idx])


def rhs6(dbeta1, dbeta2, gamma, alpha):
    """Six waves: oracle.np_rhs6 point by point."""
    import oracle as O
    d1, d2 = np.asarray(dbeta1, dtype=float), np.asarray(dbeta2, dtype=float)
    g = np.broadcast_to(np.asarray(gamma, dtype=float), d1.shape)
    al = _alpha_of(alpha)

    def f(z, y, idx):
        return np.stack([O.np_rhs6(z[k], y[:, k], g[i], al(i), d1[i], d2[i]) for k, i in enumerate(idx)], axis=1)
    return f


def rk45(rhs, y0, z_max, *, rtol, atol, h_max=np.inf, first_step=0.0, max_steps=1_000_000, n_out=0, record=None):
    y = np.array(y0, dtype=np.complex128)
    n, N = y.shape
    z = np.zeros(N)
    status = np.full(N, -1, dtype=np.int32)
    n_acc = np.zeros(N, dtype=np.int64)
    n_rej = np.zeros(N, dtype=np.int64)
    pm = np.abs(y[2]) ** 2
    traj = None
    if n_out > 0:
        traj = np.full((N, n_out + 1, n), np.nan + 1j * np.nan)
        traj[:, 0] = y.T
        t_eval = np.linspace(0.0, z_max, n_out + 1)
    next_row = np.ones(N, dtype=np.int64)
    steps = [] if record is not None else None
    active = np.isfinite(y).all(0)
    status[~active] = 1
    all_idx = np.arange(N)
    with np.errstate(all="ignore"):
        f = np.zeros_like(y)
        ia = all_idx[active]
        if ia.size:
            f[:, ia] = rhs(z[ia], y[:, ia], ia)
        h_abs = np.full(N, float(first_step))
        if first_step <= 0.0 and ia.size:   # common.select_initial_step, order 4
            y0a, f0 = y[:, ia], f[:, ia]
            scale = atol + np.abs(y0a) * rtol
            d0, d1 = _norm(y0a / scale), _norm(f0 / scale)
            h0 = np.where((d0 < 1e-5) | (d1 < 1e-5), 1e-6, 0.01 * d0 / d1)
            h0 = np.minimum(h0, z_max)
            f1 = rhs(z[ia] + h0, y0a + h0 * f0, ia)
            d2 = _norm((f1 - f0) / scale) / h0
            h1 = np.where((d1 <= 1e-15) & (d2 <= 1e-15), np.maximum(1e-6, h0 * 1e-3),
                          (0.01 / np.maximum(d1, d2)) ** (1 / 5))
            h_abs[ia] = np.minimum(np.minimum(np.minimum(100 * h0, h1), z_max), h_max)
        min_step = 10 * np.abs(np.nextafter(z, np.inf) - z)
        h_abs = np.where(h_abs > h_max, h_max, np.where(h_abs < min_step, min_step, h_abs))
        rejected = np.zeros(N, dtype=bool)
        while True:
            s1 = active & (h_abs < min_step)
            status[s1] = 1
            active &= ~s1
            s2 = active & (n_acc + n_rej >= max_steps)
            status[s2] = 2
            active &= ~s2
            ia = all_idx[active]
            if ia.size == 0:
                break
            t, ya, hh = z[ia], y[:, ia], h_abs[ia]
            t_new = t + hh
            t_new = np.where(t_new > z_max, z_max, t_new)
            h = t_new - t
            K = [f[:, ia]]
            for s in range(1, 6):
                K.append(rhs(t + C[s] * h, ya + _comb(K, A[s]) * h, ia))
            y_new = ya + h * _comb(K, B)
            K.append(rhs(t + h, y_new, ia))
            scale = atol + np.maximum(np.abs(ya), np.abs(y_new)) * rtol
            en = _norm(_comb(K, E) * h / scale)
            acc = en < 1
            fe = SAFETY * en ** ERR_EXP
            fac_acc = np.where(en == 0, MAX_FACTOR, np.where(fe < MAX_FACTOR, fe, MAX_FACTOR))
            fac_acc = np.where(rejected[ia] & ~(fac_acc < 1), 1.0, fac_acc)
            fac_rej = np.where(fe > MIN_FACTOR, fe, MIN_FACTOR)
            hh = np.abs(h) * np.where(acc, fac_acc, fac_rej)
            if traj is not None:
                for k in np.nonzero(acc)[0]:
                    i = ia[k]
                    Q = None
                    while next_row[i] <= n_out and t_eval[next_row[i]] <= t_new[k]:
                        if Q is None:
                            Q = np.stack([Kk[:, k] for Kk in K], axis=1).dot(P)   # K.T @ P
                        x = (t_eval[next_row[i]] - t[k]) / h[k]
                        p = np.cumprod(np.full(4, x))
                        traj[i, next_row[i]] = h[k] * np.dot(Q, p) + ya[:, k]
                        next_row[i] += 1
            if steps is not None and acc[ia == record].any():
                steps.append((float(t[ia == record][0]), float(h[ia == record][0])))
            ai = ia[acc]
            y[:, ai] = y_new[:, acc]
            f[:, ai] = K[6][:, acc]
            z[ai] = t_new[acc]
            n_acc[ai] += 1
            n_rej[ia[~acc]] += 1
            rejected[ia] = ~acc
            ps = np.abs(y[2, ai]) ** 2
            pm[ai] = np.where((ps > pm[ai]) | np.isnan(ps), ps, pm[ai])
            h_abs[ia] = hh
            fin = ai[z[ai] >= z_max]
            status[fin] = 0
            active[fin] = False
            ms = 10 * np.abs(np.nextafter(z[ai], np.inf) - z[ai])
            min_step[ai] = ms
            ha = h_abs[ai]
            h_abs[ai] = np.where(ha > h_max, h_max, np.where(ha < ms, ms, ha))
    return dict(a_end=y.T.copy(), p_end=np.abs(y[2]) ** 2, p_max=pm, status=status, z_end=z, n_accepted=n_acc,
                n_rejected=n_rej, traj=traj, steps=steps)
