"""Batched NumPy restatement of the single-pump (degenerate) three-wave model: the yardstick of
tests/test_single_pump_host.py and tests/test_gpu_single_pump.py.  Independent of the kernel: complex arithmetic, np.exp at
every stage, the classic k1..k4 combination, no regrouping.

Waves [p, s, i]; with P_j = |A_j|^2, S = P_p + P_s + P_i, E(z) = 2 gamma exp(i dbeta z):

    dA_p/dz = (-alpha/2 + i gamma (2S - P_p)) A_p + i conj(A_p) E A_s A_i
    dA_s/dz = (-alpha/2 + i gamma (2S - P_s)) A_s + i conj(A_i) (conj(E)/2) A_p^2
    dA_i/dz = (-alpha/2 + i gamma (2S - P_i)) A_i + i conj(A_s) (conj(E)/2) A_p^2
"""
import functools

import numpy as np

GAMMA, LENGTH, P_PUMP = 0.0115, 1000.0, 0.5


def rhs(z, a, gamma, alpha, dbeta):
    """a (N, 3) complex, dbeta / gamma / alpha (N,) -> dA/dz (N, 3)."""
    a = np.asarray(a, dtype=np.complex128)
    g, al = np.asarray(gamma, dtype=float)[:, None], np.asarray(alpha, dtype=float)[:, None]
    P = a.real ** 2 + a.imag ** 2
    f = 2.0 * P.sum(axis=1, keepdims=True) - P
    E = 2.0 * g[:, 0] * np.exp(1j * np.asarray(dbeta, dtype=float) * z)
    p, s, i = a[:, 0], a[:, 1], a[:, 2]
    D = 0.5 * np.conj(E) * p * p
    out = (-0.5 * al + 1j * g * f) * a
    out[:, 0] += 1j * np.conj(p) * E * s * i
    out[:, 1] += 1j * np.conj(i) * D
    out[:, 2] += 1j * np.conj(s) * D
    return out


def integrate(a0, dbeta, *, z_max, n, save_every, gamma, alpha, want_traj=False):
    """Classic RK4 on np.linspace(0, z_max, n + 1) with the save-row rules of integrate_fixed_step (integrators.py:68-142):
    row 0 is z = 0, a row after every step i with (i + 1) % save_every == 0.  A point is tested after every step; the first
    step after which it is non-finite is its first_bad_step (-1: none), and it goes on being integrated (NaNs propagate).

    a0 (3,) or (N, 3); dbeta (N,); gamma / alpha scalar or (N,).
    -> dict(a_end (N, 3): the last saved row, p_wave_end, p_wave_max (N, 3): np.max over the saved rows, first_bad_step,
            traj (N, n_saved, 3) or None)."""
    dbeta = np.atleast_1d(np.asarray(dbeta, dtype=float))
    N = dbeta.shape[0]
    y = np.array(np.broadcast_to(np.asarray(a0, dtype=np.complex128), (N, 3)))
    gamma = np.broadcast_to(np.asarray(gamma, dtype=float), (N,))
    alpha = np.broadcast_to(np.asarray(alpha, dtype=float), (N,))
    zg = np.linspace(0.0, z_max, n + 1)
    bad = np.full(N, -1, dtype=np.int64)
    a_end = y.copy()
    p_max = np.abs(y) ** 2
    rows = [y.copy()]
    with np.errstate(all="ignore"):
        for i in range(n):
            z, h = zg[i], zg[i + 1] - zg[i]
            k1 = rhs(z, y, gamma, alpha, dbeta)
            k2 = rhs(z + 0.5 * h, y + 0.5 * h * k1, gamma, alpha, dbeta)
            k3 = rhs(z + 0.5 * h, y + 0.5 * h * k2, gamma, alpha, dbeta)
            k4 = rhs(z + h, y + h * k3, gamma, alpha, dbeta)
            y = y + (h / 6.0) * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
            newly = (bad < 0) & ~np.isfinite(y).all(axis=1)
            bad[newly] = i
            if (i + 1) % save_every == 0:
                a_end = y.copy()
                p_max = np.maximum(p_max, np.abs(y) ** 2)   # NaN-propagating, like np.max over the rows
                if want_traj:
                    rows.append(y.copy())
    return dict(a_end=a_end, p_wave_end=np.abs(a_end) ** 2, p_wave_max=p_max, first_bad_step=bad,
                traj=np.stack(rows, axis=1) if want_traj else None)


# ---- the closed-form case both test files tie to -------------------------------------------------------------------------
def analytic_gain(dbeta, gamma=GAMMA, p=P_PUMP, length=LENGTH):
    """Undepleted pump, alpha = 0: G = 1 + (gamma P / g)^2 sinh^2(g L), g^2 = (gamma P)^2 - (kappa/2)^2,
    kappa = dbeta + 2 gamma P (g imaginary outside the gain band: sinh becomes sin)."""
    kappa = np.asarray(dbeta, dtype=float) + 2.0 * gamma * p
    g = np.sqrt(((gamma * p) ** 2 - (0.5 * kappa) ** 2).astype(complex))
    return 1.0 + ((gamma * p / g) ** 2 * np.sinh(g * length) ** 2).real


@functools.lru_cache(maxsize=None)
def analytic_case():
    """The closed-form case of the issue, shared with the GPU test: 41 dbeta in [-4.8, 0.3] gamma P, a 1e-12 W seed."""
    dbeta = np.linspace(-4.8, 0.3, 41) * GAMMA * P_PUMP
    a0 = np.sqrt(np.array([P_PUMP, 1e-12, 0.0])).astype(complex)
    return dict(dbeta=dbeta, a0=a0, p_seed=1e-12, n=2000, z_max=LENGTH, gain=analytic_gain(dbeta))
