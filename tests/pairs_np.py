"""Batched NumPy restatement of the multi-channel model (two pumps and K signal/idler pairs): the yardstick of
tests/test_pairs_host.py and tests/test_gpu_pairs.py.  Independent of the kernel: complex arithmetic, np.exp at every
stage, the classic k1..k4 combination, no regrouping.

Waves [p1, p2, s_1, i_1, ..., s_K, i_K]; with P_j = |A_j|^2, S = sum_j P_j, E_k(z) = 2 gamma exp(i dbeta_k z):

    dA_p1/dz = (-alpha/2 + i gamma (2S - P_p1)) A_p1 + i conj(A_p2) sum_k E_k A_sk A_ik        (p2: p1 <-> p2)
    dA_sk/dz = (-alpha/2 + i gamma (2S - P_sk)) A_sk + i conj(A_ik) conj(E_k) A_p1 A_p2        (ik: sk <-> ik)

FWM products between channels are not modelled."""
import numpy as np


def rhs(z, a, gamma, alpha, dbeta):
    """a (N, NW) complex, dbeta (N, K), gamma / alpha (N,) -> dA/dz (N, NW)."""
    a = np.asarray(a, dtype=np.complex128)
    g, al = np.asarray(gamma, dtype=float)[:, None], np.asarray(alpha, dtype=float)[:, None]
    P = a.real ** 2 + a.imag ** 2
    f = 2.0 * P.sum(axis=1, keepdims=True) - P
    E = 2.0 * g * np.exp(1j * np.asarray(dbeta, dtype=float) * z)
    s, i = a[:, 2::2], a[:, 3::2]
    F = (E * s * i).sum(axis=1)
    D = np.conj(E) * (a[:, 0] * a[:, 1])[:, None]
    out = (-0.5 * al + 1j * g * f) * a
    out[:, 0] += 1j * np.conj(a[:, 1]) * F
    out[:, 1] += 1j * np.conj(a[:, 0]) * F
    out[:, 2::2] += 1j * np.conj(i) * D
    out[:, 3::2] += 1j * np.conj(s) * D
    return out


def integrate(a0, dbeta, *, z_max, n, save_every, gamma, alpha):
    """Classic RK4 on np.linspace(0, z_max, n + 1) with the save-row rules of integrate_fixed_step (integrators.py:68-142):
    row 0 is z = 0, a row after every step i with (i + 1) % save_every == 0.  A point is tested after every step; the first
    step after which it is non-finite is its first_bad_step (-1: none), and it goes on being integrated (NaNs propagate).

    a0 (NW,) or (N, NW); dbeta (N, K); gamma / alpha scalar or (N,).
    -> dict(a_end (N, NW): the last saved row, p_wave_end, p_wave_max (N, NW): np.max over the saved rows, first_bad_step)."""
    dbeta = np.asarray(dbeta, dtype=float)
    N, K = dbeta.shape
    y = np.array(np.broadcast_to(np.asarray(a0, dtype=np.complex128), (N, 2 + 2 * K)))
    gamma = np.broadcast_to(np.asarray(gamma, dtype=float), (N,))
    alpha = np.broadcast_to(np.asarray(alpha, dtype=float), (N,))
    zg = np.linspace(0.0, z_max, n + 1)
    bad = np.full(N, -1, dtype=np.int64)
    a_end = y.copy()
    p_max = np.abs(y) ** 2
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
    return dict(a_end=a_end, p_wave_end=np.abs(a_end) ** 2, p_wave_max=p_max, first_bad_step=bad)
