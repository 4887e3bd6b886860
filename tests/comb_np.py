"""Batched NumPy restatement of the CW multi-line ("frequency comb") model: the yardstick of tests/test_comb_host.py and
tests/test_gpu_comb.py.  Independent of the kernel: complex arithmetic, np.exp at every stage, the classic k1..k4
combination, no regrouping, no carried phase.

Lines m = 0..M-1 ascending in frequency, field A_m e^{i kappa_m z}; with u_m(z) = exp(i kappa_m z) and B_m = A_m u_m

    S_m     = sum over every ordered triple k + l - n = m (all indices inside 0..M-1) of B_k B_l conj(B_n)
    dA_m/dz = -alpha/2 A_m + i gamma conj(u_m) S_m

``triple_sum`` is that definition, term by term; ``pair_sum`` is the O(M^2) form through the autocorrelation
C_d = sum_n B_{n+d} conj(B_n), S_m = sum_l B_l C_{m-l}.  Both add their terms one after the other in ascending index order
(a Python loop over the summation index, NumPy over the points), so a dark line only ever contributes exact zeros: a run
with dark odd lines repeats the run of the bright lines alone bit for bit.
"""
import numpy as np


def triple_sum(B):
    """B (N, M) complex -> S (N, M): the definition, one product per ordered triple."""
    N, M = B.shape
    S = np.zeros((N, M), dtype=np.complex128)
    for k in range(M):
        for l in range(M):
            for n in range(M):
                m = k + l - n
                if 0 <= m < M:
                    S[:, m] += B[:, k] * B[:, l] * np.conj(B[:, n])
    return S


def pair_sum(B):
    """B (N, M) complex -> S (N, M) through C_d, d = -(M-1)..M-1, held at column d + M - 1."""
    N, M = B.shape
    C = np.zeros((N, 2 * M - 1), dtype=np.complex128)
    for n in range(M):                       # C_d += B_{n+d} conj(B_n) for every d with 0 <= n + d < M
        C[:, M - 1 - n:2 * M - 1 - n] += B * np.conj(B[:, n:n + 1])
    S = np.zeros((N, M), dtype=np.complex128)
    for l in range(M):                       # S_m += B_l C_{m-l} for every m
        S += B[:, l:l + 1] * C[:, M - 1 - l:2 * M - 1 - l]
    return S


def rhs(z, a, gamma, alpha, kappa, sum_form=pair_sum):
    """a, kappa (N, M), gamma / alpha (N,) -> dA/dz (N, M)."""
    a = np.asarray(a, dtype=np.complex128)
    u = np.exp(1j * np.asarray(kappa, dtype=float) * z)
    g, al = np.asarray(gamma, dtype=float)[:, None], np.asarray(alpha, dtype=float)[:, None]
    return -0.5 * al * a + 1j * g * np.conj(u) * sum_form(a * u)


def integrate(a0, kappa, *, z_max, n, save_every, gamma, alpha, want_traj=False, sum_form=pair_sum):
    """Classic RK4 on np.linspace(0, z_max, n + 1) with the save-row rules of integrate_fixed_step (integrators.py:68-142):
    row 0 is z = 0, a row after every step i with (i + 1) % save_every == 0.  A point is tested after every step; the first
    step after which it is non-finite is its first_bad_step (-1: none), and it goes on being integrated (NaNs propagate).

    a0 (M,) or (N, M); kappa (N, M); gamma / alpha scalar or (N,).
    -> dict(a_end (N, M): the last saved row, p_wave_end, p_wave_max (N, M): np.max over the saved rows, first_bad_step,
            traj (N, n_saved, M) or None)."""
    kappa = np.atleast_2d(np.asarray(kappa, dtype=float))
    N, M = kappa.shape
    y = np.array(np.broadcast_to(np.asarray(a0, dtype=np.complex128), (N, M)))
    gamma = np.broadcast_to(np.asarray(gamma, dtype=float), (N,))
    alpha = np.broadcast_to(np.asarray(alpha, dtype=float), (N,))
    zg = np.linspace(0.0, z_max, n + 1)
    bad = np.full(N, -1, dtype=np.int64)
    a_end = y.copy()
    p_max = np.abs(y) ** 2
    rows = [y.copy()]
    f = lambda z, a: rhs(z, a, gamma, alpha, kappa, sum_form)   # noqa: E731
    with np.errstate(all="ignore"):
        for i in range(n):
            z, h = zg[i], zg[i + 1] - zg[i]
            k1 = f(z, y)
            k2 = f(z + 0.5 * h, y + 0.5 * h * k1)
            k3 = f(z + 0.5 * h, y + 0.5 * h * k2)
            k4 = f(z + h, y + h * k3)
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


def random_inputs(N, M, seed, per_point=True, lossy=True):
    """The inputs of the GPU tests: kappa_m = (m-c)^2 U(-2e-3, 5e-4) + (m-c)^3 U(-1e-4, 1e-4) per point, c = (M-1)/2; line
    powers 10^U(-9, -3) W with lines 1 and M-2 at U(0.2, 0.4) W; random phases; gamma = 0.0115 U(0.9, 1.1), alpha =
    1.15e-4 U(0.5, 1.5) (0 where not lossy).  Broadcast: one a0, gamma and alpha for every point."""
    rng = np.random.default_rng(seed)
    x = np.arange(M) - 0.5 * (M - 1)
    kappa = x ** 2 * rng.uniform(-2e-3, 5e-4, (N, 1)) + x ** 3 * rng.uniform(-1e-4, 1e-4, (N, 1))
    n0 = N if per_point else 1
    p = 10 ** rng.uniform(-9, -3, (n0, M))
    p[:, 1] = rng.uniform(0.2, 0.4, n0)
    p[:, M - 2] = rng.uniform(0.2, 0.4, n0)
    a0 = np.sqrt(p) * np.exp(1j * rng.uniform(-3, 3, (n0, M)))
    gamma = 0.0115 * rng.uniform(0.9, 1.1, n0)
    alpha = 1.15e-4 * rng.uniform(0.5, 1.5, n0) if lossy else np.zeros(n0)
    if not per_point:
        a0, gamma, alpha = a0[0], float(gamma[0]), float(alpha[0])
    return kappa, a0, gamma, alpha
