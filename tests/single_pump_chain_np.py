"""NumPy restatements of a single-pump fibre chain (waves [p, s, i]), built on tests/single_pump_np.py: the yardstick of
tests/test_single_pump_chain_host.py and tests/test_gpu_single_pump_chain.py.

* ``direct``: classic RK4 of the accumulated-phase model in the physical (A) frame.  Span s on its local coordinate zeta has
  E = 2 gamma_s exp(i (Theta_s + dbeta_s zeta)), Theta_s = sum_{k<s} dbeta_k L_k; the transfers act on A.
* ``chain``: the same chain span by span through single_pump_np.integrate (each span the plain model with its own dbeta and
  local z) in the B frame, B_s = A_s e^{+i Theta_s}: a boundary is B' = T B with the signal also times e^{+i dbeta_s L_s}; rows
  are brought back to A with e^{-i Theta_s} on wave 1.  ``gauge=False`` leaves the boundary phase and the rotation out: the
  chain that forgot the gauge.

spans: (length, n_steps, dbeta, gamma, alpha) per span, the last three a scalar or (N,); transfers: S-1 entries (3,) or (N, 3).
"""
import numpy as np

import single_pump_np


def _points(a0, spans):
    sizes = {np.size(v) for sp in spans for v in sp[2:]} | ({np.shape(a0)[0]} if np.ndim(a0) == 2 else set())
    sizes.discard(1)
    assert len(sizes) <= 1
    return sizes.pop() if sizes else 1


def _per_point(x, N):
    return np.array(np.broadcast_to(np.asarray(x, dtype=float), (N,)))


def rhs_theta(theta, a, gamma, alpha):
    """dA/dz (N, 3) of the model with the FWM phase theta (N,) in place of dbeta * z."""
    g, al = gamma[:, None], alpha[:, None]
    P = a.real ** 2 + a.imag ** 2
    f = 2.0 * P.sum(axis=1, keepdims=True) - P
    E = 2.0 * gamma * np.exp(1j * theta)
    p, s, i = a[:, 0], a[:, 1], a[:, 2]
    D = 0.5 * np.conj(E) * p * p
    out = (-0.5 * al + 1j * g * f) * a
    out[:, 0] += 1j * np.conj(p) * E * s * i
    out[:, 1] += 1j * np.conj(i) * D
    out[:, 2] += 1j * np.conj(s) * D
    return out


def direct(a0, spans, transfers, save_every):
    """-> rows (N, n_saved_total, 3) in the A frame: every span's row 0 (the post-transfer state) and a row after every
    save_every-th step."""
    N = _points(a0, spans)
    y = np.array(np.broadcast_to(np.asarray(a0, dtype=np.complex128), (N, 3)))
    theta0 = np.zeros(N)
    rows = []
    for k, (L, n, db, g, al) in enumerate(spans):
        db, g, al = _per_point(db, N), _per_point(g, N), _per_point(al, N)
        zg = np.linspace(0.0, L, n + 1)
        rows.append(y.copy())
        for i in range(n):
            z, h = zg[i], zg[i + 1] - zg[i]
            k1 = rhs_theta(theta0 + db * z, y, g, al)
            k2 = rhs_theta(theta0 + db * (z + 0.5 * h), y + 0.5 * h * k1, g, al)
            k3 = rhs_theta(theta0 + db * (z + 0.5 * h), y + 0.5 * h * k2, g, al)
            k4 = rhs_theta(theta0 + db * (z + h), y + h * k3, g, al)
            y = y + (h / 6.0) * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
            if (i + 1) % save_every == 0:
                rows.append(y.copy())
        if k + 1 < len(spans):
            y = y * np.asarray(transfers[k], dtype=np.complex128)
            theta0 = theta0 + db * L
    return np.stack(rows, axis=1)


def chain(a0, spans, transfers, save_every, gauge=True):
    """-> dict(rows (N, n_saved_total, 3) A frame, a_end (N, 3), p_wave_end, p_wave_max (N, 3) over every saved row,
    first_bad_step (N,) counted over the whole chain (first failure wins), z_out (n_saved_total,))."""
    N = _points(a0, spans)
    b = np.array(np.broadcast_to(np.asarray(a0, dtype=np.complex128), (N, 3)))
    theta = np.zeros(N)
    bad = np.full(N, -1, dtype=np.int64)
    rows, z_out, z0, step0 = [], [], 0.0, 0
    for k, (L, n, db, g, al) in enumerate(spans):
        db = _per_point(db, N)
        r = single_pump_np.integrate(b, db, z_max=L, n=n, save_every=save_every, gamma=g, alpha=al, want_traj=True)
        A = r["traj"].copy()
        if gauge:
            A[:, :, 1] *= np.exp(-1j * theta)[:, None]
        rows.append(A)
        z_out.append(z0 + np.linspace(0.0, L, n + 1)[::save_every])
        new = (bad < 0) & (r["first_bad_step"] >= 0)
        bad[new] = r["first_bad_step"][new] + step0
        z0, step0 = z0 + L, step0 + n
        if k + 1 < len(spans):
            with np.errstate(all="ignore"):
                b = r["a_end"] * np.asarray(transfers[k], dtype=np.complex128)
                if gauge:
                    b[:, 1] *= np.exp(1j * db * L)
                    theta = theta + db * L
    rows = np.concatenate(rows, axis=1)
    with np.errstate(all="ignore"):
        p = np.abs(rows) ** 2
    return dict(rows=rows, a_end=rows[:, -1], p_wave_end=p[:, -1], p_wave_max=np.max(p, axis=1), first_bad_step=bad,
                z_out=np.concatenate(z_out))


def mid_stage(gain_db, phase):
    """sqrt(10^(gain_db/10)) e^{i phase}, written out here so the restatement does not lean on the package."""
    return np.sqrt(10.0 ** (np.asarray(gain_db, dtype=float) / 10.0)) * np.exp(1j * np.asarray(phase, dtype=float))


# ---- the two cases of the issue, shared between the CPU and the GPU tests -------------------------------------------------
def lossy_case(N, seed=11, steps=(600, 1000, 400), lengths=(300.0, 500.0, 200.0)):
    """3 lossy spans with per-point dbeta, gamma, alpha; one per-point and one broadcast transfer with gain and phase on every
    wave; pump 0.3-0.6 W, seeds 1e-7..1e-3 W."""
    rng = np.random.default_rng(seed)
    G, P = single_pump_np.GAMMA, single_pump_np.P_PUMP
    spans = [(L, n, rng.uniform(-4.5, 0.5, N) * G * P, G * rng.uniform(0.8, 1.6, N), 1.15e-4 * rng.uniform(0.5, 2.0, N))
             for L, n in zip(lengths, steps)]
    p = np.column_stack([rng.uniform(0.3, 0.6, N), 10 ** rng.uniform(-7, -3, N), 10 ** rng.uniform(-7, -3, N)])
    a0 = np.sqrt(p) * np.exp(1j * rng.uniform(-3, 3, (N, 3)))
    transfers = [mid_stage(rng.uniform(-3, 1, (N, 3)), rng.uniform(-np.pi, np.pi, (N, 3))),
                 mid_stage((-0.5, -2.0, 1.0), (0.7, -1.1, 2.3))]
    return a0, spans, transfers


def closed_form_case(K=16, steps=(150, 350)):
    """The copier - PSA closed form: alpha = 0, gamma = 0.0115, P = 0.5 W, a 1e-12 W seed, the idler dark; copier dbeta =
    -2 gamma P over 150 m, PSA dbeta = -2 gamma P over 300 m, 500 steps in all; the mid-stage rotates the pump by K uniform
    phases.  With mu = cosh gL + i (kappa/2g) sinh gL, nu = (gamma P/g) sinh gL, kappa = dbeta + 2 gamma P, g^2 = (gamma P)^2
    - (kappa/2)^2 the signal gain over the pump phase is a + b cos(2 phi + const): a = |mu_p mu_c|^2 + |nu_p nu_c|^2,
    b = 2 |mu_p nu_p mu_c nu_c|.  -> dict(...)."""
    G, P = single_pump_np.GAMMA, single_pump_np.P_PUMP

    def mu_nu(dbeta, L):
        kappa = dbeta + 2.0 * G * P
        g = np.sqrt(complex((G * P) ** 2 - (0.5 * kappa) ** 2))
        return np.cosh(g * L) + 1j * (kappa / (2.0 * g)) * np.sinh(g * L), (G * P / g) * np.sinh(g * L)

    copier, psa = (-2.0 * G * P, 150.0), (-2.0 * G * P, 300.0)
    (mc, nc), (mp, npsa) = mu_nu(*copier), mu_nu(*psa)
    a = abs(mp * mc) ** 2 + abs(npsa * nc) ** 2
    b = 2.0 * abs(mp * npsa * mc * nc)
    return dict(gamma=G, p_pump=P, p_seed=1e-12, a0=np.sqrt(np.array([P, 1e-12, 0.0])).astype(complex), copier=copier, psa=psa,
                steps=steps, phases=np.linspace(0.0, 2.0 * np.pi, K, endpoint=False), a=a, b=b)


def check_harmonics(gain, a, b):
    """gain (K,) linear over the K uniform pump phases -> (relative error of DFT bin 0 against a, of 2 |bin 2| against b, the
    largest other bin over bin 0)."""
    K = gain.size
    F = np.fft.rfft(gain) / K
    e0, e2 = abs(F[0].real / a - 1.0), abs(2.0 * abs(F[2]) / b - 1.0)
    rest = max(abs(F[j]) for j in range(1, F.size) if j != 2) / abs(F[0])
    return e0, e2, rest


def subset(case, idx):
    """(a0, spans, transfers) of lossy_case cut to the points ``idx``."""
    a0, spans, transfers = case
    return (a0[idx], [(L, n, db[idx], g[idx], al[idx]) for L, n, db, g, al in spans],
            [t[idx] if t.ndim == 2 else t for t in transfers])
