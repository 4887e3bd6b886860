"""NumPy restatements of a multi-channel fibre chain (two pumps and K signal/idler pairs, waves [p1, p2, s_1, i_1, ..., s_K,
i_K]), built on tests/pairs_np.py: the yardstick of tests/test_pairs_chain_host.py and tests/test_gpu_pairs_chain.py.

* ``integrate``: pairs_np.integrate (the same right-hand side, the same classic RK4, the same save and NaN rules) that also
  returns the saved rows.
* ``direct``: classic RK4 of the accumulated-phase model in the physical (A) frame.  Span s on its local coordinate zeta has
  E_k = 2 gamma_s exp(i (Theta_{s,k} + dbeta_{s,k} zeta)), Theta_{s,k} = sum_{j<s} dbeta_{j,k} L_j; the transfers act on A.
* ``chain``: the same chain span by span through ``integrate`` (each span the plain model with its own dbeta and local z) in
  the B frame, B_sk = A_sk e^{+i Theta_{s,k}}: a boundary is B' = T B with signal k also times e^{+i dbeta_{s,k} L_s}; rows are
  brought back to A with e^{-i Theta_{s,k}} on wave 2 + 2k.  ``gauge=False`` leaves the boundary phase and the rotation out:
  the chain that forgot the gauge.

Both are the span loop of tests/chain_np.py over this module's MODEL: its span integrator, its accumulated-phase right-hand
side and the waves that carry the phase.

spans: (length, n_steps, dbeta, gamma, alpha) per span, dbeta (K,) or (N, K), gamma / alpha a scalar or (N,); transfers: S-1
entries (NW,) or (N, NW).
"""
import functools

import numpy as np

import chain_np
import pairs_np

GAMMA, P_PUMP = 0.0115, 0.25          # 1/(W m); each of the two pumps, W


def integrate(a0, dbeta, *, z_max, n, save_every, gamma, alpha):
    """pairs_np.integrate with the saved rows: -> its dict and traj (N, n // save_every + 1, NW), row 0 the state at z = 0."""
    dbeta = np.asarray(dbeta, dtype=float)
    N, K = dbeta.shape
    y = np.array(np.broadcast_to(np.asarray(a0, dtype=np.complex128), (N, 2 + 2 * K)))
    gamma, alpha = chain_np._per_point(gamma, N), chain_np._per_point(alpha, N)
    zg = np.linspace(0.0, z_max, n + 1)
    bad = np.full(N, -1, dtype=np.int64)
    rows = [y.copy()]
    with np.errstate(all="ignore"):
        for i in range(n):
            z, h = zg[i], zg[i + 1] - zg[i]
            k1 = pairs_np.rhs(z, y, gamma, alpha, dbeta)
            k2 = pairs_np.rhs(z + 0.5 * h, y + 0.5 * h * k1, gamma, alpha, dbeta)
            k3 = pairs_np.rhs(z + 0.5 * h, y + 0.5 * h * k2, gamma, alpha, dbeta)
            k4 = pairs_np.rhs(z + h, y + h * k3, gamma, alpha, dbeta)
            y = y + (h / 6.0) * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
            newly = (bad < 0) & ~np.isfinite(y).all(axis=1)
            bad[newly] = i
            if (i + 1) % save_every == 0:
                rows.append(y.copy())
        traj = np.stack(rows, axis=1)
        p = np.abs(traj) ** 2
    return dict(a_end=traj[:, -1], p_wave_end=p[:, -1], p_wave_max=np.max(p, axis=1), first_bad_step=bad, traj=traj)


def rhs_theta(theta, a, gamma, alpha):
    """dA/dz (N, NW) of the model with the FWM phases theta (N, K) in place of dbeta_k * z."""
    g, al = gamma[:, None], alpha[:, None]
    P = a.real ** 2 + a.imag ** 2
    f = 2.0 * P.sum(axis=1, keepdims=True) - P
    E = 2.0 * g * np.exp(1j * theta)
    s, i = a[:, 2::2], a[:, 3::2]
    F = (E * s * i).sum(axis=1)
    D = np.conj(E) * (a[:, 0] * a[:, 1])[:, None]
    out = (-0.5 * al + 1j * g * f) * a
    out[:, 0] += 1j * np.conj(a[:, 1]) * F
    out[:, 1] += 1j * np.conj(a[:, 0]) * F
    out[:, 2::2] += 1j * np.conj(i) * D
    out[:, 3::2] += 1j * np.conj(s) * D
    return out


MODEL = chain_np.Model(integrate=integrate, rhs=rhs_theta, gauged=slice(2, None, 2))
direct = functools.partial(chain_np.direct, MODEL)
chain = functools.partial(chain_np.chain, MODEL)
mid_stage, subset = chain_np.mid_stage, chain_np.subset


# ---- the cases of the issue, shared between the CPU and the GPU tests -----------------------------------------------------
def random_a0(rng, N, K):
    """Pumps 0.15-0.3 W each, every seed and idler 1e-7..1e-3 W, every phase random."""
    p = np.concatenate([rng.uniform(0.15, 0.3, (N, 2)), 10 ** rng.uniform(-7, -3, (N, 2 * K))], axis=1)
    return np.sqrt(p) * np.exp(1j * rng.uniform(-3, 3, (N, 2 + 2 * K)))


def lossy_case(N, K, seed=11, steps=(600, 1000, 400), lengths=(300.0, 500.0, 200.0)):
    """3 lossy spans with per-point dbeta (N, K), gamma, alpha; one per-point and one broadcast transfer with gain and phase
    on every wave.  gamma (P1 + P2) L stays near 2-4 per span, the mismatches around the phase-matched -gamma (P1 + P2)."""
    rng = np.random.default_rng(seed)
    nw = 2 + 2 * K
    spans = [(L, n, rng.uniform(-3.5, 1.5, (N, K)) * GAMMA * 2 * P_PUMP, GAMMA * rng.uniform(0.8, 1.6, N),
              1.15e-4 * rng.uniform(0.5, 2.0, N)) for L, n in zip(lengths, steps)]
    a0 = random_a0(rng, N, K)
    transfers = [mid_stage(rng.uniform(-3, 1, (N, nw)), rng.uniform(-np.pi, np.pi, (N, nw))),
                 mid_stage(rng.uniform(-2, 1, nw), rng.uniform(-np.pi, np.pi, nw))]
    return a0, spans, transfers


def mu_nu(dbeta, L, gamma, p1, p2):
    """The dual-pump parametric amplifier with undepleted pumps: a_s(L) = mu a_s(0) + nu conj(a_i(0)) up to common phases,
    mu = cosh gL + i (kappa/2g) sinh gL, |nu| = (2 gamma sqrt(P1 P2)/g) sinh gL, kappa = dbeta + gamma (P1 + P2),
    g^2 = 4 gamma^2 P1 P2 - (kappa/2)^2 (g imaginary: the same expressions, oscillating).  -> (mu, |nu|), arrays over dbeta."""
    kappa = np.asarray(dbeta, dtype=float) + gamma * (p1 + p2)
    r = 2.0 * gamma * np.sqrt(p1 * p2)
    g = np.sqrt((r * r - (0.5 * kappa) ** 2).astype(complex))
    return np.cosh(g * L) + 1j * (kappa / (2.0 * g)) * np.sinh(g * L), np.abs((r / g) * np.sinh(g * L))


def closed_form_gain(db_copier, L_copier, db_psa, L_psa, gamma, p1, p2):
    """The signal gain of channel k of a lossless copier - PSA link (dark idlers in, both pumps rotated by phi in between) is
    a_k + b_k cos(2 phi + const): a = |mu_p mu_c|^2 + |nu_p nu_c|^2, b = 2 |mu_p nu_p mu_c nu_c|.  -> (a (K,), b (K,))."""
    (mc, nc), (mp, npsa) = mu_nu(db_copier, L_copier, gamma, p1, p2), mu_nu(db_psa, L_psa, gamma, p1, p2)
    return np.abs(mp * mc) ** 2 + (npsa * nc) ** 2, 2.0 * np.abs(mp * mc) * npsa * nc


def check_harmonics(gain, a, b):
    """gain (F,) linear over F uniform pump phases -> (relative error of DFT bin 0 against a, of 2 |bin 2| against b, the
    largest other bin over bin 0), as single_pump_chain_np.check_harmonics."""
    F = np.fft.rfft(gain) / gain.size
    e0, e2 = abs(F[0].real / a - 1.0), abs(2.0 * abs(F[2]) / b - 1.0)
    rest = max(abs(F[j]) for j in range(1, F.size) if j != 2) / abs(F[0])
    return e0, e2, rest


def wdm_case(steps=(150, 350)):
    """The WDM copier - PSA closed-form case: K = 4 channels on pumps at 1540 and 1560 nm (0.25 W each), one fibre type
    (gamma 0.0115 /W/m, alpha = 0, a dispersion-shifted beta2 / beta3 / beta4 around 1553 nm) for a 150 m copier and a 300 m
    PSA, 1e-12 W seeds, dark idlers, F = 16 uniform pump phases; the detunings put dbeta_k between -2.6 and -0.2 times
    gamma (P1 + P2), inside the gain band.  BAR_BIN / BAR_REST: ten times what the restatement itself leaves against the
    closed form at these step counts (7.06e-9 on bins 0 and 2, 5.9e-11 of bin 0 on every other bin: its step error and the
    neglected depletion), checked in tests/test_pairs_chain_host.py."""
    c = 299792458.0
    w1, w2 = 2.0 * np.pi * c / 1540e-9, 2.0 * np.pi * c / 1560e-9
    return dict(lambda_p1_m=1540e-9, lambda_p2_m=1560e-9, Omega=np.array([1.1, 1.2, 1.35, 1.5]) * 0.5 * (w1 - w2),
                disp=dict(omega_ref=1.21291603e15, beta2=-1.92057096e-28, beta3=3.31041782e-41, beta4=-1.62191731e-55),
                gamma=GAMMA, p_pump=P_PUMP, p_seed=1e-12, lengths=(150.0, 300.0), steps=steps,
                phases=np.linspace(0.0, 2.0 * np.pi, 16, endpoint=False), BAR_BIN=7.1e-8, BAR_REST=5.9e-10)


def failing_case(K=3):
    """5 points, two spans of 400 and 600 steps: span 2 has gamma = 300 at points 1 and 3, far past the RK4 stability edge, so
    the arithmetic overflows there at local step 1 (finite input, non-finite after two steps); span 1 is healthy everywhere.
    -> (a0 (5, NW), spans)."""
    n = 5
    rng = np.random.default_rng(2)
    db = np.linspace(-0.02, 0.02, n)[:, None] * np.linspace(0.5, 1.5, K)[None, :]
    gam2 = np.full(n, GAMMA)
    gam2[[1, 3]] = 300.0
    a0 = np.sqrt(np.array([P_PUMP, P_PUMP] + [1e-5, 1e-6] * K)) * np.exp(1j * rng.uniform(-3, 3, (n, 2 + 2 * K)))
    return a0, [(40.0, 400, db, GAMMA, 1e-4), (60.0, 600, db, gam2, 0.0)]
