"""NumPy restatements of a single-pump fibre chain (waves [p, s, i]), built on tests/single_pump_np.py: the yardstick of
tests/test_single_pump_chain_host.py and tests/test_gpu_single_pump_chain.py.

* ``direct``: classic RK4 of the accumulated-phase model in the physical (A) frame.  Span s on its local coordinate zeta has
  E = 2 gamma_s exp(i (Theta_s + dbeta_s zeta)), Theta_s = sum_{k<s} dbeta_k L_k; the transfers act on A.
* ``chain``: the same chain span by span through single_pump_np.integrate (each span the plain model with its own dbeta and
  local z) in the B frame, B_s = A_s e^{+i Theta_s}: a boundary is B' = T B with the signal also times e^{+i dbeta_s L_s}; rows
  are brought back to A with e^{-i Theta_s} on wave 1.  ``gauge=False`` leaves the boundary phase and the rotation out: the
  chain that forgot the gauge.

Both are the span loop of tests/chain_np.py over this module's MODEL: its span integrator, its accumulated-phase right-hand
side and the waves that carry the phase.

spans: (length, n_steps, dbeta, gamma, alpha) per span, the last three a scalar or (N,); transfers: S-1 entries (3,) or (N, 3).
"""
import functools

import numpy as np

import chain_np
import single_pump_np


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


MODEL = chain_np.Model(integrate=functools.partial(single_pump_np.integrate, want_traj=True), rhs=rhs_theta, gauged=1)
direct = functools.partial(chain_np.direct, MODEL)
chain = functools.partial(chain_np.chain, MODEL)
mid_stage, subset = chain_np.mid_stage, chain_np.subset


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
