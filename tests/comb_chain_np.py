"""NumPy restatements of a multi-line ("frequency comb") fibre chain (M lines ascending in frequency, every FWM product among
them), built on tests/comb_np.py: the yardstick of tests/test_comb_chain_host.py and tests/test_gpu_comb_chain.py.

* ``direct``: classic RK4 of the accumulated-phase model in the physical (A) frame.  The field of line m is A_m e^{i Phi_m(z)};
  span s on its local coordinate zeta has Phi_m = Phi_{s,m} + kappa_{s,m} zeta, Phi_{s,m} = sum_{j<s} kappa_{j,m} L_j, and
  dA_m/dz = -alpha/2 A_m + i gamma conj(U_m) S_m(A o U) with U_m = np.exp(i Phi_m(z)) formed at every stage; the transfers act
  on A.
* ``chain``: the same chain span by span through comb_np.integrate (each span the plain model with its own kappa and local z)
  in the B frame, B_m = A_m e^{+i Phi_{s,m}} for EVERY line: a boundary is B'_m = T[m] B_m e^{+i kappa_{s,m} L_s}; rows are
  brought back to A with e^{-i Phi_{s,m}} on every line.  ``gauge=False`` leaves the boundary phase and the rotation out: the
  chain that forgot the gauge.

Both are the span loop of tests/chain_np.py over this module's MODEL: its span integrator, its accumulated-phase right-hand
side and the waves that carry the phase.

spans: (length, n_steps, kappa, gamma, alpha) per span, kappa (M,) or (N, M), gamma / alpha a scalar or (N,); transfers: S-1
entries (M,) or (N, M).
"""
import functools

import numpy as np

import chain_np
import comb_np

GAMMA = 0.0115          # 1/(W m)


def rhs_phi(phi, a, gamma, alpha):
    """dA/dz (N, M) of the model with the lines' phases phi (N, M) in place of kappa_m * z."""
    u = np.exp(1j * phi)
    return -0.5 * alpha[:, None] * a + 1j * gamma[:, None] * np.conj(u) * comb_np.pair_sum(a * u)


MODEL = chain_np.Model(integrate=functools.partial(comb_np.integrate, want_traj=True), rhs=rhs_phi, gauged=slice(None))
direct = functools.partial(chain_np.direct, MODEL)
chain = functools.partial(chain_np.chain, MODEL)
mid_stage, subset = chain_np.mid_stage, chain_np.subset


# ---- the cases of the issue, shared between the CPU and the GPU tests -----------------------------------------------------
def random_kappa(rng, N, M):
    """comb_np.random_inputs' propagation constants: (m-c)^2 U(-2e-3, 5e-4) + (m-c)^3 U(-1e-4, 1e-4) per point, c = (M-1)/2."""
    x = np.arange(M) - 0.5 * (M - 1)
    return x ** 2 * rng.uniform(-2e-3, 5e-4, (N, 1)) + x ** 3 * rng.uniform(-1e-4, 1e-4, (N, 1))


def random_a0(rng, N, M):
    """Line powers 10^U(-9, -3) W with lines 1 and M-2 at U(0.1, 0.2) W (M = 3: the one pump at U(0.2, 0.4) W), random phases."""
    p = 10 ** rng.uniform(-9, -3, (N, M))
    p[:, 1] = rng.uniform(0.1, 0.2, N)
    p[:, M - 2] = rng.uniform(0.1, 0.2, N) if M > 3 else rng.uniform(0.2, 0.4, N)
    return np.sqrt(p) * np.exp(1j * rng.uniform(-3, 3, (N, M)))


def lossy_case(N, M, seed=11, steps=(600, 1000, 400), lengths=(300.0, 500.0, 200.0)):
    """3 lossy spans with per-point kappa (N, M), gamma, alpha; one per-point and one broadcast transfer with gain and phase
    on every line.  kappa_m L reaches several radians on the outer lines of a wide comb, so a chain that forgets the gauge is
    off by order 1; gamma P L stays near 1-3 per span."""
    rng = np.random.default_rng(seed)
    spans = [(L, n, random_kappa(rng, N, M), GAMMA * rng.uniform(0.8, 1.6, N), 1.15e-4 * rng.uniform(0.5, 2.0, N))
             for L, n in zip(lengths, steps)]
    a0 = random_a0(rng, N, M)
    transfers = [mid_stage(rng.uniform(-3, 1, (N, M)), rng.uniform(-np.pi, np.pi, (N, M))),
                 mid_stage(rng.uniform(-2, 1, M), rng.uniform(-np.pi, np.pi, M))]
    return a0, spans, transfers


def split_fibre(rng, N, M, n_steps, length, pieces):
    """One lossy fibre (per-point kappa, gamma, alpha) and the same fibre cut into ``pieces`` spans of equal step counts where
    possible (multiples of 10 steps), joined by identity transfers -> (a0, kappa, gamma, alpha, spans)."""
    kp, a0 = random_kappa(rng, N, M), random_a0(rng, N, M)
    g, al = GAMMA * rng.uniform(0.9, 1.1, N), 1.15e-4 * rng.uniform(0.5, 1.5, N)
    cuts = np.round(np.linspace(0, n_steps // 10, pieces + 1)).astype(int) * 10
    spans = [(length * (b - a) / n_steps, int(b - a), kp, g, al) for a, b in zip(cuts[:-1], cuts[1:])]
    return a0, kp, g, al, spans


def from_single_pump(case, rng):
    """single_pump_chain_np's (a0, spans, transfers) on waves [p, s, i] -> the same chain on lines [s, p, i] = [0, 1, 2]: every
    span's dbeta split at random into kappa_0 + kappa_2 - 2 kappa_1 = dbeta (another split in every span)."""
    a0, spans, transfers = case
    order = [1, 0, 2]
    out = []
    for L, n, db, g, al in spans:
        db = np.atleast_1d(np.asarray(db, dtype=float))
        k0, k1 = rng.uniform(-0.01, 0.01, db.shape), rng.uniform(-0.01, 0.01, db.shape)
        out.append((L, n, np.stack([k0, k1, db - k0 + 2.0 * k1], axis=-1), g, al))
    return np.asarray(a0)[..., order], out, [np.asarray(t)[..., order] for t in transfers]


def failing_case(M=4):
    """5 points, two spans of 400 and 600 steps: span 2 has gamma = 300 at points 1 and 3, far past the RK4 stability edge, so
    the arithmetic overflows there within a few local steps (finite input); span 1 is healthy everywhere.
    -> (a0 (5, M), spans)."""
    n = 5
    rng = np.random.default_rng(2)
    kp = random_kappa(rng, n, M)
    gam2 = np.full(n, GAMMA)
    gam2[[1, 3]] = 300.0
    return random_a0(rng, n, M), [(40.0, 400, kp, GAMMA, 1e-4), (60.0, 600, kp, gam2, 0.0)]


def closed_form_case(F=16):
    """single_pump_chain_np.closed_form_case on lines [s, p, i] = [0, 1, 2]: alpha = 0, gamma = 0.0115, a 0.5 W pump, a 1e-12 W
    seed on line 0, line 2 dark; a 150 m copier and a 300 m PSA of 150 + 350 steps, both with kappa_0 + kappa_2 - 2 kappa_1 =
    -2 gamma P (kappa = [0, gamma P, 0]); the mid-stage rotates the pump by F uniform phases.  For the drivers the same fibre is
    beta2 alone around the centre line, beta2 dw^2 = -2 gamma P at dw = 2 pi 500 GHz.  a, b: the closed form's gain
    a + b cos(2 phi + const).  MEASURED: what the restatement itself leaves against the closed form at these step counts (3.01e-9
    on bin 0, 3.31e-9 on 2 |bin 2|, 1.74e-11 of bin 0 on every other bin: its step error and the neglected depletion), rounded
    up in the third digit and checked in tests/test_comb_chain_host.py; BARS: ten times that, the bars of the GPU test."""
    import single_pump_chain_np
    c = single_pump_chain_np.closed_form_case(F)
    G, P, dw = c["gamma"], c["p_pump"], 2.0 * np.pi * 500e9
    assert c["copier"][0] == c["psa"][0] == -2.0 * G * P
    return dict(gamma=G, p_pump=P, p_seed=c["p_seed"], a0=c["a0"][[1, 0, 2]], kappa=np.array([0.0, G * P, 0.0]),
                lengths=(c["copier"][1], c["psa"][1]), steps=c["steps"], phases=c["phases"], a=c["a"], b=c["b"],
                lambda_center_m=1550e-9, line_spacing=dw, beta2=-2.0 * G * P / dw ** 2, MEASURED=(3.02e-9, 3.32e-9, 1.75e-11), BARS=(3.02e-8, 3.32e-8, 1.75e-10))
