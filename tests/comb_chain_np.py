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

spans: (length, n_steps, kappa, gamma, alpha) per span, kappa (M,) or (N, M), gamma / alpha a scalar or (N,); transfers: S-1
entries (M,) or (N, M).
"""
import numpy as np

import comb_np

GAMMA = 0.0115          # 1/(W m)


def _points(a0, spans, transfers=()):
    sizes = {np.size(v) for sp in spans for v in sp[3:]} | {np.shape(x)[0] for x in [sp[2] for sp in spans] + list(transfers)
                                                            if np.ndim(x) == 2}
    if np.ndim(a0) == 2:
        sizes.add(np.shape(a0)[0])
    sizes.discard(1)
    assert len(sizes) <= 1
    return sizes.pop() if sizes else 1


def _per_point(x, N):
    return np.array(np.broadcast_to(np.asarray(x, dtype=float), (N,)))


def rhs_phi(phi, a, gamma, alpha):
    """dA/dz (N, M) of the model with the lines' phases phi (N, M) in place of kappa_m * z."""
    u = np.exp(1j * phi)
    return -0.5 * alpha[:, None] * a + 1j * gamma[:, None] * np.conj(u) * comb_np.pair_sum(a * u)


def direct(a0, spans, transfers, save_every):
    """-> rows (N, n_saved_total, M) in the A frame: every span's row 0 (the post-transfer state) and a row after every
    save_every-th step."""
    N = _points(a0, spans, transfers)
    M = np.shape(a0)[-1]
    y = np.array(np.broadcast_to(np.asarray(a0, dtype=np.complex128), (N, M)))
    phi0 = np.zeros((N, M))
    rows = []
    for k, (L, n, kp, g, al) in enumerate(spans):
        kp = np.array(np.broadcast_to(np.asarray(kp, dtype=float), (N, M)))
        g, al = _per_point(g, N), _per_point(al, N)
        zg = np.linspace(0.0, L, n + 1)
        rows.append(y.copy())
        for i in range(n):
            z, h = zg[i], zg[i + 1] - zg[i]
            k1 = rhs_phi(phi0 + kp * z, y, g, al)
            k2 = rhs_phi(phi0 + kp * (z + 0.5 * h), y + 0.5 * h * k1, g, al)
            k3 = rhs_phi(phi0 + kp * (z + 0.5 * h), y + 0.5 * h * k2, g, al)
            k4 = rhs_phi(phi0 + kp * (z + h), y + h * k3, g, al)
            y = y + (h / 6.0) * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
            if (i + 1) % save_every == 0:
                rows.append(y.copy())
        if k + 1 < len(spans):
            y = y * np.asarray(transfers[k], dtype=np.complex128)
            phi0 = phi0 + kp * L
    return np.stack(rows, axis=1)


def chain(a0, spans, transfers, save_every, gauge=True):
    """-> dict(rows (N, n_saved_total, M) A frame, a_end (N, M), p_wave_end, p_wave_max (N, M) over every saved row,
    first_bad_step (N,) counted over the whole chain (first failure wins), z_out (n_saved_total,))."""
    N = _points(a0, spans, transfers)
    M = np.shape(a0)[-1]
    b = np.array(np.broadcast_to(np.asarray(a0, dtype=np.complex128), (N, M)))
    phi = np.zeros((N, M))
    bad = np.full(N, -1, dtype=np.int64)
    rows, z_out, z0, step0 = [], [], 0.0, 0
    for k, (L, n, kp, g, al) in enumerate(spans):
        kp = np.array(np.broadcast_to(np.asarray(kp, dtype=float), (N, M)))
        r = comb_np.integrate(b, kp, z_max=L, n=n, save_every=save_every, gamma=g, alpha=al, want_traj=True)
        A = r["traj"].copy()
        with np.errstate(all="ignore"):
            if gauge:
                A *= np.exp(-1j * phi)[:, None, :]
            rows.append(A)
            z_out.append(z0 + np.linspace(0.0, L, n + 1)[::save_every])
            new = (bad < 0) & (r["first_bad_step"] >= 0)
            bad[new] = r["first_bad_step"][new] + step0
            z0, step0 = z0 + L, step0 + n
            if k + 1 < len(spans):
                b = r["a_end"] * np.asarray(transfers[k], dtype=np.complex128)
                if gauge:
                    b = b * np.exp(1j * kp * L)
                    phi = phi + kp * L
    rows = np.concatenate(rows, axis=1)
    with np.errstate(all="ignore"):
        p = np.abs(rows) ** 2
    return dict(rows=rows, a_end=rows[:, -1], p_wave_end=p[:, -1], p_wave_max=np.max(p, axis=1), first_bad_step=bad,
                z_out=np.concatenate(z_out))


def mid_stage(gain_db, phase):
    """sqrt(10^(gain_db/10)) e^{i phase}, written out here so the restatement does not lean on the package."""
    return np.sqrt(10.0 ** (np.asarray(gain_db, dtype=float) / 10.0)) * np.exp(1j * np.asarray(phase, dtype=float))


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


def subset(case, idx):
    """(a0, spans, transfers) of lossy_case cut to the points ``idx``."""
    a0, spans, transfers = case
    return (a0[idx], [(L, n, kp[idx], g[idx], al[idx]) for L, n, kp, g, al in spans],
            [t[idx] if t.ndim == 2 else t for t in transfers])


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
