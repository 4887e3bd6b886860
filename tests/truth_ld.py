"""The 80-bit yardstick: classic RK4 of every sweep model in np.longdouble / np.clongdouble (x87 extended, eps 1.1e-19), the
fixed point of tests/test_truth_host.py and tests/test_gpu_truth.py.

It is the SAME discrete scheme as the kernels and their float64 twins (k1..k4 on the grid z_i = i h, h = z_max / n), so the
step-size error cancels in a comparison and what is left is each implementation's rounding, measured 2 000 times finer than
float64 resolves.  Nothing here is shared with a twin and nothing is clever: the phase is cos / sin of the longdouble product
at every stage, no carried phase, no regrouping, no fused operations.

Each right-hand side is written from the model's equations (kernel headers) with the FWM phase as an
argument, so that a span of a chain -- phase Theta_s + dbeta_s (z - z_s) -- and a plain sweep -- phase dbeta z -- are one
function.  Batched over the points: states (N, NW), parameters (N,).

    four / six waves [p1, p2, s1, i1(, s2, i2)]  (yaman_model conventions)
        dA_j/dz = -alpha/2 A_j + i gamma (P_j + 2 sum_{k != j} P_k) A_j + 2 i gamma M_j
        M_p1 = conj(A_p2) sum_c A_sc A_ic e^{+i th_c}    M_sc = conj(A_ic) A_p1 A_p2 e^{-i th_c}    (p2, ic: partners swapped)
    K pairs [p1, p2, s_1, i_1, ..., s_K, i_K], E_k = 2 gamma e^{i th_k}, S = sum_j P_j  (psa_rk4_pairs_kernel.inc.h)
        dA_p1/dz = (-alpha/2 + i gamma (2S - P_p1)) A_p1 + i conj(A_p2) sum_k E_k A_sk A_ik          (p2: p1 <-> p2)
        dA_sk/dz = (-alpha/2 + i gamma (2S - P_sk)) A_sk + i conj(A_ik) conj(E_k) A_p1 A_p2          (ik: sk <-> ik)
    single pump [p, s, i]
        dA_p/dz = (-alpha/2 + i gamma (2S - P_p)) A_p + 2 i gamma conj(A_p) A_s A_i e^{+i th}
        dA_s/dz = (-alpha/2 + i gamma (2S - P_s)) A_s +   i gamma conj(A_i) A_p^2 e^{-i th}          (i: s <-> i)
    M-line comb, B_m = A_m e^{i kappa_m z}
        dA_m/dz = -alpha/2 A_m + i gamma e^{-i kappa_m z} sum_{k + l - n = m} B_k B_l conj(B_n)

Rows follow integrate_fixed_step: row 0 at z = 0, a row after every step with (i + 1) % save_every == 0; a_end is the last
saved row, p_wave_max the maximum over the saved rows.
"""
import numpy as np

LD, CLD = np.longdouble, np.clongdouble

assert np.finfo(LD).nmant >= 63, (
    f"np.longdouble has a {np.finfo(LD).nmant}-bit mantissa here: the yardstick needs x87 extended precision (>= 63 bits) "
    "and means nothing in float64")

I = CLD(1j)


def ld(x):
    return np.asarray(x, dtype=LD)


def cld(x):
    return np.asarray(x, dtype=CLD)


def expi(theta):
    """exp(i theta) from cos and sin of the longdouble phase."""
    theta = ld(theta)
    out = np.empty(theta.shape, dtype=CLD)
    out.real = np.cos(theta)
    out.imag = np.sin(theta)
    return out


def power(a):
    return a.real * a.real + a.imag * a.imag


# ---- right-hand sides: f(theta, a, gamma, alpha), theta the FWM phase(s) of this stage -------------------------------------
def rhs_waves(theta, a, gamma, alpha):
    """Two pumps and K = 1 (four waves), 2 (six waves) or more pairs: a (N, 2 + 2K), theta (N, K), gamma / alpha (N,)."""
    g, al = gamma[:, None], alpha[:, None]
    P = power(a)
    total = P.sum(axis=1, keepdims=True)
    kerr = P + LD(2) * (total - P)
    p1, p2 = a[:, 0:1], a[:, 1:2]
    s, i = a[:, 2::2], a[:, 3::2]
    e = expi(theta)
    mix = (s * i * e).sum(axis=1, keepdims=True)          # sum_c A_sc A_ic e^{+i th_c}
    down = p1 * p2 * np.conj(e)                           # A_p1 A_p2 e^{-i th_c}, one column per channel
    M = np.empty_like(a)
    M[:, 0:1] = np.conj(p2) * mix
    M[:, 1:2] = np.conj(p1) * mix
    M[:, 2::2] = np.conj(i) * down
    M[:, 3::2] = np.conj(s) * down
    return -(al / LD(2)) * a + I * g * kerr * a + LD(2) * I * g * M


def rhs_pairs(theta, a, gamma, alpha):
    """The multi-channel model as psa_rk4_pairs_kernel.inc.h states it, E_k = 2 gamma e^{i th_k}: a (N, 2 + 2K), theta (N, K)."""
    g, al = gamma[:, None], alpha[:, None]
    P = power(a)
    S = P.sum(axis=1, keepdims=True)
    E = LD(2) * g * expi(theta)
    F = (E * a[:, 2::2] * a[:, 3::2]).sum(axis=1, keepdims=True)
    D = np.conj(E) * (a[:, 0:1] * a[:, 1:2])
    out = (-(al / LD(2)) + I * g * (LD(2) * S - P)) * a
    out[:, 0:1] += I * np.conj(a[:, 1:2]) * F
    out[:, 1:2] += I * np.conj(a[:, 0:1]) * F
    out[:, 2::2] += I * np.conj(a[:, 3::2]) * D
    out[:, 3::2] += I * np.conj(a[:, 2::2]) * D
    return out


def rhs_single_pump(theta, a, gamma, alpha):
    """One pump, a signal and an idler at 2 w_p - w_s: a (N, 3), theta (N, 1) or (N,)."""
    g, al = gamma[:, None], alpha[:, None]
    P = power(a)
    kerr = LD(2) * P.sum(axis=1, keepdims=True) - P
    e = expi(np.reshape(theta, (a.shape[0], 1)))
    p, s, i = a[:, 0:1], a[:, 1:2], a[:, 2:3]
    M = np.empty_like(a)
    M[:, 0:1] = LD(2) * np.conj(p) * s * i * e
    M[:, 1:2] = np.conj(i) * p * p * np.conj(e)
    M[:, 2:3] = np.conj(s) * p * p * np.conj(e)
    return -(al / LD(2)) * a + I * g * kerr * a + I * g * M


_TRIPLES = {}


def _triples(M):
    """Every product B_k B_l conj(B_n) with k + l - n = m inside 0..M-1, taken once for k <= l (weight 2 where k < l: the
    ordered triples (k, l, n) and (l, k, n) are one product), sorted by m.
    -> (k, l, weight of the distinct pairs k <= l; per triple: its pair, its n; the first triple of each m)."""
    if M not in _TRIPLES:
        pairs = [(k, l) for k in range(M) for l in range(k, M)]
        t = sorted((k + l - n, j, n) for j, (k, l) in enumerate(pairs) for n in range(M) if 0 <= k + l - n < M)
        m, pair, n = (np.array(c) for c in zip(*t))
        k, l = (np.array(c) for c in zip(*pairs))
        _TRIPLES[M] = (k, l, ld(np.where(k < l, 2, 1))[:, None], pair, n, np.searchsorted(m, np.arange(M)))
    return _TRIPLES[M]


def rhs_comb(theta, a, gamma, alpha):
    """M equally spaced lines: a, theta = kappa z (N, M).  One term per triple, added in ascending (k, l, n) for each m; the
    lines lead inside (B is transposed) only because gathering whole rows is the fast way to index in NumPy."""
    g, al = gamma[:, None], alpha[:, None]
    k, l, w, pair, n, first = _triples(a.shape[1])
    u = expi(theta)
    B = np.ascontiguousarray((a * u).T)
    BB = w * (B[k] * B[l])
    S = np.add.reduceat(BB[pair] * np.conj(B)[n], first, axis=0).T
    return -(al / LD(2)) * a + I * g * np.conj(u) * S


# ---- the integrator --------------------------------------------------------------------------------------------------------
def _span(f, y, rate, theta0, gamma, alpha, length, n, save_every, rows):
    """n classic RK4 steps of f over one span on its local grid z = i h; the saved rows are appended to ``rows``."""
    h = LD(length) / LD(n)
    half = h / LD(2)
    for i in range(n):
        z = LD(i) * h
        th0, thm, th1 = theta0 + rate * z, theta0 + rate * (z + half), theta0 + rate * (z + h)
        k1 = f(th0, y, gamma, alpha)
        k2 = f(thm, y + half * k1, gamma, alpha)
        k3 = f(thm, y + half * k2, gamma, alpha)
        k4 = f(th1, y + h * k3, gamma, alpha)
        y = y + (h / LD(6)) * (k1 + LD(2) * k2 + LD(2) * k3 + k4)
        if (i + 1) % save_every == 0:
            rows.append(y)
    return y


def _result(rows, want_rows):
    rows = np.stack(rows, axis=1)
    p = power(rows)
    return dict(a_end=rows[:, -1], p_wave_end=p[:, -1], p_wave_max=p.max(axis=1), rows=rows if want_rows else None)


def _per_point(x, N):
    return np.array(np.broadcast_to(ld(x), (N,)))


def integrate(f, a0, rate, *, z_max, n, save_every, gamma, alpha, want_rows=False):
    """One sweep: f one of the right-hand sides, rate (N, C) the phase rates (dbeta per channel, kappa per line; (N,) for one
    channel), a0 (NW,) or (N, NW), gamma / alpha a scalar or (N,).
    -> dict(a_end (N, NW) clongdouble, p_wave_end, p_wave_max (N, NW) longdouble, rows (N, n_saved, NW) or None)."""
    rate = ld(rate)
    if rate.ndim == 1:
        rate = rate[:, None]
    N = rate.shape[0]
    y = np.array(np.broadcast_to(cld(a0), (N, np.shape(a0)[-1])))
    rows = [y]
    _span(f, y, rate, LD(0), _per_point(gamma, N), _per_point(alpha, N), z_max, int(n), int(save_every), rows)
    return _result(rows, want_rows)


def chain(f, a0, spans, transfers, save_every, want_rows=True):
    """The accumulated-phase model integrated directly, in the physical frame: span s has the FWM phase Theta_s + dbeta_s zeta
    on its local coordinate zeta, Theta_s = sum_{k < s} dbeta_k L_k, its own h, gamma and alpha; a boundary multiplies the
    amplitudes by the transfer.  spans: (length, n_steps, dbeta, gamma, alpha), dbeta (N,) or (N, K); transfers: S - 1 entries
    (NW,) or (N, NW).  Rows: every span's row 0 (the state after the transfer) and its saved rows.  -> the dict of integrate."""
    first = ld(spans[0][2])
    N = first.shape[0]
    y = np.array(np.broadcast_to(cld(a0), (N, np.shape(a0)[-1])))
    theta = np.zeros((N, 1 if first.ndim == 1 else first.shape[1]), dtype=LD)
    rows = []
    for s, (length, n, rate, gamma, alpha) in enumerate(spans):
        rate = ld(rate).reshape(N, -1)
        rows.append(y)
        y = _span(f, y, rate, theta, _per_point(gamma, N), _per_point(alpha, N), length, int(n), int(save_every), rows)
        if s + 1 < len(spans):
            y = y * cld(transfers[s])
            theta = theta + rate * LD(length)
    return _result(rows, want_rows)


# ---- errors ----------------------------------------------------------------------------------------------------------------
def point_err(got, truth):
    """The project's wave_err convention per point: max over the waves (and rows) of |got - truth| over the point's largest
    |truth|.  got / truth (N, ...) -> (N,) float64.  Powers are passed as they are and compared as moduli."""
    truth = np.asarray(truth)
    N = truth.shape[0]
    wide = CLD if np.iscomplexobj(truth) or np.iscomplexobj(got) else LD
    d = np.abs(np.asarray(got).astype(wide) - truth.astype(wide)).reshape(N, -1)
    return np.asarray(d.max(axis=1) / np.abs(truth).reshape(N, -1).max(axis=1), dtype=np.float64)


def elementwise_err(got, truth):
    """max |got - truth| / |truth| over every element: the figure rel_err quotes."""
    truth = np.asarray(truth)
    wide = CLD if np.iscomplexobj(truth) or np.iscomplexobj(got) else LD
    return float(np.max(np.abs(np.asarray(got).astype(wide) - truth.astype(wide)) / np.abs(truth)))


def median_err(got, truth):
    return float(np.median(point_err(got, truth)))


def max_err(got, truth):
    return float(np.max(point_err(got, truth)))
