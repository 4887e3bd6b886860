"""The 80-bit yardstick of the adaptive sweep: Dormand-Prince 5(4) with scipy's step-size controller in np.longdouble /
np.clongdouble, the fixed point of tests/test_truth_rk45_host.py and tests/test_gpu_rk45_truth.py.

An adaptive run has a discrete scheme of its own: the step sequence is part of it.  Where the 80-bit controller accepts and
rejects the same attempts as a float64 run -- every set of tests/truth_cases.py, asserted there point by point -- the two take
the same steps to ~1e-6 of a step (the error norm is a difference that cancels to rtol of its terms, so float64 knows the
next step size to ~1e-7 of itself; measured: step ends up to 1.2e-6 m apart after 1 300 steps), the truncation error, itself
below 100 rtol, moves by that fraction of itself and cancels in a comparison as it does for a fixed grid, and what is left is
the float64 run's rounding.  The one output that sees the displacement is p_max, a sample AT the step ends
(tests/test_truth_rk45_host.py accounts for it).

What belongs to the scheme is taken as the kernel and scipy have it, as float64 VALUES: the tableau (each entry the correctly
rounded quotient), E, the dense-output matrix P, SAFETY, the factor limits, the exponent -1/5, the constants of the initial
step, rtol, atol, h_max, first_step, and the minimum step 10 ulp_double(z).  Everything else -- the state, z, h, the stages,
the error norm, the factor, the interpolant -- is 80-bit arithmetic on them.  The right-hand side is truth_ld.rhs_waves with
theta = rate z at each stage's own z.  Written from scipy 1.15's algorithm (_ivp/rk.py: RungeKutta._step_impl, rk_step,
RkDenseOutput; _ivp/common.py: select_initial_step, norm) and the header of psa_rk45.hip; nothing is shared with
tests/rk45_np.py.  All points advance together, one attempt per pass, each with its own z and h; a point that has ended is
carried along unchanged.

    integrate(a0, rate, z_max=..., rtol=..., atol=..., gamma=..., alpha=...) -> dict as the kernel's outputs:
        a_end (N, NW), p_end, p_max (N,: wave 2, p_max over z = 0 and every accepted step end), p_wave_end, p_wave_max (N, NW:
        the same for every wave, the form truth_cases.errors scales by), status (0 reached z_max, 1 step below the minimum,
        2 max_steps attempts), z_end, n_accepted, n_rejected, rows (N, n_out + 1, NW) at np.linspace(0, z_max, n_out + 1) or
        None, steps (the recorded point's accepted (z, h) pairs) and step_ends (its state after each of them) or None.
"""
import numpy as np

import truth_ld as T

LD, CLD = T.LD, T.CLD

# float64 values, then widened: Python's a / b is the correctly rounded quotient
C_NODE = [LD(x) for x in (0.0, 1 / 5, 3 / 10, 4 / 5, 8 / 9, 1.0)]
A_ROWS = [[LD(x) for x in row] for row in (
    (), (1 / 5,), (3 / 40, 9 / 40), (44 / 45, -56 / 15, 32 / 9), (19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729),
    (9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656))]
B_ROW = [LD(x) for x in (35 / 384, 0.0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84)]
E_ROW = [LD(x) for x in (-71 / 57600, 0.0, 71 / 16695, -71 / 1920, 17253 / 339200, -22 / 525, 1 / 40)]
P_DENSE = [[LD(x) for x in row] for row in (
    (1.0, -8048581381 / 2820520608, 8663915743 / 2820520608, -12715105075 / 11282082432),
    (0.0, 0.0, 0.0, 0.0),
    (0.0, 131558114200 / 32700410799, -68118460800 / 10900136933, 87487479700 / 32700410799),
    (0.0, -1754552775 / 470086768, 14199869525 / 1410260304, -10690763975 / 1880347072),
    (0.0, 127303824393 / 49829197408, -318862633887 / 49829197408, 701980252875 / 199316789632),
    (0.0, -282668133 / 205662961, 2019193451 / 616988883, -1453857185 / 822651844),
    (0.0, 40617522 / 29380423, -110615467 / 29380423, 69997945 / 29380423))]
SAFETY, MIN_FACTOR, MAX_FACTOR, ERR_EXP = LD(0.9), LD(0.2), LD(10.0), LD(-1 / 5)


def _weighted(K, w):
    """sum_s w_s K_s over the stages present, in ascending s."""
    total = None
    for k, ws in zip(K, w):
        if ws != 0:
            total = ws * k if total is None else total + ws * k
    return total


def _rms(x):
    """scipy's common.norm per point: the 2-norm of the complex row over sqrt(its length).  x (N, NW) -> (N,)."""
    return np.sqrt((x.real * x.real + x.imag * x.imag).sum(axis=1)) / np.sqrt(LD(x.shape[1]))


def _min_step(z):
    """10 ulp of z as a double, the kernel's and scipy's floor on a step."""
    z64 = np.asarray(z, dtype=np.float64)
    return LD(10) * T.ld(np.nextafter(z64, np.inf) - z64)


def integrate(a0, rate, *, z_max, rtol, atol, gamma, alpha, h_max=np.inf, first_step=0.0, max_steps=1_000_000, n_out=0,
              record=None):
    rate = T.ld(rate)
    if rate.ndim == 1:
        rate = rate[:, None]
    N = rate.shape[0]
    y = np.array(np.broadcast_to(T.cld(a0), (N, np.shape(a0)[-1])))
    NW = y.shape[1]
    g, al = T._per_point(gamma, N), T._per_point(alpha, N)
    z_max, rtol, atol, h_max = LD(z_max), LD(rtol), LD(atol), LD(h_max)

    def f(z, a):
        return T.rhs_waves(rate * z[:, None], a, g, al)

    z = np.zeros(N, dtype=LD)
    status = np.full(N, -1, dtype=np.int32)
    n_acc, n_rej = np.zeros(N, dtype=np.int64), np.zeros(N, dtype=np.int64)
    p_top = T.power(y)
    rows = None
    if n_out > 0:
        rows = np.full((N, n_out + 1, NW), np.nan, dtype=CLD)
        rows[:, 0] = y
        z_rows = T.ld(np.linspace(0.0, float(z_max), n_out + 1))      # the grid the kernel is asked for: float64 values
    next_row = np.ones(N, dtype=np.int64)
    steps, ends = ([], []) if record is not None else (None, None)

    with np.errstate(all="ignore"):
        live = np.isfinite(y.real).all(axis=1) & np.isfinite(y.imag).all(axis=1)
        status[~live] = 1
        k_first = f(z, y)                                             # f(z, y): the next attempt's first stage
        if first_step > 0.0:
            h_abs = np.full(N, LD(first_step))
        else:                                                         # select_initial_step, error estimator order 4
            scale = atol + np.abs(y) * rtol
            d0, d1 = _rms(y / scale), _rms(k_first / scale)
            h0 = np.where((d0 < LD(1e-5)) | (d1 < LD(1e-5)), LD(1e-6), LD(0.01) * d0 / d1)
            h0 = np.minimum(h0, z_max)
            d2 = _rms((f(z + h0, y + h0[:, None] * k_first) - k_first) / scale) / h0
            h1 = np.where((d1 <= LD(1e-15)) & (d2 <= LD(1e-15)), np.maximum(LD(1e-6), h0 * LD(1e-3)),
                          (LD(0.01) / np.maximum(d1, d2)) ** LD(1 / 5))
            h_abs = np.minimum(np.minimum(np.minimum(LD(100) * h0, h1), z_max), h_max)
        floor = _min_step(z)
        h_abs = np.where(h_abs > h_max, h_max, np.where(h_abs < floor, floor, h_abs))
        after_rejection = np.zeros(N, dtype=bool)

        while True:
            too_small = live & (h_abs < floor)
            status[too_small] = 1
            live &= ~too_small
            capped = live & (n_acc + n_rej >= max_steps)
            status[capped] = 2
            live &= ~capped
            if not live.any():
                break
            z_new = np.minimum(z + h_abs, z_max)
            h = z_new - z
            hc = h[:, None]
            K = [k_first]
            for s in range(1, 6):
                K.append(f(z + C_NODE[s] * h, y + hc * _weighted(K, A_ROWS[s])))
            y_new = y + hc * _weighted(K, B_ROW)
            K.append(f(z_new, y_new))
            scale = atol + np.maximum(np.abs(y), np.abs(y_new)) * rtol
            err = _rms(hc * _weighted(K, E_ROW) / scale)
            accept = live & (err < 1)
            reject = live & ~accept                                   # a NaN norm is a rejection by MIN_FACTOR
            grow = np.where(err == 0, MAX_FACTOR, np.minimum(MAX_FACTOR, SAFETY * err ** ERR_EXP))
            grow = np.where(after_rejection, np.minimum(LD(1), grow), grow)
            shrink = SAFETY * err ** ERR_EXP
            shrink = np.where(shrink > MIN_FACTOR, shrink, MIN_FACTOR)
            h_next = np.abs(h) * np.where(accept, grow, shrink)

            if rows is not None:
                for i in np.nonzero(accept & (next_row <= n_out))[0]:
                    if z_rows[next_row[i]] > z_new[i]:
                        continue
                    Q = [_weighted([k[i] for k in K], [P_DENSE[s][j] for s in range(7)]) for j in range(4)]
                    while next_row[i] <= n_out and z_rows[next_row[i]] <= z_new[i]:
                        x = (z_rows[next_row[i]] - z[i]) / h[i]
                        poly, xp = 0, x
                        for j in range(4):
                            poly = poly + Q[j] * xp
                            xp = xp * x
                        rows[i, next_row[i]] = y[i] + h[i] * poly
                        next_row[i] += 1
            if steps is not None and accept[record]:
                steps.append((z[record], h[record]))
                ends.append(y_new[record].copy())

            y = np.where(accept[:, None], y_new, y)
            k_first = np.where(accept[:, None], K[6], k_first)
            z = np.where(accept, z_new, z)
            n_acc += accept
            n_rej += reject
            after_rejection = np.where(live, reject, after_rejection)
            p_now = T.power(y)
            p_top = np.where(accept[:, None] & ((p_now > p_top) | np.isnan(p_now)), p_now, p_top)
            done = accept & (z >= z_max)
            status[done] = 0
            live &= ~done
            floor = np.where(accept, _min_step(z), floor)
            clamped = np.where(h_next > h_max, h_max, np.where(h_next < floor, floor, h_next))
            h_abs = np.where(accept, clamped, np.where(reject, h_next, h_abs))

    p = T.power(y)
    return dict(a_end=y, p_end=p[:, 2], p_max=p_top[:, 2], p_wave_end=p, p_wave_max=p_top, status=status, z_end=z,
                n_accepted=n_acc, n_rejected=n_rej, rows=rows, steps=steps, step_ends=ends)
