"""The frame-anchored RK4 step of the fused float64 four-wave sweeps (rk4_step_on with FRAME in csrc/psa_rk4_kernel.inc.h;
DESIGN.md 3.1, items 1, 2 and 8) restated in NumPy, beside the step it replaces, which carries the phase factor
E(z) = 2*d*gamma*exp(i*dbeta*z) by two rotations per step and re-seeds it every 64 steps:

  (1)  both steps end in the same place to rounding.  A Runge-Kutta step is invariant under a constant linear change of
       variables; the frame step takes each step on B = diag(1, 1, tau, tau) * A with tau = exp(i*dbeta*(z_n + d)/2), where the
       phase factor is e*conj(r), e, 2e, e*r at the four stages of every step, and multiplies the sidebands by r between steps;
  (2)  the frame step is exchange-symmetric: A1 <-> A2, A3 <-> A4 permutes the result of a whole run and changes no bit;
  (3)  on mirrored states the general frame step is the mirrored frame step pairwise, in every bit;
  (4)  F(step) = exp(i*dbeta*(z_step + d)/2), which takes a row out of the frame, is ONE function of the absolute step index:
       built for a row from the seed below it, it is the F a loop carries (rotated once per step, re-seeded at the multiples of
       64 BEFORE the row that falls there), in every bit.

(2) to (4) are statements about the expression lists -- which operand meets which, in what order -- and hold for any
deterministic rounding, so a*b + c rounded twice stands in for the kernel's FMA here and everything runs vectorised.  (1)
is a statement about rounding noise; NumPy estimates it and does not reproduce the kernel's bits.

Measured in (1) (carried against frame, 200 steps, dbeta*h from 1e-9 to 12): worst |difference| = 0.61 * steps * eps *
max|A| for four-wave states and 0.63 for mirrored ones (both at dbeta*h = -12), against the bound of 40 reasoned in the test."""
import numpy as np

EPS = float(np.finfo(np.float64).eps)
RESYNC = 64
STEPS = 200
H = 0.05                                    # step: 200 steps are 10 m, 2*gamma*P*L ~ 0.25 -- almost no parametric gain
DBH = np.concatenate([10.0 ** np.arange(-9.0, 1.0), [2.0, 3.0, 5.0, 8.0, 12.0]])     # |dbeta * h|, as tests/test_gpu_parity.py


def fma(a, b, c):
    return a * b + c


def rotate(er, ei, rc, rs):
    return fma(er, rc, -(ei * rs)), fma(er, rs, ei * rc)


# ---- the stages, operation for operation as in the kernel (FUSED, LOSS, CROSS); real = the phase factor is Er alone ----------
def stage(a, base, Er, Ei, g, tg, ha, real=False):
    x1, y1, x2, y2, x3, y3, x4, y4 = a
    p = [fma(a[2 * j], a[2 * j], a[2 * j + 1] * a[2 * j + 1]) for j in range(4)]
    gs = tg * ((p[0] + p[1]) + (p[2] + p[3]))
    gj = [fma(-g, pj, gs) for pj in p]
    b23r, b23i = fma(x2, x3, y2 * y3), fma(x2, y3, -(y2 * x3))
    b14r, b14i = fma(x1, x4, y1 * y4), fma(x1, y4, -(y1 * x4))
    if real:
        h23r, h23i, h14r, h14i = Er * b23r, Er * b23i, Er * b14r, Er * b14i
    else:
        h23r, h23i = fma(Er, b23r, -(Ei * b23i)), fma(Er, b23i, Ei * b23r)
        h14r, h14i = fma(Er, b14r, -(Ei * b14i)), fma(Er, b14i, Ei * b14r)
    lk = lambda gsig, v, c: fma(gsig, v, fma(ha, a[c], base[c]))   # noqa: E731
    return [fma(-y4, h23r, fma(-x4, h23i, lk(-gj[0], y1, 0))), fma(x4, h23r, fma(-y4, h23i, lk(gj[0], x1, 1))),
            fma(-y3, h14r, fma(-x3, h14i, lk(-gj[1], y2, 2))), fma(x3, h14r, fma(-y3, h14i, lk(gj[1], x2, 3))),
            fma(-y2, h14r, fma(x2, h14i, lk(-gj[2], y3, 4))), fma(x2, h14r, fma(y2, h14i, lk(gj[2], x3, 5))),
            fma(-y1, h23r, fma(x1, h23i, lk(-gj[3], y4, 6))), fma(x1, h23r, fma(y1, h23i, lk(gj[3], x4, 7)))]


def stage_mirrored(a, base, Er, Ei, g, tg, ha, real=False):
    x1, y1, xs, ys = a
    sg = tg + tg
    p0, p2 = fma(x1, x1, y1 * y1), fma(xs, xs, ys * ys)
    gs = sg * (p0 + p2)
    g1, g3 = fma(-g, p0, gs), fma(-g, p2, gs)
    br, bi = fma(x1, xs, y1 * ys), fma(x1, ys, -(y1 * xs))
    if real:
        hr, hi = Er * br, Er * bi
    else:
        hr, hi = fma(Er, br, -(Ei * bi)), fma(Er, bi, Ei * br)
    lk = lambda gsig, v, c: fma(gsig, v, fma(ha, a[c], base[c]))   # noqa: E731
    return [fma(-ys, hr, fma(-xs, hi, lk(-g1, y1, 0))), fma(xs, hr, fma(-ys, hi, lk(g1, x1, 1))),
            fma(-y1, hr, fma(x1, hi, lk(-g3, ys, 2))), fma(x1, hr, fma(y1, hi, lk(g3, xs, 3)))]


class Lane:
    """the lane constants of sweep_point for arrays of points: gamma, alpha, dbeta per point, one step h"""

    def __init__(self, gamma, alpha, dbeta, h=H):
        self.dbeta, self.hd, hh = dbeta, h, 0.5 * h
        g, ha = gamma, -0.5 * alpha
        tg = g + g
        self.g_d, self.tg_d, self.ha_d = hh * g, hh * tg, hh * ha
        self.g_h, self.tg_h, self.ha_h = h * g, h * tg, h * ha
        self.rc, self.rs = np.cos(dbeta * (0.5 * h)), np.sin(dbeta * (0.5 * h))
        self.ec, self.es = self.tg_d * self.rc, self.tg_d * self.rs


def _combine(y, Y2, Y3, Y4):
    return [fma(2.0, Y3[c], fma(-4.0, y[c], Y2[c])) + Y4[c] for c in range(len(y))]


def step_carried(L, y, Er, Ei, st=stage):
    Y2 = st(y, y, Er, Ei, L.g_d, L.tg_d, L.ha_d)
    Er, Ei = rotate(Er, Ei, L.rc, L.rs)
    Y3 = st(Y2, y, Er, Ei, L.g_d, L.tg_d, L.ha_d)
    Y4 = st(Y3, y, Er + Er, Ei + Ei, L.g_h, L.tg_h, L.ha_h)
    t = _combine(y, Y2, Y3, Y4)
    Er, Ei = rotate(Er, Ei, L.rc, L.rs)
    D = st(Y4, t, Er, Ei, L.g_d, L.tg_d, L.ha_d)
    return [fma(D[c], 1.0 / 3.0, y[c]) for c in range(len(y))], Er, Ei


def step_frame(L, y, st=stage):
    sig = len(y) // 2
    Y2 = st(y, y, L.ec, -L.es, L.g_d, L.tg_d, L.ha_d)
    Y3 = st(Y2, y, L.tg_d, None, L.g_d, L.tg_d, L.ha_d, real=True)
    Y4 = st(Y3, y, L.tg_h, None, L.g_h, L.tg_h, L.ha_h, real=True)
    t = _combine(y, Y2, Y3, Y4)
    D = st(Y4, t, L.ec, L.es, L.g_d, L.tg_d, L.ha_d)
    y = [fma(D[c], 1.0 / 3.0, y[c]) for c in range(len(y))]
    for c in range(sig, len(y), 2):
        y[c], y[c + 1] = rotate(y[c], y[c + 1], L.rc, L.rs)
    return y


def frame_seed(L, step):
    ph = L.dbeta * (0.5 * fma(float(step), L.hd, 0.5 * L.hd))
    return np.cos(ph), np.sin(ph)


def frame_at(L, step):
    k = step % RESYNC
    fc, fs = frame_seed(L, step - k)
    for _ in range(k):
        fc, fs = rotate(fc, fs, L.rc, L.rs)
    return fc, fs


def enter_frame(L, y):
    fc, fs = frame_seed(L, 0)
    y, sig = list(y), len(y) // 2
    for c in range(sig, len(y), 2):
        y[c], y[c + 1] = rotate(y[c], y[c + 1], fc, fs)
    return y


def leave_frame(y, fc, fs):
    """sidebands times conj(F), F renormalised to first order: F * (1 - (|F|^2 - 1) / 2)"""
    ce = -0.5 * fma(fs, fs, fma(fc, fc, -1.0))
    nc, ns = fma(fc, ce, fc), fma(fs, ce, fs)
    a, sig = list(y), len(y) // 2
    for c in range(sig, len(y), 2):
        a[c], a[c + 1] = fma(y[c], nc, y[c + 1] * ns), fma(y[c + 1], nc, -(y[c] * ns))
    return a


def run_carried(L, y, n, st=stage):
    Er = Ei = None
    for i in range(n):
        if i % RESYNC == 0:
            ph = L.dbeta * (float(i) * L.hd)
            Er, Ei = L.tg_d * np.cos(ph), L.tg_d * np.sin(ph)
        y, Er, Ei = step_carried(L, y, Er, Ei, st)
    return y


def run_frame(L, y, n, st=stage):
    y = enter_frame(L, y)
    for _ in range(n):
        y = step_frame(L, y, st)
    return leave_frame(y, *frame_at(L, n))


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all(a.view(np.uint64) == b.view(np.uint64)))


def _points(seed, mirrored):
    """one random state per (|dbeta*h|, sign, draw): pumps 0.3..1, sidebands 1e-4..1e-1 of any phase (the sweeps' kind)"""
    rng = np.random.default_rng(seed)
    dbh = np.repeat(np.concatenate([DBH, -DBH]), 8)
    n = dbh.size
    amp = np.column_stack([rng.uniform(0.3, 1.0, (n, 2)), 10.0 ** rng.uniform(-4, -1, (n, 2))])
    A = amp * np.exp(1j * rng.uniform(-np.pi, np.pi, (n, 4)))
    if mirrored:
        A[:, 1], A[:, 3] = A[:, 0], A[:, 2]
    y = [np.ascontiguousarray(c) for c in A.view(np.float64).T]
    return Lane(rng.uniform(5e-3, 2e-2, n), rng.uniform(0.0, 3e-4, n), dbh / H), y


EXCHANGE = [2, 3, 0, 1, 6, 7, 4, 5]          # components after A1 <-> A2, A3 <-> A4
HALF = [0, 1, 4, 5]                          # the mirrored state's components in the record


def test_carried_and_frame_anchored_steps_agree_to_rounding():
    """Bound, per unit of steps * eps * max|A|.  One step of either form rounds each component a handful of times on values
    of at most 4 max|A| (t = Y2 + 2 Y3 + Y4 - 4 y: two roundings at ~4 |y| u; y + D/3: one; the stage chains and the sideband
    rotation, 2.2 u + 1 u for the modulus of the rounded r, stay below that): under 16 u = 8 eps per step and form, 16 for the
    two.  Both forms take sincos of a phase that reaches |dbeta*h| * steps <= 12 * steps rad with an argument rounded to a
    relative eps; it multiplies sidebands of at most 0.1 max|A|: 1.2 per form, 2.4 for the two.  Sum 18.4.  An error made
    at step k reaches the end multiplied by at most exp(2*gamma*P*L) with gamma <= 0.02, P <= 2, L = 10: 2.2, and on average
    over k under 2.  40 is asserted; the measured worst is in the module docstring."""
    for mirrored in (False, True):
        L, y0 = _points(20261018, mirrored)
        a = run_carried(L, y0, STEPS)
        b = run_frame(L, y0, STEPS)
        big = np.max(np.abs(np.array(y0)), axis=0)
        ratio = np.max(np.abs(np.array(a) - np.array(b)), axis=0) / (STEPS * EPS * big)
        worst = int(np.argmax(ratio))
        print(f"mirrored={mirrored}: worst |carried - frame| = {ratio.max():.3f} * steps * eps * max|A| at dbeta*h = {L.dbeta[worst] * H:g}")
        assert ratio.max() < 40.0
        if mirrored:                         # and on half the state
            bm = run_frame(L, [y0[c] for c in HALF], STEPS, stage_mirrored)
            assert same_bits(bm, [b[c] for c in HALF])


def test_the_frame_anchored_run_is_exchange_symmetric_in_bits():
    L, y0 = _points(7, False)
    out = run_frame(L, y0, STEPS)
    swapped = run_frame(L, [y0[c] for c in EXCHANGE], STEPS)
    assert same_bits([out[c] for c in EXCHANGE], swapped)
    assert not same_bits(out, swapped)       # the states were not symmetric to begin with


def test_on_mirrored_states_the_general_frame_step_is_the_mirrored_one_pairwise():
    L, y0 = _points(11, True)
    full, half = enter_frame(L, y0), enter_frame(L, [y0[c] for c in HALF])
    for _ in range(STEPS):
        full, half = step_frame(L, full), step_frame(L, half, stage_mirrored)
    assert same_bits(full[0:2], half[0:2]) and same_bits(full[2:4], half[0:2])
    assert same_bits(full[4:6], half[2:4]) and same_bits(full[6:8], half[2:4])
    assert np.all(np.isfinite(np.array(full))) and np.all(np.array(full) != 0.0)


def test_the_frame_of_a_row_is_one_function_of_the_step_index():
    """carried through a loop as the trajectory kernels do (one rotation per step, the exact seed at the multiples of 64
    before the row that falls there) against built for the row alone, as the summary kernels do for A[-1]"""
    L, _ = _points(3, False)
    fc, fs = frame_seed(L, 0)
    checked = []
    for step in range(1, 2 * RESYNC + 3):
        fc, fs = rotate(fc, fs, L.rc, L.rs)
        if step % RESYNC == 0:
            fc, fs = frame_seed(L, step)
        bc, bs = frame_at(L, step)
        assert same_bits(fc, bc) and same_bits(fs, bs), step
        checked.append(step)
        if step % RESYNC:                    # between the seeds F is carried: not the sincos of its own phase, in general
            continue
        ph = L.dbeta * (0.5 * (step * L.hd + 0.5 * L.hd))
        assert same_bits(fc, np.cos(ph)) and same_bits(fs, np.sin(ph))
    assert {63, 64, 65, 127, 128, 129} <= set(checked)
    # 63 rotations from an exact seed leave |F| within 63 roundings of one; what leave_frame applies is renormalised, so a
    # row's moduli are the frame's to a few ulp (a + b*c is rounded twice here: the product to 3 u, the renormalised F to 2 u)
    fc, fs = frame_at(L, RESYNC - 1)
    assert np.max(np.abs(np.hypot(fc, fs) - 1.0)) < 64 * 2 * EPS
    _, y = _points(5, False)
    a = leave_frame(y, fc, fs)
    for c in (4, 6):
        pb, pa = y[c] ** 2 + y[c + 1] ** 2, a[c] ** 2 + a[c + 1] ** 2
        assert np.max(np.abs(pa - pb) / pb) < 8 * EPS
