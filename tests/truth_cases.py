"""The input sets of tests/test_truth_host.py and tests/test_gpu_truth.py, each with its 80-bit run (truth_ld) and its twin's
run, computed once per process; the float32 twins; and the bar both files apply.

Shapes: N = 67 points (one full wave and a ragged one with one lane per point, an odd count for two points per lane, four full
waves and a ragged one with four lanes per point), 1 500 steps over 300 m (not a multiple of the 64-step seed grid: 23
re-seeds), rows every 7 steps (a tail of 2 behind the last row).  Per-point gamma, alpha and amplitudes with random phases.

Every result is a dict in one form: a_end (N, NW), p_wave_end, p_wave_max (N, NW), rows (N, n_saved, NW) or None.

Chains: two spans of every family (chain), and three spans of the 4/6-wave model in float64 and float32 with a middle span
shorter than a seed interval (chain3, chain3_f32), whose twins restate the kernels' B gauge span by span (chain_b_gauge).

At the end, the sets of the adaptive sweep (tests/test_truth_rk45_host.py, tests/test_gpu_rk45_truth.py): the same 67 points and
fibre draws, each with the 80-bit run of Dormand-Prince 5(4) and its controller (truth_rk45_ld) and the twin's (rk45_np).
"""
import functools
import os

import numpy as np

import comb_chain_np
import comb_np
import pairs_chain_np
import pairs_np
import single_pump_chain_np
import single_pump_np
import truth_ld as T

N, N_STEPS, Z_MAX, SAVE_EVERY = 67, 1500, 300.0, 7
GAMMA, ALPHA = 0.0115, 1.15e-4
CHAIN_STEPS, CHAIN_LENGTHS, CHAIN_SAVE_EVERY = (700, 800), (140.0, 200.0), 20   # a chain's spans end on a saved row: 20 | 700, 800
FLOOR_F64, FLOOR_F32 = 2e-14, 2e-6
TWIN_CONDITION = 1e-11                 # every float64 input set: the twin's largest point_err stays below this
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def from_rows(rows):
    """Saved rows (N, n_saved, NW) -> the result dict."""
    rows = np.asarray(rows)
    p = rows.real ** 2 + rows.imag ** 2
    return dict(a_end=rows[:, -1], p_wave_end=p[:, -1], p_wave_max=p.max(axis=1), rows=rows)


def strided(res, save_every):
    """The result of a run that saved every step, read at a save stride."""
    return from_rows(res["rows"][:, ::save_every])


# ---- the bar ---------------------------------------------------------------------------------------------------------------
def errors(got, truth):
    """Per-point errors against the yardstick of everything ``got`` holds: a_end, the power summaries as moduli against the
    point's largest modulus (p_end / p_max are wave 2's), the rows.  -> {key: (N,) float64}."""
    out = dict(a_end=T.point_err(got["a_end"], truth["a_end"]))
    for key, one in (("p_wave_end", "p_end"), ("p_wave_max", "p_max")):
        mod = np.sqrt(truth[key])
        scale = mod.max(axis=1)
        if got.get(key) is not None:
            out[key] = T.point_err(np.sqrt(T.ld(got[key])), mod)
        elif got.get(one) is not None:
            out[one] = np.asarray(np.abs(np.sqrt(T.ld(got[one])) - mod[:, 2]) / scale, dtype=np.float64)
    rows = got.get("rows") if got.get("rows") is not None else got.get("traj")
    if rows is not None and truth["rows"] is not None:
        out["rows"] = T.point_err(rows, truth["rows"])
    return out


def pump_power_errors(got, truth):
    """errors' figure for the per-wave powers with the two pumps' columns alone: their moduli against the point's largest
    modulus.  -> {p_wave_end, p_wave_max: (N,) float64}."""
    out = {}
    for key in ("p_wave_end", "p_wave_max"):
        mod = np.sqrt(truth[key])
        out[key] = np.asarray(np.abs(np.sqrt(T.ld(got[key][:, :2])) - mod[:, :2]).max(axis=1) / mod.max(axis=1), dtype=np.float64)
    return out


def like(got, twin):
    """The twin's result in the form of ``got``: wave 2's p_end / p_max where the entry point returns those alone."""
    if got.get("p_wave_end") is None and got.get("p_end") is not None and twin.get("p_end") is None:
        return dict(a_end=twin["a_end"], p_end=twin["p_wave_end"][:, 2], p_max=twin["p_wave_max"][:, 2], rows=twin["rows"])
    return twin


def bar(e_got, e_twin, floor):
    """The assertion of every case: no worse than the plain twin by more than a stated factor, on the aggregates over the
    points.  -> (passes, median ratio, max ratio)."""
    med, mx = float(np.median(e_got)), float(np.max(e_got))
    tmed, tmx = float(np.median(e_twin)), float(np.max(e_twin))
    ok = med <= max(4.0 * tmed, floor) and mx <= max(8.0 * tmx, floor)
    return ok, med / tmed if tmed > 0 else float("inf"), mx / tmx if tmx > 0 else float("inf")


def judge(family, case, got, inputs, floor=FLOOR_F64):
    """Print the case's line of the record (and one more for every output that misses the bar) and -> the outputs that miss
    it: {key: (its figures as a readable line, kernel median, kernel max, twin median, twin max)}."""
    e_got, e_twin = errors(got, inputs["truth"]), errors(like(got, inputs["twin"]), inputs["truth"])
    missed, worst = {}, None
    for key, e in e_got.items():
        ok, r_med, r_max = bar(e, e_twin[key], floor)
        line = (f"{key}: kernel median {np.median(e):.2e} max {e.max():.2e}, twin median {np.median(e_twin[key]):.2e} "
                f"max {e_twin[key].max():.2e}, ratio {r_med:.2f} / {r_max:.2f}")
        if not ok:
            missed[key] = (line, float(np.median(e)), float(e.max()), float(np.median(e_twin[key])), float(e_twin[key].max()))
        if worst is None or max(r_med / 4.0, r_max / 8.0) > worst[0]:
            worst = (max(r_med / 4.0, r_max / 8.0), key, r_med, r_max)
    a, t = e_got["a_end"], e_twin["a_end"]
    print(f"\ntruth | {family} | {case} | a_end kernel {np.median(a):.2e} {a.max():.2e} twin {np.median(t):.2e} {t.max():.2e} "
          f"ratio {np.median(a) / np.median(t):.2f} {a.max() / t.max():.2f} | worst {worst[1]} {worst[2]:.2f} {worst[3]:.2f}", end="")
    for line, *_ in missed.values():
        print(f"\ntruth | {family} | {case} | misses the bar | {line}", end="")
    print()
    return missed


# ---- four and six waves ----------------------------------------------------------------------------------------------------
def _oracle_rows(a0, dbeta, dbeta2, gamma, alpha, z_max, n, save_every):
    """The C oracle point by point, with its saved rows."""
    import oracle
    n_pts = dbeta.shape[0]
    gamma, alpha = np.broadcast_to(gamma, (n_pts,)), np.broadcast_to(alpha, (n_pts,))
    rows = []
    for j in range(n_pts):
        _, A, bad = oracle.integrate(a0[j], z_max=z_max, n=n, save_every=save_every, gamma=gamma[j], alpha=alpha[j],
                                     dbeta=dbeta[j], dbeta2=0.0 if dbeta2 is None else dbeta2[j])
        assert bad < 0
        rows.append(A)
    return np.stack(rows)


def _amplitudes(rng, n_pts, pumps, sidebands):
    """Pumps 0.2-0.6 W each, sidebands 1e-7..1e-3 W, every phase random."""
    p = np.column_stack([rng.uniform(0.2, 0.6, (n_pts, pumps)), 10 ** rng.uniform(-7.0, -3.0, (n_pts, sidebands))])
    return np.sqrt(p) * np.exp(1j * rng.uniform(-3.0, 3.0, p.shape))


def _fibre(rng, n_pts, lossy):
    return GAMMA * rng.uniform(0.9, 1.1, n_pts), (ALPHA * rng.uniform(0.5, 1.5, n_pts) if lossy else 0.0)


def _waves_set(inp):
    rate = inp["dbeta"] if inp.get("dbeta2") is None else np.column_stack([inp["dbeta"], inp["dbeta2"]])
    kw = dict(z_max=inp["z_max"], n=inp["n_steps"], save_every=inp["save_every"])
    truth = T.integrate(T.rhs_waves, inp["a0"], rate, gamma=inp["gamma"], alpha=inp["alpha"], want_rows=True, **kw)
    twin = from_rows(_oracle_rows(inp["a0"], inp["dbeta"], inp.get("dbeta2"), inp["gamma"], inp["alpha"], **kw))
    return dict(inp, truth=truth, twin=twin)


@functools.lru_cache(maxsize=None)
def waves4(mirrored, lossy):
    """General amplitudes (A2 != A1, A4 != A3) or mirrored ones (A2 == A1 and A4 == A3 bit for bit in every lane: the loop
    the headline benchmark runs)."""
    rng = np.random.default_rng(4100 + 2 * mirrored + lossy)
    a0 = _amplitudes(rng, N, 2, 2)
    if mirrored:
        a0[:, 1], a0[:, 3] = a0[:, 0], a0[:, 2]
    gamma, alpha = _fibre(rng, N, lossy)
    return _waves_set(dict(dbeta=rng.uniform(-0.05, 0.05, N), gamma=gamma, alpha=alpha, a0=a0, z_max=Z_MAX, n_steps=N_STEPS,
                           save_every=SAVE_EVERY))


@functools.lru_cache(maxsize=None)
def waves4_without_mismatch(mirrored):
    """The lossy set with dbeta = 0: no phase to carry, and the one-lane step's frame rotation is the identity."""
    inp = {k: v for k, v in waves4(mirrored, True).items() if k not in ("truth", "twin")}
    return _waves_set(dict(inp, dbeta=np.zeros(N)))


def g8_inputs(alpha_i):
    """Every 4th of golden G8's first 256 mismatches (64 points: one wave), its fibre and powers, 10 000 steps over 1000 m."""
    g = np.load(os.path.join(GOLDEN, "G8.npz"))
    pick = np.arange(0, 256, 4)
    a0 = np.repeat(np.sqrt(g["p_in"]).astype(complex)[None, :], 64, axis=0)
    return dict(dbeta=g["dbeta257"][pick], gamma=float(g["gamma"]), alpha=float(g["alphas"][alpha_i]), a0=a0,
                z_max=float(g["z_max"]), n_steps=10_000, save_every=int(g["save_every"]),
                golden=g[f"n1e4_a{alpha_i}_A_end"][pick])


@functools.lru_cache(maxsize=None)
def g8(mirrored, alpha_i):
    """G8's powers are mirrored.  The general loop runs the same fibre with A2 one ulp off A1 in lane 5 -- a wave leaves the
    mirrored loop when one live lane does -- and A4 = 1.5 A3 in lane 40."""
    inp = g8_inputs(alpha_i)
    if not mirrored:
        inp["a0"][5, 1] = complex(np.nextafter(inp["a0"][5, 0].real, np.inf), inp["a0"][5, 0].imag)
        inp["a0"][40, 3] = 1.5 * inp["a0"][40, 2]
    return _waves_set(inp)


@functools.lru_cache(maxsize=None)
def waves6():
    rng = np.random.default_rng(4600)
    gamma, alpha = _fibre(rng, N, True)
    return _waves_set(dict(dbeta=rng.uniform(-0.05, 0.05, N), dbeta2=rng.uniform(-0.05, 0.05, N), gamma=gamma, alpha=alpha,
                           a0=_amplitudes(rng, N, 2, 4), z_max=Z_MAX, n_steps=N_STEPS, save_every=SAVE_EVERY))


# ---- K pairs, single pump, comb --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pairs(K):
    """K = 1, 2, 3, 5, 8, 16: every lane-group width (2, 2, 4, 8, 8, 16), a padded group at 1, 3 and 5.  K = 3 keeps the rows."""
    rng = np.random.default_rng(4200 + K)
    gamma, alpha = _fibre(rng, N, True)
    inp = dict(dbeta=rng.uniform(-0.05, 0.05, (N, K)), gamma=gamma, alpha=alpha, a0=_amplitudes(rng, N, 2, 2 * K), z_max=Z_MAX,
               n_steps=N_STEPS, save_every=SAVE_EVERY)
    kw = dict(z_max=Z_MAX, n=N_STEPS, save_every=SAVE_EVERY, gamma=gamma, alpha=alpha)
    truth = T.integrate(T.rhs_pairs, inp["a0"], inp["dbeta"], want_rows=(K == 3), **kw)
    if K == 3:
        twin = from_rows(pairs_chain_np.integrate(inp["a0"], inp["dbeta"], **kw)["traj"])
    else:
        twin = dict(pairs_np.integrate(inp["a0"], inp["dbeta"], **kw), rows=None)
    return dict(inp, truth=truth, twin=twin)


@functools.lru_cache(maxsize=None)
def single_pump(lossy):
    """Every step is saved: the rows case reads them all, the summary cases every 7th (``strided``)."""
    rng = np.random.default_rng(4300 + lossy)
    gamma, alpha = _fibre(rng, N, lossy)
    inp = dict(dbeta=rng.uniform(-4.5, 0.5, N) * GAMMA * 0.5, gamma=gamma, alpha=alpha, a0=_amplitudes(rng, N, 1, 2),
               z_max=Z_MAX, n_steps=N_STEPS)
    kw = dict(z_max=Z_MAX, n=N_STEPS, save_every=1, gamma=gamma, alpha=alpha)
    truth = T.integrate(T.rhs_single_pump, inp["a0"], inp["dbeta"], want_rows=True, **kw)
    twin = from_rows(single_pump_np.integrate(inp["a0"], inp["dbeta"], want_traj=True, **kw)["traj"])
    return dict(inp, truth=truth, twin=twin)


def at_stride(inputs, save_every):
    return dict(inputs, save_every=save_every, truth=strided(inputs["truth"], save_every), twin=strided(inputs["twin"], save_every))


@functools.lru_cache(maxsize=None)
def comb(M, lossy):
    kappa, a0, gamma, alpha = comb_np.random_inputs(N, M, 4400 + 2 * M + lossy, per_point=True, lossy=lossy)
    kw = dict(z_max=Z_MAX, n=N_STEPS, save_every=SAVE_EVERY, gamma=gamma, alpha=alpha)
    truth = T.integrate(T.rhs_comb, a0, kappa, **kw)
    twin = dict(comb_np.integrate(a0, kappa, **kw), rows=None)
    return dict(kappa=kappa, a0=a0, gamma=gamma, alpha=alpha, z_max=Z_MAX, n_steps=N_STEPS, save_every=SAVE_EVERY,
                truth=truth, twin=twin)


@functools.lru_cache(maxsize=None)
def comb_without_dispersion(M):
    """The lossy set with kappa = 0: u_m = 1 and every rotator is (1, 0), so nothing carried can drift."""
    inp = {k: v for k, v in comb(M, True).items() if k not in ("truth", "twin")}
    kappa = np.zeros_like(inp["kappa"])
    kw = dict(z_max=Z_MAX, n=N_STEPS, save_every=SAVE_EVERY, gamma=inp["gamma"], alpha=inp["alpha"])
    return dict(inp, kappa=kappa, truth=T.integrate(T.rhs_comb, inp["a0"], kappa, **kw),
                twin=dict(comb_np.integrate(inp["a0"], kappa, **kw), rows=None))


# ---- chains ----------------------------------------------------------------------------------------------------------------
def _mid_stage(rng, shape):
    """One mid-stage transfer per point with gain (-3..1 dB) and phase on every wave."""
    return np.sqrt(10.0 ** (rng.uniform(-3.0, 1.0, shape) / 10.0)) * np.exp(1j * rng.uniform(-np.pi, np.pi, shape))


def _chain_spans(rng, dbeta_shape, scale):
    return [(L, n, rng.uniform(-1.0, 1.0, dbeta_shape) * scale, GAMMA * rng.uniform(0.8, 1.6, N), ALPHA * rng.uniform(0.5, 2.0, N))
            for L, n in zip(CHAIN_LENGTHS, CHAIN_STEPS)]


@functools.lru_cache(maxsize=None)
def chain(family):
    """Two spans of 700 and 800 steps (h = 0.2 and 0.25 m) with different per-point dbeta, gamma and alpha and one per-point
    mid-stage transfer.  family: "waves" (4 waves), "single_pump", "pairs" (K = 3), "comb" (M = 5: kappa per line, a transfer on
    every line)."""
    rng = np.random.default_rng(dict(waves=4500, single_pump=4501, pairs=4502, comb=4503)[family])
    if family == "comb":
        a0 = comb_chain_np.random_a0(rng, N, 5)
        spans = [(L, n, comb_chain_np.random_kappa(rng, N, 5), GAMMA * rng.uniform(0.8, 1.6, N), ALPHA * rng.uniform(0.5, 2.0, N))
                 for L, n in zip(CHAIN_LENGTHS, CHAIN_STEPS)]
        transfers = [_mid_stage(rng, (N, 5))]
        twin = comb_chain_np.chain(a0, spans, transfers, CHAIN_SAVE_EVERY)["rows"]
        f = T.rhs_comb
    elif family == "waves":
        import test_chain_host
        a0, spans = _amplitudes(rng, N, 2, 2), _chain_spans(rng, N, 0.05)
        transfers = [_mid_stage(rng, (N, 4))]
        twin = np.stack([test_chain_host._oracle_chain(a0[j], [(L, n, db[j], g[j], al[j]) for L, n, db, g, al in spans],
                                                       [transfers[0][j]], CHAIN_SAVE_EVERY) for j in range(N)])
        f = T.rhs_waves
    elif family == "single_pump":
        a0, spans = _amplitudes(rng, N, 1, 2), _chain_spans(rng, N, 2.5 * GAMMA * 0.5)
        transfers = [_mid_stage(rng, (N, 3))]
        twin = single_pump_chain_np.chain(a0, spans, transfers, CHAIN_SAVE_EVERY)["rows"]
        f = T.rhs_single_pump
    else:
        a0, spans = _amplitudes(rng, N, 2, 6), _chain_spans(rng, (N, 3), 0.05)
        transfers = [_mid_stage(rng, (N, 8))]
        twin = pairs_chain_np.chain(a0, spans, transfers, CHAIN_SAVE_EVERY)["rows"]
        f = T.rhs_pairs
    truth = T.chain(f, a0, spans, transfers, CHAIN_SAVE_EVERY)
    return dict(a0=a0, spans=spans, transfers=transfers, save_every=CHAIN_SAVE_EVERY, truth=truth, twin=from_rows(twin))


def chain_arrays(inputs):
    """The spans of a chain as the C entry points take them."""
    spans = inputs["spans"]
    return dict(dbeta=np.stack([s[2] for s in spans]), n_steps=[s[1] for s in spans], seg_len=[s[0] for s in spans],
                gamma=np.stack([s[3] for s in spans]), alpha=np.stack([s[4] for s in spans]), a0=inputs["a0"],
                transfers=np.stack(inputs["transfers"]), save_every=inputs["save_every"])


# ---- float32: the twin is a plain float32 classic RK4 ------------------------------------------------------------------------
F32, C64 = np.float32, np.complex64


def _expi32(dbeta32, z):
    """exp(i dbeta z) in float32: the phase is formed and reduced to [-pi, pi] in float64, then a float32 cos / sin, as
    psa_rk4_kernel.inc.h says the float32 kernels do."""
    ph = dbeta32.astype(np.float64) * z
    r = (ph - 2.0 * np.pi * np.rint(ph / (2.0 * np.pi))).astype(F32)
    return (np.cos(r) + 1j * np.sin(r)).astype(C64)


def _rhs32_waves(e, a, g, al):
    P = a.real * a.real + a.imag * a.imag
    kerr = P + F32(2) * (P.sum(axis=1, keepdims=True) - P)
    e = e[:, None]
    M = np.concatenate([np.conj(a[:, 1:2]) * a[:, 2:3] * a[:, 3:4] * e, np.conj(a[:, 0:1]) * a[:, 2:3] * a[:, 3:4] * e,
                        np.conj(a[:, 3:4]) * a[:, 0:1] * a[:, 1:2] * np.conj(e),
                        np.conj(a[:, 2:3]) * a[:, 0:1] * a[:, 1:2] * np.conj(e)], axis=1)
    return (F32(-0.5) * al) * a + C64(1j) * (g * kerr * a) + C64(2j) * (g * M)


def _rhs32_single_pump(e, a, g, al):
    P = a.real * a.real + a.imag * a.imag
    kerr = F32(2) * P.sum(axis=1, keepdims=True) - P
    e = e[:, None]
    p, s, i = a[:, 0:1], a[:, 1:2], a[:, 2:3]
    M = np.concatenate([F32(2) * np.conj(p) * s * i * e, np.conj(i) * p * p * np.conj(e), np.conj(s) * p * p * np.conj(e)],
                       axis=1)
    return (F32(-0.5) * al) * a + C64(1j) * (g * kerr * a) + C64(1j) * (g * M)


def rk4_f32(rhs, a0, dbeta, *, z_max, n, save_every, gamma, alpha, kahan=False, carried_for=0):
    """State and arithmetic in float32 / complex64; z = i h in float64 for the phase alone.
    kahan: the compensated state update of the scalar float32 kernel (psa_rk4_kernel.inc.h, rk4_step_classic) in the place of
    y += increment.  carried_for = 16: the phase factor as the float32 kernels have it -- an exact seed every 16 steps and one
    rotation by the rounded exp(i dbeta h / 2) per half step from there -- in the place of cos / sin at every stage."""
    dbeta = np.asarray(dbeta, dtype=F32)
    n_pts = dbeta.shape[0]
    y = np.array(np.broadcast_to(np.asarray(a0, dtype=C64), (n_pts, np.shape(a0)[-1])))
    g = np.broadcast_to(np.asarray(gamma, dtype=F32), (n_pts,))[:, None]
    al = np.broadcast_to(np.asarray(alpha, dtype=F32), (n_pts,))[:, None]
    h64 = z_max / n
    h, half, sixth = F32(h64), F32(0.5 * h64), F32(h64 / 6.0)
    rows, lo, rot = [y], np.zeros_like(y), _expi32(dbeta, 0.5 * h64)
    for i in range(n):
        if carried_for:
            e0 = _expi32(dbeta, i * h64) if i % carried_for == 0 else e1
            em = e0 * rot
            e1 = em * rot
        else:
            e0, em, e1 = _expi32(dbeta, i * h64), _expi32(dbeta, (i + 0.5) * h64), _expi32(dbeta, (i + 1) * h64)
        k1 = rhs(e0, y, g, al)
        k2 = rhs(em, y + half * k1, g, al)
        k3 = rhs(em, y + half * k2, g, al)
        k4 = rhs(e1, y + h * k3, g, al)
        inc = sixth * (k1 + F32(2) * k2 + F32(2) * k3 + k4)
        if kahan:
            inc = inc + lo
            lo = inc - ((y + inc) - y)
        y = y + inc
        assert y.dtype == C64 and e1.dtype == C64
        if (i + 1) % save_every == 0:
            rows.append(y)
    return from_rows(np.stack(rows, axis=1))


def _rounded(inp):
    """The inputs as the float32 entry points see them: what the yardstick integrates."""
    out = dict(inp)
    for k in ("dbeta", "gamma", "alpha"):
        out[k] = np.asarray(inp[k], dtype=F32)
    out["a0"] = np.asarray(inp["a0"], dtype=C64)
    return out


@functools.lru_cache(maxsize=None)
def waves4_f32(mirrored):
    inp = _rounded({k: v for k, v in waves4(mirrored, True).items() if k not in ("truth", "twin")})
    kw = dict(z_max=Z_MAX, n=N_STEPS, save_every=SAVE_EVERY, gamma=inp["gamma"], alpha=inp["alpha"])
    truth = T.integrate(T.rhs_waves, inp["a0"], inp["dbeta"], **kw)
    return dict(inp, truth=truth, twin=rk4_f32(_rhs32_waves, inp["a0"], inp["dbeta"], **kw))


@functools.lru_cache(maxsize=None)
def single_pump_f32():
    inp = _rounded({k: v for k, v in single_pump(True).items() if k not in ("truth", "twin")})
    kw = dict(z_max=Z_MAX, n=N_STEPS, save_every=SAVE_EVERY, gamma=inp["gamma"], alpha=inp["alpha"])
    truth = T.integrate(T.rhs_single_pump, inp["a0"], inp["dbeta"], **kw)
    return dict(inp, save_every=SAVE_EVERY, truth=truth, twin=rk4_f32(_rhs32_single_pump, inp["a0"], inp["dbeta"], **kw))


# ---- the long runs: 1e5 steps in float64, 1e5 and 1e6 in float32, yardstick and twins from the compiled plain RK4 ------------
# oracle/plain_rk4.py: one C text of the scheme above per precision.  Its 80-bit instantiation is pinned against truth_ld and
# mpmath, its double and float ones against the twins above, in tests/test_truth_long_host.py.
LONG_N, LONG_STEPS, LONG_Z = 64, 100_000, 1000.0     # one wave of every float64 lane layout; the headline's step count and fibre
F32_N = 17                                           # 8 packed lanes and the odd tail


def _plain(model, inp, rate, precision, update="plain"):
    import plain_rk4
    return plain_rk4.integrate(model, inp["a0"], rate, z_max=inp["z_max"], n=inp["n_steps"], save_every=inp["save_every"],
                               gamma=inp["gamma"], alpha=inp["alpha"], precision=precision, update=update)


def _long_set(model, inp, rate):
    """The 80-bit run and the plain float64 twin of a float64 input set, both from the one C text."""
    return dict(inp, truth=_plain(model, inp, rate, "ld"), twin=_plain(model, inp, rate, "f64"))


def _rate2(inp):
    return inp["dbeta"] if inp.get("dbeta2") is None else np.column_stack([inp["dbeta"], inp["dbeta2"]])


@functools.lru_cache(maxsize=None)
def g8_long(mirrored, alpha_i, save_every=10):
    """g8()'s inputs at the headline's 100 000 steps; save_every = 10 is the stride the benchmark runs."""
    inp = g8_inputs(alpha_i)
    del inp["golden"]
    if not mirrored:
        inp["a0"][5, 1] = complex(np.nextafter(inp["a0"][5, 0].real, np.inf), inp["a0"][5, 0].imag)
        inp["a0"][40, 3] = 1.5 * inp["a0"][40, 2]
    inp.update(n_steps=LONG_STEPS, save_every=save_every)
    return _long_set("pairs", inp, inp["dbeta"])


@functools.lru_cache(maxsize=None)
def g8_long_frame_drift(mirrored, alpha_i, save_every=10, off_unit=5.5e-17):
    """What a sideband modulus off by ``off_unit`` per step -- the figure psa_rk4_kernel.inc.h states for |r| - 1 of the
    frame-anchored step's one rounded rotation -- does to the outputs of g8_long's set, evaluated and not estimated: the 80-bit
    run with that scaling planted after every step (psa_plain_rk4.inc.h, ``drift``) against the clean one.  While the pumps are
    undepleted the equations are linear in the sidebands and the result is n off_unit of the sideband exactly; where the
    sidebands have reached the pumps' scale the propagation amplifies it.  -> {output: (median, maximum) of its point_err over
    the points}, the budgets of the band's median and maximum, in the form sweep_host returns (a_end, wave 2's p_end and p_max)."""
    import plain_rk4
    s = g8_long(mirrored, alpha_i, save_every)
    planted = plain_rk4.integrate("pairs", s["a0"], s["dbeta"], z_max=s["z_max"], n=s["n_steps"], save_every=s["save_every"],
                                  gamma=s["gamma"], alpha=s["alpha"], precision="ld", sideband_drift=off_unit)
    form = dict(a_end=planted["a_end"], p_end=planted["p_wave_end"][:, 2], p_max=planted["p_wave_max"][:, 2])
    return {k: (float(np.median(v)), float(v.max())) for k, v in errors(form, s["truth"]).items()}


def _long_fibre(rng, n_pts, **inp):
    gamma, alpha = _fibre(rng, n_pts, True)
    return dict(inp, gamma=gamma, alpha=alpha, z_max=LONG_Z, n_steps=LONG_STEPS, save_every=10)


@functools.lru_cache(maxsize=None)
def waves6_long():
    rng = np.random.default_rng(5600)
    inp = _long_fibre(rng, LONG_N, dbeta=rng.uniform(-0.05, 0.05, LONG_N), dbeta2=rng.uniform(-0.05, 0.05, LONG_N),
                      a0=_amplitudes(rng, LONG_N, 2, 4))
    return _long_set("pairs", inp, _rate2(inp))


@functools.lru_cache(maxsize=None)
def pairs_long(K):
    """K = 3: 64 points, four waves of its 4-lane groups.  K = 16: 32 points, eight waves of 16-lane groups -- the 80-bit run of
    34 waves costs ten times the 4-wave one per point, and 32 is what fits into about 5 s on 16 cores; fewer would also leave
    the bar's aggregates, a median and a maximum that were calibrated on 64..67 points, to a handful of points."""
    rng = np.random.default_rng(5200 + K)
    n_pts = LONG_N if K <= 3 else 32
    inp = _long_fibre(rng, n_pts, dbeta=rng.uniform(-0.05, 0.05, (n_pts, K)), a0=_amplitudes(rng, n_pts, 2, 2 * K))
    return _long_set("pairs", inp, inp["dbeta"])


@functools.lru_cache(maxsize=None)
def single_pump_long():
    rng = np.random.default_rng(5300)
    inp = _long_fibre(rng, LONG_N, dbeta=rng.uniform(-4.5, 0.5, LONG_N) * GAMMA * 0.5, a0=_amplitudes(rng, LONG_N, 1, 2))
    return _long_set("single_pump", inp, inp["dbeta"])


@functools.lru_cache(maxsize=None)
def comb_long(M, dispersion=True):
    """dispersion = False: the same set with kappa = 0, where nothing carried can drift."""
    kappa, a0, gamma, alpha = comb_np.random_inputs(LONG_N, M, 5400 + 2 * M, per_point=True, lossy=True)
    inp = dict(kappa=kappa if dispersion else np.zeros_like(kappa), a0=a0, gamma=gamma, alpha=alpha, z_max=LONG_Z,
               n_steps=LONG_STEPS, save_every=10)
    return _long_set("comb", inp, inp["kappa"])


LONG_F64_SETS = ([(f"g8-1e5-{'mirrored' if m else 'general'}-a{a}", lambda m=m, a=a: g8_long(m, a)) for m in (False, True)
                  for a in (0, 1)]
                 + [("g8-1e5-mirrored-a1-save_every-7", lambda: g8_long(True, 1, 7)), ("waves6-1e5", waves6_long),
                    ("pairs-1e5-K3", lambda: pairs_long(3)), ("pairs-1e5-K16", lambda: pairs_long(16)),
                    ("single_pump-1e5", single_pump_long), ("comb-1e5-M4", lambda: comb_long(4)),
                    ("comb-1e5-M7", lambda: comb_long(7)), ("comb-1e5-M7-kappa0", lambda: comb_long(7, False))])


# ---- float32 against a compensated twin ---------------------------------------------------------------------------------------
# The second float32 bar: beside "no worse than a PLAIN float32 RK4" (floor 2e-6), which a kernel that lost its compensated state
# altogether still meets, the kernel is held to the compensated float32 statement of its own kind -- Kahan per component for the
# scalar kernel, base + offset with a Fast2Sum fold every 16 steps for the packed ones -- with no floor:
#     median(e_gpu) <= F32C_MED median(e_twin_c)   and   max(e_gpu) <= F32C_MAX max(e_twin_c)
# The factors are 4 and 8 where the spread between the two compensated statements is at most a third of them, as the float64
# factors were set from the spread of two plain float64 statements, and three times the measured spread where it is more;
# tests/test_truth_long_host.py measures the spread on every set below and asserts it (record: profiles/truth_errors.txt).
#   a_end, p_wave_end, p_wave_max (every wave's power, scaled to the point's largest wave): medians within 1.28x, maxima within
#       1.56x of each other -> 4 and 8.
#   p_end, p_max (wave 2's power ALONE, what a launch without the per-wave summary returns -- the benchmark's): maxima within
#       1.22x -> 8; medians up to 3.2345x apart (0.5 / 0.4 W pumps, 1e5 steps: a sideband far below the pumps is known to 1e-9 of
#       the point's largest modulus by either statement, no better) -> 3 x 3.2345 = 9.71, rounded up in the third digit.
# Neither factor comes from a kernel's figures.
F32C_MED, F32C_MAX = 4.0, 8.0
F32C_ONE_WAVE_MED, F32C_ONE_WAVE_MAX = 9.71, 8.0
COMPENSATED = ("kahan", "base_offset")


def factors_compensated(key):
    """-> (F_med, F_max) of the second float32 bar for the output ``key``."""
    return (F32C_ONE_WAVE_MED, F32C_ONE_WAVE_MAX) if key in ("p_end", "p_max") else (F32C_MED, F32C_MAX)


def bar_compensated(e_got, e_twin_c, key):
    """-> (passes, median ratio, max ratio): the second float32 bar on the output ``key``, no floor."""
    med, mx, tmed, tmx = float(np.median(e_got)), float(np.max(e_got)), float(np.median(e_twin_c)), float(np.max(e_twin_c))
    f_med, f_max = factors_compensated(key)
    return med <= f_med * tmed and mx <= f_max * tmx, med / tmed, mx / tmx


def judge_compensated(family, case, got, inputs, kind):
    """The record line of the second bar and -> the outputs that miss it, in judge's form."""
    e_got, e_twin = errors(got, inputs["truth"]), errors(like(got, inputs[kind]), inputs["truth"])
    missed = {}
    for key, e in e_got.items():
        ok, r_med, r_max = bar_compensated(e, e_twin[key], key)
        line = (f"{key}: kernel median {np.median(e):.2e} max {e.max():.2e}, {kind} twin median {np.median(e_twin[key]):.2e} "
                f"max {e_twin[key].max():.2e}, ratio {r_med:.2f} / {r_max:.2f} (factors {factors_compensated(key)[0]:g} / "
                f"{factors_compensated(key)[1]:g})")
        print(f"\ntruth | {family} | {case} | compensated bar{'' if ok else ' MISSED'} | {line}", end="")
        if not ok:
            missed[key] = (line, float(np.median(e)), float(e.max()), float(np.median(e_twin[key])), float(e_twin[key].max()))
    print()
    return missed


def _f32_set(model, inp, rate, truth=None, twin=None):
    """inp: float32-rounded inputs.  truth: the C double run of them; twin: the plain float32 statement; kahan, base_offset: the
    compensated ones; no_residue: base + offset with the fold's residue thrown away (the planted defect of the host test)."""
    out = dict(inp, truth=truth if truth is not None else _plain(model, inp, rate, "f64"),
               twin=twin if twin is not None else _plain(model, inp, rate, "f32"))
    for update in COMPENSATED + ("base_offset_no_residue",):
        out[update] = _plain(model, inp, rate, "f32", update)
    return out


@functools.lru_cache(maxsize=None)
def waves4_f32_compensated(mirrored):
    """waves4_f32's set (its 80-bit truth and NumPy plain twin kept) with the compensated statements."""
    s = waves4_f32(mirrored)
    return _f32_set("pairs", {k: v for k, v in s.items() if k not in ("truth", "twin")}, s["dbeta"], s["truth"], s["twin"])


@functools.lru_cache(maxsize=None)
def single_pump_f32_compensated():
    s = single_pump_f32()
    return _f32_set("single_pump", {k: v for k, v in s.items() if k not in ("truth", "twin")}, s["dbeta"], s["truth"], s["twin"])


def _config4_like(p_in, n_steps, extra_pairs=0):
    inp = dict(dbeta=np.linspace(-0.02, 0.02, F32_N), gamma=GAMMA, alpha=ALPHA, z_max=LONG_Z, n_steps=n_steps, save_every=10,
               a0=np.repeat(np.sqrt(np.asarray(p_in, dtype=float)).astype(complex)[None, :], F32_N, axis=0))
    inp = _rounded(inp)
    if extra_pairs:
        inp["dbeta2"] = np.linspace(0.015, -0.025, F32_N).astype(F32)
    return inp


@functools.lru_cache(maxsize=None)
def config4_f32(kind, n_steps):
    """Config 4's shape at 17 points: dbeta from -0.02 to 0.02 over 1000 m, rows every 10 steps.  kind: "mirrored" p_in = (0.1, 0.1,
    1e-7, 1e-7), the benchmark's; "general" (0.1, 0.08, 1e-7, 1e-7); "strong" 0.5 and 0.4 W pumps with 1e-5 W sidebands (general);
    "six" the general powers with a second pair at its own mismatch."""
    p_in = dict(mirrored=(0.1, 0.1, 1e-7, 1e-7), general=(0.1, 0.08, 1e-7, 1e-7), strong=(0.5, 0.4, 1e-5, 1e-5),
                six=(0.1, 0.08, 1e-7, 1e-7, 1e-7, 1e-7))[kind]
    inp = _config4_like(p_in, n_steps, extra_pairs=kind == "six")
    return _f32_set("pairs", inp, _rate2(inp))


@functools.lru_cache(maxsize=None)
def single_pump_f32_long(n_steps):
    """A 0.1 W pump with 1e-7 W sidebands, dbeta across the gain band (-4.5 .. 0.5 times gamma P)."""
    inp = _rounded(dict(dbeta=np.linspace(-4.5, 0.5, F32_N) * GAMMA * 0.1, gamma=GAMMA, alpha=ALPHA, z_max=LONG_Z, n_steps=n_steps,
                        save_every=10, a0=np.repeat(np.sqrt(np.array([0.1, 1e-7, 1e-7])).astype(complex)[None, :], F32_N, axis=0)))
    return _f32_set("single_pump", inp, inp["dbeta"])


# (name, set, the compensated statement of the kernels that run it)
F32_COMPENSATED_SETS = (
    [("waves4_f32-general-1500", lambda: waves4_f32_compensated(False)), ("waves4_f32-mirrored-1500", lambda: waves4_f32_compensated(True)),
     ("single_pump_f32-1500", single_pump_f32_compensated)]
    + [(f"config4-{kind}-{n}", lambda kind=kind, n=n: config4_f32(kind, n))
       for kind, n in (("mirrored", 100_000), ("mirrored", 1_000_000), ("general", 100_000), ("general", 1_000_000),
                       ("strong", 100_000), ("six", 100_000))]
    + [(f"single_pump_f32-{n}", lambda n=n: single_pump_f32_long(n)) for n in (100_000, 1_000_000)])


# ---- every float64 input set, for the CPU test that pins the twins ---------------------------------------------------------
F64_SETS = ([(f"waves4-{'mirrored' if m else 'general'}-{'lossy' if l else 'lossless'}", lambda m=m, l=l: waves4(m, l))
             for m in (False, True) for l in (True, False)]
            + [(f"g8-{'mirrored' if m else 'general'}-a{a}", lambda m=m, a=a: g8(m, a)) for m in (False, True) for a in (0, 1)]
            + [("waves6", waves6)]
            + [(f"pairs-K{K}", lambda K=K: pairs(K)) for K in (1, 2, 3, 5, 8, 16)]
            + [(f"single_pump-{'lossy' if l else 'lossless'}", lambda l=l: single_pump(l)) for l in (True, False)]
            + [(f"comb-M{M}-lossy", lambda M=M: comb(M, True)) for M in range(3, 13)]
            + [(f"comb-M{M}-lossless", lambda M=M: comb(M, False)) for M in (3, 7, 10, 12)]
            + [(f"chain-{f}", lambda f=f: chain(f)) for f in ("waves", "single_pump", "pairs", "comb")]
            + [(f"waves4-{'mirrored' if m else 'general'}-dbeta0", lambda m=m: waves4_without_mismatch(m)) for m in (False, True)]
            + [("comb-M7-kappa0", lambda: comb_without_dispersion(7))])
F32_SETS = [("waves4_f32-general", lambda: waves4_f32(False)), ("waves4_f32-mirrored", lambda: waves4_f32(True)),
            ("single_pump_f32", single_pump_f32)]


# ---- three-span chains of the 4/6-wave model, float64 and float32 ----------------------------------------------------------
# What chain("waves") leaves out: six waves with transfers on both pairs (theta2 / dbeta2 of the chain epilogue), the forced lane
# layouts, the per-wave summary, float32, and spans that end before the first re-seed (64 steps in float64, 16 in float32) --
# in float32 before the first base + offset fold as well, so that the boundary carries a base with an unfolded offset.
#   float64: 460 + 40 + 1000 steps over 92 + 10 + 240 m, rows every 20: the middle span is two rows long, no span a multiple of 64.
#   float32: 460 + 12 + 1028 steps over 92 + 3 + 246.72 m, rows every 4; the float32-rounded inputs are what is integrated.
# The yardstick is truth_ld.chain, the accumulated-phase model in the physical frame; the twins restate the kernels' B gauge
# (psa_chain.hip) span by span on the compiled plain RK4, so their agreement checks the gauge and not only the arithmetic.
CHAIN3_SHAPES = {False: ((460, 40, 1000), (92.0, 10.0, 240.0), 20), True: ((460, 12, 1028), (92.0, 3.0, 246.72), 4)}
CHAIN3_KINDS = ((4, False), (4, True), (6, False))        # (n_waves, mirrored)


def chain3_name(n_waves, mirrored, float32=False):
    return f"chain3{'_f32' if float32 else ''}-{'waves6' if n_waves == 6 else 'mirrored' if mirrored else 'general'}"


def chain3_inputs(n_waves, mirrored, float32):
    """-> a0 (N, NW), spans [(length, n_steps, dbeta (N, K), gamma (N,), alpha (N,))], transfers [2 x (N, NW)], save_every; K =
    1 or 2, column 0 of a span's dbeta the first pair's mismatch and column 1 the second's.  mirrored: A2 == A1 and A4 == A3 in
    a0 and in both transfers -- span 0 is mirrored, and the gauge phase of the first boundary ends that."""
    steps, lengths, save_every = CHAIN3_SHAPES[bool(float32)]
    rng = np.random.default_rng((4900 if float32 else 4800) + n_waves + mirrored)
    K = (n_waves - 2) // 2
    a0 = _amplitudes(rng, N, 2, 2 * K)
    if mirrored:
        a0[:, 1], a0[:, 3] = a0[:, 0], a0[:, 2]
    spans = [(L, n, rng.uniform(-0.05, 0.05, (N, K)), GAMMA * rng.uniform(0.8, 1.6, N), ALPHA * rng.uniform(0.5, 2.0, N))
             for L, n in zip(lengths, steps)]
    transfers = [_mid_stage(rng, (N, n_waves)) for _ in range(2)]
    if mirrored:
        for t in transfers:
            t[:, 1], t[:, 3] = t[:, 0], t[:, 2]
    if float32:
        a0, transfers = a0.astype(C64), [t.astype(C64) for t in transfers]
        spans = [(L, n, db.astype(F32), g.astype(F32), al.astype(F32)) for L, n, db, g, al in spans]
    return dict(a0=a0, spans=spans, transfers=transfers, save_every=save_every)


def _clear_low_bits(x, bits=12):
    """A float64 array with the low ``bits`` of every mantissa cleared."""
    out = np.array(x, dtype=np.float64)
    out.view(np.uint64)[...] &= ~np.uint64((1 << bits) - 1)
    return out


def chain_b_gauge(inp, precision, update="plain", later_update=None, phase=lambda ph: ph, span_run=None):
    """The chain as psa_chain.hip's header states it, on oracle/plain_rk4.py (model "pairs"): every span runs on its local
    coordinate from the current B state; its rows come back to A with e^{-i Theta^(k)} on wave 2 + 2k; at a boundary the signal
    columns are multiplied by e^{+i dbeta_{s,k} L_s}, then every wave by its transfer, and Theta^(k) += dbeta_{s,k} L_s.  Theta
    and all boundary arithmetic are float64; precision "f32" rounds to complex64 after the rotation and again after the
    transfer, as the epilogue does, and rounds the rotated rows.
    later_update: the state update of spans >= 1 where it is not ``update`` (planted: a compensation lost at the first boundary).
    phase: applied to the boundary phase dbeta_s L_s before it is used and accumulated (planted: low bits cleared).
    span_run: another statement of one span in the place of the compiled one: f(b, dbeta (N, K), z_max=, n=, save_every=, gamma=,
    alpha=) -> the result dict with its rows.
    -> the result dict: a_end and rows in the A frame; the powers are the spans' own, phase-blind and so taken in B as the
    epilogue folds them (the last span's end, the maximum over the spans)."""
    import plain_rk4
    cplx = C64 if precision == "f32" else np.complex128
    b = np.asarray(inp["a0"], dtype=np.complex128)
    n_pts, nw = b.shape
    theta, rows, p_max = np.zeros((n_pts, (nw - 2) // 2)), [], None
    for s, (length, n, dbeta, gamma, alpha) in enumerate(inp["spans"]):
        dbeta = np.asarray(dbeta, dtype=np.float64).reshape(n_pts, -1)
        kw = dict(z_max=length, n=n, save_every=inp["save_every"], gamma=gamma, alpha=alpha)
        span = span_run(b, dbeta, **kw) if span_run else plain_rk4.integrate(
            "pairs", b, dbeta, precision=precision, update=update if s == 0 or later_update is None else later_update,
            want_rows=True, **kw)
        B = span["rows"]
        assert B.dtype == cplx
        p_max = span["p_wave_max"] if p_max is None else np.maximum(p_max, span["p_wave_max"])
        A = B.astype(np.complex128)
        if s:
            A[:, :, 2::2] *= np.exp(-1j * theta)[:, None, :]
        rows.append(A.astype(cplx))
        if s + 1 < len(inp["spans"]):
            ph = phase(dbeta * length)
            b = B[:, -1].astype(np.complex128)
            b[:, 2::2] *= np.exp(1j * ph)
            b = b.astype(cplx).astype(np.complex128) * np.asarray(inp["transfers"][s], dtype=np.complex128)
            b = b.astype(cplx).astype(np.complex128)
            theta = theta + ph
    rows = np.concatenate(rows, axis=1)
    return dict(a_end=rows[:, -1], p_wave_end=span["p_wave_end"], p_wave_max=p_max, rows=rows)


def _chain3_truth(inp):
    return T.chain(T.rhs_waves, inp["a0"], inp["spans"], inp["transfers"], inp["save_every"])


@functools.lru_cache(maxsize=None)
def chain3(n_waves, mirrored):
    """The float64 set: the 80-bit run, the B-gauge twin, and ``short_phase``, the twin with the low 12 mantissa bits of every
    boundary phase (and so of Theta) cleared -- the planted defect of the host test."""
    inp = chain3_inputs(n_waves, mirrored, False)
    return dict(inp, truth=_chain3_truth(inp), twin=chain_b_gauge(inp, "f64"),
                short_phase=chain_b_gauge(inp, "f64", phase=_clear_low_bits))


@functools.lru_cache(maxsize=None)
def chain3_f32(n_waves, mirrored):
    """The float32 set in _f32_set's form (twin: the plain float32 chain; kahan, base_offset, base_offset_no_residue), with the
    80-bit run of the rounded inputs as the yardstick, and the planted defect of the host test under "<kind>_lost": the
    compensation kept in span 0 and dropped from the first boundary on."""
    inp = chain3_inputs(n_waves, mirrored, True)
    out = dict(inp, truth=_chain3_truth(inp), twin=chain_b_gauge(inp, "f32"))
    for update in COMPENSATED + ("base_offset_no_residue",):
        out[update] = chain_b_gauge(inp, "f32", update)
    for update in COMPENSATED:
        out[update + "_lost"] = chain_b_gauge(inp, "f32", update, later_update="plain")
    return out


F32_RESYNC = 16                        # psa_rk4_kernel.inc.h: the float32 kernels re-seed their carried phase factor every 16 steps


@functools.lru_cache(maxsize=None)
def chain3_f32_kahan_np(carried):
    """The four-wave general float32 chain once more, in NumPy with the scalar kernel's Kahan update (rk4_f32): with cos / sin at
    every stage -- a third compensated statement -- or with ONE thing planted, the phase factor carried as the float32 kernels
    carry it.  What places the finding of test_gpu_truth.test_chain_of_three_spans_float32 (CARRIED_E_F32 there)."""
    def span_run(b, dbeta, **kw):
        return rk4_f32(_rhs32_waves, b, dbeta[:, 0], kahan=True, carried_for=F32_RESYNC if carried else 0, **kw)
    return chain_b_gauge(chain3_inputs(4, False, True), "f32", span_run=span_run)


def chain3_signal_report(p_end, p_max, rows, s):
    """Where wave 2's power alone is worst in a run of a chain3 set, as one readable line: the point with the largest p_max
    error and the next one, with their p_end / p_max errors; at the worst point the mismatch of the last span, how far the signal
    grows (its largest modulus over the point's largest), and the error of the signal's modulus in the saved rows at the start of
    the last span and at its largest inside it -- whether the error arrives over a boundary or grows within the span."""
    e = errors(dict(a_end=s["truth"]["a_end"], p_end=p_end, p_max=p_max), s["truth"])
    first, second = (int(j) for j in np.argsort(e["p_max"])[::-1][:2])
    mod = np.sqrt(s["truth"]["p_wave_max"][first])
    start = sum(n // s["save_every"] + 1 for _, n, *_ in s["spans"][:-1])
    in_rows = np.asarray(np.abs(np.abs(np.asarray(rows)[first, :, 2].astype(T.CLD)) - np.abs(s["truth"]["rows"][first, :, 2]))
                         / mod.max(), dtype=np.float64)
    return (f"wave 2's power alone is worst at point {first}: p_end {e['p_end'][first]:.2e} p_max {e['p_max'][first]:.2e}, last span dbeta "
            f"{float(s['spans'][-1][2][first, 0]):.4f} 1/m over {s['spans'][-1][1]} steps, signal up to {float(mod[2] / mod.max()):.2f} of the "
            f"largest wave, its modulus in the rows {in_rows[start]:.2e} off at the start of the last span and up to "
            f"{in_rows[start:].max():.2e} inside it; next point {second}: p_end {e['p_end'][second]:.2e} p_max {e['p_max'][second]:.2e}")


def _rhs_waves_coupling_off_by(delta):
    """truth_ld.rhs_waves with every FWM term scaled by 1 + delta: a phase factor E = 2 gamma exp(i theta) whose modulus is off."""
    def f(theta, a, gamma, alpha):
        full = T.rhs_waves(theta, a, gamma, alpha)
        P = T.power(a)
        without = (-(alpha[:, None] / T.LD(2)) + T.I * gamma[:, None] * (T.LD(2) * P.sum(axis=1, keepdims=True) - P)) * a
        return full + T.LD(delta) * (full - without)
    return f


@functools.lru_cache(maxsize=None)
def chain3_f32_coupling_drift(n_waves, mirrored, off):
    """What a phase factor off by ``off`` in modulus -- the drift psa_rk4_kernel.inc.h's rule allows a carried factor between two
    seeds -- does to the outputs of chain3_f32's set, evaluated and not estimated as in g8_long_frame_drift: the 80-bit chain
    with every FWM term scaled by 1 + off, at every z and with one sign, against the clean one.  -> {output: (median, maximum)
    of its point_err over the points}: the budgets of a band's median and maximum, for both launches' outputs."""
    s = chain3_f32(n_waves, mirrored)
    planted = T.chain(_rhs_waves_coupling_off_by(off), s["a0"], s["spans"], s["transfers"], s["save_every"])
    e = errors(planted, s["truth"])
    e.update({k: v for k, v in errors(dict(a_end=planted["a_end"], p_end=planted["p_wave_end"][:, 2],
                                           p_max=planted["p_wave_max"][:, 2]), s["truth"]).items() if k != "a_end"})
    return {k: (float(np.median(v)), float(v.max())) for k, v in e.items()}


CHAIN3_F64_SETS = [(chain3_name(nw, m), lambda nw=nw, m=m: chain3(nw, m)) for nw, m in CHAIN3_KINDS]
CHAIN3_F32_SETS = [(chain3_name(nw, m, True), lambda nw=nw, m=m: chain3_f32(nw, m)) for nw, m in CHAIN3_KINDS]
F64_SETS += CHAIN3_F64_SETS


# ---- the adaptive sweep: Dormand-Prince 5(4) against the 80-bit run of its own scheme (truth_rk45_ld) ------------------------
# The yardstick is of the kernel's discrete scheme only where its controller takes the kernel's steps: twin (tests/rk45_np.py)
# and yardstick have identical status, n_accepted and n_rejected at every point of every set below (asserted in
# tests/test_truth_rk45_host.py; a set that ever fails it gets another seed).  atol = 1e-3 rtol unless a set says otherwise; rows
# at linspace(0, z_max, 44) -- 43 divides neither length, so no row but the last lies on a step end.
# The floor of this bar is NOT FLOOR_F64: that is the drift budget of a carried phase, and the adaptive kernel takes an exact sincos
# at every stage.  It is zero: two plain float64 statements meet the bar against each other on every set and every output without
# one (test_truth_rk45_host.test_spread_between_two_plain_statements).
RK45_N_OUT = 43
FLOOR_RK45 = 0.0
RK45_TWIN_RTOL = 1e-10                 # what tests/test_gpu_rk45.py holds kernel and twin to; kept beside the bar
RK45_KEYS = ("a_end", "p_end", "p_max", "p_wave_end", "p_wave_max", "status", "z_end", "n_accepted", "n_rejected", "rows")


def rk45_random_points(n, seed, six=False):
    """The seeded random sweep of tests/test_gpu_rk45.py: -> dbeta, gamma, a0 (n, 4 or 6), dbeta2 or None.  The strong set
    below is its first 67 points, so the draws stay as they are."""
    rng = np.random.default_rng(seed)
    db = rng.uniform(-0.1, 0.1, n)
    gamma = rng.uniform(5e-3, 2e-2, n)
    pp = rng.uniform(0.05, 1.0, (n, 2))
    nw = 6 if six else 4
    p = np.concatenate([pp, np.full((n, nw - 2), 1e-5)], axis=1)
    return db, gamma, np.sqrt(p).astype(complex), (rng.uniform(-0.1, 0.1, n) if six else None)


def rk45_form(result, rows=True):
    """A run of rk45_np.rk45 or nat.rk45_sweep_host in the yardstick's form: the outputs above, its dense rows ("traj" there)
    under "rows"; rows = False leaves them out, as a launch with n_out = 0 does."""
    out = {k: result[k] for k in RK45_KEYS[:-1] if result.get(k) is not None}
    out["rows"] = (result.get("rows") if result.get("rows") is not None else result.get("traj")) if rows else None
    return out


def _rk45_set(inp):
    import rk45_np
    import truth_rk45_ld
    inp = dict(dict(rtol=1e-9, h_max=np.inf, first_step=0.0, n_out=RK45_N_OUT, z_max=Z_MAX), **inp)
    inp.setdefault("atol", 1e-3 * inp["rtol"])
    tol = {k: inp[k] for k in ("z_max", "rtol", "atol", "h_max", "first_step", "n_out")}
    truth = truth_rk45_ld.integrate(inp["a0"], _rate2(inp), gamma=inp["gamma"], alpha=inp["alpha"], **tol)
    rhs = (rk45_np.rhs4(inp["dbeta"], inp["gamma"], inp["alpha"]) if inp.get("dbeta2") is None
           else rk45_np.rhs6(inp["dbeta"], inp["dbeta2"], inp["gamma"], inp["alpha"]))
    return dict(inp, truth=truth, twin=rk45_form(rk45_np.rk45(rhs, inp["a0"].T, **tol)))


def _rk45_lossy_inputs():
    rng = np.random.default_rng(4700)
    gamma, alpha = _fibre(rng, N, True)
    return dict(dbeta=rng.uniform(-0.05, 0.05, N), gamma=gamma, alpha=alpha, a0=_amplitudes(rng, N, 2, 2))


def _rk45_six_inputs(lossy):
    rng = np.random.default_rng(4760 + lossy)
    gamma, alpha = _fibre(rng, N, lossy)
    return dict(dbeta=rng.uniform(-0.05, 0.05, N), dbeta2=rng.uniform(-0.05, 0.05, N), gamma=gamma, alpha=alpha,
                a0=_amplitudes(rng, N, 2, 4))


def _rk45_strong_inputs():
    """The first 67 points of the 4 096-point random sweep of tests/test_gpu_rk45.py over its 1000 m: gamma P L up to ~20 rad,
    up to ~1 600 steps, one alpha for all points."""
    db, gamma, a0, _ = rk45_random_points(4096, 20261016)
    return dict(dbeta=db[:N], gamma=gamma[:N], alpha=ALPHA, a0=a0[:N], z_max=1000.0, rtol=1e-9, atol=1e-12)


def _rk45_lossless_inputs():
    rng = np.random.default_rng(4710)
    gamma, alpha = _fibre(rng, N, False)                   # the scalar 0.0: the LOSSLESS instantiation
    return dict(dbeta=rng.uniform(-0.05, 0.05, N), gamma=gamma, alpha=alpha, a0=_amplitudes(rng, N, 2, 2))


RK45_INPUTS = {
    "lossy-r9": lambda: _rk45_lossy_inputs(),                                        # per-point gamma and alpha, ~150 steps
    "lossless-r9": _rk45_lossless_inputs,
    "lossy-r6": lambda: dict(_rk45_lossy_inputs(), rtol=1e-6),                       # the tolerance ends: ~20 steps ...
    "lossy-r11": lambda: dict(_rk45_lossy_inputs(), rtol=1e-11),                     # ... and ~500
    "lossy-dbeta0": lambda: dict(_rk45_lossy_inputs(), dbeta=np.zeros(N)),
    "strong-r9": _rk45_strong_inputs,
    "six-lossy-r9": lambda: _rk45_six_inputs(True),                                  # the instantiations that use AGPRs
    "six-lossless-r9": lambda: _rk45_six_inputs(False),
    # the controller's other branches: rejections (1..3 per point, then factor <= 1), the h_max clamp on every step, both
    "first_step50-r4": lambda: dict(_rk45_lossy_inputs(), first_step=50.0, rtol=1e-4, atol=1e-9),
    "h_max1.3-r9": lambda: dict(_rk45_lossy_inputs(), h_max=1.3),
    "first_step100-h_max7-r7": lambda: dict(_rk45_lossy_inputs(), first_step=100.0, h_max=7.0, rtol=1e-7),
}
RK45_SETS = tuple(RK45_INPUTS)


@functools.lru_cache(maxsize=None)
def rk45(name):
    """One input set of the adaptive sweep with its 80-bit run and its twin's, both in the kernel's output form."""
    return _rk45_set(RK45_INPUTS[name]())


def rk45_tolerances(inputs):
    """The set's controller settings as nat.rk45_sweep_host and rk45_np.rk45 take them."""
    return {k: inputs[k] for k in ("z_max", "rtol", "atol", "h_max", "first_step")}


def rk45_same_steps(got, truth):
    """The points where ``got`` took the yardstick's accepted and rejected attempts: where the two are one discrete scheme."""
    return (np.asarray(got["n_accepted"]) == truth["n_accepted"]) & (np.asarray(got["n_rejected"]) == truth["n_rejected"])


def rk45_at(result, mask):
    """The arrays of a result in the yardstick's form (rk45_form) at the points of ``mask``."""
    return {k: (None if result.get(k) is None else np.asarray(result[k])[mask]) for k in RK45_KEYS if k in result}
