"""Multi-line ("comb") fibre chains without a GPU: the every-line gauge on the NumPy restatement (tests/comb_chain_np.py) against
a direct integration of the accumulated-phase model, against the unsplit fibre, against the single-pump chain (M = 3) and
against the single-pump copier - PSA closed form; a gauge of its own in every span; the failing case the GPU test leans on; the
argument rules of rk4_chain_comb, comb_mid_stage, run_concatenated_comb_simulation and scan_comb_copier_psa_phase; every
argument code of psa_rk4_comb_chain_f64 / _dev (all before any device call); the binding against the header; the workspace
size; the device split of a chain's points; the drivers' propagation constants per span."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import comb_chain_np as chain_np
import comb_np
import psa_amd._native as nat
import single_pump_chain_np
from psa_amd import scan_mismtach, simulation, sweep
from psa_amd._partition import PAIRS_CHAIN_AXES, cut
from psa_amd.config import custom_simulation_config
from psa_amd.dispersion import DispersionParams
from psa_amd.sweep import CombChainResult, CombResult, FibreSpan, rk4_chain_comb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NPOINTS, E_NSTEPS, E_ZMAX, E_SAVE_EVERY, E_NULLPTR, E_DEVICE, E_TOO_LARGE, E_FLAGS, E_NLINES = -2, -3, -4, -5, -6, -7, -9, -11, -14
A0 = np.sqrt(np.array([1e-5, 0.25, 0.25, 1e-6, 2e-5])).astype(complex)   # M = 5


def _scaled(got, want):
    n = want.shape[0]
    return float(np.max(np.abs(got - want) / np.abs(want).reshape(n, -1).max(axis=1).reshape((n,) + (1,) * (want.ndim - 1))))


# ---- the gauge on the restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [4, 7])
def test_gauge_reproduces_the_accumulated_phase_model(M):
    """8 random points through 3 lossy spans of 600, 1000 and 400 steps with per-point kappa (N, M), gamma and alpha and complex
    per-point transfers on every line: the B-frame run, span by span, against the direct RK4 of the accumulated-phase model at
    1e-12 of the point's largest line (measured 7.1e-15 at M = 4, 1.0e-14 at M = 7).  kappa L runs to several radians on the
    outer lines, so the same run without the boundary phase is off by order 1 (measured 0.95 and 0.21)."""
    a0, spans, transfers = chain_np.lossy_case(8, M)
    want = chain_np.direct(a0, spans, transfers, 50)
    got = chain_np.chain(a0, spans, transfers, 50)
    assert got["rows"].shape == want.shape == (8, sum(n // 50 + 1 for _, n, *_ in spans), M)
    err = _scaled(got["rows"], want)
    wrong = _scaled(chain_np.chain(a0, spans, transfers, 50, gauge=False)["rows"], want)
    print(f"M = {M}: gauge against the direct model: {err:.2e} of the largest line; without the boundary phase {wrong:.2e}")
    assert err < 1e-12
    assert wrong > 1e-3
    assert np.array_equal(got["a_end"], got["rows"][:, -1]) and (got["first_bad_step"] == -1).all()


@pytest.mark.parametrize("pieces", [2, 3, 7])
def test_a_split_fibre_is_the_unsplit_fibre(pieces):
    """One lossy fibre of 1 400 steps cut into 2, 3 or 7 spans joined by identity transfers: every row the chain shares with
    comb_np.integrate on the whole fibre within 1e-12 of the point's largest line (measured <= 2e-14), p_wave_max too."""
    rng = np.random.default_rng(40 + pieces)
    N, M, n = 6, 5, 1400
    a0, kp, g, al, spans = chain_np.split_fibre(rng, N, M, n, 700.0, pieces)
    assert sum(s[1] for s in spans) == n and abs(sum(s[0] for s in spans) - 700.0) < 1e-9 and len(spans) == pieces
    whole = comb_np.integrate(a0, kp, z_max=700.0, n=n, save_every=10, gamma=g, alpha=al, want_traj=True)
    got = chain_np.chain(a0, spans, [np.ones(M)] * (pieces - 1), 10)
    keep = np.ones(got["rows"].shape[1], dtype=bool)          # a boundary's row appears twice: drop each span's row 0 but the first
    keep[np.cumsum([s[1] // 10 + 1 for s in spans])[:-1]] = False
    err = max(_scaled(got["rows"][:, keep], whole["traj"]), _scaled(got["a_end"], whole["a_end"]),
              _scaled(got["p_wave_max"], whole["p_wave_max"]))
    print(f"{pieces} spans against the whole fibre: {err:.2e}")
    assert err < 1e-12


def test_three_lines_are_the_single_pump_chain():
    """Lines [s, p, i] with every span's dbeta split at random into kappa_0 + kappa_2 - 2 kappa_1 against
    single_pump_chain_np.chain on its lossy_case, within 1e-12 of the point's largest wave (measured 1.0e-14)."""
    case = single_pump_chain_np.lossy_case(8)
    a0, spans, transfers = chain_np.from_single_pump(case, np.random.default_rng(5))
    for (_, _, kp, *_), (_, _, db, *_) in zip(spans, case[1]):
        np.testing.assert_allclose(kp[:, 0] + kp[:, 2] - 2.0 * kp[:, 1], db, rtol=1e-12)
    got = chain_np.chain(a0, spans, transfers, 50)
    want = single_pump_chain_np.chain(*case, 50)
    err = max(_scaled(got["rows"], want["rows"][..., [1, 0, 2]]), _scaled(got["p_wave_max"], want["p_wave_max"][:, [1, 0, 2]]))
    print(f"M = 3 against the single-pump chain: {err:.2e}")
    assert err < 1e-12
    assert np.array_equal(got["first_bad_step"], want["first_bad_step"])


def test_every_span_may_have_a_gauge_of_its_own():
    """kappa_s + a_s + b_s m with another (a_s, b_s) in every span (a_s L_s, b_s L_s up to +-3 rad) leaves every power of
    every saved row and p_wave_max unchanged within 1e-12 of the point's largest (measured 8.4e-15), and the amplitudes A with
    them (8.1e-15): only kappa_k + kappa_l - kappa_n - kappa_m ever acts on A.  The B frame the spans are integrated in does
    move: a chain that forgot to rotate the rows back would show it."""
    a0, spans, transfers = chain_np.lossy_case(8, 6, seed=17)
    rng = np.random.default_rng(18)
    m = np.arange(6.0)
    moved = [(L, n, kp + rng.uniform(-3, 3, (8, 1)) / L + rng.uniform(-3, 3, (8, 1)) / L * m, g, al) for L, n, kp, g, al in spans]
    base, got = chain_np.chain(a0, spans, transfers, 50), chain_np.chain(a0, moved, transfers, 50)
    err = max(_scaled(np.abs(got["rows"]) ** 2, np.abs(base["rows"]) ** 2), _scaled(got["p_wave_max"], base["p_wave_max"]),
              _scaled(got["p_wave_end"], base["p_wave_end"]))
    amplitudes = _scaled(got["rows"], base["rows"])
    print(f"a gauge per span: powers move by {err:.2e}, amplitudes by {amplitudes:.2e}")
    assert err < 1e-12 and amplitudes < 1e-12
    forgot = chain_np.chain(a0, moved, transfers, 50, gauge=False)
    assert _scaled(np.abs(forgot["rows"]) ** 2, np.abs(base["rows"]) ** 2) > 1e-3


def test_the_failing_case_fails_in_span_two():
    """The case of the GPU failure test: gamma = 300 in span 2 at points 1 and 3 overflows at local step 1, span 1 is
    finite; a third span behind it changes nothing about first_bad_step."""
    a0, spans = chain_np.failing_case()
    first = chain_np.chain(a0, spans[:1], [], 10)
    assert (first["first_bad_step"] == -1).all() and np.all(np.isfinite(first["rows"]))
    ref = chain_np.chain(a0, spans, [np.ones(4)], 10)
    bad = ref["first_bad_step"]
    assert np.array_equal(bad, [-1, 401, -1, 401, -1])
    more = chain_np.chain(a0, spans + [(10.0, 100, spans[0][2], chain_np.GAMMA, 0.0)], [np.ones(4)] * 2, 10)
    assert np.array_equal(more["first_bad_step"], bad)


def test_restatement_against_the_single_pump_closed_form():
    """The signal gain of the lossless M = 3 copier - PSA link over F = 16 pump phases is a + b cos(2 phi + const): DFT bin 0
    and 2 |bin 2| of comb_chain_np.chain against the closed form, and every other bin over bin 0.  Measured 3.01e-9 / 3.31e-9 /
    1.74e-11 (the restatement's step error and the neglected depletion: the single-pump restatement's figures); the bars of
    tests/test_gpu_comb_chain.py are ten times the figures asserted here."""
    c = chain_np.closed_form_case()
    T = np.ones((c["phases"].size, 3), complex)
    T[:, 1] = np.exp(1j * c["phases"])
    r = chain_np.chain(c["a0"], [(L, n, c["kappa"], c["gamma"], 0.0) for L, n in zip(c["lengths"], c["steps"])], [T], 50)
    e0, e2, rest = single_pump_chain_np.check_harmonics(r["p_wave_end"][:, 0] / c["p_seed"], c["a"], c["b"])
    print(f"gain {c['a']:.3f} +- {c['b']:.3f}; bin 0 {e0:.2e}, bin 2 {e2:.2e}, the other bins {rest:.2e} of bin 0")
    assert e0 <= c["MEASURED"][0] and e2 <= c["MEASURED"][1] and rest <= c["MEASURED"][2]
    assert np.allclose(c["BARS"], 10.0 * np.array(c["MEASURED"]), rtol=1e-12)


# ---- argument rules of the Python layers (all raise before any native call) -------------------------------------------
def test_rk4_chain_comb_rules():
    def s(**kw):
        return [FibreSpan(10.0, n_steps=100, gamma=0.01, **dict(dict(dbeta=np.zeros(5)), **kw)) for _ in range(2)]
    with pytest.raises(ValueError, match="multiple of save_every"):
        rk4_chain_comb(s(), a0=A0, save_every=7)
    with pytest.raises(ValueError, match="non-empty"):
        rk4_chain_comb([], a0=A0)
    with pytest.raises(ValueError, match="dbeta2"):
        rk4_chain_comb(s(dbeta2=np.zeros(5)), a0=A0)
    with pytest.raises(ValueError, match="transfers"):
        rk4_chain_comb(s(), a0=A0, transfers=[np.ones(5), np.ones(5)])
    for width in (3, 4, 6, 10):
        with pytest.raises(ValueError, match="transfer must have shape"):
            rk4_chain_comb(s(), a0=A0, transfers=[np.ones(width)])
    # a span's propagation constants: (M,) for every point or (N, M); M comes from a0
    for bad in (0.0, np.zeros(4), np.zeros(6), np.zeros((5, 4)), np.zeros((5, 6)), np.zeros((2, 5, 5))):
        with pytest.raises(ValueError, match="dbeta must have shape"):
            rk4_chain_comb(s(dbeta=bad), a0=A0)
    with pytest.raises(ValueError, match="disagree"):
        rk4_chain_comb([FibreSpan(10.0, n_steps=100, dbeta=np.zeros((7, 5))), FibreSpan(10.0, n_steps=100, dbeta=np.zeros((4, 5)))], a0=A0)
    with pytest.raises(ValueError, match="disagree"):
        rk4_chain_comb(s(dbeta=np.zeros((7, 5))), a0=np.ones((4, 5)))
    with pytest.raises(ValueError, match="dbeta must have shape"):
        rk4_chain_comb(s(dbeta=np.zeros((1, 5)), alpha=np.zeros(7)), a0=A0)
    for a0 in (np.ones(2), np.ones(13), np.ones(1), np.ones((2, 2, 5))):
        with pytest.raises(ValueError, match="a0"):
            rk4_chain_comb(s(), a0=a0)
    with pytest.raises(ValueError, match="devices"):
        rk4_chain_comb(s(), a0=A0, devices=[])
    assert issubclass(CombChainResult, CombResult) and "rk4_chain_comb" in sweep.__all__ and "CombChainResult" in sweep.__all__


def test_comb_mid_stage():
    g = np.linspace(-3.0, 2.0, 7)
    t = simulation.comb_mid_stage(g, np.linspace(-1.0, 1.0, 7))
    np.testing.assert_allclose(np.abs(t) ** 2, 10.0 ** (g / 10.0), rtol=1e-15)
    np.testing.assert_allclose(np.angle(t), np.linspace(-1.0, 1.0, 7), rtol=1e-15)
    for M in range(3, 13):
        assert simulation.comb_mid_stage(np.zeros((7, M)), 0.0).shape == (7, M)
    assert np.array_equal(simulation.comb_mid_stage(np.zeros(3), np.zeros(3)), simulation.single_pump_mid_stage())
    for bad in ((np.zeros(2), 0.0), (np.zeros(13), 0.0), (0.0, 0.0), (np.full(5, np.nan), 0.0), (np.zeros(5), np.inf)):
        with pytest.raises(ValueError):
            simulation.comb_mid_stage(*bad)


def _dispersion(scale=1.0):
    return DispersionParams(omega_ref=2.0 * np.pi * 299792458.0 / 1554e-9, beta2=-2.3e-28 * scale, beta3=4.1e-41, beta4=-3.2e-55 * scale)


def test_scan_and_driver_input_errors():
    d = _dispersion()
    cfg = custom_simulation_config(z_max=10.0, dz=0.1)
    kw = dict(psa_cfg=cfg, lambda_center_m=1550e-9, line_spacing=6e11, p_lines=[1e-6, 0.3, 0.3, 1e-6], gamma=0.0115, alpha=0.0,
              dispersion=d, phase_lines=[1, 2])
    scan = scan_mismtach.scan_comb_copier_psa_phase
    for lines in ((), [4], [-1], [1, 1], [1.0], [True], "12", None, 1):
        with pytest.raises(ValueError, match="phase_lines"):
            scan(**dict(kw, phase_lines=lines))
    for ph in ([], np.zeros((2, 2)), [0.0, np.inf]):
        with pytest.raises(ValueError, match="phase must"):
            scan(**kw, phase=ph)
    with pytest.raises(ValueError, match="gain_mode"):
        scan(**kw, gain_mode="mean")
    with pytest.raises(ValueError, match="gain_unit"):
        scan(**kw, gain_unit="neper")
    for bad in (dict(p_lines=[0.3, 0.3]), dict(p_lines=np.ones(13)), dict(p_lines=[0.3, -1.0, 0.3]), dict(p_lines=np.ones((2, 4))),
                dict(p_lines=[0.3, np.nan, 0.3]), dict(phase_in=[0.0, 1.0]), dict(line_spacing=0.0), dict(line_spacing=1e15),
                dict(dispersion=None), dict(max_order=1), dict(mid_gain_db=np.zeros(3)), dict(mid_phase=np.zeros(8)),
                dict(length_unit="mi"), dict(devices=[])):
        with pytest.raises(ValueError):
            scan(**dict(kw, **bad))
    with pytest.raises(ValueError, match="share save_every"):
        scan(**kw, copier_cfg=custom_simulation_config(z_max=10.0, dz=0.1, save_every=5))
    with pytest.raises(ValueError, match="multiple of save_every"):
        scan(**kw, copier_cfg=custom_simulation_config(z_max=10.3, dz=0.1))
    run = dict(omega_center=1.2e15, line_spacing=6e11, p_in=[1e-3, 0.3, 0.3, 1e-3])
    span = dict(cfg=cfg, gamma=0.0115, alpha=0.0, dispersion=d)
    drive = simulation.run_concatenated_comb_simulation
    for bad in (dict(p_in=np.ones((2, 4))), dict(p_in=[0.3, 0.3]), dict(phase_in=[0.0] * 5), dict(omega_center=-1.0),
                dict(line_spacing=-1.0), dict(length_unit="mile"), dict(transfers=[np.ones(4)]), dict(transfers=[1.0])):
        with pytest.raises(ValueError):
            drive([span], **dict(run, **bad))
    for spans in ([], [dict(span, dispersion=None)], [dict(cfg=cfg, gamma=0.0115, dispersion=d)], [dict(span, beta_legacy=1.0)],
                  [span, dict(span, cfg=custom_simulation_config(z_max=10.0, dz=0.1, save_every=5))]):
        with pytest.raises(ValueError):
            drive(spans, **run)
    with pytest.raises(ValueError):
        drive([span, span], **dict(run, transfers=[np.ones(5)]))
    with pytest.raises(TypeError):
        drive([dict(span, max_order=4.0)], **run)


# ---- the C-ABI validates before touching a device -------------------------------------------------------------------
def _call(host, **over):
    """psa_rk4_comb_chain_f64 (host) or _dev with dummy pointers: every call here must end in validation."""
    buf = np.zeros(256)
    p = buf.ctypes.data_as(C.c_void_p)
    a = dict(M=5, n=8, S=2, steps=[10, 20], lens=[1.0, 2.0], se=5, flags=0, null=False, traj=False, ws=p)
    a.update(over)
    steps = None if a["steps"] is None else np.asarray(a["steps"], dtype=np.int64)
    lens = None if a["lens"] is None else np.asarray(a["lens"], dtype=np.float64)
    sp = None if steps is None else steps.ctypes.data_as(C.c_void_p)
    lp = None if lens is None else lens.ctypes.data_as(C.c_void_p)
    q, t = (None if a["null"] else p), (p if a["traj"] else None)
    L = nat.lib()
    if host:
        return L.psa_rk4_comb_chain_f64(0, a["M"], a["n"], a["S"], sp, lp, a["se"], p, p, p, p, None, a["flags"], p, p, q, p, t, None)
    return L.psa_rk4_comb_chain_f64_dev(None, a["M"], a["n"], a["S"], sp, lp, a["se"], q, p, p, p, None, a["flags"], p, p, p, p, t,
                                        a["ws"])


@pytest.mark.parametrize("host", [False, True], ids=["dev", "host"])
def test_every_argument_error_comes_back_before_any_device_call(host):
    call = lambda **over: _call(host, **over)   # noqa: E731
    # the line count is the first of the multi-line rules: before the grid, the flags and the pointers
    for M in (2, 13, 0, -1):
        assert call(M=M) == E_NLINES and call(M=M, n=-1, flags=nat.OPT_ONE_LANE, null=True, steps=[0, 20]) == E_NLINES, M
    assert b"n_lines" in nat.lib().psa_last_error()
    assert call(S=0) == E_NSTEPS and call(S=-1) == E_NSTEPS
    assert call(steps=None) == E_NULLPTR and call(lens=None) == E_NULLPTR
    assert call(n=-1) == E_NPOINTS and call(n=nat.MAX_POINTS + 1) == E_TOO_LARGE
    assert call(steps=[0, 20]) == E_NSTEPS and call(steps=[10, 0]) == E_NSTEPS and call(steps=[10, 5 * 2**29]) == E_NSTEPS
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert call(lens=[bad, 2.0]) == E_ZMAX and call(lens=[1.0, bad]) == E_ZMAX
    assert call(se=0) == E_SAVE_EVERY
    assert call(steps=[10, 21]) == E_SAVE_EVERY and call(steps=[11, 20]) == E_SAVE_EVERY
    # one span, too, ends on a saved row (the single-pump chain's rule)
    assert call(S=1, steps=[11], lens=[1.0]) == E_SAVE_EVERY and call(S=1, steps=[11], lens=[1.0], n=0) == E_SAVE_EVERY
    assert call(null=True) == E_NULLPTR
    for bit in (nat.OPT_ONE_LANE, nat.OPT_SPLIT_POINT, nat.OPT_QUAD_POINT, nat.OPT_F32_SCALAR, nat.OPT_F32_PACKED,
                nat.OPT_LDS_STAGING, 1 << 19, 1 << 30):
        assert call(flags=bit | nat.OPT_CHECK_NAN) == E_FLAGS, bit
    # the order: the span count and the two host arrays, n_lines, the first span's grid, the flags, the pointers, the later spans
    assert call(S=0, M=2) == E_NSTEPS and call(steps=None, M=2) == E_NULLPTR
    assert call(n=-1, flags=nat.OPT_ONE_LANE, null=True) == E_NPOINTS
    assert call(flags=nat.OPT_ONE_LANE, null=True) == E_FLAGS and call(null=True, steps=[10, 21]) == E_NULLPTR
    # a trajectory: ld * 16 < 2^32; without one the same size passes on to the next rule
    assert call(M=3, n=2**28, traj=True) == E_TOO_LARGE and call(M=12, n=2**28, traj=True) == E_TOO_LARGE
    assert call(n=2**28, null=True) == E_NULLPTR and call(n=2**28 - 1, traj=True, null=True) == E_NULLPTR
    assert len(nat.lib().psa_last_error()) > 0


def test_flags_and_workspace_of_the_two_forms():
    ok = nat.BCAST_GAMMA | nat.BCAST_ALPHA | nat.BCAST_A0 | nat.BCAST_TRANSFER | nat.OPT_CHECK_NAN | nat.OPT_EXACT_STEP \
        | nat.OPT_LOSSLESS | nat.OPT_BLOCK64
    # every accepted bit passes validation: the next rule (a NULL pointer) is the one that answers
    assert _call(False, flags=ok | nat.OPT_TRAJ_LD, null=True) == E_NULLPTR and _call(True, flags=ok, null=True) == E_NULLPTR
    # the padded leading dimension belongs to the chain's device form, not to its host form
    assert _call(True, flags=nat.OPT_TRAJ_LD) == E_FLAGS and _call(True, flags=nat.OPT_TRAJ_LD, traj=True) == E_FLAGS
    # more than one span needs the caller's workspace on the _dev form
    assert _call(False, ws=None) == E_NULLPTR and b"d_workspace" in nat.lib().psa_last_error()
    assert _call(False, n=0, ws=None) == 0


def test_an_empty_chain_is_a_successful_no_op():
    assert _call(False, n=0) == 0 and _call(True, n=0) == 0
    L = nat.lib()
    steps, lens = np.array([10], dtype=np.int64), np.array([1.0])
    sp, lp = steps.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p)
    assert L.psa_rk4_comb_chain_f64_dev(None, 5, 0, 1, sp, lp, 5, *([None] * 5), 0, *([None] * 6)) == 0
    assert L.psa_rk4_comb_chain_f64(0, 5, 0, 1, sp, lp, 5, *([None] * 5), 0, *([None] * 6)) == 0
    assert L.psa_rk4_comb_chain_f64(0, 2, 0, 1, sp, lp, 5, *([None] * 5), 0, *([None] * 6)) == E_NLINES


def test_workspace_bytes():
    """Phi [M][N] in one block (8 M N) and the span's first_bad_step (8 N), the next a0 and the span's a_end (16 M N each), the
    span's two per-line summaries (8 M N each), every slice rounded up to 256 B; -1 for a call no chain takes; monotone in M.
    The other families' sizes are what they were."""
    def want(m, n):
        al = lambda b: (b + 255) // 256 * 256   # noqa: E731
        return al(8 * m * n) + al(8 * n) + 2 * al(16 * m * n) + 2 * al(8 * m * n)
    for n in (0, 1, 5, 32, 300, 65536, 10**6 + 7):
        sizes = [nat.comb_chain_workspace_bytes(m, n) for m in range(3, 13)]
        assert sizes == [want(m, n) for m in range(3, 13)], n
        assert all(b >= a for a, b in zip(sizes, sizes[1:])) and (n < 32 or sizes[-1] > sizes[0])
    for m, n in ((2, 8), (13, 8), (0, 8), (-1, 8), (5, -1), (5, -2**40)):
        assert nat.lib().psa_rk4_comb_chain_workspace_bytes(m, n) == -1
    assert nat.chain_workspace_bytes(6, 300, np.float64, True) == 2 * 2560 + 2 * 28928 + 3 * 2560 + 2 * 14592
    assert nat.single_pump_chain_workspace_bytes(300) == 2 * 2560 + 2 * 14592 + 2 * 7424
    assert nat.pairs_chain_workspace_bytes(3, 300) == 7424 + 2560 + 2 * 38400 + 2 * 19200


_CTYPE = {"int": C.c_int, "int64_t": C.c_int64, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "double": C.c_double}


def test_the_binding_equals_the_header():
    """The three prototypes of include/psa_rk4.h, argument by argument, against the ctypes table; shaped like the multi-channel
    chain's trio; no new PSA_E_* code."""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "psa_rk4.h"), encoding="utf-8").read(), flags=re.S)
    for name, ret in (("psa_rk4_comb_chain_f64", "int"), ("psa_rk4_comb_chain_f64_dev", "int"),
                      ("psa_rk4_comb_chain_workspace_bytes", "int64_t")):
        m = re.search(r"\b" + ret + r"\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
        assert m, name
        args = []
        for decl in m.group(1).split(","):
            decl = decl.strip()
            args.append(C.c_void_p if "*" in decl else _CTYPE[decl.replace("const ", "").split()[0]])
        res, want = nat._SIGS[name]
        assert res is _CTYPE[ret] and list(want) == args, name
        assert name in nat.EXPORTED_SYMBOLS and hasattr(nat.lib(), name)
        assert list(want) == list(nat._SIGS[name.replace("comb_chain", "pairs_chain")][1])
    assert len(nat._SIGS["psa_rk4_comb_chain_f64"][1]) == 19
    codes = [int(x) for x in re.findall(r"#define\s+PSA_E_\w+\s+\(?(-\d+)\)?", src)]      # -14 is written (-14)
    assert sorted(codes) == list(range(-14, 0))


@pytest.mark.skipif(nat.device_count() > 0, reason="CPU box only")
def test_without_a_device_a_valid_call_is_an_error_not_a_fallback():
    for S in (1, 2):
        with pytest.raises(nat.PsaNativeError) as e:
            nat.comb_chain_host(np.zeros((S, 3, 4)), n_steps=[1] * S, seg_len=[1.0] * S, save_every=1, gamma=[1.0] * S,
                                alpha=[0.0] * S, a0=np.ones(4, complex), want_traj=True)
        assert e.value.code == E_DEVICE and "no CPU fallback" in str(e.value)


def test_native_wrapper_shape_rules():
    kw = dict(dbeta=np.zeros((2, 3, 4)), n_steps=[1, 1], seg_len=[1.0, 1.0], save_every=1, gamma=[1.0, 1.0], alpha=[0.0, 0.0],
              a0=np.ones(4, complex))
    for bad in (dict(dbeta=np.zeros((2, 3))), dict(dbeta=np.zeros((2, 3, 13))), dict(dbeta=np.zeros((2, 3, 2))), dict(n_steps=[1]),
                dict(seg_len=[1.0] * 3), dict(gamma=[1.0]), dict(alpha=np.zeros((2, 2))), dict(a0=np.ones(5, complex)),
                dict(a0=np.ones((2, 4), complex)), dict(transfers=np.ones((1, 5), complex)),
                dict(transfers=np.ones((2, 3, 4), complex))):
        with pytest.raises(ValueError):
            nat.comb_chain_host(**dict(kw, **bad))
    with pytest.raises(ValueError):
        nat.comb_chain_device(stream=0, n_lines=4, n_points=1, n_steps=[1, 2], seg_len=[1.0], save_every=1, d_kappa_soa=0,
                              d_gamma=0, d_alpha=0, d_a0_soa=0, d_transfer_soa=0, flags=0, d_a_end_soa=0, d_p_wave_end_soa=0,
                              d_p_wave_max_soa=0, d_first_bad=0)


# ---- devices=[...] ------------------------------------------------------------------------------------------------------
def test_devices_list_splits_the_chain_points_over_threads(monkeypatch):
    """rk4_chain_comb(devices=[...]) without a GPU: a spy in place of the native call sees contiguous blocks (4, 4, 3 of 11
    points), the (S, N, M) propagation constants cut on axis 1 and every other per-point argument on its axis of
    PAIRS_CHAIN_AXES, broadcast ones whole; the outputs come back concatenated in point order."""
    seen = []

    def spy(dbeta, *, device, n_steps, seg_len, gamma, alpha, a0, transfers=None, **kw):
        n, M = dbeta.shape[1], dbeta.shape[2]
        assert set(kw) == {"save_every", "check_nan", "exact_step", "want_traj"}
        seen.append((int(device), n, dbeta.shape, np.shape(gamma), np.shape(alpha), a0.shape,
                     None if transfers is None else transfers.shape, np.shape(n_steps)))
        rows = int(np.sum(np.asarray(n_steps) // kw["save_every"] + 1))
        return dict(a_end=np.broadcast_to(np.asarray(a0, dtype=complex), (n, M)).copy(), p_wave_end=dbeta[0].copy(),
                    p_wave_max=np.abs(np.broadcast_to(a0, (n, M))) + 0.0, first_bad_step=np.full(n, -1, dtype=np.int64),
                    traj=np.zeros((n, rows, M), complex) if kw["want_traj"] else None, elapsed_ms=float(device) + 1.0)

    monkeypatch.setattr(nat, "comb_chain_host", spy)
    rng = np.random.default_rng(4)
    N, M = 11, 5
    kp0, gam1 = rng.uniform(-0.02, 0.02, (N, M)), rng.uniform(5e-3, 2e-2, N)
    a0 = np.sqrt(rng.uniform(1e-5, 0.5, (N, M))).astype(complex)
    T = np.exp(1j * rng.uniform(-3, 3, (N, M))) * rng.uniform(0.5, 1.5, (N, M))
    spans = [FibreSpan(10.0, n_steps=100, dbeta=kp0, gamma=0.01, alpha=1e-4),
             FibreSpan(20.0, n_steps=200, dbeta=np.arange(5.0) * 1e-3, gamma=gam1, alpha=2e-4),
             FibreSpan(5.0, n_steps=50, dbeta=np.zeros(5), gamma=0.01, alpha=1e-4)]
    one = rk4_chain_comb(spans, a0=a0, transfers=[T, np.ones(M)], devices=[0])
    assert seen == [(0, N, (3, N, M), (3, N), (3,), (N, M), (2, N, M), (3,))]
    seen.clear()
    many = rk4_chain_comb(spans, a0=a0, transfers=[T, np.ones(M)], devices=[0, 1, 2])
    assert sorted(seen) == [(d, n, (3, n, M), (3, n), (3,), (n, M), (2, n, M), (3,)) for d, n in ((0, 4), (1, 4), (2, 3))]
    assert PAIRS_CHAIN_AXES["dbeta"] == (1, 3)
    part = cut(dict(dbeta=np.arange(3.0 * N * M).reshape(3, N, M)), PAIRS_CHAIN_AXES, N, slice(4, 8))
    assert np.array_equal(part["dbeta"], np.arange(3.0 * N * M).reshape(3, N, M)[:, 4:8])
    assert np.array_equal(many.a_end, a0) and np.array_equal(many.p_wave_end, kp0) and many.traj is None and many.elapsed_ms == 3.0
    assert isinstance(many, CombChainResult) and isinstance(many, CombResult)
    assert many.n_steps == 350 and many.save_every == 10 and np.array_equal(many.p_wave_in, np.abs(a0) ** 2)
    assert np.array_equal(many.step_offsets, [0, 100, 300, 350]) and np.array_equal(many.row_offsets, [0, 11, 32, 38])
    np.testing.assert_allclose(many.z_out[[0, 10, 11, 31, 32, 37]], [0.0, 10.0, 10.0, 30.0, 30.0, 35.0], rtol=1e-15)
    for f in ("a_end", "p_wave_end", "p_wave_max", "first_bad_step", "z_out", "row_offsets", "step_offsets"):
        assert np.array_equal(getattr(one, f), getattr(many, f)), f
    assert many.line_gain(np.full(M, 1e-5), mode="end", unit="linear").shape == (N, M) and many.total_power().shape == (N,)


# ---- the drivers' propagation constants, span by span ----------------------------------------------------------------------
def _fake_result(spans, a0, transfers=None, save_every=10, **kw):
    a0 = np.atleast_2d(np.asarray(a0, dtype=complex))
    N = max([a0.shape[0]] + [np.shape(s.dbeta)[0] for s in spans if np.ndim(s.dbeta) == 2])
    M = a0.shape[1]
    steps = np.array([s.n_steps for s in spans])
    rows = int(np.sum(steps // save_every + 1))
    p = np.broadcast_to(np.abs(a0) ** 2, (N, M)).copy()
    return CombChainResult(np.broadcast_to(a0, (N, M)).copy(), 2.0 * p, 3.0 * p, np.full(N, -1, dtype=np.int64), int(steps.sum()),
                           save_every, 0.0, np.abs(a0) ** 2, np.zeros((N, rows, M), complex), z_out=np.zeros(rows),
                           row_offsets=np.zeros(len(spans) + 1, dtype=np.int64),
                           step_offsets=np.concatenate([[0], np.cumsum(steps)]).astype(np.int64))


def test_the_drivers_take_every_spans_kappa_from_comb_lines(monkeypatch):
    """run_concatenated_comb_simulation and scan_comb_copier_psa_phase launch span s with comb_lines' kappa on THAT span's
    dispersion, the step counts of the configs and the mid-stage as a per-point
    transfer; a line dark at the input has a NaN gain."""
    seen = {}

    def spy(spans, **kw):
        seen.update(spans=spans, **kw)
        return _fake_result(spans, **kw)

    d_copier, d_psa = _dispersion(), _dispersion(1.7)
    wc, dw = 2.0 * np.pi * 299792458.0 / 1550e-9, 2.0 * np.pi * 200e9
    want = [simulation.comb_lines(wc, dw, 5, d, max_order=4)[1] for d in (d_copier, d_psa)]
    assert not np.allclose(want[0], want[1])
    monkeypatch.setattr(simulation, "rk4_chain_comb", spy)
    cfgs = [custom_simulation_config(z_max=150.0, dz=1.0), custom_simulation_config(z_max=300.0, dz=1.0)]
    z, A = simulation.run_concatenated_comb_simulation(
        [dict(cfg=cfgs[0], gamma=0.0115, alpha=0.0, dispersion=d_copier), dict(cfg=cfgs[1], gamma=0.0115, alpha=2e-5, dispersion=d_psa)],
        omega_center=wc, line_spacing=dw, p_in=[1e-6, 0.2, 0.0, 0.2, 1e-6], transfers=[simulation.comb_mid_stage(np.zeros(5), 0.3)],
        length_unit="m")
    assert [s.n_steps for s in seen["spans"]] == [150, 300] and A.shape == (47, 5) and z.shape == (47,)
    for s, kp, L in zip(seen["spans"], want, (150.0, 300.0)):
        assert np.array_equal(s.dbeta, kp) and abs(s.length - L) < 1e-9 and abs(s.gamma - 0.0115) < 1e-15
    assert seen["want_traj"] and seen["check_nan"] and seen["save_every"] == 10 and seen["transfers"][0].shape == (5,)

    monkeypatch.setattr(sweep, "rk4_chain_comb", spy)
    ph = np.linspace(0.0, 2.0 * np.pi, 6, endpoint=False)
    out = scan_mismtach.scan_comb_copier_psa_phase(
        psa_cfg=cfgs[1], copier_cfg=cfgs[0], lambda_center_m=1550e-9, line_spacing=dw, p_lines=[1e-6, 0.2, 0.0, 0.2, 1e-6],
        gamma=0.0115, alpha=0.0, dispersion=d_psa, copier_dispersion=d_copier, phase=ph, phase_lines=[1, 3],
        mid_gain_db=[0.0, -1.0, 0.0, -1.0, 0.0], mid_phase=0.25, gain_mode="end", gain_unit="linear")
    for s, kp in zip(seen["spans"], want):
        assert s.dbeta.shape == (6, 5) and np.array_equal(s.dbeta, np.broadcast_to(kp, (6, 5)))
    np.testing.assert_allclose(out["kappa"], np.stack(want), rtol=1e-15)
    T = seen["transfers"][0]
    assert T.shape == (6, 5) and seen["a0"].shape == (5,)
    np.testing.assert_allclose(T / np.abs(T), np.exp(1j * (0.25 + ph[:, None] * np.array([0, 1, 0, 1, 0.0]))), atol=1e-14)
    np.testing.assert_allclose(np.abs(T) ** 2, np.broadcast_to(10.0 ** (np.array([0.0, -1.0, 0.0, -1.0, 0.0]) / 10.0), (6, 5)), rtol=1e-14)
    assert out["gain"].shape == out["p_out"].shape == (6, 5) and np.isnan(out["gain"][:, 2]).all()
    assert np.allclose(out["gain"][:, [0, 1, 3, 4]], 2.0) and out["extinction_db"].shape == (5,) and np.isnan(out["extinction_db"][2])
    assert np.allclose(out["extinction_db"][[0, 1, 3, 4]], 0.0) and out["first_bad_step"].shape == (6,)
    # without a copier the mid-stage acts on the input: one span, no transfer
    scan_mismtach.scan_comb_copier_psa_phase(psa_cfg=cfgs[1], lambda_center_m=1550e-9, line_spacing=dw, p_lines=[1e-6, 0.2, 0.2, 1e-6],
                                             gamma=0.0115, alpha=0.0, dispersion=d_psa, phase=ph, phase_lines=[1])
    assert len(seen["spans"]) == 1 and seen["transfers"] is None and seen["a0"].shape == (6, 4)
