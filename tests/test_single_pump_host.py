"""The single-pump (degenerate) three-wave sweep without a GPU: the NumPy restatement (tests/single_pump_np.py) pinned to the
undepleted-pump closed form, to scipy's DOP853 on depleted lossy points and to the model's conservation laws; the argument
rules of psa_rk4_single_pump_f64 / _dev (every code comes back before any device call); the binding against the header; the
Python wrappers' shape rules, SinglePumpResult's reductions and the device split of the inputs."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import psa_amd._native as nat
import single_pump_np
from psa_amd import config, dispersion, scan_mismtach, simulation, sweep
from psa_amd._partition import SWEEP_AXES, cut

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NPOINTS, E_NSTEPS, E_ZMAX, E_SAVE_EVERY, E_NULLPTR, E_DEVICE, E_TOO_LARGE, E_FLAGS = -2, -3, -4, -5, -6, -7, -9, -11
GAMMA, LENGTH, P_PUMP = 0.0115, 1000.0, 0.5


def test_restatement_matches_the_closed_form_gain():
    """Bar 1e-6 on G and on the idler's G - 1: a decade over the physical depletion term 2 G p_s / P_p (1e-7 here)."""
    c = single_pump_np.analytic_case()
    r = single_pump_np.integrate(c["a0"], c["dbeta"], z_max=c["z_max"], n=c["n"], save_every=c["n"], gamma=GAMMA, alpha=0.0)
    G, Gi = r["p_wave_end"][:, 1] / c["p_seed"], r["p_wave_end"][:, 2] / c["p_seed"]
    err_s, err_i = np.max(np.abs(G / c["gain"] - 1.0)), np.max(np.abs(Gi / (c["gain"] - 1.0) - 1.0))
    print(f"closed form: signal {err_s:.2e} idler {err_i:.2e}; peak gain {c['gain'].max():.4g} at dbeta/(gamma P) = "
          f"{c['dbeta'][np.argmax(c['gain'])] / (GAMMA * P_PUMP):.3f}")
    assert err_s < 1e-6 and err_i < 1e-6
    assert abs(c["dbeta"][np.argmax(G)] / (GAMMA * P_PUMP) + 2.0) < 0.07        # the peak sits at dbeta = -2 gamma P


def _depleted_points():
    rng = np.random.default_rng(42)
    N = 12
    dbeta = rng.uniform(-3.5, -0.5, N) * GAMMA * P_PUMP
    p = np.column_stack([np.full(N, P_PUMP), 10 ** rng.uniform(-4, -2, N), 10 ** rng.uniform(-6, -3, N)])
    a0 = np.sqrt(p) * np.exp(1j * rng.uniform(-3, 3, (N, 3)))
    return dbeta, a0, GAMMA * rng.uniform(0.9, 1.1, N), 1.15e-4 * rng.uniform(0.5, 1.5, N)


def test_restatement_matches_scipy_on_depleted_lossy_points():
    """scipy's DOP853 at rtol 1e-13 on the same equations written out by hand (real and imaginary parts, no shared code):
    within 1e-9 of the point's largest wave at 1e4 steps (RK4's own truncation error there is ~2e-11)."""
    from scipy.integrate import solve_ivp
    dbeta, a0, gamma, alpha = _depleted_points()
    r = single_pump_np.integrate(a0, dbeta, z_max=LENGTH, n=10_000, save_every=10_000, gamma=gamma, alpha=alpha)
    depletion = 1.0 - r["p_wave_end"][:, 0] * np.exp(alpha * LENGTH) / P_PUMP
    print("pump depletion (loss taken out):", np.round(depletion, 3))
    assert depletion.max() > 0.5 and (depletion > 0.1).sum() >= 6    # strongly depleted points are among them
    worst = 0.0
    for k in range(dbeta.size):
        g, al, db = gamma[k], alpha[k], dbeta[k]

        def f(z, y):
            xp, yp, xs, ys, xi, yi = y
            pp, ps, pi = xp * xp + yp * yp, xs * xs + ys * ys, xi * xi + yi * yi
            tot = pp + ps + pi
            c, s = np.cos(db * z), np.sin(db * z)
            ap, as_, ai = complex(xp, yp), complex(xs, ys), complex(xi, yi)
            e = 2.0 * g * complex(c, s)
            dp = (-0.5 * al + 1j * g * (2 * tot - pp)) * ap + 1j * ap.conjugate() * e * as_ * ai
            ds = (-0.5 * al + 1j * g * (2 * tot - ps)) * as_ + 0.5j * ai.conjugate() * e.conjugate() * ap * ap
            di = (-0.5 * al + 1j * g * (2 * tot - pi)) * ai + 0.5j * as_.conjugate() * e.conjugate() * ap * ap
            return [dp.real, dp.imag, ds.real, ds.imag, di.real, di.imag]

        sol = solve_ivp(f, (0.0, LENGTH), a0[k].view(float), method="DOP853", rtol=1e-13, atol=1e-20)
        ref = sol.y[:, -1].view(complex)
        worst = max(worst, float(np.max(np.abs(r["a_end"][k] - ref)) / np.max(np.abs(ref))))
    print(f"restatement vs DOP853: {worst:.2e} of the largest wave")
    assert worst < 1e-9


def test_restatement_conserves_the_models_invariants():
    """alpha = 0: P_p + P_s + P_i, P_s - P_i and P_p + 2 P_s within 1e-12 of the input total; with loss the total times
    e^{alpha z}."""
    dbeta, a0, gamma, alpha = _depleted_points()
    p_in = np.abs(a0) ** 2
    total = p_in.sum(axis=1)
    r = single_pump_np.integrate(a0, dbeta, z_max=LENGTH, n=10_000, save_every=10_000, gamma=gamma, alpha=0.0)
    p = r["p_wave_end"]
    d_total = np.max(np.abs(p.sum(axis=1) - total) / total)
    d_mr = np.max(np.abs((p[:, 1] - p[:, 2]) - (p_in[:, 1] - p_in[:, 2])) / total)
    d_ps = np.max(np.abs((p[:, 0] + 2 * p[:, 1]) - (p_in[:, 0] + 2 * p_in[:, 1])) / total)
    lossy = single_pump_np.integrate(a0, dbeta, z_max=LENGTH, n=10_000, save_every=10_000, gamma=gamma, alpha=alpha)
    d_loss = np.max(np.abs(lossy["p_wave_end"].sum(axis=1) * np.exp(alpha * LENGTH) - total) / total)
    print(f"conservation: total {d_total:.2e} P_s - P_i {d_mr:.2e} P_p + 2 P_s {d_ps:.2e} lossy total {d_loss:.2e}")
    assert max(d_total, d_mr, d_ps, d_loss) < 1e-12


def test_dark_sidebands_leave_self_phase_modulation():
    """No sideband light: the pump follows exp(-alpha z / 2) exp(i gamma P_0 L_eff) -- gamma |A_p|^2, not the 1.5 gamma |A_p|^2
    of the 4-wave system with equal pumps."""
    al = 1.15e-4
    r = single_pump_np.integrate(np.array([np.sqrt(P_PUMP), 0, 0], complex), [0.013], z_max=LENGTH, n=10_000, save_every=10_000,
                                 gamma=GAMMA, alpha=al)
    leff = (1.0 - np.exp(-al * LENGTH)) / al
    want = np.sqrt(P_PUMP) * np.exp(-0.5 * al * LENGTH) * np.exp(1j * GAMMA * P_PUMP * leff)
    assert abs(r["a_end"][0, 0] - want) / abs(want) < 1e-9 and np.all(r["a_end"][0, 1:] == 0)


def test_restatement_save_rows_and_failure_index():
    a0 = np.sqrt(np.array([0.5, 1e-5, 0.0])).astype(complex)
    kw = dict(z_max=10.0, gamma=GAMMA, alpha=1e-4)
    full = single_pump_np.integrate(a0, [0.01], n=25, save_every=1, want_traj=True, **kw)
    strided = single_pump_np.integrate(a0, [0.01], n=25, save_every=10, want_traj=True, **kw)
    assert full["traj"].shape == (1, 26, 3) and strided["traj"].shape == (1, 3, 3)
    assert np.array_equal(strided["traj"][0], full["traj"][0, ::10]) and np.array_equal(strided["a_end"][0], full["traj"][0, 20])
    none = single_pump_np.integrate(a0, [0.01], n=7, save_every=10, **kw)
    assert np.array_equal(none["a_end"][0], a0) and np.array_equal(none["p_wave_max"], np.abs(none["a_end"]) ** 2)
    bad = single_pump_np.integrate(a0, [0.01, 0.01], z_max=200.0, n=2000, save_every=10, gamma=GAMMA, alpha=np.array([-12.0, 1e-4]))
    assert bad["first_bad_step"][0] >= 0 and bad["first_bad_step"][1] == -1 and np.isnan(bad["p_wave_max"][0]).all()


# ---- the argument rules of the two entry points ------------------------------------------------------------------------
def _dev(n=8, steps=10, z=1.0, se=1, flags=0, null=False, traj=False):
    """psa_rk4_single_pump_f64_dev with dummy pointers: every call here must fail in validation, before any launch."""
    buf = np.zeros(64)
    p = buf.ctypes.data_as(C.c_void_p)
    q = None if null else p
    return nat.lib().psa_rk4_single_pump_f64_dev(None, n, steps, z, se, q, p, p, p, flags, p, p, p, p, p if traj else None)


def _host(n=8, steps=10, z=1.0, se=1, flags=0, null=False, traj=False):
    buf = np.zeros(64)
    p = buf.ctypes.data_as(C.c_void_p)
    q = None if null else p
    return nat.lib().psa_rk4_single_pump_f64(0, n, steps, z, se, p, p, p, p, flags, p, p, q, p, p if traj else None, None)


@pytest.mark.parametrize("call", [_dev, _host], ids=["dev", "host"])
def test_every_argument_error_comes_back_before_any_device_call(call):
    assert call(n=-1) == E_NPOINTS
    assert call(n=nat.MAX_POINTS + 1) == E_TOO_LARGE
    assert call(steps=0) == E_NSTEPS and call(steps=2**31) == E_NSTEPS
    assert call(z=0.0) == E_ZMAX and call(z=float("inf")) == E_ZMAX and call(z=float("nan")) == E_ZMAX
    assert call(se=0) == E_SAVE_EVERY
    assert call(null=True) == E_NULLPTR
    for bit in (nat.OPT_ONE_LANE, nat.OPT_SPLIT_POINT, nat.OPT_QUAD_POINT, nat.OPT_F32_SCALAR, nat.OPT_F32_PACKED,
                nat.OPT_LDS_STAGING, nat.BCAST_TRANSFER, 1 << 19, 1 << 30):
        assert call(flags=bit | nat.OPT_CHECK_NAN) == E_FLAGS, bit
    assert b"only" in nat.lib().psa_last_error()
    # the order of validate_common: the grid before the flags, the flags before the pointers
    assert call(n=-1, flags=nat.OPT_ONE_LANE, null=True) == E_NPOINTS and call(flags=nat.OPT_ONE_LANE, null=True) == E_FLAGS


def test_the_padded_leading_dimension_belongs_to_the_device_form():
    assert _host(flags=nat.OPT_TRAJ_LD) == E_FLAGS and _host(flags=nat.OPT_TRAJ_LD, traj=True) == E_FLAGS
    # on the _dev form the flag passes validation: the next rule (here: a NULL pointer) is the one that answers
    assert _dev(flags=nat.OPT_TRAJ_LD, traj=True, null=True) == E_NULLPTR


@pytest.mark.parametrize("call", [_dev, _host], ids=["dev", "host"])
def test_a_trajectory_needs_a_leading_dimension_below_2_to_the_28(call):
    """Rows are addressed with the lane's 32-bit byte offset: ld * 16 < 2^32.  Without a trajectory the same size passes
    validation (dummy pointers: the call then stops at the NULL-pointer rule, not at the size)."""
    assert call(n=2**28, traj=True) == E_TOO_LARGE and b"2^28" in nat.lib().psa_last_error()
    assert call(n=2**28, traj=False, null=True) == E_NULLPTR
    assert call(n=2**28 - 1, traj=True, null=True) == E_NULLPTR


def test_an_empty_sweep_is_a_successful_no_op():
    L = nat.lib()
    assert L.psa_rk4_single_pump_f64_dev(None, 0, 10, 1.0, 1, None, None, None, None, 0, None, None, None, None, None) == 0
    assert L.psa_rk4_single_pump_f64(0, 0, 10, 1.0, 1, None, None, None, None, 0, None, None, None, None, None, None) == 0


_CTYPE = {"int": C.c_int, "int64_t": C.c_int64, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "double": C.c_double}


def test_the_binding_equals_the_header():
    """Both prototypes of include/psa_rk4.h, argument by argument, against the ctypes table; no new PSA_E_* code."""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "psa_rk4.h"), encoding="utf-8").read(), flags=re.S)
    for name in ("psa_rk4_single_pump_f64", "psa_rk4_single_pump_f64_dev"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
        assert m, name
        args = []
        for decl in m.group(1).split(","):
            decl = decl.strip()
            args.append(C.c_void_p if "*" in decl else _CTYPE[decl.replace("const ", "").split()[0]])
        res, want = nat._SIGS[name]
        assert res is C.c_int and list(want) == args, name
        assert name in nat.EXPORTED_SYMBOLS and hasattr(nat.lib(), name)
    codes = [int(x) for x in re.findall(r"#define\s+PSA_E_\w+\s+(-\d+)", src)]
    assert sorted(codes) == list(range(-13, 0))


@pytest.mark.skipif(nat.device_count() > 0, reason="CPU box only")
def test_without_a_device_a_valid_call_is_an_error_not_a_fallback():
    with pytest.raises(nat.PsaNativeError) as e:
        nat.single_pump_host(np.zeros(3), n_steps=1, z_max=1.0, save_every=1, gamma=1.0, alpha=0.0, a0=np.ones(3, complex))
    assert e.value.code == E_DEVICE and "no CPU fallback" in str(e.value)


# ---- Python --------------------------------------------------------------------------------------------------------------
def test_python_wrapper_shape_rules():
    kw = dict(n_steps=1, z_max=1.0, save_every=1, gamma=1.0, alpha=0.0)
    for dbeta, a0 in ((np.zeros((3, 1)), np.ones(3, complex)),             # dbeta must be (N,)
                      (np.zeros(3), np.ones(4, complex)),                   # a0 of another model
                      (np.zeros(3), np.ones((2, 3), complex)),              # neither 1 nor N rows
                      (np.zeros(3), np.ones((3, 1, 3), complex))):
        with pytest.raises(ValueError):
            nat.single_pump_host(dbeta, a0=a0, **kw)
    for bad in (dict(gamma=[1.0, 2.0]), dict(alpha=np.ones((3, 1)))):
        with pytest.raises(ValueError):
            nat.single_pump_host(np.zeros(3), a0=np.ones(3, complex), **dict(kw, **bad))
    ok = dict(gamma=1.0, alpha=0.0, a0=np.ones(3, complex))
    for bad in (dict(z_max=0.0, dz=0.1), dict(z_max=1.0), dict(z_max=1.0, dz=-0.1), dict(z_max=1.0, dz=0.1, save_every=0),
                dict(z_max=1.0, dz=10.0), dict(z_max=1.0, dz=0.1, devices=[])):
        with pytest.raises(ValueError):
            sweep.rk4_sweep_single_pump(np.zeros(3), **ok, **bad)
    with pytest.raises(ValueError):
        sweep.rk4_sweep_single_pump(np.zeros((3, 2)), z_max=1.0, dz=0.1, **ok)
    with pytest.raises(ValueError):
        sweep.rk4_sweep_single_pump(np.zeros(3), z_max=1.0, dz=0.1, gamma=1.0, alpha=0.0, a0=np.ones(4, complex))


def test_the_device_split_cuts_the_inputs_by_points():
    """rk4_sweep_single_pump hands _run the table SWEEP_AXES: dbeta, gamma, alpha and a0 rows follow the block."""
    kw = dict(dbeta=np.arange(6.0), gamma=np.arange(6.0), alpha=0.5, a0=np.arange(18.0).reshape(6, 3).astype(complex),
              n_steps=3, want_traj=True)
    part = cut(kw, SWEEP_AXES, 6, slice(2, 5))
    assert np.array_equal(part["dbeta"], [2.0, 3.0, 4.0]) and np.array_equal(part["gamma"], [2.0, 3.0, 4.0])
    assert part["alpha"] == 0.5 and np.array_equal(part["a0"], kw["a0"][2:5]) and part["n_steps"] == 3 and part["want_traj"]
    bcast = cut(dict(kw, a0=np.ones(3, complex)), SWEEP_AXES, 6, slice(0, 2))
    assert bcast["a0"].shape == (3,)                                       # a broadcast a0 passes through


def _result():
    # N = 4 points, waves [p, s, i]
    end = np.array([[0.4, 2e-3, 1e-3], [0.5, 1e-5, 0.0], [0.1, 1.0, 1.0], [0.25, 1e-4, 1e-6]])
    mx = end * np.array([1.25, 2.0, 1.0])
    bad = np.array([-1, -1, 41, -1])
    return sweep.SinglePumpResult(np.sqrt(end).astype(complex), end, mx, bad, 100, 10, 0.0, np.array([[0.5, 1e-5, 0.0]]))


def test_single_pump_result_reductions_and_their_nan_rule():
    r = _result()
    g = r.signal_gain(1e-5, mode="end", unit="linear")
    assert g.shape == (4,) and np.allclose(g[[0, 1, 3]], [200.0, 1.0, 10.0], rtol=1e-14) and np.isnan(g[2])
    g = r.signal_gain(1e-5)                                              # max, dB
    assert np.allclose(g[[0, 1, 3]], 10 * np.log10([400.0, 2.0, 20.0]), rtol=1e-14) and np.isnan(g[2])
    g = r.signal_gain(np.array([1e-5, 0.0, 1e-5, 2e-5]), mode="end", unit="linear")   # a dark seed defines no gain
    assert g[0] == pytest.approx(200.0) and np.isnan(g[1]) and np.isnan(g[2]) and g[3] == pytest.approx(5.0)
    c = r.idler_conversion(1e-5, mode="end", unit="linear")
    assert c[0] == pytest.approx(100.0) and np.isnan(c[1]) and np.isnan(c[2]) and c[3] == pytest.approx(0.1)
    d = r.pump_depletion()
    assert d.shape == (4,) and np.allclose(d[[0, 1, 3]], [0.2, 0.0, 0.5], atol=1e-15) and np.isnan(d[2])
    for bad in (dict(mode="mean"), dict(unit="neper")):
        with pytest.raises(ValueError):
            r.signal_gain(1e-5, **bad)
    with pytest.raises(ValueError):
        r.signal_gain([1e-5, 1e-5])
    with pytest.raises(ValueError):
        r.idler_conversion(np.ones((4, 1)))
    with pytest.raises(ValueError):
        sweep.SinglePumpResult(r.a_end, r.p_wave_end, r.p_wave_max, r.first_bad_step, 100, 10, 0.0).pump_depletion()


def _dispersion(golden):
    dv = golden("G11")["disp_m"]
    return dispersion.DispersionParams(omega_ref=dv[0], beta2=dv[1], beta3=dv[2], beta4=dv[3])


def test_driver_input_errors(golden):
    d = _dispersion(golden)
    cfg = config.custom_simulation_config(z_max=10.0, dz=0.1)
    ok = dict(cfg=cfg, lambda_pump_m=1550e-9, lambda_signal_m=[1540e-9, 1545e-9], p_pump=0.5, p_signal=1e-6, gamma=GAMMA,
              alpha=1e-4, dispersion=d)
    for bad in (dict(lambda_signal_m=[]), dict(lambda_signal_m=np.ones((2, 2))), dict(p_pump=-0.1), dict(p_signal=0.0),
                dict(p_idler=-1e-7), dict(p_idler=np.nan), dict(phase_in=[0.0] * 4), dict(dispersion=None),
                dict(gain_mode="mean"), dict(gain_unit="neper"), dict(lambda_pump_m=-1.0), dict(max_order=-1),
                dict(length_unit="mile")):
        with pytest.raises(ValueError):
            scan_mismtach.scan_single_pump_gain(**dict(ok, **bad))
    w = 2.0 * np.pi * 299792458.0 / 1550e-9
    one = dict(gamma=GAMMA, alpha=1e-4, omega_pump=w, omega_signal=1.01 * w, p_in=[0.5, 1e-6, 0.0], dispersion=d)
    for bad in (dict(omega_signal=2.0 * w), dict(omega_signal=2.5 * w), dict(omega_pump=-w), dict(omega_signal=np.inf),
                dict(p_in=[0.5, 1e-6]), dict(p_in=[0.5, -1e-6, 0.0]), dict(phase_in=[0.0] * 4), dict(dispersion=None),
                dict(length_unit="mile"), dict(max_order=-1)):
        with pytest.raises(ValueError):
            simulation.run_single_pump_simulation(cfg, **dict(one, **bad))
    with pytest.raises(TypeError):
        simulation.run_single_pump_simulation(cfg, **dict(one, dispersion="smf28"))
    with pytest.raises(ValueError):
        simulation.run_single_pump_simulation(config.custom_simulation_config(z_max=-1.0, dz=0.1), **one)
