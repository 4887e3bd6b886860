"""The multi-line ("frequency comb") model without a GPU: the NumPy restatement tests/comb_np.py against its own definition,
against the single-pump restatement at M = 3 and against the model's symmetries; the argument rules of psa_rk4_comb_f64 and
psa_rk4_comb_f64_dev, which answer before any device call; the Python wrappers' shape rules and the drivers' propagation
constants."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import comb_np
import psa_amd._native as nat
import single_pump_np
from psa_amd import config, dispersion, scan_mismtach, simulation, sweep
from psa_amd._partition import COMB_AXES, cut

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NPOINTS, E_NSTEPS, E_ZMAX, E_SAVE_EVERY, E_NULLPTR, E_DEVICE, E_TOO_LARGE, E_FLAGS, E_NLINES = -2, -3, -4, -5, -6, -7, -9, -11, -14


def rel(got, ref):
    """max |got - ref| over the largest line of the point."""
    ref = np.asarray(ref)
    return float(np.max(np.abs(np.asarray(got) - ref) / np.abs(ref).max(axis=-1, keepdims=True)))


# ---- the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [3, 4, 7, 12])
def test_the_pair_sum_equals_the_triple_sum(M):
    rng = np.random.default_rng(M)
    B = rng.normal(size=(50, M)) + 1j * rng.normal(size=(50, M))
    S3, S2 = comb_np.triple_sum(B), comb_np.pair_sum(B)
    err = rel(S2, S3)
    print(f"M={M}: pair sum against triple sum {err:.2e}")
    assert err < 1e-13
    # S_m holds the SPM/XPM term (2 sum_j P_j - P_m) B_m: the triples (k, l, n) = (m, j, j) and (j, m, j)
    P = np.abs(B) ** 2
    only = np.zeros_like(B)
    only[:, 0] = B[:, 0]
    assert rel(comb_np.pair_sum(only)[:, 0], (P[:, 0] * B[:, 0])) < 1e-15


@pytest.mark.parametrize("split", ["symmetric", "random"])
def test_three_lines_are_the_single_pump_model(split):
    """Lines [0, 1, 2] = waves [s, p, i] with kappa_0 + kappa_2 - 2 kappa_1 = dbeta, on single_pump_np's own kind of inputs."""
    N = 40
    rng = np.random.default_rng(5)
    dbeta = rng.uniform(-4.5, 0.5, N) * single_pump_np.GAMMA * single_pump_np.P_PUMP
    p = np.column_stack([rng.uniform(0.3, 0.6, N), 10 ** rng.uniform(-12, -2, N), 10 ** rng.uniform(-12, -2, N)])
    a0 = np.sqrt(p) * np.exp(1j * rng.uniform(-3, 3, (N, 3)))            # [p, s, i]
    gamma, alpha = single_pump_np.GAMMA * rng.uniform(0.9, 1.1, N), 1.15e-4 * rng.uniform(0.5, 1.5, N)
    if split == "symmetric":
        kappa = np.column_stack([0.5 * dbeta, np.zeros(N), 0.5 * dbeta])
    else:
        k1, k0 = rng.uniform(-0.01, 0.01, N), rng.uniform(-0.01, 0.01, N)
        kappa = np.column_stack([k0, k1, dbeta + 2.0 * k1 - k0])
    kw = dict(z_max=300.0, n=600, save_every=7, gamma=gamma, alpha=alpha)
    ref = single_pump_np.integrate(a0, dbeta, **kw)
    got = comb_np.integrate(a0[:, [1, 0, 2]], kappa, **kw)
    err = rel(got["a_end"][:, [1, 0, 2]], ref["a_end"])
    print(f"{split} split: a_end {err:.2e}")
    assert err < 1e-12 and rel(got["p_wave_max"][:, [1, 0, 2]], ref["p_wave_max"]) < 1e-12


@pytest.mark.parametrize("M", [4, 7])
def test_gauge_mirror_and_conservation(M):
    """The invariants hold to the step's truncation error: 1 500 steps over 300 m is the GPU test's grid, where the defect
    is of the order 1e-11."""
    kappa, a0, gamma, _ = comb_np.random_inputs(30, M, 11, lossy=False)
    kw = dict(z_max=300.0, n=1500, save_every=10, gamma=gamma, alpha=0.0)
    ref = comb_np.integrate(a0, kappa, **kw)
    m = np.arange(M)
    gauged = comb_np.integrate(a0, kappa + 0.017 - 0.004 * m, **kw)
    mirrored = comb_np.integrate(a0[:, ::-1], kappa[:, ::-1], **kw)
    e_g, e_m = rel(gauged["a_end"], ref["a_end"]), rel(mirrored["a_end"][:, ::-1], ref["a_end"])
    P0, P = np.abs(a0) ** 2, ref["p_wave_end"]
    d_p = np.max(np.abs(P.sum(1) - P0.sum(1)) / P0.sum(1))
    d_m = np.max(np.abs((m * P).sum(1) - (m * P0).sum(1)) / P0.sum(1))
    print(f"M={M}: gauge {e_g:.2e} mirror {e_m:.2e} sum P {d_p:.2e} sum m P {d_m:.2e}")
    assert e_g < 1e-12 and e_m < 1e-12 and d_p < 1e-10 and d_m < 1e-10
    assert np.max(np.abs(P / P0 - 1.0)) > 1e-3            # the points do mix: the invariants are not trivial


def test_dark_odd_lines_stay_dark_and_the_even_lines_repeat_the_smaller_comb():
    kappa, a0, gamma, alpha = comb_np.random_inputs(20, 7, 3)
    a0 = a0.copy()
    a0[:, 1::2] = 0.0
    a0[:, 2] *= 30.0                                       # a strong line among the bright ones
    kw = dict(z_max=200.0, n=400, save_every=10, gamma=gamma, alpha=alpha, want_traj=True)
    seven = comb_np.integrate(a0, kappa, **kw)
    four = comb_np.integrate(a0[:, ::2], kappa[:, ::2], **kw)
    assert np.all(seven["traj"][:, :, 1::2] == 0)
    assert np.array_equal(seven["traj"][:, :, ::2], four["traj"])
    assert np.max(np.abs(four["p_wave_end"] / np.abs(a0[:, ::2]) ** 2 - 1.0)) > 1e-3


def test_restatement_save_rows_and_failure_index():
    kappa, a0, gamma, _ = comb_np.random_inputs(6, 4, 2)
    alpha = np.array([1e-4, -6.0, 1e-4, -9.0, 1e-4, 1e-4])
    r = comb_np.integrate(a0, kappa, z_max=6.5, n=65, save_every=10, gamma=gamma, alpha=alpha, want_traj=True)
    assert r["traj"].shape == (6, 7, 4) and np.array_equal(r["traj"][:, 0], a0)
    assert np.array_equal(r["traj"][:, -1].view(float), r["a_end"].view(float), equal_nan=True)
    ok = np.array([True, False, True, False, True, True])
    assert (r["first_bad_step"][ok] == -1).all() and (r["first_bad_step"][~ok] > 0).all()
    assert np.isnan(r["p_wave_max"][~ok]).all() and np.isfinite(r["p_wave_max"][ok]).all()


# ---- the argument rules of the two entry points ------------------------------------------------------------------------
def _dev(M=4, n=8, steps=10, z=1.0, se=1, flags=0, null=False, traj=False):
    """psa_rk4_comb_f64_dev with dummy pointers: every call here must fail in validation, before any launch."""
    buf = np.zeros(64)
    p = buf.ctypes.data_as(C.c_void_p)
    q = None if null else p
    return nat.lib().psa_rk4_comb_f64_dev(None, M, n, steps, z, se, q, p, p, p, flags, p, p, p, p, p if traj else None)


def _host(M=4, n=8, steps=10, z=1.0, se=1, flags=0, null=False, traj=False):
    buf = np.zeros(64)
    p = buf.ctypes.data_as(C.c_void_p)
    q = None if null else p
    return nat.lib().psa_rk4_comb_f64(0, M, n, steps, z, se, p, p, p, p, flags, p, p, q, p, p if traj else None, None)


@pytest.mark.parametrize("call", [_dev, _host], ids=["dev", "host"])
def test_every_argument_error_comes_back_before_any_device_call(call):
    for M in (-1, 0, 2, 13, 64):
        assert call(M=M) == E_NLINES, M
    assert b"n_lines" in nat.lib().psa_last_error()
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
    # the order: the line count first, then the single-pump entry's: the grid before the flags, the flags before the pointers
    assert call(M=2, n=-1, flags=nat.OPT_ONE_LANE, null=True) == E_NLINES
    assert call(n=-1, flags=nat.OPT_ONE_LANE, null=True) == E_NPOINTS and call(flags=nat.OPT_ONE_LANE, null=True) == E_FLAGS
    # PSA_OPT_EXACT_STEP is accepted: with dummy pointers the call then stops at the NULL-pointer rule
    assert call(flags=nat.OPT_CHECK_NAN | nat.OPT_EXACT_STEP | nat.OPT_BLOCK64 | nat.OPT_LOSSLESS, null=True) == E_NULLPTR


def test_the_padded_leading_dimension_belongs_to_the_device_form():
    assert _host(flags=nat.OPT_TRAJ_LD) == E_FLAGS and _host(flags=nat.OPT_TRAJ_LD, traj=True) == E_FLAGS
    assert _dev(flags=nat.OPT_TRAJ_LD, traj=True, null=True) == E_NULLPTR


@pytest.mark.parametrize("call", [_dev, _host], ids=["dev", "host"])
def test_a_trajectory_needs_a_leading_dimension_below_2_to_the_28(call):
    assert call(n=2**28, traj=True) == E_TOO_LARGE and b"2^28" in nat.lib().psa_last_error()
    assert call(n=2**28, traj=False, null=True) == E_NULLPTR
    assert call(n=2**28 - 1, traj=True, null=True) == E_NULLPTR


def test_an_empty_sweep_is_a_successful_no_op():
    L = nat.lib()
    assert L.psa_rk4_comb_f64_dev(None, 5, 0, 10, 1.0, 1, None, None, None, None, 0, None, None, None, None, None) == 0
    assert L.psa_rk4_comb_f64(0, 5, 0, 10, 1.0, 1, None, None, None, None, 0, None, None, None, None, None, None) == 0
    assert L.psa_rk4_comb_f64(0, 2, 0, 10, 1.0, 1, None, None, None, None, 0, None, None, None, None, None, None) == E_NLINES


_CTYPE = {"int": C.c_int, "int64_t": C.c_int64, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "double": C.c_double}


def test_the_binding_equals_the_header():
    """Both prototypes of include/psa_rk4.h, argument by argument, against the ctypes table; PSA_E_NLINES is the next free
    code and PSA_MAX_LINES the wrapper's."""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "psa_rk4.h"), encoding="utf-8").read(), flags=re.S)
    for name in ("psa_rk4_comb_f64", "psa_rk4_comb_f64_dev"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
        assert m, name
        args = []
        for decl in m.group(1).split(","):
            decl = decl.strip()
            args.append(C.c_void_p if "*" in decl else _CTYPE[decl.replace("const ", "").split()[0]])
        res, want = nat._SIGS[name]
        assert res is C.c_int and list(want) == args, name
        assert name in nat.EXPORTED_SYMBOLS and hasattr(nat.lib(), name)
    codes = [int(x) for x in re.findall(r"#define\s+PSA_E_\w+\s+\(?(-\d+)\)?", src)]      # -14 is written (-14)
    assert sorted(codes) == list(range(-14, 0)) and re.search(r"#define\s+PSA_E_NLINES\s+\(-14\)", src)
    assert int(re.search(r"#define\s+PSA_MAX_LINES\s+(\d+)", src).group(1)) == nat.MAX_LINES == 12


@pytest.mark.skipif(nat.device_count() > 0, reason="CPU box only")
def test_without_a_device_a_valid_call_is_an_error_not_a_fallback():
    with pytest.raises(nat.PsaNativeError) as e:
        nat.comb_host(np.zeros((3, 4)), n_steps=1, z_max=1.0, save_every=1, gamma=1.0, alpha=0.0, a0=np.ones(4, complex))
    assert e.value.code == E_DEVICE and "no CPU fallback" in str(e.value)


# ---- Python --------------------------------------------------------------------------------------------------------------
def test_python_wrapper_shape_rules():
    kw = dict(n_steps=1, z_max=1.0, save_every=1, gamma=1.0, alpha=0.0)
    for kappa, a0 in ((np.zeros(4), np.ones(4, complex)),                   # kappa must be (N, M)
                      (np.zeros((3, 2)), np.ones(2, complex)),              # fewer than 3 lines
                      (np.zeros((3, 13)), np.ones(13, complex)),            # more than PSA_MAX_LINES
                      (np.zeros((3, 4)), np.ones(5, complex)),              # a0 of another width
                      (np.zeros((3, 4)), np.ones((2, 4), complex)),         # neither 1 nor N rows
                      (np.zeros((3, 4)), np.ones((3, 1, 4), complex))):
        with pytest.raises(ValueError):
            nat.comb_host(kappa, a0=a0, **kw)
        with pytest.raises(ValueError):
            sweep.rk4_sweep_comb(kappa, z_max=1.0, dz=0.1, gamma=1.0, alpha=0.0, a0=a0)
    for bad in (dict(gamma=[1.0, 2.0]), dict(alpha=np.ones((3, 1)))):
        with pytest.raises(ValueError):
            nat.comb_host(np.zeros((3, 4)), a0=np.ones(4, complex), **dict(kw, **bad))
    ok = dict(gamma=1.0, alpha=0.0, a0=np.ones(4, complex))
    for bad in (dict(z_max=0.0, dz=0.1), dict(z_max=1.0), dict(z_max=1.0, dz=-0.1), dict(z_max=1.0, dz=0.1, save_every=0),
                dict(z_max=1.0, dz=10.0), dict(z_max=1.0, dz=0.1, devices=[]), dict(z_max=float("nan"), dz=0.1)):
        with pytest.raises(ValueError):
            sweep.rk4_sweep_comb(np.zeros((3, 4)), **ok, **bad)


def test_the_device_split_cuts_the_inputs_by_points():
    kw = dict(kappa=np.arange(24.0).reshape(6, 4), gamma=np.arange(6.0), alpha=0.5, a0=np.arange(24.0).reshape(6, 4).astype(complex),
              n_steps=3, want_traj=True)
    part = cut(kw, COMB_AXES, 6, slice(2, 5))
    assert np.array_equal(part["kappa"], kw["kappa"][2:5]) and np.array_equal(part["gamma"], [2.0, 3.0, 4.0])
    assert part["alpha"] == 0.5 and np.array_equal(part["a0"], kw["a0"][2:5]) and part["n_steps"] == 3 and part["want_traj"]
    assert cut(dict(kw, a0=np.ones(4, complex)), COMB_AXES, 6, slice(0, 2))["a0"].shape == (4,)


def test_comb_result_reductions_and_their_nan_rule():
    p_end = np.array([[2.0, 4.0, 0.0], [1.0, 1.0, 1.0], [3.0, np.nan, 1.0]])
    r = sweep.CombResult(np.sqrt(np.nan_to_num(p_end)).astype(complex), p_end, 2.0 * p_end, np.array([-1, 7, -1]), 100, 10, 0.0,
                         np.ones((1, 3)))
    g = r.line_gain([1.0, 2.0, 0.0], mode="end", unit="linear")
    assert np.array_equal(g[0, :2], [2.0, 2.0]) and np.isnan(g[0, 2])          # a dark line has no gain
    assert np.isnan(g[1]).all()                                               # a failed point
    assert g[2, 0] == 3.0 and np.isnan(g[2, 1:]).all()                        # a non-finite ratio, a dark line
    assert np.allclose(r.line_gain(np.ones((3, 3)), mode="max")[0, :2], 10 * np.log10([4.0, 8.0]))
    assert np.isnan(r.line_gain(np.ones(3))[0, 2])                            # a ratio of 0 has no dB value
    tp = r.total_power()
    assert tp[0] == 6.0 and np.isnan(tp[1]) and np.isnan(tp[2])
    for bad in (np.ones(2), np.ones((2, 3)), 1.0):
        with pytest.raises(ValueError):
            r.line_gain(bad)
    with pytest.raises(ValueError):
        r.line_gain(np.ones(3), mode="peak")


# ---- the drivers' propagation constants ------------------------------------------------------------------------------------
def _dispersion():
    return dispersion.DispersionParams(omega_ref=2.0 * np.pi * 299792458.0 / 1554e-9, beta2=-2.3e-28, beta3=4.1e-41, beta4=-3.2e-55,
                                       extra={5: 2.0e-70, 6: -1.0e-84})


@pytest.mark.parametrize("M,max_order", [(3, 4), (7, 4), (12, 6), (8, 3)])
def test_driver_kappa_gives_the_mismatch_of_every_product(M, max_order):
    """kappa_k + kappa_l - kappa_n - kappa_m of comb_lines (what scan_comb_gain and run_comb_simulation launch with) is
    delta_beta_from_omegas_array of the four frequencies, for random quadruples k + l = n + m: the gauge term a + b*m cancels,
    beta_0 and beta_1 never enter.  Bar: 1e-12 of the largest |b| involved (the sums are of four numbers of that size)."""
    d = _dispersion()
    wc, dw = 2.0 * np.pi * 299792458.0 / 1550e-9, 2.0 * np.pi * 100e9
    omega, kappa, b = simulation.comb_lines(wc, dw, M, d, max_order=max_order)
    assert omega.shape == kappa.shape == b.shape == (M,) and kappa[0] == 0.0 and abs(kappa[-1]) <= 1e-15 * np.max(np.abs(b))
    assert np.allclose(np.diff(omega), dw, rtol=1e-12) and abs(omega[(M - 1) // 2] + omega[M // 2] - 2.0 * wc) < 1e-3
    rng = np.random.default_rng(M)
    worst, seen = 0.0, 0
    while seen < 200:
        k, l, n = rng.integers(0, M, 3)
        m = k + l - n
        if not 0 <= m < M:
            continue
        seen += 1
        got = kappa[k] + kappa[l] - kappa[n] - kappa[m]
        want = float(dispersion.delta_beta_from_omegas_array(omega[[n, m, k, l]], d, max_order=max_order))
        worst = max(worst, abs(got - want) / np.max(np.abs(b[[k, l, n, m]])))
    print(f"M={M} max_order={max_order}: worst {worst:.2e}")
    assert worst < 1e-12


def test_driver_input_errors():
    d = _dispersion()
    cfg = config.custom_simulation_config(z_max=10.0, dz=0.1)
    ok = dict(cfg=cfg, lambda_center_m=1550e-9, line_spacing=6e11, p_lines=[1e-3, 0.3, 0.3, 1e-3], gamma=0.0115, alpha=0.0,
              dispersion=d)
    for bad in (dict(p_lines=[0.3, 0.3]), dict(p_lines=np.ones(13)), dict(p_lines=[0.3, -1.0, 0.3]), dict(p_lines=np.ones((2, 2, 4))),
                dict(p_lines=[0.3, np.nan, 0.3]), dict(phase_in=[0.0, 1.0]), dict(line_spacing=0.0), dict(line_spacing=float("inf")),
                dict(line_spacing=1e15), dict(dispersion=None), dict(max_order=1), dict(gain_mode="peak"), dict(gain_unit="nepers"),
                dict(length_unit="mile"), dict(devices=[])):
        with pytest.raises(ValueError):
            scan_mismtach.scan_comb_gain(**dict(ok, **bad))
    run = dict(gamma=0.0115, alpha=0.0, omega_center=1.2e15, line_spacing=6e11, p_in=[1e-3, 0.3, 0.3, 1e-3], dispersion=d)
    for bad in (dict(p_in=np.ones((2, 4))), dict(p_in=[0.3, 0.3]), dict(phase_in=[0.0] * 5), dict(omega_center=-1.0),
                dict(line_spacing=-1.0), dict(dispersion=None), dict(length_unit="mile")):
        with pytest.raises(ValueError):
            simulation.run_comb_simulation(cfg, **dict(run, **bad))
    with pytest.raises(TypeError):
        simulation.run_comb_simulation(cfg, **dict(run, max_order=4.0))
