"""The multi-channel sweep without a GPU: the NumPy restatement (tests/pairs_np.py) pinned to the oracle's 6-wave statement
and to numbers the reference produced (golden G8), the argument rules of psa_rk4_sweep_pairs_f64 / _dev (every code comes
back before any device call), the Python wrappers' shape rules and PairsResult's reductions."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pairs_np
import psa_amd._native as nat
from conftest import RTOL_F64, rel_err
from psa_amd import config, dispersion, scan_mismtach, sweep
from psa_amd._partition import PAIRS_AXES, cut

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NPOINTS, E_NSTEPS, E_ZMAX, E_SAVE_EVERY, E_NULLPTR, E_DEVICE, E_TOO_LARGE, E_FLAGS, E_NPAIRS = -2, -3, -4, -5, -6, -7, -9, -11, -13


def test_restatement_rhs_at_two_pairs_is_the_oracles_six_wave_statement(oracle):
    rng = np.random.default_rng(0)
    for _ in range(16):
        a = rng.normal(size=6) + 1j * rng.normal(size=6)
        z, g, al, d1, d2 = rng.uniform(0, 50), rng.uniform(0.005, 0.02), rng.uniform(0, 1e-3), *rng.uniform(-0.05, 0.05, 2)
        got = pairs_np.rhs(z, a[None], [g], [al], np.array([[d1, d2]]))[0]
        assert np.max(np.abs(got - oracle.np_rhs6(z, a, g, al, d1, d2))) <= 1e-15


@pytest.mark.parametrize("K", [3, 16])
def test_restatement_with_one_pair_lit_reproduces_the_reference(golden, K):
    """Every 16th point of G8's 1e4-step lossy sweep, the light in the last pair, random mismatches on the dark ones: the
    yardstick of the GPU tests is itself pinned to numbers the reference produced."""
    g = golden("G8")
    db = g["dbeta257"][::16]
    rng = np.random.default_rng(K)
    dbeta = rng.uniform(-0.05, 0.05, (db.size, K))
    dbeta[:, K - 1] = db
    w = [0, 1, 2 * K, 2 * K + 1]
    a0 = np.zeros(2 + 2 * K, complex)
    a0[w] = np.sqrt(g["p_in"])
    r = pairs_np.integrate(a0, dbeta, z_max=float(g["z_max"]), n=10_000, save_every=10, gamma=float(g["gamma"]),
                           alpha=float(g["alphas"][1]))
    assert rel_err(r["a_end"][:, w], g["n1e4_a1_A_end"][::16]) < RTOL_F64
    assert rel_err(r["p_wave_max"][:, 2 * K], g["n1e4_a1_p_max"][::16]) < RTOL_F64
    dark = [c for c in range(2 + 2 * K) if c not in w]
    assert np.all(r["a_end"][:, dark] == 0) and (r["first_bad_step"] == -1).all()


def test_restatement_save_rows_and_failure_index():
    a0 = np.zeros(8, complex)
    a0[:2], a0[2::2] = np.sqrt(0.5), np.sqrt(1e-5)
    db = np.array([[0.01, 0.02, -0.01]])
    kw = dict(z_max=10.0, gamma=0.0115, alpha=1e-4)
    full = pairs_np.integrate(a0, db, n=25, save_every=1, **kw)
    strided = pairs_np.integrate(a0, db, n=25, save_every=10, **kw)
    at20 = pairs_np.integrate(a0, db, z_max=8.0, n=20, save_every=1, gamma=0.0115, alpha=1e-4)
    assert rel_err(strided["a_end"], at20["a_end"]) < 1e-13 and rel_err(strided["a_end"], full["a_end"]) > 1e-6
    none = pairs_np.integrate(a0, db, n=7, save_every=10, **kw)
    assert np.array_equal(none["a_end"][0], a0) and np.array_equal(none["p_wave_max"], np.abs(none["a_end"]) ** 2)
    bad = pairs_np.integrate(a0, np.repeat(db, 2, axis=0), z_max=200.0, n=2000, save_every=10, gamma=0.0115,
                             alpha=np.array([-12.0, 1e-4]))
    assert bad["first_bad_step"][0] >= 0 and bad["first_bad_step"][1] == -1 and np.isnan(bad["p_wave_max"][0]).all()


def _dev(n_pairs=3, n=8, steps=10, z=1.0, se=1, flags=0, null=False):
    """psa_rk4_sweep_pairs_f64_dev with dummy pointers: every call here must fail in validation, before any launch."""
    buf = np.zeros(64)
    p = buf.ctypes.data_as(C.c_void_p)
    q = None if null else p
    return nat.lib().psa_rk4_sweep_pairs_f64_dev(None, n_pairs, n, steps, z, se, q, p, p, p, flags, p, p, p, p)


def _host(n_pairs=3, n=8, steps=10, z=1.0, se=1, flags=0, null=False):
    buf = np.zeros(64)
    p = buf.ctypes.data_as(C.c_void_p)
    q = None if null else p
    return nat.lib().psa_rk4_sweep_pairs_f64(0, n_pairs, n, steps, z, se, p, p, p, p, flags, p, p, q, p, None)


@pytest.mark.parametrize("call", [_dev, _host], ids=["dev", "host"])
def test_every_argument_error_comes_back_before_any_device_call(call):
    assert call(n_pairs=0) == E_NPAIRS and call(n_pairs=17) == E_NPAIRS and call(n_pairs=-1) == E_NPAIRS
    assert b"n_pairs" in nat.lib().psa_last_error()
    assert call(n=-1) == E_NPOINTS
    assert call(steps=0) == E_NSTEPS and call(steps=2**31) == E_NSTEPS
    assert call(z=0.0) == E_ZMAX and call(z=float("inf")) == E_ZMAX and call(z=float("nan")) == E_ZMAX
    assert call(se=0) == E_SAVE_EVERY
    assert call(null=True) == E_NULLPTR
    for bit in (nat.OPT_ONE_LANE, nat.OPT_SPLIT_POINT, nat.OPT_QUAD_POINT, nat.OPT_F32_SCALAR, nat.OPT_F32_PACKED,
                nat.OPT_LDS_STAGING, nat.OPT_TRAJ_LD, nat.BCAST_TRANSFER, 1 << 30):
        assert call(flags=bit | nat.OPT_CHECK_NAN) == E_FLAGS, bit
    assert b"only" in nat.lib().psa_last_error()


@pytest.mark.parametrize("call", [_dev, _host], ids=["dev", "host"])
def test_the_launch_limit_knows_the_lanes_per_point(call):
    """L * n_points lanes must fit the launch grid (2 * PSA_MAX_POINTS = 2^32 - 512 threads): the limit on n_points falls
    with the lane count -- 1 and 2 pairs: 2 lanes, 3..4: 4, 5..8: 8, 9..16: 16."""
    lanes = 2 * nat.MAX_POINTS
    for n_pairs, L in ((1, 2), (2, 2), (3, 4), (4, 4), (5, 8), (8, 8), (9, 16), (16, 16)):
        assert call(n_pairs=n_pairs, n=lanes // L + 1) == E_TOO_LARGE, n_pairs
    assert call(n_pairs=16, n=2**31) == E_TOO_LARGE and b"lanes per point" in nat.lib().psa_last_error()


def test_an_empty_sweep_is_a_successful_no_op():
    L = nat.lib()
    assert L.psa_rk4_sweep_pairs_f64_dev(None, 5, 0, 10, 1.0, 1, None, None, None, None, 0, None, None, None, None) == 0
    assert L.psa_rk4_sweep_pairs_f64(0, 5, 0, 10, 1.0, 1, None, None, None, None, 0, None, None, None, None, None) == 0


def test_header_constants_match_the_binding():
    src = open(os.path.join(ROOT, "include", "psa_rk4.h"), encoding="utf-8").read()
    assert int(re.search(r"#define\s+PSA_E_NPAIRS\s+(-\d+)", src).group(1)) == E_NPAIRS
    assert int(re.search(r"#define\s+PSA_MAX_PAIRS\s+(\d+)", src).group(1)) == nat.MAX_PAIRS == 16
    codes = [int(x) for x in re.findall(r"#define\s+PSA_E_\w+\s+(-\d+)", src)]
    assert sorted(codes) == list(range(-13, 0))            # the next free code, no gap and no clash


@pytest.mark.skipif(nat.device_count() > 0, reason="CPU box only")
def test_without_a_device_a_valid_call_is_an_error_not_a_fallback():
    with pytest.raises(nat.PsaNativeError) as e:
        nat.sweep_pairs_host(np.zeros((3, 2)), n_steps=1, z_max=1.0, save_every=1, gamma=1.0, alpha=0.0, a0=np.ones(6, complex))
    assert e.value.code == E_DEVICE and "no CPU fallback" in str(e.value)


def test_python_wrapper_shape_rules():
    kw = dict(n_steps=1, z_max=1.0, save_every=1, gamma=1.0, alpha=0.0)
    for dbeta, a0 in ((np.zeros(3), np.ones(4, complex)),                  # dbeta must be (N, K)
                      (np.zeros((3, 17)), np.ones(36, complex)),            # more than 16 pairs
                      (np.zeros((3, 0)), np.ones(2, complex)),              # no pair
                      (np.zeros((3, 2)), np.ones(4, complex)),              # a0 of another K
                      (np.zeros((3, 2)), np.ones((2, 6), complex)),         # neither 1 nor N rows
                      (np.zeros((3, 2)), np.ones((3, 2, 6), complex))):
        with pytest.raises(ValueError):
            nat.sweep_pairs_host(dbeta, a0=a0, **kw)
    with pytest.raises(ValueError):
        nat.sweep_pairs_host(np.zeros((3, 2)), a0=np.ones(6, complex), **dict(kw, gamma=[1.0, 2.0]))
    ok = dict(gamma=1.0, alpha=0.0, a0=np.ones(6, complex))
    for bad in (dict(z_max=0.0, dz=0.1), dict(z_max=1.0), dict(z_max=1.0, dz=-0.1), dict(z_max=1.0, dz=0.1, save_every=0),
                dict(z_max=1.0, dz=10.0), dict(z_max=1.0, dz=0.1, devices=[])):
        with pytest.raises(ValueError):
            sweep.rk4_sweep_pairs(np.zeros((3, 2)), **ok, **bad)
    with pytest.raises(ValueError):
        sweep.rk4_sweep_pairs(np.zeros(3), z_max=1.0, dz=0.1, **ok)
    with pytest.raises(ValueError):
        sweep.rk4_sweep_pairs(np.zeros((3, 2)), z_max=1.0, dz=0.1, gamma=1.0, alpha=0.0, a0=np.ones(4, complex))


# the four host wrappers on N = 3 points and 4 waves (one pair; a chain of two spans): valid but for what a case replaces
_WRAPPERS = {"sweep": (nat.sweep_host, dict(dbeta=np.zeros(3), n_steps=1, z_max=1.0, save_every=1)),
             "pairs": (nat.sweep_pairs_host, dict(dbeta=np.zeros((3, 1)), n_steps=1, z_max=1.0, save_every=1)),
             "chain": (nat.chain_host, dict(dbeta=np.zeros((2, 3)), n_steps=[1, 1], seg_len=[1.0, 1.0], save_every=1)),
             "rk45": (nat.rk45_sweep_host, dict(dbeta=np.zeros(3), z_max=1.0, rtol=1e-8, atol=1e-12))}
_WRONG = {"gamma_2d": dict(gamma=np.ones((3, 2))), "alpha_wrong_length": dict(alpha=np.ones(4)),
          "a0_wrong_width": dict(a0=np.ones(5, complex)), "a0_wrong_row_count": dict(a0=np.ones((2, 4), complex)),
          "a0_3d": dict(a0=np.ones((3, 1, 4), complex)), "six_waves_without_dbeta2": dict(a0=np.ones(6, complex)),
          "four_waves_with_dbeta2": dict(dbeta2=0)}       # 0: replaced by zeros shaped as the wrapper's dbeta


@pytest.mark.parametrize("wrapper,wrong", [(w, x) for w in sorted(_WRAPPERS) for x in sorted(_WRONG)
                                           if (w, x) != ("pairs", "four_waves_with_dbeta2")])   # pairs take no dbeta2
def test_the_host_wrappers_share_their_per_point_shape_rules(wrapper, wrong):
    """One helper prepares gamma, alpha, a0 and dbeta2 for all four: each wrapper refuses the same wrong inputs with a
    ValueError, before any native call."""
    fn, kw = _WRAPPERS[wrapper]
    bad = dict(_WRONG[wrong])
    if "dbeta2" in bad:
        bad["dbeta2"] = np.zeros_like(kw["dbeta"])
    with pytest.raises(ValueError):
        fn(**dict(kw, gamma=1.0 if wrapper != "chain" else [1.0, 1.0], alpha=0.0 if wrapper != "chain" else [0.0, 0.0],
                  a0=np.ones(4, complex)) | bad)


def test_the_device_split_cuts_dbeta_by_points():
    kw = dict(dbeta=np.arange(12.0).reshape(6, 2), gamma=np.arange(6.0), alpha=0.5, a0=np.ones((6, 6), complex), n_steps=3)
    part = cut(kw, PAIRS_AXES, 6, slice(2, 5))
    assert np.array_equal(part["dbeta"], kw["dbeta"][2:5]) and np.array_equal(part["gamma"], [2.0, 3.0, 4.0])
    assert part["alpha"] == 0.5 and part["a0"].shape == (3, 6) and part["n_steps"] == 3
    square = cut(dict(kw, dbeta=np.zeros((6, 6)), a0=np.ones(14, complex)), PAIRS_AXES, 6, slice(0, 2))
    assert square["dbeta"].shape == (2, 6) and square["a0"].shape == (14,)      # a broadcast a0 passes through


def _result():
    # N = 3 points, K = 2 pairs: waves [p1, p2, s1, i1, s2, i2]
    end = np.array([[0.4, 0.3, 2e-3, 1e-3, 4e-4, 0.0],
                    [0.5, 0.5, 1e-4, 1e-5, 1e-5, 1e-6],
                    [0.1, 0.1, 1.0, 1.0, 1.0, 1.0]])
    mx = end * np.array([1.25, 1.0, 2.0, 1.0, 1.0, 1.0])
    bad = np.array([-1, -1, 41])
    return sweep.PairsResult(np.sqrt(end).astype(complex), end, mx, bad, 100, 10, 0.0, np.array([[0.5, 0.5, 1e-5, 0, 1e-5, 0]]))


def test_pairs_result_reductions_and_their_nan_rule():
    r = _result()
    assert r.n_pairs == 2
    g = r.channel_gain([1e-5, 1e-5], mode="end", unit="linear")
    assert g.shape == (3, 2) and np.allclose(g[:2], [[200.0, 40.0], [10.0, 1.0]], rtol=1e-14) and np.isnan(g[2]).all()
    g = r.channel_gain([1e-5, 1e-5])                                   # max, dB
    assert np.allclose(g[:2], 10 * np.log10([[400.0, 40.0], [20.0, 1.0]]), rtol=1e-14) and np.isnan(g[2]).all()
    per_point = np.array([[1e-5, 2e-5], [0.0, 1e-5], [1e-5, 1e-5]])    # a dark seed defines no gain
    g = r.channel_gain(per_point, mode="end", unit="linear")
    assert np.allclose(g[0], [200.0, 20.0]) and np.isnan(g[1, 0]) and g[1, 1] == pytest.approx(1.0) and np.isnan(g[2]).all()
    c = r.idler_conversion([1e-5, 1e-5], mode="end", unit="linear")
    assert c[0, 0] == pytest.approx(100.0) and np.isnan(c[0, 1])       # an idler that stayed dark: no (log of) zero
    assert np.allclose(c[1], [1.0, 0.1]) and np.isnan(c[2]).all()
    d = r.pump_depletion()
    assert d.shape == (3,) and np.allclose(d[:2], [0.3, 0.0], atol=1e-15) and np.isnan(d[2])
    for bad in (dict(mode="mean"), dict(unit="neper")):
        with pytest.raises(ValueError):
            r.channel_gain([1e-5, 1e-5], **bad)
    with pytest.raises(ValueError):
        r.channel_gain([1e-5, 1e-5, 1e-5])
    with pytest.raises(ValueError):
        r.idler_conversion(np.ones((2, 2)))


def test_wdm_driver_input_errors(golden):
    dv = golden("G11")["disp_m"]
    d = dispersion.DispersionParams(omega_ref=dv[0], beta2=dv[1], beta3=dv[2], beta4=dv[3])
    ok = dict(cfg=config.custom_simulation_config(z_max=10.0, dz=0.1), lambda_p1_m=1550e-9, lambda_p2_m=1556e-9,
              Omega=[2e12, 3e12], p_pump=[0.3, 0.25], p_signal=[1e-6, 1e-6], gamma=0.0115, alpha=1e-4, dispersion=d)
    for bad in (dict(Omega=[]), dict(Omega=np.linspace(1e12, 2e12, 17), p_signal=np.full(17, 1e-6)), dict(Omega=[2e12, np.nan]),
                dict(Omega=[2e12, 1e16]), dict(p_pump=[0.3]), dict(p_pump=[0.3, -0.1]), dict(p_signal=[1e-6]),
                dict(p_signal=[1e-6, 0.0]), dict(p_signal=np.full((2, 3), 1e-6)), dict(p_idler=[1e-7] * 3),
                dict(p_idler=-1e-7), dict(phase_in=[0.0] * 4), dict(dispersion=None), dict(gain_mode="mean"),
                dict(gain_unit="neper")):
        with pytest.raises(ValueError):
            scan_mismtach.scan_wdm_gain(**dict(ok, **bad))
