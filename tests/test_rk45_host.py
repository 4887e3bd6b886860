"""The adaptive (RK45) sweep without a GPU: exported symbols, argument validation before any device is touched, the
AdaptiveConfig rules, the NumPy restatement (tests/rk45_np.py) against G18 (scipy's RK45 on the reference's RHS), and
the host loop of integrate_adaptive against scipy on a linear test equation."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import psa_amd._native as nat
import rk45_np
from psa_amd.config import AdaptiveConfig
from psa_amd.integrators import integrate_adaptive

G18 = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "G18.npz"))
PSA_E_NWAVES, PSA_E_DBETA2, PSA_E_FLAGS, PSA_E_TOL = -1, -8, -11, -12
EPS = np.finfo(float).eps
GOOD = dict(rtol=1e-9, atol=1e-12, h_max=math.inf, first_step=0.0, max_steps=1000)
BAD_TOL = [dict(rtol=50 * EPS), dict(rtol=math.nan), dict(rtol=math.inf), dict(atol=0.0), dict(atol=-1.0),
           dict(atol=math.inf), dict(atol=math.nan), dict(h_max=0.0), dict(h_max=-1.0), dict(h_max=math.nan),
           dict(first_step=-1e-3), dict(first_step=math.inf), dict(first_step=math.nan), dict(max_steps=0)]


def test_library_exports_the_adaptive_entry_points():
    L = nat.lib()
    for name in ("psa_rk45_sweep_f64", "psa_rk45_sweep_f64_dev"):
        assert hasattr(L, name) and name in nat.EXPORTED_SYMBOLS


def _call(dev: bool, *, n_waves=4, n_out=0, flags=0, with_dbeta2=False, **tol):
    t = dict(GOOD, **tol)
    n = 3
    bufs = [np.zeros(n) for _ in range(2)] + [np.ones(1), np.zeros(1), np.ones(2 * n_waves)]
    d2 = np.zeros(n) if with_dbeta2 else None
    outs = [np.empty(2 * n_waves * n), np.empty(n), np.empty(n), np.empty(n, np.int32), np.empty(n),
            np.empty(n, np.int64), np.empty(n, np.int64)]
    p = nat._ptr
    flags |= nat.BCAST_GAMMA | nat.BCAST_ALPHA | nat.BCAST_A0
    head = [None if dev else 0, n_waves, n, 100.0, t["rtol"], t["atol"], t["h_max"], t["first_step"], t["max_steps"],
            n_out, p(bufs[0]), p(d2), p(bufs[2]), p(bufs[3]), p(bufs[4]), flags] + [p(o) for o in outs] + [None]
    L = nat.lib()
    return L.psa_rk45_sweep_f64_dev(*head) if dev else L.psa_rk45_sweep_f64(*head, None)


@pytest.mark.parametrize("dev", [False, True])
def test_argument_errors_come_before_the_device(dev):
    for bad in BAD_TOL:
        assert _call(dev, **bad) == PSA_E_TOL, bad
    assert _call(dev, n_out=-1) == PSA_E_TOL
    for fl in (nat.OPT_CHECK_NAN, nat.OPT_EXACT_STEP, nat.OPT_SPLIT_POINT, nat.OPT_TRAJ_LD, nat.OPT_BLOCK64, 1 << 30):
        assert _call(dev, flags=fl) == PSA_E_FLAGS, fl
    assert _call(dev, n_waves=5) == PSA_E_NWAVES
    assert _call(dev, n_waves=6) == PSA_E_DBETA2
    assert _call(dev, n_waves=4, with_dbeta2=True) == PSA_E_DBETA2


def test_adaptive_config_rejects_what_the_c_abi_rejects():
    AdaptiveConfig().validate()
    AdaptiveConfig(rtol=100 * EPS, h_max=1.0, first_step=0.5, max_steps=1).validate()
    for bad in BAD_TOL:
        with pytest.raises(ValueError):
            AdaptiveConfig(**bad).validate()
    assert AdaptiveConfig() == AdaptiveConfig(rtol=1e-9, atol=1e-12, h_max=math.inf, first_step=0.0, max_steps=1_000_000)
    with pytest.raises(Exception):
        AdaptiveConfig().rtol = 1.0   # frozen


def g18_cases():
    return sorted({k.rsplit("_", 2)[0] for k in G18.files if k.endswith("_a_end")})


def g18_run(case):
    g = {k[len(case) + 1:]: G18[k] for k in G18.files if k.startswith(case + "_")}
    db = np.atleast_1d(g["dbeta"])
    y0 = np.repeat(np.sqrt(g["p_in"]).astype(complex)[:, None], db.size, axis=1)
    n_out = int(g["n_out"]) if "n_out" in g else 0
    r = rk45_np.rk45(rk45_np.rhs4(db, g["gamma"], float(g["alpha"])), y0, float(g["z_max"]), rtol=float(g["rtol"]),
                     atol=float(g["atol"]), max_steps=int(g["max_steps"]), n_out=n_out)
    return g, r


def _rel(got, want):
    return float(np.max(np.abs(got - want)) / np.max(np.abs(want)))


@pytest.mark.parametrize("case", ["g1_r6", "g1_r9", "g1_r11", "sw", "zero", "g9"])
def test_numpy_restatement_reproduces_g18(case):
    assert case in g18_cases()
    g, r = g18_run(case)
    np.testing.assert_array_equal(r["n_accepted"], g["n_accepted"])
    np.testing.assert_array_equal(r["n_rejected"], g["n_rejected"])
    np.testing.assert_array_equal(r["status"], g["status"])
    np.testing.assert_array_equal(r["z_end"], g["z_end"])
    # The restatement's RHS (oracle.np_rhs) and the reference's round differently; over the ~50 000 steps of the G9 runs the
    # difference grows to ~1e-10, so the bound is 1e-12 or 5e-15 per accepted step, whichever is larger
    for k in range(g["a_end"].shape[0]):
        assert _rel(r["a_end"][k], g["a_end"][k]) < max(1e-12, 5e-15 * g["n_accepted"][k]), (case, k)
    # p_max is the small signal's power: relative to the point's largest wave power, as A_end is to its largest wave
    # (a power doubles the amplitude's relative error: 1e-12 on A is 2e-12 on |A|^2)
    p_top = np.max(np.abs(g["a_end"]) ** 2, axis=1)
    assert np.max(np.abs(r["p_max"] - g["p_max"]) / p_top) < 2e-12
    if "rows" in g:
        assert r["traj"].shape == (1,) + g["rows"].shape
        assert np.max(np.abs(r["traj"][0] - g["rows"]) / np.max(np.abs(g["rows"]), axis=0)) < 1e-12


def test_g18_status_two_cases_hit_the_cap():
    g = {k[3:]: G18[k] for k in G18.files if k.startswith("g9_")}
    capped = g["gamma"] >= 50
    assert np.all(g["status"][capped] == 2) and np.all(g["status"][~capped] == 0)
    assert np.all(g["n_accepted"][capped] + g["n_rejected"][capped] == g["max_steps"])
    assert np.all(g["z_end"][capped] < g["z_max"])


def test_host_loop_matches_scipy_on_a_linear_equation():
    scipy_integrate = pytest.importorskip("scipy.integrate")
    lam = -0.3 + 2j
    y0 = np.array([1.0 + 0.5j, -0.25j])
    rhs = lambda z, y, p: p * y  # noqa: E731
    for tol in (AdaptiveConfig(rtol=1e-6, atol=1e-9), AdaptiveConfig(rtol=1e-10, atol=1e-13),
                AdaptiveConfig(rtol=1e-8, atol=1e-12, h_max=0.05, first_step=0.01)):
        kw = dict(method="RK45", rtol=tol.rtol, atol=tol.atol, max_step=tol.h_max)
        if tol.first_step:
            kw["first_step"] = tol.first_step
        ref = scipy_integrate.solve_ivp(lambda z, y: lam * y, (0.0, 3.0), y0, **kw)
        dense = scipy_integrate.solve_ivp(lambda z, y: lam * y, (0.0, 3.0), y0, t_eval=np.linspace(0.0, 3.0, 31), **kw)
        z, rows, info = integrate_adaptive(rhs, 3.0, y0, lam, tol=tol, n_out=30)
        assert info["status"] == 0 and info["z_end"] == 3.0
        init = 1 if tol.first_step else 2
        assert info["n_accepted"] == ref.t.size - 1
        assert info["n_accepted"] + info["n_rejected"] == (ref.nfev - init) // 6
        assert np.max(np.abs(info["y_end"] - ref.y[:, -1])) <= 1e-13 * np.max(np.abs(ref.y[:, -1]))
        np.testing.assert_array_equal(z, dense.t)
        assert np.max(np.abs(rows - dense.y.T)) <= 1e-13 * np.max(np.abs(dense.y))


def test_host_loop_statuses():
    tol = AdaptiveConfig(rtol=1e-9, atol=1e-12, max_steps=5)
    _, rows, info = integrate_adaptive(lambda z, y, p: -y, 100.0, np.ones(2), None, tol=tol, n_out=4)
    assert info["status"] == 2 and info["n_accepted"] + info["n_rejected"] == 5 and info["z_end"] < 100.0
    assert np.all(np.isnan(rows[-1]))
    _, rows, info = integrate_adaptive(lambda z, y, p: -y, 1.0, np.array([np.nan, 1.0]), None, tol=AdaptiveConfig(),
                                       n_out=2)
    assert info["status"] == 1 and info["n_accepted"] == 0 and info["z_end"] == 0.0
    _, _, info = integrate_adaptive(lambda z, y, p: y * y, 2.0, np.ones(1), None, tol=AdaptiveConfig(), n_out=1)
    assert info["status"] == 1 and info["z_end"] < 1.0   # blows up at z = 1


def test_kernel_compiles_without_scratch():
    """Every instantiation of the adaptive kernel keeps its state and seven stage vectors in registers: ScratchSize 0."""
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "psa-simulation-ode-rk-mvp-dispersion_amd", "csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-c",
                          "-I" + os.path.join(root, "include"), "-I" + csrc, "-Wno-unused-function",
                          "-Rpass-analysis=kernel-resource-usage", os.path.join(csrc, "psa_rk45.hip"), "-o", os.devnull],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    names = re.findall(r"Function Name: (\S*rk45_sweep_kernel\S*)", out.stderr)
    scratch = re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stderr)
    assert len(names) == 8 and len(scratch) == 8, out.stderr[-2000:]
    assert all(int(x) == 0 for x in scratch)
