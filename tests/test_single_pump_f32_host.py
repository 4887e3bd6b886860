"""The float32 single-pump sweep without a GPU: psa_rk4_single_pump_f32 / _f32_dev are exported and bound as the header declares
them, every argument code comes back before any device call in the order of the float64 forms (PSA_OPT_F32_SCALAR and
PSA_OPT_F32_PACKED are refused: there is one float32 layout), an empty sweep is a no-op, and the Python wrappers' dtype rules."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import psa_amd._native as nat
from psa_amd import config, dispersion, scan_mismtach, sweep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NPOINTS, E_NSTEPS, E_ZMAX, E_SAVE_EVERY, E_NULLPTR, E_DEVICE, E_TOO_LARGE, E_FLAGS = -2, -3, -4, -5, -6, -7, -9, -11
NAMES = ("psa_rk4_single_pump_f32", "psa_rk4_single_pump_f32_dev")
_CTYPE = {"int": C.c_int, "int64_t": C.c_int64, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "double": C.c_double}


def _prototype(name):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "psa_rk4.h"), encoding="utf-8").read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, name
    return [d.strip() for d in m.group(1).split(",")]


def test_both_symbols_are_exported_and_bound_as_the_header_declares():
    for name in NAMES:
        decls = _prototype(name)
        args = [C.c_void_p if "*" in d else _CTYPE[d.replace("const ", "").split()[0]] for d in decls]
        res, want = nat._SIGS[name]
        assert res is C.c_int and list(want) == args, name
        assert name in nat.EXPORTED_SYMBOLS and hasattr(nat.lib(), name)
        # the float64 form's list with every double buffer a float buffer: z_max and elapsed_ms stay double, the index int64
        twin = _prototype(name.replace("f32", "f64"))
        assert len(twin) == len(decls)
        for d32, d64 in zip(decls, twin):
            if "*" in d64 and "double" in d64 and "elapsed_ms" not in d64:
                assert d32 == d64.replace("double", "float"), (d32, d64)
            else:
                assert d32 == d64, (d32, d64)
    src = open(os.path.join(ROOT, "include", "psa_rk4.h"), encoding="utf-8").read()
    codes = [int(x) for x in re.findall(r"#define\s+PSA_E_\w+\s+(-\d+)", src)]
    assert sorted(codes) == list(range(-13, 0))                              # no new error code


def _dev(n=8, steps=10, z=1.0, se=1, flags=0, null=False, traj=False):
    """psa_rk4_single_pump_f32_dev with dummy pointers: every call here must fail in validation, before any launch."""
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    q = None if null else p
    return nat.lib().psa_rk4_single_pump_f32_dev(None, n, steps, z, se, q, p, p, p, flags, p, p, p, p, p if traj else None)


def _host(n=8, steps=10, z=1.0, se=1, flags=0, null=False, traj=False):
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    q = None if null else p
    return nat.lib().psa_rk4_single_pump_f32(0, n, steps, z, se, p, p, p, p, flags, p, p, q, p, p if traj else None, None)


@pytest.mark.parametrize("call", [_dev, _host], ids=["dev", "host"])
def test_every_argument_error_comes_back_before_any_device_call(call):
    assert call(n=-1) == E_NPOINTS
    assert call(n=nat.MAX_POINTS + 1) == E_TOO_LARGE
    assert call(steps=0) == E_NSTEPS and call(steps=2**31) == E_NSTEPS
    assert call(z=0.0) == E_ZMAX and call(z=float("inf")) == E_ZMAX and call(z=float("nan")) == E_ZMAX
    assert call(se=0) == E_SAVE_EVERY
    assert call(null=True) == E_NULLPTR
    for bit in (nat.OPT_F32_SCALAR, nat.OPT_F32_PACKED, nat.OPT_ONE_LANE, nat.OPT_SPLIT_POINT, nat.OPT_QUAD_POINT,
                nat.OPT_LDS_STAGING, nat.BCAST_TRANSFER, 1 << 19, 1 << 30):
        assert call(flags=bit | nat.OPT_CHECK_NAN) == E_FLAGS, bit
    assert b"only" in nat.lib().psa_last_error()
    # the order of the float64 forms: the grid before the flags, the flags before the pointers, the pointers before the bound
    assert call(n=-1, flags=nat.OPT_F32_PACKED, null=True) == E_NPOINTS
    assert call(flags=nat.OPT_F32_PACKED, null=True) == E_FLAGS
    assert call(n=2**28, flags=nat.OPT_F32_SCALAR, traj=True) == E_FLAGS
    assert call(n=2**28, traj=True, null=True) == E_NULLPTR


def test_the_padded_leading_dimension_belongs_to_the_device_form():
    assert _host(flags=nat.OPT_TRAJ_LD) == E_FLAGS and _host(flags=nat.OPT_TRAJ_LD, traj=True) == E_FLAGS
    # on the _dev form the flag passes validation: the next rule (here: a NULL pointer) is the one that answers
    assert _dev(flags=nat.OPT_TRAJ_LD, traj=True, null=True) == E_NULLPTR


@pytest.mark.parametrize("call", [_dev, _host], ids=["dev", "host"])
def test_the_trajectory_bound_is_the_packed_sweeps(call):
    """psa_rk4_sweep_f32 takes a packed trajectory launch while n_points * 8 B < 2^31 (the lane's 32-bit byte offset); here the
    leading dimension ld = N or psa_traj_ld(N, 4) takes the place of n_points.  2^28 points are 2 GiB of pairs: refused with
    and (on the `_dev` form) without the padding, and accepted without a trajectory (dummy pointers: the call then stops at
    the NULL-pointer rule, not at the size)."""
    assert call(n=2**28, traj=True) == E_TOO_LARGE
    assert call(n=2**28, traj=False, null=True) == E_NULLPTR
    if call is _dev:
        assert nat.traj_ld(2**28, np.float32) == 2**28 + 544
        assert call(n=2**28, traj=True, flags=nat.OPT_TRAJ_LD) == E_TOO_LARGE
    # the same size through psa_rk4_sweep_f32_dev: the bound this one copies
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    assert nat.lib().psa_rk4_sweep_f32_dev(None, 4, 2**28, 10, 1.0, 1, p, None, p, p, p, 0, p, p, p, p, p) == E_TOO_LARGE
    assert nat.lib().psa_rk4_sweep_f32_dev(None, 4, 2**28 - 1, 10, 1.0, 1, None, None, p, p, p, 0, p, p, p, p, p) == E_NULLPTR


def test_an_empty_sweep_is_a_successful_no_op():
    L = nat.lib()
    assert L.psa_rk4_single_pump_f32_dev(None, 0, 10, 1.0, 1, None, None, None, None, 0, None, None, None, None, None) == 0
    ms = C.c_double(7.0)
    assert L.psa_rk4_single_pump_f32(0, 0, 10, 1.0, 1, None, None, None, None, 0, None, None, None, None, None,
                                     C.cast(C.byref(ms), C.c_void_p)) == 0
    assert L.psa_rk4_single_pump_f32(0, 0, 10, 1.0, 1, None, None, None, None, 0, None, None, None, None, None, None) == 0


@pytest.mark.skipif(nat.device_count() > 0, reason="CPU box only")
def test_without_a_device_a_valid_call_is_an_error_not_a_fallback():
    with pytest.raises(nat.PsaNativeError) as e:
        nat.single_pump_host(np.zeros(3), n_steps=1, z_max=1.0, save_every=1, gamma=1.0, alpha=0.0, a0=np.ones(3, complex),
                             dtype=np.float32)
    assert e.value.code == E_DEVICE and "no CPU fallback" in str(e.value)


# ---- Python --------------------------------------------------------------------------------------------------------------
def test_python_shape_and_dtype_rules():
    kw = dict(n_steps=1, z_max=1.0, save_every=1, gamma=1.0, alpha=0.0)
    for dbeta, a0 in ((np.zeros((3, 1)), np.ones(3, complex)), (np.zeros(3), np.ones(4, complex)),
                      (np.zeros(3), np.ones((2, 3), complex))):
        with pytest.raises(ValueError):
            nat.single_pump_host(dbeta, a0=a0, dtype=np.float32, **kw)
    ok = dict(gamma=1.0, alpha=0.0, a0=np.ones(3, complex))
    for bad in (np.float16, np.int32, np.int64, np.complex64, "int8"):
        with pytest.raises(ValueError):
            nat.single_pump_host(np.zeros(3), dtype=bad, **kw, a0=np.ones(3, complex))
        with pytest.raises(ValueError):
            nat.single_pump_device(stream=0, n_points=0, n_steps=1, z_max=1.0, save_every=1, d_dbeta=0, d_gamma=0, d_alpha=0,
                                   d_a0_soa=0, flags=0, d_a_end_soa=0, d_p_wave_end_soa=0, d_p_wave_max_soa=0, d_first_bad=0,
                                   dtype=bad)
        with pytest.raises(ValueError):
            sweep.rk4_sweep_single_pump(np.zeros(3), z_max=1.0, dz=0.1, dtype=bad, **ok)
    with pytest.raises(ValueError):
        sweep.rk4_sweep_single_pump(np.zeros(3), z_max=1.0, dz=0.1, dtype=np.float32, gamma=1.0, alpha=0.0, a0=np.ones(4, complex))
    with pytest.raises(ValueError):
        sweep.rk4_sweep_single_pump(np.zeros(3), z_max=1.0, dz=0.1, dtype=np.float32, devices=[], **ok)


def _spy(monkeypatch):
    """Replace the entry-point lookup by one that records which face was asked for and returns a function that does nothing."""
    asked = []

    def fake_fn(stem, f64=True, dev=False):
        asked.append((stem, bool(f64), bool(dev)))
        return lambda *args: 0
    monkeypatch.setattr(nat, "_fn", fake_fn)
    return asked


def test_without_a_dtype_the_float64_face_is_called(monkeypatch):
    asked = _spy(monkeypatch)
    kw = dict(z_max=1.0, n_steps=4, save_every=2, gamma=1.0, alpha=0.0, a0=np.ones(3, complex), want_traj=True)
    r = sweep.rk4_sweep_single_pump(np.zeros(5), **kw)
    assert asked == [("psa_rk4_single_pump", True, False)]
    assert r.a_end.dtype == np.complex128 and r.p_wave_end.dtype == np.float64 and r.traj.dtype == np.complex128
    r = sweep.rk4_sweep_single_pump(np.zeros(5), dtype=np.float64, **kw)
    assert asked[-1] == ("psa_rk4_single_pump", True, False) and r.a_end.dtype == np.complex128
    r = sweep.rk4_sweep_single_pump(np.zeros(5), dtype=np.float32, **kw)
    assert asked[-1] == ("psa_rk4_single_pump", False, False)
    assert r.a_end.dtype == np.complex64 and r.a_end.shape == (5, 3) and r.p_wave_end.dtype == r.p_wave_max.dtype == np.float32
    assert r.traj.dtype == np.complex64 and r.traj.shape == (5, 3, 3) and r.first_bad_step.dtype == np.int64
    assert r.p_wave_in.dtype == np.float32
    nat.single_pump_device(stream=0, n_points=0, n_steps=1, z_max=1.0, save_every=1, d_dbeta=0, d_gamma=0, d_alpha=0, d_a0_soa=0,
                           flags=0, d_a_end_soa=0, d_p_wave_end_soa=0, d_p_wave_max_soa=0, d_first_bad=0)
    assert asked[-1] == ("psa_rk4_single_pump", True, True)
    nat.single_pump_device(stream=0, n_points=0, n_steps=1, z_max=1.0, save_every=1, d_dbeta=0, d_gamma=0, d_alpha=0, d_a0_soa=0,
                           flags=0, d_a_end_soa=0, d_p_wave_end_soa=0, d_p_wave_max_soa=0, d_first_bad=0, dtype=np.float32)
    assert asked[-1] == ("psa_rk4_single_pump", False, True)


def test_the_inputs_reach_the_float32_face_rounded_once(monkeypatch):
    """dbeta, gamma, alpha and a0 arrive as float32 / complex64 buffers with the BCAST bits of the float64 wrapper."""
    seen = {}

    def fake_fn(stem, f64=True, dev=False):
        def call(device, n, n_steps, z_max, se, dbeta, gamma, alpha, a0, flags, *outs):
            seen.update(n=n, flags=flags, dbeta=np.ctypeslib.as_array(C.cast(dbeta, C.POINTER(C.c_float)), (n,)).copy(),
                        gamma=np.ctypeslib.as_array(C.cast(gamma, C.POINTER(C.c_float)), (1,)).copy())
            return 0
        return call
    monkeypatch.setattr(nat, "_fn", fake_fn)
    db = np.array([0.1, -1.0 / 3.0, 2.0 / 3.0])
    nat.single_pump_host(db, n_steps=2, z_max=1.0, save_every=1, gamma=0.0115, alpha=np.zeros(3), a0=np.ones(3, complex),
                         dtype=np.float32)
    assert seen["n"] == 3 and np.array_equal(seen["dbeta"], db.astype(np.float32)) and seen["gamma"][0] == np.float32(0.0115)
    assert seen["flags"] == nat.BCAST_GAMMA | nat.BCAST_A0 | nat.OPT_CHECK_NAN | nat.OPT_EXACT_STEP


def test_the_gain_driver_passes_the_dtype_on(golden, monkeypatch):
    dv = golden("G11")["disp_m"]
    d = dispersion.DispersionParams(omega_ref=dv[0], beta2=dv[1], beta3=dv[2], beta4=dv[3])
    asked = _spy(monkeypatch)
    cfg = config.custom_simulation_config(z_max=10.0, dz=0.1)
    kw = dict(cfg=cfg, lambda_pump_m=1550e-9, lambda_signal_m=[1540e-9, 1545e-9], p_pump=0.5, p_signal=1e-6, gamma=0.0115,
              alpha=1e-4, dispersion=d)
    out = scan_mismtach.scan_single_pump_gain(**kw)
    assert asked[-1] == ("psa_rk4_single_pump", True, False) and out["result"].a_end.dtype == np.complex128
    out = scan_mismtach.scan_single_pump_gain(dtype=np.float32, **kw)
    assert asked[-1] == ("psa_rk4_single_pump", False, False) and out["result"].a_end.dtype == np.complex64
    assert out["dbeta"].dtype == np.float64                                  # formed in float64 on the host
    with pytest.raises(ValueError):
        scan_mismtach.scan_single_pump_gain(dtype=np.float16, **kw)
