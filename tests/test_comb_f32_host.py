"""The float32 multi-line ("frequency comb") sweep without a GPU: psa_rk4_comb_f32 / _f32_dev are exported and bound as the
header declares them, every argument code comes back before any device call in the order of the float64 forms (n_lines first;
PSA_OPT_F32_SCALAR and PSA_OPT_F32_PACKED are refused: there is one float32 layout), the packed sweep's trajectory bound, the
empty sweep, the Python wrappers' dtype rules, and the unit's device code without scratch memory in every instantiation."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import psa_amd._native as nat
from psa_amd import config, dispersion, scan_mismtach, sweep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NPOINTS, E_NSTEPS, E_ZMAX, E_SAVE_EVERY, E_NULLPTR, E_DEVICE, E_TOO_LARGE, E_FLAGS, E_NLINES = -2, -3, -4, -5, -6, -7, -9, -11, -14
NAMES = ("psa_rk4_comb_f32", "psa_rk4_comb_f32_dev")
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
        assert list(want) == list(nat._SIGS[name.replace("f32", "f64")][1])
    src = open(os.path.join(ROOT, "include", "psa_rk4.h"), encoding="utf-8").read()
    codes = [int(x) for x in re.findall(r"#define\s+PSA_E_\w+\s+\(?(-\d+)\)?", src)]
    assert sorted(codes) == list(range(-14, 0))                              # no new error code


def _dev(M=4, n=8, steps=10, z=1.0, se=1, flags=0, null=False, traj=False):
    """psa_rk4_comb_f32_dev with dummy pointers: every call here must fail in validation, before any launch."""
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    q = None if null else p
    return nat.lib().psa_rk4_comb_f32_dev(None, M, n, steps, z, se, q, p, p, p, flags, p, p, p, p, p if traj else None)


def _host(M=4, n=8, steps=10, z=1.0, se=1, flags=0, null=False, traj=False):
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    q = None if null else p
    return nat.lib().psa_rk4_comb_f32(0, M, n, steps, z, se, p, p, p, p, flags, p, p, q, p, p if traj else None, None)


@pytest.mark.parametrize("call", [_dev, _host], ids=["dev", "host"])
def test_every_argument_error_comes_back_before_any_device_call(call):
    for M in (-1, 0, 2, 13, 64):
        assert call(M=M) == E_NLINES, M
    assert b"n_lines" in nat.lib().psa_last_error()
    for M in range(3, 13):                                                   # every M is served: the next rule answers
        assert call(M=M, null=True) == E_NULLPTR, M
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
    # the float64 order: the line count first, the grid before the flags, the flags before the pointers, those before the bound
    assert call(M=2, n=-1, flags=nat.OPT_F32_PACKED, null=True) == E_NLINES
    assert call(n=-1, flags=nat.OPT_F32_PACKED, null=True) == E_NPOINTS
    assert call(flags=nat.OPT_F32_PACKED, null=True) == E_FLAGS
    assert call(n=2**28, flags=nat.OPT_F32_SCALAR, traj=True) == E_FLAGS
    assert call(n=2**28, traj=True, null=True) == E_NULLPTR
    # PSA_OPT_EXACT_STEP, BLOCK64 and LOSSLESS are accepted: with dummy pointers the call then stops at the NULL-pointer rule
    assert call(flags=nat.OPT_CHECK_NAN | nat.OPT_EXACT_STEP | nat.OPT_BLOCK64 | nat.OPT_LOSSLESS, null=True) == E_NULLPTR


def test_the_padded_leading_dimension_belongs_to_the_device_form():
    assert _host(flags=nat.OPT_TRAJ_LD) == E_FLAGS and _host(flags=nat.OPT_TRAJ_LD, traj=True) == E_FLAGS
    assert _dev(flags=nat.OPT_TRAJ_LD, traj=True, null=True) == E_NULLPTR


@pytest.mark.parametrize("call", [_dev, _host], ids=["dev", "host"])
def test_the_trajectory_bound_is_the_packed_sweeps(call):
    """ld * 8 B < 2^31 (the lane's 32-bit byte offset of the packed kernels), ld = N or psa_traj_ld(N, 4): 2^28 points are
    refused with and (on the `_dev` form) without the padding, 2^28 - 1 dense points pass, and so does any size without a
    trajectory (dummy pointers: the call then stops at the NULL-pointer rule, not at the size)."""
    assert call(n=2**28, traj=True) == E_TOO_LARGE and b"2^28" in nat.lib().psa_last_error()
    assert call(n=2**28, traj=False, null=True) == E_NULLPTR
    if call is _dev:
        assert call(n=2**28 - 1, traj=True, null=True) == E_NULLPTR
        assert nat.traj_ld(2**28, np.float32) == 2**28 + 544
        assert call(n=2**28, traj=True, flags=nat.OPT_TRAJ_LD) == E_TOO_LARGE
        # the padding counts: the largest N whose padded leading dimension stays below 2^28
        n = 2**28 - 1
        while nat.traj_ld(n, np.float32) >= 2**28:
            n -= 1
        assert call(n=n, traj=True, flags=nat.OPT_TRAJ_LD, null=True) == E_NULLPTR
        assert call(n=n + 1, traj=True, flags=nat.OPT_TRAJ_LD) == E_TOO_LARGE


def test_an_empty_sweep_is_a_successful_no_op():
    L = nat.lib()
    assert L.psa_rk4_comb_f32_dev(None, 5, 0, 10, 1.0, 1, None, None, None, None, 0, None, None, None, None, None) == 0
    ms = C.c_double(7.0)
    assert L.psa_rk4_comb_f32(0, 5, 0, 10, 1.0, 1, None, None, None, None, 0, None, None, None, None, None,
                              C.cast(C.byref(ms), C.c_void_p)) == 0 and ms.value == 0.0
    assert L.psa_rk4_comb_f32(0, 12, 0, 10, 1.0, 1, None, None, None, None, 0, None, None, None, None, None, None) == 0
    assert L.psa_rk4_comb_f32(0, 2, 0, 10, 1.0, 1, None, None, None, None, 0, None, None, None, None, None, None) == E_NLINES


@pytest.mark.skipif(nat.device_count() > 0, reason="CPU box only")
def test_without_a_device_a_valid_call_is_an_error_not_a_fallback():
    with pytest.raises(nat.PsaNativeError) as e:
        nat.comb_host(np.zeros((3, 4)), n_steps=1, z_max=1.0, save_every=1, gamma=1.0, alpha=0.0, a0=np.ones(4, complex),
                      dtype=np.float32)
    assert e.value.code == E_DEVICE and "no CPU fallback" in str(e.value)


# ---- Python --------------------------------------------------------------------------------------------------------------
def _dispersion(golden):
    dv = golden("G11")["disp_m"]
    return dispersion.DispersionParams(omega_ref=dv[0], beta2=dv[1], beta3=dv[2], beta4=dv[3])


def _gain_kw(golden):
    return dict(cfg=config.custom_simulation_config(z_max=10.0, dz=0.1), lambda_center_m=1550e-9, line_spacing=2.0 * np.pi * 200e9,
                p_lines=[[1e-6, 0.3, 0.0, 0.3, 1e-6], [1e-5, 0.3, 0.0, 0.3, 1e-5]], gamma=0.0115, alpha=1e-4,
                dispersion=_dispersion(golden))


def test_python_shape_and_dtype_rules(golden):
    kw = dict(n_steps=1, z_max=1.0, save_every=1, gamma=1.0, alpha=0.0)
    for kappa, a0 in ((np.zeros(4), np.ones(4, complex)), (np.zeros((3, 2)), np.ones(2, complex)),
                      (np.zeros((3, 13)), np.ones(13, complex)), (np.zeros((3, 4)), np.ones(5, complex)),
                      (np.zeros((3, 4)), np.ones((2, 4), complex))):
        with pytest.raises(ValueError):
            nat.comb_host(kappa, a0=a0, dtype=np.float32, **kw)
        with pytest.raises(ValueError):
            sweep.rk4_sweep_comb(kappa, z_max=1.0, dz=0.1, gamma=1.0, alpha=0.0, a0=a0, dtype=np.float32)
    ok = dict(gamma=1.0, alpha=0.0, a0=np.ones(4, complex))
    for bad in (np.float16, np.int32, np.int64, np.complex64, "int8"):
        with pytest.raises(ValueError):
            nat.comb_host(np.zeros((3, 4)), dtype=bad, **kw, a0=np.ones(4, complex))
        with pytest.raises(ValueError):
            nat.comb_device(stream=0, n_lines=4, n_points=0, n_steps=1, z_max=1.0, save_every=1, d_kappa_soa=0, d_gamma=0, d_alpha=0,
                            d_a0_soa=0, flags=0, d_a_end_soa=0, d_p_wave_end_soa=0, d_p_wave_max_soa=0, d_first_bad=0, dtype=bad)
        with pytest.raises(ValueError):
            sweep.rk4_sweep_comb(np.zeros((3, 4)), z_max=1.0, dz=0.1, dtype=bad, **ok)
        with pytest.raises(ValueError):
            scan_mismtach.scan_comb_gain(dtype=bad, **_gain_kw(golden))
    with pytest.raises(ValueError):
        sweep.rk4_sweep_comb(np.zeros((3, 4)), z_max=1.0, dz=0.1, dtype=np.float32, devices=[], **ok)


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
    kw = dict(z_max=1.0, n_steps=4, save_every=2, gamma=1.0, alpha=0.0, a0=np.ones(5, complex), want_traj=True)
    r = sweep.rk4_sweep_comb(np.zeros((6, 5)), **kw)
    assert asked == [("psa_rk4_comb", True, False)]
    assert r.a_end.dtype == np.complex128 and r.p_wave_end.dtype == np.float64 and r.traj.dtype == np.complex128
    r = sweep.rk4_sweep_comb(np.zeros((6, 5)), dtype=np.float64, **kw)
    assert asked[-1] == ("psa_rk4_comb", True, False) and r.a_end.dtype == np.complex128
    r = sweep.rk4_sweep_comb(np.zeros((6, 5)), dtype=np.float32, **kw)
    assert asked[-1] == ("psa_rk4_comb", False, False)
    assert r.a_end.dtype == np.complex64 and r.a_end.shape == (6, 5) and r.p_wave_end.dtype == r.p_wave_max.dtype == np.float32
    assert r.traj.dtype == np.complex64 and r.traj.shape == (6, 3, 5) and r.first_bad_step.dtype == np.int64
    assert r.p_wave_in.dtype == np.float32
    dev = dict(stream=0, n_lines=5, n_points=0, n_steps=1, z_max=1.0, save_every=1, d_kappa_soa=0, d_gamma=0, d_alpha=0, d_a0_soa=0,
               flags=0, d_a_end_soa=0, d_p_wave_end_soa=0, d_p_wave_max_soa=0, d_first_bad=0)
    nat.comb_device(**dev)
    assert asked[-1] == ("psa_rk4_comb", True, True)
    nat.comb_device(dtype=np.float32, **dev)
    assert asked[-1] == ("psa_rk4_comb", False, True)


def _record(monkeypatch, real):
    """Replace the entry-point lookup by one whose function copies the inputs it is handed, as arrays of ``real``."""
    seen = {}

    def fake_fn(stem, f64=True, dev=False):
        def call(device, M, n, n_steps, z_max, se, kappa, gamma, alpha, a0, flags, *outs):
            at = lambda p, k: np.ctypeslib.as_array(C.cast(p, C.POINTER(real)), (k,)).copy()   # noqa: E731
            seen.update(stem=stem, f64=f64, M=M, n=n, flags=flags, kappa=at(kappa, n * M), gamma=at(gamma, 1), alpha=at(alpha, n),
                        a0=at(a0, 2 * M), n_outs=len(outs))
            return 0
        return call
    monkeypatch.setattr(nat, "_fn", fake_fn)
    return seen


def test_the_inputs_reach_the_float32_face_rounded_once(monkeypatch):
    """kappa, gamma, alpha and a0 arrive as float32 / complex64 buffers, each the one rounding of the float64 value, with the
    BCAST bits of the float64 wrapper; the call without dtype hands the float64 face the float64 values themselves."""
    kappa = np.array([[0.1, -1.0 / 3.0, 2.0 / 3.0, 1e-3], [1.0 / 7.0, 0.0, -1e-9, 3.0]])
    a0 = np.array([1.0 / 3.0 + 0.1j, 0.6 - 2.0j / 3.0, 1e-4j, 1.0 / 9.0])
    kw = dict(n_steps=2, z_max=1.0, save_every=1, gamma=0.0115, alpha=np.array([1.0 / 3.0, 0.0]), a0=a0)
    seen = _record(monkeypatch, C.c_float)
    nat.comb_host(kappa, dtype=np.float32, **kw)
    assert (seen["stem"], seen["f64"], seen["M"], seen["n"], seen["n_outs"]) == ("psa_rk4_comb", False, 4, 2, 6)
    assert np.array_equal(seen["kappa"], kappa.astype(np.float32).ravel()) and seen["gamma"][0] == np.float32(0.0115)
    assert np.array_equal(seen["alpha"], kw["alpha"].astype(np.float32))
    assert np.array_equal(seen["a0"], a0.astype(np.complex64).view(np.float32))
    flags32 = seen["flags"]
    seen = _record(monkeypatch, C.c_double)
    nat.comb_host(kappa, **kw)
    # the BCAST bits of the float64 wrapper; PSA_OPT_EXACT_STEP goes to the float64 face alone, as in sweep_host (both kernels
    # test after every step whatever it says)
    assert (seen["stem"], seen["f64"], seen["flags"]) == ("psa_rk4_comb", True, flags32 | nat.OPT_EXACT_STEP)
    assert flags32 == nat.BCAST_GAMMA | nat.BCAST_A0 | nat.OPT_CHECK_NAN
    assert np.array_equal(seen["kappa"], kappa.ravel()) and np.array_equal(seen["a0"], a0.view(np.float64))
    # through the driver the rounding is still the only one: kappa stays float64 until comb_host
    seen = _record(monkeypatch, C.c_float)
    sweep.rk4_sweep_comb(kappa, z_max=1.0, n_steps=2, save_every=1, gamma=0.0115, alpha=kw["alpha"], a0=a0, dtype=np.float32)
    assert np.array_equal(seen["kappa"], kappa.astype(np.float32).ravel())
    assert np.array_equal(seen["a0"], a0.astype(np.complex64).view(np.float32))


def test_the_gain_driver_passes_the_dtype_on(golden, monkeypatch):
    asked = _spy(monkeypatch)
    kw = _gain_kw(golden)
    out = scan_mismtach.scan_comb_gain(**kw)
    assert asked[-1] == ("psa_rk4_comb", True, False) and out["result"].a_end.dtype == np.complex128
    out = scan_mismtach.scan_comb_gain(dtype=np.float32, **kw)
    assert asked[-1] == ("psa_rk4_comb", False, False) and out["result"].a_end.dtype == np.complex64
    assert out["p_end"].dtype == np.float32 and out["gain"].shape == (2, 5)
    # kappa is formed in float64 on the host, in the gauge that pins both end lines to 0
    assert out["kappa"].dtype == np.float64 and out["kappa"][0] == 0.0 and abs(out["kappa"][-1]) <= 1e-15 * np.max(np.abs(out["kappa"]))


def test_the_unit_compiles_without_scratch_in_every_instantiation():
    """psa_rk4_comb_f32.hip under the Makefile's flags for the sweep units: M = 3..12 with and without the check, each with
    ScratchSize 0 (from M = 8 part of the state lives in the lane's LDS column, psa_rk4_comb_pk_kernel.inc.h)."""
    csrc = os.path.join(ROOT, "psa-simulation-ode-rk-mvp-dispersion_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile"), encoding="utf-8").read()
    sched = re.search(r"^SCHED\s*\?=\s*(.+)$", mk, re.M).group(1).split()
    align = re.search(r"^ALIGN\s*\?=\s*(.+)$", mk, re.M).group(1).split()
    # the unit stands beside its float64 sibling in the one list of sweep units, which OBJS, the flags and the encoding-alignment
    # rule all read; its header dependencies are the compiler's (tests/test_build_steps.py)
    assert "psa_rk4_comb.o psa_rk4_comb_f32.o" in re.search(r"^SWEEP\s*:=\s*(.+)$", mk, re.M).group(1)
    assert re.search(r"^OBJS\s*:=\s*\$\(SWEEP\)", mk, re.M) and re.search(r"^\$\(SWEEP\): HIPFLAGS \+= \$\(SCHED\) \$\(ALIGN\)$", mk, re.M)
    assert re.search(r"^\$\(SWEEP\): %\.o: %\.hip align_encodings\.py$", mk, re.M) and "-include $(OBJS:.o=.d)" in mk
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-c",
                          "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-Wall", "-Wno-unused-function", *sched, *align,
                          "-Rpass-analysis=kernel-resource-usage", os.path.join(csrc, "psa_rk4_comb_f32.hip"), "-o", os.devnull],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    names = re.findall(r"Function Name: (\S*rk4_sweep_comb_pk_kernel\S*)", out.stderr)
    scratch = re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stderr)
    assert len(set(names)) == 20 and len(scratch) == 20, out.stderr[-2000:]
    assert all(f"ILi{M}ELb{c}E" in " ".join(names) for M in range(3, 13) for c in (0, 1))
    assert [int(x) for x in scratch] == [0] * 20, list(zip(names, scratch))
