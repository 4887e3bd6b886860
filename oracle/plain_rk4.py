"""plain_rk4.py -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Python face of ``libpsa_plain_rk4.so`` (``psa_plain_rk4.c`` / ``psa_plain_rk4.inc.h``): ONE text of the plain classic RK4
of tests/truth_ld.py -- k1..k4 on the grid z_i = i h, cos / sin of the phase at every stage, nothing carried, nothing fused
-- compiled in three precisions:

* ``"ld"``   long double (x87 extended): the yardstick where the NumPy longdouble run (0.5 ms per step) cannot go;
             results come back as np.longdouble / np.clongdouble, never through float64;
* ``"f64"``  a plain float64 twin;
* ``"f32"``  state and every operation in float32 (the phase reduced in float64 before cosf / sinf), with the state update
             ``"plain"``, ``"kahan"`` (compensated per component), ``"base_offset"`` (base + offset, Fast2Sum fold every 16
             steps) or ``"base_offset_no_residue"`` (the fold's residue thrown away: a planted defect).

Models: ``"pairs"`` two pumps and K pairs (4 waves, 6 waves, the multi-channel model), ``"single_pump"``, ``"comb"``.
OpenMP over the points with the runtime's default thread count.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

MODELS = dict(pairs=0, single_pump=1, comb=2)
UPDATES = dict(plain=0, kahan=1, base_offset=2, base_offset_no_residue=3)
# precision -> (entry point, real dtype, complex dtype)
PRECISIONS = dict(ld=("psa_plain_rk4_ld", np.longdouble, np.clongdouble), f64=("psa_plain_rk4_f64", np.float64, np.complex128),
                  f32=("psa_plain_rk4_f32", np.float32, np.complex64))

_f64p = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")


def build(force: bool = False) -> str:
    so = os.path.join(_HERE, "libpsa_plain_rk4.so")
    srcs = [os.path.join(_HERE, f) for f in ("psa_plain_rk4.c", "psa_plain_rk4.inc.h")]
    if force or not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["make", "-C", _HERE, "-s", "-B", "libpsa_plain_rk4.so"])
    return so


def lib() -> C.CDLL:
    global _LIB
    if _LIB is None:
        assert np.finfo(np.longdouble).nmant >= 63 and np.dtype(np.longdouble).itemsize == C.sizeof(C.c_longdouble), \
            "np.longdouble is not the C long double of this build"
        L = C.CDLL(build())
        for name, _, _ in PRECISIONS.values():
            f = getattr(L, name)
            f.restype = C.c_int
            f.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double, C.c_int64, C.c_double, C.c_int64, C.c_int64, _f64p, _f64p, _f64p, _f64p,
                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _LIB = L
    return _LIB


def integrate(model, a0, rate, *, z_max, n, save_every, gamma, alpha, precision="ld", update="plain", want_rows=False,
              sideband_drift=0.0):
    """One sweep of N points.  rate (N,) or (N, C): dbeta per pair, kappa per line; a0 (NW,) or (N, NW); gamma / alpha a scalar
    or (N,).  The inputs are float64 values (float32-rounded ones for a float32 run: their conversion is then exact).
    sideband_drift (model "pairs", update "plain"): the planted defect of psa_plain_rk4.inc.h, every sideband scaled by
    1 + sideband_drift after every step.
    -> dict(a_end (N, NW), p_wave_end, p_wave_max (N, NW), rows (N, n // save_every + 1, NW) or None) in the precision's types."""
    name, real, cplx = PRECISIONS[precision]
    rate = np.ascontiguousarray(rate, dtype=np.float64)
    if rate.ndim == 1:
        rate = np.ascontiguousarray(rate[:, None])
    N = rate.shape[0]
    nw = np.shape(a0)[-1]
    a0 = np.ascontiguousarray(np.broadcast_to(np.asarray(a0, dtype=np.complex128), (N, nw)))
    gamma = np.ascontiguousarray(np.broadcast_to(np.asarray(gamma, dtype=np.float64), (N,)))
    alpha = np.ascontiguousarray(np.broadcast_to(np.asarray(alpha, dtype=np.float64), (N,)))
    assert rate.shape[1] == dict(pairs=(nw - 2) // 2, single_pump=1, comb=nw)[model], (model, rate.shape, nw)
    n, save_every = int(n), int(save_every)
    rows = np.empty((N, n // save_every + 1, nw), dtype=cplx) if want_rows else None
    a_end = np.empty((N, nw), dtype=cplx)
    p_end, p_max = np.empty((N, nw), dtype=real), np.empty((N, nw), dtype=real)
    rc = getattr(lib(), name)(MODELS[model], nw, UPDATES[update], float(sideband_drift), N, float(z_max), n, save_every, rate, gamma, alpha,
                              a0.view(np.float64).reshape(-1), None if rows is None else rows.ctypes.data, a_end.ctypes.data,
                              p_end.ctypes.data, p_max.ctypes.data)
    if rc != 0:
        raise ValueError(f"{name} rc={rc}")
    return dict(a_end=a_end, p_wave_end=p_end, p_wave_max=p_max, rows=rows)
