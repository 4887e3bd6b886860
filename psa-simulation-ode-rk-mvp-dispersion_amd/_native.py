"""ctypes binding of ``libpsa_hip.so`` (the C-ABI declared in ``include/psa_rk4.h``).

This is the ONLY compute path of the package: there is no CPU fallback.  If the
shared library is missing, or no gfx950 device is visible when a compute entry
point is called, a ``NativeUnavailableError`` / ``PsaNativeError`` is raised.

Two faces:

* ``sweep_host`` / ``yaman_rhs_host`` / ``gain_summary_host`` take NumPy arrays
  (host buffers, blocking) -- what the reference-shaped Python API uses;
* ``sweep_device`` takes raw device pointers + a hipStream_t handle (e.g. from
  torch tensors) -- what ``bench.py`` and the multi-GPU driver use.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
# PSA_HIP_LIB: developer hook to load an A/B build of the same library (tools/ab_build.sh); never a different backend
LIB_PATH = os.environ.get("PSA_HIP_LIB") or os.path.join(_PKG_DIR, "libpsa_hip.so")

# flags (mirror include/psa_rk4.h)
BCAST_GAMMA = 1 << 0
BCAST_ALPHA = 1 << 1
BCAST_A0 = 1 << 2
BCAST_TRANSFER = 1 << 3
OPT_CHECK_NAN = 1 << 8
OPT_EXACT_STEP = 1 << 9
OPT_LDS_STAGING = 1 << 10
OPT_BLOCK64 = 1 << 11
OPT_F32_SCALAR = 1 << 12
OPT_F32_PACKED = 1 << 13
OPT_LOSSLESS = 1 << 14
OPT_SPLIT_POINT = 1 << 15
OPT_ONE_LANE = 1 << 16
OPT_TRAJ_LD = 1 << 17
OPT_QUAD_POINT = 1 << 18
MAX_POINTS = 2**31 - 256          # PSA_MAX_POINTS: the most points one launch takes
MAX_PAIRS = 16                    # PSA_MAX_PAIRS: the most signal/idler pairs of the multi-channel sweep
MAX_LINES = 12                    # PSA_MAX_LINES: the most lines of the multi-line ("comb") sweep

# every symbol the header declares, with (restype, argtypes)
_P, _I, _L, _D, _I32, _U32 = C.c_void_p, C.c_int, C.c_int64, C.c_double, C.c_int32, C.c_uint32
_BOTH = ("f64", "f32")


def _family(stem, body, host=(), dev=(), host_types=_BOTH, dev_types=_BOTH, dev_first=False) -> dict:
    """The faces of one entry point: ``<stem>_<type>(device, *body, *host)`` and ``<stem>_<type>_dev(stream, *body, *dev)``,
    in the header's order (the host faces first unless ``dev_first``)."""
    hosts = {f"{stem}_{t}": (_I, [_I, *body, *host]) for t in host_types}
    devs = {f"{stem}_{t}_dev": (_I, [_P, *body, *dev]) for t in dev_types}
    return {**devs, **hosts} if dev_first else {**hosts, **devs}


# n_waves, N, n_steps, z_max, save_every, dbeta, dbeta2, gamma, alpha, a0, flags, a_end, p_end, p_max, first_bad, traj
_SWEEP = [_I, _L, _L, _D, _I32] + [_P] * 5 + [_U32] + [_P] * 5
# method, orders, n_orders, max_order, beta, n_beta, omega_ref, two_pi_c, atol, rtol
_MODEL = [_I, _P, _I, _I, _P, _I] + [_D] * 4
_GAIN = [_L, _P, _P, _D, _I] + [_P] * 4
_SIGS = {
    "psa_device_count": (_I, []),
    "psa_last_error": (C.c_char_p, []),
    "psa_version": (C.c_char_p, []),
    "psa_n_saved": (_L, [_L, _I32]),
    "psa_release_cache": (_I, []),
    "psa_traj_ld": (_L, [_L, _I32]),
    **_family("psa_rk4_sweep", _SWEEP, host=[_P]),                               # host: elapsed_ms
    **_family("psa_rk4_sweep_waves", _SWEEP, host=[_P] * 3, dev=[_P] * 2),       # [elapsed_ms,] p_wave_end, p_wave_max
    # n_waves, N, S, n_steps[S], seg_len[S], save_every, dbeta, dbeta2, gamma, alpha, a0, transfer, flags, a_end, p_end, p_max,
    # first_bad, traj; host: elapsed_ms, p_wave_end, p_wave_max; dev: p_wave_end, p_wave_max, workspace
    **_family("psa_rk4_chain", [_I, _L, _I, _P, _P, _I32] + [_P] * 6 + [_U32] + [_P] * 5, host=[_P] * 3, dev=[_P] * 3),
    "psa_rk4_chain_workspace_bytes": (_L, [_I, _L, _I32, _I]),
    # n_waves, N, z_max, rtol, atol, h_max, first_step, max_steps, n_out, dbeta, dbeta2, gamma, alpha, a0, flags, a_end, p_end,
    # p_max, status, z_end, n_accepted, n_rejected, traj; host: elapsed_ms
    **_family("psa_rk45_sweep", [_I, _L] + [_D] * 5 + [_L, _L] + [_P] * 5 + [_U32] + [_P] * 8, host=[_P],
              host_types=("f64",), dev_types=("f64",)),
    # n_pairs, N, n_steps, z_max, save_every, dbeta, gamma, alpha, a0, flags, a_end, p_wave_end, p_wave_max, first_bad; host: elapsed_ms
    **_family("psa_rk4_sweep_pairs", [_I, _L, _L, _D, _I32] + [_P] * 4 + [_U32] + [_P] * 4, host=[_P],
              host_types=("f64",), dev_types=("f64",)),
    # N, n_steps, z_max, save_every, dbeta, gamma, alpha, a0, flags, a_end, p_wave_end, p_wave_max, first_bad, traj; host: elapsed_ms
    **_family("psa_rk4_single_pump", [_L, _L, _D, _I32] + [_P] * 4 + [_U32] + [_P] * 5, host=[_P]),
    # n_lines, N, n_steps, z_max, save_every, kappa, gamma, alpha, a0, flags, a_end, p_wave_end, p_wave_max, first_bad, traj; host: elapsed_ms
    **_family("psa_rk4_comb", [_I, _L, _L, _D, _I32] + [_P] * 4 + [_U32] + [_P] * 5, host=[_P]),
    # N, S, n_steps[S], seg_len[S], save_every, dbeta, gamma, alpha, a0, transfer, flags, a_end, p_wave_end, p_wave_max, first_bad,
    # traj; host: elapsed_ms; dev: workspace
    **_family("psa_rk4_single_pump_chain", [_L, _I, _P, _P, _I32] + [_P] * 5 + [_U32] + [_P] * 5, host=[_P], dev=[_P],
              host_types=("f64",), dev_types=("f64",)),
    "psa_rk4_single_pump_chain_workspace_bytes": (_L, [_L]),
    # n_pairs, then the arguments of psa_rk4_single_pump_chain
    **_family("psa_rk4_pairs_chain", [_I, _L, _I, _P, _P, _I32] + [_P] * 5 + [_U32] + [_P] * 5, host=[_P], dev=[_P],
              host_types=("f64",), dev_types=("f64",)),
    "psa_rk4_pairs_chain_workspace_bytes": (_L, [_I, _L]),
    # n_lines, then the arguments of psa_rk4_single_pump_chain
    **_family("psa_rk4_comb_chain", [_I, _L, _I, _P, _P, _I32] + [_P] * 5 + [_U32] + [_P] * 5, host=[_P], dev=[_P],
              host_types=("f64",), dev_types=("f64",)),
    "psa_rk4_comb_chain_workspace_bytes": (_L, [_I, _L]),
    "psa_yaman_rhs_f64": (_I, [_I, _L] + [_P] * 9),
    # N, p_metric, first_bad, p0_sig, gain_db, gain, best_index, best_gain, n_finite; dev: workspace
    **_family("psa_gain_summary", _GAIN, dev=[_P], host_types=("f64",), dev_types=("f64",)),
    "psa_gain_summary_workspace_bytes": (_L, [_L]),
    **_family("psa_gain_summary", _GAIN, dev=[_P], host_types=("f32",), dev_types=("f32",)),
    # model, lambda1, axis2, n2, axis3, n3, first, n, out, valid
    **_family("psa_dbeta_grid", _MODEL + [_D, _P, _L, _P, _L, _L, _L, _P, _P], host_types=("f64",), dev_first=True),
    # orders, n_orders, beta, n_beta, omega_d, axis1, n1, axis2, n2, first, n, out1, out2
    **_family("psa_dbeta_pairs", [_P, _I, _P, _I, _D, _P, _L, _P, _L, _L, _L, _P, _P], host_types=("f64",),
              dev_first=True),
}
DBETA_SYMMETRIC_EVEN, DBETA_GENERAL_TAYLOR = 0, 1
DBETA_MAX_ORDER = 8
EXPORTED_SYMBOLS = tuple(_SIGS)


class NativeUnavailableError(RuntimeError):
    """libpsa_hip.so cannot be loaded (not built, or the HIP runtime is missing)."""


class PsaNativeError(RuntimeError):
    """A C-ABI call returned non-zero (argument error < 0, hipError_t > 0)."""

    def __init__(self, code: int, message: str):
        super().__init__(f"libpsa_hip rc={code}: {message}")
        self.code = code


_LIB: Optional[C.CDLL] = None


def _pin_hip_runtime() -> None:
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own ``libamdhip64.so`` with the same SONAME
    as /opt/rocm's; whichever is mapped first serves every later dlopen of that SONAME.  If torch is installed but
    not imported yet, map ITS copy now, so that a later ``import torch`` (bench.py, the multi-GPU driver) and this
    library share device pointers and streams whatever the import order.  PSA_HIP_RUNTIME=system skips this."""
    import sys
    if "torch" in sys.modules or os.environ.get("PSA_HIP_RUNTIME", "") == "system":
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.submodule_search_locations:
            return
        cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(cand):
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
    except Exception:
        pass  # fall through to the system runtime; a mismatch would surface as a loud HIP error, not a wrong result


def lib() -> C.CDLL:
    """Load the shared library once; raise loudly if it is not there."""
    global _LIB
    if _LIB is None:
        _pin_hip_runtime()
        if not os.path.exists(LIB_PATH):
            raise NativeUnavailableError(
                f"{LIB_PATH} not found: build it with `python __graft_entry__.py` "
                "(or `make -C psa-simulation-ode-rk-mvp-dispersion_amd/csrc`). There is no CPU fallback: "
                "the sweep only runs in the HIP library.")
        try:
            L = C.CDLL(LIB_PATH)
        except OSError as e:  # missing libamdhip64 etc.
            raise NativeUnavailableError(f"cannot load {LIB_PATH}: {e}") from e
        for name, (res, args) in _SIGS.items():
            fn = getattr(L, name)  # AttributeError if the build is stale
            fn.restype = res
            fn.argtypes = args
        _LIB = L
    return _LIB


def device_count() -> int:
    return int(lib().psa_device_count())


def version() -> str:
    return lib().psa_version().decode()


def traj_ld(n_points: int, dtype=np.float64) -> int:
    """Leading dimension of a device trajectory buffer launched with OPT_TRAJ_LD (psa_traj_ld)."""
    return int(lib().psa_traj_ld(int(n_points), int(np.dtype(dtype).itemsize)))


def release_cache() -> int:
    """Destroy the idle per-device call contexts (stream, events, scratch) the host-buffer entry points keep; -> how many."""
    return int(lib().psa_release_cache())


def _check(rc: int) -> None:
    if rc != 0:
        raise PsaNativeError(rc, lib().psa_last_error().decode(errors="replace"))


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _prep(x, dtype, n_points: int, name: str, spans=None):
    """A scalar or (N,) -> (contiguous 1-D array, is_broadcast)."""
    arr = np.ascontiguousarray(np.atleast_1d(np.asarray(x)), dtype=dtype)
    if arr.ndim != 1:
        raise ValueError(f"{name} must be a scalar or 1-D array")
    if arr.shape[0] == n_points and n_points != 1:
        return arr, False
    if arr.shape[0] == 1:
        return arr, True
    raise ValueError(f"{name} must have 1 or {n_points} entries, got {arr.shape[0]}")


def _prep_spans(x, dtype, n_points: int, name: str, spans: int):
    """(S,) or (S, N) of a chain -> (contiguous array, is_broadcast)."""
    arr = np.ascontiguousarray(np.asarray(x), dtype=dtype)
    if arr.shape == (spans,):
        return arr, True
    if arr.shape != (spans, n_points):
        raise ValueError(f"{name} must have shape ({spans},) or ({spans}, {n_points})")
    return arr, False


_FN: dict = {}    # (stem, f64, dev) -> bound C function: resolved once, one dictionary look-up per call afterwards


def _fn(stem: str, f64: bool = True, dev: bool = False):
    """The entry point ``<stem>_f64`` or (``f64`` false) ``<stem>_f32``, its ``_dev`` face on request."""
    try:
        return _FN[stem, f64, dev]
    except KeyError:
        fn = _FN[stem, f64, dev] = getattr(lib(), f"{stem}_{'f64' if f64 else 'f32'}{'_dev' if dev else ''}")
        return fn


def _is_f64(dtype) -> bool:
    """A ``_dev`` wrapper's dtype argument: float64 selects the _f64 entry point, anything else the _f32 one."""
    return np.dtype(dtype) == np.float64


_F64, _F32 = np.dtype(np.float64), np.dtype(np.float32)


def _dtypes(dtype):
    """-> (real dtype, its complex dtype, is it float64) of a host wrapper's dtype argument: float64 or float32."""
    dtype = np.dtype(dtype)
    if dtype == _F64:
        return dtype, np.complex128, True
    if dtype == _F32:
        return dtype, np.complex64, False
    raise ValueError("dtype must be float64 or float32")


def _check_flags(check_nan: bool, exact_step: Optional[bool], f64: bool = True) -> int:
    """OPT_CHECK_NAN, and with it OPT_EXACT_STEP where asked for or (exact_step None) where it is free: in float64."""
    if not check_nan:
        return 0
    return OPT_CHECK_NAN | (OPT_EXACT_STEP if exact_step or (exact_step is None and f64) else 0)


def _point_inputs(N: int, dtype, cdt, flags: int, gamma, alpha, a0, widths, dbeta=None, dbeta2=None, spans=None):
    """The per-point inputs of a host wrapper -> (flags with the BCAST bits, gamma, alpha, a0, dbeta2).

    a0 (n_waves,) or (N, n_waves) complex with n_waves in ``widths``; gamma / alpha a scalar or (N,) -- for a chain of
    ``spans`` spans (S,) or (S, N); dbeta2 shaped as ``dbeta`` for 6 waves and absent for 4 (a family without dbeta2 passes
    no ``dbeta``).  One value where N are possible sets the argument's BCAST bit."""
    a0 = np.ascontiguousarray(np.asarray(a0), dtype=cdt)
    if a0.ndim == 1:
        a0 = a0[None, :]
    if a0.ndim != 2 or a0.shape[1] not in widths:
        raise ValueError(f"a0 must have shape (n_waves,) or ({N}, n_waves) with n_waves in {tuple(widths)}, got {a0.shape}")
    if a0.shape[0] == 1:
        flags |= BCAST_A0
    elif a0.shape[0] != N:
        raise ValueError(f"a0 must have 1 or {N} rows, got {a0.shape[0]}")
    prep = _prep if spans is None else _prep_spans
    gamma, bcast = prep(gamma, dtype, N, "gamma", spans)
    if bcast:
        flags |= BCAST_GAMMA
    alpha, bcast = prep(alpha, dtype, N, "alpha", spans)
    if bcast:
        flags |= BCAST_ALPHA
    d2 = None
    if dbeta is not None and a0.shape[1] == 6:
        if dbeta2 is None:
            raise ValueError("n_waves == 6 needs dbeta2")
        d2 = np.ascontiguousarray(np.atleast_1d(np.asarray(dbeta2)), dtype=dtype)
        if d2.shape != dbeta.shape:
            raise ValueError("dbeta2 must match dbeta")
    elif dbeta2 is not None:
        raise ValueError("dbeta2 is only meaningful for 6 waves")
    return flags, gamma, alpha, a0, d2


def sweep_host(dbeta, *, n_steps: int, z_max: float, save_every: int, gamma, alpha, a0, dbeta2=None,
               check_nan: bool = True, exact_step: Optional[bool] = None, want_traj: bool = False, dtype=np.float64,
               device: int = 0, extra_flags: int = 0, wave_summary: bool = False) -> dict:
    """Run N independent RK4 propagations on the GPU (host buffers in, host buffers out).

    wave_summary: also return p_wave_end / p_wave_max (N, n_waves), the end and maximum power of every wave
    (psa_rk4_sweep_waves_*; no trajectory with it).  Without it both are None.

    exact_step: None = exact first_bad_step in float64 (free there: block test + replay of a failing block) and the
    per-save-block index in float32; True / False force either.

    dbeta (N,); gamma/alpha scalar or (N,); a0 (n_waves,) or (N, n_waves) complex.
    Returns a_end (N, n_waves) complex, p_end, p_max (N,), first_bad_step (N,) int64,
    traj (N, n_saved, n_waves) complex or None, elapsed_ms (kernel only).
    """
    dtype, cdt, f64 = _dtypes(dtype)
    dbeta = np.ascontiguousarray(np.atleast_1d(np.asarray(dbeta)), dtype=dtype)
    if dbeta.ndim != 1:
        raise ValueError("dbeta must be 1-D")
    N = int(dbeta.shape[0])
    flags, gamma, alpha, a0, d2 = _point_inputs(N, dtype, cdt, int(extra_flags), gamma, alpha, a0, (4, 6), dbeta, dbeta2)
    flags |= _check_flags(check_nan, exact_step, f64)
    nw = int(a0.shape[1])
    n_saved = int(n_steps) // int(save_every) + 1 if save_every > 0 else 0
    a_end = np.empty((N, nw), dtype=cdt)
    p_end = np.empty(N, dtype=dtype)
    p_max = np.empty(N, dtype=dtype)
    bad = np.empty(N, dtype=np.int64)
    traj = np.empty((N, n_saved, nw), dtype=cdt) if want_traj else None
    w_end = np.empty((N, nw), dtype=dtype) if wave_summary else None
    w_max = np.empty((N, nw), dtype=dtype) if wave_summary else None
    ms = C.c_double(0.0)
    _check(_fn("psa_rk4_sweep_waves" if wave_summary else "psa_rk4_sweep", f64)(
        int(device), nw, N, int(n_steps), float(z_max), int(save_every), _ptr(dbeta), _ptr(d2), _ptr(gamma), _ptr(alpha),
        _ptr(a0), flags, _ptr(a_end), _ptr(p_end), _ptr(p_max), _ptr(bad), _ptr(traj), C.cast(C.byref(ms), _P),
        *((_ptr(w_end), _ptr(w_max)) if wave_summary else ())))
    return dict(a_end=a_end, p_end=p_end, p_max=p_max, first_bad_step=bad, traj=traj, elapsed_ms=ms.value,
                p_wave_end=w_end, p_wave_max=w_max)


def sweep_device(*, stream: int, n_waves: int, n_points: int, n_steps: int, z_max: float, save_every: int,
                 d_dbeta: int, d_dbeta2: int, d_gamma: int, d_alpha: int, d_a0_soa: int, flags: int,
                 d_a_end_soa: int, d_p_end: int, d_p_max: int, d_first_bad: int, d_traj_soa: int = 0,
                 dtype=np.float64) -> None:
    """Asynchronous launch on device pointers (ints), SoA layout -- see psa_rk4_sweep_f64_dev."""
    _check(_fn("psa_rk4_sweep", _is_f64(dtype), dev=True)(
        stream or None, int(n_waves), int(n_points), int(n_steps), float(z_max), int(save_every),
        d_dbeta or None, d_dbeta2 or None, d_gamma or None, d_alpha or None, d_a0_soa or None, int(flags),
        d_a_end_soa or None, d_p_end or None, d_p_max or None, d_first_bad or None, d_traj_soa or None))


def sweep_waves_device(*, stream: int, n_waves: int, n_points: int, n_steps: int, z_max: float, save_every: int,
                       d_dbeta: int, d_dbeta2: int, d_gamma: int, d_alpha: int, d_a0_soa: int, flags: int,
                       d_a_end_soa: int, d_p_end: int, d_p_max: int, d_first_bad: int, d_p_wave_end_soa: int,
                       d_p_wave_max_soa: int, d_traj_soa: int = 0, dtype=np.float64) -> None:
    """sweep_device with the per-wave summary ([n_waves][N] device buffers) -- see psa_rk4_sweep_waves_f64_dev."""
    _check(_fn("psa_rk4_sweep_waves", _is_f64(dtype), dev=True)(
        stream or None, int(n_waves), int(n_points), int(n_steps), float(z_max), int(save_every),
        d_dbeta or None, d_dbeta2 or None, d_gamma or None, d_alpha or None, d_a0_soa or None, int(flags),
        d_a_end_soa or None, d_p_end or None, d_p_max or None, d_first_bad or None, d_traj_soa or None,
        d_p_wave_end_soa or None, d_p_wave_max_soa or None))


def _wave_host(stem: str, dtypes, mismatch: np.ndarray, head: tuple, nw: int, check: int, rows: bool, n_steps, z_max,
               save_every, gamma, alpha, a0, want_traj: bool, device: int, extra_flags: int) -> dict:
    """The host-buffer sweep of a wave-summary family (multi-channel, single-pump, multi-line): ``<stem>_f64`` / ``_f32`` with
    ``head`` (the family's count, or nothing) in front of N.  ``dtypes``: _dtypes' answer; ``mismatch``: the family's checked
    and converted array, N its first axis; ``nw``: the columns of a0; ``check``: _check_flags' answer; ``rows``: the entry point
    takes a trajectory, and the result has the key traj."""
    dtype, cdt, f64 = dtypes
    N = int(mismatch.shape[0])
    flags, gamma, alpha, a0, _ = _point_inputs(N, dtype, cdt, int(extra_flags), gamma, alpha, a0, (nw,))
    a_end = np.empty((N, nw), dtype=cdt)
    w_end = np.empty((N, nw), dtype=dtype)
    w_max = np.empty((N, nw), dtype=dtype)
    bad = np.empty(N, dtype=np.int64)
    ms = C.c_double(0.0)
    out = dict(a_end=a_end, p_wave_end=w_end, p_wave_max=w_max, first_bad_step=bad)
    tail = ()
    if rows:
        n_saved = int(n_steps) // int(save_every) + 1 if save_every > 0 else 0
        out["traj"] = np.empty((N, n_saved, nw), dtype=cdt) if want_traj else None
        tail = (_ptr(out["traj"]),)
    _check(_fn(stem, f64)(int(device), *head, N, int(n_steps), float(z_max), int(save_every), _ptr(mismatch), _ptr(gamma),
                          _ptr(alpha), _ptr(a0), flags | check, _ptr(a_end), _ptr(w_end), _ptr(w_max), _ptr(bad), *tail,
                          C.cast(C.byref(ms), _P)))
    out["elapsed_ms"] = ms.value
    return out


def _wave_device(stem: str, f64: bool, stream: int, head: tuple, inputs: tuple, flags: int, outputs: tuple) -> None:
    """``<stem>_*_dev``: ``head`` ([the family's count,] n_points, n_steps, z_max, save_every) as the caller converted it, then
    the device pointers (ints, 0 for NULL) with the flags between the inputs and the outputs."""
    _check(_fn(stem, f64, dev=True)(stream or None, *head, *(p or None for p in inputs), int(flags), *(p or None for p in outputs)))


def sweep_pairs_host(dbeta, *, n_steps: int, z_max: float, save_every: int, gamma, alpha, a0, check_nan: bool = True,
                     exact_step: Optional[bool] = None, device: int = 0, extra_flags: int = 0) -> dict:
    """N independent propagations of two pumps and K signal/idler pairs on the GPU (psa_rk4_sweep_pairs_f64; host buffers
    in and out, float64).  The channels couple through pump depletion and SPM/XPM; signal-signal FWM is not modelled
    here (on a uniform frequency grid, comb_host models every product).

    dbeta (N, K) with 1 <= K <= 16; gamma / alpha scalar or (N,); a0 (NW,) or (N, NW) complex, NW = 2 + 2K, waves
    [p1, p2, s_1, i_1, ..., s_K, i_K].  exact_step None or True: the exact first_bad_step; False: the save block's last step.
    Returns a_end (N, NW) complex, p_wave_end, p_wave_max (N, NW), first_bad_step (N,) int64, elapsed_ms (kernel only)."""
    dbeta = np.ascontiguousarray(np.asarray(dbeta), dtype=np.float64)
    if dbeta.ndim != 2 or not 1 <= dbeta.shape[1] <= MAX_PAIRS:
        raise ValueError(f"dbeta must have shape (N, K) with 1 <= K <= {MAX_PAIRS}, got {dbeta.shape}")
    K = int(dbeta.shape[1])
    return _wave_host("psa_rk4_sweep_pairs", (np.float64, np.complex128, True), dbeta, (K,), 2 + 2 * K,
                      _check_flags(check_nan, exact_step), False, n_steps, z_max, save_every, gamma, alpha, a0, False, device, extra_flags)


def sweep_pairs_device(*, stream: int, n_pairs: int, n_points: int, n_steps: int, z_max: float, save_every: int,
                       d_dbeta_soa: int, d_gamma: int, d_alpha: int, d_a0_soa: int, flags: int, d_a_end_soa: int,
                       d_p_wave_end_soa: int, d_p_wave_max_soa: int, d_first_bad: int) -> None:
    """Asynchronous multi-channel launch on device pointers (ints), SoA layout -- see psa_rk4_sweep_pairs_f64_dev."""
    _wave_device("psa_rk4_sweep_pairs", True, stream, (int(n_pairs), int(n_points), int(n_steps), float(z_max), int(save_every)),
                 (d_dbeta_soa, d_gamma, d_alpha, d_a0_soa), flags, (d_a_end_soa, d_p_wave_end_soa, d_p_wave_max_soa, d_first_bad))


def single_pump_host(dbeta, *, n_steps: int, z_max: float, save_every: int, gamma, alpha, a0, check_nan: bool = True,
                     exact_step: Optional[bool] = None, want_traj: bool = False, device: int = 0, extra_flags: int = 0,
                     dtype=np.float64) -> dict:
    """N independent propagations of the single-pump three-wave model on the GPU (psa_rk4_single_pump_f64 or, with
    ``dtype=np.float32``, psa_rk4_single_pump_f32; host buffers in and out): one pump, a signal and an idler at 2 w_p - w_s,
    waves [p, s, i].  Inputs are converted to ``dtype`` and outputs come back in it, as in sweep_host.

    dbeta (N,); gamma / alpha scalar or (N,); a0 (3,) or (N, 3) complex.  exact_step None or True: the exact first_bad_step
    (both precisions: the float32 kernel tests after every step); False: the save block's last step.
    Returns a_end (N, 3) complex, p_wave_end, p_wave_max (N, 3), first_bad_step (N,) int64, traj (N, n_saved, 3) complex or
    None, elapsed_ms (kernel only)."""
    dtypes = _dtypes(dtype)
    dbeta = np.ascontiguousarray(np.atleast_1d(np.asarray(dbeta)), dtype=dtypes[0])
    if dbeta.ndim != 1:
        raise ValueError("dbeta must be 1-D")
    return _wave_host("psa_rk4_single_pump", dtypes, dbeta, (), 3, _check_flags(check_nan, exact_step), True, n_steps, z_max,
                      save_every, gamma, alpha, a0, want_traj, device, extra_flags)


def single_pump_device(*, stream: int, n_points: int, n_steps: int, z_max: float, save_every: int, d_dbeta: int,
                       d_gamma: int, d_alpha: int, d_a0_soa: int, flags: int, d_a_end_soa: int, d_p_wave_end_soa: int,
                       d_p_wave_max_soa: int, d_first_bad: int, d_traj_soa: int = 0, dtype=np.float64) -> None:
    """Asynchronous single-pump launch on device pointers (ints), SoA layout -- see psa_rk4_single_pump_f64_dev; ``dtype``
    float32 is psa_rk4_single_pump_f32_dev on float buffers."""
    _wave_device("psa_rk4_single_pump", _dtypes(dtype)[2], stream, (int(n_points), int(n_steps), float(z_max), int(save_every)),
                 (d_dbeta, d_gamma, d_alpha, d_a0_soa), flags,
                 (d_a_end_soa, d_p_wave_end_soa, d_p_wave_max_soa, d_first_bad, d_traj_soa))


def comb_host(kappa, *, n_steps: int, z_max: float, save_every: int, gamma, alpha, a0, check_nan: bool = True,
              want_traj: bool = False, device: int = 0, extra_flags: int = 0, dtype=np.float64) -> dict:
    """N independent propagations of the multi-line ("comb") model on the GPU (psa_rk4_comb_f64 or, with ``dtype=np.float32``,
    psa_rk4_comb_f32; host buffers in and out): M equally spaced lines, ascending in frequency, with every FWM product among
    them that falls on the grid.  Inputs are converted to ``dtype`` once and outputs come back in it, as in single_pump_host.

    kappa (N, M) with 3 <= M <= 12, the lines' propagation constants in any gauge; gamma / alpha scalar or (N,); a0 (M,) or
    (N, M) complex.  With check_nan first_bad_step is the exact step index (the point is tested after every step).
    Returns a_end (N, M) complex, p_wave_end, p_wave_max (N, M), first_bad_step (N,) int64, traj (N, n_saved, M) complex or
    None, elapsed_ms (kernel only)."""
    dtypes = _dtypes(dtype)
    kappa = np.ascontiguousarray(np.asarray(kappa), dtype=dtypes[0])
    if kappa.ndim != 2 or not 3 <= kappa.shape[1] <= MAX_LINES:
        raise ValueError(f"kappa must have shape (N, M) with 3 <= M <= {MAX_LINES}, got {kappa.shape}")
    M = int(kappa.shape[1])
    # float32 goes without PSA_OPT_EXACT_STEP: the kernel tests after every step anyway
    return _wave_host("psa_rk4_comb", dtypes, kappa, (M,), M, _check_flags(check_nan, None, dtypes[2]), True, n_steps, z_max,
                      save_every, gamma, alpha, a0, want_traj, device, extra_flags)


def comb_device(*, stream: int, n_lines: int, n_points: int, n_steps: int, z_max: float, save_every: int, d_kappa_soa: int,
                d_gamma: int, d_alpha: int, d_a0_soa: int, flags: int, d_a_end_soa: int, d_p_wave_end_soa: int,
                d_p_wave_max_soa: int, d_first_bad: int, d_traj_soa: int = 0, dtype=np.float64) -> None:
    """Asynchronous multi-line launch on device pointers (ints), SoA layout -- see psa_rk4_comb_f64_dev; ``dtype`` float32 is
    psa_rk4_comb_f32_dev on float buffers."""
    _wave_device("psa_rk4_comb", _dtypes(dtype)[2], stream, (int(n_lines), int(n_points), int(n_steps), float(z_max), int(save_every)),
                 (d_kappa_soa, d_gamma, d_alpha, d_a0_soa), flags,
                 (d_a_end_soa, d_p_wave_end_soa, d_p_wave_max_soa, d_first_bad, d_traj_soa))


def _chain_host(stem: str, widths, sweep_family: bool, dbeta, *, n_steps, seg_len, save_every: int, gamma, alpha, a0,
                transfers, dbeta2, check_nan: bool, exact_step: Optional[bool], want_traj: bool, dtype, device: int,
                wave_summary: bool, extra_flags: int, pairs: bool = False, lines: bool = False) -> dict:
    """The host-buffer chain of a family: ``<stem>_f64`` / ``_f32`` on a0 of a width in ``widths``.  ``sweep_family``:
    the 4/6-wave entry points, which take n_waves and dbeta2, have p_end / p_max and put the per-wave summary last.
    ``pairs``: the multi-channel entry point, whose dbeta is (S, N, K) and which takes K in front; K fixes the width.
    ``lines``: the multi-line entry point, whose dbeta is (S, N, M), the lines' propagation constants, with M in front."""
    dtype, cdt, f64 = _dtypes(dtype)
    dbeta = np.ascontiguousarray(np.asarray(dbeta), dtype=dtype)
    if lines:
        if dbeta.ndim != 3 or dbeta.shape[0] < 1 or not 3 <= dbeta.shape[2] <= MAX_LINES:
            raise ValueError(f"kappa must have shape (S, N, M) with 3 <= M <= {MAX_LINES}, got {dbeta.shape}")
        widths = (int(dbeta.shape[2]),)
    elif pairs:
        if dbeta.ndim != 3 or dbeta.shape[0] < 1 or not 1 <= dbeta.shape[2] <= MAX_PAIRS:
            raise ValueError(f"dbeta must have shape (S, N, K) with 1 <= K <= {MAX_PAIRS}, got {dbeta.shape}")
        widths = (2 + 2 * int(dbeta.shape[2]),)
    elif dbeta.ndim != 2 or dbeta.shape[0] < 1:
        raise ValueError("dbeta must have shape (S, N)")
    S, N = (int(x) for x in dbeta.shape[:2])
    steps = np.ascontiguousarray(np.asarray(n_steps), dtype=np.int64)
    lens = np.ascontiguousarray(np.asarray(seg_len), dtype=np.float64)
    if steps.shape != (S,) or lens.shape != (S,):
        raise ValueError(f"n_steps and seg_len must have shape ({S},)")
    flags, gamma, alpha, a0, d2 = _point_inputs(N, dtype, cdt, int(extra_flags), gamma, alpha, a0, widths,
                                                dbeta if sweep_family else None, dbeta2, S)
    flags |= _check_flags(check_nan, exact_step, f64)
    nw = int(a0.shape[1])
    tr = None
    if transfers is not None and S > 1:
        tr = np.ascontiguousarray(np.asarray(transfers), dtype=cdt)
        if tr.shape == (S - 1, nw):
            flags |= BCAST_TRANSFER
        elif tr.shape != (S - 1, N, nw):
            raise ValueError(f"transfers must have shape ({S - 1}, {nw}) or ({S - 1}, {N}, {nw})")
    n_rows = int(np.sum(steps // save_every + 1)) if save_every > 0 else 0
    out = dict(a_end=np.empty((N, nw), dtype=cdt))
    if sweep_family:
        out.update(p_end=np.empty(N, dtype=dtype), p_max=np.empty(N, dtype=dtype))
    bad = np.empty(N, dtype=np.int64)
    traj = np.empty((N, n_rows, nw), dtype=cdt) if want_traj else None
    w_end = np.empty((N, nw), dtype=dtype) if wave_summary else None
    w_max = np.empty((N, nw), dtype=dtype) if wave_summary else None
    ms = C.c_double(0.0)
    grid = (N, S, _ptr(steps), _ptr(lens), int(save_every), _ptr(dbeta))
    point = (_ptr(gamma), _ptr(alpha), _ptr(a0), _ptr(tr), flags, _ptr(out["a_end"]))
    run = (_ptr(bad), _ptr(traj), C.cast(C.byref(ms), _P))
    if sweep_family:
        _check(_fn(stem, f64)(int(device), nw, *grid, _ptr(d2), *point, _ptr(out["p_end"]), _ptr(out["p_max"]), *run,
                              _ptr(w_end), _ptr(w_max)))
        return dict(out, first_bad_step=bad, traj=traj, elapsed_ms=ms.value, p_wave_end=w_end, p_wave_max=w_max)
    _check(_fn(stem, f64)(int(device), *((int(dbeta.shape[2]),) if pairs or lines else ()), *grid, *point, _ptr(w_end), _ptr(w_max), *run))
    return dict(out, p_wave_end=w_end, p_wave_max=w_max, first_bad_step=bad, traj=traj, elapsed_ms=ms.value)


def _chain_device(stem: str, f64: bool, stream: int, head: tuple, n_steps, seg_len, tail: tuple) -> None:
    """``<stem>_*_dev``: ``head`` (n_waves, n_points), the span count and the two host arrays, then ``tail`` as it is."""
    steps = np.ascontiguousarray(np.asarray(n_steps), dtype=np.int64)
    lens = np.ascontiguousarray(np.asarray(seg_len), dtype=np.float64)
    if steps.ndim != 1 or steps.shape != lens.shape:
        raise ValueError("n_steps and seg_len must be 1-D of equal length")
    _check(_fn(stem, f64, dev=True)(stream or None, *head, int(steps.shape[0]), _ptr(steps), _ptr(lens), *tail))


def single_pump_chain_host(dbeta, *, n_steps, seg_len, save_every: int, gamma, alpha, a0, transfers=None,
                           check_nan: bool = True, exact_step: Optional[bool] = None, want_traj: bool = False,
                           device: int = 0, extra_flags: int = 0) -> dict:
    """A chain of S single-pump spans on the GPU (psa_rk4_single_pump_chain_f64; host buffers in and out, float64).

    dbeta (S, N); n_steps, seg_len (S,); gamma / alpha (S,) broadcast or (S, N); a0 (3,) or (N, 3) complex; transfers None,
    (S-1, 3) broadcast or (S-1, N, 3) complex.  Returns the keys of single_pump_host; traj is (N, n_saved_total, 3)."""
    return _chain_host("psa_rk4_single_pump_chain", (3,), False, dbeta, n_steps=n_steps, seg_len=seg_len, save_every=save_every,
                       gamma=gamma, alpha=alpha, a0=a0, transfers=transfers, dbeta2=None, check_nan=check_nan,
                       exact_step=exact_step, want_traj=want_traj, dtype=np.float64, device=device, wave_summary=True,
                       extra_flags=extra_flags)


def single_pump_chain_workspace_bytes(n_points: int) -> int:
    """Device scratch a single-pump chain of more than one span needs (psa_rk4_single_pump_chain_workspace_bytes)."""
    return int(lib().psa_rk4_single_pump_chain_workspace_bytes(int(n_points)))


def single_pump_chain_device(*, stream: int, n_points: int, n_steps, seg_len, save_every: int, d_dbeta: int, d_gamma: int,
                             d_alpha: int, d_a0_soa: int, d_transfer_soa: int, flags: int, d_a_end_soa: int,
                             d_p_wave_end_soa: int, d_p_wave_max_soa: int, d_first_bad: int, d_traj_soa: int = 0,
                             d_workspace: int = 0) -> None:
    """psa_rk4_single_pump_chain_f64_dev on device pointers (ints); n_steps / seg_len are host sequences of length S."""
    _chain_device("psa_rk4_single_pump_chain", True, stream, (int(n_points),), n_steps, seg_len, (
        int(save_every), d_dbeta or None, d_gamma or None, d_alpha or None, d_a0_soa or None, d_transfer_soa or None, int(flags),
        d_a_end_soa or None, d_p_wave_end_soa or None, d_p_wave_max_soa or None, d_first_bad or None, d_traj_soa or None,
        d_workspace or None))


def pairs_chain_host(dbeta, *, n_steps, seg_len, save_every: int, gamma, alpha, a0, transfers=None, check_nan: bool = True,
                     exact_step: Optional[bool] = None, want_traj: bool = False, device: int = 0, extra_flags: int = 0) -> dict:
    """A chain of S multi-channel spans on the GPU (psa_rk4_pairs_chain_f64; host buffers in and out, float64): two pumps
    and K signal/idler pairs, waves [p1, p2, s_1, i_1, ..., s_K, i_K], NW = 2 + 2K.

    dbeta (S, N, K) with 1 <= K <= 16; n_steps, seg_len (S,); gamma / alpha (S,) broadcast or (S, N); a0 (NW,) or (N, NW)
    complex; transfers None, (S-1, NW) broadcast or (S-1, N, NW) complex.  One span with want_traj is the multi-channel
    sweep's trajectory form.  Returns the keys of sweep_pairs_host and traj (N, n_saved_total, NW) or None."""
    return _chain_host("psa_rk4_pairs_chain", None, False, dbeta, n_steps=n_steps, seg_len=seg_len, save_every=save_every,
                       gamma=gamma, alpha=alpha, a0=a0, transfers=transfers, dbeta2=None, check_nan=check_nan,
                       exact_step=exact_step, want_traj=want_traj, dtype=np.float64, device=device, wave_summary=True,
                       extra_flags=extra_flags, pairs=True)


def pairs_chain_workspace_bytes(n_pairs: int, n_points: int) -> int:
    """Device scratch a multi-channel chain of more than one span needs (psa_rk4_pairs_chain_workspace_bytes)."""
    return int(lib().psa_rk4_pairs_chain_workspace_bytes(int(n_pairs), int(n_points)))


def pairs_chain_device(*, stream: int, n_pairs: int, n_points: int, n_steps, seg_len, save_every: int, d_dbeta_soa: int,
                       d_gamma: int, d_alpha: int, d_a0_soa: int, d_transfer_soa: int, flags: int, d_a_end_soa: int,
                       d_p_wave_end_soa: int, d_p_wave_max_soa: int, d_first_bad: int, d_traj_soa: int = 0,
                       d_workspace: int = 0) -> None:
    """psa_rk4_pairs_chain_f64_dev on device pointers (ints); n_steps / seg_len are host sequences of length S."""
    _chain_device("psa_rk4_pairs_chain", True, stream, (int(n_pairs), int(n_points)), n_steps, seg_len, (
        int(save_every), d_dbeta_soa or None, d_gamma or None, d_alpha or None, d_a0_soa or None, d_transfer_soa or None,
        int(flags), d_a_end_soa or None, d_p_wave_end_soa or None, d_p_wave_max_soa or None, d_first_bad or None,
        d_traj_soa or None, d_workspace or None))


def comb_chain_host(dbeta, *, n_steps, seg_len, save_every: int, gamma, alpha, a0, transfers=None, check_nan: bool = True,
                    exact_step: Optional[bool] = None, want_traj: bool = False, device: int = 0, extra_flags: int = 0) -> dict:
    """A chain of S multi-line ("comb") spans on the GPU (psa_rk4_comb_chain_f64; host buffers in and out, float64): M equally
    spaced lines with every FWM product among them, every line's phase accumulated across the spans.

    dbeta (S, N, M) with 3 <= M <= 12: the lines' propagation constants kappa of every span, under the name every chain
    wrapper gives its per-span array; n_steps, seg_len (S,); gamma / alpha (S,) broadcast or (S, N); a0 (M,) or (N, M) complex;
    transfers None, (S-1, M) broadcast or (S-1, N, M) complex.  Returns the keys of comb_host; traj is (N, n_saved_total, M)."""
    return _chain_host("psa_rk4_comb_chain", None, False, dbeta, n_steps=n_steps, seg_len=seg_len, save_every=save_every,
                       gamma=gamma, alpha=alpha, a0=a0, transfers=transfers, dbeta2=None, check_nan=check_nan,
                       exact_step=exact_step, want_traj=want_traj, dtype=np.float64, device=device, wave_summary=True,
                       extra_flags=extra_flags, lines=True)


def comb_chain_workspace_bytes(n_lines: int, n_points: int) -> int:
    """Device scratch a multi-line chain of more than one span needs (psa_rk4_comb_chain_workspace_bytes)."""
    return int(lib().psa_rk4_comb_chain_workspace_bytes(int(n_lines), int(n_points)))


def comb_chain_device(*, stream: int, n_lines: int, n_points: int, n_steps, seg_len, save_every: int, d_kappa_soa: int,
                      d_gamma: int, d_alpha: int, d_a0_soa: int, d_transfer_soa: int, flags: int, d_a_end_soa: int,
                      d_p_wave_end_soa: int, d_p_wave_max_soa: int, d_first_bad: int, d_traj_soa: int = 0,
                      d_workspace: int = 0) -> None:
    """psa_rk4_comb_chain_f64_dev on device pointers (ints); n_steps / seg_len are host sequences of length S."""
    _chain_device("psa_rk4_comb_chain", True, stream, (int(n_lines), int(n_points)), n_steps, seg_len, (
        int(save_every), d_kappa_soa or None, d_gamma or None, d_alpha or None, d_a0_soa or None, d_transfer_soa or None,
        int(flags), d_a_end_soa or None, d_p_wave_end_soa or None, d_p_wave_max_soa or None, d_first_bad or None,
        d_traj_soa or None, d_workspace or None))


def chain_host(dbeta, *, n_steps, seg_len, save_every: int, gamma, alpha, a0, transfers=None, dbeta2=None,
               check_nan: bool = True, exact_step: Optional[bool] = None, want_traj: bool = False, dtype=np.float64,
               device: int = 0, wave_summary: bool = False, extra_flags: int = 0) -> dict:
    """A chain of S fibre spans on the GPU (psa_rk4_chain_*; host buffers in and out).

    dbeta (S, N) [and dbeta2 (S, N) for 6 waves]; n_steps, seg_len (S,); gamma / alpha (S,) broadcast or (S, N);
    a0 (n_waves,) or (N, n_waves) complex; transfers None, (S-1, n_waves) broadcast or (S-1, N, n_waves) complex.
    Returns the keys of sweep_host; traj is (N, n_saved_total, n_waves).
    """
    return _chain_host("psa_rk4_chain", (4, 6), True, dbeta, n_steps=n_steps, seg_len=seg_len, save_every=save_every,
                       gamma=gamma, alpha=alpha, a0=a0, transfers=transfers, dbeta2=dbeta2, check_nan=check_nan,
                       exact_step=exact_step, want_traj=want_traj, dtype=dtype, device=device, wave_summary=wave_summary,
                       extra_flags=extra_flags)


def chain_workspace_bytes(n_waves: int, n_points: int, dtype=np.float64, wave_summary: bool = False) -> int:
    """Device scratch a chain of more than one span needs (psa_rk4_chain_workspace_bytes)."""
    return int(lib().psa_rk4_chain_workspace_bytes(int(n_waves), int(n_points), int(np.dtype(dtype).itemsize),
                                                   int(bool(wave_summary))))


def chain_device(*, stream: int, n_waves: int, n_points: int, n_steps, seg_len, save_every: int, d_dbeta: int,
                 d_dbeta2: int, d_gamma: int, d_alpha: int, d_a0_soa: int, d_transfer_soa: int, flags: int,
                 d_a_end_soa: int, d_p_end: int, d_p_max: int, d_first_bad: int, d_traj_soa: int = 0,
                 d_p_wave_end: int = 0, d_p_wave_max: int = 0, d_workspace: int = 0, dtype=np.float64) -> None:
    """psa_rk4_chain_*_dev on device pointers (ints); n_steps / seg_len are host sequences of length S."""
    _chain_device("psa_rk4_chain", _is_f64(dtype), stream, (int(n_waves), int(n_points)), n_steps, seg_len, (
        int(save_every), d_dbeta or None, d_dbeta2 or None, d_gamma or None, d_alpha or None, d_a0_soa or None,
        d_transfer_soa or None, int(flags), d_a_end_soa or None, d_p_end or None, d_p_max or None,
        d_first_bad or None, d_traj_soa or None, d_p_wave_end or None, d_p_wave_max or None, d_workspace or None))


def rk45_sweep_host(dbeta, *, z_max: float, rtol: float, atol: float, h_max: float = float("inf"),
                    first_step: float = 0.0, max_steps: int = 1_000_000, n_out: int = 0, gamma, alpha, a0, dbeta2=None,
                    device: int = 0, extra_flags: int = 0) -> dict:
    """N independent adaptive (RK45) propagations on the GPU (psa_rk45_sweep_f64; host buffers in and out, float64).

    dbeta (N,); gamma / alpha scalar or (N,); a0 (n_waves,) or (N, n_waves) complex.  n_out > 0 also returns the
    dense-output rows traj (N, n_out + 1, n_waves) at np.linspace(0, z_max, n_out + 1).
    Returns a_end (N, n_waves) complex, p_end, p_max, z_end (N,), status (N,) int32, n_accepted, n_rejected (N,) int64,
    traj or None, elapsed_ms (kernel only)."""
    dbeta = np.ascontiguousarray(np.atleast_1d(np.asarray(dbeta)), dtype=np.float64)
    if dbeta.ndim != 1:
        raise ValueError("dbeta must be 1-D")
    N = int(dbeta.shape[0])
    flags, gamma, alpha, a0, d2 = _point_inputs(N, np.float64, np.complex128, int(extra_flags), gamma, alpha, a0, (4, 6),
                                                dbeta, dbeta2)
    nw = int(a0.shape[1])
    n_out = int(n_out)
    a_end = np.empty((N, nw), dtype=np.complex128)
    p_end, p_max, z_end = (np.empty(N, dtype=np.float64) for _ in range(3))
    status = np.empty(N, dtype=np.int32)
    n_acc, n_rej = np.empty(N, dtype=np.int64), np.empty(N, dtype=np.int64)
    traj = np.empty((N, n_out + 1, nw), dtype=np.complex128) if n_out > 0 else None
    ms = C.c_double(0.0)
    _check(_fn("psa_rk45_sweep")(int(device), nw, N, float(z_max), float(rtol), float(atol), float(h_max),
                                 float(first_step), int(max_steps), n_out, _ptr(dbeta), _ptr(d2), _ptr(gamma),
                                 _ptr(alpha), _ptr(a0), flags, _ptr(a_end), _ptr(p_end), _ptr(p_max), _ptr(status),
                                 _ptr(z_end), _ptr(n_acc), _ptr(n_rej), _ptr(traj), C.cast(C.byref(ms), _P)))
    return dict(a_end=a_end, p_end=p_end, p_max=p_max, status=status, z_end=z_end, n_accepted=n_acc,
                n_rejected=n_rej, traj=traj, elapsed_ms=ms.value)


def rk45_sweep_device(*, stream: int, n_waves: int, n_points: int, z_max: float, rtol: float, atol: float,
                      h_max: float, first_step: float, max_steps: int, n_out: int, d_dbeta: int, d_dbeta2: int,
                      d_gamma: int, d_alpha: int, d_a0_soa: int, flags: int, d_a_end_soa: int, d_p_end: int,
                      d_p_max: int, d_status: int, d_z_end: int, d_n_accepted: int, d_n_rejected: int,
                      d_traj_soa: int = 0) -> None:
    """Asynchronous adaptive launch on device pointers (ints), SoA layout -- see psa_rk45_sweep_f64_dev."""
    _check(_fn("psa_rk45_sweep", dev=True)(
        stream or None, int(n_waves), int(n_points), float(z_max), float(rtol), float(atol), float(h_max),
        float(first_step), int(max_steps), int(n_out), d_dbeta or None, d_dbeta2 or None, d_gamma or None,
        d_alpha or None, d_a0_soa or None, int(flags), d_a_end_soa or None, d_p_end or None, d_p_max or None,
        d_status or None, d_z_end or None, d_n_accepted or None, d_n_rejected or None, d_traj_soa or None))


def yaman_rhs_host(z, a, gamma, alpha, dbeta, *, terms: bool = False, device: int = 0):
    """Batched yaman_model.rhs_yaman_simplified on the GPU: a (N,4) complex -> (N,4) complex."""
    a = np.ascontiguousarray(np.asarray(a), dtype=np.complex128)
    if a.ndim == 1:
        a = a[None, :]
    if a.ndim != 2 or a.shape[1] != 4:
        raise ValueError("a_arr must have shape (4,)")
    N = a.shape[0]
    bc = lambda x: np.ascontiguousarray(np.broadcast_to(np.asarray(x, dtype=np.float64), (N,)))  # noqa: E731
    z, gamma, alpha, dbeta = bc(z), bc(gamma), bc(alpha), bc(dbeta)
    out = np.empty((N, 4), dtype=np.complex128)
    parts = [np.empty((N, 4), dtype=np.complex128) for _ in range(3)] if terms else [None, None, None]
    _check(lib().psa_yaman_rhs_f64(int(device), N, _ptr(z), _ptr(a), _ptr(gamma), _ptr(alpha), _ptr(dbeta),
                                   _ptr(out), _ptr(parts[0]), _ptr(parts[1]), _ptr(parts[2])))
    return (out, *parts) if terms else out


def gain_summary_host(p_metric, first_bad_step, p0_sig: float, *, gain_db: bool = True, device: int = 0):
    """Per-point gain (NaN on failure) + (argmax, max, #finite) over the sweep, reduced on the GPU.
    A float32 ``p_metric`` (a float32 sweep) goes through ``psa_gain_summary_f32`` and returns float32 gains."""
    p = np.asarray(p_metric)
    f32 = p.dtype == np.float32
    p = np.ascontiguousarray(p, dtype=np.float32 if f32 else np.float64)
    bad = None if first_bad_step is None else np.ascontiguousarray(np.asarray(first_bad_step), dtype=np.int64)
    N = p.shape[0]
    gain = np.empty(N, dtype=p.dtype)
    bi = C.c_int64(-1)
    bg = C.c_double(float("nan"))
    nf = C.c_int64(0)
    _check(_fn("psa_gain_summary", not f32)(int(device), N, _ptr(p), _ptr(bad), float(p0_sig), int(bool(gain_db)), _ptr(gain),
                                            C.cast(C.byref(bi), _P), C.cast(C.byref(bg), _P), C.cast(C.byref(nf), _P)))
    return gain, int(bi.value), float(bg.value), int(nf.value)


def gain_summary_device(*, stream: int, n_points: int, d_p_metric: int, d_first_bad: int, p0_sig: float, gain_db: bool,
                        d_gain: int, d_best_index: int, d_best_gain: int, d_n_finite: int, d_workspace: int,
                        dtype=np.float64) -> None:
    """Asynchronous gain reduction on device pointers (ints) -- see psa_gain_summary_f64_dev / _f32_dev."""
    _check(_fn("psa_gain_summary", _is_f64(dtype), dev=True)(
        stream or None, int(n_points), d_p_metric or None, d_first_bad or None, float(p0_sig), int(bool(gain_db)),
        d_gain or None, d_best_index or None, d_best_gain or None, d_n_finite or None, d_workspace or None))


def gain_summary_workspace_bytes(n_points: int) -> int:
    return int(lib().psa_gain_summary_workspace_bytes(int(n_points)))


# ---- device-side dbeta producer (psa_dbeta_grid_* / psa_dbeta_pairs_*) -------------------------------------------
def dbeta_model(disp, pm_cfg=None, *, even_orders=None) -> dict:
    """The C-ABI's description of (DispersionParams, PhaseMatchingConfig): method, even orders / max order, beta_0..beta_8,
    omega_ref, tolerances.  ``pm_cfg=None`` + ``even_orders`` describes the symmetric closed form alone (six-wave grid).
    Raises ValueError for what the device producer does not cover (PROVIDED, orders above 8)."""
    from .phase_matching import PhaseMatchingMethod
    if disp is None:
        raise ValueError("disp must be provided unless method == 'provided'")
    top = DBETA_MAX_ORDER
    if disp.extra is not None and any(int(k) > top and v != 0.0 for k, v in disp.extra.items()):
        raise ValueError(f"the device dbeta producer covers dispersion orders up to {top}")
    beta = np.array([disp.get_beta_n(n) for n in range(top + 1)], dtype=np.float64)
    if pm_cfg is None:
        method, orders, max_order, atol, rtol = DBETA_SYMMETRIC_EVEN, tuple(even_orders or (2, 4)), 0, 0.0, 1e-12
    elif pm_cfg.method == PhaseMatchingMethod.SYMMETRIC_EVEN:
        method, orders, max_order, atol, rtol = DBETA_SYMMETRIC_EVEN, tuple(pm_cfg.even_orders), 0, pm_cfg.atol, pm_cfg.rtol
    elif pm_cfg.method == PhaseMatchingMethod.GENERAL_TAYLOR:
        method, orders, max_order, atol, rtol = DBETA_GENERAL_TAYLOR, (), int(pm_cfg.max_order), pm_cfg.atol, pm_cfg.rtol
    else:
        raise ValueError("a PROVIDED dbeta is an input, not something to generate")
    if method == DBETA_SYMMETRIC_EVEN and (not 1 <= len(orders) <= 4 or any(n > top for n in orders)):
        raise ValueError(f"the device dbeta producer takes 1..4 even orders up to {top}")
    if method == DBETA_GENERAL_TAYLOR and max_order > top:
        raise ValueError(f"the device dbeta producer covers max_order up to {top}")
    from . import constants
    return dict(method=method, orders=np.asarray(orders, dtype=np.int32), max_order=max_order, beta=beta,
                omega_ref=float(disp.omega_ref), two_pi_c=2.0 * np.pi * constants.c, atol=float(atol), rtol=float(rtol))


def _model_head(m: dict):
    return (int(m["method"]), _ptr(m["orders"]) if m["orders"].size else None, int(m["orders"].size), int(m["max_order"]),
            _ptr(m["beta"]), int(m["beta"].size), m["omega_ref"], m["two_pi_c"], m["atol"], m["rtol"])


def dbeta_grid_host(model: dict, lambda1_m: float, lambda2_axis, lambda3_axis, *, first: int = 0,
                    n_points: Optional[int] = None, device: int = 0):
    """dbeta (and validity) of points [first, first + n_points) of the flattened lambda2 x lambda3 grid, on the GPU."""
    ax2 = np.ascontiguousarray(np.atleast_1d(lambda2_axis), dtype=np.float64)
    ax3 = np.ascontiguousarray(np.atleast_1d(lambda3_axis), dtype=np.float64)
    n = ax2.size * ax3.size - int(first) if n_points is None else int(n_points)
    out = np.empty(n, dtype=np.float64)
    valid = np.empty(n, dtype=np.uint8)
    _check(lib().psa_dbeta_grid_f64(int(device), *_model_head(model), float(lambda1_m), _ptr(ax2), ax2.size, _ptr(ax3),
                                    ax3.size, int(first), n, _ptr(out), _ptr(valid)))
    return out, valid.astype(bool)


def dbeta_grid_device(model: dict, lambda1_m: float, *, stream: int, d_lambda2_axis: int, n2: int, d_lambda3_axis: int,
                      n3: int, first: int, n_points: int, d_dbeta: int, d_valid: int = 0, dtype=np.float64) -> None:
    _check(_fn("psa_dbeta_grid", _is_f64(dtype), dev=True)(
        stream or None, *_model_head(model), float(lambda1_m), d_lambda2_axis or None, int(n2), d_lambda3_axis or None,
        int(n3), int(first), int(n_points), d_dbeta or None, d_valid or None))


def dbeta_pairs_host(model: dict, omega_d: float, Omega1_axis, Omega2_axis, *, first: int = 0,
                     n_points: Optional[int] = None, device: int = 0):
    ax1 = np.ascontiguousarray(np.atleast_1d(Omega1_axis), dtype=np.float64)
    ax2 = np.ascontiguousarray(np.atleast_1d(Omega2_axis), dtype=np.float64)
    n = ax1.size * ax2.size - int(first) if n_points is None else int(n_points)
    o1, o2 = np.empty(n, dtype=np.float64), np.empty(n, dtype=np.float64)
    _check(lib().psa_dbeta_pairs_f64(int(device), _ptr(model["orders"]), int(model["orders"].size), _ptr(model["beta"]),
                                     int(model["beta"].size), float(omega_d), _ptr(ax1), ax1.size, _ptr(ax2), ax2.size,
                                     int(first), n, _ptr(o1), _ptr(o2)))
    return o1, o2


def dbeta_pairs_device(model: dict, omega_d: float, *, stream: int, d_Omega1_axis: int, n1: int, d_Omega2_axis: int,
                       n2: int, first: int, n_points: int, d_dbeta1: int, d_dbeta2: int, dtype=np.float64) -> None:
    _check(_fn("psa_dbeta_pairs", _is_f64(dtype), dev=True)(
        stream or None, _ptr(model["orders"]), int(model["orders"].size), _ptr(model["beta"]), int(model["beta"].size),
        float(omega_d), d_Omega1_axis or None, int(n1), d_Omega2_axis or None, int(n2), int(first), int(n_points),
        d_dbeta1 or None, d_dbeta2 or None))
