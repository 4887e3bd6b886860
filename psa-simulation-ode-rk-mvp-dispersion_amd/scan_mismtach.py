"""Sweep drivers with the reference's call surface (the module keeps the upstream spelling ``scan_mismtach``).

* ``plot_max_signal_gain_vs_lambda_signal(...) -> (x, gain_max)``            reference scan_mismtach.py:262-430
* ``plot_max_gain_and_dbeta_vs_lambda_signal(...) -> (x, gain_max, dbeta)``  reference scan_mismtach.py:588-783
* ``plot_dbeta_vs_lambda_signal(...) -> (x, dbeta)``: what reference scan_mismtach.py:473-585 sets out to return (there every
  point comes back NaN: its ``_omega0_from_dispersion`` looks for a field the dataclass does not have)
* ``scan_dbeta_seeded_signal(...)``: a working direct-dbeta scan with gain_mode "end" | "max" and the
  argmax-over-sweep summary -- what the reference's dead ``scan_mismatch_seeded_signal`` (:43-259) set out to do.
  ``with_idler=True`` adds the idler gain Gi (per-wave summary, psa_rk4_sweep_waves_*).
* ``seeded_mismatch_scan(gain_mode)``: the scenario that dead function hard-codes (:56-93), run: delta, Gs, Gi, best point.
* ``scan_copier_psa_phase(...)``: signal gain of a copier - mid-stage - PSA chain against the mid-stage phase (optionally
  times the PSA span's dbeta) in one chain launch, with its maximum, minimum and extinction (no reference counterpart).
* ``scan_single_pump_copier_psa_phase(...)``: the same scan for the single-pump three-wave model [p, s, i], with the
  idler's gain next to the signal's.
* ``scan_gain_grid(...)``: the same sweep over a 2-D (pump-2 wavelength x signal wavelength) grid in one launch
  (BASELINE config 3's shape: 1024 x 1024 points); the reference has no grid builder.
* ``scan_six_wave_grid(...)``: BASELINE config 5's shape -- a grid over the detunings (Omega1, Omega2) of two
  signal/idler pairs sharing the two pumps, on the build-defined 6-wave model (no reference counterpart).

Where the reference loops over lambda3 in Python and calls ``run_single_simulation`` per point, these drivers
build every plan and every dbeta at once on the host (``plan_from_wavelengths_batch``,
``compute_phase_mismatch_batch``), launch ONE HIP sweep over all valid points and reduce the gain on the GPU.

Several GPUs (the reference's loop over points is embarrassingly parallel, scan_mismtach.py:357-392, :694-738):
* under a ``torch.distributed`` process group (one process per GPU, ``torchrun``) every driver takes its rank's share of
  the points (``_partition.Share``), produces the phase mismatch of ITS block (on its GPU with the device producer),
  integrates it and hands the block to ``distributed.exchange_blocks``: ONE all_gather of the output record (RCCL under
  ``nccl``); every rank returns the full arrays.  If a rank's block raises (a native error in its producer or its sweep),
  every rank raises after the gather -- except a failing Δβ producer of ``_sweep_gain``'s grid, whose points become NaN;
* a plain Python caller passes ``devices=[0, 1, ...]``: one host thread per GPU (``_partition.over_devices``).

Failure conventions kept from the reference: malformed arguments raise ``ValueError`` up front
(:315-349, :630-671); anything that would raise INSIDE the per-point ``try`` (an impossible plan, a bad cfg,
FloatingPointError from ``check_nan``) never raises -- the point's gain (and dbeta) is NaN (:391-392, :736-738).
Plotting is presentation only: it happens after the numbers exist and only if matplotlib is importable.
"""
from __future__ import annotations

from typing import Literal, Optional, Sequence, Tuple

import numpy as np

from .config import SimulationConfig, custom_simulation_config, n_steps_of  # noqa: F401
from .dispersion import DispersionParams, delta_beta_symmetric_array
from .frequency_plan import plan_from_wavelengths_batch
from ._partition import SWEEP_AXES, Share, cut
from .phase_matching import PhaseMatchingConfig, PhaseMatchingMethod, compute_phase_mismatch_batch
from .simulation import _prepare, make_initial_amplitudes
from .sweep import SweepResult, check_gain, rk4_sweep

GainMode = Literal["end", "max"]
_PROVIDED = PhaseMatchingConfig(method=PhaseMatchingMethod.PROVIDED, provided_delta_beta=0.0)


def _select_power_metric(Pz: np.ndarray, mode: GainMode) -> float:
    """P(z_max) ("end") or max_z P(z) ("max") of one power trace (scan_mismtach.py:27-40)."""
    Pz = np.asarray(Pz)
    if Pz.ndim != 1:
        raise ValueError("Pz must be a 1D array of power versus z.")
    check_gain(mode)
    return float(Pz[-1]) if mode == "end" else float(np.max(Pz))


# ---- argument checks shared by the two lambda3 drivers ---------------------------------------------------
def _check_sweep_inputs(lambda_signal_m, p_in, phase_in):
    lam3 = np.asarray(list(lambda_signal_m), dtype=float)
    if lam3.ndim != 1 or lam3.size == 0:
        raise ValueError("lambda_signal_m must be a non-empty 1D sequence")
    if not np.all(np.isfinite(lam3)) or np.any(lam3 <= 0.0):
        raise ValueError("lambda_signal_m must contain finite positive wavelengths (m)")
    p0 = np.asarray(list(p_in), dtype=float)
    if p0.shape != (4,):
        raise ValueError(f"p_in must have shape (4,), got {p0.shape}")
    if not np.all(np.isfinite(p0)) or np.any(p0 < 0.0):
        raise ValueError("p_in must contain finite non-negative powers")
    if p0[2] <= 0.0:
        raise ValueError("p_in[2] (signal seed power) must be > 0 to define gain")
    ph0 = None
    if phase_in is not None:
        ph0 = np.asarray(list(phase_in), dtype=float)
        if ph0.shape != (4,):
            raise ValueError(f"phase_in must have shape (4,), got {ph0.shape}")
        if not np.all(np.isfinite(ph0)):
            raise ValueError("phase_in must contain finite values")
    return lam3, p0, ph0


def _norm_choice(value, name, allowed):
    v = str(value).strip().lower()
    if v not in allowed:
        raise ValueError(f"{name} must be " + " or ".join(f"'{a}'" for a in allowed))
    return v


def _wavelength_axis(lam3, unit):
    u = unit.strip().lower()
    if u == "nm":
        return lam3 * 1e9, r"Signal wavelength $\lambda_3$ (nm)"
    if u == "m":
        return lam3, r"Signal wavelength $\lambda_3$ (m)"
    raise ValueError("return_wavelength_unit must be 'm' or 'nm'")


NEVER_RAN = -2    # first_bad_step of a point whose plan / dbeta was invalid: it never reached the kernel


def _run_block(share: Share, inputs, *, n_extras=0, n_waves=4, dtype=np.float64, devices=None, **run_kw):
    """Integrate the valid points of this process's block and, when the call is sharded over a process group, exchange
    the blocks (``distributed.exchange_blocks``): every rank ends up with the whole sweep.

    ``inputs()`` -> (ok | None (all valid), dbeta, dbeta2 | None, extras) of the block: its validity mask, per-metre
    mismatch and ``n_extras`` per-point float64 arrays that travel with the record (the caller-unit dbeta); it runs inside
    the exchange, so a rank whose producer raises makes every rank raise.  run_kw: rk4_sweep's arguments for the WHOLE
    sweep.  Returns (SweepResult over the valid points of the whole sweep in order | None, ok[n], [extras over n]).  With
    ``wave_summary=True`` in run_kw the per-wave columns (p_wave_end, p_wave_max) ride in the same all_gather as
    2 * n_waves more extras (float64; a float32 sweep's values convert exactly)."""
    waves = bool(run_kw.get("wave_summary"))

    def block():
        ok, db, db2, extras = inputs()
        ok = np.ones(len(db), dtype=bool) if ok is None else np.asarray(ok, dtype=bool)
        idx = np.flatnonzero(ok)
        res = None
        if idx.size:
            res = rk4_sweep(np.asarray(db)[idx], dbeta2=(None if db2 is None else np.asarray(db2)[idx]), dtype=dtype,
                            device=share.device, devices=(None if share.sharded else devices),
                            **cut(run_kw, SWEEP_AXES, share.n, share.lo + idx if share.lo else idx))
        return ok, idx, res, list(extras)

    if not share.sharded:
        ok, _, res, extras = block()
        return res, ok, [np.asarray(e) for e in extras]

    from .distributed import RecordLayout, exchange_blocks
    layout = RecordLayout(n_waves, dtype)

    def record():
        ok, idx, res, extras = block()
        nb = ok.size
        a_end = np.full((nb, n_waves), np.nan, dtype=layout.cdtype)
        p_end, p_max = np.full(nb, np.nan, dtype=layout.dtype), np.full(nb, np.nan, dtype=layout.dtype)
        bad = np.full(nb, NEVER_RAN, dtype=np.int64)
        if res is not None:
            a_end[idx], p_end[idx], p_max[idx], bad[idx] = res.a_end, res.p_end, res.p_max, res.first_bad_step
        if waves:                               # columns j of p_wave_end, then of p_wave_max
            wcols = np.full((nb, 2 * n_waves), np.nan)
            if res is not None:
                wcols[idx, :n_waves], wcols[idx, n_waves:] = res.p_wave_end, res.p_wave_max
            extras += [wcols[:, k] for k in range(2 * n_waves)]
        return dict(a_end=a_end, p_end=p_end, p_max=p_max, first_bad_step=bad, extras=extras,
                    elapsed_ms=(0.0 if res is None else res.elapsed_ms))

    local, (a_end, p_end, p_max, bad), ext = exchange_blocks(share, layout, record, n_extras + (2 * n_waves if waves else 0))
    ok = bad != NEVER_RAN
    full = None
    if ok.any():
        w_end = w_max = None
        if waves:
            w = np.stack(ext[n_extras:], axis=1)[ok].astype(layout.dtype)
            w_end, w_max = np.ascontiguousarray(w[:, :n_waves]), np.ascontiguousarray(w[:, n_waves:])
        full = SweepResult(a_end[ok], p_end[ok], p_max[ok], bad[ok], int(run_kw["n_steps"]), int(run_kw["save_every"]),
                           local["elapsed_ms"], None, w_end, w_max)
    return full, ok, ext[:n_extras]


# ---- the engine call shared by the drivers ------------------------------------------------------------------
def _grid_dbeta(lam1, lam2_axis, lam3_axis, disp, pm_cfg, producer, device, lo=0, hi=None):
    """dbeta and validity of points [lo, hi) of the flattened lambda_p2 x lambda_signal grid (row-major; default: all).
    producer "host": the NumPy array restatement (frequency_plan / phase_matching ``*_batch``);
    producer "device": the same operations on the GPU (psa_dbeta_grid_f64, csrc/psa_dbeta.hip) -- a rank of a sharded sweep
    produces exactly its own block, so no per-point input ever travels."""
    ax2, ax3 = np.atleast_1d(lam2_axis), np.atleast_1d(lam3_axis)
    hi = ax2.size * ax3.size if hi is None else hi
    if producer == "device":
        from . import _native
        if hi == lo:
            return np.zeros(0), np.zeros(0, dtype=bool)
        return _native.dbeta_grid_host(_native.dbeta_model(disp, pm_cfg), float(lam1), ax2, ax3, first=lo, n_points=hi - lo,
                                       device=device)
    if producer != "host":
        raise ValueError("dbeta_producer must be 'host' or 'device'")
    i = np.arange(lo, hi)
    omega, ok = plan_from_wavelengths_batch(float(lam1), ax2[i // ax3.size], ax3[i % ax3.size])
    db, ok_db = compute_phase_mismatch_batch(omega, disp, pm_cfg)
    ok = ok & ok_db
    return np.where(ok, db, np.nan), ok


def _pick_producer(choice, n_points, disp, pm_cfg, even_orders=None):
    """"host" | "device" | "auto": auto takes the device producer for grids of 4 096 points or more when the model is one
    it covers (the NumPy producer costs ~0.2 us per point, 230 ms on BASELINE config 3's 1024 x 1024 grid against 19 ms
    of host time with the device producer; the two agree bit for bit on the reference's vectors).  The
    choice follows the size of the WHOLE sweep, so a sharded call picks what the unsharded one would."""
    if choice in ("host", "device"):
        return choice
    if choice != "auto":
        raise ValueError("dbeta_producer must be 'auto', 'host' or 'device'")
    if n_points < 4096 or disp is None:
        return "host"
    try:
        from . import _native
        _native.dbeta_model(disp, pm_cfg, even_orders=even_orders)
        return "device"
    except ValueError:
        return "host"


def _sweep_gain(*, cfg, lam1, grid_axes, gamma, alpha, p0, ph0, dispersion, pm_cfg, length_unit, gain_unit,
                gain_mode="max", device=None, devices=None, dbeta_producer="host", caller_dbeta=None):
    """Everything the reference does inside its per-point ``try``, for all points of the lambda_p2 x lambda_signal grid
    ``grid_axes`` at once (a lambda3 sweep is its 1 x N case).

    ``caller_dbeta = (dispersion as given, pm_cfg)`` also produces the drivers' returned dbeta (1/length_unit, computed
    from the UNSCALED dispersion like scan_mismtach.py:700-706) block by block.  Returns (gain[N], dbeta_caller[N] | None,
    SweepResult | None).  Never raises for per-point or cfg problems: those become NaN, as ``except Exception`` does upstream.
    """
    if dbeta_producer not in ("auto", "host", "device"):       # a caller error, not a per-point failure
        raise ValueError("dbeta_producer must be 'auto', 'host' or 'device'")
    ax2, ax3 = np.atleast_1d(grid_axes[0]), np.atleast_1d(grid_axes[1])
    N = ax2.size * ax3.size
    shard = Share(N, device)
    gain = np.full(N, np.nan)
    nb = shard.hi - shard.lo
    try:
        # plan-independent part of run_single_simulation (validation, unit scaling, containers)
        pre = _prepare(cfg, gamma=gamma, alpha=alpha, dispersion=dispersion, phase_matching_cfg=pm_cfg,
                       beta_legacy=None, length_unit=length_unit)
        a0 = make_initial_amplitudes(p0, ph0)
        fiber, grid, pm = pre["fiber"], pre["grid"], pre["pm"].config
        producer = _pick_producer(dbeta_producer, N, fiber.dispersion, pm)
        n_steps = n_steps_of(fiber.length_m, grid.dz_m)
        if n_steps < 1:
            raise ValueError("no steps")
        run_kw = dict(z_max=fiber.length_m, n_steps=n_steps, save_every=cfg.save_every, check_nan=bool(cfg.check_nan),
                      gamma=fiber.gamma_W_m, alpha=fiber.alpha_1_m, a0=a0)
    except Exception:
        # a bad cfg fails identically on every rank (same arguments), so nobody enters the collective: the returned dbeta
        # (which upstream is set before the run is attempted) is then produced for the whole grid by each rank itself
        cd = None
        if caller_dbeta is not None:
            try:
                cd, _ = _grid_dbeta(lam1, ax2, ax3, caller_dbeta[0], caller_dbeta[1],
                                    _pick_producer(dbeta_producer, N, caller_dbeta[0], caller_dbeta[1]), shard.device)
            except Exception:
                cd = np.full(N, np.nan)
        return gain, cd, None

    def inputs():
        try:
            dbeta_m, ok = _grid_dbeta(lam1, ax2, ax3, fiber.dispersion, pm, producer, shard.device, shard.lo, shard.hi)
        except Exception:       # this block's producer failed (e.g. a native error on this rank only): its points are NaN
            dbeta_m, ok = np.full(nb, np.nan), np.zeros(nb, dtype=bool)
        extras = []
        if caller_dbeta is not None:
            try:
                cd, _ = _grid_dbeta(lam1, ax2, ax3, caller_dbeta[0], caller_dbeta[1],
                                    _pick_producer(dbeta_producer, N, caller_dbeta[0], caller_dbeta[1]), shard.device,
                                    shard.lo, shard.hi)
            except Exception:
                cd = np.full(nb, np.nan)
            extras = [cd]
        return ok, dbeta_m, None, extras

    res, ok_full, extras_full = _run_block(shard, inputs, n_extras=int(caller_dbeta is not None), devices=devices, **run_kw)
    if res is not None:
        gain[ok_full] = res.gain(p0[2], mode=gain_mode, unit=gain_unit, device=shard.device)
    return gain, (extras_full[0] if extras_full else None), res


def _maybe_plot(draw, save_path, show):
    """Presentation tail (scan_mismtach.py:412-428, :753-781); skipped when there is nothing to show or save."""
    if save_path is None and not show:
        return
    try:
        import matplotlib.pyplot as plt
    except Exception:  # plotting is optional here
        return
    fig = draw(plt)
    if save_path is not None:
        fig.savefig(save_path, dpi=200, bbox_inches="tight")
    if show:
        plt.show()
    else:
        plt.close(fig)


def plot_max_signal_gain_vs_lambda_signal(*, cfg: SimulationConfig, lambda_p1_m: float, lambda_p2_m: float,
                                          lambda_signal_m: Sequence[float], gamma: float, alpha: float,
                                          p_in: Sequence[float], phase_in: Optional[Sequence[float]] = None,
                                          dispersion: Optional[DispersionParams] = None,
                                          phase_matching_cfg: Optional[PhaseMatchingConfig] = None,
                                          length_unit: str = "m", return_wavelength_unit: str = "nm",
                                          gain_unit: str = "dB", xscale: str = "linear", yscale: str = "linear",
                                          show_progress: bool = True, tqdm_desc: str = "Sweeping λ3",
                                          save_path: Optional[str] = None, show: bool = True,
                                          devices: Optional[Sequence[int]] = None) -> Tuple[np.ndarray, np.ndarray]:
    """Max-over-z signal gain versus lambda3 -> (x_wavelength, gain_max); NaN where a point failed.

    ``show_progress`` / ``tqdm_desc`` are accepted for compatibility: the sweep is a single kernel launch.
    ``devices`` (not upstream): GPUs of this process to split the points over; under a process group the ranks split them.
    """
    lam1, lam2 = float(lambda_p1_m), float(lambda_p2_m)
    lam3, p0, ph0 = _check_sweep_inputs(lambda_signal_m, p_in, phase_in)
    unit = check_gain(unit=gain_unit)
    xs = _norm_choice(xscale, "xscale", ("linear", "log"))
    ys = _norm_choice(yscale, "yscale", ("linear", "log"))
    if ys == "log" and unit == "db":
        raise ValueError("yscale='log' is not supported with gain_unit='dB'. Use gain_unit='linear'.")
    _wavelength_axis(lam3, return_wavelength_unit)   # the reference raises this only AFTER its sweep; here before any device work

    # a lambda3 sweep is the 1 x N case of the grid: sweeps of 4 096 points or more get their dbeta from the device producer
    gain, _, _ = _sweep_gain(cfg=cfg, lam1=lam1, grid_axes=(np.array([lam2]), lam3), gamma=gamma, alpha=alpha, p0=p0, ph0=ph0,
                             dispersion=dispersion, pm_cfg=phase_matching_cfg, length_unit=length_unit,
                             gain_unit=unit, dbeta_producer="auto", devices=devices)
    x, x_label = _wavelength_axis(lam3, return_wavelength_unit)

    def draw(plt):
        fig = plt.figure()
        plt.plot(x, gain, marker="o")
        plt.xlabel(x_label)
        plt.ylabel(r"Max signal gain $G_{\max}$ (linear)" if unit == "linear" else r"Max signal gain $G_{\max}$ (dB)")
        plt.title("Maximum signal gain vs signal wavelength")
        plt.grid(True, which="both")
        plt.xscale(xs)
        plt.yscale(ys)
        return fig

    _maybe_plot(draw, save_path, show)
    return x, gain


def plot_max_gain_and_dbeta_vs_lambda_signal(*, cfg: SimulationConfig, lambda_p1_m: float, lambda_p2_m: float,
                                             lambda_signal_m: Sequence[float], gamma: float, alpha: float,
                                             p_in: Sequence[float], phase_in: Optional[Sequence[float]] = None,
                                             dispersion: DispersionParams,
                                             phase_matching_cfg: Optional[PhaseMatchingConfig] = None,
                                             length_unit: str = "m", return_wavelength_unit: str = "nm",
                                             gain_unit: str = "dB", xscale: str = "linear",
                                             yscale_gain: str = "linear", yscale_dbeta: str = "linear",
                                             show_progress: bool = True,
                                             tqdm_desc: str = "Sweeping λ3 (gain + dBeta)",
                                             save_path: Optional[str] = None, show: bool = True,
                                             devices: Optional[Sequence[int]] = None
                                             ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """One sweep that returns both the max signal gain and dbeta(lambda3) -> (x, gain_max, dbeta).

    ``dbeta`` is in 1/length_unit, computed from the dispersion AS GIVEN (scan_mismtach.py:700-706); the kernel
    uses the per-metre value derived from the scaled dispersion (simulation.py:340), exactly as upstream.
    """
    lam1, lam2 = float(lambda_p1_m), float(lambda_p2_m)
    lam3, p0, ph0 = _check_sweep_inputs(lambda_signal_m, p_in, phase_in)
    if dispersion is None:
        raise ValueError("dispersion must be provided to compute dBeta(λ3)")
    unit = check_gain(unit=gain_unit)
    xs = _norm_choice(xscale, "xscale", ("linear", "log"))
    ysg = _norm_choice(yscale_gain, "yscale_gain", ("linear", "log"))
    ysd = _norm_choice(yscale_dbeta, "yscale_dbeta", ("linear", "log"))
    if ysg == "log" and unit == "db":
        raise ValueError("yscale_gain='log' is not supported with gain_unit='dB'. Use gain_unit='linear'.")
    pm_cfg = phase_matching_cfg if phase_matching_cfg is not None else PhaseMatchingConfig(
        method=PhaseMatchingMethod.SYMMETRIC_EVEN, max_order=4, even_orders=(2, 4), atol=0.0, rtol=1e-12)
    _wavelength_axis(lam3, return_wavelength_unit)   # validated up front (upstream: after the sweep)

    # dbeta in the caller's units travels with the sweep: per point, NaN where the plan or the mismatch is invalid (a lambda3
    # sweep is the 1 x N case of the grid: 4 096 points or more go through the device producer)
    gain, dbeta, _ = _sweep_gain(cfg=cfg, lam1=lam1, grid_axes=(np.array([lam2]), lam3), gamma=gamma, alpha=alpha, p0=p0,
                                 ph0=ph0, dispersion=dispersion, pm_cfg=pm_cfg, length_unit=length_unit, gain_unit=unit,
                                 dbeta_producer="auto", caller_dbeta=(dispersion, pm_cfg), devices=devices)
    gain = np.where(np.isnan(dbeta), np.nan, gain)   # a point whose dbeta failed never reaches the run upstream
    x, x_label = _wavelength_axis(lam3, return_wavelength_unit)
    ref_line = -float(gamma) * float(p0[0] + p0[1])

    def draw(plt):
        fig, (ax1, ax2) = plt.subplots(2, 1, sharex=True, figsize=(9, 7))
        ax1.plot(x, gain, marker="o")
        ax1.set_ylabel("Max signal gain (linear)" if unit == "linear" else "Max signal gain (dB)")
        ax1.grid(True, which="both", alpha=0.3)
        ax1.set_yscale(ysg)
        ax2.plot(x, dbeta, marker="o", label=r"$\Delta\beta(\lambda_3)$")
        ax2.axhline(ref_line, ls="--", lw=2, label=r"$\gamma(P_1+P_2)$")
        ax2.set_xlabel(x_label)
        ax2.set_ylabel(rf"$\Delta\beta$  [1/{length_unit}]")
        ax2.grid(True, which="both", alpha=0.3)
        ax2.set_xscale(xs)
        ax2.set_yscale(ysd)
        ax2.legend()
        fig.suptitle("Max signal gain and phase mismatch vs signal wavelength")
        fig.tight_layout()
        return fig

    _maybe_plot(draw, save_path, show)
    return x, gain, dbeta


def plot_dbeta_vs_lambda_signal(*, gamma: float, lambda_p1_m: float, lambda_p2_m: float, lambda_signal_m: Sequence[float],
                                p_in: Sequence[float], dispersion: DispersionParams, return_wavelength_unit: str = "nm",
                                xscale: str = "linear", yscale: str = "linear", length_unit: str = "m",
                                show_progress: bool = True, tqdm_desc: str = "Scanning dBeta(λ3)",
                                title: Optional[str] = None, save_path: Optional[str] = None, show: bool = True,
                                device: Optional[int] = None, dbeta_producer: str = "auto"
                                ) -> Tuple[np.ndarray, np.ndarray]:
    """dbeta(lambda3) = beta(w1) + beta(w2) - beta(w3) - beta(w4) with beta by its Taylor series through order 4, next to the
    line gamma*(P1 + P2) -> (x, dbeta); dbeta in 1/(the length unit of the dispersion coefficients).

    The call surface, argument checks and NaN-per-failed-point rule of reference scan_mismtach.py:473-585.  Upstream the
    function returns NaN for every point (its helper asks the dispersion object for ``omega0``, the field is ``omega_ref``,
    and the exception is swallowed: SURVEY R3); the quantity its docstring and ``_beta_taylor`` (:441-459) describe is the
    reference's own ``delta_beta_from_omegas`` (dispersion.py:282-318, beta0 and beta1 cancel by energy conservation), which
    is what is returned here -- through the array producer, or the device one for 4 096 points or more.
    """
    lam1, lam2 = float(lambda_p1_m), float(lambda_p2_m)
    lam3 = np.asarray(list(lambda_signal_m), dtype=float)
    if lam3.ndim != 1 or lam3.size == 0:
        raise ValueError("lambda_signal_m must be a non-empty 1D sequence")
    if not np.all(np.isfinite(lam3)) or np.any(lam3 <= 0.0):
        raise ValueError("lambda_signal_m must contain finite positive wavelengths (m)")
    p0 = np.asarray(list(p_in), dtype=float)
    if p0.shape != (4,):
        raise ValueError(f"p_in must have shape (4,), got {p0.shape}")
    if not np.all(np.isfinite(p0)) or np.any(p0 < 0.0):
        raise ValueError("p_in must contain finite non-negative powers")
    xs = _norm_choice(xscale, "xscale", ("linear", "log"))
    ys = _norm_choice(yscale, "yscale", ("linear", "log"))
    if dispersion is None:
        raise ValueError("dispersion must be provided to compute dBeta(λ3)")

    pm_cfg = PhaseMatchingConfig(method=PhaseMatchingMethod.GENERAL_TAYLOR, max_order=4, atol=0.0, rtol=1e-12)
    producer = _pick_producer(dbeta_producer, lam3.size, dispersion, pm_cfg)
    dbeta, _ = _grid_dbeta(lam1, np.array([lam2]), lam3, dispersion, pm_cfg, producer, 0 if device is None else int(device))
    x, x_label = _wavelength_axis(lam3, return_wavelength_unit)
    y_unit = "1/km" if str(length_unit).strip().lower() == "km" else "1/m"
    ref_line = float(gamma) * float(p0[0] + p0[1])
    if ys == "log" and (not np.nanmin(dbeta) > 0.0 or ref_line <= 0.0):     # all-NaN counts as "not > 0" (upstream: a warning + NaN)
        raise ValueError("yscale='log' requires dBeta and gamma*(P1+P2) to be strictly > 0.")

    def draw(plt):
        fig = plt.figure(figsize=(8.0, 5.0))
        plt.plot(x, dbeta, label=r"$d\beta(\lambda_3)$")
        plt.axhline(ref_line, linestyle="--", label=r"$\gamma(P_1+P_2)$")
        plt.xlabel(x_label)
        plt.ylabel(rf"$d\beta$ [{y_unit}]")
        plt.xscale(xs)
        plt.yscale(ys)
        if title is not None:
            plt.title(title)
        plt.grid(True, which="both", linestyle="--", alpha=0.5)
        plt.legend()
        plt.tight_layout()
        return fig

    _maybe_plot(draw, save_path, show)
    return x, dbeta


def scan_dbeta_seeded_signal(*, cfg: SimulationConfig, delta_beta: Sequence[float], gamma, alpha,
                             p_in: Sequence[float], phase_in: Optional[Sequence[float]] = None,
                             length_unit: str = "m", gain_mode: GainMode = "end", gain_unit: str = "dB",
                             dtype=np.float64, device: Optional[int] = None,
                             devices: Optional[Sequence[int]] = None, with_idler: bool = False) -> dict:
    """Scan the phase mismatch directly (PROVIDED dbeta per point) and summarise the signal gain.

    delta_beta: (N,) in 1/length_unit.  gamma / alpha: scalars or (N,) in per-length_unit.
    Returns dict(delta_beta, gain, best_index, best_delta_beta, best_gain, n_finite, result=SweepResult,
    points_per_s) -- gain with the reference's NaN rules, argmax/max reduced on the GPU.
    with_idler=True also returns, as the reference's seeded scan reports Gi next to Gs (scan_mismtach.py:139-153):
    gain_idler (the idler's metric over the SIGNAL's input power p_in[2], its Gi definition :83, :150), best_gain_idler
    (that gain at best_index) and p_wave_metric (N, n_waves), the gain_mode metric of every wave.
    """
    unit = check_gain(gain_mode, gain_unit)
    db = np.asarray(delta_beta, dtype=float)
    if db.ndim != 1 or db.size == 0:
        raise ValueError("delta_beta must be a non-empty 1D sequence")
    _, p0, ph0 = _check_sweep_inputs([1.0], p_in, phase_in)
    pre = _prepare(cfg, gamma=0.0, alpha=0.0, dispersion=None,
                   phase_matching_cfg=PhaseMatchingConfig(method=PhaseMatchingMethod.PROVIDED, provided_delta_beta=0.0),
                   beta_legacy=None, length_unit=length_unit)
    scale, L, dz_m = pre["scale"], pre["fiber"].length_m, pre["grid"].dz_m
    shard = Share(db.size, device)
    gam, alp = np.asarray(gamma, dtype=float) / scale, np.asarray(alpha, dtype=float) / scale
    for name, v in (("gamma", gam), ("alpha", alp)):
        if v.ndim > 1 or (v.ndim == 1 and v.shape[0] not in (1, db.size)):
            raise ValueError(f"{name} must be a scalar or have one entry per delta_beta point")
    res, _, _ = _run_block(shard, lambda: (None, db[shard.lo:shard.hi] / scale, None, ()), dtype=dtype, devices=devices,
                           z_max=L, n_steps=n_steps_of(L, dz_m), save_every=cfg.save_every, check_nan=bool(cfg.check_nan),
                           gamma=gam, alpha=alp, a0=make_initial_amplitudes(p0, ph0), wave_summary=bool(with_idler))
    gain, bi, bg, nf = res.summary(p0[2], mode=gain_mode, unit=unit, device=shard.device)
    secs = max(res.elapsed_ms, 1e-9) * 1e-3
    out = dict(delta_beta=db, gain=gain, best_index=bi, best_delta_beta=(float(db[bi]) if bi >= 0 else float("nan")),
               best_gain=bg, n_finite=nf, result=res, points_per_s=db.size / secs)
    if with_idler:
        gi = res.summary(p0[2], mode=gain_mode, unit=unit, device=shard.device, wave=3)[0]
        out.update(gain_idler=gi, best_gain_idler=(float(gi[bi]) if bi >= 0 else float("nan")),
                   p_wave_metric=(res.p_wave_max if gain_mode == "max" else res.p_wave_end))
    return out


def seeded_mismatch_scan(gain_mode: GainMode = "end", *, device: Optional[int] = None,
                         devices: Optional[Sequence[int]] = None, verbose: bool = False) -> dict:
    """The scenario hard-coded in the reference's ``scan_mismatch_seeded_signal`` (scan_mismtach.py:43-259), which cannot
    run upstream (it passes ``beta=`` to run_single_simulation): 200 mismatches delta over +-40 1/km put on the idler's
    beta (beta0 = 5.8e9 1/km for every wave), gamma = 10 1/(W km), alpha = 0, p_in = [0.1, 0.1, 1e-5, 0] W, z_max = 0.5 km
    in 1e-3 km steps (scan_mismtach.py:56-93), each point's dbeta formed as run_single_simulation(beta_legacy=betas,
    length_unit="km") forms it.  Gains as the reference defines them (:139-153): Gs = P_s metric / (P_s(z=0) + eps),
    Gi = P_i metric / (p_in[2] + eps), eps = 1e-30; best = argmax Gs (:183-186).

    Returns dict(delta, Gs, Gi, p_wave_metric (200, 4), best_index, best_delta, best_Gs, best_Gi, result=SweepResult);
    with verbose the reference's result block is printed."""
    from .constants import c as c_light
    from .phase_matching import compute_phase_mismatch
    mode = gain_mode
    check_gain(mode)
    cfg = custom_simulation_config(z_max=0.5, dz=1e-3)
    gamma, alpha, P1_total = 10.0, 0.0, 0.1
    p_in = np.array([P1_total, P1_total, 1e-5, 0.0])
    beta0, omega = 5.8e9, np.full(4, c_light / 1.55e-6)
    Ps0_ref = Pi0_ref = float(p_in[2])
    delta = np.linspace(-40.0, 40.0, 200)
    eps = 1e-30
    dbeta_m = np.empty(delta.size)
    for k, d in enumerate(delta):
        pre = _prepare(cfg, gamma=gamma, alpha=alpha, dispersion=None, phase_matching_cfg=None,
                       beta_legacy=beta0 * np.ones(4) + np.array([0.0, 0.0, 0.0, d]), length_unit="km")
        dbeta_m[k] = compute_phase_mismatch(omega, None, pre["pm"].config).delta_beta
    L, dz_m = pre["fiber"].length_m, pre["grid"].dz_m
    shard = Share(delta.size, device)
    a0 = make_initial_amplitudes(p_in, None)
    res, _, _ = _run_block(shard, lambda: (None, dbeta_m[shard.lo:shard.hi], None, ()), devices=devices,
                           z_max=L, n_steps=n_steps_of(L, dz_m), save_every=cfg.save_every, check_nan=bool(cfg.check_nan),
                           gamma=gamma / 1e3, alpha=alpha / 1e3, a0=a0, wave_summary=True)
    metric = res.p_wave_max if mode == "max" else res.p_wave_end
    Ps0 = float(np.abs(a0[2]) ** 2)                # Ps[0]: the saved row at z = 0
    Gs = metric[:, 2] / (Ps0 + eps)
    Gi = metric[:, 3] / (Pi0_ref + eps)
    best_idx = int(np.argmax(Gs))
    out = dict(delta=delta, Gs=Gs, Gi=Gi, p_wave_metric=metric, best_index=best_idx, best_delta=float(delta[best_idx]),
               best_Gs=float(Gs[best_idx]), best_Gi=float(Gi[best_idx]), result=res)
    if verbose:
        label = "P(z_max)" if mode == "end" else "max_z P(z)"
        print("=== Mismatch scan results ===")
        print(f"gamma = {gamma:.6g} 1/(W*km)")
        print(f"Total pump power P1_total = {P1_total:.6g} W  (split: {P1_total/2:.6g} + {P1_total/2:.6g} W)")
        print(f"Seed signal Ps(0) = {Ps0_ref:.6g} W")
        print(f"Seed idler  Pi(0) = {Pi0_ref:.6g} W")
        print(f"Ideal_mismatch_guess = {0.0:.6g} 1/km")
        print(f"Gain metric mode = {mode!r}  -> using {label}")
        print("--- Best point (max signal gain) ---")
        print(f"best_delta = {out['best_delta']:.6g} 1/km")
        print(f"Signal gain Gs = {label}/Ps(0) = {out['best_Gs']:.6g}")
        print(f"Idler  level Gi = {label}/Pi(0) = {out['best_Gi']:.6g}")
    return out


def scan_gain_grid(*, cfg: SimulationConfig, lambda_p1_m: float, lambda_p2_m: Sequence[float],
                   lambda_signal_m: Sequence[float], gamma: float, alpha: float, p_in: Sequence[float],
                   phase_in: Optional[Sequence[float]] = None, dispersion: DispersionParams,
                   phase_matching_cfg: Optional[PhaseMatchingConfig] = None, length_unit: str = "m",
                   gain_unit: str = "dB", gain_mode: GainMode = "max", device: Optional[int] = None,
                   dbeta_producer: str = "auto", devices: Optional[Sequence[int]] = None) -> dict:
    """Signal gain over the grid lambda_p2[Ny] x lambda_signal[Nx]: Ny*Nx independent runs, one kernel launch.
    ``dbeta_producer``: "host" (NumPy), "device" (the grid's phase mismatch computed on the GPU as well: same operations, see
    _grid_dbeta) or "auto" (device for grids of 4 096 points or more).

    Row iy is what ``plot_max_gain_and_dbeta_vs_lambda_signal(lambda_p2_m=lambda_p2[iy], ...)`` returns (same plans, same
    NaN rules; the same dbeta bit for bit when both calls use the same producer -- "auto" decides by the size of the whole
    call, and the two producers differ by a few ulp on ~0.2 % of points).  ``device`` / ``devices``: one GPU,
    or several of this process; under a ``torch.distributed`` process group the ranks split the grid.  Returns dict(gain (Ny, Nx), dbeta (Ny, Nx) in 1/length_unit,
    best_index (iy, ix) | None, best_gain, n_finite, result=SweepResult | None).
    """
    unit = check_gain(gain_mode, gain_unit)
    lam3, p0, ph0 = _check_sweep_inputs(lambda_signal_m, p_in, phase_in)
    lam2 = np.asarray(list(lambda_p2_m), dtype=float)
    if lam2.ndim != 1 or lam2.size == 0 or not np.all(np.isfinite(lam2)) or np.any(lam2 <= 0.0):
        raise ValueError("lambda_p2_m must be a non-empty 1D sequence of finite positive wavelengths (m)")
    if dispersion is None:
        raise ValueError("dispersion must be provided")
    pm_cfg = phase_matching_cfg if phase_matching_cfg is not None else PhaseMatchingConfig()
    gain, dbeta, res = _sweep_gain(cfg=cfg, lam1=float(lambda_p1_m), grid_axes=(lam2, lam3), gamma=gamma, alpha=alpha, p0=p0,
                                   ph0=ph0, dispersion=dispersion, pm_cfg=pm_cfg, length_unit=length_unit, gain_unit=unit,
                                   gain_mode=gain_mode, device=device, devices=devices, dbeta_producer=dbeta_producer,
                                   caller_dbeta=(dispersion, pm_cfg))
    gain = np.where(np.isnan(dbeta), np.nan, gain)
    finite = np.isfinite(gain)
    best = None
    if finite.any():
        flat = int(np.nanargmax(gain))
        best = (flat // lam3.size, flat % lam3.size)
    return dict(gain=gain.reshape(lam2.size, lam3.size), dbeta=dbeta.reshape(lam2.size, lam3.size), best_index=best,
                best_gain=(float(gain.reshape(-1)[best[0] * lam3.size + best[1]]) if best else float("nan")),
                n_finite=int(finite.sum()), result=res)


def scan_six_wave_grid(*, cfg: SimulationConfig, lambda_p1_m: float, lambda_p2_m: float, Omega1: Sequence[float],
                       Omega2: Sequence[float], gamma: float, alpha: float, p_in: Sequence[float],
                       phase_in: Optional[Sequence[float]] = None, dispersion: DispersionParams,
                       even_orders: Tuple[int, ...] = (2, 4), length_unit: str = "m", gain_unit: str = "dB",
                       gain_mode: GainMode = "max", device: Optional[int] = None, dbeta_producer: str = "auto",
                       devices: Optional[Sequence[int]] = None) -> dict:
    """Six waves [p1, p2, s1, i1, s2, i2]: pair k sits at omega_c +- Omega_k (omega_c, omega_d from the two pumps) and
    has dbeta_k = sum_{n even} beta_n (Omega_k^n - omega_d^n) 2/n!  (the symmetric-even form, dispersion.py:321-372).
    Runs the Omega1[Ny] x Omega2[Nx] grid in ONE launch of the 6-wave kernel.

    p_in / phase_in: six entries.  Returns dict(gain (Ny, Nx) of signal 1 -- the kernel's summary wave --, dbeta1 (Ny,),
    dbeta2 (Nx,), a_end (Ny, Nx, 6), first_bad_step (Ny, Nx), result=SweepResult).  The 6-wave model is build-defined:
    with pair 2 dark every row equals the 4-wave run at dbeta1 (tested), beyond that parity is unpinned.
    """
    unit = check_gain(gain_mode, gain_unit)
    p0 = np.asarray(list(p_in), dtype=float)
    if p0.shape != (6,) or not np.all(np.isfinite(p0)) or np.any(p0 < 0.0):
        raise ValueError("p_in must hold six finite non-negative powers [p1, p2, s1, i1, s2, i2]")
    if p0[2] <= 0.0:
        raise ValueError("p_in[2] (signal-1 seed power) must be > 0 to define gain")
    ph = None if phase_in is None else np.asarray(list(phase_in), dtype=float)
    if ph is not None and (ph.shape != (6,) or not np.all(np.isfinite(ph))):
        raise ValueError("phase_in must hold six finite phases")
    O1, O2 = np.asarray(list(Omega1), dtype=float), np.asarray(list(Omega2), dtype=float)
    if O1.ndim != 1 or O2.ndim != 1 or O1.size == 0 or O2.size == 0 or not (np.all(np.isfinite(O1)) and np.all(np.isfinite(O2))):
        raise ValueError("Omega1 and Omega2 must be non-empty 1D sequences of finite detunings (rad/s)")
    if dispersion is None:
        raise ValueError("dispersion must be provided")
    from .frequency_plan import omega_from_lambda
    w1, w2 = omega_from_lambda(lambda_p1_m), omega_from_lambda(lambda_p2_m)
    wc, wd = 0.5 * (w1 + w2), 0.5 * (w1 - w2)
    if np.any(np.abs(O1) >= wc) or np.any(np.abs(O2) >= wc):
        raise ValueError("|Omega| must stay below omega_c (sideband frequencies must be positive)")
    pre = _prepare(cfg, gamma=gamma, alpha=alpha, dispersion=dispersion, phase_matching_cfg=None, beta_legacy=None,
                   length_unit=length_unit)
    disp_m, fiber, grid = pre["fiber"].dispersion, pre["fiber"], pre["grid"]
    db1 = delta_beta_symmetric_array(wd, O1, disp_m, even_orders=even_orders)      # per metre
    db2 = delta_beta_symmetric_array(wd, O2, disp_m, even_orders=even_orders)
    dbeta_producer = _pick_producer(dbeta_producer, O1.size * O2.size, disp_m, None, even_orders=even_orders)
    shard = Share(O1.size * O2.size, device)

    def inputs():
        if dbeta_producer == "device" and shard.hi > shard.lo:   # the block's (dbeta_1, dbeta_2) from psa_dbeta_pairs_f64
            from . import _native
            d1, d2 = _native.dbeta_pairs_host(_native.dbeta_model(disp_m, None, even_orders=even_orders), wd, O1, O2,
                                              first=shard.lo, n_points=shard.hi - shard.lo, device=shard.device)
            return None, d1, d2, ()
        i = np.arange(shard.lo, shard.hi)
        return None, db1[i // O2.size], db2[i % O2.size], ()

    from .sweep import initial_amplitudes
    res, _, _ = _run_block(shard, inputs, n_waves=6, devices=devices, z_max=fiber.length_m, n_steps=n_steps_of(fiber.length_m, grid.dz_m),
                           save_every=cfg.save_every, check_nan=bool(cfg.check_nan), gamma=fiber.gamma_W_m,
                           alpha=fiber.alpha_1_m, a0=initial_amplitudes(p0, ph))
    gain = res.gain(p0[2], mode=gain_mode, unit=unit, device=shard.device)
    shape = (O1.size, O2.size)
    return dict(gain=gain.reshape(shape), dbeta1=db1 * pre["scale"], dbeta2=db2 * pre["scale"],
                a_end=res.a_end.reshape(shape + (6,)), first_bad_step=res.first_bad_step.reshape(shape), result=res)


def _wdm_channels(Omega, p_pump):
    """The channels and the pumps of a multi-channel scan -> (Omega (K,), K, p_pump (2,))."""
    Om = np.asarray(list(Omega), dtype=float)
    if Om.ndim != 1 or not 1 <= Om.size <= 16 or not np.all(np.isfinite(Om)):
        raise ValueError("Omega must be a 1D sequence of 1..16 finite detunings (rad/s)")
    pp = np.asarray(list(p_pump), dtype=float)
    if pp.shape != (2,) or not np.all(np.isfinite(pp)) or np.any(pp < 0.0):
        raise ValueError("p_pump must hold two finite non-negative powers [p1, p2]")
    return Om, int(Om.size), pp


def _wdm_plan(Om, lambda_p1_m, lambda_p2_m, dispersion, pp, ps, pi):
    """The frequency plan of a multi-channel scan, once its powers stand -> (omega_d, the powers [p1, p2, s_1, i_1, ...] of
    ps's leading shape): a dispersion, the pumps at omega_c +- omega_d, every sideband omega_c +- Omega_k positive."""
    from .frequency_plan import omega_from_lambda
    if dispersion is None:
        raise ValueError("dispersion must be provided")
    w1, w2 = omega_from_lambda(lambda_p1_m), omega_from_lambda(lambda_p2_m)
    wc, wd = 0.5 * (w1 + w2), 0.5 * (w1 - w2)
    if np.any(np.abs(Om) >= wc):
        raise ValueError("|Omega| must stay below omega_c (sideband frequencies must be positive)")
    p_all = np.empty(ps.shape[:-1] + (2 + 2 * Om.size,))
    p_all[..., :2], p_all[..., 2::2], p_all[..., 3::2] = pp, ps, np.broadcast_to(pi, ps.shape)
    return wd, p_all


def scan_wdm_gain(*, cfg: SimulationConfig, lambda_p1_m: float, lambda_p2_m: float, Omega: Sequence[float],
                  p_pump: Sequence[float], p_signal, p_idler=0.0, phase_in: Optional[Sequence[float]] = None, gamma: float,
                  alpha: float, dispersion: DispersionParams, even_orders: Tuple[int, ...] = (2, 4), length_unit: str = "m",
                  gain_unit: str = "dB", gain_mode: GainMode = "max", device: Optional[int] = None,
                  devices: Optional[Sequence[int]] = None) -> dict:
    """A dual-pump amplifier carrying K = 1..16 channels at once (no reference counterpart): waves
    [p1, p2, s_1, i_1, ..., s_K, i_K], channel k at omega_c +- Omega_k with dbeta_k = delta_beta_symmetric(omega_d, Omega_k)
    as scan_six_wave_grid computes its two.  All channels draw on the same two pumps and shift each other's phase matching
    through XPM; FWM products between channels (signal-signal mixing) are not modelled here (scan_comb_gain models them on
    a uniform frequency grid).

    The N sweep points are input-power settings: p_signal (K,) is one point, (N, K) is N of them; p_idler a scalar, (K,)
    or (N, K); p_pump (2,); phase_in None or NW = 2 + 2K phases.  One launch of the multi-channel kernel
    (sweep.rk4_sweep_pairs) on ``device``, or split over ``devices``; sharding over a ``torch.distributed`` process group
    is out of scope here -- every rank would run the whole sweep.

    Returns dict(gain (N, K) of every signal over its seed, idler (N, K) every idler's power over its signal's seed,
    pump_depletion (N,), dbeta (K,) in 1/length_unit, first_bad_step (N,), result=PairsResult)."""
    from .sweep import initial_amplitudes, rk4_sweep_pairs
    unit = check_gain(gain_mode, gain_unit)
    Om, K, pp = _wdm_channels(Omega, p_pump)
    ps = np.asarray(p_signal, dtype=float)
    if ps.ndim not in (1, 2) or ps.shape[-1] != K or ps.size == 0:
        raise ValueError(f"p_signal must have shape ({K},) or (N, {K})")
    ps = np.atleast_2d(ps)
    if not np.all(np.isfinite(ps)) or np.any(ps <= 0.0):
        raise ValueError("p_signal (the seed powers) must be finite and > 0 to define gain")
    N = int(ps.shape[0])
    pi = np.asarray(p_idler, dtype=float)
    if pi.shape not in ((), (K,), (N, K)) or not np.all(np.isfinite(pi)) or np.any(pi < 0.0):
        raise ValueError(f"p_idler must be a scalar, ({K},) or ({N}, {K}) of finite non-negative powers")
    ph = None if phase_in is None else np.asarray(list(phase_in), dtype=float)
    if ph is not None and (ph.shape != (2 + 2 * K,) or not np.all(np.isfinite(ph))):
        raise ValueError(f"phase_in must hold {2 + 2 * K} finite phases")
    wd, p_all = _wdm_plan(Om, lambda_p1_m, lambda_p2_m, dispersion, pp, ps, pi)
    pre = _prepare(cfg, gamma=gamma, alpha=alpha, dispersion=dispersion, phase_matching_cfg=None, beta_legacy=None,
                   length_unit=length_unit)
    fiber, grid = pre["fiber"], pre["grid"]
    db = delta_beta_symmetric_array(wd, Om, fiber.dispersion, even_orders=even_orders)      # per metre
    res = rk4_sweep_pairs(np.broadcast_to(db, (N, K)), z_max=fiber.length_m, n_steps=n_steps_of(fiber.length_m, grid.dz_m),
                          save_every=cfg.save_every, check_nan=bool(cfg.check_nan), gamma=fiber.gamma_W_m,
                          alpha=fiber.alpha_1_m, a0=initial_amplitudes(p_all, ph), device=(0 if device is None else int(device)),
                          devices=devices)
    return dict(gain=res.channel_gain(ps, mode=gain_mode, unit=unit), idler=res.idler_conversion(ps, mode=gain_mode, unit=unit),
                pump_depletion=res.pump_depletion(), dbeta=db * pre["scale"], first_bad_step=res.first_bad_step, result=res)


def scan_single_pump_gain(*, cfg: SimulationConfig, lambda_pump_m: float, lambda_signal_m: Sequence[float], p_pump: float,
                          p_signal: float, p_idler: float = 0.0, phase_in: Optional[Sequence[float]] = None, gamma: float,
                          alpha: float, dispersion: DispersionParams, max_order: int = 4, length_unit: str = "m",
                          gain_unit: str = "dB", gain_mode: GainMode = "max", device: Optional[int] = None,
                          devices: Optional[Sequence[int]] = None, dtype=np.float64) -> dict:
    """The gain spectrum of a single-pump amplifier (no reference counterpart): waves [p, s, i], the pump at lambda_pump_m,
    sweep point k with its signal at lambda_signal_m[k] and its idler at 2 w_p - w_s, dbeta = beta(w_s) + beta(w_i) -
    2 beta(w_p) from the Taylor expansion of ``dispersion`` up to ``max_order``, formed on the host.  One launch of the
    single-pump kernel (sweep.rk4_sweep_single_pump) over the signal wavelengths on ``device``, or split over ``devices``;
    sharding over a ``torch.distributed`` process group is out of scope here -- every rank would run the whole sweep.
    A point whose plan is invalid (a wavelength that is not positive and finite, an idler frequency <= 0, a non-finite
    dbeta) gets NaN in every output instead of an exception.  ``dtype=np.float32`` runs the packed float32 kernel; dbeta is
    still formed in float64 on the host and rounded once.

    Returns dict(gain (n,) of the signal over p_signal, idler (n,) the idler's power over p_signal, pump_depletion (n,),
    dbeta (n,) in 1/length_unit, first_bad_step (n,), result=SinglePumpResult)."""
    from .frequency_plan import omega_from_lambda, omega_from_lambda_array
    from .simulation import _single_pump_mismatch
    from .sweep import initial_amplitudes, rk4_sweep_single_pump
    unit = check_gain(gain_mode, gain_unit)
    lam = np.asarray(lambda_signal_m, dtype=float)
    if lam.ndim != 1 or lam.size == 0:
        raise ValueError("lambda_signal_m must be a non-empty 1D sequence")
    p0 = np.array([p_pump, p_signal, p_idler], dtype=float)
    if not np.all(np.isfinite(p0)) or np.any(p0 < 0.0):
        raise ValueError("p_pump, p_signal and p_idler must be finite non-negative powers")
    if not p0[1] > 0.0:
        raise ValueError("p_signal (the seed power) must be > 0 to define gain")
    ph = None if phase_in is None else np.asarray(list(phase_in), dtype=float)
    if ph is not None and (ph.shape != (3,) or not np.all(np.isfinite(ph))):
        raise ValueError("phase_in must hold 3 finite phases")
    if dispersion is None:
        raise ValueError("dispersion must be provided")
    if not isinstance(max_order, int) or max_order < 0:
        raise ValueError("max_order must be a non-negative int")
    wp = omega_from_lambda(lambda_pump_m)
    pre = _prepare(cfg, gamma=gamma, alpha=alpha, dispersion=dispersion, phase_matching_cfg=None, beta_legacy=None,
                   length_unit=length_unit)
    fiber, grid = pre["fiber"], pre["grid"]
    with np.errstate(all="ignore"):
        ok = np.isfinite(lam) & (lam > 0.0)
        ws = omega_from_lambda_array(np.where(ok, lam, 1.0))
        wi = 2.0 * wp - ws
        ok &= np.isfinite(ws) & (wi > 0.0)
        db = _single_pump_mismatch(wp, np.where(ok, ws, wp), np.where(ok, wi, wp), fiber.dispersion, max_order)   # per metre
        ok &= np.isfinite(db)
    res = rk4_sweep_single_pump(np.where(ok, db, 0.0), z_max=fiber.length_m, n_steps=n_steps_of(fiber.length_m, grid.dz_m),
                                save_every=cfg.save_every, check_nan=bool(cfg.check_nan), gamma=fiber.gamma_W_m,
                                alpha=fiber.alpha_1_m, a0=initial_amplitudes(p0, ph), device=(0 if device is None else int(device)),
                                devices=devices, dtype=dtype)
    nan = lambda x: np.where(ok, x, np.nan)   # noqa: E731
    return dict(gain=nan(res.signal_gain(p0[1], mode=gain_mode, unit=unit)),
                idler=nan(res.idler_conversion(p0[1], mode=gain_mode, unit=unit)), pump_depletion=nan(res.pump_depletion()),
                dbeta=nan(db) * pre["scale"], first_bad_step=res.first_bad_step, result=res)


def scan_comb_gain(*, cfg: SimulationConfig, lambda_center_m: float, line_spacing: float, p_lines,
                   phase_in: Optional[Sequence[float]] = None, gamma: float, alpha: float, dispersion: DispersionParams,
                   max_order: int = 4, length_unit: str = "m", gain_unit: str = "dB", gain_mode: GainMode = "max",
                   device: Optional[int] = None, devices: Optional[Sequence[int]] = None, dtype=np.float64) -> dict:
    """A multi-line ("comb") parametric amplifier (no reference counterpart): M = 3..12 lines at omega_c + (m - (M-1)/2) *
    line_spacing (rad/s), omega_c from lambda_center_m, ascending in frequency, coupled by EVERY four-wave-mixing product
    that falls on the grid: inter-channel crosstalk, the cascaded pump products at 2 w_1 - w_2 and 2 w_2 - w_1, higher-order
    idlers.  b_m is the Taylor sum of ``dispersion`` over the orders 2..max_order at line m and kappa_m = b_m - [b_0 +
    (b_{M-1} - b_0) * m / (M-1)] (simulation.comb_lines): the large beta_1 phase never reaches a sincos.

    The N sweep points are input-power settings: p_lines (M,) is one point, (N, M) is N of them (a dark line is 0 W);
    phase_in None or M phases.  One launch of the multi-line kernel (sweep.rk4_sweep_comb) on ``device``, or split over
    ``devices``; sharding over a ``torch.distributed`` process group is out of scope here -- every rank would run the whole
    sweep -- and so are RK45 and non-uniform grids; the copier - PSA link is scan_comb_copier_psa_phase (float64).
    ``dtype=np.float32`` runs the packed float32 kernel (sweep.rk4_sweep_comb has from what N it pays): kappa is still formed
    in float64 here, in the gauge kappa_0 = kappa_{M-1} = 0 that keeps |kappa| smallest, and rounded once; the outputs come back
    in float32.  Any other dtype is a ValueError.

    Returns dict(gain (N, M) of every line over its input power -- NaN for a line with zero input --, p_end, p_max (N, M),
    kappa (M,) in 1/length_unit, omega (M,), first_bad_step (N,), result=CombResult)."""
    from .frequency_plan import omega_from_lambda
    from .simulation import _comb_input, comb_lines
    from .sweep import rk4_sweep_comb
    unit = check_gain(gain_mode, gain_unit)
    if np.dtype(dtype) not in (np.dtype(np.float64), np.dtype(np.float32)):
        raise ValueError(f"dtype must be float64 or float32, got {np.dtype(dtype)}")
    p, a0 = _comb_input(p_lines, "p_lines", phase_in, points=True)
    N, M = (int(x) for x in p.shape)
    if dispersion is None:
        raise ValueError("dispersion must be provided")
    pre = _prepare(cfg, gamma=gamma, alpha=alpha, dispersion=dispersion, phase_matching_cfg=None, beta_legacy=None,
                   length_unit=length_unit)
    fiber, grid = pre["fiber"], pre["grid"]
    omega, kappa, _ = comb_lines(omega_from_lambda(lambda_center_m), line_spacing, M, fiber.dispersion, max_order=max_order)
    res = rk4_sweep_comb(np.broadcast_to(kappa, (N, M)), z_max=fiber.length_m, n_steps=n_steps_of(fiber.length_m, grid.dz_m),
                         save_every=cfg.save_every, check_nan=bool(cfg.check_nan), gamma=fiber.gamma_W_m, alpha=fiber.alpha_1_m,
                         a0=a0, device=(0 if device is None else int(device)), devices=devices, dtype=dtype)
    return dict(gain=res.line_gain(p, mode=gain_mode, unit=unit), p_end=res.p_wave_end, p_max=res.p_wave_max,
                kappa=kappa * pre["scale"], omega=omega, first_bad_step=res.first_bad_step, result=res)


def _phase_scan_axes(phase, psa_delta_beta):
    """The rules the copier - PSA scans share for their axes -> (phase (K,), psa_delta_beta () or (M,))."""
    ph = np.linspace(0.0, 2.0 * np.pi, 32, endpoint=False) if phase is None else np.asarray(phase, dtype=float)
    if ph.ndim != 1 or ph.size == 0 or not np.all(np.isfinite(ph)):
        raise ValueError("phase must be a non-empty 1D sequence of finite values")
    dbp = np.asarray(psa_delta_beta, dtype=float)
    if dbp.ndim > 1 or dbp.size == 0 or not np.all(np.isfinite(dbp)):
        raise ValueError("psa_delta_beta must be a finite scalar or a non-empty 1D sequence")
    return ph, dbp


def _copier_psa_link(chain, transfer_of, a_in, gain_db_of, *, psa_cfg, copier_cfg, gamma, alpha, copier_gamma, copier_alpha,
                     psa_x, copier_x, length_unit, device, devices, mismatch_of=None, **chain_kw):
    """The copier - mid-stage - PSA link under the four scan_*_copier_psa_phase functions -> (the chain's result, what
    ``mismatch_of`` kept of every span, gain_db, its extremes as the scans return them).

    The spans are the PSA's (psa_cfg, gamma, alpha, psa_x) and, with a copier_cfg, the copier's in front, whose gamma and alpha
    default to the PSA's; the two configs share save_every and check_nan.  ``mismatch_of(x, prepared)`` -> (the span's
    per-metre mismatch as FibreSpan takes it, something to keep) forms it from the span's dispersion x, scaled by _prepare.
    Without it x is the mismatch itself in 1/length_unit, psa_x per point and copier_x a scalar (the 4-wave and single-pump
    scans): a span is then prepared without gamma, alpha or a dispersion, so none of FiberParams' rules applies to them, and
    the configs are compared after the spans are prepared, not before -- the order those two scans always had.
    ``transfer_of()`` is the mid-stage (points, n_waves) with the scanned phase in it; without a copier it acts on the input
    ``a_in``.  One call of ``chain`` (the family's rk4_chain_*), then ``gain_db_of(result)``: (points,) has its extremes taken
    over all points, as floats, (points, columns) per column; NaN where no gain is finite."""
    from .sweep import FibreSpan
    provided = mismatch_of is None
    fibres = [(psa_cfg, gamma, alpha, psa_x)]
    if copier_cfg is not None:
        fibres.insert(0, (copier_cfg, gamma if copier_gamma is None else copier_gamma,
                          alpha if copier_alpha is None else copier_alpha, copier_x))

    def shared():
        if any(int(c.save_every) != int(psa_cfg.save_every) or bool(c.check_nan) != bool(psa_cfg.check_nan) for c, *_ in fibres):
            raise ValueError("copier_cfg and psa_cfg must share save_every and check_nan")

    if not provided:
        shared()
    pres, mismatches, kept = [], [], []
    for cfg, g, a, x in fibres:
        if provided:
            pre = _prepare(cfg, gamma=0.0, alpha=0.0, dispersion=None, phase_matching_cfg=_PROVIDED, beta_legacy=None,
                           length_unit=length_unit)
            m, keep = (x if x is psa_x else float(x)) / pre["scale"], None
        else:
            pre = _prepare(cfg, gamma=g, alpha=a, dispersion=x, phase_matching_cfg=None, beta_legacy=None, length_unit=length_unit)
            m, keep = mismatch_of(x, pre)
        pres.append(pre), mismatches.append(m), kept.append(keep)
    if provided:
        shared()
    T = transfer_of()
    spans = [FibreSpan(pre["fiber"].length_m, dz=pre["grid"].dz_m, dbeta=m, gamma=float(g) / pre["scale"],
                       alpha=float(a) / pre["scale"]) for (_, g, a, _), pre, m in zip(fibres, pres, mismatches)]
    a0, transfers = (T * a_in[None, :], None) if copier_cfg is None else (a_in, [T])
    res = chain(spans, a0=a0, transfers=transfers, save_every=int(psa_cfg.save_every), check_nan=bool(psa_cfg.check_nan),
                device=(0 if device is None else int(device)), devices=devices, **chain_kw)
    gain_db = gain_db_of(res)
    with np.errstate(all="ignore"):
        finite = np.isfinite(gain_db)
        some = finite.any(axis=0)
        gmax = np.where(some, np.max(np.where(finite, gain_db, -np.inf), axis=0), np.nan)
        gmin = np.where(some, np.min(np.where(finite, gain_db, np.inf), axis=0), np.nan)
    if gain_db.ndim == 1:
        gmax, gmin = float(gmax), float(gmin)
    return res, kept, gain_db, dict(gain_max_db=gmax, gain_min_db=gmin, extinction_db=gmax - gmin)


def scan_copier_psa_phase(*, psa_cfg: SimulationConfig, psa_delta_beta, gamma: float, alpha: float, p_in: Sequence[float],
                          phase_in: Optional[Sequence[float]] = None, copier_cfg: Optional[SimulationConfig] = None,
                          copier_delta_beta: float = 0.0, copier_gamma: Optional[float] = None,
                          copier_alpha: Optional[float] = None, mid_gain_db: Sequence[float] = (0.0, 0.0, 0.0, 0.0),
                          mid_phase: Sequence[float] = (0.0, 0.0, 0.0, 0.0), phase: Optional[Sequence[float]] = None,
                          phase_wave="pumps", length_unit: str = "m", gain_mode: GainMode = "max",
                          gain_unit: str = "dB", dtype=np.float64, device: Optional[int] = None,
                          devices: Optional[Sequence[int]] = None) -> dict:
    """Signal gain of a copier - mid-stage - PSA chain against the mid-stage phase (no reference counterpart).

    An optional copier span (``copier_cfg``: length, dz; its own dbeta, gamma, alpha -- gamma / alpha default to the PSA
    span's) makes the phase-conjugated idler; the mid-stage applies ``mid_gain_db`` / ``mid_phase`` per wave plus the
    scanned ``phase`` (K values, default 32 over [0, 2 pi)) on ``phase_wave`` -- "pumps" (both pumps) or a wave index
    0..3; the PSA span (``psa_cfg``) then amplifies phase-sensitively.  ``psa_delta_beta`` a scalar or M values: the scan
    runs K x M chains in ONE launch per span with per-point transfers.  Without a copier the mid-stage acts on the input.
    dbeta in 1/length_unit, gamma / alpha per length_unit; save_every and check_nan come from psa_cfg (the copier's must
    agree, and every span's step count must be a multiple of save_every).

    gain: (K,) or (K, M), the signal's gain_mode metric over every saved row of the chain over p_in[2], with the drivers'
    NaN rules (a point that went non-finite is NaN, scan_mismtach.py:391-392).  Returns dict(phase, psa_delta_beta, gain,
    gain_max_db, gain_min_db, extinction_db (max - min over the finite gains, dB), result=ChainResult)."""
    from .simulation import mid_stage
    from .sweep import rk4_chain
    unit = check_gain(gain_mode, gain_unit)
    ph, dbp = _phase_scan_axes(phase, psa_delta_beta)
    if phase_wave == "pumps":
        mask = np.array([1.0, 1.0, 0.0, 0.0])
    elif isinstance(phase_wave, (int, np.integer)) and 0 <= int(phase_wave) < 4:
        mask = np.eye(4)[int(phase_wave)]
    else:
        raise ValueError("phase_wave must be 'pumps' or a wave index 0..3")
    _, p0, ph0 = _check_sweep_inputs([1.0], p_in, phase_in)
    M = max(dbp.size, 1)                  # point k * M + m: phase k, mismatch m
    res, _, gain_db, extremes = _copier_psa_link(
        rk4_chain,
        lambda: np.repeat(mid_stage(np.broadcast_to(np.asarray(mid_gain_db, dtype=float), (4,)),
                                    np.asarray(mid_phase, dtype=float)[None, :] + ph[:, None] * mask[None, :]), M, axis=0),
        make_initial_amplitudes(p0, ph0),
        lambda r: r.gain(p0[2], mode=gain_mode, unit="dB",
                         device=(int(devices[0]) if devices else 0 if device is None else int(device))),
        psa_cfg=psa_cfg, copier_cfg=copier_cfg, gamma=gamma, alpha=alpha, copier_gamma=copier_gamma, copier_alpha=copier_alpha,
        psa_x=np.tile(np.atleast_1d(dbp), ph.size), copier_x=copier_delta_beta, length_unit=length_unit, device=device,
        devices=devices, dtype=dtype)
    shape = (ph.size,) + dbp.shape
    return dict(phase=ph, psa_delta_beta=dbp, gain=(gain_db if unit == "db" else 10.0 ** (gain_db / 10.0)).reshape(shape),
                **extremes, result=res)


def scan_single_pump_copier_psa_phase(*, psa_cfg: SimulationConfig, psa_delta_beta, gamma: float, alpha: float,
                                      p_in: Sequence[float], phase_in: Optional[Sequence[float]] = None,
                                      copier_cfg: Optional[SimulationConfig] = None, copier_delta_beta: float = 0.0,
                                      copier_gamma: Optional[float] = None, copier_alpha: Optional[float] = None,
                                      mid_gain_db: Sequence[float] = (0.0, 0.0, 0.0),
                                      mid_phase: Sequence[float] = (0.0, 0.0, 0.0), phase: Optional[Sequence[float]] = None,
                                      phase_wave="pump", length_unit: str = "m", gain_mode: GainMode = "max",
                                      gain_unit: str = "dB", device: Optional[int] = None,
                                      devices: Optional[Sequence[int]] = None) -> dict:
    """scan_copier_psa_phase for the single-pump model, waves [p, s, i] (no reference counterpart): the
    signal and idler gain of a copier - mid-stage - PSA chain on one pump against the mid-stage phase.

    An optional copier span (``copier_cfg``: length, dz; its own dbeta, gamma, alpha -- gamma / alpha default to the PSA
    span's) makes the phase-conjugated idler; the mid-stage applies ``mid_gain_db`` / ``mid_phase`` per wave plus the
    scanned ``phase`` (K values, default 32 over [0, 2 pi)) on ``phase_wave`` -- "pump" or a wave index 0..2; the PSA span
    (``psa_cfg``) then amplifies phase-sensitively.  ``psa_delta_beta`` a scalar or M values: the scan runs K x M chains in
    ONE launch per span with per-point transfers.  Without a copier the mid-stage acts on the input.  dbeta in
    1/length_unit, gamma / alpha per length_unit; save_every and check_nan come from psa_cfg (the copier's must agree, and
    every span's step count must be a multiple of save_every).  Sharding over a process group is out of scope here.

    gain / gain_idler: (K,) or (K, M), the signal's / the idler's gain_mode metric over every saved row of the chain over
    p_in[1], with the drivers' NaN rule for every point with first_bad_step >= 0.  Returns dict(phase, psa_delta_beta, gain,
    gain_idler, gain_max_db, gain_min_db, extinction_db (max - min over the signal's finite gains, dB),
    result=SinglePumpChainResult)."""
    from .simulation import single_pump_mid_stage
    from .sweep import initial_amplitudes, rk4_chain_single_pump
    unit = check_gain(gain_mode, gain_unit)
    ph, dbp = _phase_scan_axes(phase, psa_delta_beta)
    if isinstance(phase_wave, str) and phase_wave == "pump":
        mask = np.eye(3)[0]
    elif isinstance(phase_wave, (int, np.integer)) and not isinstance(phase_wave, bool) and 0 <= int(phase_wave) < 3:
        mask = np.eye(3)[int(phase_wave)]
    else:
        raise ValueError("phase_wave must be 'pump' or a wave index 0..2")
    p0 = np.asarray(list(p_in), dtype=float)
    if p0.shape != (3,) or not np.all(np.isfinite(p0)) or np.any(p0 < 0.0):
        raise ValueError("p_in must hold 3 finite non-negative powers [pump, signal, idler]")
    if not p0[1] > 0.0:
        raise ValueError("p_in[1] (signal seed) must be > 0 to define gain")
    ph0 = None if phase_in is None else np.asarray(list(phase_in), dtype=float)
    if ph0 is not None and (ph0.shape != (3,) or not np.all(np.isfinite(ph0))):
        raise ValueError("phase_in must hold 3 finite phases")
    M = max(dbp.size, 1)                  # point k * M + m: phase k, mismatch m
    res, _, _, extremes = _copier_psa_link(
        rk4_chain_single_pump,
        lambda: np.repeat(single_pump_mid_stage(np.broadcast_to(np.asarray(mid_gain_db, dtype=float), (3,)),
                                                np.broadcast_to(np.asarray(mid_phase, dtype=float), (3,))[None, :]
                                                + ph[:, None] * mask[None, :]), M, axis=0),
        initial_amplitudes(p0, ph0), lambda r: r.signal_gain(p0[1], mode=gain_mode, unit="dB"),
        psa_cfg=psa_cfg, copier_cfg=copier_cfg, gamma=gamma, alpha=alpha, copier_gamma=copier_gamma, copier_alpha=copier_alpha,
        psa_x=np.tile(np.atleast_1d(dbp), ph.size), copier_x=copier_delta_beta, length_unit=length_unit, device=device,
        devices=devices)
    shape = (ph.size,) + dbp.shape
    return dict(phase=ph, psa_delta_beta=dbp, gain=np.asarray(res.signal_gain(p0[1], mode=gain_mode, unit=unit)).reshape(shape),
                gain_idler=np.asarray(res.idler_conversion(p0[1], mode=gain_mode, unit=unit)).reshape(shape), **extremes,
                result=res)


def scan_wdm_copier_psa_phase(*, psa_cfg: SimulationConfig, copier_cfg: Optional[SimulationConfig] = None, lambda_p1_m: float,
                              lambda_p2_m: float, Omega: Sequence[float], p_pump: Sequence[float], p_signal, p_idler=0.0,
                              gamma: float, alpha: float, dispersion: DispersionParams,
                              copier_dispersion: Optional[DispersionParams] = None, copier_gamma: Optional[float] = None,
                              copier_alpha: Optional[float] = None, mid_gain_db=0.0, mid_phase=0.0,
                              phase: Optional[Sequence[float]] = None, phase_wave: str = "pumps",
                              even_orders: Tuple[int, ...] = (2, 4), length_unit: str = "m", gain_mode: GainMode = "max",
                              gain_unit: str = "dB", device: Optional[int] = None,
                              devices: Optional[Sequence[int]] = None) -> dict:
    """scan_copier_psa_phase for the multi-channel model (no reference counterpart): the gain of every
    channel of a WDM copier - mid-stage - PSA link on two pumps against the mid-stage phase.  Waves
    [p1, p2, s_1, i_1, ..., s_K, i_K], channel k at omega_c +- Omega_k; per span dbeta_k = delta_beta_symmetric(omega_d,
    Omega_k) from that span's dispersion, as scan_wdm_gain forms it.  The channels couple through pump depletion and
    SPM/XPM; signal-signal FWM is not modelled.

    An optional copier span (``copier_cfg``: length, dz; ``copier_dispersion`` / ``copier_gamma`` / ``copier_alpha`` default
    to the PSA span's) generates the K idlers; the mid-stage applies ``mid_gain_db`` / ``mid_phase`` (a scalar or NW = 2 + 2K
    values) plus the scanned ``phase`` (F values, default 32 over [0, 2 pi)) on ``phase_wave`` -- "pumps", "signals" or
    "idlers"; the PSA span (``psa_cfg``) then amplifies all channels phase-sensitively from the same two pumps.  The F
    phase points are the sweep points: ONE launch per span (sweep.rk4_chain_pairs) with per-point transfers, on ``device``
    or split over ``devices``.  Without a copier the mid-stage acts on the input.  p_pump (2,), p_signal (K,) > 0, p_idler a
    scalar or (K,); gamma / alpha per length_unit; save_every and check_nan come from psa_cfg (the copier's must agree, and
    every span's step count must be a multiple of save_every).  Sharding over a process group is out of scope here.

    Returns dict(phase (F,), gain (F, K) of every signal over its seed, idler (F, K) every idler's power over its signal's
    seed, gain_max_db, gain_min_db, extinction_db (K,): per channel over the finite gains, dbeta (S, K) in 1/length_unit,
    first_bad_step (F,), result=PairsChainResult)."""
    from .simulation import wdm_mid_stage
    from .sweep import initial_amplitudes, rk4_chain_pairs
    unit = check_gain(gain_mode, gain_unit)
    ph, _ = _phase_scan_axes(phase, 0.0)
    Om, K, pp = _wdm_channels(Omega, p_pump)
    nw = 2 + 2 * K
    ps = np.asarray(p_signal, dtype=float)
    if ps.shape != (K,) or not np.all(np.isfinite(ps)) or np.any(ps <= 0.0):
        raise ValueError(f"p_signal (the seed powers) must have shape ({K},), finite and > 0 to define gain")
    pi = np.asarray(p_idler, dtype=float)
    if pi.shape not in ((), (K,)) or not np.all(np.isfinite(pi)) or np.any(pi < 0.0):
        raise ValueError(f"p_idler must be a scalar or ({K},) of finite non-negative powers")
    masks = {"pumps": (slice(0, 2),), "signals": (slice(2, None, 2),), "idlers": (slice(3, None, 2),)}
    if not isinstance(phase_wave, str) or phase_wave not in masks:
        raise ValueError("phase_wave must be 'pumps', 'signals' or 'idlers'")
    mask = np.zeros(nw)
    mask[masks[phase_wave]] = 1.0
    mg, mp = np.asarray(mid_gain_db, dtype=float), np.asarray(mid_phase, dtype=float)
    if mg.shape not in ((), (nw,)) or mp.shape not in ((), (nw,)):
        raise ValueError(f"mid_gain_db and mid_phase must be a scalar or hold {nw} values")
    wd, p_all = _wdm_plan(Om, lambda_p1_m, lambda_p2_m, dispersion, pp, ps, pi)

    def mismatch_of(d, pre):     # per point: the F phase points are the sweep points, and a chain counts them in the spans and a0
        db = delta_beta_symmetric_array(wd, Om, pre["fiber"].dispersion, even_orders=even_orders)      # per metre
        return np.broadcast_to(db, (ph.size, K)), db * pre["scale"]

    res, dbs, gain_db, extremes = _copier_psa_link(
        rk4_chain_pairs, lambda: wdm_mid_stage(np.broadcast_to(mg, (nw,)), np.broadcast_to(mp, (nw,))[None, :]
                                               + ph[:, None] * mask[None, :]),       # (F, NW)
        initial_amplitudes(p_all), lambda r: r.channel_gain(ps, mode=gain_mode, unit="dB"), mismatch_of=mismatch_of,
        psa_cfg=psa_cfg, copier_cfg=copier_cfg, gamma=gamma, alpha=alpha, copier_gamma=copier_gamma, copier_alpha=copier_alpha,
        psa_x=dispersion, copier_x=dispersion if copier_dispersion is None else copier_dispersion, length_unit=length_unit,
        device=device, devices=devices)
    return dict(phase=ph, gain=gain_db if unit == "db" else res.channel_gain(ps, mode=gain_mode, unit=unit),
                idler=res.idler_conversion(ps, mode=gain_mode, unit=unit), **extremes, dbeta=np.stack(dbs),
                first_bad_step=res.first_bad_step, result=res)


def scan_comb_copier_psa_phase(*, psa_cfg: SimulationConfig, copier_cfg: Optional[SimulationConfig] = None, lambda_center_m: float,
                               line_spacing: float, p_lines, phase_in: Optional[Sequence[float]] = None, gamma: float,
                               alpha: float, dispersion: DispersionParams, copier_dispersion: Optional[DispersionParams] = None,
                               copier_gamma: Optional[float] = None, copier_alpha: Optional[float] = None, mid_gain_db=0.0,
                               mid_phase=0.0, phase: Optional[Sequence[float]] = None, phase_lines: Sequence[int] = (),
                               max_order: int = 4, length_unit: str = "m", gain_mode: GainMode = "max", gain_unit: str = "dB",
                               device: Optional[int] = None, devices: Optional[Sequence[int]] = None) -> dict:
    """scan_copier_psa_phase for the multi-line ("comb") model (no reference counterpart): the gain of every
    line of a copier - mid-stage - PSA link against the mid-stage phase, with EVERY four-wave-mixing product on the grid --
    what scan_wdm_copier_psa_phase leaves out: signal-signal crosstalk, the cascaded pump products, higher-order idlers.
    M = 3..12 lines at omega_c + (m - (M-1)/2) * line_spacing (rad/s), omega_c from lambda_center_m, ascending in frequency;
    per span kappa_m comes from simulation.comb_lines on that span's dispersion, as scan_comb_gain forms it.

    An optional copier span (``copier_cfg``: length, dz; ``copier_dispersion`` / ``copier_gamma`` / ``copier_alpha`` default
    to the PSA span's) generates the idlers; the mid-stage applies ``mid_gain_db`` / ``mid_phase`` (a scalar or M values) plus
    the scanned ``phase`` (F values, default 32 over [0, 2 pi)) on the lines ``phase_lines`` (distinct indices 0..M-1, at
    least one: the pumps, say); the PSA span (``psa_cfg``) then amplifies phase-sensitively.  The F phase points are the
    sweep points: ONE launch per span (sweep.rk4_chain_comb) with a per-point transfer, on ``device`` or split over
    ``devices``.  Without a copier the mid-stage acts on the input.  p_lines (M,) in W, a dark line is 0; phase_in None or M
    phases; gamma / alpha per length_unit; save_every and check_nan come from psa_cfg (the copier's must agree, and every
    span's step count must be a multiple of save_every).  Sharding over a process group is out of scope here.

    Returns dict(phase (F,), gain (F, M) of every line over its input power -- NaN for a line with zero input, as
    CombResult.line_gain --, p_out (F, M) the lines' powers at the end of the link, gain_max_db, gain_min_db, extinction_db
    (M,): per line over the finite gains, kappa (S, M) in 1/length_unit, omega (M,), first_bad_step (F,),
    result=CombChainResult)."""
    from .frequency_plan import omega_from_lambda
    from .simulation import _comb_input, comb_lines, comb_mid_stage
    from .sweep import rk4_chain_comb
    unit = check_gain(gain_mode, gain_unit)
    ph, _ = _phase_scan_axes(phase, 0.0)
    p, a_in = _comb_input(p_lines, "p_lines", phase_in)
    M = int(p.shape[0])
    try:
        lines = list(phase_lines)
    except TypeError:
        lines = []
    if not lines or not all(isinstance(m, (int, np.integer)) and not isinstance(m, bool) and 0 <= m < M for m in lines) \
            or len(set(int(m) for m in lines)) != len(lines):
        raise ValueError(f"phase_lines must name at least one of the lines 0..{M - 1}, each once")
    mask = np.zeros(M)
    mask[lines] = 1.0
    mg, mp = np.asarray(mid_gain_db, dtype=float), np.asarray(mid_phase, dtype=float)
    if mg.shape not in ((), (M,)) or mp.shape not in ((), (M,)):
        raise ValueError(f"mid_gain_db and mid_phase must be a scalar or hold {M} values")
    if dispersion is None:
        raise ValueError("dispersion must be provided")
    wc = omega_from_lambda(lambda_center_m)

    def mismatch_of(d, pre):     # per point: the F phase points are the sweep points, and a chain counts them in the spans and a0
        omega, kappa, _ = comb_lines(wc, line_spacing, M, pre["fiber"].dispersion, max_order=max_order)      # per metre
        return np.broadcast_to(kappa, (ph.size, M)), (kappa * pre["scale"], omega)

    res, kept, gain_db, extremes = _copier_psa_link(
        rk4_chain_comb, lambda: comb_mid_stage(np.broadcast_to(mg, (M,)), np.broadcast_to(mp, (M,))[None, :]
                                               + ph[:, None] * mask[None, :]),       # (F, M)
        a_in, lambda r: r.line_gain(p, mode=gain_mode, unit="dB"), mismatch_of=mismatch_of,
        psa_cfg=psa_cfg, copier_cfg=copier_cfg, gamma=gamma, alpha=alpha, copier_gamma=copier_gamma, copier_alpha=copier_alpha,
        psa_x=dispersion, copier_x=dispersion if copier_dispersion is None else copier_dispersion, length_unit=length_unit,
        device=device, devices=devices)
    return dict(phase=ph, gain=gain_db if unit == "db" else res.line_gain(p, mode=gain_mode, unit=unit), p_out=res.p_wave_end,
                **extremes, kappa=np.stack([k for k, _ in kept]), omega=kept[-1][1], first_bad_step=res.first_bad_step, result=res)
