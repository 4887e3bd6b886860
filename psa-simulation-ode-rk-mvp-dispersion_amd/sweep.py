"""The batched engine behind the sweep drivers: N independent propagations in one kernel launch.

The reference runs a sweep as a Python ``for`` over points, each calling ``run_single_simulation``
(scan_mismtach.py:357-392, :694-738).  Here the per-point scalars become arrays (dbeta[N], optionally
gamma[N], alpha[N], A0[N,4]) and the loop becomes the grid of ``psa_rk4_sweep_f64``: one sweep point per
lane, the z-loop inside the kernel, only the summary (A_end, |A3|^2 at the last saved row, max over saved
rows, first non-finite step) written back.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import _native
from ._partition import CHAIN_AXES, COMB_AXES, PAIRS_AXES, PAIRS_CHAIN_AXES, SWEEP_AXES, over_devices
from .config import AdaptiveConfig, n_steps_of

__all__ = ["AdaptiveResult", "ChainResult", "CombChainResult", "CombResult", "FibreSpan", "PairsChainResult", "PairsResult",
           "SinglePumpChainResult", "SinglePumpResult", "SweepResult", "check_gain", "initial_amplitudes", "rk4_chain",
           "rk4_chain_comb", "rk4_chain_pairs", "rk4_chain_single_pump", "rk4_sweep", "rk4_sweep_comb", "rk4_sweep_pairs",
           "rk4_sweep_single_pump", "rk45_sweep"]


def initial_amplitudes(p_in, phase_in=None) -> np.ndarray:
    """A0 = sqrt(P) * exp(i*phi) for p_in (..., n_waves); the phase factor is skipped when every phase is 0
    (simulation.py:120-123, so sqrt(P) stays bit-exact in the common seed-phase-zero case)."""
    p = np.asarray(p_in, dtype=float)
    amp = np.sqrt(p).astype(np.complex128)
    if phase_in is not None:
        ph = np.asarray(phase_in, dtype=float)
        if np.any(ph != 0.0):
            amp = amp * np.exp(1j * ph)
    return amp


def check_gain(mode: str = "max", unit: str = "dB") -> str:
    """The gain rules every summary accepts: gain_mode "end" | "max", gain_unit "dB" | "linear" (any case, spaces
    ignored).  Returns the unit lower-cased; raises ValueError otherwise."""
    if mode not in ("end", "max"):
        raise ValueError(f"Unknown gain_mode={mode!r}. Use 'end' or 'max'.")
    u = str(unit).strip().lower()
    if u not in ("db", "linear"):
        raise ValueError("gain_unit must be 'dB' or 'linear'")
    return u


@dataclass
class SweepResult:
    a_end: np.ndarray            # (N, n_waves) complex: state at the last SAVED row
    p_end: np.ndarray            # (N,) |A_signal|^2 there
    p_max: np.ndarray            # (N,) max over saved rows (z = 0 included), NaN-propagating
    first_bad_step: np.ndarray   # (N,) int64, -1 = finite everywhere (or check_nan off)
    n_steps: int
    save_every: int
    elapsed_ms: float            # kernel time (hipEvents)
    traj: Optional[np.ndarray] = None   # (N, n_saved, n_waves) when requested
    p_wave_end: Optional[np.ndarray] = None   # (N, n_waves) |A_j|^2 at the last saved row (wave_summary=True)
    p_wave_max: Optional[np.ndarray] = None   # (N, n_waves) max over saved rows, NaN-propagating (wave_summary=True)

    def gain(self, p0_sig: float, *, mode: str = "max", unit: str = "dB", device: int = 0) -> np.ndarray:
        """Per-point signal gain with the drivers' NaN rules (scan_mismtach.py:376-392); reduced on the GPU."""
        return self.summary(p0_sig, mode=mode, unit=unit, device=device)[0]

    def summary(self, p0_sig: float, *, mode: str = "max", unit: str = "dB", device: int = 0, wave: int = 2):
        """(gain[N], best_index, best_gain, n_finite) -- gain_mode "end" | "max" (scan_mismtach.py:27-40).  ``wave`` other
        than 2 (the signal) reduces that wave's column of p_wave_end / p_wave_max (a sweep run with wave_summary=True)."""
        u = check_gain(mode, unit)
        if int(wave) == 2:
            metric = self.p_max if mode == "max" else self.p_end
        else:
            cols = self.p_wave_max if mode == "max" else self.p_wave_end
            if cols is None:
                raise ValueError("wave != 2 needs the per-wave summary: run the sweep with wave_summary=True")
            if not 0 <= int(wave) < cols.shape[1]:
                raise ValueError(f"wave must be in [0, {cols.shape[1]}), got {wave}")
            metric = np.ascontiguousarray(cols[:, int(wave)])
        # a float32 sweep keeps float32 gains (psa_gain_summary_f32); everything else is reduced in float64
        metric = np.asarray(metric)
        if metric.dtype != np.float32:
            metric = metric.astype(np.float64, copy=False)
        return _native.gain_summary_host(metric, self.first_bad_step, float(p0_sig), gain_db=(u == "db"), device=device)


def _fixed_grid(z_max, dz, n_steps, save_every):
    """The fixed-step grid arguments -> (n_steps, save_every): z_max positive and finite, ``dz`` giving
    n = int(round(z_max/dz)) as integrators.py:194 unless ``n_steps`` is passed, at least one step, save_every positive."""
    if not 0.0 < z_max < math.inf:   # NaN included; plain comparisons: a NumPy call here shows in a 50 us sweep
        raise ValueError("z_max must be positive")
    if n_steps is None:
        if dz is None or dz <= 0.0:
            raise ValueError("dz must be positive")
        n_steps = n_steps_of(z_max, dz)
    if save_every <= 0:
        raise ValueError("save_every must be a positive integer")
    if n_steps < 1:
        raise ValueError("z_max / dz rounds to zero steps")
    return int(n_steps), int(save_every)


def _run(host_fn, axes, n_points: int, kw: dict, device: int, devices) -> dict:
    """host_fn(**kw) on ``device`` (on devices[0] where a list names one GPU), or the points split over several ``devices``
    of this process (one thread per device)."""
    devs = None if devices is None else [int(d) for d in devices]
    if devs is not None and len(devs) == 0:
        raise ValueError("devices must name at least one GPU")
    if devs is not None and len(devs) > 1 and n_points > 1:
        return over_devices(host_fn, devs, n_points, axes, kw)
    return host_fn(device=(devs[0] if devs else device), **kw)


def rk4_sweep(dbeta, *, z_max: float, dz: Optional[float] = None, n_steps: Optional[int] = None,
              save_every: int = 10, check_nan: bool = True, gamma, alpha, a0, dbeta2=None, dtype=np.float64,
              device: int = 0, exact_step: Optional[bool] = None, want_traj: bool = False,
              devices: Optional[Sequence[int]] = None, wave_summary: bool = False) -> SweepResult:
    """Propagate N points.  ``dz`` gives n = int(round(z_max/dz)) as integrators.py:194; or pass ``n_steps``.
    ``devices=[0, 1, ...]`` splits the points over several GPUs of this process (one thread per device).
    ``wave_summary=True`` also fills p_wave_end / p_wave_max: the end and maximum power of every wave."""
    n_steps, save_every = _fixed_grid(z_max, dz, n_steps, save_every)
    db = np.atleast_1d(np.asarray(dbeta))
    kw = dict(dbeta=db, n_steps=n_steps, z_max=float(z_max), save_every=save_every, gamma=gamma, alpha=alpha, a0=a0,
              dbeta2=dbeta2, check_nan=check_nan, exact_step=exact_step, want_traj=want_traj, dtype=dtype)
    if wave_summary:
        kw["wave_summary"] = True
    # a dbeta that is not 1-D goes to sweep_host as it is, which rejects it
    r = _run(_native.sweep_host, SWEEP_AXES, db.shape[0] if db.ndim == 1 else 1, kw, device, devices)
    return SweepResult(r["a_end"], r["p_end"], r["p_max"], r["first_bad_step"], n_steps, save_every,
                       r["elapsed_ms"], r.get("traj"), r.get("p_wave_end"), r.get("p_wave_max"))


# ---- the wave-summary families: multi-channel, single-pump and multi-line sweeps ------------------------------------------
@dataclass
class _WaveResult:
    """What the results of the three families share: the fields, and the drivers' NaN rules for a power over a seed power."""
    a_end: np.ndarray            # (N, n_waves) complex: state at the last SAVED row
    p_wave_end: np.ndarray       # (N, n_waves) |A_j|^2 there
    p_wave_max: np.ndarray       # (N, n_waves) max over saved rows (z = 0 included), NaN-propagating
    first_bad_step: np.ndarray   # (N,) int64, -1 = finite everywhere (or check_nan off)
    n_steps: int
    save_every: int
    elapsed_ms: float            # kernel time (hipEvents)
    p_wave_in: Optional[np.ndarray] = None   # (1 | N, n_waves) |A_j(0)|^2: what pump_depletion compares with
    traj: Optional[np.ndarray] = None        # (N, n_saved, n_waves) complex when requested

    def _over_seed(self, cols, p0, mode: str, unit: str) -> np.ndarray:
        """The metric columns ``cols`` over the seed power p0 with the drivers' NaN rule (scan_mismtach.py:376-392): a point
        with first_bad_step >= 0, a non-positive or non-finite seed power, a non-finite or non-positive ratio give NaN.  One
        column (an int) gives (N,) and takes p0 as a scalar or (N,); C columns (a slice) give (N, C) and take (C,) or (N, C)."""
        u = check_gain(mode, unit)
        metric = (self.p_wave_max if mode == "max" else self.p_wave_end)[:, cols]
        N = int(self.p_wave_end.shape[0])
        p0 = np.asarray(p0, dtype=float)
        if metric.ndim == 1:
            if p0.shape not in ((), (1,), (N,)):
                raise ValueError(f"p0 must be a scalar or have shape ({N},), got {p0.shape}")
        elif p0.shape not in (metric.shape[1:], metric.shape):
            raise ValueError(f"p0 must have shape ({metric.shape[1]},) or ({N}, {metric.shape[1]}), got {p0.shape}")
        p0 = np.broadcast_to(p0, metric.shape)
        finite = np.asarray(self.first_bad_step) < 0
        with np.errstate(all="ignore"):
            ok = (p0 > 0.0) & np.isfinite(p0) & (finite if metric.ndim == 1 else finite[:, None])
            g = metric / np.where(ok, p0, 1.0)
            ok &= np.isfinite(g) & (g > 0.0)
            return np.where(ok, g if u == "linear" else 10.0 * np.log10(np.where(ok, g, 1.0)), np.nan)

    def _depletion(self, pumps: slice, driver: str) -> np.ndarray:
        """(N,): the fraction of the input power of the columns ``pumps`` that is gone at the last saved row; NaN for a
        failed point or dark pumps."""
        if self.p_wave_in is None:
            raise ValueError(f"pump_depletion needs p_wave_in (set by {driver})")
        N = int(self.p_wave_end.shape[0])
        p_in = np.broadcast_to(self.p_wave_in[:, pumps].sum(axis=1), (N,))
        with np.errstate(all="ignore"):
            ok = (p_in > 0.0) & np.isfinite(p_in) & (np.asarray(self.first_bad_step) < 0)
            d = 1.0 - self.p_wave_end[:, pumps].sum(axis=1) / np.where(ok, p_in, 1.0)
            return np.where(ok & np.isfinite(d), d, np.nan)


def _mismatch_columns(x, name: str, letter: str, low: int, high: int) -> np.ndarray:
    """A mismatch of several columns, (N, C) with low <= C <= high, as float64."""
    x = np.asarray(x, dtype=float)
    if x.ndim != 2 or not low <= x.shape[1] <= high:
        raise ValueError(f"{name} must have shape (N, {letter}) with {low} <= {letter} <= {high}, got {x.shape}")
    return x


def _sweep_waves(result, host_fn, axes, key: str, checked, *, z_max, dz, n_steps, save_every, a0, dtype, device, devices,
                 reroute=None, **options):
    """The driver of a wave-summary family: the dtype and grid rules, ``checked()`` -> (the mismatch (N, ...), the columns of
    a0, what the a0 error says they are for), the a0 rule, host_fn(**{key: mismatch}, ...) over the devices, and the family's
    ``result``.  ``reroute(kw, N)`` -> (host_fn, axes, kw) sends the call elsewhere once its arguments stand."""
    f64 = np.dtype(dtype) == np.dtype(np.float64)
    if not f64 and np.dtype(dtype) != np.dtype(np.float32):
        raise ValueError(f"dtype must be float64 or float32, got {np.dtype(dtype)}")
    n_steps, save_every = _fixed_grid(z_max, dz, n_steps, save_every)
    mismatch, nw, what = checked()
    N = int(mismatch.shape[0])
    a0 = np.asarray(a0, dtype=np.complex128 if f64 else np.complex64)
    if a0.shape not in ((nw,), (1, nw), (N, nw)):
        raise ValueError(f"a0 must have shape ({nw},) or ({N}, {nw}){what}, got {a0.shape}")
    kw = dict({key: mismatch}, n_steps=n_steps, z_max=float(z_max), save_every=save_every, a0=a0, **options)
    if not f64:
        kw["dtype"] = np.float32          # the float64 call stays as it was: no dtype argument
    if reroute is not None:
        host_fn, axes, kw = reroute(kw, N)
    r = _run(host_fn, axes, N, kw, device, devices)
    return result(r["a_end"], r["p_wave_end"], r["p_wave_max"], r["first_bad_step"], n_steps, save_every, r["elapsed_ms"],
                  np.abs(np.atleast_2d(a0)) ** 2, r.get("traj"))


@dataclass
class PairsResult(_WaveResult):
    """Outcome of a multi-channel sweep; waves [p1, p2, s_1, i_1, ..., s_K, i_K], NW = 2 + 2K columns."""

    @property
    def n_pairs(self) -> int:
        return (int(self.p_wave_end.shape[1]) - 2) // 2

    def channel_gain(self, p0, *, mode: str = "max", unit: str = "dB") -> np.ndarray:
        """(N, K): every signal's gain over its seed power p0 (K,) or (N, K); gain_mode "end" | "max"."""
        return self._over_seed(slice(2, None, 2), p0, mode, unit)

    def idler_conversion(self, p0, *, mode: str = "max", unit: str = "dB") -> np.ndarray:
        """(N, K): every idler's power over the SIGNAL's seed power p0 (K,) or (N, K): the conversion efficiency."""
        return self._over_seed(slice(3, None, 2), p0, mode, unit)

    def pump_depletion(self) -> np.ndarray:
        """(N,): the fraction of the two pumps' input power that is gone at the last saved row,
        1 - (P_p1 + P_p2)_end / (P_p1 + P_p2)_in (fibre loss included); NaN for a failed point or dark pumps."""
        return self._depletion(slice(0, 2), "rk4_sweep_pairs")


def rk4_sweep_pairs(dbeta, *, z_max: float, dz: Optional[float] = None, n_steps: Optional[int] = None,
                    save_every: int = 10, check_nan: bool = True, exact_step: Optional[bool] = None, gamma, alpha, a0,
                    device: int = 0, devices: Optional[Sequence[int]] = None, want_traj: bool = False) -> PairsResult:
    """Propagate N points of the multi-channel model: two pumps and K = 1..16 signal/idler pairs, waves
    [p1, p2, s_1, i_1, ..., s_K, i_K] (build-defined; K = 1 is the reference's 4-wave system, K = 2 the
    6-wave model).  All channels draw on the same two pumps and shift each other's phase matching through SPM/XPM; FWM
    products between channels (signal-signal mixing) are NOT modelled here, where the detunings are arbitrary: on a uniform
    frequency grid rk4_sweep_comb models every one of them.

    dbeta (N, K): the mismatch of every pair; gamma / alpha a scalar or (N,); a0 (NW,) or (N, NW) complex, NW = 2 + 2K.
    ``dz`` gives n = int(round(z_max/dz)) as integrators.py:194; or pass ``n_steps``.  ``devices=[0, 1, ...]`` splits the
    points over several GPUs of this process.  ``want_traj`` also returns every saved row (the chain's entry point with one
    span: the summaries are the same bits).  Fixed-step float64 only: no float32 or adaptive form; concatenated spans
    (copier - mid-stage - PSA) are rk4_chain_pairs."""
    def checked():
        db = _mismatch_columns(dbeta, "dbeta", "K", 1, _native.MAX_PAIRS)
        return db, 2 + 2 * int(db.shape[1]), f" for {db.shape[1]} pairs"

    def one_span(kw, N):   # one span of the chain's entry point: dbeta (1, N, K), gamma / alpha (1,) or (1, N)
        kw.update(dbeta=kw["dbeta"][None], n_steps=[kw.pop("n_steps")], seg_len=[kw.pop("z_max")], want_traj=True,
                  gamma=_span_column([gamma], 1, N, "gamma", np.float64), alpha=_span_column([alpha], 1, N, "alpha", np.float64))
        return _native.pairs_chain_host, PAIRS_CHAIN_AXES, kw

    return _sweep_waves(PairsResult, _native.sweep_pairs_host, PAIRS_AXES, "dbeta", checked, z_max=z_max, dz=dz, n_steps=n_steps,
                        save_every=save_every, a0=a0, dtype=np.float64, device=device, devices=devices,
                        reroute=one_span if want_traj else None, gamma=gamma, alpha=alpha, check_nan=check_nan, exact_step=exact_step)


@dataclass
class SinglePumpResult(_WaveResult):
    """Outcome of a single-pump sweep; waves [p, s, i], 3 columns."""

    def signal_gain(self, p0, *, mode: str = "max", unit: str = "dB") -> np.ndarray:
        """(N,): the signal's gain over its seed power p0, a scalar or (N,); gain_mode "end" | "max"."""
        return self._over_seed(1, p0, mode, unit)

    def idler_conversion(self, p0, *, mode: str = "max", unit: str = "dB") -> np.ndarray:
        """(N,): the idler's power over the SIGNAL's seed power p0, a scalar or (N,): the conversion efficiency."""
        return self._over_seed(2, p0, mode, unit)

    def pump_depletion(self) -> np.ndarray:
        """(N,): the fraction of the pump's input power that is gone at the last saved row, 1 - P_p_end / P_p_in (fibre
        loss included); NaN for a failed point or a dark pump."""
        return self._depletion(slice(0, 1), "rk4_sweep_single_pump")


def rk4_sweep_single_pump(dbeta, *, z_max: float, dz: Optional[float] = None, n_steps: Optional[int] = None,
                          save_every: int = 10, check_nan: bool = True, exact_step: Optional[bool] = None, gamma, alpha, a0,
                          want_traj: bool = False, device: int = 0,
                          devices: Optional[Sequence[int]] = None, dtype=np.float64) -> SinglePumpResult:
    """Propagate N points of the single-pump (degenerate) model: one pump, a signal and an idler at 2 w_p - w_s, waves
    [p, s, i] (build-defined).  Not rk4_sweep with equal pumps: that system gives the pump 1.5 times the
    self-phase modulation.

    dbeta (N,): beta(w_s) + beta(w_i) - 2 beta(w_p) per point; gamma / alpha a scalar or (N,); a0 (3,) or (N, 3) complex.
    ``dz`` gives n = int(round(z_max/dz)) as integrators.py:194; or pass ``n_steps``.  ``want_traj`` also returns every saved
    row; ``devices=[0, 1, ...]`` splits the points (and the trajectory) over several GPUs of this process.
    ``dtype=np.float32`` runs the packed float32 kernel (two points per lane) and returns float32 / complex64
    arrays; any dtype but float64 and float32 is a ValueError.  Fixed-step only: no adaptive form; concatenated spans (copier
    - mid-stage - PSA) are rk4_chain_single_pump, in float64."""
    def checked():
        db = np.atleast_1d(np.asarray(dbeta, dtype=float))
        if db.ndim != 1:
            raise ValueError(f"dbeta must be a scalar or have shape (N,), got {db.shape}")
        return db, 3, ""

    return _sweep_waves(SinglePumpResult, _native.single_pump_host, SWEEP_AXES, "dbeta", checked, z_max=z_max, dz=dz,
                        n_steps=n_steps, save_every=save_every, a0=a0, dtype=dtype, device=device, devices=devices, gamma=gamma,
                        alpha=alpha, check_nan=check_nan, exact_step=exact_step, want_traj=want_traj)


@dataclass
class CombResult(_WaveResult):
    """Outcome of a multi-line sweep; lines 0..M-1 ascending in frequency, M columns."""

    def line_gain(self, p0, *, mode: str = "max", unit: str = "dB") -> np.ndarray:
        """(N, M): every line's power over its input power p0 (M,) or (N, M); gain_mode "end" | "max".  The drivers' NaN
        rule per line (scan_mismtach.py:376-392): a point with first_bad_step >= 0, a non-positive or non-finite input
        power (a dark line), a non-finite or non-positive ratio give NaN."""
        return self._over_seed(slice(None), p0, mode, unit)

    def total_power(self) -> np.ndarray:
        """(N,): sum of the lines' powers at the last saved row (conserved for alpha = 0); NaN for a failed point."""
        with np.errstate(all="ignore"):
            return np.where(np.asarray(self.first_bad_step) < 0, self.p_wave_end.sum(axis=1), np.nan)


def rk4_sweep_comb(kappa, *, z_max: float, dz: Optional[float] = None, n_steps: Optional[int] = None, save_every: int = 10,
                   check_nan: bool = True, gamma, alpha, a0, want_traj: bool = False, device: int = 0,
                   devices: Optional[Sequence[int]] = None, dtype=np.float64) -> CombResult:
    """Propagate N points of the CW multi-line ("frequency comb") model: M = 3..12 lines at w_0 + m dw, ascending in
    frequency, coupled by EVERY four-wave-mixing product k + l - n = m that falls on the grid -- SPM, XPM, pump-pump,
    pump-signal and signal-signal mixing (build-defined).  It is what the multi-channel model of
    rk4_sweep_pairs leaves out and needs the uniform grid that model does not have.  M = 3 is rk4_sweep_single_pump with
    lines [0, 1, 2] = waves [s, p, i].

    kappa (N, M): the lines' propagation constants in any gauge (kappa + a + b*m is the same system);  gamma / alpha a scalar
    or (N,); a0 (M,) or (N, M) complex.  ``dz`` gives n = int(round(z_max/dz)) as integrators.py:194; or pass ``n_steps``.
    With ``check_nan`` first_bad_step is the exact step.  ``want_traj`` also returns every saved row; ``devices=[0, 1, ...]``
    splits the points over several GPUs of this process.
    ``dtype=np.float32`` runs the packed float32 kernel (two points per lane) and returns float32 / complex64
    arrays; kappa is rounded to float32 once, so pass it in a gauge that keeps |kappa| small.  It pays from sweeps that fill
    the chip with two points per lane (131 072 points on one device; DESIGN.md 3.3f has the rates per M) and gains nothing on
    smaller ones.  Any dtype but float64 and float32 is a ValueError.  Fixed-step on a uniform grid only: no RK45 or
    process-group form; chains of spans are rk4_chain_comb, in float64."""
    def checked():
        kp = _mismatch_columns(kappa, "kappa", "M", 3, _native.MAX_LINES)
        return kp, int(kp.shape[1]), f" for {kp.shape[1]} lines"

    return _sweep_waves(CombResult, _native.comb_host, COMB_AXES, "kappa", checked, z_max=z_max, dz=dz, n_steps=n_steps,
                        save_every=save_every, a0=a0, dtype=dtype, device=device, devices=devices, gamma=gamma, alpha=alpha,
                        check_nan=check_nan, want_traj=want_traj)


# ---- chains of fibre spans ------------------------------------------------------------------------------------------
@dataclass
class FibreSpan:
    """One span of a chain: ``length`` with ``dz`` (n = int(round(length/dz)), as n_steps_of) or ``n_steps``; dbeta,
    gamma, alpha (and dbeta2 for 6 waves) a scalar or one value per sweep point, per length unit of ``length``."""
    length: float
    dbeta: object = 0.0
    gamma: object = 0.0
    alpha: object = 0.0
    dz: Optional[float] = None
    n_steps: Optional[int] = None
    dbeta2: object = None

    def __post_init__(self):
        if not (np.isfinite(self.length) and self.length > 0.0):
            raise ValueError("FibreSpan.length must be positive and finite")
        if (self.dz is None) == (self.n_steps is None):
            raise ValueError("FibreSpan needs exactly one of dz and n_steps")
        if self.n_steps is None:
            if not self.dz > 0.0:
                raise ValueError("FibreSpan.dz must be positive")
            self.n_steps = n_steps_of(self.length, self.dz)
        if int(self.n_steps) < 1:
            raise ValueError("FibreSpan: length / dz rounds to zero steps")
        self.n_steps = int(self.n_steps)


@dataclass
class _ChainGrid:
    """The grid of a chain's result, after the fields of the family's own result."""
    z_out: Optional[np.ndarray] = None         # (n_saved_total,) absolute z of every saved row (repeats at a boundary)
    row_offsets: Optional[np.ndarray] = None   # (S + 1,) span s owns rows [row_offsets[s], row_offsets[s + 1])
    step_offsets: Optional[np.ndarray] = None  # (S + 1,) span s owns steps [step_offsets[s], step_offsets[s + 1])


@dataclass
class ChainResult(_ChainGrid, SweepResult):
    """SweepResult of a chain: rows of every span in order (each span's z = 0 row is the post-transfer state), amplitudes
    in the physical frame, first_bad_step counted over the whole chain.  n_steps is the chain's total."""


def _span_column(values, S: int, N: int, name: str, dtype) -> np.ndarray:
    """Per-span scalars -> (S,); as soon as one span gives N values -> (S, N)."""
    arrs = [np.atleast_1d(np.asarray(v, dtype=dtype)) for v in values]
    for a in arrs:
        if a.ndim != 1 or a.shape[0] not in (1, N):
            raise ValueError(f"{name} of a span must be a scalar or have {N} entries, got shape {a.shape}")
    if all(a.shape[0] == 1 for a in arrs) and N != 1:
        return np.array([a[0] for a in arrs], dtype=dtype)
    return np.stack([np.broadcast_to(a, (N,)) for a in arrs]).astype(dtype)


def _chain_inputs(spans, a0, transfers, save_every, widths, dtype, pairs=False, lines=False):
    """The span, a0 and transfer rules every chain shares, in rk4_chain's order -> (spans, save_every, dtype, N, n_waves,
    dbeta (S, N), dbeta2 (S, N) for 6 waves else None, gamma, alpha (S,) | (S, N), transfers None | (S-1, n_waves) |
    (S-1, N, n_waves), n_steps (S,), lengths (S,)).  ``pairs``: the multi-channel model, K = (n_waves - 2) / 2 mismatches per
    span: a span's dbeta is (K,) for every point or (N, K), the returned dbeta (S, N, K), and dbeta2 is an error.  ``lines``: the
    multi-line model, the same rules with K = n_waves: a span's dbeta holds the propagation constant of every line."""
    spans = list(spans)
    if not spans or not all(isinstance(s, FibreSpan) for s in spans):
        raise ValueError("spans must be a non-empty sequence of FibreSpan")
    if int(save_every) <= 0:
        raise ValueError("save_every must be a positive integer")
    save_every = int(save_every)
    for k, s in enumerate(spans):
        if s.n_steps % save_every:
            raise ValueError(f"span {k}: n_steps = {s.n_steps} is not a multiple of save_every = {save_every}")
    dtype = np.dtype(dtype)
    S = len(spans)
    a0 = np.asarray(a0)
    if a0.ndim not in (1, 2) or a0.shape[-1] not in widths:
        raise ValueError(f"a0 must have shape (n_waves,) or (N, n_waves) with n_waves in {tuple(widths)}")
    nw = int(a0.shape[-1])
    what = "lines" if lines else "pairs"
    pairs = pairs or lines   # from here on: a span's dbeta has K columns
    sizes = {int(np.size(v)) for s in spans for v in (s.gamma, s.alpha) + (() if pairs else (s.dbeta, s.dbeta2)) if v is not None}
    if pairs:
        K = nw if lines else (nw - 2) // 2
        if any(s.dbeta2 is not None for s in spans):
            raise ValueError("the multi-line model takes its M propagation constants in dbeta: dbeta2 must be None" if lines else
                             "the multi-channel model takes its K mismatches in dbeta: dbeta2 must be None")
        for k, s in enumerate(spans):
            shape = np.shape(s.dbeta)
            if len(shape) not in (1, 2) or shape[-1] != K:
                raise ValueError(f"span {k}: dbeta must have shape ({K},) or (N, {K}) for {K} {what}, got {shape}")
            if len(shape) == 2:
                sizes.add(int(shape[0]))
    if a0.ndim == 2:
        sizes.add(int(a0.shape[0]))
    sizes.discard(1)
    if len(sizes) > 1:
        raise ValueError(f"per-point arguments disagree on the number of points: {sorted(sizes)}")
    N = sizes.pop() if sizes else 1
    if pairs:
        for k, s in enumerate(spans):
            if np.ndim(s.dbeta) == 2 and np.shape(s.dbeta)[0] != N:   # a single (1, K) row among N points
                raise ValueError(f"span {k}: dbeta must have shape ({K},) or ({N}, {K}), got {np.shape(s.dbeta)}")
        dbeta = np.stack([np.broadcast_to(np.asarray(s.dbeta, dtype=dtype), (N, K)) for s in spans])
    else:
        dbeta = np.stack([np.broadcast_to(np.asarray(s.dbeta, dtype=dtype).reshape(-1), (N,)) for s in spans])
    dbeta2 = None
    if pairs:
        pass
    elif nw == 6:
        if any(s.dbeta2 is None for s in spans):
            raise ValueError("6 waves: every span needs dbeta2")
        dbeta2 = np.stack([np.broadcast_to(np.asarray(s.dbeta2, dtype=dtype).reshape(-1), (N,)) for s in spans])
    elif any(s.dbeta2 is not None for s in spans):
        raise ValueError("dbeta2 is only meaningful for 6 waves")
    gamma = _span_column([s.gamma for s in spans], S, N, "gamma", dtype)
    alpha = _span_column([s.alpha for s in spans], S, N, "alpha", dtype)
    tr = None
    if transfers is not None:
        tl = list(transfers)
        if len(tl) != S - 1:
            raise ValueError(f"{S} spans need {S - 1} transfers, got {len(tl)}")
        if tl:
            arrs = [np.asarray(t, dtype=np.complex128) for t in tl]
            for t in arrs:
                if t.shape not in ((nw,), (N, nw)):
                    raise ValueError(f"a transfer must have shape ({nw},) or ({N}, {nw}), got {t.shape}")
            if all(t.ndim == 1 for t in arrs):
                tr = np.stack(arrs)
            else:
                tr = np.stack([np.broadcast_to(t, (N, nw)) for t in arrs])
    steps = np.array([s.n_steps for s in spans], dtype=np.int64)
    lens = np.array([float(s.length) for s in spans])
    return spans, save_every, dtype, N, nw, dbeta, dbeta2, gamma, alpha, tr, steps, lens


def _run_chain(host_name: str, widths, spans, a0, transfers, save_every, dtype, a0_dtype, device, devices, pairs=False,
               lines=False, **options):
    """What every chain driver does: the shared input rules, the family's host call (looked up in _native when called) over
    the devices, and the grid of the saved rows -> (outputs, save_every, a0 as passed on, the _ChainGrid fields).  ``pairs``:
    the multi-channel family (_chain_inputs' rules for it, PAIRS_CHAIN_AXES), ``lines``: the multi-line family (the same
    axes); otherwise the family is the 4/6-wave one where 6 is among ``widths`` and the single-pump one where it is not."""
    spans, save_every, dtype, N, nw, dbeta, dbeta2, gamma, alpha, tr, steps, lens = _chain_inputs(
        spans, a0, transfers, save_every, widths, dtype, pairs=pairs, lines=lines)
    a0 = np.asarray(a0, dtype=a0_dtype)
    kw = dict(dbeta=dbeta, n_steps=steps, seg_len=lens, save_every=save_every, gamma=gamma, alpha=alpha, a0=a0,
              transfers=tr, **options)
    pairs = pairs or lines
    if 6 in widths and not pairs:   # the 4/6-wave family
        kw.update(dbeta2=dbeta2, dtype=dtype)
    r = _run(getattr(_native, host_name), PAIRS_CHAIN_AXES if pairs else CHAIN_AXES, N, kw, device, devices)
    rows = steps // save_every + 1
    z0 = np.concatenate([[0.0], np.cumsum(lens)])
    z_out = np.concatenate([z0[k] + np.linspace(0.0, lens[k], int(steps[k]) + 1)[::save_every] for k in range(len(steps))])
    grid = dict(z_out=z_out, row_offsets=np.concatenate([[0], np.cumsum(rows)]).astype(np.int64),
                step_offsets=np.concatenate([[0], np.cumsum(steps)]).astype(np.int64))
    return r, save_every, a0, grid


def rk4_chain(spans: Sequence[FibreSpan], *, a0, transfers=None, save_every: int = 10, check_nan: bool = True,
              exact_step: Optional[bool] = None, dtype=np.float64, want_traj: bool = False, wave_summary: bool = False,
              device: int = 0, devices: Optional[Sequence[int]] = None) -> ChainResult:
    """Propagate N points through a chain of fibre spans (psa_rk4_chain_*): each span one launch of the sweep kernel,
    the mismatch phase accumulated across spans, ``transfers[s]`` applied between span s and s+1.

    transfers: None (identity), or S-1 entries, each (n_waves,) complex for every point or (N, n_waves) per point
    (see simulation.mid_stage).  Every span's n_steps must be a multiple of ``save_every``."""
    r, save_every, _, grid = _run_chain("chain_host", (4, 6), spans, a0, transfers, save_every, dtype, None, device, devices,
                                        check_nan=check_nan, exact_step=exact_step, want_traj=want_traj,
                                        wave_summary=wave_summary)
    return ChainResult(r["a_end"], r["p_end"], r["p_max"], r["first_bad_step"], int(grid["step_offsets"][-1]), save_every,
                       r["elapsed_ms"], r.get("traj"), r.get("p_wave_end"), r.get("p_wave_max"), **grid)


@dataclass
class SinglePumpChainResult(_ChainGrid, SinglePumpResult):
    """SinglePumpResult of a chain: rows of every span in order (each span's z = 0 row is the post-transfer state),
    amplitudes in the physical frame, first_bad_step counted over the whole chain.  n_steps is the chain's total."""


def rk4_chain_single_pump(spans: Sequence[FibreSpan], *, a0, transfers=None, save_every: int = 10, check_nan: bool = True,
                          exact_step: Optional[bool] = None, want_traj: bool = False, device: int = 0,
                          devices: Optional[Sequence[int]] = None) -> SinglePumpChainResult:
    """Propagate N points of the single-pump model, waves [p, s, i], through a chain of fibre spans
    (psa_rk4_single_pump_chain_f64): each span one launch of the single-pump kernel, the mismatch phase
    accumulated across spans, ``transfers[s]`` applied between span s and s+1.  The kernel assumes nothing about which wave
    is strong: the signal-degenerate dual-pump PSA is the same call with the degenerate signal in slot 0, the two pumps in
    slots 1 and 2 and dbeta = beta_1 + beta_2 - 2 beta_s.

    a0 (3,) or (N, 3) complex; transfers: None (identity), or S-1 entries, each (3,) complex for every point or (N, 3) per
    point (see simulation.single_pump_mid_stage).  Every span's n_steps must be a multiple of ``save_every``; a span with
    dbeta2 is an error.  float64 only."""
    r, save_every, a0, grid = _run_chain("single_pump_chain_host", (3,), spans, a0, transfers, save_every, np.float64,
                                         np.complex128, device, devices, check_nan=check_nan, exact_step=exact_step,
                                         want_traj=want_traj)
    return SinglePumpChainResult(r["a_end"], r["p_wave_end"], r["p_wave_max"], r["first_bad_step"],
                                 int(grid["step_offsets"][-1]), save_every, r["elapsed_ms"], np.abs(np.atleast_2d(a0)) ** 2,
                                 r.get("traj"), **grid)


@dataclass
class PairsChainResult(_ChainGrid, PairsResult):
    """PairsResult of a chain: rows of every span in order (each span's z = 0 row is the post-transfer state), amplitudes
    in the physical frame, first_bad_step counted over the whole chain.  n_steps is the chain's total."""


def rk4_chain_pairs(spans: Sequence[FibreSpan], *, a0, transfers=None, save_every: int = 10, check_nan: bool = True,
                    exact_step: Optional[bool] = None, want_traj: bool = False, device: int = 0,
                    devices: Optional[Sequence[int]] = None) -> PairsChainResult:
    """Propagate N points of the multi-channel model, waves [p1, p2, s_1, i_1, ..., s_K, i_K], through a chain of fibre
    spans (psa_rk4_pairs_chain_f64): each span one launch of the multi-channel kernel, every pair's
    mismatch phase accumulated across spans, ``transfers[s]`` applied between span s and s+1 -- the WDM copier - mid-stage -
    PSA link, whose channels couple through pump depletion and SPM/XPM.

    a0 (NW,) or (N, NW) complex fixes K = (NW - 2) / 2 in 1..16; a span's dbeta is (K,) for every point or (N, K); transfers:
    None (identity), or S-1 entries, each (NW,) complex for every point or (N, NW) per point (see
    simulation.wdm_mid_stage).  Every span's n_steps must be a multiple of ``save_every``; a span with dbeta2 is an error.
    float64 only."""
    r, save_every, a0, grid = _run_chain("pairs_chain_host", tuple(range(4, 2 * _native.MAX_PAIRS + 3, 2)), spans, a0, transfers,
                                         save_every, np.float64, np.complex128, device, devices, pairs=True,
                                         check_nan=check_nan, exact_step=exact_step, want_traj=want_traj)
    return PairsChainResult(r["a_end"], r["p_wave_end"], r["p_wave_max"], r["first_bad_step"], int(grid["step_offsets"][-1]),
                            save_every, r["elapsed_ms"], np.abs(np.atleast_2d(a0)) ** 2, r.get("traj"), **grid)


@dataclass
class CombChainResult(_ChainGrid, CombResult):
    """CombResult of a chain: rows of every span in order (each span's z = 0 row is the post-transfer state), amplitudes in
    the physical frame, first_bad_step counted over the whole chain.  n_steps is the chain's total."""


def rk4_chain_comb(spans: Sequence[FibreSpan], *, a0, transfers=None, save_every: int = 10, check_nan: bool = True,
                   exact_step: Optional[bool] = None, want_traj: bool = False, device: int = 0,
                   devices: Optional[Sequence[int]] = None) -> CombChainResult:
    """Propagate N points of the multi-line ("frequency comb") model, lines 0..M-1 ascending in frequency, through a chain of
    fibre spans (psa_rk4_comb_chain_f64): each span one launch of the multi-line kernel, EVERY line's phase
    kappa_{s,m} L_s accumulated across spans, ``transfers[s]`` applied between span s and s+1 -- the copier - mid-stage - PSA
    link with every FWM product on the grid: WDM crosstalk, cascaded pump products, higher-order idlers.

    a0 (M,) or (N, M) complex fixes M in 3..12; a span's propagation constants go in ``FibreSpan.dbeta`` as (M,) for every
    point or (N, M), in any gauge kappa + a_s + b_s*m per span (no output depends on it); transfers: None (identity),
    or S-1 entries, each (M,) complex for every point or (N, M) per point (see simulation.comb_mid_stage).  Every span's
    n_steps must be a multiple of ``save_every``; a span with dbeta2 is an error.  first_bad_step is the exact step
    (``exact_step`` changes nothing).  float64 only."""
    r, save_every, a0, grid = _run_chain("comb_chain_host", tuple(range(3, _native.MAX_LINES + 1)), spans, a0, transfers,
                                         save_every, np.float64, np.complex128, device, devices, lines=True,
                                         check_nan=check_nan, exact_step=exact_step, want_traj=want_traj)
    return CombChainResult(r["a_end"], r["p_wave_end"], r["p_wave_max"], r["first_bad_step"], int(grid["step_offsets"][-1]),
                           save_every, r["elapsed_ms"], np.abs(np.atleast_2d(a0)) ** 2, r.get("traj"), **grid)


# ---- adaptive (RK45) sweeps ----------------------------------------------------------------------------------------
@dataclass
class AdaptiveResult:
    """Per-point outcome of an adaptive sweep (psa_rk45_sweep_f64)."""
    a_end: np.ndarray            # (N, n_waves) complex: the state at z_end
    p_end: np.ndarray            # (N,) |A_signal|^2 there
    p_max: np.ndarray            # (N,) max over z = 0 and every accepted step end, NaN-propagating
    status: np.ndarray           # (N,) int32: 0 reached z_max, 1 step below the minimum (non-finite state), 2 max_steps
    z_end: np.ndarray            # (N,) the z reached
    n_accepted: np.ndarray       # (N,) int64
    n_rejected: np.ndarray       # (N,) int64
    elapsed_ms: float            # kernel time (hipEvents)
    traj: Optional[np.ndarray] = None    # (N, n_out + 1, n_waves) dense-output rows (NaN past z_end) when n_out > 0
    z_out: Optional[np.ndarray] = None   # (n_out + 1,) np.linspace(0, z_max, n_out + 1)

    @property
    def first_bad_step(self) -> np.ndarray:
        """-1 where the point reached z_max, else its accepted step count: what the gain reduction marks as failed."""
        return np.where(self.status == 0, -1, self.n_accepted).astype(np.int64)

    def gain(self, p0_sig: float, *, mode: str = "max", unit: str = "dB", device: int = 0) -> np.ndarray:
        """Per-point signal gain with SweepResult's meaning; NaN exactly where status != 0."""
        return self.summary(p0_sig, mode=mode, unit=unit, device=device)[0]

    def summary(self, p0_sig: float, *, mode: str = "max", unit: str = "dB", device: int = 0):
        """(gain[N], best_index, best_gain, n_finite): SweepResult's reduction of the signal's p_max / p_end."""
        return SweepResult.summary(self, p0_sig, mode=mode, unit=unit, device=device)


def rk45_sweep(dbeta, *, z_max: float, tol: AdaptiveConfig = AdaptiveConfig(), gamma, alpha, a0, dbeta2=None,
               n_out: int = 0, device: int = 0) -> AdaptiveResult:
    """Propagate N points to the tolerance ``tol`` with embedded Dormand-Prince 5(4) (scipy's RK45, step for step), each
    point with its own step size.  ``n_out > 0`` also returns the dense-output rows at np.linspace(0, z_max, n_out + 1)."""
    if not (np.isfinite(z_max) and z_max > 0.0):
        raise ValueError("z_max must be positive")
    if not isinstance(tol, AdaptiveConfig):
        raise TypeError("tol must be an AdaptiveConfig")
    tol.validate()
    if int(n_out) < 0:
        raise ValueError("n_out must be >= 0")
    r = _native.rk45_sweep_host(dbeta, z_max=float(z_max), rtol=tol.rtol, atol=tol.atol, h_max=tol.h_max,
                                first_step=tol.first_step, max_steps=int(tol.max_steps), n_out=int(n_out), gamma=gamma,
                                alpha=alpha, a0=a0, dbeta2=dbeta2, device=device)
    z_out = np.linspace(0.0, float(z_max), int(n_out) + 1) if int(n_out) > 0 else None
    return AdaptiveResult(r["a_end"], r["p_end"], r["p_max"], r["status"], r["z_end"], r["n_accepted"], r["n_rejected"],
                          r["elapsed_ms"], r["traj"], z_out)
