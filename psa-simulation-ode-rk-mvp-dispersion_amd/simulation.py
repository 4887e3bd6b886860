"""Single-point runner with the reference's call surface (simulation.py:220-364).

``run_single_simulation(cfg, *, gamma, alpha, omega, p_in, ...) -> (z_out, A[n_saved, 4])``: validates,
converts ``length_unit`` quantities to metres (gamma, alpha, dbeta, beta_n divided by the scale; lengths
multiplied), builds A0 = sqrt(P)*exp(i*phi), computes dbeta ONCE on the host, then hands the whole
propagation to the HIP kernel through ``integrators.integrate_interval(rhs_yaman_simplified, ...)``.
"""
from __future__ import annotations

import dataclasses
from typing import Optional, Sequence

import numpy as np

from . import constants
from ._native import MAX_LINES
from .config import (AdaptiveConfig, SimulationConfig, custom_simulation_config, default_simulation_config,  # noqa: F401
                     n_steps_of, validate_config)
from .dispersion import DispersionParams, delta_beta_from_omegas_array
from .integrators import integrate_adaptive, integrate_interval
from .parameters import FiberParams, PhaseMatchingParams, SimulationGrid, WavesParams, make_model_params
from .phase_matching import PhaseMatchingConfig, PhaseMatchingMethod, PhaseMatchingResult, compute_phase_mismatch  # noqa: F401
from .sweep import (FibreSpan, initial_amplitudes, rk4_chain, rk4_chain_comb, rk4_chain_single_pump, rk4_sweep_comb,
                    rk4_sweep_single_pump)
from .yaman_model import rhs_yaman_simplified

_UNITS = {"m": 1.0, "km": 1000.0}


def _length_scale_to_m(length_unit: str) -> float:
    try:
        return _UNITS[str(length_unit).strip().lower()]
    except KeyError:
        raise ValueError(f"Unsupported length_unit={length_unit!r}. Use 'm' or 'km'.") from None


def _vec(x, name: str, *, what: str, lower: Optional[float] = None, strict: bool = False, n: int = 4) -> np.ndarray:
    arr = np.asarray(list(x), dtype=float)
    if arr.shape != (n,):
        raise ValueError(f"{name} must have shape ({n},), got {arr.shape}")
    if not np.all(np.isfinite(arr)):
        raise ValueError(f"{name} must be finite")
    if lower is not None and np.any(arr <= lower if strict else arr < lower):
        raise ValueError(f"{name} must be {what}")
    return arr


def _to_omega_array(omega) -> np.ndarray:
    return _vec(omega, "omega", what="positive (rad/s)", lower=0.0, strict=True)


def _to_power_array(p_in) -> np.ndarray:
    return _vec(p_in, "p_in", what="non-negative (W)", lower=0.0)


def _to_phase_array(phase_in) -> np.ndarray:
    return np.zeros(4) if phase_in is None else _vec(phase_in, "phase_in", what="")


def make_initial_amplitudes(p_in: Sequence[float], phase_in: Optional[Sequence[float]] = None) -> np.ndarray:
    """|A_j|^2 = P_j, A_j = sqrt(P_j)*exp(i*phi_j) -> complex128 (4,)  (simulation.py:103-123)."""
    return initial_amplitudes(_to_power_array(p_in), _to_phase_array(phase_in))


def _default_phase_matching_cfg(*, dispersion, beta_legacy) -> PhaseMatchingConfig:
    """dispersion -> SYMMETRIC_EVEN (2,4); only legacy betas -> PROVIDED b3+b4-b1-b2; neither -> ValueError."""
    if dispersion is not None:
        return PhaseMatchingConfig(method=PhaseMatchingMethod.SYMMETRIC_EVEN, max_order=4, even_orders=(2, 4),
                                   atol=0.0, rtol=1e-12)
    if beta_legacy is not None:
        b = np.asarray(beta_legacy, dtype=float)
        if b.shape != (4,):
            raise ValueError("beta_legacy must have shape (4,)")
        return PhaseMatchingConfig(method=PhaseMatchingMethod.PROVIDED, max_order=0, even_orders=(2,), atol=0.0,
                                   rtol=1e-12, provided_delta_beta=float((b[2] + b[3]) - (b[0] + b[1])))
    raise ValueError("Provide either dispersion or beta_legacy (or an explicit phase_matching_cfg).")


def _prepare(cfg, *, gamma, alpha, dispersion, phase_matching_cfg, beta_legacy, length_unit):
    """Everything of run_single_simulation that does not depend on the frequency plan (shared with the sweep
    drivers, which run it once instead of once per point).  Returns a dict of per-metre quantities."""
    validate_config(cfg)
    scale = _length_scale_to_m(length_unit)
    legacy_m = None
    if beta_legacy is not None:
        b = np.asarray(list(beta_legacy), dtype=float)
        if b.shape != (4,):
            raise ValueError(f"beta_legacy must have shape (4,), got {b.shape}")
        if not np.all(np.isfinite(b)):
            raise ValueError("beta_legacy must be finite")
        legacy_m = b / scale
    disp_m = None
    if dispersion is not None:
        if not isinstance(dispersion, DispersionParams):
            raise TypeError("dispersion must be DispersionParams or None")
        disp_m = dispersion.scaled(scale)
    pm_cfg = phase_matching_cfg if phase_matching_cfg is not None else \
        _default_phase_matching_cfg(dispersion=disp_m, beta_legacy=legacy_m)
    if not isinstance(pm_cfg, PhaseMatchingConfig):
        raise TypeError("phase_matching_cfg must be PhaseMatchingConfig or None")
    fiber = FiberParams(length_m=float(cfg.z_max) * scale, gamma_W_m=float(gamma) / scale,
                        alpha_1_m=float(alpha) / scale, dispersion=disp_m, beta_legacy_1_m=legacy_m)
    grid = SimulationGrid(dz_m=float(cfg.dz) * scale, z0_m=0.0)
    return dict(scale=scale, fiber=fiber, grid=grid, pm=PhaseMatchingParams(config=pm_cfg.scaled(scale)))


def run_single_simulation(cfg: SimulationConfig, *, gamma: float, alpha: float, omega: Sequence[float],
                          p_in: Sequence[float], phase_in: Optional[Sequence[float]] = None,
                          dispersion: Optional[DispersionParams] = None,
                          phase_matching_cfg: Optional[PhaseMatchingConfig] = None,
                          beta_legacy: Optional[Sequence[float]] = None, length_unit: str = "m",
                          return_length_unit: Optional[str] = None) -> tuple[np.ndarray, np.ndarray]:
    """One propagation on the GPU -> (z_out in ``return_length_unit``, A complex128 (n_saved, 4))."""
    validate_config(cfg)
    _length_scale_to_m(length_unit)
    om = _to_omega_array(omega)
    A0 = make_initial_amplitudes(_to_power_array(p_in), phase_in)
    pre = _prepare(cfg, gamma=gamma, alpha=alpha, dispersion=dispersion, phase_matching_cfg=phase_matching_cfg,
                   beta_legacy=beta_legacy, length_unit=length_unit)
    params = make_model_params(waves=WavesParams(omega=om, symmetric=None), fiber=pre["fiber"], grid=pre["grid"],
                               phase_matching=pre["pm"])
    res = compute_phase_mismatch(params.waves.omega, params.fiber.dispersion, params.phase_matching.config,
                                 symmetric_hint=params.waves.symmetric)
    params.cache.set_phase_mismatch(res.delta_beta, symmetric=res.symmetric)
    z_m, A = integrate_interval(rhs_yaman_simplified, params.fiber.length_m, params.grid.dz_m, A0, params,
                                save_every=cfg.save_every, check_nan=cfg.check_nan)
    out_unit = length_unit if return_length_unit is None else return_length_unit
    return z_m / _length_scale_to_m(out_unit), A


def run_single_simulation_adaptive(cfg: SimulationConfig, *, tol: AdaptiveConfig = AdaptiveConfig(), gamma: float,
                                   alpha: float, omega: Sequence[float], p_in: Sequence[float],
                                   phase_in: Optional[Sequence[float]] = None,
                                   dispersion: Optional[DispersionParams] = None,
                                   phase_matching_cfg: Optional[PhaseMatchingConfig] = None,
                                   beta_legacy: Optional[Sequence[float]] = None, length_unit: str = "m",
                                   return_length_unit: Optional[str] = None) -> tuple[np.ndarray, np.ndarray]:
    """run_single_simulation integrated to the tolerance ``tol`` (adaptive RK45 on the GPU) -> (z_out, A (n_rows, 4)).

    z_out is the grid run_single_simulation(cfg, ...) returns, bit for bit: np.linspace(0, z_max, n_steps + 1)[::save_every]
    with n_steps = n_steps_of(z_max, dz) -- when save_every does not divide n_steps the last row lies short of z_max, as
    there.  The rows are the dense output at those z: cfg.dz and cfg.save_every only say where rows are sampled, the step
    is chosen by ``tol``, and the integration always runs to z_max.  tol.h_max and tol.first_step are lengths in
    ``length_unit``, like cfg.z_max and cfg.dz; rtol and atol are amplitude tolerances and take no unit.  With
    cfg.check_nan a non-finite state (status 1) raises FloatingPointError; running out of tol.max_steps (status 2) always
    raises RuntimeError."""
    validate_config(cfg)
    if not isinstance(tol, AdaptiveConfig):
        raise TypeError("tol must be an AdaptiveConfig")
    tol.validate()
    _length_scale_to_m(length_unit)
    om = _to_omega_array(omega)
    A0 = make_initial_amplitudes(_to_power_array(p_in), phase_in)
    pre = _prepare(cfg, gamma=gamma, alpha=alpha, dispersion=dispersion, phase_matching_cfg=phase_matching_cfg,
                   beta_legacy=beta_legacy, length_unit=length_unit)
    params = make_model_params(waves=WavesParams(omega=om, symmetric=None), fiber=pre["fiber"], grid=pre["grid"],
                               phase_matching=pre["pm"])
    res = compute_phase_mismatch(params.waves.omega, params.fiber.dispersion, params.phase_matching.config,
                                 symmetric_hint=params.waves.symmetric)
    params.cache.set_phase_mismatch(res.delta_beta, symmetric=res.symmetric)
    n_steps = n_steps_of(params.fiber.length_m, params.grid.dz_m)
    if n_steps < 1:
        raise ValueError("z_max / dz rounds to zero steps")
    scale = pre["scale"]
    tol_m = dataclasses.replace(tol, h_max=float(tol.h_max) * scale, first_step=float(tol.first_step) * scale)
    # every point of the fixed-step grid, then its stride: the same z values as integrate_interval's rows
    z_m, A, info = integrate_adaptive(rhs_yaman_simplified, params.fiber.length_m, A0, params, tol=tol_m, n_out=n_steps)
    se = int(cfg.save_every)
    z_m, A = z_m[::se].copy(), A[::se].copy()
    if info["status"] == 2:
        raise RuntimeError(f"adaptive integration used up max_steps = {tol.max_steps} attempts at z = {info['z_end']} "
                           f"of {params.fiber.length_m} m")
    if info["status"] == 1 and cfg.check_nan:
        raise FloatingPointError(f"NaN or Inf detected: adaptive step fell below the minimum at z = {info['z_end']}")
    out_unit = length_unit if return_length_unit is None else return_length_unit
    return z_m / _length_scale_to_m(out_unit), A


# ---- single-pump (degenerate) amplifier: one pump, a signal, an idler at 2 w_p - w_s ---------------------------------------
def _positive_omega(x, name: str) -> float:
    v = float(x)
    if not np.isfinite(v):
        raise ValueError(f"{name} must be finite")
    if v <= 0.0:
        raise ValueError(f"{name} must be positive (rad/s)")
    return v


def _single_pump_plan(omega_pump, omega_signal, p_in, phase_in) -> tuple[tuple[float, float, float], np.ndarray]:
    """The frequency plan and the input of the single-pump model -> ((w_p, w_s, w_i), A0 (3,)): both frequencies and the idler's
    2 w_p - w_s positive, three finite non-negative powers and three finite phases [pump, signal, idler]."""
    wp, ws = _positive_omega(omega_pump, "omega_pump"), _positive_omega(omega_signal, "omega_signal")
    wi = 2.0 * wp - ws
    if wi <= 0.0:
        raise ValueError("the idler frequency 2*omega_pump - omega_signal must be positive")
    return (wp, ws, wi), initial_amplitudes(_vec(p_in, "p_in", what="non-negative (W)", lower=0.0, n=3),
                                            np.zeros(3) if phase_in is None else _vec(phase_in, "phase_in", what="", n=3))


def _single_pump_mismatch(wp, ws, wi, dispersion: DispersionParams, max_order: int):
    """dbeta = beta(w_s) + beta(w_i) - 2 beta(w_p) of the single-pump model from the Taylor expansion of ``dispersion`` up to
    ``max_order``: delta_beta_from_omegas_array on [w_p, w_p, w_s, w_i].  Scalars give a scalar; w_s, w_i (n,) give (n,)."""
    om = np.empty(np.shape(ws) + (4,))
    om[..., 0], om[..., 1], om[..., 2], om[..., 3] = wp, wp, ws, wi
    return delta_beta_from_omegas_array(om, dispersion, max_order=max_order)


def _run_one(sweep, mismatch, cfg, pre, A0, out_unit, **options):
    """The end of the single-run functions of the wave-summary families: one point through ``sweep`` (rk4_sweep_single_pump or
    rk4_sweep_comb) with its saved rows, the failure at its step, and z_out in ``out_unit``."""
    fiber = pre["fiber"]
    n_steps = n_steps_of(fiber.length_m, pre["grid"].dz_m)
    r = sweep(mismatch, z_max=fiber.length_m, n_steps=n_steps, save_every=int(cfg.save_every), check_nan=bool(cfg.check_nan),
              gamma=fiber.gamma_W_m, alpha=fiber.alpha_1_m, a0=A0, want_traj=True, **options)
    z_m = np.linspace(0.0, fiber.length_m, n_steps + 1)
    bad = int(r.first_bad_step[0])
    if cfg.check_nan and bad >= 0:
        raise FloatingPointError(f"NaN or Inf detected at step {bad}, z = {z_m[bad]}")
    return z_m[::int(cfg.save_every)] / _length_scale_to_m(out_unit), r.traj[0]


def run_single_pump_simulation(cfg: SimulationConfig, *, gamma: float, alpha: float, omega_pump: float, omega_signal: float,
                               p_in: Sequence[float], phase_in: Optional[Sequence[float]] = None,
                               dispersion: DispersionParams, max_order: int = 4, length_unit: str = "m",
                               return_length_unit: Optional[str] = None) -> tuple[np.ndarray, np.ndarray]:
    """One propagation of the single-pump model on the GPU -> (z_out in ``return_length_unit``, A complex128 (n_saved, 3)),
    waves [pump, signal, idler] (no reference counterpart).  The idler sits at 2 omega_pump - omega_signal,
    which must be positive; dbeta = beta(w_s) + beta(w_i) - 2 beta(w_p) from the Taylor expansion of ``dispersion`` up to
    ``max_order`` (delta_beta_from_omegas_array on [w_p, w_p, w_s, w_i]).  Validation, units and the failure behaviour are
    run_single_simulation's: with cfg.check_nan a non-finite state raises FloatingPointError at its step."""
    validate_config(cfg)
    _length_scale_to_m(length_unit)
    plan, A0 = _single_pump_plan(omega_pump, omega_signal, p_in, phase_in)
    if dispersion is None:
        raise ValueError("dispersion must be provided")
    if not isinstance(max_order, int):
        raise TypeError("max_order must be int")
    if max_order < 0:
        raise ValueError("max_order must be >= 0")
    pre = _prepare(cfg, gamma=gamma, alpha=alpha, dispersion=dispersion, phase_matching_cfg=None, beta_legacy=None,
                   length_unit=length_unit)
    dbeta = float(_single_pump_mismatch(*plan, pre["fiber"].dispersion, max_order))
    if not np.isfinite(dbeta):
        raise ValueError("the phase mismatch is not finite")
    return _run_one(rk4_sweep_single_pump, [dbeta], cfg, pre, A0, length_unit if return_length_unit is None else return_length_unit,
                    exact_step=True)


# ---- multi-line ("comb") amplifier: M equally spaced lines, every FWM product among them ------------------------------------
def comb_lines(omega_center: float, line_spacing: float, n_lines: int, dispersion: DispersionParams, *,
               max_order: int = 4) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The lines of a comb -> (omega (M,), kappa (M,), b (M,)): line m at omega_center + (m - (M-1)/2) * line_spacing, b_m the
    Taylor sum of ``dispersion`` over the orders 2..max_order at that frequency and kappa_m = b_m - [b_0 + (b_{M-1} - b_0) *
    m / (M-1)], the same propagation constants in the gauge where the two outer lines have none.  beta_0 and beta_1 cancel in
    every product k + l - n = m, so they are left out rather than cancelled: the large beta_1 phase never reaches a sincos."""
    from math import factorial
    M = int(n_lines)
    if not 3 <= M <= MAX_LINES:
        raise ValueError(f"a comb has 3..{MAX_LINES} lines, got {M}")
    wc, dw = _positive_omega(omega_center, "omega_center"), float(line_spacing)
    if not np.isfinite(dw) or dw <= 0.0:
        raise ValueError("line_spacing must be positive and finite (rad/s)")
    if not isinstance(max_order, int):
        raise TypeError("max_order must be int")
    if max_order < 2:
        raise ValueError("max_order must be >= 2")
    if dispersion is None:
        raise ValueError("dispersion must be provided")
    m = np.arange(M, dtype=float)
    omega = wc + (m - 0.5 * (M - 1)) * dw
    if omega[0] <= 0.0:
        raise ValueError("the lowest line's frequency must be positive")
    x = omega - dispersion.omega_ref
    b = np.zeros(M)
    for n in range(2, max_order + 1):
        bn = dispersion.get_beta_n(n)
        if bn != 0.0:
            b = b + bn * (x**n) / float(factorial(n))
    kappa = b - (b[0] + (b[-1] - b[0]) * m / (M - 1))
    if not np.all(np.isfinite(kappa)):
        raise ValueError("the lines' propagation constants are not finite")
    return omega, kappa, b


def _comb_input(p, name: str, phase_in, *, points: bool = False) -> tuple[np.ndarray, np.ndarray]:
    """The input of the multi-line model -> (the powers, A0 of their shape): ``p`` (called ``name``) finite non-negative powers
    of M = 3..MAX_LINES lines, (M,) -- or, where the sweep points are power settings (``points``), (M,) or (N, M), returned as
    (N, M) --, phase_in None or M finite phases."""
    p = np.asarray(p, dtype=float)
    if p.ndim not in (1, 2) or p.size == 0 or not 3 <= p.shape[-1] <= MAX_LINES:
        raise ValueError(f"{name} must have shape (M,) or (N, M) with 3 <= M <= {MAX_LINES}, got {p.shape}")
    if not np.all(np.isfinite(p)) or np.any(p < 0.0):
        raise ValueError(f"{name} must hold finite non-negative powers (W)")
    if points:
        p = np.atleast_2d(p)
    elif p.ndim != 1:
        raise ValueError(f"{name} must have shape (M,), got {p.shape}")
    M = int(p.shape[-1])
    ph = None
    if phase_in is not None:
        ph = np.asarray(phase_in, dtype=float)
        if ph.shape != (M,) or not np.all(np.isfinite(ph)):
            raise ValueError(f"phase_in must hold {M} finite phases")
    return p, initial_amplitudes(p, ph)


def run_comb_simulation(cfg: SimulationConfig, *, gamma: float, alpha: float, omega_center: float, line_spacing: float,
                        p_in: Sequence[float], phase_in: Optional[Sequence[float]] = None, dispersion: DispersionParams,
                        max_order: int = 4, length_unit: str = "m") -> tuple[np.ndarray, np.ndarray]:
    """One propagation of the multi-line ("comb") model on the GPU -> (z_out in ``length_unit``, A complex128 (n_saved, M)):
    M = len(p_in) = 3..12 lines at omega_center + (m - (M-1)/2) * line_spacing (rad/s), ascending in frequency, with every
    FWM product among them (no reference counterpart; see comb_lines for the propagation constants).
    Validation, units and the failure behaviour are run_single_simulation's: with cfg.check_nan a non-finite state raises
    FloatingPointError at its step."""
    validate_config(cfg)
    _length_scale_to_m(length_unit)
    p, A0 = _comb_input(p_in, "p_in", phase_in)
    if dispersion is None:
        raise ValueError("dispersion must be provided")
    pre = _prepare(cfg, gamma=gamma, alpha=alpha, dispersion=dispersion, phase_matching_cfg=None, beta_legacy=None,
                   length_unit=length_unit)
    _, kappa, _ = comb_lines(omega_center, line_spacing, int(p.shape[0]), pre["fiber"].dispersion, max_order=max_order)
    return _run_one(rk4_sweep_comb, kappa[None, :], cfg, pre, A0, length_unit)


# ---- concatenated spans (copier - mid-stage - PSA chains) ------------------------------------------------------------
def _mid_stage(name: str, widths, gain_db, phase) -> np.ndarray:
    g, ph = np.broadcast_arrays(np.asarray(gain_db, dtype=float), np.asarray(phase, dtype=float))
    if g.ndim == 0 or g.shape[-1] not in widths:
        raise ValueError(f"{name}: gain_db / phase need one entry per wave ({' or '.join(map(str, widths))})")
    if not (np.all(np.isfinite(g)) and np.all(np.isfinite(ph))):
        raise ValueError(f"{name}: gain_db and phase must be finite")
    return np.sqrt(10.0 ** (g / 10.0)) * np.exp(1j * ph)


def mid_stage(gain_db=(0.0, 0.0, 0.0, 0.0), phase=(0.0, 0.0, 0.0, 0.0)) -> np.ndarray:
    """Per-wave transfer of a mid-stage (pump recovery, attenuator, phase shifter): sqrt(10^(gain_db/10)) e^{i phase}.
    The last axis is the wave (4 or 6); leading axes (one row per sweep point) broadcast."""
    return _mid_stage("mid_stage", (4, 6), gain_db, phase)


def wdm_mid_stage(gain_db, phase) -> np.ndarray:
    """mid_stage for the multi-channel model's NW = 2 + 2K waves [p1, p2, s_1, i_1, ..., s_K, i_K], K = 1..16:
    sqrt(10^(gain_db/10)) e^{i phase}.  The last axis is the wave (4, 6, ..., 34 entries); leading axes (one row per sweep
    point) broadcast."""
    return _mid_stage("wdm_mid_stage", tuple(range(4, 36, 2)), gain_db, phase)


def _run_spans(chain, fibre, cfgs, A0, transfers, length_unit, return_length_unit):
    """The end of every run_concatenated_* function: the rules the spans' configs and the transfers share, the chain call
    (``chain``: rk4_chain, rk4_chain_single_pump or rk4_chain_comb, on A0's waves), the failure and the unit of z_out."""
    save_every, check_nan = int(cfgs[0].save_every), bool(cfgs[0].check_nan)
    if any(int(c.save_every) != save_every or bool(c.check_nan) != check_nan for c in cfgs):
        raise ValueError("all spans must share save_every and check_nan")
    if transfers is not None:
        transfers = [np.asarray(t, dtype=np.complex128) for t in transfers]
        if len(transfers) != len(fibre) - 1 or any(t.shape != A0.shape for t in transfers):
            raise ValueError(f"transfers must be {len(fibre) - 1} per-wave factors of shape ({A0.shape[0]},)")
    r = chain(fibre, a0=A0, transfers=transfers, save_every=save_every, check_nan=check_nan, exact_step=True, want_traj=True)
    bad = int(r.first_bad_step[0])
    if check_nan and bad >= 0:
        k = int(np.searchsorted(r.step_offsets, bad, side="right")) - 1
        raise FloatingPointError(f"NaN or Inf detected at step {bad} (span {k}, local step {bad - r.step_offsets[k]})")
    out_unit = length_unit if return_length_unit is None else return_length_unit
    return r.z_out / _length_scale_to_m(out_unit), r.traj[0]


def _span_list(spans, length_unit) -> list:
    """What every run_concatenated_* function checks before its frequency plan: at least one span and a known unit."""
    spans = list(spans)
    if not spans:
        raise ValueError("spans must name at least one span")
    _length_scale_to_m(length_unit)
    return spans


def _run_span_maps(chain, spans, A0, transfers, length_unit, return_length_unit, *, optional, needs, mismatch_of, required=(),
                   rules=None):
    """The span loop of every run_concatenated_* function, then _run_spans: each mapping of ``spans`` holds cfg, gamma, alpha,
    the keys ``required`` (present and not None) and any of ``optional``, or the error names what it ``needs``;
    ``rules(k, span)`` are the family's own rules on the mapping, _prepare scales the span to metres, and
    ``mismatch_of(k, span, prepared)`` is its per-metre mismatch (a scalar, or the lines' propagation constants)."""
    fibre, cfgs, known = [], [], {"cfg", "gamma", "alpha", *required, *optional}
    for k, sp in enumerate(spans):
        sp = dict(sp)
        unknown = set(sp) - known
        if unknown or "cfg" not in sp or "gamma" not in sp or "alpha" not in sp or any(sp.get(key) is None for key in required):
            raise ValueError(f"span {k}: needs cfg, gamma, alpha{needs}; unknown keys {sorted(unknown)}")
        if rules is not None:
            rules(k, sp)
        pre = _prepare(sp["cfg"], gamma=sp["gamma"], alpha=sp["alpha"], dispersion=sp.get("dispersion"),
                       phase_matching_cfg=sp.get("phase_matching_cfg"), beta_legacy=sp.get("beta_legacy"),
                       length_unit=length_unit)
        fiber = pre["fiber"]
        fibre.append(FibreSpan(length=fiber.length_m, dz=pre["grid"].dz_m, dbeta=mismatch_of(k, sp, pre), gamma=fiber.gamma_W_m,
                               alpha=fiber.alpha_1_m))
        cfgs.append(sp["cfg"])
    return _run_spans(chain, fibre, cfgs, A0, transfers, length_unit, return_length_unit)


def run_concatenated_simulation(spans, *, omega: Sequence[float], p_in: Sequence[float],
                                phase_in: Optional[Sequence[float]] = None, transfers=None, length_unit: str = "m",
                                return_length_unit: Optional[str] = None) -> tuple[np.ndarray, np.ndarray]:
    """run_single_simulation over a chain of spans -> (z_out, A complex128 (n_saved_total, 4)).

    ``spans``: one mapping per span with ``cfg`` (SimulationConfig: length z_max, dz, save_every, check_nan), ``gamma``,
    ``alpha`` and one of ``dispersion`` / ``phase_matching_cfg`` / ``beta_legacy``, all in ``length_unit``.  Each span's
    dbeta comes from compute_phase_mismatch exactly as in run_single_simulation.  ``transfers``: None or S-1 complex
    (4,) per-wave factors (mid_stage).  The FWM phase accumulates over the spans; rows are those of every span in order,
    each span's z = 0 row being the post-transfer state (z repeats at a boundary).  save_every and check_nan must agree
    between spans; with check_nan a non-finite state raises FloatingPointError at the chain's step index."""
    spans = _span_list(spans, length_unit)
    om = _to_omega_array(omega)
    A0 = make_initial_amplitudes(_to_power_array(p_in), phase_in)

    def mismatch_of(k, sp, pre):
        params = make_model_params(waves=WavesParams(omega=om, symmetric=None), fiber=pre["fiber"], grid=pre["grid"],
                                   phase_matching=pre["pm"])
        return float(compute_phase_mismatch(params.waves.omega, params.fiber.dispersion, params.phase_matching.config,
                                            symmetric_hint=params.waves.symmetric).delta_beta)

    return _run_span_maps(rk4_chain, spans, A0, transfers, length_unit, return_length_unit,
                          optional=("dispersion", "phase_matching_cfg", "beta_legacy"),
                          needs=" (+ dispersion / phase_matching_cfg / beta_legacy)", mismatch_of=mismatch_of)


def single_pump_mid_stage(gain_db=(0.0, 0.0, 0.0), phase=(0.0, 0.0, 0.0)) -> np.ndarray:
    """mid_stage for the single-pump model's three waves [p, s, i]: sqrt(10^(gain_db/10)) e^{i phase}.  The last axis is the
    wave (3 entries); leading axes (one row per sweep point) broadcast."""
    return _mid_stage("single_pump_mid_stage", (3,), gain_db, phase)


def run_concatenated_single_pump_simulation(spans, *, omega_pump: float, omega_signal: float, p_in: Sequence[float],
                                            phase_in: Optional[Sequence[float]] = None, transfers=None,
                                            length_unit: str = "m",
                                            return_length_unit: Optional[str] = None) -> tuple[np.ndarray, np.ndarray]:
    """run_single_pump_simulation over a chain of spans -> (z_out, A complex128 (n_saved_total, 3)), waves [p, s, i].

    ``spans``: one mapping per span with ``cfg`` (SimulationConfig: length z_max, dz, save_every, check_nan), ``gamma``,
    ``alpha`` and either ``dispersion`` (with an optional ``max_order``, default 4: dbeta = beta(w_s) + beta(w_i) -
    2 beta(w_p) from delta_beta_from_omegas_array on [w_p, w_p, w_s, 2 w_p - w_s], as run_single_pump_simulation forms it)
    or a ``phase_matching_cfg`` of method PROVIDED carrying the span's dbeta, all in ``length_unit``.  ``transfers``: None
    or S-1 complex (3,) per-wave factors (single_pump_mid_stage).  The FWM phase accumulates over the spans; rows are those
    of every span in order, each span's z = 0 row being the post-transfer state (z repeats at a boundary).  save_every and
    check_nan must agree between spans; with check_nan a non-finite state raises FloatingPointError at the chain's step
    index."""
    spans = _span_list(spans, length_unit)
    plan, A0 = _single_pump_plan(omega_pump, omega_signal, p_in, phase_in)

    def rules(k, sp):
        pm = sp.get("phase_matching_cfg")
        if (pm is None) == (sp.get("dispersion") is None):
            raise ValueError(f"span {k}: needs exactly one of dispersion and phase_matching_cfg")
        if pm is not None and (not isinstance(pm, PhaseMatchingConfig) or pm.method != PhaseMatchingMethod.PROVIDED):
            raise ValueError(f"span {k}: phase_matching_cfg must be a PhaseMatchingConfig of method PROVIDED")
        max_order = sp.get("max_order", 4)
        if not isinstance(max_order, int) or max_order < 0:
            raise ValueError(f"span {k}: max_order must be a non-negative int")

    def mismatch_of(k, sp, pre):
        if sp.get("phase_matching_cfg") is not None:
            dbeta = float(pre["pm"].config.provided_delta_beta)
        else:
            dbeta = float(_single_pump_mismatch(*plan, pre["fiber"].dispersion, sp.get("max_order", 4)))
        if not np.isfinite(dbeta):
            raise ValueError(f"span {k}: the phase mismatch is not finite")
        return dbeta

    return _run_span_maps(rk4_chain_single_pump, spans, A0, transfers, length_unit, return_length_unit,
                          optional=("dispersion", "max_order", "phase_matching_cfg"), needs=" (+ dispersion / phase_matching_cfg)",
                          rules=rules, mismatch_of=mismatch_of)


def comb_mid_stage(gain_db, phase) -> np.ndarray:
    """mid_stage for the multi-line model's M = 3..12 lines, ascending in frequency: sqrt(10^(gain_db/10)) e^{i phase}.  The
    last axis is the line (3..12 entries); leading axes (one row per sweep point) broadcast."""
    return _mid_stage("comb_mid_stage", tuple(range(3, MAX_LINES + 1)), gain_db, phase)


def run_concatenated_comb_simulation(spans, *, omega_center: float, line_spacing: float, p_in: Sequence[float],
                                     phase_in: Optional[Sequence[float]] = None, transfers=None, length_unit: str = "m",
                                     return_length_unit: Optional[str] = None) -> tuple[np.ndarray, np.ndarray]:
    """run_comb_simulation over a chain of spans -> (z_out, A complex128 (n_saved_total, M)), lines ascending in frequency.

    ``spans``: one mapping per span with ``cfg`` (SimulationConfig: length z_max, dz, save_every, check_nan), ``gamma``,
    ``alpha`` and ``dispersion`` (with an optional ``max_order``, default 4), all in ``length_unit``; the span's propagation
    constants are comb_lines' kappa on that span's dispersion.  ``transfers``: None or S-1 complex (M,) per-line factors
    (comb_mid_stage).  Every line's phase accumulates over the spans; rows are those of every span in order, each span's
    z = 0 row being the post-transfer state (z repeats at a boundary).  save_every and check_nan must agree between spans;
    with check_nan a non-finite state raises FloatingPointError at the chain's step index."""
    spans = _span_list(spans, length_unit)
    p, A0 = _comb_input(p_in, "p_in", phase_in)
    return _run_span_maps(rk4_chain_comb, spans, A0, transfers, length_unit, return_length_unit, required=("dispersion",),
                          optional=("max_order",), needs=" and dispersion (+ max_order)",
                          mismatch_of=lambda k, sp, pre: comb_lines(omega_center, line_spacing, int(p.shape[0]),
                                                                    pre["fiber"].dispersion, max_order=sp.get("max_order", 4))[1])


# ---- the reference's two ready-made scenarios (simulation.py:371-447), km-unit path -----------------------
def _omega_1550x4() -> np.ndarray:
    return np.full(4, 2.0 * np.pi * constants.c / 1.55e-6)


def example_zero_signal() -> tuple[np.ndarray, np.ndarray]:
    """Two 0.5 W pumps, no signal/idler, dbeta = 0, gamma = 1.3 /(W km), 0.5 km in 1e-3 km steps."""
    pm = PhaseMatchingConfig(method=PhaseMatchingMethod.PROVIDED, provided_delta_beta=0.0)
    return run_single_simulation(default_simulation_config(), gamma=1.3, alpha=0.0, omega=_omega_1550x4(),
                                 p_in=np.array([0.5, 0.5, 0.0, 0.0]), phase_matching_cfg=pm, length_unit="km",
                                 return_length_unit="km")


def custom_seeded_signal() -> tuple[np.ndarray, np.ndarray]:
    """0.1 W pumps, 1e-4 / 1e-6 W seeds, dbeta = 0, gamma = 10 /(W km), 0.5 km in 1e-4 km steps."""
    pm = PhaseMatchingConfig(method=PhaseMatchingMethod.PROVIDED, provided_delta_beta=0.0)
    return run_single_simulation(custom_simulation_config(z_max=0.5, dz=1e-4), gamma=10.0, alpha=0.0,
                                 omega=_omega_1550x4(), p_in=np.array([1e-1, 1e-1, 1e-4, 1e-6]), phase_in=np.zeros(4),
                                 phase_matching_cfg=pm, length_unit="km", return_length_unit="km")
