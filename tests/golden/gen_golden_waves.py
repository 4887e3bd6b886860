#!/usr/bin/env python3
"""Writes tests/golden/G16.npz: per-wave end / max powers from the REFERENCE (run on CPU), for the per-wave summary
(psa_rk4_sweep_waves_*, scan_dbeta_seeded_signal(with_idler=True), seeded_mismatch_scan).

  (a) "seed_*": the scenario hard-coded in the reference's scan_mismatch_seeded_signal (scan_mismtach.py:56-93), repaired:
      run_single_simulation(beta_legacy=betas, length_unit="km") where upstream passes beta=.  All 200 points; per point the
      end and max of |A_j|^2 of every wave (200, 4), and per gain_mode the reference's Gs, Gi and best index, computed with
      its own _select_power_metric and eps (:110, :139-153, :183-186).
  (b) "lossy_*": 65 PROVIDED-dbeta points over G8's range, 1e4 steps over 1000 m, alpha = 1.15e-4, save_every = 10, seeded
      idler: the pumps' maximum is at z = 0, the signal's and idler's later.
  (c) "fail_*": G9's gammas past the RK4 stability edge with check_nan=False (NaNs stored silently), so np.max of a wave
      that goes non-finite is NaN.

Usage: python tests/golden/gen_golden_waves.py   (PSA_REFERENCE=<reference tree>; a few seconds with a process pool)
"""
from __future__ import annotations

import os
import sys
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402  (puts the reference on sys.path)

SEED_DELTA = np.linspace(-40.0, 40.0, 200)
LOSSY_DBETA = np.linspace(-0.05, 0.05, 65)
FAIL_GAMMAS = np.array([50.0, 200.0, 1e3, 12.0, 10.29664, 10.0])


def _wave_powers(A):
    P = np.abs(A) ** 2
    return P[-1].copy(), np.max(P, axis=0)


def _seed_point(delta):
    import config
    import simulation
    cfg = config.custom_simulation_config(z_max=0.5, dz=1e-3)
    betas = 5.8e9 * np.ones(4, dtype=float) + np.array([0.0, 0.0, 0.0, delta], dtype=float)
    omega = 299792458.0 / 1.55e-6 * np.ones(4, dtype=float)
    z, A = simulation.run_single_simulation(cfg, gamma=10.0, alpha=0.0, beta_legacy=betas, omega=omega,
                                            p_in=np.array([0.1, 0.1, 1e-5, 0.0]), phase_in=None, length_unit="km")
    return A


def _lossy_point(dbeta):
    z, A = G._provided_run(1000.0, 0.1, 10, float(dbeta), 0.0115, 1.15e-4, np.array([0.5, 0.5, 1e-5, 1e-5]))
    return _wave_powers(A)


def _fail_point(gamma):
    with np.errstate(all="ignore"):
        z, A = G._provided_run(100.0, 0.1, 10, 0.01, float(gamma), 0.0, np.array([0.5, 0.5, 1e-5, 1e-5]), check_nan=False)
        return _wave_powers(A)


def main() -> None:
    import scan_mismtach as ref_sm
    out = {}
    with Pool() as pool:
        seeds = pool.map(_seed_point, [float(d) for d in SEED_DELTA], chunksize=8)
        lossy = pool.map(_lossy_point, [float(d) for d in LOSSY_DBETA], chunksize=2)
        fail = pool.map(_fail_point, [float(g) for g in FAIL_GAMMAS])
    eps = 1e-30
    Pi0_ref = 1e-5
    out["seed_delta"] = SEED_DELTA
    out["seed_p_wave_end"] = np.array([_wave_powers(A)[0] for A in seeds])
    out["seed_p_wave_max"] = np.array([_wave_powers(A)[1] for A in seeds])
    for mode in ("end", "max"):
        Gs, Gi = np.empty(SEED_DELTA.size), np.empty(SEED_DELTA.size)
        for k, A in enumerate(seeds):
            P = np.abs(A) ** 2
            Ps, Pi = P[:, 2], P[:, 3]
            Gs[k] = ref_sm._select_power_metric(Ps, mode) / (float(Ps[0]) + eps)
            Gi[k] = ref_sm._select_power_metric(Pi, mode) / (Pi0_ref + eps)
        best = int(np.argmax(Gs))
        out[f"seed_{mode}_Gs"], out[f"seed_{mode}_Gi"], out[f"seed_{mode}_best_idx"] = Gs, Gi, best
        print(f"  seed {mode}: best_delta {SEED_DELTA[best]:.6g} 1/km, Gs {Gs[best]:.6g}, Gi {Gi[best]:.6g}", flush=True)
    out["lossy_dbeta"] = LOSSY_DBETA
    out["lossy_p_wave_end"] = np.array([r[0] for r in lossy])
    out["lossy_p_wave_max"] = np.array([r[1] for r in lossy])
    out["fail_gammas"] = FAIL_GAMMAS
    out["fail_p_wave_end"] = np.array([r[0] for r in fail])
    out["fail_p_wave_max"] = np.array([r[1] for r in fail])
    G._save("G16", seed_gamma=10.0, seed_p_in=np.array([0.1, 0.1, 1e-5, 0.0]), seed_z_max_km=0.5, seed_dz_km=1e-3,
            lossy_gamma=0.0115, lossy_alpha=1.15e-4, lossy_z_max=1000.0, lossy_n_steps=10_000, lossy_save_every=10,
            fail_dbeta=0.01, fail_z_max=100.0, fail_dz=0.1, fail_save_every=10, p_in=np.array([0.5, 0.5, 1e-5, 1e-5]),
            **out)


if __name__ == "__main__":
    main()
