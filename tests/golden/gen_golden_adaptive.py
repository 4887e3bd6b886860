#!/usr/bin/env python3
"""Generate G18.npz: the adaptive (RK45) fixtures, from the reference's own right-hand side driven by scipy.

Runs ONLY where the upstream reference is mounted read-only (PSA_REFERENCE, default /root/reference) and scipy is
installed.  Every case integrates yaman_model.rhs_yaman_simplified, through a ModelParams built as gen_golden.py builds
one (PROVIDED dbeta), with scipy.integrate.solve_ivp(method="RK45").  Nothing from the reference is copied: the outputs
are data (inputs -> expected outputs) stored as .npz without pickles.

    MPLBACKEND=Agg PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_adaptive.py

Cases (prefix in the archive):
  g1_r6, g1_r9, g1_r11   G1 inputs (L = 1000 m) at rtol 1e-6 / 1e-9 / 1e-11; g1_r9 also the 1 001 dense rows at
                         t_eval = linspace(0, 1000, 1001)
  sw                     a 64-point dbeta sweep, linspace(-0.05, 0.05, 64), BASELINE config-2 inputs, rtol 1e-9
  zero                   simulation.example_zero_signal in metres (zero signal and idler: the atol branch of the scale)
  g9                     the G9 gammas with max_steps = 100 000: gamma <= 12 from scipy; gamma >= 50 use up the cap, which
                         scipy does not have, so their record (status 2, z_end, A_end, counts) comes from tests/rk45_np.py
Per case: inputs, rtol / atol, A_end, p_max over accepted steps, accepted / rejected counts (from t.size and nfev: 2 + 6
per attempt with the selected first step), status and t[-1].
"""
from __future__ import annotations

import os
import sys

os.environ.setdefault("MPLBACKEND", "Agg")
sys.dont_write_bytecode = True
REF = os.environ.get("PSA_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REF)

import numpy as np  # noqa: E402

ATOL = 1e-12
P_C2 = np.array([0.5, 0.5, 1e-5, 1e-5])


def _params(gamma, alpha, dbeta, z_max):
    from parameters import FiberParams, PhaseMatchingParams, SimulationGrid, WavesParams, make_model_params
    from phase_matching import PhaseMatchingConfig, PhaseMatchingMethod
    w0 = 2 * np.pi * 299792458.0 / 1.55e-6
    pm = PhaseMatchingParams(config=PhaseMatchingConfig(method=PhaseMatchingMethod.PROVIDED,
                                                        provided_delta_beta=float(dbeta)))
    p = make_model_params(waves=WavesParams(omega=np.full(4, w0), symmetric=None),
                          fiber=FiberParams(length_m=float(z_max), gamma_W_m=float(gamma), alpha_1_m=float(alpha)),
                          grid=SimulationGrid(dz_m=float(z_max) / 10.0, z0_m=0.0), phase_matching=pm)
    p.cache.set_phase_mismatch(float(dbeta))
    return p


def _solve(gamma, alpha, dbeta, z_max, p_in, rtol, n_out=0):
    from scipy.integrate import solve_ivp
    from yaman_model import rhs_yaman_simplified
    params = _params(gamma, alpha, dbeta, z_max)
    y0 = np.sqrt(p_in).astype(np.complex128)
    fun = lambda z, y: rhs_yaman_simplified(z, y, params)  # noqa: E731
    r = solve_ivp(fun, (0.0, float(z_max)), y0, method="RK45", rtol=rtol, atol=ATOL)
    attempts = (r.nfev - 2) // 6
    acc = r.t.size - 1
    out = dict(a_end=r.y[:, -1], p_max=np.max(np.abs(r.y[2]) ** 2), n_accepted=acc, n_rejected=attempts - acc,
               status=0 if r.status == 0 else 1, z_end=r.t[-1])
    if n_out:
        rr = solve_ivp(fun, (0.0, float(z_max)), y0, method="RK45", rtol=rtol, atol=ATOL,
                       t_eval=np.linspace(0.0, float(z_max), n_out + 1))
        out["rows"] = rr.y.T
    return out


def _stack(recs, key):
    return np.array([r[key] for r in recs])


def main() -> None:
    G1 = np.load(os.path.join(HERE, "G1.npz"))
    g1 = dict(gamma=float(G1["gamma"]), alpha=float(G1["alpha"]), dbeta=float(G1["dbeta_sym"]), z_max=1000.0,
              p_in=G1["p_in"])
    out = {}

    def put(prefix, recs, **inputs):
        for k in ("a_end", "p_max", "n_accepted", "n_rejected", "status", "z_end"):
            out[f"{prefix}_{k}"] = _stack(recs, k)
        for k, v in inputs.items():
            out[f"{prefix}_{k}"] = np.asarray(v)

    for tag, rtol in (("g1_r6", 1e-6), ("g1_r9", 1e-9), ("g1_r11", 1e-11)):
        rec = _solve(g1["gamma"], g1["alpha"], g1["dbeta"], g1["z_max"], g1["p_in"], rtol,
                     n_out=1000 if tag == "g1_r9" else 0)
        put(tag, [rec], dbeta=[g1["dbeta"]], gamma=g1["gamma"], alpha=g1["alpha"], p_in=g1["p_in"], z_max=g1["z_max"],
            rtol=rtol, atol=ATOL, max_steps=1_000_000)
        if "rows" in rec:
            out[f"{tag}_rows"] = rec["rows"]
            out[f"{tag}_n_out"] = np.asarray(1000)
        print(tag, rec["n_accepted"], rec["n_rejected"], flush=True)

    db = np.linspace(-0.05, 0.05, 64)
    recs = [_solve(0.0115, 1.15e-4, d, 1000.0, P_C2, 1e-9) for d in db]
    put("sw", recs, dbeta=db, gamma=0.0115, alpha=1.15e-4, p_in=P_C2, z_max=1000.0, rtol=1e-9, atol=ATOL,
        max_steps=1_000_000)
    print("sw", _stack(recs, "n_accepted").min(), _stack(recs, "n_accepted").max(), flush=True)

    # simulation.example_zero_signal in metres: 0.5 km -> 500 m, gamma 1.3 /(W km) -> 1.3e-3 /(W m)
    p0 = np.array([0.5, 0.5, 0.0, 0.0])
    rec = _solve(1.3e-3, 0.0, 0.0, 500.0, p0, 1e-9)
    put("zero", [rec], dbeta=[0.0], gamma=1.3e-3, alpha=0.0, p_in=p0, z_max=500.0, rtol=1e-9, atol=ATOL,
        max_steps=1_000_000)

    G9 = np.load(os.path.join(HERE, "G9.npz"))
    gammas = G9["gammas"]
    cap = 100_000
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import rk45_np
    recs = []
    capped = gammas >= 50.0
    np_run = rk45_np.rk45(rk45_np.rhs4(np.full(capped.sum(), 0.01), gammas[capped], 0.0),
                          np.repeat(np.sqrt(P_C2).astype(complex)[:, None], capped.sum(), axis=1), 100.0,
                          rtol=1e-9, atol=ATOL, max_steps=cap)
    k = 0
    for g, c in zip(gammas, capped):
        if c:
            recs.append({key: np_run[key][k] for key in ("a_end", "p_max", "n_accepted", "n_rejected", "status", "z_end")})
            k += 1
        else:
            recs.append(_solve(float(g), 0.0, 0.01, 100.0, P_C2, 1e-9))
            assert recs[-1]["n_accepted"] + recs[-1]["n_rejected"] <= cap
        print("g9", g, recs[-1]["status"], recs[-1]["n_accepted"], recs[-1]["n_rejected"], recs[-1]["z_end"], flush=True)
    put("g9", recs, dbeta=np.full(gammas.size, 0.01), gamma=gammas, alpha=0.0, p_in=P_C2, z_max=100.0, rtol=1e-9,
        atol=ATOL, max_steps=cap)

    path = os.path.join(HERE, "G18.npz")
    np.savez_compressed(path, **out)
    print(f"wrote G18.npz ({os.path.getsize(path)} B)")


if __name__ == "__main__":
    main()
