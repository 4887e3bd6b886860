#!/usr/bin/env python3
"""Writes tests/golden/G17.npz: chains of fibre spans from the REFERENCE (run on CPU), for psa_rk4_chain_* / rk4_chain /
run_concatenated_simulation / scan_copier_psa_phase.

The reference integrates one uniform fibre, so a chain is a sequence of its run_single_simulation calls with a PROVIDED
dbeta per span (gen_golden._provided_run).  Each call starts from p_in = |B|^2, phase_in = arg B, and between calls this
script applies the transfer and the gauge: the FWM phase of span s is Theta_s + dbeta_s * zeta (Theta_s = sum_{k<s}
dbeta_k L_k), which the reference's e^{i dbeta z} with z restarting at 0 reproduces on B_sig = A_sig e^{i Theta_s}; so the
next span starts from B' = T_s B with the signal also times e^{i dbeta_s L_s}, and the signal column of span s's rows is
rotated back by e^{-i Theta_s}.  Rows of every span are stored in order, each span's z = 0 row included.

  (a) "split*": a G8-like fibre (1000 m, dz = 0.1, gamma 0.0115, alpha 1.15e-4, save_every 10, 5 dbeta points) run whole
      and cut into 2 and 3 spans with identity transfers: rows, z and per-point A_end.
  (b) "lossy_*": three spans with unequal dbeta, gamma, alpha and non-identity transfers, 5 input phases: rows, z.
  (c) "scan_*": a copier - mid-stage - PSA scan: 32 mid-stage pump phases x 2 PSA-span dbeta values; A_end and the
      signal's max over every saved row of the chain for each of the 64 points.

Usage: python tests/golden/gen_golden_chain.py   (PSA_REFERENCE=<reference tree>; about a minute with a process pool)
"""
from __future__ import annotations

import os
import sys
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402  (puts the reference on sys.path)

# (a)
SPLIT_DBETA = np.linspace(-0.05, 0.05, 5)
SPLIT_P_IN = np.array([0.5, 0.5, 1e-5, 1e-5])
SPLIT_STEPS = {1: [10_000], 2: [5_000, 5_000], 3: [3_330, 3_330, 3_340]}
# (b): (length, dz, dbeta, gamma, alpha) per span
LOSSY_SPANS = np.array([[300.0, 0.5, 0.011, 0.0115, 1.2e-4], [200.0, 0.5, -0.007, 0.02, 0.0],
                        [250.0, 0.5, 0.019, 0.009, 2e-4]])
LOSSY_GAIN_DB = np.array([[-1.0, -2.0, 0.5, -3.0], [0.0, 0.0, 0.0, -1.0]])
LOSSY_PHASE = np.array([[0.3, -0.2, 1.1, 0.0], [0.0, 2.0, 0.0, 0.4]])
LOSSY_P_IN = np.array([0.5, 0.5, 1e-5, 1e-6])
LOSSY_PHASE_IN = np.linspace(-1.0, 1.0, 5)            # input signal phase per point
# (c)
SCAN_P_IN = np.array([0.5, 0.5, 1e-5, 0.0])
SCAN_GAMMA, SCAN_ALPHA = 0.0115, 1e-4
SCAN_COPIER = (500.0, 0.5, -0.0115)                   # length, dz, dbeta
SCAN_PSA = (500.0, 0.5)
SCAN_PSA_DBETA = np.array([-0.0115, -0.005])
SCAN_MID_GAIN_DB = np.array([0.0, 0.0, 0.0, -3.0])
SCAN_PHASES = np.linspace(0.0, 2.0 * np.pi, 32, endpoint=False)   # added to both pumps
SAVE_EVERY = 10


def _transfer(gain_db, phase):
    return np.sqrt(10.0 ** (np.asarray(gain_db, dtype=float) / 10.0)) * np.exp(1j * np.asarray(phase, dtype=float))


def ref_chain(spans, transfers, a0, save_every):
    """spans: (length, dz, dbeta, gamma, alpha) rows; transfers: S-1 complex (4,).  -> (z, A rows in the physical frame)."""
    theta, z0, b, zs, rows = 0.0, 0.0, np.asarray(a0, dtype=complex), [], []
    for k, (L, dz, db, g, al) in enumerate(spans):
        z, B = G._provided_run(float(L), float(dz), save_every, float(db), float(g), float(al), np.abs(b) ** 2,
                               phase=np.angle(b))
        A = np.array(B, dtype=complex)
        A[:, 2] *= np.exp(-1j * theta)
        rows.append(A)
        zs.append(z0 + np.asarray(z))
        if k + 1 < len(spans):
            b = A[-1] * transfers[k]          # in the A frame, then into span k+1's gauge
            theta += float(db) * float(L)
            b[2] *= np.exp(1j * theta)
            z0 += float(L)
    return np.concatenate(zs), np.concatenate(rows)


def _split_point(args):
    cuts, db = args
    spans = [(s * 0.1, 0.1, db, 0.0115, 1.15e-4) for s in SPLIT_STEPS[cuts]]
    return ref_chain(spans, [np.ones(4)] * (cuts - 1), np.sqrt(SPLIT_P_IN).astype(complex), SAVE_EVERY)


def _lossy_point(phi):
    a0 = np.sqrt(LOSSY_P_IN).astype(complex)
    a0[2] *= np.exp(1j * phi)
    tr = [_transfer(g, p) for g, p in zip(LOSSY_GAIN_DB, LOSSY_PHASE)]
    return ref_chain(LOSSY_SPANS, tr, a0, SAVE_EVERY)


def _scan_point(args):
    phi, db_psa = args
    L1, dz1, db1 = SCAN_COPIER
    L2, dz2 = SCAN_PSA
    spans = [(L1, dz1, db1, SCAN_GAMMA, SCAN_ALPHA), (L2, dz2, db_psa, SCAN_GAMMA, SCAN_ALPHA)]
    tr = [_transfer(SCAN_MID_GAIN_DB, np.array([phi, phi, 0.0, 0.0]))]
    _, A = ref_chain(spans, tr, np.sqrt(SCAN_P_IN).astype(complex), SAVE_EVERY)
    return A[-1], float(np.max(np.abs(A[:, 2]) ** 2))


def main() -> None:
    out = {}
    with Pool() as pool:
        for cuts in SPLIT_STEPS:
            res = pool.map(_split_point, [(cuts, float(d)) for d in SPLIT_DBETA])
            out[f"split{cuts}_z"] = res[0][0]
            out[f"split{cuts}_A"] = np.array([r[1] for r in res])
            out[f"split{cuts}_steps"] = np.array(SPLIT_STEPS[cuts])
            print(f"  split {cuts}: {out[f'split{cuts}_A'].shape}", flush=True)
        res = pool.map(_lossy_point, [float(p) for p in LOSSY_PHASE_IN])
        out["lossy_z"] = res[0][0]
        out["lossy_A"] = np.array([r[1] for r in res])
        print(f"  lossy: {out['lossy_A'].shape}", flush=True)
        pts = [(float(p), float(d)) for p in SCAN_PHASES for d in SCAN_PSA_DBETA]     # point k * M + m
        res = pool.map(_scan_point, pts)
        out["scan_A_end"] = np.array([r[0] for r in res]).reshape(SCAN_PHASES.size, SCAN_PSA_DBETA.size, 4)
        out["scan_p_sig_max"] = np.array([r[1] for r in res]).reshape(SCAN_PHASES.size, SCAN_PSA_DBETA.size)
        g = 10 * np.log10(out["scan_p_sig_max"] / SCAN_P_IN[2])
        print(f"  scan: gain {g.min():.3f} .. {g.max():.3f} dB", flush=True)
    G._save("G17", save_every=SAVE_EVERY, split_dbeta=SPLIT_DBETA, split_p_in=SPLIT_P_IN, split_gamma=0.0115,
            split_alpha=1.15e-4, split_dz=0.1, lossy_spans=LOSSY_SPANS, lossy_gain_db=LOSSY_GAIN_DB,
            lossy_phase=LOSSY_PHASE, lossy_p_in=LOSSY_P_IN, lossy_phase_in=LOSSY_PHASE_IN, scan_p_in=SCAN_P_IN,
            scan_gamma=SCAN_GAMMA, scan_alpha=SCAN_ALPHA, scan_copier=np.array(SCAN_COPIER), scan_psa=np.array(SCAN_PSA),
            scan_psa_dbeta=SCAN_PSA_DBETA, scan_mid_gain_db=SCAN_MID_GAIN_DB, scan_phases=SCAN_PHASES, **out)


if __name__ == "__main__":
    main()
