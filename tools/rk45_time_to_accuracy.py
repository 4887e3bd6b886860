#!/usr/bin/env python3
"""Time to accuracy: fixed-step RK4 against adaptive RK45 on BASELINE config-2 inputs, one MI355X.

65 536 points, dbeta = linspace(-0.05, 0.05), gamma 0.0115, alpha 1.15e-4, P = (0.5, 0.5, 1e-5, 1e-5) W, L = 1000 m.
Truth: rk4_sweep at 4e5 steps; its distance to 2e5 steps is reported as the truth's own uncertainty.  For every
configuration: kernel ms (hipEvents of the host call, best of 3 after one warm-up call) and the max over points of
|A_end - truth| / max_j |truth_j|.  For RK45 also the step counts and the lane-idle fraction of the launch:
sum over 64-point waves of (wave max - lane attempts) / sum of wave max, attempts = accepted + rejected.
atol = 1e-3 * rtol, so that the absolute floor never loosens the control of the small signal and idler.

    python tools/rk45_time_to_accuracy.py [--points 65536]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import psa_amd._native as nat  # noqa: E402

P = np.array([0.5, 0.5, 1e-5, 1e-5])
KW = dict(z_max=1000.0, gamma=0.0115, alpha=1.15e-4, a0=np.sqrt(P).astype(complex))


def best_of(fn, reps=3):
    fn()   # warm-up
    runs = [fn() for _ in range(reps)]
    return min(runs, key=lambda r: r["elapsed_ms"])


def rel_err(a, truth):
    return float(np.max(np.max(np.abs(a - truth), axis=1) / np.max(np.abs(truth), axis=1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=65_536)
    args = ap.parse_args()
    db = np.linspace(-0.05, 0.05, args.points)
    rk4 = lambda n: (lambda: nat.sweep_host(db, n_steps=n, save_every=n, check_nan=False, **KW))  # noqa: E731
    t4 = rk4(400_000)()
    t2 = rk4(200_000)()
    truth = t4["a_end"]
    print(f"# {nat.version()}  N = {args.points}, L = 1000 m, config-2 inputs")
    print(f"truth: RK4 n = 4e5 ({t4['elapsed_ms']:.1f} ms); |RK4(2e5) - RK4(4e5)| = {rel_err(t2['a_end'], truth):.2e}")
    print(f"{'method':<8} {'setting':>10} {'kernel ms':>10} {'max rel err':>12} {'steps/pt (min/med/max)':>24} "
          f"{'rejected':>9} {'lane idle':>9}")
    for n in (1_000, 3_000, 10_000, 30_000, 100_000):
        r = best_of(rk4(n))
        print(f"{'RK4':<8} {n:>10.0e} {r['elapsed_ms']:>10.2f} {rel_err(r['a_end'], truth):>12.2e} "
              f"{f'{n}/{n}/{n}':>24} {0:>9} {0.0:>9.3f}", flush=True)
    for rtol in (1e-6, 1e-8, 1e-10, 1e-12):
        r = best_of(lambda: nat.rk45_sweep_host(db, rtol=rtol, atol=1e-3 * rtol,
                                                max_steps=1_000_000, **KW))
        att = r["n_accepted"] + r["n_rejected"]
        pad = (-att.size) % 64
        w = np.concatenate([att, np.zeros(pad, att.dtype)]).reshape(-1, 64)
        live = np.concatenate([np.ones(att.size, bool), np.zeros(pad, bool)]).reshape(-1, 64)
        wmax = np.max(w, axis=1, keepdims=True)
        idle = float(np.sum((wmax - w) * live) / np.sum(wmax * live))
        acc = r["n_accepted"]
        assert np.all(r["status"] == 0), "every point must reach z_max"
        print(f"{'RK45':<8} {rtol:>10.0e} {r['elapsed_ms']:>10.2f} {rel_err(r['a_end'], truth):>12.2e} "
              f"{f'{acc.min()}/{int(np.median(acc))}/{acc.max()}':>24} {int(r['n_rejected'].sum()):>9} {idle:>9.3f}",
              flush=True)


if __name__ == "__main__":
    main()
