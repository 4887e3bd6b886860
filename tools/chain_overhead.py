"""Cost of cutting one sweep into spans (psa_rk4_chain_f64): a C2-sized sweep -- 65 536 points x 100 000 steps, float64,
4 waves -- run as one launch of psa_rk4_sweep_f64 and as chains of 1, 4, 16 and 1 000 equal spans with identity
transfers.  Times are the chain's hipEvent time (every span's sweep launch and epilogue, no host copies); the median of
--reps runs after one warm-up each.

    python tools/chain_overhead.py [--points 65536] [--steps 100000] [--save-every 50] [--reps 5] [--out log]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import psa_amd._native as nat  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=65_536)
    ap.add_argument("--steps", type=int, default=100_000)
    ap.add_argument("--save-every", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--spans", default="1,4,16,1000")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, steps, se = a.points, a.steps, a.save_every
    db = np.linspace(-0.05, 0.05, n)
    a0 = np.sqrt(np.array([0.5, 0.5, 1e-5, 0.0])).astype(complex)
    L = 1000.0
    lines = [f"# chain overhead: {n} points x {steps} steps, float64, 4 waves, save_every {se}, lossy, "
             f"median of {a.reps} ({nat.version()})"]

    def timed(fn):
        fn()
        t = []
        for _ in range(a.reps):
            t.append(fn())
        return float(np.median(t)), float(np.min(t)), float(np.max(t))

    base = timed(lambda: nat.sweep_host(db, n_steps=steps, z_max=L, save_every=se, gamma=0.0115, alpha=1.15e-4,
                                        a0=a0)["elapsed_ms"])
    lines.append(f"sweep (one launch)       median {base[0]:10.3f} ms  min {base[1]:10.3f}  max {base[2]:10.3f}")
    ref = nat.sweep_host(db, n_steps=steps, z_max=L, save_every=se, gamma=0.0115, alpha=1.15e-4, a0=a0)
    for S in (int(s) for s in a.spans.split(",")):
        if steps % S or (steps // S) % se:
            lines.append(f"{S} spans: skipped ({steps} steps do not split into {S} multiples of {se})")
            continue
        kw = dict(n_steps=np.full(S, steps // S), seg_len=np.full(S, L / S), save_every=se, gamma=np.full(S, 0.0115),
                  alpha=np.full(S, 1.15e-4), a0=a0)
        dbs = np.broadcast_to(db, (S, n))
        t0 = time.perf_counter()
        r = timed(lambda: nat.chain_host(dbs, **kw)["elapsed_ms"])
        wall = (time.perf_counter() - t0) / (a.reps + 1)
        got = nat.chain_host(dbs, **kw)
        err = float(np.max(np.abs(got["a_end"] - ref["a_end"])) / np.max(np.abs(ref["a_end"])))
        per_span = f"{(r[0] - base[0]) / (S - 1) * 1e3:8.1f} us per extra span; " if S > 1 else "same single launch; "
        lines.append(f"{S:5d} spans               median {r[0]:10.3f} ms  min {r[1]:10.3f}  max {r[2]:10.3f}  "
                     f"{100.0 * (r[0] / base[0] - 1.0):+7.2f} % vs one launch  ({per_span}"
                     f"call wall {wall * 1e3:.1f} ms; a_end vs unsplit {err:.2e})")
    again = timed(lambda: nat.sweep_host(db, n_steps=steps, z_max=L, save_every=se, gamma=0.0115, alpha=1.15e-4,
                                         a0=a0)["elapsed_ms"])
    lines.append(f"sweep again (drift)      median {again[0]:10.3f} ms  min {again[1]:10.3f}  max {again[2]:10.3f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
