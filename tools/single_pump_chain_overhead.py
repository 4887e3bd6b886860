"""Cost of cutting one single-pump sweep into spans (psa_rk4_single_pump_chain_f64): 65 536 points x 100 000 steps, float64,
waves [p, s, i], run as one launch of psa_rk4_single_pump_f64 and as chains of 1, 4 and 16 equal spans with identity
transfers.  Times are hipEvent times of the whole call's compute (every span's launch and epilogue, no host copies).  Every
repetition runs the single launch and then each chain, so the figures alternate in one process; the medians are reported
against the single launch's own run-to-run spread.

    python tools/single_pump_chain_overhead.py [--points 65536] [--steps 100000] [--save-every 50] [--reps 7] [--out log]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import psa_amd._native as nat  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=65_536)
    ap.add_argument("--steps", type=int, default=100_000)
    ap.add_argument("--save-every", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--spans", default="1,4,16")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, steps, se, L = a.points, a.steps, a.save_every, 1000.0
    db = np.linspace(-4.5, 0.5, n) * 0.0115 * 0.5
    a0 = np.sqrt(np.array([0.5, 1e-5, 0.0])).astype(complex)
    spans = [int(s) for s in a.spans.split(",") if steps % int(s) == 0 and (steps // int(s)) % se == 0]

    def single():
        return nat.single_pump_host(db, n_steps=steps, z_max=L, save_every=se, gamma=0.0115, alpha=1.15e-4, a0=a0)

    def chain(S):
        return nat.single_pump_chain_host(np.broadcast_to(db, (S, n)), n_steps=np.full(S, steps // S), seg_len=np.full(S, L / S),
                                          save_every=se, gamma=np.full(S, 0.0115), alpha=np.full(S, 1.15e-4), a0=a0)

    ref = single()                                                    # warm-up of every path, and the unsplit result
    errs = {S: float(np.max(np.abs(chain(S)["a_end"] - ref["a_end"])) / np.max(np.abs(ref["a_end"]))) for S in spans}
    t = {0: [], **{S: [] for S in spans}}
    for _ in range(a.reps):
        t[0].append(single()["elapsed_ms"])
        for S in spans:
            t[S].append(chain(S)["elapsed_ms"])
    base = float(np.median(t[0]))
    lines = [f"# single-pump chain overhead: {n} points x {steps} steps, float64, save_every {se}, lossy, median of {a.reps} "
             f"alternating runs ({nat.version()})",
             f"single launch            median {base:10.3f} ms  min {min(t[0]):10.3f}  max {max(t[0]):10.3f}  "
             f"spread {100.0 * (max(t[0]) - min(t[0])) / base:5.2f} %"]
    for S in spans:
        m = float(np.median(t[S]))
        lines.append(f"{S:5d} spans               median {m:10.3f} ms  min {min(t[S]):10.3f}  max {max(t[S]):10.3f}  "
                     f"{100.0 * (m / base - 1.0):+7.2f} % vs the single launch  (a_end vs unsplit {errs[S]:.2e})")
    lines.append("raw ms: " + "; ".join(f"{'single' if S == 0 else S}: " + " ".join(f"{x:.3f}" for x in v) for S, v in t.items()))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
