#!/usr/bin/env python3
"""What a multi-line ("comb") chain costs over the single comb launch (psa_rk4_comb_chain_f64_dev) for DESIGN.md 3.5e: kernel ms
from events on the launch stream, the median of `--repeats` (>= 5) after a warm launch, everything in one process.

  python tools/comb_chain_timing.py > profiles/comb_chain.log       on one MI355X:
      65 536 points x 10 000 steps, save_every 10, check on, lossy, M = 4 and 12; the whole chain for 1, 4 and 16 spans of one
      fibre (identity transfers, the span's kappa per point) against the single launch of psa_rk4_comb_f64_dev, without and
      with the trajectory (padded leading dimension).  Spans >= 1 start from a per-point a0 and every span is followed by an
      epilogue launch; with the trajectory the epilogue also rotates all M columns of the span's rows.  The single launch's
      own (max - min) over its repeats is printed next to every overhead: a difference below it says nothing.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, STEPS, SAVE = 65536, 10_000, 10


def median_ms(torch, fn, repeats):
    """median kernel ms of `repeats` launches after a warm one, and their (min, max)"""
    ms = []
    for rep in range(repeats + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if rep:
            ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def span_steps(S):
    """STEPS cut into S spans of multiples of SAVE, the last one taking the rest"""
    steps = [(STEPS // SAVE // S) * SAVE] * S
    steps[-1] = STEPS - sum(steps[:-1])
    return steps


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    import numpy as np
    import torch
    import psa_amd._native as nat
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    print(f"# {nat.version()}; {torch.cuda.get_device_name(0)}; {N} points x {STEPS} steps, save_every {SAVE}, check on, lossy, "
          f"broadcast gamma / alpha, median of {args.repeats} after a warm launch")
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev)   # noqa: E731
    check = nat.OPT_CHECK_NAN | nat.OPT_EXACT_STEP
    ld = nat.traj_ld(N)
    for M in (4, 12):
        x = np.arange(M) - 0.5 * (M - 1)
        kappa = (x ** 2)[:, None] * np.linspace(-2e-3, 5e-4, N)[None, :]                  # SoA [M][N]
        p = np.full(M, 1e-5)
        p[1] = p[M - 2] = 0.25
        a0 = np.repeat(np.column_stack([np.sqrt(p), np.zeros(M)]).ravel()[:, None], N, axis=1)   # SoA [2M][N]
        d_a0 = t(a0)
        outs = [torch.empty((2 * M, N), dtype=torch.float64, device=dev), torch.empty((M, N), dtype=torch.float64, device=dev),
                torch.empty((M, N), dtype=torch.float64, device=dev), torch.empty(N, dtype=torch.int64, device=dev)]
        d_ws = torch.empty(nat.comb_chain_workspace_bytes(M, N), dtype=torch.uint8, device=dev)
        d_traj = torch.empty((STEPS // SAVE + 16, M, ld, 2), dtype=torch.float64, device=dev)
        d_kp1, d_g1, d_al1 = t(kappa), t([0.0115]), t([1.15e-4])
        for traj in (False, True):
            flags = nat.BCAST_GAMMA | nat.BCAST_ALPHA | check | (nat.OPT_TRAJ_LD if traj else 0)

            def single():
                nat.comb_device(stream=stream, n_lines=M, n_points=N, n_steps=STEPS, z_max=0.1 * STEPS, save_every=SAVE,
                                d_kappa_soa=d_kp1.data_ptr(), d_gamma=d_g1.data_ptr(), d_alpha=d_al1.data_ptr(),
                                d_a0_soa=d_a0.data_ptr(), flags=flags, d_a_end_soa=outs[0].data_ptr(),
                                d_p_wave_end_soa=outs[1].data_ptr(), d_p_wave_max_soa=outs[2].data_ptr(),
                                d_first_bad=outs[3].data_ptr(), d_traj_soa=d_traj.data_ptr() if traj else 0)
            base, lo, hi = median_ms(torch, single, args.repeats)
            spread = hi - lo
            what = "with the trajectory" if traj else "summary only"
            print(f"RESULT M={M} {what}: single launch {base:.3f} ms (min {lo:.3f}, max {hi:.3f}, spread {spread:.3f} ms = "
                  f"{100.0 * spread / base:.2f} %)", flush=True)
            for S in (1, 4, 16):
                steps = span_steps(S)
                d_kp, d_g, d_al = t(np.tile(kappa, (S, 1, 1))), t([0.0115] * S), t([1.15e-4] * S)

                def chain():
                    nat.comb_chain_device(stream=stream, n_lines=M, n_points=N, n_steps=steps, seg_len=[0.1 * n for n in steps],
                                          save_every=SAVE, d_kappa_soa=d_kp.data_ptr(), d_gamma=d_g.data_ptr(),
                                          d_alpha=d_al.data_ptr(), d_a0_soa=d_a0.data_ptr(), d_transfer_soa=0, flags=flags,
                                          d_a_end_soa=outs[0].data_ptr(), d_p_wave_end_soa=outs[1].data_ptr(),
                                          d_p_wave_max_soa=outs[2].data_ptr(), d_first_bad=outs[3].data_ptr(),
                                          d_traj_soa=d_traj.data_ptr() if traj else 0, d_workspace=d_ws.data_ptr())
                ms, clo, chi = median_ms(torch, chain, args.repeats)
                print(f"RESULT M={M} {what}: {S:2d} spans {ms:.3f} ms (min {clo:.3f}, max {chi:.3f}); chain - single {ms - base:+.3f} ms "
                      f"= {100.0 * (ms - base) / base:+.2f} % against the single launch's spread of {spread:.3f} ms"
                      + (" (below the spread)" if abs(ms - base) <= spread else ""), flush=True)
                del d_kp
        del d_traj, d_ws, outs


if __name__ == "__main__":
    main()
