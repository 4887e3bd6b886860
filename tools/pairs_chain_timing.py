#!/usr/bin/env python3
"""Timing of multi-channel chains and rows (psa_rk4_pairs_chain_f64_dev) for DESIGN.md 3.5d: kernel ms from events on the
launch stream, the median of `--repeats` (>= 5) after a warm launch.

  python tools/pairs_chain_timing.py [--parent-lib PATH] > profiles/pairs_chain.log       on one MI355X:
      (a) the summary kernel (psa_rk4_sweep_pairs_f64_dev, no rows) at 32 768 points x 1e5 steps, K = 2 and K = 16.  With
          --parent-lib (a libpsa_hip.so built from the parent commit, tools/ab_build.sh) the two libraries run in child
          processes that alternate, parent first, `--rounds` times each: the spread between the parent's own runs is the
          yardstick for the difference.
      (b) a three-span summary chain (3e4 + 5e4 + 2e4 steps, identity transfers) against the sum of three standalone sweeps
          of the same spans: what the two epilogue launches and the per-point a0 of the later spans cost.
      (c) rows at save_every = 1 (500 steps, 262 144 lanes: K = 2, 8, 16 at 131 072 / 32 768 / 16 384 points): achieved HBM
          write bandwidth, beside the 4-wave trajectory mode at 131 072 points.
"""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = 100_000
BCAST_GAMMA, BCAST_ALPHA, BCAST_A0, CHECK_NAN, EXACT_STEP, TRAJ_LD = 1, 2, 4, 1 << 8, 1 << 9, 1 << 17


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


def summary_child(lib_path, repeats):
    """(a) in a process of its own, on the library at lib_path through ctypes alone (a parent build lacks the new symbols the
    package binds): prints `SUMMARY K median min max` per K."""
    import numpy as np
    import torch
    dev = torch.device("cuda:0")
    torch.zeros(1, device=dev)                      # the HIP runtime torch brought is the one the library binds to
    lib = C.CDLL(lib_path)
    fn = lib.psa_rk4_sweep_pairs_f64_dev
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_double, C.c_int32] + [C.c_void_p] * 4 + [C.c_uint32] + [C.c_void_p] * 4
    stream = torch.cuda.current_stream().cuda_stream
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev)   # noqa: E731
    d_g, d_al = t([0.0115]), t([1.15e-4])
    N = 32768
    for K in (2, 16):
        nw = 2 + 2 * K
        p = np.full(nw, 1e-5)
        p[:2] = 0.5
        d_a0 = t(np.column_stack([np.sqrt(p), np.zeros(nw)]).ravel())
        d_db = t(np.linspace(-0.05, 0.05, N)[None, :] * np.linspace(1.0, 0.5, K)[:, None])
        outs = [torch.empty((2 * nw, N), dtype=torch.float64, device=dev), torch.empty((nw, N), dtype=torch.float64, device=dev),
                torch.empty((nw, N), dtype=torch.float64, device=dev), torch.empty(N, dtype=torch.int64, device=dev)]

        def launch():
            rc = fn(stream or None, K, N, STEPS, 0.1 * STEPS, 10, d_db.data_ptr(), d_g.data_ptr(), d_al.data_ptr(), d_a0.data_ptr(),
                    BCAST_GAMMA | BCAST_ALPHA | BCAST_A0 | CHECK_NAN | EXACT_STEP, *(o.data_ptr() for o in outs))
            assert rc == 0, rc
        med, lo, hi = median_ms(torch, launch, repeats)
        print(f"SUMMARY {K} {med:.4f} {lo:.4f} {hi:.4f}", flush=True)


def summary_ab(parent_lib, this_lib, rounds, repeats):
    print(f"## (a) summary kernel, 32 768 points x {STEPS} steps, save_every 10, check exact, lossy; median of {repeats} per run, "
          f"{rounds} runs per library, alternating")
    libs = ([("parent", parent_lib)] if parent_lib else []) + [("this", this_lib)]
    got = {(name, K): [] for name, _ in libs for K in (2, 16)}
    for rnd in range(rounds):
        for name, path in libs:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--summary-child", path, "--repeats", str(repeats)],
                                 check=True, capture_output=True, text=True, timeout=600).stdout
            for line in out.splitlines():
                if line.startswith("SUMMARY"):
                    _, K, med, lo, hi = line.split()
                    got[name, int(K)].append(float(med))
                    print(f"  run {rnd} {name:6s} K={int(K):2d}: median {float(med):9.3f} ms (min {float(lo):.3f}, max {float(hi):.3f})", flush=True)
    for K in (2, 16):
        this = statistics.median(got["this", K])
        if parent_lib:
            par = got["parent", K]
            print(f"RESULT (a) K={K}: parent {statistics.median(par):.3f} ms (its runs spread {max(par) - min(par):.3f} ms), this commit "
                  f"{this:.3f} ms, difference {this - statistics.median(par):+.3f} ms")
        else:
            print(f"RESULT (a) K={K}: this commit {this:.3f} ms (no parent library given)")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--summary-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if args.summary_child:
        summary_child(args.summary_child, args.repeats)
        return
    import numpy as np
    import torch
    import psa_amd._native as nat
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    print(f"# {nat.version()}; {torch.cuda.get_device_name(0)}")
    summary_ab(args.parent_lib, nat.LIB_PATH, args.rounds, args.repeats)

    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev)   # noqa: E731
    check = nat.OPT_CHECK_NAN | nat.OPT_EXACT_STEP

    def a0_of(nw, N=None):
        p = np.full(nw, 1e-5)
        p[:2] = 0.5
        a = np.column_stack([np.sqrt(p), np.zeros(nw)]).ravel()
        return t(a if N is None else np.repeat(a[:, None], N, axis=1))

    def outputs(nw, N):
        return [torch.empty((2 * nw, N), dtype=torch.float64, device=dev), torch.empty((nw, N), dtype=torch.float64, device=dev),
                torch.empty((nw, N), dtype=torch.float64, device=dev), torch.empty(N, dtype=torch.int64, device=dev)]

    # ---- (b) ---------------------------------------------------------------------------------------------------------
    print("## (b) three-span summary chain (30 000 + 50 000 + 20 000 steps, save_every 10, identity transfers, per-span dbeta) "
          "against three standalone sweeps of the same spans, 32 768 points")
    N, steps = 32768, [30_000, 50_000, 20_000]
    lens = [0.1 * n for n in steps]
    for K in (2, 16):
        nw = 2 + 2 * K
        db = np.stack([s * np.linspace(-0.05, 0.05, N)[None, :] * np.linspace(1.0, 0.5, K)[:, None] for s in (1.0, 0.8, 1.2)])
        d_db, d_g, d_al = t(db), t([0.0115] * 3), t([1.15e-4] * 3)
        d_a0, d_a0_pts, outs = a0_of(nw), a0_of(nw, N), outputs(nw, N)
        d_ws = torch.empty(nat.pairs_chain_workspace_bytes(K, N), dtype=torch.uint8, device=dev)
        flags = nat.BCAST_GAMMA | nat.BCAST_ALPHA | check

        def chain():
            nat.pairs_chain_device(stream=stream, n_pairs=K, n_points=N, n_steps=steps, seg_len=lens, save_every=10,
                                   d_dbeta_soa=d_db.data_ptr(), d_gamma=d_g.data_ptr(), d_alpha=d_al.data_ptr(),
                                   d_a0_soa=d_a0.data_ptr(), d_transfer_soa=0, flags=flags | nat.BCAST_A0,
                                   d_a_end_soa=outs[0].data_ptr(), d_p_wave_end_soa=outs[1].data_ptr(),
                                   d_p_wave_max_soa=outs[2].data_ptr(), d_first_bad=outs[3].data_ptr(), d_workspace=d_ws.data_ptr())

        def sweep(s, a0, bcast):
            def launch():
                nat.sweep_pairs_device(stream=stream, n_pairs=K, n_points=N, n_steps=steps[s], z_max=lens[s], save_every=10,
                                       d_dbeta_soa=d_db[s].data_ptr(), d_gamma=d_g[s:].data_ptr(), d_alpha=d_al[s:].data_ptr(),
                                       d_a0_soa=a0.data_ptr(), flags=flags | bcast, d_a_end_soa=outs[0].data_ptr(),
                                       d_p_wave_end_soa=outs[1].data_ptr(), d_p_wave_max_soa=outs[2].data_ptr(),
                                       d_first_bad=outs[3].data_ptr())
            return launch
        ms_chain = median_ms(torch, chain, args.repeats)
        parts = [median_ms(torch, sweep(0, d_a0, nat.BCAST_A0), args.repeats)] + \
                [median_ms(torch, sweep(s, d_a0_pts, 0), args.repeats) for s in (1, 2)]
        total = sum(p[0] for p in parts)
        print(f"RESULT (b) K={K}: chain {ms_chain[0]:.3f} ms (min {ms_chain[1]:.3f}, max {ms_chain[2]:.3f}); sweeps "
              + " + ".join(f"{p[0]:.3f}" for p in parts) + f" = {total:.3f} ms; chain - sweeps {ms_chain[0] - total:+.3f} ms = "
              f"{100.0 * (ms_chain[0] - total) / ms_chain[0]:+.2f} % of the chain")
        del d_ws, outs, d_db

    # ---- (c) ---------------------------------------------------------------------------------------------------------
    print("## (c) rows at save_every = 1, 500 steps, padded leading dimension (PSA_OPT_TRAJ_LD), check exact, lossy")
    n_steps = 500
    d_g, d_al = t([0.0115]), t([1.15e-4])
    flags = nat.BCAST_GAMMA | nat.BCAST_ALPHA | nat.BCAST_A0 | check | nat.OPT_TRAJ_LD
    results = []
    for K, N in ((2, 131072), (8, 32768), (16, 16384)):
        nw, ld = 2 + 2 * K, nat.traj_ld(N)
        d_db = t(np.linspace(-0.05, 0.05, N)[None, :] * np.linspace(1.0, 0.5, K)[:, None])
        d_a0, outs = a0_of(nw), outputs(nw, N)
        d_traj = torch.empty((n_steps + 1, nw, ld, 2), dtype=torch.float64, device=dev)

        def rows():
            nat.pairs_chain_device(stream=stream, n_pairs=K, n_points=N, n_steps=[n_steps], seg_len=[0.1 * n_steps], save_every=1,
                                   d_dbeta_soa=d_db.data_ptr(), d_gamma=d_g.data_ptr(), d_alpha=d_al.data_ptr(),
                                   d_a0_soa=d_a0.data_ptr(), d_transfer_soa=0, flags=flags, d_a_end_soa=outs[0].data_ptr(),
                                   d_p_wave_end_soa=outs[1].data_ptr(), d_p_wave_max_soa=outs[2].data_ptr(),
                                   d_first_bad=outs[3].data_ptr(), d_traj_soa=d_traj.data_ptr())

        def no_rows():
            nat.sweep_pairs_device(stream=stream, n_pairs=K, n_points=N, n_steps=n_steps, z_max=0.1 * n_steps, save_every=1,
                                   d_dbeta_soa=d_db.data_ptr(), d_gamma=d_g.data_ptr(), d_alpha=d_al.data_ptr(),
                                   d_a0_soa=d_a0.data_ptr(), flags=flags & ~nat.OPT_TRAJ_LD, d_a_end_soa=outs[0].data_ptr(),
                                   d_p_wave_end_soa=outs[1].data_ptr(), d_p_wave_max_soa=outs[2].data_ptr(),
                                   d_first_bad=outs[3].data_ptr())
        ms, lo, hi = median_ms(torch, rows, args.repeats)
        ms0 = median_ms(torch, no_rows, args.repeats)[0]
        gb = (n_steps + 1) * nw * N * 16 / 1e9
        results.append((f"pairs K={K:2d} (L={max(2, 1 << (K - 1).bit_length()):2d}, {64 // max(2, 1 << (K - 1).bit_length()):2d} points = "
                        f"{1024 // max(2, 1 << (K - 1).bit_length()):3d} B per wave region and store)", N, gb, ms, lo, hi, ms0))
        del d_traj
    N = 131072
    ld = nat.traj_ld(N)
    d_db, d_a0 = t(np.linspace(-0.05, 0.05, N)), a0_of(4)
    outs = [torch.empty((8, N), dtype=torch.float64, device=dev), torch.empty(N, dtype=torch.float64, device=dev),
            torch.empty(N, dtype=torch.float64, device=dev), torch.empty(N, dtype=torch.int64, device=dev)]
    d_traj = torch.empty((n_steps + 1, 4, ld, 2), dtype=torch.float64, device=dev)

    def four(traj):
        def launch():
            nat.sweep_device(stream=stream, n_waves=4, n_points=N, n_steps=n_steps, z_max=0.1 * n_steps, save_every=1,
                             d_dbeta=d_db.data_ptr(), d_dbeta2=0, d_gamma=d_g.data_ptr(), d_alpha=d_al.data_ptr(),
                             d_a0_soa=d_a0.data_ptr(), flags=flags if traj else flags & ~nat.OPT_TRAJ_LD, d_a_end_soa=outs[0].data_ptr(),
                             d_p_end=outs[1].data_ptr(), d_p_max=outs[2].data_ptr(), d_first_bad=outs[3].data_ptr(),
                             d_traj_soa=d_traj.data_ptr() if traj else 0)
        return launch
    ms, lo, hi = median_ms(torch, four(True), args.repeats)
    results.append(("4-wave trajectory mode (64 points = 1024 B per wave region and store)", N, (n_steps + 1) * 4 * N * 16 / 1e9, ms, lo,
                    hi, median_ms(torch, four(False), args.repeats)[0]))
    for name, N, gb, ms, lo, hi, ms0 in results:
        print(f"RESULT (c) {name}: {N} points, {gb:.3f} GB of rows in {ms:.3f} ms (min {lo:.3f}, max {hi:.3f}) = {gb / ms:.3f} TB/s; "
              f"the same launch without rows {ms0:.3f} ms")


if __name__ == "__main__":
    main()
