#!/usr/bin/env python3
"""Timing of the multi-channel kernel (psa_rk4_sweep_pairs_f64_dev) for DESIGN.md 3.3b: kernel ms from events on the launch
stream, best of 3 after a warm launch, the candidates of a comparison alternating in one process.

  python tools/pairs_timing.py            on one MI355X:
      A/B   K = 2 against the existing two-lane 6-wave kernel on the config-5 shard (32 768 points x 1e5 steps)
      K in {4, 8, 16} at 65 536 / L points x 1e5 steps (a constant 65 536 lanes: one wave per SIMD), beside the 4-wave
      one-lane kernel at 65 536 points; time per lane-step against the static VALU count per step
  python tools/pairs_timing.py --static   no GPU: compiles csrc/psa_rk4_pairs.hip to gfx950 assembly and prints, per
      instantiation, VGPRs, scratch and the VALU instructions of one RK4 step (the hot loop holds two)
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CSRC = os.path.join(ROOT, "psa-simulation-ode-rk-mvp-dispersion_amd", "csrc")
STEPS = 100_000


def static_counts(unit="psa_rk4_pairs.hip", pattern="rk4_sweep_pairs_kernel"):
    """{kernel: (vgprs, scratch bytes, VALU per RK4 step, of which DPP moves)} from the unit's gfx950 assembly."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "unit.s")
        subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                        "-mllvm", "-amdgpu-sched-strategy=max-ilp", "-mllvm", "-align-all-blocks=3", "-S", "--cuda-device-only",
                        os.path.join(CSRC, unit), "-o", asm], check=True, stderr=subprocess.DEVNULL)
        text = open(asm).read()
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)\n\s*\.amdhsa_kernel \1\n(.*?)\.end_amdhsa_kernel", text, re.S | re.M):
        name, body, meta = m.groups()
        if pattern not in name:
            continue
        # the hot loop: the self-looping basic block with the most vector instructions (two RK4 steps per trip)
        best = (0, 0)
        for blk in re.finditer(r"^(\.LBB\d+_\d+):[^\n]*\n(.*?)(?=^\.LBB|\Z)", body, re.S | re.M):
            label, code = blk.groups()
            if not re.search(r"s_cbranch_\w+ " + re.escape(label) + r"\b", code):
                continue
            valu = len(re.findall(r"^\s+v_", code, re.M))
            if valu > best[0]:
                best = (valu, len(re.findall(r"^\s+v_mov_b32_dpp", code, re.M)))
        vgpr = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", meta).group(1))
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", meta).group(1))
        out[name] = (vgpr, scratch, best[0] / 2.0, best[1] / 2.0)
    return out


def print_static():
    print("# static: VGPRs, scratch, VALU instructions per RK4 step (DPP moves among them) from the gfx950 assembly")
    for name, (vgpr, scratch, valu, dpp) in sorted(static_counts().items()):
        m = re.search(r"ILi(\d+)ELi(\d)ELi(\d+)ELb([01])ELb([01])E", name)
        lanes, check, block, loss = int(m.group(1)), "none block exact".split()[int(m.group(2))], int(m.group(3)), m.group(4) == "1"
        print(f"L={lanes:2d} check={check:5s} block={block:3d} {'lossy   ' if loss else 'lossless'}  VGPRs {vgpr:3d}  scratch {scratch}  "
              f"VALU/step {valu:6.1f}  (DPP {dpp:5.1f}){'  rows' if m.group(5) == '1' else ''}")
    ref = static_counts("psa_rk4_f64.hip", "rk4_sweep_kernelIdLi4ELi2ELb0ELi256ELb0ELb1ELb0E")
    for name, (vgpr, scratch, valu, dpp) in ref.items():
        print(f"4-wave one-lane (check=exact block=256 lossy)  VGPRs {vgpr}  scratch {scratch}  VALU/step {valu:.1f}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--static", action="store_true")
    ap.add_argument("--steps", type=int, default=STEPS)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    if args.static:
        print_static()
        return
    import numpy as np
    import torch
    import psa_amd._native as nat
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    flags = nat.BCAST_GAMMA | nat.BCAST_ALPHA | nat.BCAST_A0 | nat.OPT_CHECK_NAN | nat.OPT_EXACT_STEP
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev)   # noqa: E731
    d_g, d_al = t([0.0115]), t([1.15e-4])
    n_steps, z_max = args.steps, 0.1 * args.steps

    def a0_soa(nw):
        p = np.full(nw, 1e-5)
        p[:2] = 0.5
        return t(np.column_stack([np.sqrt(p), np.zeros(nw)]).ravel())

    def pairs(K, N):
        nw = 2 + 2 * K
        d_db = t(np.linspace(-0.05, 0.05, N)[None, :] * np.linspace(1.0, 0.5, K)[:, None])
        d_a0 = a0_soa(nw)
        outs = [torch.empty((2 * nw, N), dtype=torch.float64, device=dev), torch.empty((nw, N), dtype=torch.float64, device=dev),
                torch.empty((nw, N), dtype=torch.float64, device=dev), torch.empty(N, dtype=torch.int64, device=dev)]
        keep = (d_db, d_a0, outs)

        def launch():
            nat.sweep_pairs_device(stream=stream, n_pairs=K, n_points=N, n_steps=n_steps, z_max=z_max, save_every=10,
                                   d_dbeta_soa=d_db.data_ptr(), d_gamma=d_g.data_ptr(), d_alpha=d_al.data_ptr(),
                                   d_a0_soa=d_a0.data_ptr(), flags=flags, d_a_end_soa=outs[0].data_ptr(),
                                   d_p_wave_end_soa=outs[1].data_ptr(), d_p_wave_max_soa=outs[2].data_ptr(),
                                   d_first_bad=outs[3].data_ptr())
        launch.keep = keep
        return launch

    def waves(nw, N, layout):
        d_db = t(np.linspace(-0.05, 0.05, N))
        d_db2 = t(0.5 * np.linspace(-0.05, 0.05, N)) if nw == 6 else None
        d_a0 = a0_soa(nw)
        outs = [torch.empty((2 * nw, N), dtype=torch.float64, device=dev), torch.empty(N, dtype=torch.float64, device=dev),
                torch.empty(N, dtype=torch.float64, device=dev), torch.empty(N, dtype=torch.int64, device=dev)]
        keep = (d_db, d_db2, d_a0, outs)

        def launch():
            nat.sweep_device(stream=stream, n_waves=nw, n_points=N, n_steps=n_steps, z_max=z_max, save_every=10,
                             d_dbeta=d_db.data_ptr(), d_dbeta2=(d_db2.data_ptr() if nw == 6 else 0), d_gamma=d_g.data_ptr(),
                             d_alpha=d_al.data_ptr(), d_a0_soa=d_a0.data_ptr(), flags=flags | layout,
                             d_a_end_soa=outs[0].data_ptr(), d_p_end=outs[1].data_ptr(), d_p_max=outs[2].data_ptr(),
                             d_first_bad=outs[3].data_ptr())
        launch.keep = keep
        return launch

    def best_ms(cands):
        """{name: best of `repeats` kernel ms}, one warm launch each, then the candidates alternating."""
        best = {k: float("inf") for k in cands}
        for rep in range(args.repeats + 1):
            for name, fn in cands.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if rep:
                    best[name] = min(best[name], e0.elapsed_time(e1))
                print(f"  {name}: launch {rep} {e0.elapsed_time(e1):9.3f} ms{'  (warm-up)' if not rep else ''}", flush=True)
        return best

    print(f"# {nat.version()}; {torch.cuda.get_device_name(0)}; {n_steps} steps, save_every 10, check exact, lossy, broadcast inputs")
    print("## A/B: K = 2 (new kernel, 2 lanes per point) against the two-lane 6-wave kernel, 32 768 points")
    ab = best_ms({"pairs K=2": pairs(2, 32768), "six-wave two-lane": waves(6, 32768, nat.OPT_SPLIT_POINT)})
    print(f"RESULT A/B pairs K=2 {ab['pairs K=2']:.3f} ms, six-wave two-lane {ab['six-wave two-lane']:.3f} ms, ratio "
          f"{ab['pairs K=2'] / ab['six-wave two-lane']:.4f}")
    print("## constant 65 536 lanes: K = 4, 8, 16 at 65 536 / L points, the 4-wave one-lane kernel at 65 536 points")
    cands = {f"pairs K={K}": pairs(K, 65536 // K) for K in (4, 8, 16)}
    cands["four-wave one-lane"] = waves(4, 65536, nat.OPT_ONE_LANE)
    ms = best_ms(cands)
    base = ms["four-wave one-lane"]
    for name, v in ms.items():
        print(f"RESULT {name}: {v:.3f} ms, {v * 1e6 / (65536 * n_steps) * 1e3:.4f} ps per lane-step, x{v / base:.4f} of the 4-wave one-lane kernel")


if __name__ == "__main__":
    main()
