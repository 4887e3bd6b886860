#!/usr/bin/env python3
"""Timing of the single-pump three-wave kernel (psa_rk4_single_pump_f64_dev) for DESIGN.md 3.3c: kernel ms from events on the
launch stream, best of 3 after a warm launch, the two candidates alternating in one process.

  python tools/single_pump_timing.py            on one MI355X: 65 536 points x 1e5 steps, lossy, check exact, against the
      4-wave one-lane kernel on NON-MIRRORED inputs (A1 != A2: with equal pumps and equal sidebands that kernel takes its
      174-instruction two-wave loop, which is another comparison)
  python tools/single_pump_timing.py --static   no GPU: compiles csrc/psa_rk4_single_pump.hip to gfx950 assembly and prints,
      per instantiation, VGPRs, scratch and the VALU instructions of one RK4 step (the hot loop holds two)
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
POINTS = 65_536


def static_counts(unit="psa_rk4_single_pump.hip", pattern="rk4_sweep_single_pump_kernel"):
    """{kernel: (vgprs, spilled vgprs, scratch bytes, VALU per RK4 step)} from the unit's gfx950 assembly."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "unit.s")
        subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                        "-mllvm", "-amdgpu-sched-strategy=max-ilp", "-mllvm", "-align-all-blocks=3", "-S", "--cuda-device-only",
                        os.path.join(CSRC, unit), "-o", asm], check=True, stderr=subprocess.DEVNULL)
        text = open(asm).read()
    out = {}
    # spilled VGPRs: the kernel's entry in the code object's metadata
    spills = {n: int(v) for n, v in re.findall(r"\.name:\s+(\S+)\n(?:(?!\.name:).)*?\.vgpr_spill_count:\s+(\d+)", text, re.S)}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)\n\s*\.amdhsa_kernel \1\n(.*?)\.end_amdhsa_kernel", text, re.S | re.M):
        name, body, meta = m.groups()
        if pattern not in name:
            continue
        # the hot loop: the self-looping basic block with the most vector instructions (two RK4 steps per trip)
        best = 0
        for blk in re.finditer(r"^(\.LBB\d+_\d+):[^\n]*\n(.*?)(?=^\.LBB|\Z)", body, re.S | re.M):
            label, code = blk.groups()
            if re.search(r"s_cbranch_\w+ " + re.escape(label) + r"\b", code):
                best = max(best, len(re.findall(r"^\s+v_", code, re.M)))
        vgpr = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", meta).group(1))
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", meta).group(1))
        out[name] = (vgpr, spills[name], scratch, best / 2.0)
    return out


def print_static():
    print("# static: VGPRs, spilled VGPRs, scratch, VALU instructions per RK4 step from the gfx950 assembly")
    worst = 0
    for name, (vgpr, spill, scratch, valu) in sorted(static_counts().items()):
        m = re.search(r"ILi(\d)ELb([01])ELi(\d+)ELb([01])E", name)
        check, traj = "none block exact".split()[int(m.group(1))], m.group(2) == "1"
        block, loss = int(m.group(3)), m.group(4) == "1"
        worst = max(worst, scratch, spill)
        print(f"check={check:5s} traj={int(traj)} block={block:3d} {'lossy   ' if loss else 'lossless'}  VGPRs {vgpr:3d}  spilled {spill}  "
              f"scratch {scratch}  VALU/step {valu:6.1f}")
    ref = static_counts("psa_rk4_f64.hip", "rk4_sweep_kernelIdLi4ELi2ELb0ELi256ELb0ELb1ELb0E")
    for name, (vgpr, spill, scratch, valu) in ref.items():
        print(f"4-wave one-lane (check=exact block=256 lossy; the hot loop found is the general, non-mirrored one)  VGPRs {vgpr}  "
              f"scratch {scratch}  VALU/step {valu:.1f}")
    print(f"# worst scratch / spill over the single-pump instantiations: {worst}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--static", action="store_true")
    ap.add_argument("--steps", type=int, default=STEPS)
    ap.add_argument("--points", type=int, default=POINTS)
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
    n_steps, z_max, N = args.steps, 0.1 * args.steps, args.points
    d_db = t(np.linspace(-0.05, 0.05, N))

    def single_pump():
        d_a0 = t(np.column_stack([np.sqrt([1.0, 1e-5, 1e-5]), np.zeros(3)]).ravel())
        outs = [torch.empty((6, N), dtype=torch.float64, device=dev), torch.empty((3, N), dtype=torch.float64, device=dev),
                torch.empty((3, N), dtype=torch.float64, device=dev), torch.empty(N, dtype=torch.int64, device=dev)]

        def launch():
            nat.single_pump_device(stream=stream, n_points=N, n_steps=n_steps, z_max=z_max, save_every=10, d_dbeta=d_db.data_ptr(),
                                   d_gamma=d_g.data_ptr(), d_alpha=d_al.data_ptr(), d_a0_soa=d_a0.data_ptr(), flags=flags,
                                   d_a_end_soa=outs[0].data_ptr(), d_p_wave_end_soa=outs[1].data_ptr(),
                                   d_p_wave_max_soa=outs[2].data_ptr(), d_first_bad=outs[3].data_ptr())
        launch.keep = (d_a0, outs)
        return launch

    def four_wave():
        # unequal pumps and unequal sidebands: no wave starts mirrored, every lane runs the general 4-wave loop
        d_a0 = t(np.column_stack([np.sqrt([0.55, 0.45, 1e-5, 2e-5]), np.zeros(4)]).ravel())
        outs = [torch.empty((8, N), dtype=torch.float64, device=dev), torch.empty(N, dtype=torch.float64, device=dev),
                torch.empty(N, dtype=torch.float64, device=dev), torch.empty(N, dtype=torch.int64, device=dev)]

        def launch():
            nat.sweep_device(stream=stream, n_waves=4, n_points=N, n_steps=n_steps, z_max=z_max, save_every=10,
                             d_dbeta=d_db.data_ptr(), d_dbeta2=0, d_gamma=d_g.data_ptr(), d_alpha=d_al.data_ptr(),
                             d_a0_soa=d_a0.data_ptr(), flags=flags | nat.OPT_ONE_LANE, d_a_end_soa=outs[0].data_ptr(),
                             d_p_end=outs[1].data_ptr(), d_p_max=outs[2].data_ptr(), d_first_bad=outs[3].data_ptr())
        launch.keep = (d_a0, outs)
        return launch

    cands = {"single-pump three-wave": single_pump(), "four-wave one-lane (non-mirrored)": four_wave()}
    times = {k: [] for k in cands}
    print(f"# {nat.version()}; {torch.cuda.get_device_name(0)}; {N} points x {n_steps} steps, save_every 10, check exact, lossy, "
          f"broadcast inputs")
    for rep in range(args.repeats + 1):
        for name, fn in cands.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            if rep:
                times[name].append(ms)
            print(f"  {name}: launch {rep} {ms:9.3f} ms{'  (warm-up)' if not rep else ''}", flush=True)
    best = {k: min(v) for k, v in times.items()}
    for name, v in best.items():
        spread = (max(times[name]) - min(times[name])) / min(times[name])
        print(f"RESULT {name}: best {v:.3f} ms, {v * 1e6 / n_steps:.4f} ns per step of the launch, spread of the repeats {spread:.4%}")
    a, b = best["single-pump three-wave"], best["four-wave one-lane (non-mirrored)"]
    print(f"RESULT ratio three-wave / four-wave {a / b:.4f}")


if __name__ == "__main__":
    main()
