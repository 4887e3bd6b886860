#!/usr/bin/env python3
"""Timing of the single-pump three-wave kernels (psa_rk4_single_pump_f64_dev / _f32_dev) for DESIGN.md 3.3c and 3.3d: kernel ms
from events on the launch stream, best of 3 after a warm launch, the candidates alternating in one process.

  python tools/single_pump_timing.py            on one MI355X: 65 536 points x 1e5 steps, lossy, check exact, against the
      4-wave one-lane kernel on NON-MIRRORED inputs (A1 != A2: with equal pumps and equal sidebands that kernel takes its
      174-instruction two-wave loop, which is another comparison)
  python tools/single_pump_timing.py --static   no GPU: compiles csrc/psa_rk4_single_pump.hip to gfx950 assembly and prints,
      per instantiation, VGPRs, scratch and the VALU instructions of one RK4 step (the hot loop holds two); for the float32
      instantiations (csrc/psa_rk4_single_pump_f32.hip) also the packed (v_pk_*) instructions of one step
  python tools/single_pump_timing.py --f32      on one MI355X: (a) the float64 kernel at 65 536 points, (b) the float32 kernel at
      131 072 points (the same 65 536 lanes), (c) the float32 kernel at 65 536 points, all x 1e5 steps, lossy, check exact;
      then the accuracy pass: float32 against the float64 kernel on the same float32-rounded per-point inputs, 4 096 points
      at 1 500, 1e4, 1e5 and 1e6 steps, worst |delta a_end| over the point's largest wave.  PSA_HIP_LIB names another build
      of the library (EXTRA=-DPSA_SINGLE_PUMP_F32_PLAIN: the plain y += inc state update) for the same pass.
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
    """{kernel: (vgprs, spilled vgprs, scratch bytes, VALU per RK4 step, packed VALU per RK4 step)} from the unit's gfx950
    assembly."""
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
        best = packed = 0
        for blk in re.finditer(r"^(\.LBB\d+_\d+):[^\n]*\n(.*?)(?=^\.LBB|\Z)", body, re.S | re.M):
            label, code = blk.groups()
            if re.search(r"s_cbranch_\w+ " + re.escape(label) + r"\b", code):
                n = len(re.findall(r"^\s+v_", code, re.M))
                if n > best:
                    best, packed = n, len(re.findall(r"^\s+v_pk_", code, re.M))
        vgpr = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", meta).group(1))
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", meta).group(1))
        out[name] = (vgpr, spills[name], scratch, best / 2.0, packed / 2.0)
    return out


def print_static():
    print("# static: VGPRs, spilled VGPRs, scratch, VALU instructions per RK4 step from the gfx950 assembly")
    worst = 0
    for name, (vgpr, spill, scratch, valu, _) in sorted(static_counts().items()):
        m = re.search(r"ILi(\d)ELb([01])ELi(\d+)ELb([01])E", name)
        check, traj = "none block exact".split()[int(m.group(1))], m.group(2) == "1"
        block, loss = int(m.group(3)), m.group(4) == "1"
        worst = max(worst, scratch, spill)
        print(f"check={check:5s} traj={int(traj)} block={block:3d} {'lossy   ' if loss else 'lossless'}  VGPRs {vgpr:3d}  spilled {spill}  "
              f"scratch {scratch}  VALU/step {valu:6.1f}")
    ref = static_counts("psa_rk4_f64.hip", "rk4_sweep_kernelIdLi4ELi2ELb0ELi256ELb0ELb1ELb0E")
    for name, (vgpr, spill, scratch, valu, _) in ref.items():
        print(f"4-wave one-lane (check=exact block=256 lossy; the hot loop found is the general, non-mirrored one)  VGPRs {vgpr}  "
              f"scratch {scratch}  VALU/step {valu:.1f}")
    print(f"# worst scratch / spill over the single-pump instantiations: {worst}")
    print("# float32, two points per lane: packed = v_pk_* instructions per RK4 step (for two points)")
    worst = 0
    for name, (vgpr, spill, scratch, valu, packed) in sorted(static_counts("psa_rk4_single_pump_f32.hip",
                                                                           "rk4_sweep_single_pump_pk_kernel").items()):
        m = re.search(r"ILi(\d)ELb([01])ELi(\d+)EE", name)
        check, traj, block = "none block exact".split()[int(m.group(1))], m.group(2) == "1", int(m.group(3))
        worst = max(worst, scratch, spill)
        print(f"f32 check={check:5s} traj={int(traj)} block={block:3d}  VGPRs {vgpr:3d}  spilled {spill}  scratch {scratch}  "
              f"VALU/step {valu:6.1f}  packed/step {packed:6.1f}")
    print(f"# worst scratch / spill over the float32 single-pump instantiations: {worst}")


def parity_inputs(N, seed):
    """The per-point, lossy input generator of tests/test_gpu_single_pump.py (_inputs)."""
    import numpy as np
    GAMMA, P_PUMP, ALPHA = 0.0115, 0.5, 1.15e-4
    rng = np.random.default_rng(seed)
    dbeta = rng.uniform(-4.5, 0.5, N) * GAMMA * P_PUMP
    p = np.column_stack([rng.uniform(0.3, 0.6, N), 10 ** rng.uniform(-12, -2, N), 10 ** rng.uniform(-12, -2, N)])
    a0 = np.sqrt(p) * np.exp(1j * rng.uniform(-3, 3, (N, 3)))
    return dbeta, a0, GAMMA * rng.uniform(0.9, 1.1, N), ALPHA * rng.uniform(0.5, 1.5, N)


def run_f32(args):
    import numpy as np
    import torch
    import psa_amd._native as nat
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    flags = nat.BCAST_GAMMA | nat.BCAST_ALPHA | nat.BCAST_A0 | nat.OPT_CHECK_NAN | nat.OPT_EXACT_STEP
    n_steps, z_max = args.steps, 0.1 * args.steps

    def candidate(N, dtype):
        tdt = torch.float64 if dtype == np.float64 else torch.float32
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).to(dev)   # noqa: E731
        ins = [t(np.linspace(-0.05, 0.05, N)), t([0.0115]), t([1.15e-4]),
               t(np.column_stack([np.sqrt([1.0, 1e-5, 1e-5]), np.zeros(3)]).ravel())]
        outs = [torch.empty((6, N), dtype=tdt, device=dev), torch.empty((3, N), dtype=tdt, device=dev),
                torch.empty((3, N), dtype=tdt, device=dev), torch.empty(N, dtype=torch.int64, device=dev)]

        def launch():
            nat.single_pump_device(stream=stream, n_points=N, n_steps=n_steps, z_max=z_max, save_every=10, d_dbeta=ins[0].data_ptr(),
                                   d_gamma=ins[1].data_ptr(), d_alpha=ins[2].data_ptr(), d_a0_soa=ins[3].data_ptr(), flags=flags,
                                   d_a_end_soa=outs[0].data_ptr(), d_p_wave_end_soa=outs[1].data_ptr(),
                                   d_p_wave_max_soa=outs[2].data_ptr(), d_first_bad=outs[3].data_ptr(), dtype=dtype)
        launch.keep, launch.points = (ins, outs), N
        return launch

    P = args.points
    cands = {"(a) float64": candidate(P, np.float64), "(b) float32 2x points": candidate(2 * P, np.float32),
             "(c) float32": candidate(P, np.float32)}
    times = {k: [] for k in cands}
    print(f"# {nat.version()}; {torch.cuda.get_device_name(0)}; library {os.path.relpath(nat.LIB_PATH, ROOT)}")
    print(f"# timing: {n_steps} steps, save_every 10, check exact, lossy, broadcast inputs; (a) and (c) {P} points, (b) {2 * P}")
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
        print(f"RESULT {name}: best {v:.3f} ms, {v * 1e6 / n_steps / cands[name].points * 1e3:.5f} ps per point-step, "
              f"spread of the repeats {spread:.4%}")
    a = best["(a) float64"]
    print(f"RESULT time (b)/(a) {best['(b) float32 2x points'] / a:.4f}  per point-step {best['(b) float32 2x points'] / a / 2:.4f}")
    print(f"RESULT time (c)/(a) {best['(c) float32'] / a:.4f}  per point-step {best['(c) float32'] / a:.4f}")

    print("# accuracy: float32 against the float64 kernel on the same float32-rounded inputs, 4 096 per-point lossy points, "
          "z_max 1000, worst |delta a_end| over the point's largest wave")
    dbeta, a0, gamma, alpha = parity_inputs(4096, 12)
    dbeta, gamma, alpha, a0 = (dbeta.astype(np.float32), gamma.astype(np.float32), alpha.astype(np.float32), a0.astype(np.complex64))
    for n in (1500, 10_000, 100_000, 1_000_000):
        kw = dict(n_steps=n, z_max=1000.0, save_every=n, gamma=gamma, alpha=alpha, a0=a0)
        lo = nat.single_pump_host(dbeta, dtype=np.float32, **kw)
        hi = nat.single_pump_host(dbeta.astype(np.float64), **dict(kw, gamma=gamma.astype(np.float64), alpha=alpha.astype(np.float64),
                                                                  a0=a0.astype(np.complex128)))
        scale = np.abs(hi["a_end"]).max(axis=1, keepdims=True)
        err = np.abs(lo["a_end"].astype(np.complex128) - hi["a_end"]) / scale
        bad = int((lo["first_bad_step"] >= 0).sum() + (hi["first_bad_step"] >= 0).sum())
        print(f"ACCURACY steps {n:8d}: worst {err.max():.3e}  median of the points' worst {np.median(err.max(axis=1)):.3e}  "
              f"non-finite points {bad}  (float32 kernel {lo['elapsed_ms']:.2f} ms, float64 {hi['elapsed_ms']:.2f} ms)", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--static", action="store_true")
    ap.add_argument("--f32", action="store_true", help="float32 against float64: timings (a), (b), (c) and the accuracy pass")
    ap.add_argument("--steps", type=int, default=STEPS)
    ap.add_argument("--points", type=int, default=POINTS)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    if args.static:
        print_static()
        return
    if args.f32:
        run_f32(args)
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
