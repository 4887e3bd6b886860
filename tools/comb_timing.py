#!/usr/bin/env python3
"""Resources and timing of the multi-line ("comb") sweep kernels (psa_rk4_comb_f64, psa_rk4_comb_f32) for DESIGN.md 3.3e, 3.3f.

  python tools/comb_timing.py --static   no GPU: compiles csrc/psa_rk4_comb.hip to gfx950 assembly with the Makefile's flags
      and prints, per instantiation, VGPRs, AGPRs, scratch, waves per SIMD and the VALU instructions of one RK4 step (the hot
      loop holds one step), the moves between VGPRs and AGPRs among them counted apart; --remarks FILE also keeps the
      compiler's -Rpass-analysis=kernel-resource-usage output (profiles/comb_resources.txt)
  python tools/comb_timing.py            on one MI355X: 65 536 points x 10 000 steps, lossy, check on, save_every 10, for
      M in 3, 4, 6, 7, 9, 12 and the single-pump kernel at the same size, in one process: a warm-up launch of every candidate,
      then best of 3 of the kernel time the host entry reports (hipEvents on the launch stream); with the static counts the
      implied VALU issue rate next to the single-pump kernel's
  python tools/comb_timing.py --f32 --static   the same counts for csrc/psa_rk4_comb_f32.hip (two points per lane), with the
      static expectation of its time per point-step over the float64 kernel's, I_pk / (2 I_f64)
  python tools/comb_timing.py --f32      on one MI355X, per M and in one process: (a) the float64 kernel at 65 536 points, (b) the
      float32 kernel at 131 072 points (the same lanes), (c) the float32 kernel at 65 536 points; milliseconds, ps per
      point-step and (b)/(a) per point-step beside the static expectation.  Then the accuracy pass on the parity tests' lossy
      inputs (tests/comb_np.random_inputs, rounded to float32): worst |a_end(float32 kernel) - a_end(float64 kernel)| over the
      point's largest line at 1 500, 10 000 and 100 000 steps.  PSA_HIP_LIB selects another build of the library for the same
      run: EXTRA=-DPSA_COMB_F32_PLAIN (the plain y += inc state update), EXTRA=-DPSA_COMB_F32_RESYNC=8 (a shorter seed interval),
      EXTRA=-DPSA_COMB_F32_NORENORM (u_m carried without the per-step renormalisation).
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
STEPS, POINTS, LINES = 10_000, 65_536, (3, 4, 6, 7, 9, 12)


def static_counts(unit, pattern, remarks=None):
    """{kernel: dict(vgpr, agpr, scratch, occupancy, valu, acc)} from the unit's gfx950 assembly and resource remarks; valu =
    v_* instructions of the hot loop (the self-looping block with the most of them), acc = the v_accvgpr_* among them."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "unit.s")
        res = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                              "-mllvm", "-amdgpu-sched-strategy=max-ilp", "-mllvm", "-align-all-blocks=3", "-S", "--cuda-device-only",
                              "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, unit), "-o", asm], check=True,
                             stderr=subprocess.PIPE, text=True)
        text = open(asm).read()
    lines = [re.sub(r"^.*?remark: ", "", ln).replace(" [-Rpass-analysis=kernel-resource-usage]", "")
             for ln in res.stderr.splitlines() if "remark:" in ln]
    if remarks:
        with open(remarks, "w") as f:
            f.write("\n".join(lines) + "\n")
    usage = {}
    for blk in "\n".join(lines).split("Function Name: ")[1:]:
        g = lambda key: int(re.search(key + r"[^:\n]*: (\d+)", blk).group(1))   # noqa: E731
        usage[blk.split()[0]] = dict(vgpr=g("VGPRs"), agpr=g("AGPRs"), scratch=g("ScratchSize"), occupancy=g("Occupancy"))
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)\n\s*\.amdhsa_kernel \1\n", text, re.S | re.M):
        name, body = m.groups()
        if pattern not in name:
            continue
        best = acc = 0
        for blk in re.finditer(r"^(\.LBB\d+_\d+):[^\n]*\n(.*?)(?=^\.LBB|\Z)", body, re.S | re.M):
            label, code = blk.groups()
            if re.search(r"s_cbranch_\w+ " + re.escape(label) + r"\b", code):
                n = len(re.findall(r"^\s+v_", code, re.M))
                if n > best:
                    best, acc = n, len(re.findall(r"^\s+v_accvgpr_", code, re.M))
        out[name] = dict(usage[name], valu=best, acc=acc)
    return out


def comb_static(remarks=None):
    """{(M, check, loss): counts} of every comb instantiation."""
    out = {}
    for name, c in static_counts("psa_rk4_comb.hip", "rk4_sweep_comb_kernel", remarks).items():
        m = re.search(r"ILi(\d+)ELb([01])ELb([01])E", name)
        out[int(m.group(1)), m.group(2) == "1", m.group(3) == "1"] = c
    return out


def print_static(remarks):
    print("# static: registers, scratch, waves per SIMD and the VALU instructions of one RK4 step from the gfx950 assembly;")
    print("# 24 M^2 + 56 M is the step's FP64 arithmetic with loss (8 M fewer without), + 2 M + 3 for the test")
    worst = 0
    for (M, check, loss), c in sorted(comb_static(remarks).items()):
        worst = max(worst, c["scratch"])
        print(f"M={M:2d} check={int(check)} {'lossy   ' if loss else 'lossless'}  VGPRs {c['vgpr']:3d}  AGPRs {c['agpr']:3d}  scratch "
              f"{c['scratch']}  waves/SIMD {c['occupancy']}  VALU/step {c['valu']:5d}  of them AGPR moves {c['acc']:4d}  "
              f"(24 M^2 + 56 M = {24 * M * M + 56 * M})")
    print(f"# worst scratch over the comb instantiations: {worst}")


def comb_f32_static(remarks=None):
    """{(M, check): counts} of every float32 comb instantiation."""
    out = {}
    for name, c in static_counts("psa_rk4_comb_f32.hip", "rk4_sweep_comb_pk_kernel", remarks).items():
        m = re.search(r"ILi(\d+)ELb([01])E", name)
        out[int(m.group(1)), m.group(2) == "1"] = c
    return out


def print_static_f32(remarks):
    print("# static, float32 (two points per lane): registers, scratch, waves per SIMD and the VALU instructions of one RK4 step;")
    print("# 24 M^2 + 69 M is the step's packed arithmetic for two points, + 2 M for the test; expectation = I_pk / (2 I_f64) as built")
    f64 = comb_static()
    worst = 0
    for (M, check), c in sorted(comb_f32_static(remarks).items()):
        worst = max(worst, c["scratch"])
        print(f"M={M:2d} check={int(check)}  VGPRs {c['vgpr']:3d}  AGPRs {c['agpr']:3d}  scratch {c['scratch']}  waves/SIMD {c['occupancy']}  "
              f"VALU/step {c['valu']:5d}  of them AGPR moves {c['acc']:4d}  (24 M^2 + 69 M = {24 * M * M + 69 * M})  "
              f"expectation {c['valu'] / (2.0 * f64[M, check, True]['valu']):.3f}")
    print(f"# worst scratch over the float32 comb instantiations: {worst}")


def run_f32(args):
    import numpy as np
    import psa_amd._native as nat
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import comb_np
    N, n_steps = args.points, args.steps
    rng = np.random.default_rng(1)
    grid = dict(n_steps=n_steps, z_max=0.1 * n_steps, save_every=10, gamma=0.0115, alpha=1.15e-4)

    def comb(M, n, dtype):
        x = np.arange(M) - 0.5 * (M - 1)
        kappa = x ** 2 * rng.uniform(-2e-3, 5e-4, (n, 1)) + x ** 3 * rng.uniform(-1e-4, 1e-4, (n, 1))
        p = np.full(M, 1e-5)
        p[1] = p[M - 2] = 0.3
        return lambda: nat.comb_host(kappa, a0=np.sqrt(p).astype(complex), dtype=dtype, **grid)

    cands = {}
    for M in args.lines:
        cands[M, "a"] = comb(M, N, np.float64)
        cands[M, "b"] = comb(M, 2 * N, np.float32)
        cands[M, "c"] = comb(M, N, np.float32)
    print(f"# {nat.version()} ({nat.LIB_PATH}); {n_steps} steps, save_every 10, check on, lossy, broadcast gamma / alpha / a0; (a) float64 "
          f"{N} points, (b) float32 {2 * N} points, (c) float32 {N} points", flush=True)
    times = {k: [] for k in cands}
    for rep in range(args.repeats + 1):
        for (M, which), fn in cands.items():
            r = fn()
            assert (r["first_bad_step"] == -1).all(), (M, which)
            if rep:
                times[M, which].append(r["elapsed_ms"])
            print(f"  M={M} ({which}): launch {rep} {r['elapsed_ms']:9.3f} ms{'  (warm-up)' if not rep else ''}", flush=True)
    f64, f32 = (None, None) if args.no_static else (comb_static(), comb_f32_static())
    for M in args.lines:
        best = {w: min(times[M, w]) for w in "abc"}
        spread = {w: (max(times[M, w]) - best[w]) / best[w] for w in "abc"}
        pts = dict(a=N, b=2 * N, c=N)
        ps = {w: best[w] * 1e9 / n_steps / pts[w] for w in "abc"}
        print(f"RESULT M={M}: (a) {best['a']:.3f} ms {ps['a']:.2f} ps/point-step (spread {spread['a']:.2%}); (b) {best['b']:.3f} ms "
              f"{ps['b']:.2f} ps (spread {spread['b']:.2%}); (c) {best['c']:.3f} ms {ps['c']:.2f} ps (spread {spread['c']:.2%}); "
              f"(b)/(a) per point-step {ps['b'] / ps['a']:.3f}; (c)/(a) {ps['c'] / ps['a']:.3f}"
              + ("" if f32 is None else f"; static expectation {f32[M, True]['valu'] / (2.0 * f64[M, True, True]['valu']):.3f} (VALU/step "
                 f"{f32[M, True]['valu']} of them AGPR moves {f32[M, True]['acc']}, float64 {f64[M, True, True]['valu']} / {f64[M, True, True]['acc']})"))
    # accuracy: the float32 kernel against the float64 kernel on the same rounded inputs
    for M in args.lines:
        kappa, a0, gamma, alpha = comb_np.random_inputs(203, M, 100 * M + 3)
        kappa, a0, gamma, alpha = kappa.astype(np.float32), a0.astype(np.complex64), gamma.astype(np.float32), alpha.astype(np.float32)
        for steps in (1_500, 10_000, 100_000):
            z_max = 300.0 if steps == 1_500 else 1000.0         # the fibres of the truth tests
            kw = dict(n_steps=steps, z_max=z_max, save_every=10, gamma=gamma, alpha=alpha, a0=a0)
            lo, hi = nat.comb_host(kappa, dtype=np.float32, **kw), nat.comb_host(kappa, **kw)
            assert (lo["first_bad_step"] == -1).all() and (hi["first_bad_step"] == -1).all()
            e = np.max(np.abs(lo["a_end"].astype(complex) - hi["a_end"]), axis=1) / np.max(np.abs(hi["a_end"]), axis=1)
            print(f"ACCURACY M={M} {steps} steps over {z_max:g} m: a_end float32 against float64 kernel, median {np.median(e):.2e} "
                  f"worst {e.max():.2e}", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--static", action="store_true")
    ap.add_argument("--remarks", default=None, help="with --static: keep the compiler's resource remarks in this file")
    ap.add_argument("--steps", type=int, default=STEPS)
    ap.add_argument("--points", type=int, default=POINTS)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--f32", action="store_true", help="the float32 kernel (two points per lane) beside the float64 one")
    ap.add_argument("--lines", type=int, nargs="+", default=list(LINES), help="with --f32: the M to run")
    ap.add_argument("--no-static", action="store_true", help="with --f32: leave the static expectation out (no compiler run)")
    args = ap.parse_args()
    if args.static:
        (print_static_f32 if args.f32 else print_static)(args.remarks)
        return
    if args.f32:
        run_f32(args)
        return
    import numpy as np
    import psa_amd._native as nat
    N, n_steps = args.points, args.steps
    z_max = 0.1 * n_steps
    rng = np.random.default_rng(1)
    grid = dict(n_steps=n_steps, z_max=z_max, save_every=10, gamma=0.0115, alpha=1.15e-4)

    def comb(M):
        x = np.arange(M) - 0.5 * (M - 1)
        kappa = x ** 2 * rng.uniform(-2e-3, 5e-4, (N, 1)) + x ** 3 * rng.uniform(-1e-4, 1e-4, (N, 1))
        p = np.full(M, 1e-5)
        p[1] = p[M - 2] = 0.3
        return lambda: nat.comb_host(kappa, a0=np.sqrt(p).astype(complex), **grid)

    def single_pump():
        dbeta = np.linspace(-0.05, 0.05, N)
        return lambda: nat.single_pump_host(dbeta, a0=np.sqrt([0.6, 1e-5, 1e-5]).astype(complex), **grid)

    cands = {f"comb M={M}": comb(M) for M in LINES}
    cands["single-pump"] = single_pump()
    print(f"# {nat.version()}; {N} points x {n_steps} steps, save_every 10, check on, lossy, broadcast gamma / alpha / a0", flush=True)
    times = {k: [] for k in cands}
    for rep in range(args.repeats + 1):
        for name, fn in cands.items():
            r = fn()
            assert (r["first_bad_step"] == -1).all(), name
            if rep:
                times[name].append(r["elapsed_ms"])
            print(f"  {name}: launch {rep} {r['elapsed_ms']:9.3f} ms{'  (warm-up)' if not rep else ''}", flush=True)
    static = comb_static()
    sp = [c for n, c in static_counts("psa_rk4_single_pump.hip", "rk4_sweep_single_pump_kernelILi2ELb0ELi256ELb1E").items()]
    sp_valu = sp[0]["valu"] / 2.0     # that kernel's hot loop holds two steps
    best = {k: min(v) for k, v in times.items()}
    rate = lambda valu, ms: valu * n_steps * ((N + 63) // 64) / (ms * 1e-3) / 1e9      # noqa: E731  wave instructions per ns, all SIMDs
    sp_rate = rate(sp_valu, best["single-pump"])
    print(f"RESULT single-pump: best {best['single-pump']:.3f} ms, {best['single-pump'] * 1e6 / n_steps / N:.5f} ns per point-step, "
          f"VALU/step {sp_valu:.1f}, issue rate {sp_rate:.1f} wave instructions per ns")
    for M in LINES:
        name, c = f"comb M={M}", static[M, True, True]
        ms = best[name]
        spread = (max(times[name]) - ms) / ms
        print(f"RESULT {name}: best {ms:.3f} ms, {ms * 1e6 / n_steps / N:.5f} ns per point-step, VALU/step {c['valu']} (AGPR moves "
              f"{c['acc']}), waves/SIMD {c['occupancy']}, issue rate {rate(c['valu'], ms):.1f} = {rate(c['valu'], ms) / sp_rate:.3f} of the "
              f"single-pump kernel's, time over single-pump {ms / best['single-pump']:.3f}, spread {spread:.3%}")


if __name__ == "__main__":
    main()
