#!/usr/bin/env python3
"""Python cost of the twelve drivers of simulation.py / scan_mismtach.py that share one driver path, this
tree against another revision's two modules.  No GPU: the drivers run over the stand-in of the eight host functions in
tests/golden/driver_parent_cases.py, so what is timed is the drivers' own Python and NumPy.

Both builds are loaded into ONE process under different package names -- this tree as it is, and a copy whose simulation.py and
scan_mismtach.py come from ``--parent`` (a git revision, default HEAD~1; every other module is this tree's) -- and their calls
alternate, ``--calls`` each per driver, in ``--rounds`` fresh processes: a fresh process per build does not separate builds at
this scale.  Per driver: the median of a call in microseconds per round and build, and whether the median of
this build's rounds lies inside the spread of the parent's.

    python tools/driver_path_timing.py [--parent REV] [--calls 1000] [--rounds 3] > profiles/driver_path.log"""
import argparse
import importlib.util
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "psa-simulation-ode-rk-mvp-dispersion_amd")
MODULES = ("simulation.py", "scan_mismtach.py")
# one valid case per driver: a copier where there is one, two spans, K = 3 and M = 5
CASES = ("run_sp/m", "run_comb/km5_dark", "cat4/m", "cat_sp/m", "cat_comb/m3", "wdm/k3", "sp_gain/m", "comb_gain/m5_dark",
         "psa4/copier_defaults", "psa_sp/copier_defaults", "psa_wdm/copier_defaults", "psa_comb/copier_defaults")


def load(name: str, first_dir=None):
    """The package under ``name``; modules found in ``first_dir`` take precedence over the tree's."""
    path = ([first_dir] if first_dir else []) + [PKG]
    spec = importlib.util.spec_from_file_location(name, os.path.join(PKG, "__init__.py"), submodule_search_locations=path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def one_round(parent_dir: str, calls: int) -> dict:
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import driver_parent_cases as DC
    builds = {"parent": DC.package(load("psa_parent", parent_dir)), "this": DC.package(load("psa_this"))}
    assert builds["parent"].simulation.__file__.startswith(parent_dir) and builds["this"].simulation.__file__.startswith(PKG)
    out = {}
    for key in CASES:
        runs, times = {}, {b: [] for b in builds}
        for b, P in builds.items():
            fn, kw, bad = DC.cases(P)[key]
            stand_in = DC.StandIn(bad)
            stand_in.install(P.native)
            runs[b] = (fn, kw, stand_in)
            fn(**kw)                                   # imports inside the driver, first-call caches
        for _ in range(calls):
            for b, (fn, kw, stand_in) in runs.items():
                stand_in.calls.clear()
                t0 = time.perf_counter()
                fn(**kw)
                times[b].append(time.perf_counter() - t0)
        out[key] = {b: statistics.median(t) * 1e6 for b, t in times.items()}
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--parent", default="HEAD~1", help="git revision whose simulation.py and scan_mismtach.py are the parent's")
    ap.add_argument("--calls", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--round-of", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.round_of:
        print(json.dumps(one_round(args.round_of, args.calls)))
        return
    with tempfile.TemporaryDirectory() as tmp:
        for m in MODULES:
            text = subprocess.run(["git", "-C", ROOT, "show", f"{args.parent}:{os.path.basename(PKG)}/{m}"], check=True,
                                  capture_output=True).stdout
            with open(os.path.join(tmp, m), "wb") as f:
                f.write(text)
        rounds = [json.loads(subprocess.run([sys.executable, os.path.abspath(__file__), "--round-of", tmp, "--calls", str(args.calls)],
                                            check=True, capture_output=True, text=True).stdout) for _ in range(args.rounds)]
    rev = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", args.parent], capture_output=True, text=True).stdout.strip()
    print(f"driver cost over the stand-in: parent = {args.parent} ({rev}), {args.calls} alternating calls per driver and build, "
          f"{args.rounds} fresh processes; median of one call in us")
    print(f"{'driver (case)':<28} {'parent':<24} {'this build':<24} {'this - parent':<22} median of this build")
    fmt = lambda v: "  ".join(f"{x:6.1f}" for x in v)   # noqa: E731
    for key in CASES:
        par, new = [r[key]["parent"] for r in rounds], [r[key]["this"] for r in rounds]
        med = statistics.median(new)
        where = "inside" if min(par) <= med <= max(par) else ("below" if med < min(par) else "ABOVE")
        print(f"{key:<28} {fmt(par):<24} {fmt(new):<24} {'  '.join(f'{n - p:+5.1f}' for n, p in zip(new, par)):<22} "
              f"{med:.1f}: {where} the parent's {min(par):.1f} - {max(par):.1f}")


if __name__ == "__main__":
    main()
