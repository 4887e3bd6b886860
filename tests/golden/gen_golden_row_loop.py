#!/usr/bin/env python3
"""Writes tests/golden/row_loop_parent.npz: what the library built from the commit BEFORE the row-driven z-loop returns for
the case grid of row_loop_cases.py -- every output of every summary launch (a_end, p_end, p_max, first_bad_step, and
p_wave_end / p_wave_max where the per-wave summary is on), 131 points each.  Outputs only; repeats stored once.

Needs a GPU and that commit's libpsa_hip.so:
    PSA_HIP_LIB=<the parent build's libpsa_hip.so> python tests/golden/gen_golden_row_loop.py [output.npz]
The generator also checks, on that build, what the test relies on when it compares a 67-point launch with the first 67
rows of the record: a launch's size changes no bit of a point."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import row_loop_cases as RC  # noqa: E402
import psa_amd._native as nat  # noqa: E402


def same(a, b) -> bool:
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def main() -> None:
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "row_loop_parent.npz")
    print(f"library {nat.LIB_PATH}: {nat.version()}", flush=True)
    records = {}
    for which in RC.SETS:
        for n_steps, se in RC.STEPS:
            for check, lossy, wsum, block in RC.variants():
                got = RC.run(nat, which, RC.N_ALL, n_steps, se, check, lossy, wsum, block)
                small = RC.run(nat, which, 67, n_steps, se, check, lossy, wsum, block)
                for f in RC.FIELDS + (RC.WAVE_FIELDS if wsum else ()):
                    assert same(small[f], got[f][:67]), (which, n_steps, se, check, lossy, wsum, block, f)
                    records[RC.key(which, n_steps, se, check, lossy, wsum, block, f)] = got[f]
            print(f"  {which} {n_steps} x {se}: recorded", flush=True)
    store = RC.pack(records)
    np.savez_compressed(out_path, **store)
    print(f"{out_path}: {len(records)} arrays, {len(store) - 1} stored, {os.path.getsize(out_path)} bytes")


if __name__ == "__main__":
    main()
