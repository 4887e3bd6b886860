#!/usr/bin/env python3
"""Writes tests/golden/chain_parent.npz: what the library built from the commit BEFORE the two chain families shared one
host path returns for the cases of chain_parent_cases.py -- every array of every launch (a_end, the family's summaries,
first_bad_step, and the trajectory where one is asked for).  Outputs only; repeats stored once.

Needs a GPU and that commit's libpsa_hip.so:
    PSA_HIP_LIB=<the parent build's libpsa_hip.so> python tests/golden/gen_golden_chain_parent.py [output.npz]
The generator also checks that the failing cases fail where they are meant to: in the second span, at one point."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import chain_parent_cases as CC  # noqa: E402
import psa_amd._native as nat  # noqa: E402


def main() -> None:
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "chain_parent.npz")
    print(f"library {nat.LIB_PATH}: {nat.version()}", flush=True)
    records = {}
    for fam, prec, name, N in CC.cases():
        got = CC.run(nat, fam, prec, name, N)
        assert tuple(sorted(got)) == tuple(sorted(CC.expected_fields(fam, name))), (fam, prec, name, N, sorted(got))
        bad = got["first_bad_step"]
        if CC.SHAPES[name][7]:
            first = CC.STEPS[CC.SHAPES[name][0]][0]
            assert first <= bad[CC.BAD_POINT] < first + CC.STEPS[CC.SHAPES[name][0]][1], (fam, prec, name, N, bad)
            assert (np.delete(bad, CC.BAD_POINT) == -1).all(), (fam, prec, name, N, bad)
        else:
            assert (bad == -1).all(), (fam, prec, name, N, bad)
        for f, a in got.items():
            records[CC.key(fam, prec, name, N, f)] = a
        print(f"  {fam} {prec} {name} N={N}: {sum(a.nbytes for a in got.values())} bytes", flush=True)
    store = CC.pack(records)
    np.savez_compressed(out_path, **store)
    print(f"{out_path}: {len(records)} arrays, {store['blob'].size} bytes of them, {os.path.getsize(out_path)} bytes")


if __name__ == "__main__":
    main()
