#!/usr/bin/env python3
"""Writes tests/golden/wave_family_parent.npz: what the library built from the commit BEFORE the multi-channel, single-pump and
multi-line sweeps shared one host path returns for the cases of wave_family_parent_cases.py -- every array of every launch
(a_end, p_wave_end, p_wave_max, first_bad_step, and the rows where they are asked for), of the host wrappers, of the `_dev`
entry points on torch buffers and of one two-span chain per family.  Outputs only; repeats stored once.

Needs a GPU, torch and that commit's libpsa_hip.so:
    PSA_HIP_LIB=<the parent build's libpsa_hip.so> python tests/golden/gen_golden_wave_family_parent.py [output.npz]
The generator also checks that the failing cases fail at their one point and nowhere else."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import wave_family_parent_cases as WC  # noqa: E402
import psa_amd._native as nat  # noqa: E402


def main() -> None:
    import torch
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "wave_family_parent.npz")
    print(f"library {nat.LIB_PATH}: {nat.version()}", flush=True)
    records = {}
    for fam, prec, name, N, rows in WC.cases():
        got = WC.run(nat, fam, prec, name, N, rows)
        assert tuple(sorted(got)) == tuple(sorted(WC.FIELDS + (("traj",) if rows else ()))), (fam, prec, name, N, sorted(got))
        bad = got["first_bad_step"]
        if WC.SHAPES[name][2] == "bad":
            assert 0 <= bad[WC.BAD_POINT] < WC.SHAPES[name][0] and (np.delete(bad, WC.BAD_POINT) == -1).all(), (fam, prec, name, N, bad)
        else:
            assert (bad == -1).all(), (fam, prec, name, N, bad)
        for f, a in got.items():
            records[WC.key(fam, prec, name, N, rows, f)] = a
        print(f"  {fam} {prec} {name}{' rows' if rows else ''} N={N}: {sum(a.nbytes for a in got.values())} bytes", flush=True)
    for fam, prec in WC.DEV:
        for padded in (False, True):
            got = WC.run_dev(nat, torch, fam, prec, padded)
            assert (got["first_bad_step"] == -1).all(), (fam, prec, padded)
            for f, a in got.items():
                records[WC.dev_key(fam, prec, padded, f)] = a
            print(f"  {fam} {prec} _dev{' padded rows' if padded else ''}: {sum(a.nbytes for a in got.values())} bytes", flush=True)
    for fam in WC.CHAINS:
        got = WC.run_chain(nat, fam)
        assert (got["first_bad_step"] == -1).all(), fam
        for f, a in got.items():
            records[WC.chain_key(fam, f)] = a
        print(f"  {fam} two spans: {sum(a.nbytes for a in got.values())} bytes", flush=True)
    assert set(records) == WC.expected_keys()
    store = WC.pack(records)
    np.savez_compressed(out_path, **store)
    print(f"{out_path}: {len(records)} arrays, {store['blob'].size} bytes of them, {os.path.getsize(out_path)} bytes")


if __name__ == "__main__":
    main()
