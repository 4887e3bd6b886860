#!/usr/bin/env python3
"""Writes tests/golden/driver_parent.json.gz: what the twelve drivers of the single-pump, multi-channel and multi-line models
did, for the cases of driver_parent_cases.py, at the commit BEFORE simulation.py and scan_mismtach.py shared one driver path
 -- every argument they handed to the eight host functions of _native and everything they returned, or the
exception they raised.  Runs over the stand-in of driver_parent_cases.py: no GPU and no libpsa_hip.so.

    python tests/golden/gen_golden_driver_parent.py [output.json.gz]      (on that commit; the file is not regenerated later)"""
import collections
import gzip
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import driver_parent_cases as DC  # noqa: E402
import psa_amd  # noqa: E402


def main() -> None:
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "driver_parent.json.gz")
    P = DC.package(psa_amd)
    cases = DC.cases(P)
    records = {key: DC.run_case(P, case) for key, case in cases.items()}
    again = {key: DC.run_case(P, case) for key, case in DC.cases(P).items()}
    assert again == records, "the record depends on something besides the cases"
    raised, unexpected = collections.Counter(), []
    for key, rec in records.items():
        failing = key.startswith("err/") or (cases[key][2] is not None and "unchecked" not in key and key.split("/")[0] in
                                             ("run_sp", "run_comb", "cat4", "cat_sp", "cat_comb"))
        if ("raised" in rec) != failing:
            unexpected.append((key, rec.get("raised")))
        if "raised" in rec:
            raised[rec["raised"][0]] += 1
            print(f"  {key}: {rec['raised'][0]}: {rec['raised'][1]}")
        else:
            print(f"  {key}: {[c['fn'] + '@' + str(c['device']) for c in rec['calls']]}")
    assert not unexpected, f"valid cases that raised, failing cases that did not: {unexpected}"
    with gzip.GzipFile(out_path, "wb", mtime=0) as f:
        f.write(json.dumps(records, sort_keys=True, separators=(",", ":")).encode())
    print(f"{out_path}: {len(records)} cases, {len(records) - sum(raised.values())} valid, raised {dict(raised)}, "
          f"{os.path.getsize(out_path)} bytes")


if __name__ == "__main__":
    main()
