#!/usr/bin/env python3
"""Writes tests/golden/chain_twin_parent.json: the digests of what ``chain`` and ``direct`` of the three NumPy chain
restatements returned, for the cases of chain_twin_parent_cases.py, at the commit BEFORE the three twins shared the span loop
of tests/chain_np.py.  NumPy alone: no GPU and no libpsa_hip.so.

    python tests/golden/gen_golden_chain_twin_parent.py [output.json]      (on that commit; the file is not regenerated later)"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import chain_twin_parent_cases as TC  # noqa: E402


def main() -> None:
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "chain_twin_parent.json")
    records = {key: TC.run_case(case) for key, case in TC.cases().items()}
    again = {key: TC.run_case(case) for key, case in TC.cases().items()}
    assert again == records, "the record depends on something besides the cases"
    with open(out_path, "w") as f:
        json.dump(records, f, sort_keys=True, indent=0)
        f.write("\n")
    print(f"{out_path}: {len(records)} cases, {sum(len(r) for r in records.values())} digests, {os.path.getsize(out_path)} bytes")


if __name__ == "__main__":
    main()
