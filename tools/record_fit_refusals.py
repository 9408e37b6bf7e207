#!/usr/bin/env python3
"""Run the table of refused fit calls (tests/fit_refusal_cases.py) through the real entries of libk2b.so and write the code and
``k2b_last_error()`` of every row as JSON.

    python tools/record_fit_refusals.py --out tests/golden/fit_refusals.json

The committed recording was made on an MI355X at the commit BEFORE csrc/k2b_fit_rules.h existed: it is the reference the rules are
held to and is not regenerated from a later library.  A row that the library accepts is a mistake in the table: it is reported,
the exit status is 1 and nothing is written."""
import argparse
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

from tests import fit_refusal_cases as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", required=True)
    ap.add_argument("--only", default="", help="comma-separated row ids")
    args = ap.parse_args()
    import torch

    h = T.Handles()
    only = set(filter(None, args.only.split(",")))
    recorded, accepted = {}, []
    for case in T.CASES:
        if only and case["id"] not in only:
            continue
        print(case["id"], end=" ", flush=True)
        code, message = T.run_case(h, case)
        torch.cuda.synchronize()
        print(code, message, flush=True)
        if code == 0:
            accepted.append(case["id"])
        recorded[case["id"]] = {"entry": "k2b_" + case["entry"], "code": code, "message": message}
    if accepted:
        print(f"accepted by the library (fix the table): {accepted}", file=sys.stderr)
        Path(args.out + ".partial").write_text(json.dumps(recorded, indent=1) + "\n")      # (to look at, not the recording)
        return 1
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(recorded, indent=1) + "\n")
    print(f"{len(recorded)} refusals -> {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
