#!/usr/bin/env python3
"""Record what the IK-GAT entries of libk2b.so refuse and compute (tables: tests/ikgat_cases.py).

    python tools/record_ikgat_parent.py create  --out tests/golden/ikgat_refusals.json       (no GPU needed)
    python tools/record_ikgat_parent.py predict --out tests/golden/ikgat_refusals.json       (adds the predict rows; MI355X)
    python tools/record_ikgat_parent.py bits    --out tests/golden/ikgat_parent_bits.npz     (MI355X)

The committed recordings were made with the library at the commit BEFORE csrc/k2b_ikgat_plan.h existed: they are what the header
and the entries are held to and are not regenerated from a later library.  Every refusal of k2b_ikgat_create comes before its
device query, so `create` runs anywhere; its first row passes every check and is recorded as code 0 whether or not a device then
answers."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

from keypoints2body_amd import native  # noqa: E402
from tests import ikgat_cases as T  # noqa: E402


def _merge(path, key, rows):
    path = Path(path)
    doc = json.loads(path.read_text()) if path.exists() else {}
    doc[key] = rows
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(doc, indent=1) + "\n")
    print(f"{len(rows)} {key} rows -> {path}")


def record_create(out):
    rows = {}
    for case in T.CREATE_CASES:
        code, message = T.run_create(case)
        if case["id"] == "accepted":
            assert code in (native.K2B_OK, native.K2B_ERR_NO_DEVICE), (code, message)
            code, message = 0, ""
        else:
            assert code in (native.K2B_ERR_INVALID_ARGUMENT, native.K2B_ERR_UNSUPPORTED), (case["id"], code, message)
        print(case["id"], code, message)
        rows[case["id"]] = {"code": code, "message": message}
    _merge(out, "create", rows)


def record_predict(out):
    import torch
    case = T.BITS_CASES[0]
    net = T.bits_net(0, case)
    pos, q = (torch.as_tensor(a, device=net.device) for a in T.bits_inputs(0, case))
    res = torch.empty((case["frames"], case["dims"][0], 4), device=net.device)
    rows = {}
    for cid in T.PREDICT_CASES:
        code, message = T.run_predict(cid, net, pos, q, res)
        assert code != native.K2B_OK, cid
        print(cid, code, message)
        rows[cid] = {"code": code, "message": message}
    torch.cuda.synchronize()
    _merge(out, "predict", rows)


def record_bits(out):
    import torch
    arrays = {}
    for i, case in enumerate(T.BITS_CASES):
        net = T.bits_net(i, case)
        pos, q = T.bits_inputs(i, case)
        got = net.predict(torch.as_tensor(pos, device=net.device), None if q is None else torch.as_tensor(q, device=net.device),
                          chain=case["chain"]).cpu().numpy()
        assert got.dtype == np.float32 and np.isfinite(got).all()
        arrays[case["id"] + ".positions"] = pos
        if q is not None:
            arrays[case["id"] + ".quat_in"] = q
        arrays[case["id"] + ".quaternions"] = got
        print(case["id"], got.shape, float(np.abs(got).sum()))
    Path(out).parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(out, **arrays)
    print(f"{len(T.BITS_CASES)} cases -> {out}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=("create", "predict", "bits"))
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    {"create": record_create, "predict": record_predict, "bits": record_bits}[args.what](args.out)
