"""The IK-GAT entries compute and refuse what they did before csrc/k2b_ikgat_plan.h existed.

``tests/golden/ikgat_parent_bits.npz`` holds, for the smallest nets that reach every branch of the set-up and of the layout
(``tests/ikgat_cases.py``, BITS_CASES), the inputs and the output quaternions of the library at the commit before the header, run on
an MI355X (``tools/record_ikgat_parent.py``).  The comparison is exact, as integers.  The predict refusals of that library are in
``tests/golden/ikgat_refusals.json``."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import ikgat_cases as T

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"


@pytest.fixture(scope="module")
def recorded():
    with np.load(GOLDEN / "ikgat_parent_bits.npz") as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("i", range(len(T.BITS_CASES)), ids=[c["id"] for c in T.BITS_CASES])
def test_output_bits_are_the_parents(recorded, i):
    case = T.BITS_CASES[i]
    net = T.bits_net(i, case)
    pos, q = recorded[case["id"] + ".positions"], recorded.get(case["id"] + ".quat_in")
    assert (q is None) == (case["dims"][1] == 3) and pos.shape == (case["frames"], case["dims"][0], 3)
    got = net.predict(torch.as_tensor(pos, device=net.device), None if q is None else torch.as_tensor(q, device=net.device),
                      chain=case["chain"]).cpu().numpy()
    want = recorded[case["id"] + ".quaternions"]
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), int((got.view(np.int32) != want.view(np.int32)).sum())


def test_predict_refusals_are_the_parents(recorded):
    want = json.loads((GOLDEN / "ikgat_refusals.json").read_text())["predict"]
    case = T.BITS_CASES[0]
    net = T.bits_net(0, case)
    pos = torch.as_tensor(recorded[case["id"] + ".positions"], device=net.device)
    q = torch.as_tensor(recorded[case["id"] + ".quat_in"], device=net.device)
    out = torch.empty((case["frames"], case["dims"][0], 4), device=net.device)
    for cid in T.PREDICT_CASES:
        code, message = T.run_predict(cid, net, pos, q, out)
        assert {"code": code, "message": message} == want[cid], cid
    torch.cuda.synchronize()
