"""What the ten fit entries refuse, on the device: the table of bad calls (``tests/fit_refusal_cases.py``) through the real entries
of ``libk2b.so``, held to the code and the message that the entries gave before ``csrc/k2b_fit_rules.h`` existed
(``tests/golden/fit_refusals.json``), exactly - and the one intended difference: a refusal comes before anything is queued.  No fit
kernel is launched here."""
import json
from pathlib import Path

import pytest
import torch

from tests import fit_refusal_cases as T

pytestmark = pytest.mark.gpu

GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "fit_refusals.json").read_text())


@pytest.fixture(scope="module")
def handles():
    return T.Handles()


def test_every_entry_refuses_what_it_always_refused_in_the_same_words(handles):
    wrong = []
    for case in T.CASES:
        code, message = T.run_case(handles, case)
        want = GOLDEN[case["id"]]
        if (code, message) != (want["code"], want["message"]):
            wrong.append(f"{case['id']}: got {code} {message!r}, recorded {want['code']} {want['message']!r}")
    torch.cuda.synchronize()
    assert not wrong, "\n".join(wrong)
    assert len(T.CASES) == len(GOLDEN)


@pytest.mark.parametrize("case_id", ("l_dup", "sl_dup", "sl_tree_dup", "ql_dup"))
def test_a_refused_lbfgs_call_leaves_its_outputs_alone(handles, case_id):
    """Two frames (the chain entries: one sequence of two), the same kinematic joint targeted twice, inputs and outputs distinct
    arrays: K2B_ERR_UNSUPPORTED in k2b_fit_world's words, and after a stream synchronise the outputs still hold the sentinel.
    Before the rules were asked first, the start had been copied into the outputs by then wherever the entry steps in place from
    the first launch on: k2b_fit_world_lbfgs, and k2b_fit_sequence_lbfgs where it fits frame by frame (``sl_tree_dup``: SMPL-X)."""
    case = next(c for c in T.CASES if c["id"] == case_id)
    call, model = T.call_of(case), T.MODELS[case["model"]]
    assert len(call["idx"]) == 2 and call["idx"][0] == call["idx"][1] < len(model["parents"])
    widths = dict(go_out=3, bp_out=3 * (len(model["parents"]) - 1), be_out=model["NB"], tr_out=3)
    sentinel = -12345.0
    outputs = {k: torch.full((2, w), sentinel, dtype=torch.float32, device=handles.device) for k, w in widths.items()}
    code, message = T.run_case(handles, case, outputs=outputs)
    torch.cuda.synchronize()
    assert code == handles.native.K2B_ERR_UNSUPPORTED and message == GOLDEN[case_id]["message"]
    assert message == f"k2b_fit_world: joint {call['idx'][0]} is targeted twice"
    for k, t in outputs.items():
        assert bool((t == sentinel).all()), k
