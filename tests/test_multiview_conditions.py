"""No GPU: the conditions on the inputs of the multi-view term's GPU tests, from the oracle alone.  Every case that
tests/test_gpu_multiview_term.py and tests/test_gpu_multiview_fit.py gate meets ``E32_LIMIT`` (float32 autograd against float64)
and ``ROUNDING_LIMIT`` (one float32 rounding of the targets), so the gates there are the unwidened ones.  A case that leaves a
limit is changed, never the limit."""
import numpy as np
import pytest

from tests import fit_gradient_common as G
from tests import multiview_common as MV

CASES = MV.all_cases()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_the_case_meets_both_limits(case):
    ref = MV.reference(case)                # asserts the limits
    worst32, worst_round = max(list(ref.e32.values()) + [ref.e32_loss]), max(ref.rounding.values())
    print(f"{case.name}: float32 autograd off by {worst32:.2e} (limit {G.E32_LIMIT:.0e}), one target rounding moves the gradient by "
          f"{worst_round:.2e} (limit {G.ROUNDING_LIMIT:.1e}), largest pixel coordinate {np.abs(case.j3d[..., :2]).max():.0f}")
    assert worst32 <= G.E32_LIMIT and worst_round <= G.ROUNDING_LIMIT


def test_the_case_names_are_unique_and_the_rig_is_a_rig():
    assert len({c.name for c in CASES}) == len(CASES)
    for C in MV.VIEWS:
        for Rc, tc, fc in MV.rig(C):
            assert np.abs(Rc @ Rc.T - np.eye(3)).max() < 1e-6 and abs(np.linalg.det(Rc) - 1.0) < 1e-6 and (fc > 0).all()
