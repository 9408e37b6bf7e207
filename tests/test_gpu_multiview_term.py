"""The multi-view joint term of ``k2b_fit_multiview`` against its float64 oracle (tests/multiview_common.py): one evaluate-only
closure per case, loss and gradient through ``fit_gradient_common.gate`` - gradient per group and frame ``max(2e-5, 4 e32_k)``, loss
``max(2e-6, 4 e32_loss)`` -, with the fused 24-lane kernel (smpl10, smpl16) and the tree kernel (smplh, smplx20, smplx32), 1 to 8
views.  tests/test_multiview_conditions.py holds every case to the limits on the inputs without a GPU."""
import numpy as np
import pytest

from tests import multiview_common as MV

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("term", ("joint", "all"))
@pytest.mark.parametrize("kind,C", MV.term_cases())
def test_the_closure_matches_the_oracle(kind, C, term):
    case = MV.term_case(kind, C, term)
    MV.gate(case, *MV.device_eval(case))


@pytest.mark.parametrize("per_frame", (False, True))
@pytest.mark.parametrize("kind", MV.BOTH)
def test_confidences_weigh_the_pairs_and_a_zero_removes_one(kind, per_frame):
    case = MV.conf_case(kind, 3, per_frame)
    loss, grad = MV.device_eval(case)
    MV.gate(case, loss, grad)
    # the pairs of confidence zero sit 100 px off: back on their seeded places they change no bit
    clean = MV.base(kind, 3, B=3, seed=19).j3d
    assert not np.array_equal(clean, case.j3d)
    loss2, grad2 = MV.device_eval(case, j3d=clean)
    assert np.array_equal(loss, loss2) and np.array_equal(grad, grad2)


@pytest.mark.parametrize("kind", MV.BOTH)
def test_a_view_of_confidence_zero_is_no_view(kind):
    case = MV.blind_view_case(kind, 3)
    loss, grad = MV.device_eval(case)
    MV.gate(case, loss, grad)
    # the same bits as the call without that view: the sum over the views runs in their order, and what it skips is an exact zero
    two = MV.replace(case, cams=(case.cams[0], case.cams[2]), j3d=np.ascontiguousarray(case.j3d[:, [0, 2]]), conf=np.ascontiguousarray(case.conf[[0, 2]]))
    loss2, grad2 = MV.device_eval(two)
    assert np.array_equal(loss, loss2) and np.array_equal(grad, grad2)


@pytest.mark.parametrize("kind", MV.BOTH)
def test_a_body_behind_a_camera_is_legal(kind):
    case = MV.behind_case(kind, 3)
    MV.gate(case, *MV.device_eval(case))


@pytest.mark.parametrize("mask,freeze", ((15, 0), (9, 0), (2, 0), (4, 0), (15, 1)))
@pytest.mark.parametrize("kind", MV.BOTH)
def test_parameter_groups_outside_the_optimiser_have_no_gradient(kind, mask, freeze):
    case = MV.member_case(kind, 2, mask, freeze)
    MV.gate(case, *MV.device_eval(case))


@pytest.mark.parametrize("kind", MV.BOTH)
def test_a_nan_keypoint_stays_in_its_frame(kind):
    """One NaN coordinate in view 1 of frame 2 of five: that frame's loss is not finite, every other frame keeps its bits."""
    case = MV.base(kind, 3, B=5, seed=31)
    loss, grad = MV.device_eval(case)
    bad = case.j3d.copy()
    bad[2, 1, 4, 0] = np.nan
    loss2, grad2 = MV.device_eval(case, j3d=bad, finite=False)
    others = [0, 1, 3, 4]
    assert not np.isfinite(loss2[2]) and np.isfinite(loss).all()
    assert np.array_equal(loss[others], loss2[others]) and np.array_equal(grad[others], grad2[others])
