"""The conditions on the inputs of the projected joint term's gradient tests (tests/reproj_common.py), from the CPU oracle alone:
for every case the float32 oracle stays within E32_LIMIT of the float64 one in every group and in the loss, and one float32
rounding of the pixel targets moves no group of the float64 gradient by more than ROUNDING_LIMIT.  The cases use centred
targets, fx = fy = 500 px (one pair of cases 500 / 430), bodies about 3 m from the camera and residuals of about 15 px;
this test proves the conditions for each of them.  No GPU."""
import numpy as np
import pytest

from tests import fit_gradient_common as G
from tests import reproj_common as R

CASES = R.all_cases()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_case_meets_the_input_conditions(case):
    ref = R.reference(case)                                  # asserts both conditions
    print(f"{case.name}: e32 " + " ".join(f"{k}={v:.1e}" for k, v in ref.e32.items()) + f" loss={ref.e32_loss:.1e}; rounding " +
          " ".join(f"{k}={v:.1e}" for k, v in ref.rounding.items()))
    assert max(ref.e32.values()) <= G.E32_LIMIT and max(ref.rounding.values()) <= G.ROUNDING_LIMIT
    excluded = G.excluded_columns(case)
    assert not ref.g64[:, excluded].any()
    live = [k for k, a, b in G.layout(case.kind).groups if not excluded[a:b].all() and np.abs(ref.g64[:, a:b]).max() > 0]
    assert live, case.name


def test_case_names_are_unique():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)


def test_the_third_target_column_is_not_part_of_the_oracle():
    case = R.term_case("smpl10", "joint")
    other = R.replace(case, j3d=case.j3d * np.asarray([1.0, 1.0, -7.0], dtype=np.float32))
    a, b = R.oracle_eval(case, True), R.oracle_eval(other, True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_behind_the_camera_and_the_plane_cases_are_what_they_say():
    for kind in R.BOTH:
        c = R.behind_case(kind)
        z = G.joints64(kind, c.go, c.pose, c.shape, c.tr)[:, :, 2]
        assert (z[1] < 0).all() and (z[[0, 2]] > 0).all()
        root_z = R.rest_root_z(kind)
        for targeted in (False, True):
            c = R.z0_case(kind, targeted, root_z)
            p = G.joints64(kind, c.go, c.pose, c.shape, c.tr)
            assert abs(p[1, 0, 2]) < 1e-6                                   # the root on the plane (exactly so on the device: native_root_z)
            kin = [j for j in c.idx if j != 0]
            assert (np.abs(p[:, kin, 2]) >= R.Z0_MIN_DEPTH).all()
            assert (p[1, kin, 2] > 0).any() and (p[1, kin, 2] < 0).any()    # targets before and behind the camera
            assert (0 in c.idx) == targeted
