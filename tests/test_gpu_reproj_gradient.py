"""Loss and analytic gradient of the projected joint term (``k2b_fit_config.projection = 1``) of both fit kernels against float64
autograd through the CPU oracle: one evaluate-only closure per call.  Oracle, cases and gate: tests/reproj_common.py (the gate
numbers are those of tests/fit_gradient_common.py); the conditions on the inputs: tests/test_reproj_conditions.py (no GPU).
Every case runs in every forced launch shape of its kernel - the shapes agree bit for bit - at 1, 2, 3 and all of its frames
(the paired shapes carry two frames per wave: an odd count leaves half a wave without a frame)."""
import numpy as np
import pytest

from tests import fit_gradient_common as G
from tests import reproj_common as R

pytestmark = pytest.mark.gpu

FRAMES = (1, 2, 3, 17)


def _in_every_shape(case, ref=None, call=None):
    """`case` (or `call`, the same call written differently, against `case`'s oracle) in every shape at every frame count."""
    call = call or case
    shapes = R.shapes_of(case.kind)
    for n in sorted({n for n in FRAMES if n < case.frames} | {case.frames}):
        first = R.device_eval(call, shapes[0], n)
        for s in shapes[1:]:
            loss, grad = R.device_eval(call, s, n)
            diff = np.argwhere(grad != first[1])
            assert np.array_equal(loss, first[0]) and not len(diff), (
                f"{call.name}: {n} frames, shape {s} differs from shape {shapes[0]}: loss by {np.abs(loss - first[0]).max():.3e}, "
                f"{len(diff)} gradient entries by up to {np.abs(grad - first[1]).max():.3e}, the first at (frame, column) {diff[:6].tolist()}")
        R.gate(case, *first, ref=ref, what=f" [{call.name}]" if call is not case else "")


@pytest.mark.parametrize("term", ("joint", "all"))
@pytest.mark.parametrize("kind", R.KINDS_FUSED + R.KINDS_TREE)
def test_term_alone_and_all_terms(kind, term):
    """smpl10 / smpl16: both instantiations of the fused kernel in its four shapes; SMPL-H, SMPL-X with 20 and 32 shape
    coefficients: the three of the tree kernel in its two."""
    _in_every_shape(R.term_case(kind, term))


@pytest.mark.parametrize("term", ("joint", "all"))
@pytest.mark.parametrize("kind", R.BOTH)
def test_unequal_focal_lengths(kind, term):
    _in_every_shape(R.term_case(kind, term, R.FOCAL_UNEQUAL))


@pytest.mark.parametrize("per_frame", (False, True))
@pytest.mark.parametrize("kind", R.BOTH)
def test_confidences_with_zeros(kind, per_frame):
    """Shared and per-frame confidences; a target of confidence zero lies 100 px off and contributes nothing."""
    _in_every_shape(R.conf_case(kind, per_frame))


@pytest.mark.parametrize("mask,freeze", [(15, 0), (9, 0), (2, 0), (4, 0), (15, 1)])
@pytest.mark.parametrize("kind", R.BOTH)
def test_optimiser_membership(kind, mask, freeze):
    """``optimize_mask`` and ``freeze_betas``: a group outside the optimiser has a gradient of exactly zero (the gate asserts it)."""
    _in_every_shape(R.member_case(kind, mask, freeze))


@pytest.mark.parametrize("term", ("joint", "all"))
@pytest.mark.parametrize("kind", R.BOTH)
def test_robustifier_from_below_to_far_above_sigma(kind, term):
    """Sigma 20 px, residuals of 2 .. 400 px with both signs, one target on its projection."""
    _in_every_shape(R.gmof_case(kind, term))


@pytest.mark.parametrize("kind", R.BOTH)
def test_a_frame_behind_the_camera_is_finite(kind):
    case = R.behind_case(kind)
    _in_every_shape(case)
    loss, grad = R.device_eval(case)
    assert np.isfinite(loss[1]) and np.isfinite(grad[1]).all() and np.abs(grad[1]).max() > 0


@pytest.mark.parametrize("targeted", (False, True), ids=("untargeted", "confidence0"))
@pytest.mark.parametrize("kind", R.BOTH)
def test_a_lane_without_a_share_at_depth_zero_contributes_nothing(kind, targeted):
    """The root on the camera's plane, Z = 0 exactly (``transl_z`` = minus the device's float32 rest root z, betas 0), where
    fx X / Z is infinite: untargeted, and targeted with confidence 0.  Loss and gradient are finite and equal the oracle's,
    which leaves the root out (a weight of zero times an infinite factor would be NaN there as well)."""
    root_z = R.native_root_z(kind)
    case = R.z0_case(kind, targeted, root_z)
    oracle_case = R.without_root(case) if targeted else case
    _in_every_shape(oracle_case, call=case)
    if targeted:                      # the root's row of targets is not read at all: any value, a non-finite one included
        other = R.replace(case, name=case.name + "/nan", j3d=np.concatenate([np.full_like(case.j3d[:, :1], np.nan), case.j3d[:, 1:]], axis=1))
        a, b = R.device_eval(case), R.device_eval(other)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
