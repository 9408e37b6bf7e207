"""Loss and analytic gradient of the fit kernels (``k2b_fit.hip``: 24 joints; ``k2b_fit_tree.hip``: SMPL-H, SMPL-X, other trees),
term by term, against float64 autograd through the CPU oracle.  Every device call is one evaluate-only closure (one iteration,
step size 0, ``want_grad``) through ``native.fit_world``; oracle, cases and the gate - per parameter group and frame, tied to the
oracle's own float32 error - are in tests/fit_gradient_common.py, the conditions on the inputs in
tests/test_fit_gradient_conditions.py (no GPU)."""
import numpy as np
import pytest
import torch

from tests import fit_gradient_common as F

pytestmark = pytest.mark.gpu

FUSED_SHAPES, FUSED_FRAMES = (1, 2, 3, 4), (1, 2, 3, 17)       # debug_launch_shape: split, split-paired, paired, wide
TREE_SHAPES, TREE_FRAMES = (1, 2), (1, 3, 17)                  # plain, component waves


def _in_every_shape(case):
    """The case in every launch shape of its kernel at every frame count: the shapes agree bit for bit, one of them is gated."""
    fused = F.layout(case.kind).kernel == "fused"
    shapes, counts = (FUSED_SHAPES, FUSED_FRAMES) if fused else (TREE_SHAPES, TREE_FRAMES)
    for n in sorted({n for n in counts if n < case.frames} | {case.frames}):      # (every frame of the case reaches the kernel)
        first = F.device_eval(case, shapes[0], n)
        for s in shapes[1:]:
            loss, grad = F.device_eval(case, s, n)
            diff = np.argwhere(grad != first[1])
            assert np.array_equal(loss, first[0]) and not len(diff), (
                f"{case.name}: {n} frames, shape {s} differs from shape {shapes[0]}: loss by {np.abs(loss - first[0]).max():.3e}, {len(diff)} gradient "
                f"entries by up to {np.abs(grad - first[1]).max():.3e}, the first at (frame, column) {diff[:6].tolist()}")
        F.gate(case, *first)


# ---- 1. each term alone, and all together ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("term", F.TERMS + ("all",))
def test_fused_kernel_each_term_alone(term):
    _in_every_shape(F.term_case("smpl10", term))


@pytest.mark.parametrize("term", ("shape", "joint"))
@pytest.mark.parametrize("num_betas", [nb for nb in F.FUSED_BETAS if nb != 10])
def test_fused_kernel_beta_counts(num_betas, term):
    """1, 11 and 16 betas (10: above): both instantiations of the kernel, each with live and with padding betas."""
    _in_every_shape(F.term_case(f"smpl{num_betas}", term))


@pytest.mark.parametrize("term", F.TERMS[:-1] + ("all",))
@pytest.mark.parametrize("kind", F.TREE_KINDS)
def test_tree_kernel_each_term_alone(kind, term):
    _in_every_shape(F.term_case(kind, term))


def test_tree_kernel_fingers_without_targets_stay_zero():
    """22 body targets on SMPL-X: the hands' and the face's groups are identically zero in float64."""
    case = F.term_case("smplx20", "all", num_targets=22)
    ref = F.reference(case)
    lay = F.layout("smplx20")
    for name, a, b in lay.groups:
        if name in ("face", "hands"):
            assert not ref.g64[:, a:b].any()
    _in_every_shape(case)


@pytest.mark.parametrize("kind", F.TREE_KINDS)
def test_tree_kernel_refuses_the_translation_prior(kind):
    case = F.term_case(kind, "transl")
    assert case.tr_target is None and case.weights["transl"] > 0.0
    with pytest.raises(NotImplementedError, match="translation prior"):
        F.device_eval(case, 0, 1)
    with pytest.raises(NotImplementedError, match="translation prior"):     # a centre alone, weight zero
        F.device_eval(F.replace(case, weights=F.only("joint"), tr_target=case.tr + np.float32(0.1)), 0, 1)
    F.device_eval(F.replace(case, weights=F.only("joint")), 0, 1)


# ---- 2. rotation-angle ladder ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", F.BOTH + ("smplh",))
def test_rotation_angle_ladder(kind):
    """0, 1e-6, 1e-3, 1, 2, 3, 3.1415 and 3.3 rad on the joints of one frame, root included, beside an all-zero frame."""
    _in_every_shape(F.ladder_case(kind))


@pytest.mark.parametrize("kind", F.BOTH)
def test_root_rotations_of_several_turns(kind):
    """6.5 .. 5000 rad on the root (999 / 1001 straddle the branch of ``sincos_small`` to the library functions), one frame per
    angle, in every launch shape.  Up to 20 rad the frames are held to the unchanged group gate; above it the gate is dominated
    by what an ulp or two of the float32 angle do to the float64 gradient (``fit_gradient_common.turn_gate``), and the test
    catches a wrong quadrant, a broken reduction or a broken library branch, not an ulp."""
    case = F.turn_case(kind)
    shapes = FUSED_SHAPES if F.layout(kind).kernel == "fused" else TREE_SHAPES
    first = F.device_eval(case, shapes[0])
    for s in shapes[1:]:
        loss, grad = F.device_eval(case, s)
        assert np.array_equal(loss, first[0]) and np.array_equal(grad, first[1]), f"{case.name}: shape {s} differs from shape {shapes[0]}"
    F.turn_gate(kind, *first)


# ---- 3. GMoF outside its quadratic range -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("term", ("joint", "all"))
@pytest.mark.parametrize("kind", F.BOTH)
def test_gmof_below_at_and_far_above_sigma(kind, term):
    _in_every_shape(F.gmof_case(kind, term))


# ---- 4. confidences --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_frame", (False, True))
@pytest.mark.parametrize("kind", F.BOTH)
def test_confidences_zero_above_one_and_per_frame(kind, per_frame):
    """Zeros, values above 1, shared and as a per-frame table with differing rows; the targets of confidence zero lie a metre off
    and contribute nothing: the same call without them meets the same oracle."""
    case = F.conf_case(kind, per_frame)
    _in_every_shape(case)
    removed = F.conf_case(kind, per_frame, removed=True)
    F.gate(removed, *F.device_eval(removed), ref=F.reference(case), what=" against the oracle with the targets in")


# ---- 5. optimiser membership -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask,freeze", [(15, 0), (9, 0), (2, 0), (4, 0), (15, 1)])
@pytest.mark.parametrize("kind", F.BOTH)
def test_groups_outside_the_optimiser_are_exactly_zero(kind, mask, freeze):
    """optimize_mask 15, 9, 2, 4 and freeze_betas (SMPL-X: the first 10 coefficients, the expression stays in)."""
    case = F.member_case(kind, mask, freeze)
    excluded = F.excluded_columns(case)
    assert excluded.any() == (mask != 15 or bool(freeze))
    if kind == "smplx20" and freeze:
        lay = F.layout(kind)
        assert excluded.sum() == 10 and not excluded[3 + lay.D + 10:].any()
    _in_every_shape(case)


# ---- 6. mixture selection --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("term", ("mixture", "all"))
@pytest.mark.parametrize("kind", F.BOTH + ("smplh",))
def test_every_mixture_component_is_selected(kind, term):
    case = F.mixture_case(kind, term)
    chosen, gap = F.mixture_selection(case)
    assert len(set(chosen.tolist())) == len(chosen) and (gap > 1e-3).all()
    _in_every_shape(case)


# ---- 7. odd trees on the tree kernel ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("tree21", "tree26"))
def test_odd_trees(kind):
    """A small tree with junctions everywhere and a tree whose deepest targeted joints sit at the entry's depth limit."""
    assert F.layout(kind).kernel == "tree"
    _in_every_shape(F.term_case(kind, "all"))


def test_tree_past_the_depth_limit_is_refused():
    """The 26-joint tree above with one more joint, at depth 16; without that joint among the targets the entry takes it."""
    case = F.term_case("tree27", "all")
    with pytest.raises(NotImplementedError, match="depth 15"):
        F.device_eval(case, 0, 1)
    F.device_eval(F.replace(case, idx=case.idx[:-1], j3d=np.ascontiguousarray(case.j3d[:, :-1])), 0, 1)


def test_tree_past_the_joint_limit_is_refused():
    case = F.term_case("tree64", "all")
    assert F.layout("tree64").J == F.TREE_JOINT_LIMIT + 1
    with pytest.raises(NotImplementedError, match="up to 63 joints"):
        F.device_eval(case, 0, 1)


@pytest.mark.parametrize("dims", (F.TREE_PRIOR_LIMIT + 3, F.TREE_PRIOR_LIMIT - 1, 72))
def test_tree_kernel_refuses_prior_dimensions_it_does_not_take(dims):
    """More than 63 pose dimensions under the prior, a count that is no multiple of 3, more than the mixture's 69."""
    case = F.term_case("smplx20", "all")
    with pytest.raises(NotImplementedError, match="prior over the first 3..63 body-pose dimensions"):
        F.device_eval(case, 0, 1, prior_pose_dims=dims)
