"""GPU: ``k2b_lbs`` on every joint / shape-coefficient layout of ``tests/lbs_layouts_common.py`` - each route of
``k2b_model_create`` (tile, stream, stream_x, stream_xw) in both joint families, every capacity of the pose set-up's shape loop
with a coefficient count below it, the last k-step exactly full and one feature over, 17 and 56 joints - against the float64
oracle under a per-frame gate (``lbs_layouts_common.forward_gate``), in three parameter regimes that each hold an all-zero frame,
the Rodrigues angle ladder and a frame of 2 rad rotations.

Models have 333 vertices (two full 128-vertex groups, a partial one with a partial 16-vertex tile and empty waves) and five
vertex-selected joints; a batch is 37 frames (a full 32-frame tile and five frames).  Two cases run the product meshes at B = 3."""
import os

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import lbs_layouts_common as L

pytestmark = pytest.mark.gpu

TILE_SWITCH = "K2B_LBS_TILE"


def _lbs(model, p, want_vertices=True, with_transl=True, rows=slice(None)):
    go, pose, shape, tr = (H.cuda(a[rows]) for a in p)
    out = model.lbs(go, pose, shape, tr if with_transl else None, want_vertices=want_vertices)
    torch.cuda.synchronize()
    return out


def _check_forward(model, J, NB, regime, V=L.V_SMALL, B=L.FRAMES, variant="tagged", what=""):
    """The full call, the joints-only call and the call without a translation, each under the gate; returns the full call's
    (joints, vertices)."""
    ref = L.reference(J, NB, regime, V, B, variant)
    L.check_inputs(ref, regime)
    j, v = _lbs(model, ref.params)
    assert tuple(j.shape) == tuple(ref.joints.shape) and tuple(v.shape) == (B, V, 3)
    L.forward_gate(ref, j, v, what)
    j2, none = _lbs(model, ref.params, want_vertices=False)
    assert none is None and tuple(j2.shape) == tuple(j.shape)
    n = J + len(L.consts(J, NB, V, variant).extra_vertex_ids)   # (landmark rows of a joints-only call: the gate, below)
    assert torch.equal(j2[:, :n], j[:, :n]), f"{ref.name}{what}: joints-only differs from the full call by {float((j2[:, :n] - j[:, :n]).abs().max()):.3e}"
    L.forward_gate(ref, j2, None, what + " joints only")
    bare = L.reference(J, NB, regime, V, B, variant, with_transl=False)
    L.check_inputs(bare, "benign" if regime == "benign" else "wide")
    jb, vb = _lbs(model, ref.params, with_transl=False)
    L.forward_gate(bare, jb, vb, what)
    return j, v


# ---- 1. every layout against the float64 oracle ---------------------------------------------------------------------------------
@pytest.mark.parametrize("J, NB, regime", L.forward_cases())
def test_forward_matches_the_float64_oracle(J, NB, regime):
    assert TILE_SWITCH not in os.environ
    _check_forward(L.native_model(J, NB), J, NB, regime)


@pytest.mark.parametrize("J, NB", L.TURN_LAYOUTS)
def test_forward_with_rotations_of_several_turns(J, NB):
    """Regime "turns": 6.5 .. 5000 rad on the root, on joint 3, and 999 / 1001 rad on two consecutive joints of a chain (the pair
    straddles the branch of ``sincos_small`` to the library functions).  The gate of every frame is the unchanged one plus d_f,
    what two ulp of the float32 angle do to the float64 result: up to 20 rad that is below the gate, so those frames are held as
    sharply as every other; above it d_f dominates, and the test catches a wrong quadrant, a broken reduction or a broken library
    branch there, not an ulp.  Prints the worst error per angle."""
    ref = L.reference(J, NB, "turns")
    L.check_inputs(ref, "turns")
    m = L.native_model(J, NB)
    j, v = _lbs(m, ref.params)
    print(f"turns {J}/{NB} worst error / gate per angle: {L.turn_summary(ref, j, v)}")
    L.forward_gate(ref, j, v)
    j2, _ = _lbs(m, ref.params, want_vertices=False)
    L.forward_gate(ref, j2, None, " joints only")


# ---- 2. the tile kernel as twin of the stream kernels ---------------------------------------------------------------------------
@pytest.mark.parametrize("J, NB", L.STREAM_LAYOUTS)
def test_tile_twin_of_every_stream_layout(J, NB, monkeypatch):
    """The same constants created under K2B_LBS_TILE=1 (``k2b_lbs_tile_kernel<3, 12>`` / ``<7, 6>`` at the layout's k-step count),
    held to the same gate; the difference between the routes is printed."""
    route = L.expected_route(J, NB)[2]
    assert route != "tile" and TILE_SWITCH not in os.environ
    twin = L.native_model(J, NB, env=(monkeypatch, TILE_SWITCH, "1"))
    assert TILE_SWITCH not in os.environ and twin is not L.native_model(J, NB)
    for regime in ("benign", "wide"):
        a = _check_forward(L.native_model(J, NB), J, NB, regime, what=f" {route}")
        b = _check_forward(twin, J, NB, regime, what=" tile twin")
        print(f"{J}/{NB} {regime}: {route} - tile twin: vertices {float((a[1] - b[1]).abs().max()):.3e} joints {float((a[0] - b[0]).abs().max()):.3e}")


# ---- 3. determinism, frames do not interact ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("J, NB", L.REPEAT_LAYOUTS)
def test_same_bits_from_run_to_run_and_alone_or_in_a_batch(J, NB):
    m = L.native_model(J, NB)
    p = L.params(J, NB, "wide")
    j, v = _lbs(m, p)
    j_again, v_again = _lbs(m, p)
    assert torch.equal(j, j_again) and torch.equal(v, v_again)
    j5, v5 = _lbs(m, p, rows=slice(0, 5))                  # the zero frame, the ladder and the 2 rad frame among them
    assert torch.equal(v[:5], v5) and torch.equal(j[:5], j5)


# ---- 4. the three routes of the vertex-selected joints ----------------------------------------------------------------------------
@pytest.mark.parametrize("J, NB", L.EXTRA_ROUTE_LAYOUTS)
def test_extra_joints_by_the_gather_launch(J, NB):
    """Two extra joints on one vertex: no tag in the W image, ``k2b_gather_joints_kernel`` copies the rows behind the mesh launch."""
    m = L.native_model(J, NB, variant="gather")
    j, v = _check_forward(m, J, NB, "wide", variant="gather")
    ids = torch.as_tensor(L.consts(J, NB, variant="gather").extra_vertex_ids.astype(np.int64)).cuda()
    assert torch.equal(j[:, J:], v[:, ids])                # the rows are the call's own vertices
    assert torch.equal(j[:, J], j[:, J + 2])


@pytest.mark.parametrize("J, NB", L.EXTRA_ROUTE_LAYOUTS)
def test_model_without_extra_joints(J, NB):
    m = L.native_model(J, NB, variant="none")
    assert m.num_extra == 0 and m.num_output_joints == J
    j, v = _check_forward(m, J, NB, "wide", variant="none")
    assert tuple(j.shape) == (L.FRAMES, J, 3)


def test_landmarks_on_the_wide_route_by_joint_count():
    """56 joints / 16 coefficients (``k2b_lbs_stream_xw_kernel``) with 51 landmarks on the joints 15 and 22: with the mesh, and
    from the 153 landmark vertices skinned alone, against landmark rows combined from the float64 vertices."""
    J, NB = L.LANDMARK_LAYOUT
    m = L.native_model(J, NB, variant="landmarks")
    assert m.num_landmarks == 51 and m.num_output_joints == J + L.NUM_EXTRA + 51
    for regime in ("benign", "wide"):
        j, v = _check_forward(m, J, NB, regime, variant="landmarks")
        plain = _lbs(L.native_model(J, NB), L.params(J, NB, regime))
        assert torch.equal(plain[1], v) and torch.equal(plain[0], j[:, :J + L.NUM_EXTRA])


# ---- 5. product meshes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("J, NB, V", L.PRODUCT_CASES)
def test_product_size_meshes(J, NB, V):
    _check_forward(L.native_model(J, NB, V), J, NB, "benign", V=V, B=3)
