"""GPU: ``k2b_lbs_backward`` and the stand-alone surface loss terms (``k2b_vertex_term``, ``k2b_surface_term``) on the odd layouts of
``tests/lbs_layouts_common.py``, against float64 autograd through the CPU oracle.

The backward lays its features out as ``16 ceil(9 (J - 1) / 16) + (NB <= 16 ? 16 : 32)``: 17 and 49 joints have no pad column,
56 no padded joint in the last group of eight, 24 / 16 and 24 / 17 sit on either side of the row switch; ``k2b_vertex_term``
switches from its ``<24, 16>`` to its ``<64, 32>`` instantiation at the same boundary.  Body of the backward test and its gate:
``tests/test_gpu_lbs_backward.py``, ``lbs_backward_common.gate``; the terms' gate: ``tests/fit_gradient_common.py``.  V = 333, B = 3;
every case holds an all-zero pose and a frame of 2 rad rotations."""
import numpy as np
import pytest
import torch

from keypoints2body_amd import native
from tests import helpers as H
from tests import lbs_backward_common as C
from tests import lbs_layouts_common as L

pytestmark = pytest.mark.gpu

V, B = L.V_SMALL, 3
BACKWARD_CASES = ([(J, NB, "both") for J, NB in L.BACKWARD_LAYOUTS]
                  + [(J, NB, which) for J, NB in L.BACKWARD_ALL_COTANGENTS for which in ("joints", "no_transl")])


def _cotangents(J, which, seed=11):
    rng = np.random.default_rng(seed)
    gj = rng.standard_normal((B, J + L.NUM_EXTRA, 3)).astype(np.float32)
    gv = rng.standard_normal((B, V, 3)).astype(np.float32)
    return (gj, None) if which == "joints" else (gj, gv)


@pytest.mark.parametrize("J, NB, which", BACKWARD_CASES)
def test_backward_matches_float64_autograd(J, NB, which):
    m = L.native_model(J, NB)
    p = L.backward_params(J, NB, B)
    gj, gv = _cotangents(J, which)
    with_transl = which != "no_transl"
    go, pose, shape, tr = map(H.cuda, p)
    out = m.lbs_backward(go, pose, shape, tr if with_transl else None, H.cuda(gj), None if gv is None else H.cuda(gv))
    torch.cuda.synchronize()
    got = dict(zip(C.GROUPS, out))
    assert [tuple(g.shape) for g in out] == [(B, 3), (B, 3 * (J - 1)), (B, NB), (B, 3)]
    g64 = L.oracle_grads(J, NB, V, "tagged", p, gj, gv, True, with_transl)
    g32 = L.oracle_grads(J, NB, V, "tagged", p, gj, gv, False, with_transl)
    C.gate(f"{J}/{NB} V={V} B={B} {which}", got, g64, g32)


def test_backward_with_rotations_of_several_turns():
    """The frames of the forward's "turns" regime (6.5 .. 5000 rad on the root, on joint 3, 999 / 1001 rad on a chain) through
    ``k2b_lbs_backward``, per frame under ``lbs_layouts_common.turn_backward_gate``."""
    J, NB = L.TURN_BACKWARD_LAYOUT
    p, (gj, gv), _, _, _ = L.turn_backward_reference(J, NB)
    out = L.native_model(J, NB).lbs_backward(*map(H.cuda, p), H.cuda(gj), H.cuda(gv))
    torch.cuda.synchronize()
    L.turn_backward_gate(J, NB, dict(zip(C.GROUPS, out)))


@pytest.mark.parametrize("J, NB", L.VERTEX_TERM_LAYOUTS)
def test_vertex_term_matches_float64_autograd(J, NB):
    """20 / 16: the ``<24, 16>`` instantiation with fewer joints than its capacity; 24 / 17 and 56 / 32: ``<64, 32>``."""
    case = L.vertex_term_case(J, NB, B)
    loss, grad = native.vertex_term(L.native_model(J, NB), list(case.index), H.cuda(case.targets), H.cuda(case.conf), L.TERM_SIGMA, L.TERM_WEIGHT,
                                    *map(H.cuda, case.params))
    torch.cuda.synchronize()
    L.term_gate(case, loss, grad)


def test_surface_term_on_the_landmark_model_matches_float64_autograd():
    """56 joints / 16 coefficients with 51 landmarks: three extra joints and every third landmark, per-frame confidences."""
    case = L.surface_term_case(B)
    m = L.native_model(case.J, case.NB, variant="landmarks")
    assert case.conf.shape == (B, len(case.rows)) and len(case.rows) == 3 + 17
    loss, grad = native.surface_term(m, list(case.index), H.cuda(case.targets), H.cuda(case.conf), L.TERM_SIGMA, L.TERM_WEIGHT, *map(H.cuda, case.params))
    torch.cuda.synchronize()
    L.term_gate(case, loss, grad)
