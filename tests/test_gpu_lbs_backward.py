"""GPU: ``k2b_lbs_backward`` (``NativeModel.lbs_backward``), the vector-Jacobian product of ``k2b_lbs``, against the CPU oracle
in float64 with ``torch.autograd.grad`` (gate and models: ``tests/lbs_backward_common.py``).

Sizes: V = 1100 (the size of ``tests/test_gpu_smplx_wide.py``: seventeen full chunks of CHUNK vertices and a partial one, five
slab groups), 240, CHUNK - 1 and CHUNK + 1 (one chunk short of full, one vertex into a second chunk), and per model one case at
product size (6890 / 10 475 vertices, B = 2: the forward through the stream kernels, the backward through its full slab count).
Batches 1, 3, 17, 130: a partial 16-frame tile, one full tile and one more frame, nine tiles.  From three frames on every case
holds an all-zero pose and a frame with a 2 rad rotation on every joint."""
import numpy as np
import pytest
import torch

from keypoints2body_amd import native, synthetic
from tests import helpers as H
from tests import lbs_backward_common as C

pytestmark = pytest.mark.gpu

CHUNK = C.kernel_chunk()             # vertices per chunk of the dense kernel (kBwdChunk)
COTANGENTS = ("both", "vertices", "joints", "kinematic_row", "surface_row", "no_transl")

CASES = (
    [("smpl", 1100, 17, c) for c in COTANGENTS] + [("smplx20", 1100, 3, c) for c in COTANGENTS]
    + [(k, v, 3, "both") for k in ("smpl", "smplx20") for v in (240, CHUNK - 1, CHUNK + 1)]
    + [("smplh", 1100, 17, "both"), ("smplx26", 1100, 17, "both"), ("smplh", 240, 3, "joints"), ("smplx26", 240, 3, "joints")]
    + [(k, 1100, b, "both") for k in ("smpl", "smplx20") for b in (1, 130)]
    + [("smpl", 6890, 2, "both"), ("smplh", 6890, 2, "both"), ("smplx20", 10475, 2, "both"), ("smplx26", 10475, 2, "both")]
)


def test_chunk_is_what_the_sizes_assume():
    assert CHUNK + 1 <= 1100 and CHUNK - 1 >= 1


def _cotangents(kind, V, B, which, seed=11):
    """(grad_joints, grad_vertices) as float32 arrays or None: seeded normal values."""
    m = C.native_model(kind, V)
    rng = np.random.default_rng(seed)
    gj = rng.standard_normal((B, m.num_output_joints, 3)).astype(np.float32)
    gv = rng.standard_normal((B, V, 3)).astype(np.float32)
    if which == "vertices":
        return None, gv
    if which == "joints":
        return gj, None
    if which in ("kinematic_row", "surface_row"):
        # one kinematic row alone / one landmark row alone (a model without landmarks: one extra-vertex row)
        row = 5 if which == "kinematic_row" else (m.num_joints + m.num_extra + 3 if m.num_landmarks else m.num_joints + 2)
        one = np.zeros_like(gj)
        one[:, row] = gj[:, row]
        return one, None
    return gj, gv


def _device_grads(kind, V, params, gj, gv, with_transl=True, want=(True, True, True, True)):
    m = C.native_model(kind, V)
    go, pose, shape, tr = map(H.cuda, params)
    out = m.lbs_backward(go, pose, shape, tr if with_transl else None, None if gj is None else H.cuda(gj),
                         None if gv is None else H.cuda(gv), want=want)
    torch.cuda.synchronize()
    return dict(zip(C.GROUPS, out))


@pytest.mark.parametrize("kind, V, B, which", CASES)
def test_backward_matches_float64_autograd(kind, V, B, which):
    params = C.packed(kind, B, seed=5)
    gj, gv = _cotangents(kind, V, B, which)
    with_transl = which != "no_transl"
    got = _device_grads(kind, V, params, gj, gv, with_transl)
    g64 = C.oracle_grads(kind, V, params, gj, gv, True, with_transl)
    g32 = C.oracle_grads(kind, V, params, gj, gv, False, with_transl)
    C.gate(f"{kind} V={V} B={B} {which}", got, g64, g32)


@pytest.mark.parametrize("kind, which", [("smpl", "both"), ("smplx20", "both"), ("smplx20", "joints")])
def test_a_frame_has_the_same_bits_alone_and_in_a_batch_and_from_run_to_run(kind, which):
    V, B = 1100, 130
    params = C.packed(kind, B, seed=7)
    gj, gv = _cotangents(kind, V, B, which)
    full = _device_grads(kind, V, params, gj, gv)
    again = _device_grads(kind, V, params, gj, gv)
    for k in C.GROUPS:
        assert torch.equal(full[k], again[k]), k
    for f in (0, 2, 15, 16, 77, 129):
        row = lambda a: None if a is None else a[f:f + 1]
        alone = _device_grads(kind, V, tuple(p[f:f + 1] for p in params), row(gj), row(gv))
        for k in C.GROUPS:
            assert torch.equal(alone[k][0], full[k][f]), (k, f)


def test_an_output_left_out_changes_no_other_output():
    kind, V, B = "smplx20", 240, 3
    params = C.packed(kind, B, seed=9)
    gj, gv = _cotangents(kind, V, B, "both")
    full = _device_grads(kind, V, params, gj, gv)
    for want in ((True, False, True, False), (False, True, False, True), (False, False, False, True)):
        part = _device_grads(kind, V, params, gj, gv, want=want)
        for k, w in zip(C.GROUPS, want):
            assert (part[k] is not None) == w
            if w:
                assert torch.equal(part[k], full[k]), (want, k)


def test_argument_behaviour():
    kind, V = "smpl", 240
    m = C.native_model(kind, V)
    go, pose, shape, tr = map(H.cuda, C.packed(kind, 2, seed=1))
    with pytest.raises(ValueError):                       # no cotangent at all
        m.lbs_backward(go, pose, shape, tr, None, None)
    empty = m.lbs_backward(go[:0], pose[:0], shape[:0], tr[:0], torch.zeros((0, m.num_output_joints, 3), device="cuda"), None)
    assert [tuple(g.shape) for g in empty] == [(0, 3), (0, 69), (0, 10), (0, 3)]
    # a 30-joint chain: neither k2b_lbs nor its backward is built for it
    rest = 0.1 * synthetic.normalish(70, (30, 3), 0)
    c = synthetic.make_body_model(0, num_vertices=240, parents=np.arange(-1, 29), rest=rest, num_extra=0)
    m30 = native.NativeModel(c.v_template, c.shapedirs, c.posedirs, c.J_regressor, c.lbs_weights, c.parents, c.extra_vertex_ids)
    z = lambda *s: torch.zeros(s, device="cuda")
    with pytest.raises(NotImplementedError):
        m30.lbs_backward(z(1, 3), z(1, 87), z(1, 10), None, z(1, 30, 3), None)
