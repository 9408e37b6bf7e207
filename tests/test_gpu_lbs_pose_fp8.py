"""GPU: the SMPL stream kernel with the pose phase's correction products on the block-scaled e4m3 MFMA (description ``SmplF8`` of
``csrc/k2b_lbs_stream.hip``, the default of the 24-joint model; ``csrc/k2b_lbs_fp8.h``) against the float64 oracle and against its
three-f16-product twin - the same constants created under ``K2B_LBS_POSE_F16=1`` (read once, by ``k2b_model_create``).

Frames: 1, 15, 137 and 271 give partial frame groups and, with the 6890-vertex mesh, the partial vertex tile of the last vertex
group; 16 is a full 16-frame unit; 137 and 271 span two and three frame groups, so a persistent workgroup walks more than one
tile and hands the Pd buffers over.  Poses as ``_large_poses`` of ``tests/test_gpu_fullsize_oracle.py`` (root uniform in +-3 rad,
body 0.6 N(0, 1), shape uniform in +-2.5, translation uniform in +-5 m) with one all-zero frame and one frame at about 20 rad.

Gate: the project's forward gate ``5e-6 * max(1, scale)``, scale = the largest vertex coordinate of the
oracle.  Both models are held to it, and their difference to the gate minus the twin's own measured error, so that the sum stays
inside the gate by construction."""
import os

import numpy as np
import pytest
import torch

from keypoints2body_amd import native
from tests import helpers as H

pytestmark = pytest.mark.gpu

GATE = 5e-6
SWITCH = "K2B_LBS_POSE_F16"
FRAMES = (1, 15, 16, 137, 271)
_cache = {}


def _memo(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _native():
    c = H.body_consts()
    return native.NativeModel(c.v_template, c.shapedirs, c.posedirs, c.J_regressor, c.lbs_weights, c.parents, c.extra_vertex_ids)


def _default():
    assert SWITCH not in os.environ
    return _memo("default", _native)


def _twin(monkeypatch):
    def make():
        with monkeypatch.context() as mp:
            mp.setenv(SWITCH, "1")
            return _native()
    return _memo("twin", make)


def _params(B, with_transl):
    rng = np.random.default_rng(900 + B)
    go = rng.uniform(-3.0, 3.0, (B, 3)).astype(np.float32)
    pose = (0.6 * rng.standard_normal((B, 69))).astype(np.float32)
    shape = rng.uniform(-2.5, 2.5, (B, 10)).astype(np.float32)
    tr = rng.uniform(-5.0, 5.0, (B, 3)).astype(np.float32)
    pose[B // 3] = 0.0                                                 # identity rotations in one frame
    go[B // 3] = 0.0
    far = (2 * B) // 3                                                 # one frame at about 20 rad (with B = 1 it replaces the zero frame)
    sign = np.where(rng.random(69) < 0.5, -1.0, 1.0)
    pose[far] = (sign * 20.0 / np.sqrt(3.0)).astype(np.float32)
    go[far] = np.float32(20.0 / np.sqrt(3.0))
    return go, pose, shape, (tr if with_transl else None)


def _oracle(B, with_transl):
    def make():
        go, pose, shape, tr = _params(B, with_transl)
        t = lambda a: torch.tensor(a, dtype=torch.float64)
        with torch.no_grad():
            o = H.oracle_model(double=True)(global_orient=t(go), body_pose=t(pose), betas=t(shape), transl=None if tr is None else t(tr))
        return o.vertices, o.joints
    return _memo(("oracle", B, with_transl), make)


def _lbs(model, B, with_transl, want_vertices=True):
    go, pose, shape, tr = _params(B, with_transl)
    return model.lbs(H.cuda(go), H.cuda(pose), H.cuda(shape), None if tr is None else H.cuda(tr), want_vertices=want_vertices)


def _err(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max())


@pytest.mark.parametrize("with_transl", [True, False])
@pytest.mark.parametrize("B", FRAMES)
def test_fp8_pose_corrections_against_oracle_and_twin(B, with_transl, monkeypatch):
    ref_v, ref_j = _oracle(B, with_transl)
    gate = GATE * max(1.0, float(ref_v.abs().max()))
    twin = _twin(monkeypatch)
    model = _default()
    j, v = _lbs(model, B, with_transl)
    jt, vt = _lbs(twin, B, with_transl)
    assert tuple(v.shape) == (B, ref_v.shape[1], 3) and tuple(j.shape) == tuple(ref_j.shape)
    e8, e16 = max(_err(v, ref_v), _err(j, ref_j)), max(_err(vt, ref_v), _err(jt, ref_j))
    diff = max(_err(v, vt), _err(j, jt))
    print(f"B {B} transl {with_transl}: gate {gate:.3e}  e4m3 form {e8:.3e}  f16 twin {e16:.3e}  difference {diff:.3e}")
    assert torch.isfinite(v).all() and torch.isfinite(j).all()
    assert e16 <= gate, ("f16 twin", B, e16, gate)
    assert e8 <= gate, ("e4m3 form", B, e8, gate)
    assert diff <= gate - e16, ("difference", B, diff, gate - e16)
    if B > 1:
        assert diff > 0.0                                              # the two forms are two kernels: the switch did something
    # the joints-only call (the 21-vertex operand set, with the mesh's scales) equals the full call's joints bit for bit
    for m, full in ((model, j), (twin, jt)):
        j2, none = _lbs(m, B, with_transl, want_vertices=False)
        assert none is None and torch.equal(full, j2)
