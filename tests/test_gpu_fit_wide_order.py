"""The row waves of the 16-wave launch shape do in front of the iteration's second barrier what the trees do not feed (the Adam
coefficient's reciprocal, the lanes' sum of the prior losses on the last iteration) and request the three gradient reads behind
it back to back, reading the second slot's strip whether the workgroup has that frame or not; the tree pass evaluates the rare
branch of sin / cos (more than 1e3 rad) behind the fast path instead of in place of it.  None of that may change a bit: the wide
shape is held to the paired shape - the same two frames per wave, in eight waves, with its own row path - on parameters, loss and
gradient after 12 Adam iterations.

Cases: 16, 15 and 9 frames in one workgroup (at 15 and 9 the last row wave carries one frame: the packed set B's second half
and the second slot's reads are beyond the workgroup's frames), 33 frames (three workgroups, the last one with a single
frame), kernels for 10 and 16 shape coefficients, the projected joint term, a first frame without a preserve term and a
follow-up frame with one, and one joint of one frame turned by more than 1e3 rad among ordinary frames."""
import functools

import numpy as np
import pytest
import torch

from tests import helpers as H

pytestmark = pytest.mark.gpu

ITERS = 12
K = 22
KEYS = ("global_orient", "body_pose", "betas", "transl", "loss", "grad")
FOCAL = (1100.0, 1050.0)


@functools.lru_cache(maxsize=None)
def _consts(num_betas):
    from keypoints2body_amd import synthetic
    return synthetic.make_body_model(seed=3, num_vertices=512, num_betas=num_betas)


@functools.lru_cache(maxsize=None)
def _native(num_betas):
    from keypoints2body_amd.native import NativeModel
    c = _consts(num_betas)
    return NativeModel(c.v_template, c.shapedirs, c.posedirs, c.J_regressor, c.lbs_weights, c.parents, c.extra_vertex_ids)


@functools.lru_cache(maxsize=None)
def _problem(num_betas):
    """33 frames: 3D targets, their centred-pixel form, start parameters and a pose to preserve (CPU tensors, never changed)."""
    from keypoints2body_amd import synthetic
    from oracle.smpl_torch import TorchSMPL
    B = 33
    p = synthetic.make_poses(B, seed=11)
    t = lambda x: torch.as_tensor(np.asarray(x), dtype=torch.float32)
    betas = (torch.linspace(-1.0, 1.0, num_betas) * 0.5).repeat(B, 1)
    tr = t(p.transl) + torch.tensor([0.0, 0.0, 4.0])                 # in front of the camera for the projected form
    with torch.no_grad():
        j3d = TorchSMPL(_consts(num_betas))(global_orient=t(p.global_orient), body_pose=t(p.body_pose), betas=betas,
                                            transl=tr).joints[:, :K] + 0.01
    uv = torch.stack([FOCAL[0] * j3d[..., 0] / j3d[..., 2], FOCAL[1] * j3d[..., 1] / j3d[..., 2], torch.zeros_like(j3d[..., 2])], dim=-1)
    return dict(j3d=j3d.contiguous(), uv=uv.contiguous(), go=t(p.global_orient) * 0.9, bp=t(p.body_pose) * 0.9, be=betas * 0.5,
                tr=tr + 0.02, preserve=t(p.body_pose) * 0.8)


def _fit(num_betas, n, shape, projected=False, preserve=False, turns=False):
    from keypoints2body_amd import native
    q = _problem(num_betas)
    cfg = native.default_fit_config()
    cfg.num_iters = ITERS
    cfg.debug_launch_shape = H.LAUNCH_SHAPES[shape]
    cfg.pose_preserve_weight = 5.0 if preserve else 0.0
    if projected:
        cfg.projection = 1
        cfg.focal[0], cfg.focal[1] = FOCAL
    c = lambda x: x[:n].cuda().contiguous()
    bp = q["bp"].clone()
    if turns:
        # joint 7 (body_pose[18:21]) of frame 3: 1200 rad about an oblique axis, the other frames of its wave and workgroup ordinary
        bp[3, 18:21] = torch.tensor([1100.0, 400.0, -270.0])
        assert float(bp[3, 18:21].norm()) > 1.0e3
    return native.fit_world(_native(num_betas), H.native_prior(), cfg, list(range(K)), c(q["uv"] if projected else q["j3d"]), None,
                            c(q["go"]), c(bp), c(q["be"]), c(q["tr"]), preserve_pose=c(q["preserve"]) if preserve else None,
                            want_grad=True)


def _assert_wide_equals_paired(num_betas, n, **kw):
    wide, paired = _fit(num_betas, n, "wide", **kw), _fit(num_betas, n, "paired", **kw)
    for k in KEYS:
        assert wide[k].shape[0] == n
        assert torch.isfinite(wide[k]).all(), f"{n} frames, {kw}: {k} is not finite"
        assert torch.equal(wide[k], paired[k]), f"{n} frames, {num_betas} betas, {kw}: {k} of the wide shape differs from the paired shape"
    return wide


@pytest.mark.parametrize("num_betas", [10, 16])
@pytest.mark.parametrize("n", [16, 15, 9, 33])
def test_first_frame(n, num_betas):
    _assert_wide_equals_paired(num_betas, n)


@pytest.mark.parametrize("n", [15, 33])
def test_followup_frame_with_preserve_term(n):
    with_term = _assert_wide_equals_paired(10, n, preserve=True)
    without = _fit(10, n, "wide")
    assert not torch.equal(with_term["body_pose"], without["body_pose"]), "the preserve term had no effect"


@pytest.mark.parametrize("num_betas", [10, 16])
@pytest.mark.parametrize("n", [9, 33])
def test_projected_form(n, num_betas):
    _assert_wide_equals_paired(num_betas, n, projected=True)


@pytest.mark.parametrize("n", [9, 33])
def test_rotation_beyond_1e3_rad(n):
    turned = _assert_wide_equals_paired(10, n, turns=True)
    plain = _fit(10, n, "wide")
    # frames are independent: every frame but the turned one is what the batch without it gives
    keep = [i for i in range(n) if i != 3]
    for k in KEYS:
        assert torch.equal(turned[k][keep], plain[k][keep]), f"{k}: the turned frame changed another frame"
    assert not torch.equal(turned["body_pose"][3], plain["body_pose"][3])
