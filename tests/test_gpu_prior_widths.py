"""The tree kernel's lane table per prior width (``k2b_fit_config.prior_pose_dims``): one immutable device table per width on the
model handle, built on the first use of that width.  Calls of one handle with different widths - one after another on one
stream, or in flight on two streams at once - give, bit for bit, what a fresh handle that has only ever seen that width gives.

Synthetic SMPL-X model (20 shape coefficients), 2 frames, all 55 kinematic joints as targets, the default bending indices (they
reach pose dimension 55, so the widths are 57 and up)."""
import functools

import numpy as np
import pytest
import torch

from tests import helpers as H

pytestmark = pytest.mark.gpu
FRAMES, JOINTS, ITERS = 2, 55, 3
KEYS = ("global_orient", "body_pose", "betas", "transl", "loss")


@functools.lru_cache(maxsize=None)
def inputs():
    """Targets: the model's joints at a seeded pose; starts: a third of that pose."""
    from keypoints2body_amd import synthetic
    p = synthetic.make_poses_x(FRAMES, seed=5)
    pose = np.concatenate([p.body_pose, p.jaw_pose, p.leye_pose, p.reye_pose, p.left_hand_pose, p.right_hand_pose], axis=1)
    shape = np.concatenate([p.betas, p.expression], axis=1)
    go, pose, shape, tr = map(H.cuda, (p.global_orient, pose, shape, p.transl))
    joints, _ = H.native_model_x().lbs(go, pose, shape, tr, want_vertices=False)
    starts = tuple((x / 3).contiguous() for x in (go, pose, shape, tr))
    torch.cuda.synchronize()
    return joints[:, :JOINTS].contiguous(), starts


def call(model, width: int, evaluate: bool):
    """A fit of ITERS Adam iterations, or one evaluate-only closure with its gradient, on the current stream."""
    from keypoints2body_amd import native
    cfg = native.default_fit_config()
    cfg.prior_pose_dims, cfg.num_betas_prior = width, 10
    cfg.num_iters = 1 if evaluate else ITERS
    if evaluate:
        cfg.step_size = 0.0
    j3d, starts = inputs()
    return native.fit_world(model, H.native_prior(), cfg, list(range(JOINTS)), j3d, None, *starts, want_grad=evaluate)


@functools.lru_cache(maxsize=None)
def reference(width: int):
    """(fit, evaluation) of a fresh handle that sees this width alone; computed once, shared by the tests, never written."""
    from keypoints2body_amd.native import NativeModel
    c = H.body_consts_x()
    fresh = NativeModel(c.v_template, c.shapedirs, c.posedirs, c.J_regressor, c.lbs_weights, c.parents, c.extra_vertex_ids)
    out = call(fresh, width, False), call(fresh, width, True)
    torch.cuda.synchronize()
    return out


def assert_same(got: dict, want: dict, what: str):
    for k in KEYS + (("grad",) if "grad" in want else ()):
        assert torch.equal(got[k], want[k]), f"{what}: {k} differs from the fresh handle's"


def test_widths_alternate_on_one_stream():
    model = H.native_model_x()
    for step, width in enumerate((63, 60, 63)):
        fit, ev = call(model, width, False), call(model, width, True)
        assert_same(fit, reference(width)[0], f"call {step}, width {width}, fit")
        assert_same(ev, reference(width)[1], f"call {step}, width {width}, evaluation")
    assert not torch.equal(reference(60)[0]["body_pose"], reference(63)[0]["body_pose"])      # the width is not ignored


def test_widths_in_flight_on_two_streams():
    model = H.native_model_x()
    refs = {w: reference(w) for w in (60, 63)}
    inputs()
    torch.cuda.synchronize()
    streams = {60: torch.cuda.Stream(), 63: torch.cuda.Stream()}
    results = []
    for i in range(8):                                   # per stream: fit, evaluation, fit, evaluation - nothing waits in between
        width, evaluate = (60, 63)[i % 2], bool((i // 2) % 2)
        with torch.cuda.stream(streams[width]):
            results.append((i, width, evaluate, call(model, width, evaluate)))
    torch.cuda.synchronize()
    for i, width, evaluate, out in results:
        assert_same(out, refs[width][int(evaluate)], f"call {i}, width {width}, {'evaluation' if evaluate else 'fit'}")
