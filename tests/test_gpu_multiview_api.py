"""GPU: ``optimize_params_frame_multiview`` / ``optimize_params_frames_multiview`` end to end on a synthetic SMPL model.  A seeded
pose is seen by the four cameras of the rig (tests/multiview_common.py) with exact projections; from the zero pose and shape the
multi-view fit is compared with ``optimize_params_frame_2d`` on each view's keypoints alone - the existing entry on the same
data, so no absolute number is fixed here."""
import functools

import numpy as np
import pytest
import torch

import keypoints2body_amd as k2b
from keypoints2body_amd.core.config import FrameOptimizeConfig
from keypoints2body_amd.core.fitters.multiview import MultiViewFitter
from keypoints2body_amd.models.body_model import BodyModel
from keypoints2body_amd.models.smpl_data import SMPLData
from keypoints2body_amd.prior import MaxMixturePrior, MixtureBuffers
from tests import fit_gradient_common as G
from tests import helpers as H
from tests import multiview_common as MV

pytestmark = pytest.mark.gpu

KIND, C, K, FRAMES, ITERS = "smpl10", 4, 22, 3, 100
PP = ((320.5, 240.25), (300.0, 250.0), (310.0, 236.5), (330.25, 244.0))


@functools.lru_cache(maxsize=None)
def _assets():
    g = H.gmm_fixture()
    prior = MaxMixturePrior(MixtureBuffers(g["ref_means"], g["ref_precisions"], g["ref_nll_weights"].reshape(-1)))
    c = G.consts(KIND)
    return BodyModel(c.v_template, c.shapedirs, c.posedirs, c.J_regressor, c.lbs_weights, c.parents, c.extra_vertex_ids, model_type="smpl",
                     num_betas=10), prior


@functools.lru_cache(maxsize=None)
def _scene():
    """The truth (``multiview_common.base``: centred on the world origin), its joints in world space, its exact pixels in
    every view with each camera's principal point added, and the cameras."""
    truth = MV.base(KIND, C, B=FRAMES, seed=53)
    uv, _ = MV.project64(KIND, truth.go, truth.pose, truth.shape, truth.tr, truth.cams)
    pixels = uv[:, :, :K] + np.asarray(PP)[None, :, None, :]
    cams = [k2b.Camera(Rc, tc, tuple(fc), pp) for (Rc, tc, fc), pp in zip(truth.cams, PP)]
    return truth, G.joints64(KIND, truth.go, truth.pose, truth.shape, truth.tr), pixels, cams


def _start(rows=1):
    z = lambda n: torch.zeros((rows, n))
    return SMPLData(betas=z(10), global_orient=z(3), body_pose=z(69), transl=None)


def _kw():
    model, prior = _assets()
    return dict(body_model="smpl", model=model, pose_prior=prior, config=FrameOptimizeConfig(use_lbfgs=False, num_iters=ITERS, freeze_betas=False))


@functools.lru_cache(maxsize=None)
def _multi(frame):
    _, _, pixels, cams = _scene()
    return k2b.optimize_params_frame_multiview(pixels[frame], cameras=cams, init_params=_start(), **_kw())


@functools.lru_cache(maxsize=None)
def _single(frame, view):
    _, _, pixels, cams = _scene()
    return k2b.optimize_params_frame_2d(pixels[frame, view], focal=cams[view].focal, principal_point=cams[view].principal_point,
                                        init_params=_start(), **_kw())


def _residual(points_cam, cam, pixels):
    """Mean pixel distance of camera-space points (K, 3) from `pixels` (K, 2)."""
    f, pp = np.asarray(cam.focal), np.asarray(cam.principal_point)
    proj = points_cam[:, :2] / points_cam[:, 2:3] * f + pp
    return float(np.linalg.norm(proj - pixels, axis=1).mean())


@pytest.mark.parametrize("frame", range(FRAMES))
def test_four_views_do_at_least_as_well_as_any_one(frame):
    truth, joints_world, pixels, cams = _scene()
    multi = _multi(frame)
    assert isinstance(multi, k2b.BodyModelFitResult) and isinstance(multi.params, k2b.SMPLData)
    got = multi.joints[0, :K].cpu().double().numpy()                                  # world space, translation applied
    mpjpe_multi = float(np.linalg.norm(got - joints_world[frame, :K], axis=1).mean())
    for view, cam in enumerate(cams):
        one = _single(frame, view)
        in_cam = one.joints[0, :K].cpu().double().numpy() + one.params.transl[0].cpu().double().numpy()      # model space + camera translation
        truth_cam = joints_world[frame, :K] @ cam.rotation.T + cam.translation
        mpjpe_one = float(np.linalg.norm(in_cam - truth_cam, axis=1).mean())
        r_multi = _residual(got @ cam.rotation.T + cam.translation, cam, pixels[frame, view])
        r_one = _residual(in_cam, cam, pixels[frame, view])
        print(f"frame {frame} view {view}: reprojection {r_multi:.3f} px (four views) / {r_one:.3f} px (this view alone); "
              f"MPJPE {1e3 * mpjpe_multi:.2f} mm / {1e3 * mpjpe_one:.2f} mm")
        assert r_multi <= r_one, (frame, view, r_multi, r_one)
        assert mpjpe_multi < mpjpe_one, (frame, view, mpjpe_multi, mpjpe_one)


def test_the_frames_entry_is_the_frame_entry_row_by_row():
    _, _, pixels, cams = _scene()
    conf = np.ones(pixels.shape[:3] + (1,))
    conf[1, 2, 5] = 0.0                                                               # one pair out, in one frame
    batch = k2b.optimize_params_frames_multiview(np.concatenate([pixels, conf], axis=-1), cameras=cams,
                                                 init_params=[_start() for _ in range(FRAMES)], **_kw())
    assert len(batch) == FRAMES
    for t, res in enumerate(batch):
        one = _multi(t) if t != 1 else k2b.optimize_params_frame_multiview(pixels[1], cameras=cams, conf=conf[1, ..., 0], init_params=_start(), **_kw())
        for key in ("global_orient", "body_pose", "betas", "transl"):
            assert torch.equal(getattr(res.params, key), getattr(one.params, key)), (t, key)
        assert torch.equal(res.joints, one.joints) and torch.equal(res.vertices, one.vertices) and float(res.loss) == float(one.loss), t
    assert not torch.equal(batch[1].params.body_pose, _multi(1).params.body_pose)     # (the pair that was taken out did count)


def test_a_torso_joint_that_one_view_sees_is_a_value_error():
    _, _, pixels, cams = _scene()
    conf = np.ones(pixels.shape[1:3])
    conf[1:, 16] = 0.0                                                                # the left shoulder: camera 0 alone
    with pytest.raises(ValueError, match="fewer than two views"):
        k2b.optimize_params_frame_multiview(pixels[0], cameras=cams, conf=conf, init_params=_start(), **_kw())
    conf[1, 16] = 1.0                                                                 # two views: taken
    k2b.optimize_params_frame_multiview(pixels[0], cameras=cams, conf=conf, init_params=_start(), **_kw())
    with pytest.raises(ValueError, match="torso"):
        k2b.optimize_params_frame_multiview(pixels[0][:, :5], cameras=cams, target_model_indices=[0, 1, 2, 3, 4], init_params=_start(), **_kw())


def test_lbfgs_and_surface_indices_are_not_implemented():
    model, prior = _assets()
    _, _, pixels, cams = _scene()
    kw = dict(_kw(), init_params=_start(), cameras=cams)
    with pytest.raises(NotImplementedError, match="Adam only"):
        k2b.optimize_params_frame_multiview(pixels[0], **dict(kw, config=FrameOptimizeConfig(use_lbfgs=True)))
    with pytest.raises(NotImplementedError, match="Adam only"):
        MultiViewFitter(model, use_lbfgs=True, pose_prior=prior)
    idx = list(range(21)) + [24]                                                      # 24: the first index past the kinematic joints
    with pytest.raises(NotImplementedError, match="kinematic targets only"):
        k2b.optimize_params_frame_multiview(pixels[0], target_model_indices=idx, **kw)
    with pytest.raises(NotImplementedError, match="kinematic targets only"):
        k2b.optimize_params_frame_multiview({"body": pixels[0, 0]}, **kw)
