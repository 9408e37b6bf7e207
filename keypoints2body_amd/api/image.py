"""``optimize_params_frame_2d``: fit one frame of 2D keypoints under a pinhole camera, executed on the HIP engine.

The reference has no counterpart (its ``api/frame.py:71-75`` raises for ``input_type="joints2d"``, and so do this package's
existing entry points: ``common.check_request`` is untouched).  The capability is this function of its own; what it computes is
defined in ``core/fitters/image_space.py`` and ``include/k2b.h`` (``k2b_fit_config.projection``)."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from ..core.config import FrameOptimizeConfig, ModelType, frame_config_from
from ..core.engine import default_init_params, load_mean_pose_shape, upgrade_smpl_family_init_params
from ..core.fitters.image_space import ImageSpaceFitter
from ..core.joints.adapters import resolve_adapter
from ..models.smpl_data import BodyModelFitResult, BodyModelParams
from . import common


def _keypoints_and_conf(keypoints2d, conf):
    """(K,2) or (K,3) [u, v, confidence] -> float64 (K,2), float32 (K,)."""
    kp = keypoints2d.detach().cpu().numpy() if isinstance(keypoints2d, torch.Tensor) else np.asarray(keypoints2d)
    if kp.ndim != 2 or kp.shape[1] not in (2, 3):
        raise ValueError(f"Expected keypoints2d shape (K,2) or (K,3), got {tuple(kp.shape)}")
    if conf is None:
        conf = kp[:, 2] if kp.shape[1] == 3 else np.ones(kp.shape[0])
    conf = conf.detach().cpu().numpy() if isinstance(conf, torch.Tensor) else np.asarray(conf)
    if conf.shape != (kp.shape[0],):
        raise ValueError(f"conf must be ({kp.shape[0]},), got {tuple(conf.shape)}")
    return kp[:, :2].astype(np.float64), conf.astype(np.float32)


def optimize_params_frame_2d(keypoints2d, *, focal, principal_point, conf=None, body_model: ModelType = "smpl", model=None,
                             config: Optional[FrameOptimizeConfig | dict] = None, init_params: Optional[BodyModelParams] = None,
                             joint_layout: Optional[str] = None, target_model_indices=None, sigma: float = 100.0,
                             joint_loss_weight: float = 1.0, device=None, pose_prior=None,
                             mean_params: Optional[tuple] = None) -> BodyModelFitResult:
    """Optimise body parameters and the camera translation for a single frame of 2D keypoints.

    ``keypoints2d`` (K,2) pixels, or (K,3) with a confidence column; ``focal`` a number or ``(fx, fy)`` in pixels;
    ``principal_point`` ``(cx, cy)``.  The joint order is named by ``joint_layout`` as for ``optimize_params_frame`` (22 AMASS
    or 24 SMPL joints by count; layouts that rotate 3D axes make no sense for pixels and are refused), or given joint by joint
    with ``target_model_indices``.  ``config`` supplies ``step_size``, ``num_iters`` (per stage), ``pose_preserve_weight`` and
    ``freeze_betas``; ``use_lbfgs`` must be False there (without a config it is): the fit runs Adam only.  ``sigma`` (pixels) and
    ``joint_loss_weight`` are the GMoF scale and the weight of the pixel term.  ``init_params`` (without it: the mean pose and
    shape, ``mean_params`` or the reference's file) starts the fit; its ``transl`` is not read - the camera translation starts
    from similar triangles over the torso.  The result's ``params.transl`` is the camera translation; joints and vertices are in
    model space.  The term has no reference counterpart (``ImageSpaceFitter``)."""
    device = common.resolve_device(device)
    frame_cfg = frame_config_from(config) if config is not None else FrameOptimizeConfig(use_lbfgs=False)
    if body_model not in common.SMPL_FAMILY:
        raise ValueError(f"Unsupported body_model for 2D keypoints: {body_model}")
    uv, cf = _keypoints_and_conf(keypoints2d, conf)
    if target_model_indices is None:
        ad = resolve_adapter(uv.shape[0], joint_layout)
        if ad.rotate_osim_to_smpl or ad.out_layout not in ("SMPL24", "AMASS"):
            raise ValueError(f"joint_layout={joint_layout!r} is defined for 3D joints only")
        if ad.mapping is not None:
            uv, cf = uv[list(ad.mapping)], cf[list(ad.mapping)]
        category = ad.out_layout
    else:
        category = "GENERIC"
    model = common.obtain_model(model, body_model, device)
    fitter = ImageSpaceFitter(model, step_size=frame_cfg.step_size, num_iters=frame_cfg.num_iters, use_lbfgs=frame_cfg.use_lbfgs,
                              joints_category=category, device=device, pose_prior_num_gaussians=frame_cfg.pose_prior_num_gaussians,
                              pose_prior=pose_prior)
    if init_params is None:
        mean_pose, mean_shape = mean_params if mean_params is not None else load_mean_pose_shape(common.DEFAULT_MEAN_FILE, device)
        base = default_init_params(mean_pose.to(device), mean_shape.to(device), None, model, joints_category=category,
                                   coordinate_mode="camera")
        init_params = upgrade_smpl_family_init_params(base, model_type=body_model, model=model, device=device)
    else:
        common.check_param_type(init_params, body_model, "init_params")
        init_params = init_params.to(device)
    return fitter.fit_frame(init_params, uv[None], focal, principal_point, cf, seq_ind=0, target_model_indices=target_model_indices,
                            sigma=sigma, joint_loss_weight=joint_loss_weight, pose_preserve_weight=frame_cfg.pose_preserve_weight,
                            freeze_betas=frame_cfg.freeze_betas)
