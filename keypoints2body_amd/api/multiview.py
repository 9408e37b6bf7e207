"""``optimize_params_frame_multiview`` / ``optimize_params_frames_multiview`` / ``optimize_params_sequence_multiview`` /
``optimize_params_sequences_multiview``: fit one frame, T independent frames, one video or many videos of 2D keypoints seen by
several calibrated cameras at once, executed on the HIP engine.

The reference has no counterpart (its ``api/frame.py:71-75`` raises for ``input_type="joints2d"``).  What is computed is defined
in ``core/fitters/multiview.py`` and ``include/k2b.h`` (``k2b_fit_multiview``, ``k2b_fit_multiview_sequences``)."""
from __future__ import annotations

import dataclasses
from typing import Optional, Sequence

import numpy as np
import torch

from ..core.config import FrameOptimizeConfig, ModelType, SequenceOptimizeConfig, frame_config_from, sequence_config_from
from ..core.fitters.image_space import focal_pair
from ..core.fitters.multiview import MAX_VIEWS, MultiViewFitter, check_rotation
from ..core.joints.adapters import resolve_adapter
from ..models.smpl_data import BodyModelFitResult, BodyModelParams
from . import common
from .sequence import SequenceBatch, _batched_results, _packed_batch, _stack_starts


@dataclasses.dataclass(frozen=True)
class Camera:
    """A calibrated pinhole camera: ``x_camera = rotation @ x_world + translation``, pixels
    ``(fx x / z + cx, fy y / z + cy)``.  `rotation` (3,3) must be orthonormal with determinant +1 within 1e-4 and every value
    finite, `focal` a positive number or ``(fx, fy)``, else ``ValueError``."""
    rotation: np.ndarray
    translation: np.ndarray
    focal: tuple
    principal_point: tuple

    def __post_init__(self):
        object.__setattr__(self, "rotation", check_rotation(self.rotation))
        t = np.asarray(self.translation, dtype=np.float64).reshape(-1)
        if t.shape != (3,) or not np.isfinite(t).all():
            raise ValueError("translation must be three finite numbers")
        object.__setattr__(self, "translation", t)
        object.__setattr__(self, "focal", focal_pair(self.focal))
        pp = np.asarray(self.principal_point, dtype=np.float64).reshape(-1)
        if pp.shape != (2,) or not np.isfinite(pp).all():
            raise ValueError("principal_point must be two finite numbers (cx, cy)")
        object.__setattr__(self, "principal_point", (float(pp[0]), float(pp[1])))


def _views(keypoints, conf, cameras, frames: bool):
    """(C,K,2|3) - with `frames` (T,C,K,2|3) - keypoints, a third column the per-view confidence -> float64 pixels (..., 2) and
    float32 confidences of the same leading shape; `conf` (C,K), where given, takes the column's place."""
    cams = list(cameras)
    if not all(isinstance(c, Camera) for c in cams):
        raise ValueError("cameras must be a sequence of Camera objects")
    if not 1 <= len(cams) <= MAX_VIEWS:
        raise ValueError(f"between 1 and {MAX_VIEWS} cameras, got {len(cams)}")
    if isinstance(keypoints, dict):
        raise NotImplementedError("a dict of blocks names hand and face points, which are surface targets: the multi-view fit takes "
                                  "kinematic targets only")
    kp = keypoints.detach().cpu().numpy() if isinstance(keypoints, torch.Tensor) else np.asarray(keypoints)
    want = "(T,C,K,2) or (T,C,K,3)" if frames else "(C,K,2) or (C,K,3)"
    if kp.ndim != (4 if frames else 3) or kp.shape[-1] not in (2, 3) or kp.shape[-3] != len(cams):
        raise ValueError(f"Expected keypoints of shape {want} with C = {len(cams)} cameras, got {tuple(kp.shape)}")
    if conf is None:
        cf = kp[..., 2] if kp.shape[-1] == 3 else np.ones(kp.shape[:-1])
    else:
        cf = conf.detach().cpu().numpy() if isinstance(conf, torch.Tensor) else np.asarray(conf)
        if cf.shape != kp.shape[-3:-1]:
            raise ValueError(f"conf must be {tuple(kp.shape[-3:-1])}, got {tuple(cf.shape)}")
        cf = np.broadcast_to(cf, kp.shape[:-1])
    return cams, kp[..., :2].astype(np.float64), np.ascontiguousarray(cf, dtype=np.float32)


def _fitter_and_starts(uv, cf, frame_cfg, body_model, model, init_params, count, joint_layout, target_model_indices, device, pose_prior,
                       mean_params):
    """Keypoint layout -> ``(MultiViewFitter, `count` starts, keypoints and confidences in the fitter's joint order)``."""
    if frame_cfg.use_lbfgs:
        raise NotImplementedError("the multi-view fit runs Adam only: pass a config with use_lbfgs=False")
    if target_model_indices is None:
        ad = resolve_adapter(uv.shape[-2], joint_layout)
        if ad.rotate_osim_to_smpl or ad.out_layout not in ("SMPL24", "AMASS"):
            raise ValueError(f"joint_layout={joint_layout!r} is defined for 3D joints only")
        if ad.mapping is not None:
            uv, cf = uv[..., list(ad.mapping), :], cf[..., list(ad.mapping)]
        category = ad.out_layout
    else:
        category = "GENERIC"
    model = common.obtain_model(model, body_model, device)
    if target_model_indices is not None and any(int(j) >= model.num_joints for j in np.asarray(target_model_indices).reshape(-1)):
        raise NotImplementedError(f"the multi-view fit takes kinematic targets only (model indices below {model.num_joints})")
    fitter = MultiViewFitter(model, step_size=frame_cfg.step_size, num_iters=frame_cfg.num_iters, use_lbfgs=False,
                             joints_category=category, device=device, pose_prior_num_gaussians=frame_cfg.pose_prior_num_gaussians,
                             pose_prior=pose_prior, num_iters_followup=frame_cfg.num_iters_followup)
    if init_params is None:
        starts = [common.default_start(model, body_model, category, "camera", None, mean_params, device)] * count
    else:
        for p in init_params:
            common.check_param_type(p, body_model, "init_params")
        starts = [p.to(device) for p in init_params]
    return fitter, starts, uv, cf


def optimize_params_frame_multiview(keypoints2d, *, cameras: Sequence[Camera], conf=None, body_model: ModelType = "smpl", model=None,
                                    config: Optional[FrameOptimizeConfig | dict] = None,
                                    init_params: Optional[BodyModelParams] = None, joint_layout: Optional[str] = None,
                                    target_model_indices=None, sigma: float = 100.0, joint_loss_weight: float = 1.0, device=None,
                                    pose_prior=None, mean_params: Optional[tuple] = None) -> BodyModelFitResult:
    """Optimise body parameters and the body's world translation for one frame of 2D keypoints seen by C calibrated cameras.

    ``keypoints2d`` (C,K,2) pixels per view, or (C,K,3) with a per-view confidence column (``conf`` (C,K) takes its place where
    given); a pair of confidence 0 contributes nothing, so an occluded or missing detection is written that way.  ``cameras``: C
    ``Camera`` objects (1 to 8) in the order of the views.  The joint order is named by ``joint_layout`` as for
    ``optimize_params_frame_2d`` or given joint by joint with ``target_model_indices``; kinematic targets only - a dict of blocks
    or a model index at or above the joint count raises ``NotImplementedError``.  ``config`` supplies ``step_size``, ``num_iters``
    (per stage), ``pose_preserve_weight`` and ``freeze_betas``; ``use_lbfgs=True`` raises ``NotImplementedError``.  ``init_params``
    (without it: the mean pose and shape) starts the fit; its ``transl`` is not read - the translation starts from a
    triangulation of the four torso joints, each of which at least two views must see (else ``ValueError``).  The result's
    ``params.transl`` is the world translation; joints and vertices are in world space (``MultiViewFitter``).

    ``optimize_params_frames_multiview`` fits independent frames, ``optimize_params_sequence_multiview`` a video as a warm-start
    chain."""
    if body_model not in common.SMPL_FAMILY:
        raise ValueError(f"Unsupported body_model for 2D keypoints: {body_model}")
    cams, uv, cf = _views(keypoints2d, conf, cameras, frames=False)
    frame_cfg = frame_config_from(config) if config is not None else FrameOptimizeConfig(use_lbfgs=False)
    if frame_cfg.use_lbfgs:
        raise NotImplementedError("the multi-view fit runs Adam only: pass a config with use_lbfgs=False")
    device = common.resolve_device(device)
    fitter, (start,), uv, cf = _fitter_and_starts(uv, cf, frame_cfg, body_model, model, None if init_params is None else [init_params],
                                                  1, joint_layout, target_model_indices, device, pose_prior, mean_params)
    return fitter.fit_frame(start, uv, cams, cf, seq_ind=0, target_model_indices=target_model_indices, sigma=sigma,
                            joint_loss_weight=joint_loss_weight, pose_preserve_weight=frame_cfg.pose_preserve_weight,
                            freeze_betas=frame_cfg.freeze_betas)


def optimize_params_frames_multiview(keypoints, *, cameras: Sequence[Camera], body_model: ModelType = "smpl", model=None,
                                     config: Optional[FrameOptimizeConfig | dict] = None, init_params: Optional[list] = None,
                                     joint_layout: Optional[str] = None, target_model_indices=None, sigma: float = 100.0,
                                     joint_loss_weight: float = 1.0, device=None, pose_prior=None,
                                     mean_params: Optional[tuple] = None) -> list[BodyModelFitResult]:
    """``optimize_params_frame_multiview`` for T INDEPENDENT frames as one batch: ``keypoints`` (T,C,K,2) or (T,C,K,3) with a
    per-view confidence column, ``init_params`` None or one start per frame.  Two fit launches, one evaluate-only launch and one
    LBS call in total, whatever T; frame t of the result equals the frame entry on that frame bit for bit.

    The frames do not warm-start one another: ``optimize_params_sequence_multiview`` runs the chain over a video (each frame from
    its predecessor's result, with the preserve term)."""
    if body_model not in common.SMPL_FAMILY:
        raise ValueError(f"Unsupported body_model for 2D keypoints: {body_model}")
    cams, uv, cf = _views(keypoints, None, cameras, frames=True)
    frame_cfg = frame_config_from(config) if config is not None else FrameOptimizeConfig(use_lbfgs=False)
    if frame_cfg.use_lbfgs:
        raise NotImplementedError("the multi-view fit runs Adam only: pass a config with use_lbfgs=False")
    T = uv.shape[0]
    if T == 0:
        return []
    if init_params is not None and len(init_params) != T:
        raise ValueError(f"init_params must hold one start per frame: {len(init_params)} for {T} frames")
    device = common.resolve_device(device)
    fitter, starts, uv, cf = _fitter_and_starts(uv, cf, frame_cfg, body_model, model, init_params, T, joint_layout,
                                                target_model_indices, device, pose_prior, mean_params)
    out, joints, verts, loss = fitter.fit_batch(_stack_starts(starts, device), uv, cams, cf, seq_ind=0,
                                                target_model_indices=target_model_indices, sigma=sigma,
                                                joint_loss_weight=joint_loss_weight,
                                                pose_preserve_weight=frame_cfg.pose_preserve_weight,
                                                freeze_betas=frame_cfg.freeze_betas, per_frame_conf=True)
    return _batched_results(fitter, out, joints, verts, loss, starts[0], T)


def _fit_videos(videos, cameras, body_model, model, config, init_params, joint_layout, target_model_indices, sigma, joint_loss_weight,
                device, pose_prior, mean_params, want_vertices=True):
    """The shared body of the two video entry points: ``(fitter, one start per video, params, joints, vertices, loss, lengths)``
    with the results packed over all frames.  Every refusal of the arguments comes before any device call."""
    if body_model not in common.SMPL_FAMILY:
        raise ValueError(f"Unsupported body_model for 2D keypoints: {body_model}")
    seq_cfg = sequence_config_from(config) if config is not None else SequenceOptimizeConfig(frame=FrameOptimizeConfig(use_lbfgs=False))
    frame_cfg = seq_cfg.frame
    if frame_cfg.use_lbfgs:
        raise NotImplementedError("the multi-view fit runs Adam only: pass a config with use_lbfgs=False")
    S = len(videos)
    if init_params is not None and (not isinstance(init_params, (list, tuple)) or len(init_params) != S):
        raise ValueError("init_params must be None or a list with one start per sequence")
    cams, uvs, cfs = None, [], []
    for v in videos:
        cams, uv, cf = _views(v, None, cameras, frames=True)
        uvs.append(uv)
        cfs.append(cf)
    if len({u.shape[2] for u in uvs}) != 1:
        raise ValueError("every sequence must have the same number of keypoints")
    if seq_cfg.limit_frames is not None and seq_cfg.limit_frames > 0:
        uvs, cfs = [u[: seq_cfg.limit_frames] for u in uvs], [c[: seq_cfg.limit_frames] for c in cfs]
    uv, cf = np.concatenate(uvs, axis=0), np.concatenate(cfs, axis=0)
    lengths = np.asarray([u.shape[0] for u in uvs], dtype=np.int32)
    device = common.resolve_device(device)
    fitter, starts, uv, cf = _fitter_and_starts(uv, cf, frame_cfg, body_model, model, init_params, S, joint_layout, target_model_indices,
                                                device, pose_prior, mean_params)
    kw = dict(target_model_indices=target_model_indices, sigma=sigma, joint_loss_weight=joint_loss_weight, want_vertices=want_vertices,
              pose_preserve_weight=frame_cfg.pose_preserve_weight, freeze_betas=frame_cfg.freeze_betas)
    if seq_cfg.use_previous_frame_init or len(uv) == 0:
        out, joints, verts, loss = fitter.fit_sequences(_stack_starts(starts, device), uv, lengths, cams, cf, **kw)
    else:                                       # independent frames: both stages for every frame, each from its video's start
        rows = _stack_starts([starts[s] for s in range(S) for _ in range(int(lengths[s]))], device)
        out, joints, verts, loss = fitter.fit_batch(rows, uv, cams, cf, seq_ind=0, per_frame_conf=True, **kw)
    return fitter, starts, out, joints, verts, loss, lengths


def optimize_params_sequence_multiview(keypoints, *, cameras: Sequence[Camera], body_model: ModelType = "smpl", model=None,
                                       config: Optional[SequenceOptimizeConfig | dict] = None,
                                       init_params: Optional[BodyModelParams] = None, joint_layout: Optional[str] = None,
                                       target_model_indices=None, sigma: float = 100.0, joint_loss_weight: float = 1.0, device=None,
                                       pose_prior=None, mean_params: Optional[tuple] = None) -> list[BodyModelFitResult]:
    """Fit a video of a calibrated rig, ``keypoints`` (T,C,K,2) pixels or (T,C,K,3) with a per-frame, per-view confidence column,
    as ONE warm-start chain on the device: the triangulated start and stage 1 for the first frame, then one
    ``k2b_fit_multiview_sequences`` launch for all frames and one LBS call; results in temporal order, frame 0's parameters equal
    to ``optimize_params_frame_multiview`` on that frame.  ``cameras``: the rig, fixed over the video.

    ``config`` is a ``SequenceOptimizeConfig`` or dict (without one: Adam, the defaults): ``frame.num_iters`` iterations for
    stage 1 and for the first frame, ``frame.num_iters_followup`` for every later frame, ``frame.step_size``,
    ``frame.pose_preserve_weight``, ``frame.freeze_betas`` (the frames after the first hold the first frame's shape);
    ``frame.use_lbfgs=True`` raises ``NotImplementedError``.  ``use_shape_optimization`` is IGNORED: the first frame estimates the
    shape.  With ``use_previous_frame_init=False`` every frame is an independent two-stage fit from the video's start
    (``MultiViewFitter.fit_batch``, as ``optimize_params_frames_multiview``).  ``limit_frames`` applies.  A dict of blocks, or a
    model index at or above the joint count, raises ``NotImplementedError`` (kinematic targets only).  The other arguments are
    ``optimize_params_frame_multiview``'s.  Each result's ``loss`` is the chain's own: the loss of the frame's last iteration
    before its step, preserve term included (``MultiViewFitter.fit_sequences``), not the frame entry's re-evaluated loss."""
    fitter, starts, out, joints, verts, loss, lengths = _fit_videos(
        [keypoints], cameras, body_model, model, config, None if init_params is None else [init_params], joint_layout,
        target_model_indices, sigma, joint_loss_weight, device, pose_prior, mean_params)
    return _batched_results(fitter, out, joints, verts, loss, starts[0], int(lengths[0]))


def optimize_params_sequences_multiview(keypoints_seqs, *, cameras: Sequence[Camera], body_model: ModelType = "smpl", model=None,
                                        config: Optional[SequenceOptimizeConfig | dict] = None, init_params: Optional[list] = None,
                                        joint_layout: Optional[str] = None, target_model_indices=None, sigma: float = 100.0,
                                        joint_loss_weight: float = 1.0, device=None, pose_prior=None,
                                        mean_params: Optional[tuple] = None) -> SequenceBatch:
    """``optimize_params_sequence_multiview`` for many videos of different lengths recorded by ONE rig, side by side: stage 1 for
    all first frames in one launch, all chains in ONE ``k2b_fit_multiview_sequences`` launch; a packed ``SequenceBatch`` whose
    sequence s equals the single call on it bit for bit.  ``init_params``: None or one start (one row) per video; ``config`` and
    everything else as ``optimize_params_sequence_multiview``."""
    if not isinstance(keypoints_seqs, (list, tuple)):
        raise TypeError("keypoints_seqs must be a list of sequences")
    if len(keypoints_seqs) == 0:
        raise ValueError("keypoints_seqs is empty")
    fitter, starts, out, joints, _, loss, lengths = _fit_videos(
        list(keypoints_seqs), cameras, body_model, model, config, init_params, joint_layout, target_model_indices, sigma,
        joint_loss_weight, device, pose_prior, mean_params, want_vertices=False)
    from ..native import ragged_offsets
    return _packed_batch(fitter, out, joints, loss, lengths, ragged_offsets(lengths), starts)
