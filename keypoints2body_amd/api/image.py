"""``optimize_params_frame_2d`` / ``optimize_params_sequence_2d`` / ``optimize_params_sequences_2d``: fit one frame, one video or
many videos of 2D keypoints under a pinhole camera, executed on the HIP engine.

The reference has no counterpart (its ``api/frame.py:71-75`` raises for ``input_type="joints2d"``, and so do this package's
existing entry points: ``common.check_request`` is untouched).  The capability is this function of its own; what it computes is
defined in ``core/fitters/image_space.py`` and ``include/k2b.h`` (``k2b_fit_config.projection``)."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from ..core.config import FrameOptimizeConfig, ModelType, SequenceOptimizeConfig, frame_config_from, sequence_config_from
from ..core.fitters.image_space import ImageSpaceFitter, check_torso_targets
from ..core.joints.adapters import _BLOCKS, _block_indices, resolve_adapter
from ..models.smpl_data import BodyModelFitResult, BodyModelParams
from . import common
from .sequence import SequenceBatch, _batched_results, _packed_batch, _stack_starts


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


def _blocks_2d(blocks: dict, body_model: str, sequence: bool, target_model_indices):
    """The reference-style dict of blocks (``body`` 22 or 24 points, ``left_hand`` / ``right_hand`` 21, ``face`` k) as one array
    and its model indices, exactly as the 3D dict input maps them (``adapters._block_indices``; the face block at 67 ..): rows
    (K,2|3) per block for a frame, (T,K,2|3) for a sequence, a third column the confidence.  Pure host work: every refusal
    (an unknown or misplaced block, blocks of different T, missing torso joints) comes before any device call."""
    if target_model_indices is not None:
        raise ValueError("a dict of blocks names its own model indices: target_model_indices must be None")
    unknown = sorted(set(blocks) - {name for name, _, _ in _BLOCKS})
    if unknown:
        raise ValueError(f"unknown keypoint blocks {unknown}: expected body, left_hand, right_hand, face")
    pts, idx, frames = [], [], None
    for name, _, _ in _BLOCKS:
        if name not in blocks:
            continue
        b = blocks[name]
        kp = np.asarray(b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else b, dtype=np.float64)
        if kp.ndim != (3 if sequence else 2) or kp.shape[-1] not in (2, 3):
            want = "(T,K,2) or (T,K,3)" if sequence else "(K,2) or (K,3)"
            raise ValueError(f"Expected the {name} block of shape {want}, got {tuple(kp.shape)}")
        if sequence:
            if frames is None:
                frames = kp.shape[0]
            elif kp.shape[0] != frames:
                raise ValueError("all dict sequence blocks must share same T")
        if kp.shape[-1] == 2:                                 # (no confidence column: ones)
            kp = np.concatenate([kp, np.ones(kp.shape[:-1] + (1,))], axis=-1)
        idx.extend(_block_indices(name, kp.shape[-2], body_model).tolist())
        pts.append(kp)
    if not pts:
        raise ValueError("dict input must provide at least one of: body, left_hand, right_hand, face")
    check_torso_targets(idx)
    return np.concatenate(pts, axis=-2), idx


def _fitter_and_starts(uv, cf, frame_cfg, body_model, model, init_params, count, joint_layout, target_model_indices, device,
                       pose_prior, mean_params):
    """Keypoint layout -> ``(ImageSpaceFitter, `count` starts, keypoints and confidences in the fitter's joint order)``: `uv`
    (..., K, 2) and `cf` (..., K) in the order `joint_layout` names (or that of `target_model_indices`), `init_params` None
    (the mean pose and shape for every start) or a list of `count` given starts."""
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
    fitter = ImageSpaceFitter(model, step_size=frame_cfg.step_size, num_iters=frame_cfg.num_iters, use_lbfgs=frame_cfg.use_lbfgs,
                              joints_category=category, device=device, pose_prior_num_gaussians=frame_cfg.pose_prior_num_gaussians,
                              pose_prior=pose_prior, num_iters_followup=frame_cfg.num_iters_followup)
    if init_params is None:
        starts = [common.default_start(model, body_model, category, "camera", None, mean_params, device)] * count
    else:
        for p in init_params:
            common.check_param_type(p, body_model, "init_params")
        starts = [p.to(device) for p in init_params]
    return fitter, starts, uv, cf


def optimize_params_frame_2d(keypoints2d, *, focal, principal_point, conf=None, body_model: ModelType = "smpl", model=None,
                             config: Optional[FrameOptimizeConfig | dict] = None, init_params: Optional[BodyModelParams] = None,
                             joint_layout: Optional[str] = None, target_model_indices=None, sigma: float = 100.0,
                             joint_loss_weight: float = 1.0, device=None, pose_prior=None,
                             mean_params: Optional[tuple] = None) -> BodyModelFitResult:
    """Optimise body parameters and the camera translation for a single frame of 2D keypoints.

    ``keypoints2d`` (K,2) pixels, or (K,3) with a confidence column, or the reference-style dict of blocks (``body`` 22 or 24
    points, ``left_hand`` / ``right_hand`` 21 points on SMPL-H / SMPL-X, ``face`` k points on SMPL-X, each (K,2) or (K,3)), mapped
    to model indices as the 3D dict input maps them - hand and face points are surface targets, projected like the joints
    (``k2b_fit_image``); ``target_model_indices`` may name such indices too (extra joints on SMPL).  ``focal`` a number or ``(fx, fy)`` in pixels;
    ``principal_point`` ``(cx, cy)``.  The joint order is named by ``joint_layout`` as for ``optimize_params_frame`` (22 AMASS
    or 24 SMPL joints by count; layouts that rotate 3D axes make no sense for pixels and are refused), or given joint by joint
    with ``target_model_indices``.  ``config`` supplies ``step_size``, ``num_iters`` (per stage), ``pose_preserve_weight`` and
    ``freeze_betas``; ``use_lbfgs`` must be False there (without a config it is): the fit runs Adam only.  ``sigma`` (pixels) and
    ``joint_loss_weight`` are the GMoF scale and the weight of the pixel term.  ``init_params`` (without it: the mean pose and
    shape, ``mean_params`` or the reference's file) starts the fit; its ``transl`` is not read - the camera translation starts
    from similar triangles over the torso.  The result's ``params.transl`` is the camera translation; joints and vertices are in
    model space.  The term has no reference counterpart (``ImageSpaceFitter``)."""
    if body_model not in common.SMPL_FAMILY:
        raise ValueError(f"Unsupported body_model for 2D keypoints: {body_model}")
    if isinstance(keypoints2d, dict):
        keypoints2d, target_model_indices = _blocks_2d(keypoints2d, body_model, False, target_model_indices)
    device = common.resolve_device(device)
    frame_cfg = frame_config_from(config) if config is not None else FrameOptimizeConfig(use_lbfgs=False)
    uv, cf = _keypoints_and_conf(keypoints2d, conf)
    fitter, (init_params,), uv, cf = _fitter_and_starts(uv, cf, frame_cfg, body_model, model, None if init_params is None else [init_params],
                                                        1, joint_layout, target_model_indices, device, pose_prior, mean_params)
    return fitter.fit_frame(init_params, uv[None], focal, principal_point, cf, seq_ind=0, target_model_indices=target_model_indices,
                            sigma=sigma, joint_loss_weight=joint_loss_weight, pose_preserve_weight=frame_cfg.pose_preserve_weight,
                            freeze_betas=frame_cfg.freeze_betas)


def _sequence_keypoints(keypoints_seq):
    """(T,K,2) or (T,K,3) [u, v, confidence] -> float64 (T,K,2), float32 (T,K) per-frame confidences."""
    kp = keypoints_seq.detach().cpu().numpy() if isinstance(keypoints_seq, torch.Tensor) else np.asarray(keypoints_seq)
    if kp.ndim != 3 or kp.shape[2] not in (2, 3):
        raise ValueError(f"Expected a keypoint sequence of shape (T,K,2) or (T,K,3), got {tuple(kp.shape)}")
    conf = kp[..., 2] if kp.shape[2] == 3 else np.ones(kp.shape[:2])
    return kp[..., :2].astype(np.float64), conf.astype(np.float32)


def _fit_videos(seqs, focal, principal_point, body_model, model, config, init_params, joint_layout, target_model_indices, sigma,
                joint_loss_weight, device, pose_prior, mean_params, want_vertices=True):
    """The shared body of the two video entry points: ``(fitter, one start per sequence, params, joints, vertices, loss,
    lengths)`` with the results packed over all frames."""
    if body_model not in common.SMPL_FAMILY:
        raise ValueError(f"Unsupported body_model for 2D keypoints: {body_model}")
    if any(isinstance(k, dict) for k in seqs):                # dicts of blocks: every video names the same model indices
        if not all(isinstance(k, dict) for k in seqs):
            raise ValueError("either every sequence is a dict of blocks or none is")
        seqs, indices = zip(*(_blocks_2d(k, body_model, True, target_model_indices) for k in seqs))
        if any(i != indices[0] for i in indices):
            raise ValueError("every sequence must give the same blocks with the same number of keypoints")
        target_model_indices = indices[0]
    device = common.resolve_device(device)
    seq_cfg = sequence_config_from(config) if config is not None else SequenceOptimizeConfig(frame=FrameOptimizeConfig(use_lbfgs=False))
    frame_cfg = seq_cfg.frame
    S = len(seqs)
    if init_params is not None and (not isinstance(init_params, (list, tuple)) or len(init_params) != S):
        raise ValueError("init_params must be None or a list with one start per sequence")
    uvs, cfs = zip(*(_sequence_keypoints(k) for k in seqs))
    if len({u.shape[1] for u in uvs}) != 1:
        raise ValueError("every sequence must have the same number of keypoints")
    if seq_cfg.limit_frames is not None and seq_cfg.limit_frames > 0:
        uvs, cfs = [u[: seq_cfg.limit_frames] for u in uvs], [c[: seq_cfg.limit_frames] for c in cfs]
    uv, cf = np.concatenate(uvs, axis=0), np.concatenate(cfs, axis=0)
    lengths = np.asarray([u.shape[0] for u in uvs], dtype=np.int32)
    fitter, starts, uv, cf = _fitter_and_starts(uv, cf, frame_cfg, body_model, model, init_params, S, joint_layout, target_model_indices,
                                                device, pose_prior, mean_params)
    kw = dict(target_model_indices=target_model_indices, sigma=sigma, joint_loss_weight=joint_loss_weight, want_vertices=want_vertices,
              pose_preserve_weight=frame_cfg.pose_preserve_weight, freeze_betas=frame_cfg.freeze_betas)
    if seq_cfg.use_previous_frame_init or len(uv) == 0:
        out, joints, verts, loss = fitter.fit_sequences(_stack_starts(starts, device), uv, lengths, focal, principal_point, cf, **kw)
    else:                                       # independent frames: both stages for every frame, each from its sequence's start
        rows = _stack_starts([starts[s] for s in range(S) for _ in range(int(lengths[s]))], device)
        out, joints, verts, loss = fitter.fit_batch(rows, uv, focal, principal_point, cf, seq_ind=0, per_frame_conf=True, **kw)
    return fitter, starts, out, joints, verts, loss, lengths


def optimize_params_sequence_2d(keypoints_seq, *, focal, principal_point, body_model: ModelType = "smpl", model=None,
                                config: Optional[SequenceOptimizeConfig | dict] = None, init_params: Optional[BodyModelParams] = None,
                                joint_layout: Optional[str] = None, target_model_indices=None, sigma: float = 100.0,
                                joint_loss_weight: float = 1.0, device=None, pose_prior=None,
                                mean_params: Optional[tuple] = None) -> list[BodyModelFitResult]:
    """Fit a video of 2D keypoints, ``keypoints_seq`` (T,K,2) pixels or (T,K,3) with a confidence column, or a dict of such
    blocks (``optimize_params_frame_2d``), as ONE warm-start
    chain on the device (stage 1 for the first frame, then one ``k2b_fit_image_sequences`` launch for all frames - with surface
    targets among them, one ``k2b_fit_image`` call per frame index, queued without a host round trip); results in
    temporal order, frame 0's parameters equal to ``optimize_params_frame_2d`` on that frame.

    ``config`` is a ``SequenceOptimizeConfig`` or dict (without one: Adam, the defaults): ``frame.num_iters`` iterations for
    stage 1 and for a video's first frame, ``frame.num_iters_followup`` for every later frame, ``frame.step_size``, ``frame.pose_preserve_weight``,
    ``frame.freeze_betas`` (the frames after the first hold the first frame's shape); ``frame.use_lbfgs=True`` raises, as for the
    frame entry.  ``use_shape_optimization`` is IGNORED: there is no 2D shape pre-pass, the first frame estimates the shape.
    With ``use_previous_frame_init=False`` every frame is an independent two-stage fit from its sequence's start
    (``ImageSpaceFitter.fit_batch``).  ``limit_frames`` applies.  A third keypoint column is a per-frame confidence.  The other
    arguments are ``optimize_params_frame_2d``'s.  Each result's ``loss`` is the chain's own: the loss of the frame's last iteration
    before its step, preserve term included (``ImageSpaceFitter.fit_sequences``), not the frame entry's re-evaluated loss."""
    fitter, starts, out, joints, verts, loss, lengths = _fit_videos(
        [keypoints_seq], focal, principal_point, body_model, model, config, None if init_params is None else [init_params],
        joint_layout, target_model_indices, sigma, joint_loss_weight, device, pose_prior, mean_params)
    return _batched_results(fitter, out, joints, verts, loss, starts[0], int(lengths[0]))


def optimize_params_sequences_2d(keypoints_seqs, *, focal, principal_point, body_model: ModelType = "smpl", model=None,
                                 config: Optional[SequenceOptimizeConfig | dict] = None, init_params: Optional[list] = None,
                                 joint_layout: Optional[str] = None, target_model_indices=None, sigma: float = 100.0,
                                 joint_loss_weight: float = 1.0, device=None, pose_prior=None,
                                 mean_params: Optional[tuple] = None) -> SequenceBatch:
    """``optimize_params_sequence_2d`` for many videos of different lengths side by side (one camera): stage 1 for all first
    frames in one launch, all chains in ONE ``k2b_fit_image_sequences`` launch; a packed ``SequenceBatch`` whose sequence s
    equals the single call on it bit for bit.  ``init_params``: None or one start (one row) per video; ``config`` and everything
    else as ``optimize_params_sequence_2d`` (``use_shape_optimization`` ignored, ``use_lbfgs=True`` refused, independent frames with
    ``use_previous_frame_init=False``, a third keypoint column as per-frame confidence, the chain's own loss)."""
    if not isinstance(keypoints_seqs, (list, tuple)):
        raise TypeError("keypoints_seqs must be a list of sequences")
    if len(keypoints_seqs) == 0:
        raise ValueError("keypoints_seqs is empty")
    fitter, starts, out, joints, _, loss, lengths = _fit_videos(
        list(keypoints_seqs), focal, principal_point, body_model, model, config, init_params, joint_layout, target_model_indices,
        sigma, joint_loss_weight, device, pose_prior, mean_params, want_vertices=False)
    from ..native import ragged_offsets
    return _packed_batch(fitter, out, joints, loss, lengths, ragged_offsets(lengths), starts)
