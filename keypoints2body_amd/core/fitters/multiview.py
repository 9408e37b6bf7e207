"""Multi-view two-stage fitter on the HIP engine: SMPL / SMPL-H / SMPL-X fitted to the 2D keypoints of several calibrated cameras
at once (``k2b_fit_multiview``, ``include/k2b.h``).

The reference has no 2D path (``keypoints2body/api/frame.py:71-75`` raises), so the term is DEFINED here and pinned to a float64
oracle of its own formula (``tests/multiview_common.py``).  For camera c with the world-to-camera rotation ``R_c``, translation
``t_c``, focals ``(fx_c, fy_c)`` and principal point ``(cx_c, cy_c)``, a posed joint ``p`` and the body's world translation:

    q = R_c (p + transl) + t_c,    e = (fx_c q_x / q_z - (u - cx_c), fy_c q_y / q_z - (v - cy_c)),
    loss = w_j^2 sum_c sum_k conf_ck^2 (gmof(e_x, sigma) + gmof(e_y, sigma)) + the priors of the 3D fit,    sigma in pixels.

It is modelled on ``ImageSpaceFitter``; what several views change:

* the principal point of EACH camera is subtracted from that view's keypoints here, in float64, before the rounding to float32
  (``centred_keypoints``);
* initial translation: a linear (DLT) triangulation of the four torso joints (``TORSO_JOINTS``) on the host in float64, every
  joint from the views that see it (confidence not 0), then ``transl0 = mean(triangulated torso) - mean(model torso at the
  start pose)``; the model torso comes from a float64 forward of the kinematic chain on the host, so no device call precedes
  the argument checks and the final forward stays the only LBS call.  A torso joint that is not among the targets, or that
  fewer than two views see, is a ``ValueError`` before any device call;
* stage 1: ``[global_orient, transl]`` (``optimize_mask = 9``) against the torso joints in all views with a plain squared pixel
  error (``stage1_config``; a pair of confidence 0 stays out, every other pair weighs 1) and NO translation prior - several views
  fix the depth, and the tree kernel has none - so 24-joint and SMPL-H / SMPL-X models run the same stage 1;
* stage 2: all targets, all priors, ``sigma`` (default 100 px) and ``joint_loss_weight`` (default 1);
* result: ``transl`` is the WORLD translation, joints and vertices come from the final forward with it applied (as the world
  fitter returns them), ``loss`` is stage 2 re-evaluated at the result without the preserve term (one evaluate-only launch).

Videos (``fit_sequences``): S ragged videos of one rig as warm-start chains - the triangulated start and stage 1 for the S first
frames as one launch, then the whole of stage 2 for every frame of every video as ONE launch (``k2b_fit_multiview_sequences``): a
video's first frame is stage 2 as above, every later frame starts from its predecessor's result, preserves that result's body pose
and, with ``freeze_betas``, holds the shape the first frame estimated.

Adam only (``use_lbfgs=True`` raises), kinematic targets only (a model index at or above the joint count raises
``NotImplementedError``: the multi-view term is not built into the surface kernels).
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from ... import native
from ...models.smpl_data import BodyModelFitResult, SMPLData, select_rows
from ...prior import MaxMixturePrior
from ..config import FrameOptimizeConfig
from .common import TORSO_IDX, FitterBase, stage1_config, stage2_config
from .image_space import centred_keypoints, check_torso_targets, focal_pair

MAX_VIEWS = 8                       # k2b_fit_multiview: 1 <= num_views <= 8
ROTATION_TOLERANCE = 1e-4           # |R R^T - I| and |det R - 1| of a camera rotation


def check_rotation(rotation) -> np.ndarray:
    """A (3,3) float64 rotation, or ``ValueError``: orthonormal with determinant +1 within ``ROTATION_TOLERANCE``.  (The library
    takes any finite matrix - its gradient is the exact chain rule of a linear map -, so the check lives here.)"""
    r = np.asarray(rotation, dtype=np.float64)
    if r.shape != (3, 3) or not np.isfinite(r).all():
        raise ValueError(f"a camera rotation must be a finite (3,3) matrix, got shape {tuple(r.shape)}")
    if np.abs(r @ r.T - np.eye(3)).max() > ROTATION_TOLERANCE or abs(np.linalg.det(r) - 1.0) > ROTATION_TOLERANCE:
        raise ValueError(f"a camera rotation must be orthonormal with determinant +1 within {ROTATION_TOLERANCE:g}")
    return r


def camera_arrays(cameras) -> tuple:
    """``(R (C,3,3), t (C,3), focal (C,2), principal point (C,2))`` in float64 of `cameras` (objects with ``rotation``,
    ``translation``, ``focal``, ``principal_point``), every value checked; 1 .. ``MAX_VIEWS`` of them."""
    cams = list(cameras)
    if not 1 <= len(cams) <= MAX_VIEWS:
        raise ValueError(f"between 1 and {MAX_VIEWS} cameras, got {len(cams)}")
    R = np.stack([check_rotation(c.rotation) for c in cams])
    t = np.stack([np.asarray(c.translation, dtype=np.float64).reshape(-1) for c in cams])
    if t.shape != (len(cams), 3) or not np.isfinite(t).all():
        raise ValueError("a camera translation must be three finite numbers")
    f = np.array([focal_pair(c.focal) for c in cams], dtype=np.float64)
    pp = np.stack([np.asarray(c.principal_point, dtype=np.float64).reshape(-1) for c in cams])
    if pp.shape != (len(cams), 2) or not np.isfinite(pp).all():
        raise ValueError("a principal point must be two finite numbers (cx, cy)")
    return R, t, f, pp


def triangulate_dlt(uv, usable, R, t, focal) -> np.ndarray:
    """Linear (DLT) triangulation in float64: `uv` (B, C, N, 2) centred pixels, `usable` (B, C, N) which views see point n of
    frame b, the cameras' `R` (C,3,3), `t` (C,3), `focal` (C,2) -> world points (B, N, 3).  Every view contributes the two rows
    ``x P_3 - P_1``, ``y P_3 - P_2`` of its ``P = [R | t]`` in normalised image coordinates; the point is the right singular
    vector of the smallest singular value.  ``ValueError`` where fewer than two views see a point."""
    uv = np.asarray(uv, dtype=np.float64)
    usable = np.asarray(usable, dtype=bool)
    if (usable.sum(axis=1) < 2).any():
        b, n = np.argwhere(usable.sum(axis=1) < 2)[0]
        raise ValueError(f"point {int(n)} of frame {int(b)} is seen by fewer than two views: no triangulation")
    P = np.concatenate([np.asarray(R, np.float64), np.asarray(t, np.float64)[:, :, None]], axis=2)      # (C, 3, 4)
    xy = np.where(usable[..., None], uv / np.asarray(focal, np.float64)[None, :, None, :], 0.0)         # (an unseen point may be NaN)
    rows = xy[..., :, None] * P[None, :, None, 2:3, :] - P[None, :, None, 0:2, :]                      # (B, C, N, 2, 4)
    rows = rows * usable[..., None, None]
    A = rows.transpose(0, 2, 1, 3, 4).reshape(uv.shape[0], uv.shape[2], -1, 4)                         # (B, N, 2C, 4)
    X = np.linalg.svd(A)[2][..., -1, :]
    return X[..., :3] / X[..., 3:4]


def _rodrigues(rotvec: np.ndarray) -> np.ndarray:
    """(..., 3) axis-angle -> (..., 3, 3) in float64."""
    angle = np.linalg.norm(rotvec, axis=-1)[..., None, None]
    k = np.zeros(rotvec.shape[:-1] + (3, 3))
    k[..., 0, 1], k[..., 0, 2], k[..., 1, 2] = -rotvec[..., 2], rotvec[..., 1], -rotvec[..., 0]
    k = k - np.swapaxes(k, -1, -2)
    small = angle < 1e-12
    a = np.where(small, 1.0, np.sin(angle) / np.where(small, 1.0, angle))
    b = np.where(small, 0.5, (1.0 - np.cos(angle)) / np.where(small, 1.0, angle * angle))
    return np.eye(3) + a * k + b * (k @ k)


def posed_joints_host(joint_template, joint_dirs, parents, global_orient, pose, shape, upto: int) -> np.ndarray:
    """Joints 0 .. `upto` of the posed model without translation, (B, upto + 1, 3) in float64 on the host: the rest joints
    ``J_template + J_dirs shape`` carried down the kinematic chain (parents precede their children)."""
    rest = joint_template[None].astype(np.float64) + np.einsum("jck,bk->bjc", joint_dirs.astype(np.float64), shape)
    rot = _rodrigues(np.concatenate([global_orient[:, None, :], pose.reshape(pose.shape[0], -1, 3)], axis=1)[:, :upto + 1])
    G, out = [rot[:, 0]], [rest[:, 0]]
    for j in range(1, upto + 1):
        p = int(parents[j])
        out.append(out[p] + np.einsum("bij,bj->bi", G[p], rest[:, j] - rest[:, p]))
        G.append(G[p] @ rot[:, j])
    return np.stack(out, axis=1)


class MultiViewFitter(FitterBase):
    """Per-frame optimizer against the 2D keypoints of several calibrated cameras, executed on one MI355X."""

    def __init__(self, smpl_model, step_size=1e-2, num_iters=100, use_lbfgs=False, joints_category="AMASS", device=None,
                 pose_prior_num_gaussians=8, pose_prior: Optional[MaxMixturePrior] = None,
                 num_iters_followup=FrameOptimizeConfig.num_iters_followup):
        if use_lbfgs:
            raise NotImplementedError("MultiViewFitter runs Adam only: the device L-BFGS entries refuse the projected joint term; "
                                      "pass use_lbfgs=False")
        super().__init__(smpl_model, step_size, use_lbfgs, joints_category, device, pose_prior_num_gaussians, pose_prior)
        if self.smpl.num_joints not in (24, 52, 55):
            raise NotImplementedError(f"a body model with {self.smpl.num_joints} joints: the fit kernels are built for 24, 52 and 55")
        self.num_iters = num_iters
        self.num_iters_followup = num_iters_followup      # iterations of a video's frames after its first (fit_sequences)
        self._joint_basis = None

    def stage_configs(self, seq_ind=0, sigma=100.0, joint_loss_weight=1.0, pose_preserve_weight=5.0, freeze_betas=True):
        """Kernel configurations of the two stages, ``(cfg1, cfg2, fit_betas)`` (module docstring).  ``cfg.focal`` stays as it
        is: every camera carries its own."""
        cfg1 = stage1_config(self.num_iters, self.step_size, 0.0)
        cfg2, fit_betas = stage2_config(self.num_iters, self.step_size, seq_ind, joint_loss_weight, pose_preserve_weight, freeze_betas,
                                        float(sigma))
        for cfg in (cfg1, cfg2):
            cfg.projection = 1
            self._packed_config(cfg)
        return cfg1, cfg2, fit_betas

    def _check_kinematic(self, model_idx) -> None:
        if any(int(j) >= self.smpl.num_joints for j in model_idx):
            raise NotImplementedError(f"the multi-view term takes kinematic targets only (model indices below {self.smpl.num_joints}): "
                                      "no surface targets (vertex-selected joints, landmarks)")

    def _start_torso(self, go, bp, be) -> np.ndarray:
        """The four torso joints of the start pose, (B, 4, 3) float64, by the host forward."""
        if self._joint_basis is None:
            self._joint_basis = self.smpl.native.joint_basis()
        jt, jd = self._joint_basis
        host = lambda x: x.detach().cpu().numpy().astype(np.float64)
        joints = posed_joints_host(jt, jd, self.smpl.parents.numpy(), host(go), host(bp), host(be), max(TORSO_IDX))
        return joints[:, TORSO_IDX]

    def _fit_views(self, cfg, table, idx, targets, conf, params):
        if conf is not None:
            cfg.conf_per_frame = int(conf.dim() == 3)
        return native.fit_multiview(self.smpl.native, self.pose_prior.native, cfg, table, idx, targets, conf, params["global_orient"],
                                    params["body_pose"], params["betas"], params["transl"])

    def fit_batch(self, init_params: SMPLData, keypoints2d, cameras: Sequence, conf=None, seq_ind: int = 0, target_model_indices=None,
                  sigma: float = 100.0, joint_loss_weight: float = 1.0, pose_preserve_weight: float = 5.0, freeze_betas: bool = True,
                  per_frame_conf: bool = False, want_vertices: bool = True, run_forward: bool = True):
        """Both stages for B independent frames: ``(params dict of (B, .) tensors - ``transl`` = the world translation -,
        joints, vertices, per-frame loss)``.  `keypoints2d` (B, C, K, 2) in pixels, per view in the order of this fitter's joint
        category or of `target_model_indices`; `cameras` C objects with ``rotation``, ``translation``, ``focal``,
        ``principal_point``; `conf` (C, K) or, with `per_frame_conf`, (B, C, K)."""
        table, model_idx, targets_d, cf_d, torso_tgt, torso_on, (go, bp, be), transl0 = self._prepare(
            init_params, keypoints2d, None, cameras, conf, target_model_indices, per_frame_conf)
        cfg1, cfg2, _ = self.stage_configs(seq_ind, sigma, joint_loss_weight, pose_preserve_weight, freeze_betas)
        s1 = self._fit_views(cfg1, table, TORSO_IDX, torso_tgt, torso_on, dict(global_orient=go, body_pose=bp, betas=be, transl=transl0))
        s2 = self._fit_views(cfg2, table, model_idx, targets_d, cf_d, s1)
        out = {k: s2[k] for k in native.PARAM_KEYS}
        # the loss at the result: stage 2's terms without the preserve term, one evaluate-only launch
        cfg2.num_iters, cfg2.step_size, cfg2.pose_preserve_weight = 1, 0.0, 0.0
        out["loss"] = self._fit_views(cfg2, table, model_idx, targets_d, cf_d, out)["loss"]
        self.last_init_transl = transl0
        return self._result(out, run_forward, want_vertices)

    def _prepare(self, init_params, keypoints2d, first_rows, cameras, conf, target_model_indices, per_frame_conf):
        """What both stages read: ``(camera table, model joint per target, centred targets, confidences, stage 1's torso targets
        and which of them are seen, start rows, triangulated initial translation)``, everything before the first device call.
        `first_rows` (None: every frame) names the frames the start rows belong to: a video's first frames, which alone get an
        initial translation and stage 1."""
        R, t, focal, pp = camera_arrays(cameras)
        kp = keypoints2d.detach().cpu().numpy() if isinstance(keypoints2d, torch.Tensor) else np.asarray(keypoints2d)
        if kp.ndim != 4 or kp.shape[1] != len(R) or kp.shape[3] != 2:
            raise ValueError(f"keypoints2d must be (B, {len(R)}, K, 2) for {len(R)} cameras, got {tuple(kp.shape)}")
        B, C, K = kp.shape[:3]
        targets = np.stack([centred_keypoints(kp[:, c], pp[c]) for c in range(C)], axis=1)                  # (B, C, K, 3) float32
        model_idx, rows = self._target_selection(target_model_indices, K)
        if target_model_indices is not None and len(model_idx) != K:
            raise ValueError("target_model_indices must have one entry per keypoint")
        cf = None
        if conf is not None:
            cf = np.asarray(conf.detach().cpu().numpy() if isinstance(conf, torch.Tensor) else conf, dtype=np.float32)
            if cf.shape != ((B, C, K) if per_frame_conf else (C, K)):
                raise ValueError(f"conf must be {(B, C, K) if per_frame_conf else (C, K)}, got {tuple(cf.shape)}")
        if rows is not None:
            targets = targets[:, :, rows]
            cf = None if cf is None else cf[..., rows]
        if any(int(j) < 0 for j in model_idx):
            raise ValueError("target_model_indices must not be negative")
        self._check_kinematic(model_idx)
        check_torso_targets(model_idx)
        torso_cols = [model_idx.index(j) for j in TORSO_IDX]

        # initial translation: the triangulated torso against the model's (host, float64)
        firsts = targets if first_rows is None else targets[np.asarray(first_rows, dtype=np.int64)]
        torso_uv = firsts[:, :, torso_cols, :2].astype(np.float64)
        torso_cf = None if cf is None else cf[..., torso_cols]
        if torso_cf is not None and first_rows is not None and per_frame_conf:
            torso_cf = torso_cf[np.asarray(first_rows, dtype=np.int64)]
        n_first = firsts.shape[0]                                     # the frames that get a start: all, or the videos' first
        usable = np.ones((n_first, C, 4), dtype=bool) if torso_cf is None else np.broadcast_to(torso_cf != 0, (n_first, C, 4))
        world = triangulate_dlt(torso_uv, usable, R, t, focal)
        go, bp, be = self._start_rows(init_params)
        if not all(s.shape[0] == n_first for s in (go, bp, be)):
            raise ValueError("init_params and keypoints2d disagree on the number of frames")
        mean4 = lambda a: (a[:, 0] + a[:, 1] + a[:, 2] + a[:, 3]) / 4.0
        transl0 = torch.from_numpy((mean4(world) - mean4(self._start_torso(go, bp, be))).astype(np.float32)).to(self.device)

        table = native.camera_table(list(zip(R, t, focal)))
        dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
        targets_d, cf_d = dev(targets), dev(cf)
        torso_tgt = dev(firsts[:, :, torso_cols])
        torso_on = None if torso_cf is None else dev((torso_cf != 0).astype(np.float32))                    # seen: 1, not seen: out
        return table, model_idx, targets_d, cf_d, torso_tgt, torso_on, (go, bp, be), transl0

    def fit_sequences(self, init_params: SMPLData, keypoints2d, lengths, cameras: Sequence, conf=None, target_model_indices=None,
                      sigma: float = 100.0, joint_loss_weight: float = 1.0, pose_preserve_weight: float = 5.0, freeze_betas: bool = True,
                      want_vertices: bool = True, run_forward: bool = True):
        """S videos of one rig as warm-start chains: `init_params` one start row per video, `keypoints2d` packed (sum T, C, K, 2)
        pixels, `lengths` (S,) frames per video (0: an empty one, whose start row is not read), `cameras` the rig shared by all
        videos and frames, `conf` None, (C, K) or one table per frame (sum T, C, K).  Two fit launches whatever S and T: the
        triangulated translation of the S first frames and stage 1 over them exactly as ``fit_batch`` runs it, then ONE
        ``k2b_fit_multiview_sequences`` launch under stage 2's configuration of ``stage_configs(seq_ind=0)``: a video's first
        frame gets ``num_iters`` iterations and no preserve term (so its parameters equal ``fit_batch``'s on that frame alone),
        every later frame starts from its predecessor's result, preserves that result's body pose with `pose_preserve_weight`,
        runs ``num_iters_followup`` iterations with a fresh optimiser and, with `freeze_betas`, holds the shape (SMPL-H / SMPL-X:
        the betas; the expression stays free).

        Returns ``fit_batch``'s ``(params, joints, vertices, loss)`` over the sum T packed rows.  ``loss`` is the chain's own: a
        frame's loss at its LAST iteration, before that iteration's step, preserve term included - the convention of the other
        chains - and not ``fit_frame``'s loss re-evaluated at the result."""
        L = np.asarray(lengths, dtype=np.int64).reshape(-1)
        if (L < 0).any():
            raise ValueError("lengths must not be negative")
        n = int(np.shape(keypoints2d)[0])
        if int(L.sum()) != n:
            raise ValueError(f"lengths sum to {int(L.sum())}, keypoints2d has {n} frames")
        live = np.flatnonzero(L > 0)
        offsets = np.concatenate(([0], np.cumsum(L)[:-1])) if L.size else L
        per_frame = conf is not None and torch.as_tensor(conf).dim() == 3
        if live.size == 0:                                            # no frame at all: zero rows of the right widths
            camera_arrays(cameras)
            return self._result(native._fit_outputs(self.smpl.native, (0,)), run_forward, want_vertices)
        table, model_idx, targets_d, cf_d, torso_tgt, torso_on, (go, bp, be), transl0 = self._prepare(
            select_rows(init_params, live, L.size), keypoints2d, offsets[live], cameras, conf, target_model_indices, per_frame)
        cfg1, cfg2, _ = self.stage_configs(0, sigma, joint_loss_weight, pose_preserve_weight, freeze_betas)
        cfg2.pose_preserve_weight = float(pose_preserve_weight)       # (the chain leaves it out of a video's first frame itself)
        cfg2.conf_per_frame = int(per_frame)
        s1 = self._fit_views(cfg1, table, TORSO_IDX, torso_tgt, torso_on, dict(global_orient=go, body_pose=bp, betas=be, transl=transl0))
        out = native.fit_multiview_sequences(self.smpl.native, self.pose_prior.native, cfg2, int(self.num_iters_followup), bool(freeze_betas),
                                             table, model_idx, L[live], targets_d, cf_d, s1["global_orient"], s1["body_pose"], s1["betas"],
                                             s1["transl"])
        self.last_init_transl = transl0
        return self._result(out, run_forward, want_vertices)

    def final_forward(self, out, want_vertices=True):
        """World-space joints / vertices: the translation applied, as the world fitter returns them."""
        return self.smpl.native.lbs(out["global_orient"], out["body_pose"], out["betas"], out["transl"], want_vertices=want_vertices)

    def fit_frame(self, init_params: SMPLData, keypoints2d, cameras: Sequence, conf=None, seq_ind: int = 0, target_model_indices=None,
                  sigma: float = 100.0, joint_loss_weight: float = 1.0, pose_preserve_weight: float = 5.0,
                  freeze_betas: bool = True) -> BodyModelFitResult:
        """One frame: `keypoints2d` (C, K, 2), `conf` (C, K)."""
        kp = keypoints2d.detach().cpu().numpy() if isinstance(keypoints2d, torch.Tensor) else np.asarray(keypoints2d)
        return self._frame_result(self.fit_batch(init_params, kp[None], cameras, conf, seq_ind, target_model_indices, sigma,
                                                 joint_loss_weight, pose_preserve_weight, freeze_betas), init_params)
