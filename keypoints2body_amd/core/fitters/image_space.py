"""Image-space two-stage fitter on the HIP engine: SMPL / SMPL-H / SMPL-X fitted to 2D keypoints under a pinhole camera.

The reference has no such path (``keypoints2body/api/frame.py:71-75`` raises for ``joints2d``), so this fitter is DEFINED here
and pinned to a float64 oracle of its own formulas (``tests/reproj_common.py``), not to reference outputs.  It is modelled on
``CameraSpaceFitter``: two launches of the fused fit kernels for a batch of independent frames, with the joint term in its
projected form (``k2b_fit_config.projection = 1``, ``include/k2b.h``):

    e = (fx X / Z - (u - cx), fy Y / Z - (v - cy)),   (X, Y, Z) = joint + camera translation,
    loss = w_j^2 sum_k c_k^2 (gmof(e_x, sigma) + gmof(e_y, sigma)) + the priors of the 3D fit,      sigma in pixels.

The principal point never reaches the kernel: it is subtracted from the keypoints here, in float64, before they are rounded
to float32 (a pixel coordinate is a few hundred times its residual; DESIGN.md 4.4d has the figures).

* initial translation, by similar triangles over the four torso joints (``TORSO_JOINTS``) of the start pose, one joints-only
  forward as in ``guess_init_3d``: ``t_z`` = (mean 3D length of the torso's four edges) / (mean length of the same edges between
  the detections, in normalised image coordinates ``(u' / fx, v' / fy)``), and ``t_xy`` puts the torso's centroid on the detected
  centroid at that depth;
* stage 1: ``[global_orient, camera translation]`` (``optimize_mask = 9``) against the torso joints with a plain squared pixel
  error (GMoF with sigma -> inf, weight 1), every pose / shape prior off.  On 24-joint models the depth prior
  ``depth_weight^2 |t - t0|^2`` pulls toward the initial translation; the tree kernel of SMPL-H / SMPL-X has no translation
  prior (its entry refuses one), so those models run stage 1 WITHOUT it;
* stage 2: all targets, all priors, ``sigma`` (default 100 px) and ``joint_loss_weight`` (default 1: pixel residuals are two
  orders above metric ones); betas are optimised iff ``seq_ind == 0 or not freeze_betas``, as the camera fitter does;
* result: ``transl`` = the camera translation, model-space joints / vertices from the usual final forward (no translation
  applied), ``loss`` = stage 2's loss re-evaluated at the result without the preserve term (one evaluate-only launch).

Videos (``fit_sequences``): S ragged sequences of keypoints as warm-start chains - stage 1 for the S first frames as one launch,
then the whole of stage 2 for every frame of every sequence as ONE launch (``k2b_fit_image_sequences``): a sequence's first frame
is stage 2 as above, every later frame starts from its predecessor's result, preserves that result's body pose and, with
``freeze_betas``, holds the shape the first frame estimated.

Surface targets (model index at or above the joint count: smplx's vertex-selected joints - nose, eyes, ears, toes, heels,
fingertips - and its barycentric face landmarks) are projected like the joints (``k2b_fit_image``, ``include/k2b.h``): stage 2
and the loss re-evaluation then go through that entry, two launches per iteration, and a video runs its chain as queued steps
in lockstep (``fit_sequences``), since the one-launch chain takes kinematic targets only.  Stage 1 is the torso's, kinematic.

Adam only: the device L-BFGS entries refuse the projected term (``K2B_ERR_UNSUPPORTED``), so ``use_lbfgs=True`` raises.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from ... import native
from ...models.smpl_data import BodyModelFitResult, SMPLData, select_rows
from ...prior import MaxMixturePrior
from ..config import FrameOptimizeConfig
from ..constants import TORSO_JOINTS
from .common import TORSO_IDX, FitterBase, stage1_config, stage2_config

_TORSO_EDGES = ((0, 1), (2, 3), (0, 2), (1, 3))             # hips, shoulders, right side, left side (positions in TORSO_IDX)


def centred_keypoints(keypoints2d, principal_point) -> np.ndarray:
    """(B, K, 2) pixel coordinates -> float32 target rows (B, K, 3) = (u - cx, v - cy, 0); the subtraction in float64."""
    kp = keypoints2d.detach().cpu().numpy() if isinstance(keypoints2d, torch.Tensor) else np.asarray(keypoints2d)
    if kp.ndim != 3 or kp.shape[2] != 2:
        raise ValueError(f"keypoints2d must be (B,K,2), got {tuple(kp.shape)}")
    pp = np.asarray(principal_point, dtype=np.float64).reshape(-1)
    if pp.shape != (2,) or not np.isfinite(pp).all():
        raise ValueError("principal_point must be two finite numbers (cx, cy)")
    out = np.zeros(kp.shape[:2] + (3,), dtype=np.float32)
    out[..., :2] = kp.astype(np.float64) - pp
    return out


def focal_pair(focal) -> tuple:
    f = np.asarray(focal, dtype=np.float64).reshape(-1)
    if f.shape == (1,):
        f = np.repeat(f, 2)
    if f.shape != (2,) or not (np.isfinite(f).all() and (f > 0).all()):
        raise ValueError("focal must be a positive finite number or a pair (fx, fy)")
    return float(f[0]), float(f[1])


def check_torso_targets(model_idx) -> None:
    """Raise ``ValueError`` unless all four torso joints are among the targets (no device call)."""
    have = {int(j) for j in model_idx}
    missing = [TORSO_JOINTS[i] for i, j in enumerate(TORSO_IDX) if j not in have]
    if missing:
        raise ValueError(f"the torso joints {missing} are not among the targets: the initial translation and stage 1 need all four")


def guess_init_2d(model_joints: torch.Tensor, torso_uv: torch.Tensor, focal: tuple, torso_index: torch.Tensor) -> torch.Tensor:
    """Initial camera translation (B, 3) by similar triangles: `model_joints` (B, J, 3) of the start pose without translation,
    `torso_uv` (B, 4, >=2) the centred detections of ``TORSO_JOINTS`` in that order."""
    p = model_joints.index_select(1, torso_index)
    n = torso_uv[..., :2] / torch.tensor(focal, dtype=torso_uv.dtype, device=torso_uv.device)           # normalised image coordinates
    a, b = [e[0] for e in _TORSO_EDGES], [e[1] for e in _TORSO_EDGES]
    len3 = (p[:, a] - p[:, b]).norm(dim=-1).mean(dim=1)
    len2 = (n[:, a] - n[:, b]).norm(dim=-1).mean(dim=1)
    depth = len3 / len2
    c3, c2 = p.mean(dim=1), n.mean(dim=1)
    return torch.stack([c2[:, 0] * depth - c3[:, 0], c2[:, 1] * depth - c3[:, 1], depth - c3[:, 2]], dim=1)


class ImageSpaceFitter(FitterBase):
    """Per-frame optimizer against 2D keypoints under a pinhole camera, executed on one MI355X."""

    def __init__(self, smpl_model, step_size=1e-2, num_iters=100, use_lbfgs=False, joints_category="AMASS", device=None,
                 pose_prior_num_gaussians=8, pose_prior: Optional[MaxMixturePrior] = None,
                 num_iters_followup=FrameOptimizeConfig.num_iters_followup):
        if use_lbfgs:
            raise NotImplementedError("ImageSpaceFitter runs Adam only: the device L-BFGS entries (k2b_fit_world_lbfgs and the "
                                      "sequence entries) refuse the projected joint term; pass use_lbfgs=False")
        super().__init__(smpl_model, step_size, use_lbfgs, joints_category, device, pose_prior_num_gaussians, pose_prior)
        if self.smpl.num_joints not in (24, 52, 55):
            raise NotImplementedError(f"a body model with {self.smpl.num_joints} joints: the fit kernels are built for 24, 52 and 55")
        self.num_iters = num_iters
        self.num_iters_followup = num_iters_followup      # iterations of a video's frames after its first (fit_sequences)

    def stage_configs(self, focal, seq_ind=0, sigma=100.0, joint_loss_weight=1.0, pose_preserve_weight=5.0, freeze_betas=True,
                      depth_weight=100.0):
        """Kernel configurations of the two stages, ``(cfg1, cfg2, fit_betas)`` (module docstring)."""
        fx, fy = focal_pair(focal)
        tree = self.smpl.num_joints != 24 or self.smpl.packed          # (no translation prior in the tree kernel)
        cfg1 = stage1_config(self.num_iters, self.step_size, 0.0 if tree else depth_weight)
        cfg2, fit_betas = stage2_config(self.num_iters, self.step_size, seq_ind, joint_loss_weight, pose_preserve_weight, freeze_betas,
                                        float(sigma))
        for cfg in (cfg1, cfg2):
            cfg.projection, cfg.focal[0], cfg.focal[1] = 1, fx, fy
            self._packed_config(cfg)
        return cfg1, cfg2, fit_betas

    def _has_surface_targets(self, model_idx) -> bool:
        return any(int(j) >= self.smpl.num_joints for j in model_idx)

    def _fit_image(self, cfg, idx, targets, conf, params):
        """Stage 2's call: ``native.fit_image`` with surface targets among `idx`, else ``_fit`` (the same bits as ever)."""
        if not self._has_surface_targets(idx):
            return self._fit(cfg, idx, targets, conf, params)
        if conf is not None:
            cfg.conf_per_frame = int(conf.dim() == 2)
        return native.fit_image(self.smpl.native, self.pose_prior.native, cfg, idx, targets, conf, params["global_orient"],
                                params["body_pose"], params["betas"], params["transl"])

    def _prepare(self, init_params, keypoints2d, first_rows, focal, principal_point, conf, target_model_indices, per_frame_conf,
                 init_cam_t):
        """What both stages read: ``(fx, fy, centred targets, confidences, model joint per target, stage 1's torso targets, start
        rows, initial camera translation)``.  `first_rows` (None: every frame) names the frames the start rows belong to: a
        video's first frames, which alone get an initial translation and stage 1."""
        fx, fy = focal_pair(focal)
        targets = torch.from_numpy(centred_keypoints(keypoints2d, principal_point))
        B = targets.shape[0] if first_rows is None else len(first_rows)
        go, bp, be = self._start_rows(init_params)
        model_idx, targets, cf = self._targets_and_conf(targets, target_model_indices, conf, per_frame_conf, (go, bp, be), B,
                                                        names=("keypoints2d", "keypoint"))

        # stage 1's targets: the four torso joints among the detections
        check_torso_targets(model_idx)
        torso_cols = torch.tensor([model_idx.index(j) for j in TORSO_IDX], dtype=torch.int64, device=self.device)
        firsts = targets if first_rows is None else targets.index_select(
            0, torch.as_tensor(np.asarray(first_rows, dtype=np.int64), device=self.device))
        torso_tgt = firsts.index_select(1, torso_cols).contiguous()
        if init_cam_t is None:
            joints0 = self.smpl.native.lbs(go, bp, be, None, want_vertices=False)[0]
            cam_t0 = guess_init_2d(joints0, torso_tgt, (fx, fy), torch.tensor(TORSO_IDX, dtype=torch.int64, device=self.device))
        else:
            cam_t0 = self._dev(init_cam_t, 3)
        return fx, fy, targets, cf, model_idx, torso_tgt, (go, bp, be), cam_t0.detach().contiguous()

    def fit_batch(self, init_params: SMPLData, keypoints2d, focal, principal_point=(0.0, 0.0), conf=None, seq_ind: int = 0,
                  target_model_indices=None, sigma: float = 100.0, joint_loss_weight: float = 1.0,
                  pose_preserve_weight: float = 5.0, freeze_betas: bool = True, depth_weight: float = 100.0,
                  init_cam_t=None, per_frame_conf: bool = False, want_vertices: bool = True, run_forward: bool = True):
        """Both stages for B independent frames: ``(params dict of (B, .) tensors - ``transl`` = the camera translation -,
        joints, vertices, per-frame loss)``.  `keypoints2d` (B, K, 2) in pixels, in the order of this fitter's joint category
        or of `target_model_indices`; `focal` a number or ``(fx, fy)``; `conf` (K,) or, with `per_frame_conf`, (B, K)."""
        fx, fy, targets, cf, model_idx, torso_tgt, (go, bp, be), cam_t0 = self._prepare(
            init_params, keypoints2d, None, focal, principal_point, conf, target_model_indices, per_frame_conf, init_cam_t)

        cfg1, cfg2, _ = self.stage_configs((fx, fy), seq_ind, sigma, joint_loss_weight, pose_preserve_weight, freeze_betas, depth_weight)
        prior_target = cam_t0 if cfg1.transl_prior_weight != 0.0 else None
        s1 = self._fit(cfg1, TORSO_IDX, torso_tgt, None, dict(global_orient=go, body_pose=bp, betas=be, transl=cam_t0),
                       transl_prior_target=prior_target)
        s2 = self._fit_image(cfg2, model_idx, targets, cf, s1)
        out = {k: s2[k] for k in native.PARAM_KEYS}
        # the loss at the result: stage 2's terms without the preserve term, one evaluate-only launch
        cfg2.num_iters, cfg2.step_size, cfg2.pose_preserve_weight = 1, 0.0, 0.0
        out["loss"] = self._fit_image(cfg2, model_idx, targets, cf, out)["loss"]
        self.last_init_cam_t = cam_t0
        return self._result(out, run_forward, want_vertices)

    def fit_sequences(self, init_params: SMPLData, keypoints2d, lengths, focal, principal_point=(0.0, 0.0), conf=None,
                      target_model_indices=None, sigma: float = 100.0, joint_loss_weight: float = 1.0,
                      pose_preserve_weight: float = 5.0, freeze_betas: bool = True, depth_weight: float = 100.0,
                      want_vertices: bool = True, run_forward: bool = True, _one_launch=None):
        """S videos as warm-start chains: `init_params` one start row per sequence, `keypoints2d` packed (sum T, K, 2) pixels,
        `lengths` (S,) frames per sequence (0: an empty sequence, whose start row is not read), `conf` None, (K,) or one row per
        frame (sum T, K).  Three fit launches whatever S and T: the initial translation of the S first frames by ``guess_init_2d``
        and stage 1 over them exactly as ``fit_batch`` runs it, then ONE ``k2b_fit_image_sequences`` launch under stage 2's
        configuration of ``stage_configs(seq_ind=0)``: a sequence's first frame gets ``num_iters`` iterations and no preserve
        term (so it equals ``fit_batch`` on that frame alone), every later frame starts from its predecessor's result, preserves
        that result's body pose with `pose_preserve_weight`, runs ``num_iters_followup`` iterations with a fresh optimiser and,
        with `freeze_betas`, holds the shape (SMPL-H / SMPL-X: the betas; the expression stays free).

        With surface targets (which the one-launch chain refuses) the same chain runs as queued steps in lockstep
        (``_lockstep_chain``): step t is one ``k2b_fit_image`` call over the sequences that have a frame t, nothing comes back
        to the host between steps.  ``_one_launch=False`` forces that route for kinematic targets as well (tests).

        Returns ``fit_batch``'s ``(params, joints, vertices, loss)`` over the sum T packed rows.  ``loss`` is the chain's own: a
        frame's loss at its LAST iteration, before that iteration's step, preserve term included - the convention of the 3D
        chains - and not ``fit_frame``'s loss re-evaluated at the result without the preserve term."""
        L = np.asarray(lengths, dtype=np.int64).reshape(-1)
        if (L < 0).any():
            raise ValueError("lengths must not be negative")
        n = int(keypoints2d.shape[0])
        if int(L.sum()) != n:
            raise ValueError(f"lengths sum to {int(L.sum())}, keypoints2d has {n} frames")
        live = np.flatnonzero(L > 0)
        offsets = np.concatenate(([0], np.cumsum(L)[:-1])) if L.size else L
        if conf is not None and torch.as_tensor(conf).dim() == 2 and torch.as_tensor(conf).shape[0] != n:
            raise ValueError("conf must be (K,) or one row per frame")
        if live.size == 0:                                            # no frame at all: zero rows of the right widths
            return self._result(native._fit_outputs(self.smpl.native, (0,)), run_forward, want_vertices)
        fx, fy, targets, cf, model_idx, torso_tgt, (go, bp, be), cam_t0 = self._prepare(
            select_rows(init_params, live, L.size), keypoints2d, offsets[live], focal, principal_point, conf, target_model_indices,
            True, None)
        cfg1, cfg2, _ = self.stage_configs((fx, fy), 0, sigma, joint_loss_weight, pose_preserve_weight, freeze_betas, depth_weight)
        cfg2.pose_preserve_weight = float(pose_preserve_weight)       # (the chain leaves it out of a sequence's first frame itself)
        cfg2.conf_per_frame = int(cf is not None and cf.dim() == 2)
        s1 = self._fit(cfg1, TORSO_IDX, torso_tgt, None, dict(global_orient=go, body_pose=bp, betas=be, transl=cam_t0),
                       transl_prior_target=cam_t0 if cfg1.transl_prior_weight != 0.0 else None)
        one_launch = not self._has_surface_targets(model_idx) if _one_launch is None else bool(_one_launch)
        if one_launch:
            out = native.fit_image_sequences(self.smpl.native, self.pose_prior.native, cfg2, int(self.num_iters_followup), bool(freeze_betas),
                                             model_idx, L[live], targets, cf, s1["global_orient"], s1["body_pose"], s1["betas"], s1["transl"])
        else:
            out = self._lockstep_chain(cfg2, bool(freeze_betas), model_idx, L[live], targets, cf, s1)
        self.last_init_cam_t = cam_t0
        return self._result(out, run_forward, want_vertices)

    def _lockstep_chain(self, cfg2, freeze_betas, model_idx, lengths, targets, cf, s1):
        """``k2b_fit_image_sequences``' chain as queued steps: `lengths` (S,) > 0 frames per sequence over the packed rows of
        `targets` / `cf`, `s1` the S starts.  Step 0 runs `cfg2` without the preserve term; step t > 0 runs over the sequences
        longer than t, each from its row of step t - 1 (whose body pose the preserve term holds: the entry's default),
        ``num_iters_followup`` iterations, a fresh optimiser and, with `freeze_betas`, the shape held.  The row indices of every
        step are uploaded before the first launch; the host reads nothing back in between."""
        lengths = np.asarray(lengths, dtype=np.int64)
        offsets = np.concatenate(([0], np.cumsum(lengths)[:-1]))
        index = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.int64), device=self.device)
        steps, prev_live = [], np.arange(lengths.size)
        for t in range(int(lengths.max())):
            live = np.flatnonzero(lengths > t)
            # (rows of this step in the packed arrays; positions of its sequences among the previous step's)
            steps.append((index(offsets[live] + t), index(np.searchsorted(prev_live, live))))
            prev_live = live
        out = native._fit_outputs(self.smpl.native, (int(lengths.sum()),))
        per_frame = cf is not None and cf.dim() == 2
        first = native.FitConfigC.from_buffer_copy(cfg2)
        first.pose_preserve_weight = 0.0
        follow = native.FitConfigC.from_buffer_copy(cfg2)
        follow.num_iters = int(self.num_iters_followup)
        if freeze_betas:
            follow.freeze_betas = 1
        prev = s1
        for t, (rows, among_prev) in enumerate(steps):
            start = prev if t == 0 else {k: prev[k].index_select(0, among_prev) for k in native.PARAM_KEYS}
            prev = self._fit_image(first if t == 0 else follow, model_idx, targets.index_select(0, rows),
                                   cf.index_select(0, rows) if per_frame else cf, start)
            for k in out:
                out[k].index_copy_(0, rows, prev[k])
        return out

    def final_forward(self, out, want_vertices=True):
        """Model-space joints / vertices: the camera translation is part of the parameters, not applied to the mesh."""
        return self.smpl.native.lbs(out["global_orient"], out["body_pose"], out["betas"], None, want_vertices=want_vertices)

    def fit_frame(self, init_params: SMPLData, keypoints2d, focal, principal_point=(0.0, 0.0), conf=None, seq_ind: int = 0,
                  target_model_indices=None, sigma: float = 100.0, joint_loss_weight: float = 1.0,
                  pose_preserve_weight: float = 5.0, freeze_betas: bool = True, depth_weight: float = 100.0,
                  init_cam_t=None) -> BodyModelFitResult:
        return self._frame_result(self.fit_batch(init_params, keypoints2d, focal, principal_point, conf, seq_ind, target_model_indices,
                                                 sigma, joint_loss_weight, pose_preserve_weight, freeze_betas, depth_weight, init_cam_t),
                                  init_params)
