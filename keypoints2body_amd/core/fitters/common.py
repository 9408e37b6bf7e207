"""What the world-space, the camera-space and the image-space fitter share: construction, the kernel layout of starts and
results, argument handling, the one call into ``native.fit_world``, the stage configurations of the two-stage fitters, the
result tail and the host-driven ``torch.optim.LBFGS`` twin of the device optimiser."""
from __future__ import annotations

from typing import Optional

import torch

from ... import native
from ...models.body_model import BodyModel, as_body_model, check_target_indices
from ...models.smpl_data import BodyModelFitResult, SMPLData, SMPLHData, SMPLXData
from ...prior import MaxMixturePrior
from ..constants import JOINT_MAP, TORSO_JOINTS, category_indices

TORSO_IDX = [JOINT_MAP[name] for name in TORSO_JOINTS]      # RHip, LHip, RShoulder, LShoulder: the same in every SMPL-family tree
SQUARED_ERROR_SIGMA = 1.0e8                                 # gmof(e, sigma) -> e^2 in fp32


def stage1_config(num_iters, step_size, depth_weight):
    """Stage 1 of the two-stage fitters (reference ``camera_space.py:137-213``): ``[global_orient, camera_translation]``
    (``optimize_mask = 9``), plain squared error on the stage's joints (GMoF sigma -> inf, weight 1), the depth prior
    ``depth_weight^2 |t - t0|^2``, every other prior off."""
    cfg = native.default_fit_config()
    cfg.num_iters, cfg.step_size = int(num_iters), float(step_size)
    cfg.sigma, cfg.joint_loss_weight = SQUARED_ERROR_SIGMA, 1.0
    cfg.pose_prior_weight = cfg.angle_prior_weight = cfg.shape_prior_weight = cfg.pose_preserve_weight = 0.0
    cfg.optimize_mask, cfg.transl_prior_weight = 9, float(depth_weight)
    return cfg


def stage2_config(num_iters, step_size, seq_ind, joint_loss_weight, pose_preserve_weight, freeze_betas, sigma=None):
    """Stage 2 (``camera_space.py:215-298``), ``(cfg, fit_betas)``: all terms of the 3D fit (`sigma` None: the default GMoF
    scale), the preserve term from the second frame on, betas optimised iff ``seq_ind == 0 or not freeze_betas``."""
    cfg = native.default_fit_config()
    cfg.num_iters, cfg.step_size = int(num_iters), float(step_size)
    if sigma is not None:
        cfg.sigma = float(sigma)
    cfg.joint_loss_weight = float(joint_loss_weight)
    cfg.pose_preserve_weight = float(pose_preserve_weight) if seq_ind > 0 else 0.0
    fit_betas = seq_ind == 0 or not freeze_betas
    cfg.optimize_mask = 15 if fit_betas else 11
    return cfg, fit_betas


class FitterBase:
    """Model, device, joint category and prior of a fitter."""

    # "device": the optimiser on the GPU; or one of the host-driven twins the subclass names.  A class-level default, so that
    # both ``fitter.lbfgs_driver = ...`` and ``WorldSpaceFitter.lbfgs_driver = ...`` (tools/dev_lbfgs_seq_timing.py) select one
    lbfgs_driver = "device"
    # whether ``_start_rows`` puts the starts of a packed (SMPL-H / SMPL-X) model into kernel layout
    pack_starts = True

    def __init__(self, smpl_model, step_size, use_lbfgs, joints_category, device, pose_prior_num_gaussians, pose_prior):
        self.smpl: BodyModel = as_body_model(smpl_model, device=device)
        self.device = self.smpl.device
        self.step_size = step_size
        self.use_lbfgs = use_lbfgs
        self.joints_category = joints_category
        self.smpl_index, self.corr_index = category_indices(joints_category)   # raises on unknown category
        # the reference loads ./data/models/gmm_XX.pkl relative to the CWD (world_space.py:87-91)
        self.pose_prior = pose_prior if pose_prior is not None else MaxMixturePrior(
            prior_folder="./data/models/", num_gaussians=pose_prior_num_gaussians, device=self.device)

    def _dev(self, x, cols) -> torch.Tensor:
        t = torch.as_tensor(x, dtype=torch.float32).detach().to(self.device)
        if t.dim() != 2 or t.shape[1] != cols:
            raise ValueError(f"expected a (B,{cols}) tensor, got {tuple(t.shape)}")
        return t.contiguous()

    def _packed_config(self, cfg):
        if self.smpl.packed:
            cfg.prior_pose_dims = 3 * self.smpl.NUM_BODY_JOINTS       # 63: what the mixture, bending and preserve terms see
            cfg.num_betas_prior = self.smpl.num_betas                 # 10: shape prior / freeze_betas leave the expression alone
        return cfg

    def _pack(self, init, B):
        """SMPL-H / SMPL-X starts in kernel layout: one pose vector of all non-root joints, one of all shape coefficients."""
        get = lambda name: getattr(init, name, None)
        return (self.smpl.pack_pose(B, body_pose=init.body_pose, jaw_pose=get("jaw_pose"), leye_pose=get("leye_pose"),
                                    reye_pose=get("reye_pose"), left_hand_pose=get("left_hand_pose"),
                                    right_hand_pose=get("right_hand_pose")),
                self.smpl.pack_shape(B, init.betas, get("expression")))

    def packed_init(self, init):
        """Kernel layout of SMPL-X parameters: ``body_pose`` = all 162 non-root joint values, ``betas`` = betas | expression."""
        body_pose, betas = self._pack(init, init.global_orient.shape[0])
        return SMPLData(global_orient=init.global_orient, transl=init.transl, body_pose=body_pose, betas=betas)

    def _start_rows(self, init_params):
        """``(global_orient, pose, shape)`` of the start on the device, in kernel layout where the fitter packs."""
        go = self._dev(init_params.global_orient, 3)
        if self.pack_starts and self.smpl.packed:         # 52- / 55-joint trees (SMPL-H / SMPL-X)
            bp, be = self._pack(init_params, go.shape[0])
        else:
            bp = self._dev(init_params.body_pose, 3 * (self.smpl.num_joints - 1))
            be = self._dev(init_params.betas, self.smpl.num_betas)
        return go, bp, be

    def _target_selection(self, target_model_indices, num_targets):
        """``(model joint per target, rows)`` of the reference's gather (world_space.py:194-201): the category's lists, or the
        caller's indices over all targets in order.  ``rows`` is None where the targets already are in that order, so that
        the caller skips the gather.  The gather itself stays with each fitter: world mode indexes the input where it
        lies (host inputs are gathered before the upload), camera mode gathers on the device with a cached index
        tensor, together with its stage-1 targets."""
        if target_model_indices is not None:
            return [int(i) for i in torch.as_tensor(target_model_indices).reshape(-1).tolist()], None
        if self.smpl_index is None:
            raise ValueError("joints_category='GENERIC' needs target_model_indices")
        rows = list(self.corr_index)
        return list(self.smpl_index), (None if rows == list(range(num_targets)) else rows)

    def _confidence(self, conf_3d, per_frame_conf, rows=None) -> Optional[torch.Tensor]:
        """Confidences on the device; a 2-D tensor means one row per frame only with `per_frame_conf`, otherwise row 0
        serves all frames (reference quirk, world_space.py:163-164)."""
        if conf_3d is None:
            return None
        conf = torch.as_tensor(conf_3d, dtype=torch.float32)
        if conf.dim() == 2 and not per_frame_conf:
            conf = conf[0]
        if rows is not None:
            conf = conf[..., rows]
        return conf.to(self.device).contiguous()

    def _targets_and_conf(self, targets, target_model_indices, conf, per_frame_conf, starts, num_starts,
                          names=("j3d", "target joint"), check_index=None):
        """``(model joint per target, targets gathered and on the device, confidences)`` for host or device `targets`
        (B, K, 3): the row count of the start tensors `starts`, the joint gather of the reference (world_space.py:194-201) and
        its confidence rules (``:163-164``).  `names`: what the messages call the targets and one of them; `check_index`: a
        fitter's own refusal of a target set, made once the indices are known to be the model's.

        AMASS / SMPL24 inputs arrive in target order: the gather is the identity (on a device tensor it would upload its index
        list per call); host inputs are gathered before the upload."""
        if not all(s.shape[0] == num_starts for s in starts):
            raise ValueError(f"init_params and {names[0]} disagree on the number of frames")
        model_idx, rows = self._target_selection(target_model_indices, targets.shape[1])
        if target_model_indices is not None:
            if len(model_idx) != targets.shape[1]:
                raise ValueError(f"target_model_indices must have one entry per {names[1]}")
            check_target_indices(self.smpl, model_idx)
        if check_index is not None:
            check_index(model_idx)
        targets = (targets if rows is None else targets[:, rows, :]).to(self.device).contiguous()
        return model_idx, targets, self._confidence(conf, per_frame_conf, rows)

    def _fit(self, cfg, idx, targets, conf, params, *, preserve_pose=None, transl_prior_target=None, want_grad=False):
        """The one call into ``native.fit_world``: `params` maps ``native.PARAM_KEYS`` to device tensors in kernel layout;
        a 2-D `conf` is one row per frame (vertex-selected joints among `idx` are handled inside ``k2b_fit_world``)."""
        if conf is not None:
            cfg.conf_per_frame = int(conf.dim() == 2)
        return native.fit_world(self.smpl.native, self.pose_prior.native, cfg, idx, targets, conf, params["global_orient"],
                                params["body_pose"], params["betas"], params["transl"], preserve_pose=preserve_pose,
                                want_grad=want_grad, transl_prior_target=transl_prior_target)

    def _result(self, out, run_forward, want_vertices):
        """``(params, joints, vertices, per-frame loss)``; without `run_forward` the final forward is the caller's."""
        if not run_forward:
            return out, None, None, out["loss"]
        joints, verts = self.final_forward(out, want_vertices=want_vertices)
        return out, joints, verts, out["loss"]

    def _frame_result(self, fit, init_params) -> BodyModelFitResult:
        """``fit_frame``'s result object of ``fit_batch``'s tuple; ``loss`` is the sum over the frames."""
        out, joints, verts, loss = fit
        return BodyModelFitResult(params=self.result_params(out, init_params), vertices=verts, joints=joints, loss=loss.sum())

    def result_params(self, out, init_params, rows: Optional[slice] = None):
        """Fitted parameters as the data class the reference returns for this model / input type; `rows` selects
        frames of a batched result (hand / face fields a 24-joint fit does not touch are carried from `init_params`)."""
        if rows is not None:
            out = {k: v[rows] for k, v in out.items() if k != "loss"}
        if self.smpl.model_type == "smplh" and self.smpl.packed:
            u = self.smpl.unpack(out["body_pose"], out["betas"])
            return SMPLHData(betas=u["betas"], global_orient=out["global_orient"], body_pose=u["body_pose"], transl=out["transl"],
                             left_hand_pose=u["left_hand_pose"], right_hand_pose=u["right_hand_pose"])
        if self.smpl.model_type == "smplx":
            u = self.smpl.unpack(out["body_pose"], out["betas"])
            return SMPLXData(betas=u["betas"], global_orient=out["global_orient"], body_pose=u["body_pose"],
                             transl=out["transl"], left_hand_pose=u["left_hand_pose"], right_hand_pose=u["right_hand_pose"],
                             expression=u["expression"], jaw_pose=u["jaw_pose"], leye_pose=u["leye_pose"],
                             reye_pose=u["reye_pose"])
        fields = dict(betas=out["betas"], global_orient=out["global_orient"], body_pose=out["body_pose"],
                      transl=out["transl"])
        if isinstance(init_params, SMPLXData):
            keep = ("left_hand_pose", "right_hand_pose", "expression", "jaw_pose", "leye_pose", "reye_pose")
            return SMPLXData(**fields, **{k: _detached(getattr(init_params, k)) for k in keep})
        if isinstance(init_params, SMPLHData):
            keep = ("left_hand_pose", "right_hand_pose")
            return SMPLHData(**fields, **{k: _detached(getattr(init_params, k)) for k in keep})
        return SMPLData(**fields)


def _detached(x):
    return x.detach() if isinstance(x, torch.Tensor) else x


def upload_params(p, cols, device):
    """Host rows `p` (by ``native.PARAM_KEYS``) as ONE upload of the packed row, split into the four contiguous device
    tensors a fit call takes."""
    return split_params(torch.cat([p[k].detach() for k in native.PARAM_KEYS], dim=1).to(device), cols)


def split_params(flat, cols):
    return tuple(flat[:, cols[k]].contiguous() for k in native.PARAM_KEYS)


def torch_lbfgs(evaluate, p, opt_keys, cols, device, max_iter, lr):
    """``torch.optim.LBFGS(max_iter, lr, strong_wolfe).step`` over the host rows ``p[k], k in opt_keys`` - in that order:
    it is the summation order of torch's inner products - with ``evaluate(params) -> {"loss", "grad"}``, an evaluate-only
    launch, as the closure; the other rows of `p` stay fixed.  `p` is updated in place.

    The optimiser's own arithmetic (two-loop recursion, strong-Wolfe bookkeeping: hundreds of tiny tensor operations per
    iteration) runs on HOST tensors, as it does in the reference (whose default device is the CPU): on device tensors every
    one of them is a kernel launch, and a 30-iteration fit took 21 ms of which the evaluate-only launches were 0.3 ms.
    Per closure call: one upload of the packed parameters, one launch, one download of [gradient | loss]."""
    params = [p[k].requires_grad_(True) for k in opt_keys]

    def closure():
        with torch.no_grad():
            r = evaluate(upload_params(p, cols, device))
            back = torch.cat((r["grad"], r["loss"][:, None]), dim=1).cpu()
        for k in opt_keys:
            p[k].grad = back[:, cols[k]].clone()
        return back[:, -1].sum()

    torch.optim.LBFGS(params, max_iter=max_iter, lr=lr, line_search_fn="strong_wolfe").step(closure)
    for k in opt_keys:
        p[k] = p[k].detach()
