"""What the world-space and the camera-space fitter share: construction, argument handling, the result tail and the
host-driven ``torch.optim.LBFGS`` twin of the device optimiser."""
from __future__ import annotations

from typing import Optional

import torch

from ... import native
from ...models.body_model import BodyModel, as_body_model
from ...prior import MaxMixturePrior
from ..constants import category_indices


class FitterBase:
    """Model, device, joint category and prior of a fitter."""

    # "device": the optimiser on the GPU; or one of the host-driven twins the subclass names.  A class-level default, so that
    # both ``fitter.lbfgs_driver = ...`` and ``WorldSpaceFitter.lbfgs_driver = ...`` (tools/dev_lbfgs_seq_timing.py) select one
    lbfgs_driver = "device"

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

    def _result(self, out, run_forward, want_vertices):
        """``(params, joints, vertices, per-frame loss)``; without `run_forward` the final forward is the caller's."""
        if not run_forward:
            return out, None, None, out["loss"]
        joints, verts = self.final_forward(out, want_vertices=want_vertices)
        return out, joints, verts, out["loss"]


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
