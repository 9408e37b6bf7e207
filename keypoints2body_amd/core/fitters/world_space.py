"""World-space per-frame fitter on the HIP engine.

Drop-in for the reference's ``WorldSpaceFitter`` (reference
``keypoints2body/core/fitters/world_space.py:53-323``): same constructor and
``fit_frame`` signature, same result object.  Where the reference builds a loss
closure and steps ``torch.optim.Adam`` in Python (``world_space.py:248-256``), this
class validates its inputs, uploads them and makes ONE call into ``libk2b.so``
(``k2b_fit_world``: all iterations fused in one kernel, one frame per wavefront) plus
one ``k2b_lbs`` call for the final vertices/joints (``world_space.py:258-278``).

``use_lbfgs=True`` (the reference's default, ``world_space.py:231-247``) keeps L-BFGS with the strong-Wolfe line search
as the outer algorithm, exactly as the reference does, but its closure no longer builds an autograd graph: loss and
gradient of every evaluation come from an evaluate-only launch of the same kernel (``step_size = 0``, ``grad_out``).
Since round 4 the optimiser itself runs on the device too (``k2b_fit_world_lbfgs``, ``csrc/k2b_lbfgs.hip``: torch's
``LBFGS.step`` / ``_strong_wolfe`` restated as a per-frame state machine; the host only queues launches).  L-BFGS couples
all parameters it is given: the reference hands ONE optimiser the parameters of the whole batch, so for B > 1 its frames
share a line search; the API only ever calls it with B = 1 (``api/sequence.py:215``).  This class runs one independent
optimiser per frame, which equals the reference for B = 1 and deliberately differs (independent frames) for B > 1.
``lbfgs_driver = "host" | "torch"`` select the host-driven twins (``core/lbfgs_batched.py``; ``torch.optim.LBFGS`` itself).

Differences, all deliberate and documented in DESIGN.md:

* SMPL-H (52-joint models, ``SMPLHData``: both hands) and SMPL-X (55-joint models, ``SMPLXData``): hands, jaw, eyes and expression join the optimiser exactly as in the
  reference (``world_space.py:126-151,215-229``), fitted by the tree kernel (``csrc/k2b_fit_tree.hip``) over one packed
  pose / shape vector.  The reference hands SMPL-X's 63-D body pose to its 69-D mixture, which raises;
  here the mixture is evaluated at ``[body_pose | 0 x 6]``, and hands are full axis-angle poses (``use_pca=False``).
  Both branches: Adam fused, L-BFGS over evaluate-only launches of the tree kernel (one optimiser over the packed vectors:
  L-BFGS only ever forms inner products of the flattened parameters, so the packing does not change it);
  With a 24-joint model, hand / face fields of ``SMPLHData`` / ``SMPLXData`` inputs are carried through unchanged;
* vertex-selected joints (model joint index >= 24: smplx's "extra" joints, single mesh vertices): the fused
  kernel fits kinematic joints only, so ``k2b_fit_world`` then queues two launches per iteration (its kernel in
  evaluate-only mode for the kinematic targets and the priors, the vertex-term kernel with an Adam tail for the
  vertex targets and the step) - still one C call per fit, no host work between the launches, per-frame
  confidences allowed (the LBFGS branch gets loss and gradient of both terms from one evaluate-only call);
* ``fit_batch`` fits B independent frames in one launch with optional per-frame
  confidences; ``fit_frame`` keeps the reference's behaviour of using row 0 of a 2-D
  confidence tensor (``world_space.py:163-164``).
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from ... import native
from ...models.body_model import as_body_model
from ...models.smpl_data import BodyModelFitResult, SMPLData
from ...prior import MaxMixturePrior
from ..constants import root_indices
from .common import FitterBase, split_params, torch_lbfgs, upload_params


def guess_init_transl_from_root(smpl_model, pose_aa, betas, j3d_world_frame, joints_category="SMPL24"):
    """Initial translation = target root - model root at the initial pose
    (reference ``core/fitters/world_space.py:13-50``).  One joints-only LBS launch."""
    model = as_body_model(smpl_model)
    root_model, root_target = root_indices(joints_category)
    pose_aa = torch.as_tensor(pose_aa, dtype=torch.float32)
    with torch.no_grad():                          # the engine's own model calls build no graph
        out = model(global_orient=pose_aa[:, :3], body_pose=pose_aa[:, 3:], betas=betas, return_verts=False)
    target = torch.as_tensor(j3d_world_frame, dtype=torch.float32).to(model.device)
    return (target[:, root_target, :] - out.joints[:, root_model, :]).detach()


class WorldSpaceFitter(FitterBase):
    """Per-frame optimizer operating in world coordinates, executed on one MI355X."""

    def __init__(self, smpl_model, step_size=1e-2, num_iters_first=30, num_iters_followup=10, use_lbfgs=True,
                 joints_category="SMPL24", device=None, pose_prior_num_gaussians=8,
                 pose_prior: Optional[MaxMixturePrior] = None):
        smpl = as_body_model(smpl_model, device=device)
        if smpl.num_joints not in (24, 52, 55):
            raise NotImplementedError(
                f"a body model with {smpl.num_joints} joints: the fit kernels are built for the 24-joint SMPL tree "
                "(SMPL-H / SMPL-X parameter sets ride on it unfitted), the 52-joint SMPL-H and the 55-joint SMPL-X tree")
        super().__init__(smpl, step_size, use_lbfgs, joints_category, device, pose_prior_num_gaussians, pose_prior)
        self.num_iters_first = num_iters_first
        self.num_iters_followup = num_iters_followup

    # ------------------------------------------------------------------------------------
    def _config(self, seq_ind, joint_loss_weight, pose_preserve_weight, freeze_betas, per_frame_conf):
        cfg = native.default_fit_config()
        cfg.num_iters = int(self.num_iters_first if seq_ind == 0 else self.num_iters_followup)
        cfg.step_size = float(self.step_size)
        cfg.joint_loss_weight = float(joint_loss_weight)
        cfg.pose_preserve_weight = float(pose_preserve_weight) if seq_ind > 0 else 0.0   # world_space.py:211
        cfg.freeze_betas = int(bool(freeze_betas))
        cfg.conf_per_frame = int(bool(per_frame_conf))
        return cfg

    def _chain_config(self, joint_loss_weight, pose_preserve_weight, freeze_betas, per_frame):
        """Configuration of the warm-start entries: frame 0 as ``seq_ind == 0``, the preserve weight for frames >= 1."""
        cfg = self._config(0, joint_loss_weight, pose_preserve_weight, freeze_betas, per_frame)
        cfg.pose_preserve_weight = float(pose_preserve_weight)      # frames >= 1 (frame 0 has no preserve term)
        return self._packed_config(cfg)

    def _prepare(self, init_params, j3d, conf_3d, target_model_indices, per_frame_conf, num_init=None):
        """Argument handling shared by ``fit_batch`` and ``fit_chain``: device tensors in kernel layout, the joint
        gather of world_space.py:194-201 and the confidence rules of world_space.py:163-164.  ``num_init``: expected
        rows of ``init_params`` (default: one per frame of ``j3d``)."""
        if init_params.transl is None:
            raise ValueError("init_params.transl must be provided")
        j3d = torch.as_tensor(j3d, dtype=torch.float32)
        if j3d.dim() != 3 or j3d.shape[2] != 3:
            raise ValueError(f"j3d must be (B,K,3), got {tuple(j3d.shape)}")
        go, bp, be = self._start_rows(init_params)
        tr = self._dev(init_params.transl, 3)
        model_idx, tgt, conf = self._targets_and_conf(j3d, target_model_indices, conf_3d, per_frame_conf, (go, bp, be, tr),
                                                      j3d.shape[0] if num_init is None else num_init)
        return go, bp, be, tr, model_idx, tgt, conf

    def fit_batch(self, init_params: SMPLData, j3d, conf_3d=None, seq_ind: int = 0, target_model_indices=None,
                  joint_loss_weight: float = 600.0, pose_preserve_weight: float = 5.0, freeze_betas: bool = False,
                  per_frame_conf: bool = False, want_vertices: bool = True, run_forward: bool = True):
        """Fit B independent frames in one launch.

        Returns ``(params: dict of (B,.) tensors, joints, vertices, per_frame_loss)``; with
        ``run_forward=False`` the final forward is left to the caller (``final_forward``) and joints / vertices
        are ``None`` - the sharded sequence path gathers the parameters first.
        """
        go, bp, be, tr, model_idx, tgt, conf = self._prepare(init_params, j3d, conf_3d, target_model_indices, per_frame_conf)
        cfg = self._packed_config(self._config(seq_ind, joint_loss_weight, pose_preserve_weight, freeze_betas,
                                               per_frame_conf and conf is not None and conf.dim() == 2))
        if self.use_lbfgs:
            out = self._fit_lbfgs(cfg, model_idx, tgt, conf, go, bp, be, tr, freeze_betas)
        else:
            out = self._fit(cfg, model_idx, tgt, conf, dict(global_orient=go, body_pose=bp, betas=be, transl=tr))
        return self._result(out, run_forward, want_vertices)

    def _target_index(self, target_model_indices):
        """Model joint per target as ``chain_supported`` / ``chains_supported`` judge it (None: a category without a list)."""
        if target_model_indices is None:
            return self.smpl_index
        return torch.as_tensor(target_model_indices).reshape(-1).tolist()

    def chain_supported(self, target_model_indices=None) -> bool:
        """Whether ``fit_chain`` can run this fitter's sequence mode in one call: the Adam branch with kinematic targets (ONE
        launch, ``k2b_fit_sequence``), or the L-BFGS branch on the device driver (``k2b_fit_sequence_lbfgs``: one device-driven
        fit per frame, no host work between the frames); otherwise the caller fits frame by frame."""
        if self.use_lbfgs:
            return self.lbfgs_driver == "device" and (self.smpl_index is not None or target_model_indices is not None)
        idx = self._target_index(target_model_indices)
        return idx is not None and all(int(i) < self.smpl.num_joints for i in idx)

    def fit_chain(self, init_params: SMPLData, j3d, conf_3d=None, target_model_indices=None,
                  joint_loss_weight: float = 600.0, pose_preserve_weight: float = 5.0, freeze_betas: bool = False,
                  want_vertices: bool = True, run_forward: bool = True):
        """The reference's sequence mode (``api/sequence.py:214-281`` with ``use_previous_frame_init=True``) for ONE
        sequence of T frames in one launch (``k2b_fit_sequence``): frame 0 as ``seq_ind == 0`` from ``init_params``
        (one row), every later frame from its predecessor's result with the preserve term and
        ``num_iters_followup`` iterations.  ``conf_3d``: (K,) or per frame (T, K) as the sequence API passes it.
        Returns ``(params: dict of (T,.) tensors, joints, vertices, per_frame_loss)`` like ``fit_batch``."""
        if not self.chain_supported(target_model_indices):
            raise NotImplementedError("fit_chain: the Adam branch with kinematic targets, or the L-BFGS branch on the device driver")
        per_frame = conf_3d is not None and torch.as_tensor(conf_3d).dim() == 2
        go, bp, be, tr, model_idx, tgt, conf = self._prepare(init_params, j3d, conf_3d, target_model_indices, per_frame,
                                                             num_init=1)
        cfg = self._chain_config(joint_loss_weight, pose_preserve_weight, freeze_betas, per_frame)
        T = tgt.shape[0]
        if self.use_lbfgs:
            out = native.fit_sequence_lbfgs(self.smpl.native, self.pose_prior.native, cfg, int(self.num_iters_first),
                                            int(self.num_iters_followup), model_idx, tgt, conf, go, bp, be, tr, lr=float(self.step_size))
        else:
            out = native.fit_sequence(self.smpl.native, self.pose_prior.native, cfg, int(self.num_iters_followup), model_idx,
                                      tgt.unsqueeze(0), None if conf is None else (conf.unsqueeze(0) if per_frame else conf),
                                      go, bp, be, tr)
            out = {k: v.reshape((T,) + tuple(v.shape[2:])) for k, v in out.items()}
        return self._result(out, run_forward, want_vertices)

    def chains_supported(self, target_model_indices=None) -> bool:
        """Whether ``fit_chains`` takes this fitter's configuration in ONE launch - the native entries' own rules: Adam with
        kinematic targets on any model (``k2b_fit_sequences``); L-BFGS on the device driver with the 24-joint model and kinematic
        targets (``k2b_fit_sequences_lbfgs``).  Decided before anything runs, so that a caller can route first."""
        if not self.chain_supported(target_model_indices):
            return False
        if not self.use_lbfgs:
            return True
        idx = self._target_index(target_model_indices)
        return (self.smpl.num_joints == 24 and not self.smpl.packed and idx is not None
                and all(0 <= int(i) < self.smpl.num_joints for i in idx))

    def fit_chains(self, init_params: SMPLData, j3d, conf_3d, lengths, target_model_indices=None,
                   joint_loss_weight: float = 600.0, pose_preserve_weight: float = 5.0, freeze_betas: bool = False):
        """``fit_chain`` for S sequences of different lengths at once (``k2b_fit_sequences`` / ``k2b_fit_sequences_lbfgs``: ONE
        launch): ``init_params`` with one row per sequence, ``j3d`` packed (sum T, K, 3), ``conf_3d`` packed per frame
        (sum T, K) or shared (K,), ``lengths`` (S,).  Returns the packed params dict (``loss`` per frame); no forward.  Every
        sequence's rows equal ``fit_chain`` on it alone, bit for bit.  ``NotImplementedError`` where the native entry does not
        take the configuration (L-BFGS with SMPL-H / SMPL-X, surface targets): the caller fits sequence by sequence."""
        if not self.chain_supported(target_model_indices):
            raise NotImplementedError("fit_chains: the Adam branch with kinematic targets, or the L-BFGS branch on the device driver")
        per_frame = conf_3d is not None and torch.as_tensor(conf_3d).dim() == 2
        S = int(np.asarray(lengths).reshape(-1).shape[0])
        go, bp, be, tr, model_idx, tgt, conf = self._prepare(init_params, j3d, conf_3d, target_model_indices, per_frame,
                                                             num_init=S)
        cfg = self._chain_config(joint_loss_weight, pose_preserve_weight, freeze_betas, per_frame)
        if self.use_lbfgs:
            return native.fit_sequences_lbfgs(self.smpl.native, self.pose_prior.native, cfg, int(self.num_iters_first),
                                              int(self.num_iters_followup), model_idx, lengths, tgt, conf, go, bp, be, tr,
                                              lr=float(self.step_size))
        return native.fit_sequences(self.smpl.native, self.pose_prior.native, cfg, int(self.num_iters_followup), model_idx,
                                    lengths, tgt, conf, go, bp, be, tr)

    def fit_params(self, cfg, targets, init, model_idx=None):
        """The hot call alone: ONE fused-fit launch on device tensors that are already in kernel layout
        (`targets` (B,K,3) in the order of this fitter's joint category or of `model_idx`, `init` on the device, packed
        for SMPL-X).  `bench.py` times this + `final_forward`; `fit_batch` is the same two calls behind the reference's
        argument handling."""
        idx = list(self.smpl_index) if model_idx is None else list(model_idx)
        return self._fit(cfg, idx, targets, None, vars(init))        # (the data class's own field dict: nothing is built)

    def final_forward(self, out, want_vertices=True):
        """Final no-grad forward of the reference (world_space.py:258-278): joints (+ vertices) of fitted parameters."""
        return self.smpl.native.lbs(out["global_orient"], out["body_pose"], out["betas"], out["transl"],
                                    want_vertices=want_vertices)

    def _fit_lbfgs(self, cfg, model_idx, tgt, conf, go, bp, be, tr, freeze_betas):
        """LBFGS branch (world_space.py:231-247): ``torch.optim.LBFGS(params, max_iter=num_iters,
        lr=step_size, line_search_fn="strong_wolfe").step(closure)`` per frame, with the closure's
        loss and gradient evaluated by the HIP kernel; final loss re-evaluated afterwards.  One optimiser
        per frame: for B > 1 the reference couples the frames in one line search, this does not (see the module docstring).

        ``self.lbfgs_driver``: "device" (default since round 4: ``k2b_fit_world_lbfgs``, the optimiser itself on the GPU - every
        frame of every batch takes the same path, so a frame's result no longer depends on how a sequence was sharded),
        "host" (the lock-step numpy restatement ``core/lbfgs_batched.py``) or "torch" (``torch.optim.LBFGS`` itself, one frame
        at a time) - the two host drivers are the device path's twins in the tests."""
        max_iter = int(cfg.num_iters)
        B = go.shape[0]
        preserve = bp.clone()                          # world_space.py:159
        if self.lbfgs_driver == "device":
            # the optimiser's state machine runs in a kernel of its own, one instance per frame; the call only queues launches
            # (k2b_fit_world_lbfgs: max_eval + 2 rounds of [evaluate-only launch, step launch] + the final loss evaluation)
            out = native.fit_world_lbfgs(self.smpl.native, self.pose_prior.native, cfg, model_idx, tgt, conf, go, bp, be, tr,
                                         max_iter=max_iter, lr=float(self.step_size), preserve_pose=preserve)
            self.last_lbfgs_rounds = max_iter * 5 // 4 + 2
            return out
        cfg.num_iters, cfg.step_size = 1, 0.0          # evaluate-only launches, driven from the host (the round-2 / round-3 drivers,
        if B > 1 or self.lbfgs_driver == "host":       #  kept as the device path's twins: tests, diagnostics)
            return self._fit_lbfgs_lockstep(cfg, max_iter, model_idx, tgt, conf, go, bp, be, tr, preserve, freeze_betas)
        # one frame under torch.optim.LBFGS itself (common.torch_lbfgs).  Parameter order of world_space.py:215-229.
        # (SMPL-X: the packed shape vector = betas | expression always joins the optimiser; with frozen betas their part of
        #  the gradient is zero (``num_betas_prior``), which leaves them - and L-BFGS's inner products - untouched)
        opt_keys = ["global_orient", "body_pose", "transl"] + (["betas"] if not freeze_betas or self.smpl.packed else [])
        cols = native.param_columns(bp.shape[1], be.shape[1])
        p = {k: t.detach().to("cpu").clone() for k, t in zip(native.PARAM_KEYS, (go, bp, be, tr))}
        evaluate = lambda cur, want_grad=True: self._fit(cfg, model_idx, tgt, conf, dict(zip(native.PARAM_KEYS, cur)),
                                                         preserve_pose=preserve, want_grad=want_grad)
        torch_lbfgs(evaluate, p, opt_keys, cols, self.device, max_iter, float(self.step_size))
        with torch.no_grad():
            loss = evaluate(upload_params(p, cols, self.device), False)["loss"]            # world_space.py:245-246
        out = {k: p[k].detach().to(self.device).contiguous() for k in native.PARAM_KEYS}
        out["loss"] = loss.contiguous()
        return out

    def _fit_lbfgs_lockstep(self, cfg, max_iter, model_idx, tgt, conf, go, bp, be, tr, preserve, freeze_betas):
        """B > 1 frames in the L-BFGS branch: the B per-frame optimisers advance in lock-step (``core/lbfgs_batched.py``, torch's
        L-BFGS / strong-Wolfe restated and vectorised over the frames), so ONE evaluate-only launch over all B frames serves
        the pending closure call of every frame - ~max_iter * 5 / 4 launches for the whole batch instead of that many per
        frame, and the optimiser's bookkeeping is a few numpy operations per round instead of B x hundreds of tiny tensor
        operations.  Frames stay independent (each has its own history, line search and stopping rule).  Per round: one
        upload of the (B, P) points, one launch, one download of [gradient | loss]."""
        from ..lbfgs_batched import BatchedLBFGS
        cols = native.param_columns(bp.shape[1], be.shape[1])
        dev = self.device
        shape_in_optimiser = not freeze_betas or self.smpl.packed          # as in the per-frame path
        start = torch.cat((go, bp, be, tr), dim=1)                         # kernel layout [go | pose | shape | transl]
        free = np.ones(start.shape[1], dtype=bool)
        if not shape_in_optimiser:
            free[cols["betas"]] = False
        free_t = torch.as_tensor(free, device=dev)
        flat = start.clone()

        def launch(x_free, want_grad):
            with torch.no_grad():
                flat[:, free_t] = torch.from_numpy(np.ascontiguousarray(x_free, dtype=np.float32)).to(dev)
                cur = split_params(flat, cols)
                return self._fit(cfg, model_idx, tgt, conf, dict(zip(native.PARAM_KEYS, cur)), preserve_pose=preserve,
                                 want_grad=want_grad), cur

        def evaluate(x_free):
            r, _ = launch(x_free, True)
            back = torch.cat((r["grad"], r["loss"][:, None]), dim=1).cpu().numpy()
            return back[:, -1].astype(np.float64), back[:, :-1][:, free]

        opt = BatchedLBFGS(evaluate, start.cpu().numpy()[:, free], lr=float(self.step_size), max_iter=max_iter)
        x = opt.run()
        r, cur = launch(x, False)                                          # final loss re-evaluated (world_space.py:245-246)
        self.last_lbfgs_rounds = opt.rounds
        return {"global_orient": cur[0], "body_pose": cur[1], "betas": cur[2], "transl": cur[3], "loss": r["loss"]}

    def fit_frame(self, init_params: SMPLData, j3d: torch.Tensor, conf_3d: Optional[torch.Tensor] = None,
                  seq_ind: int = 0, target_model_indices: Optional[torch.Tensor] = None,
                  joint_loss_weight: float = 600.0, pose_preserve_weight: float = 5.0,
                  freeze_betas: bool = False) -> BodyModelFitResult:
        """Fit one frame (or a batch) with the reference's ``fit_frame`` contract:
        inputs are not modified, outputs are detached tensors, ``loss`` is the batch sum of
        the last iteration's loss evaluated before its step (world_space.py:256)."""
        return self._frame_result(self.fit_batch(
            init_params, j3d, conf_3d, seq_ind, target_model_indices, joint_loss_weight, pose_preserve_weight,
            freeze_betas, per_frame_conf=False), init_params)
