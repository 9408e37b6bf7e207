"""``optimize_params_sequence`` / ``optimize_shape_sequence`` (reference
``keypoints2body/api/sequence.py:40-319``), executed on the HIP engine.

Two execution modes, both with the reference's per-frame semantics:

* ``use_previous_frame_init=True`` (reference default): every frame starts from the previous
  frame's result, an inherently sequential chain (``api/sequence.py:280-281``).  World mode, Adam branch,
  kinematic targets (SMPL and SMPL-X): the WHOLE chain is one launch (``k2b_fit_sequence``: the frame loop runs
  inside the kernel, parameters and optimiser state never leave registers) followed by one final forward over
  all frames; any other configuration: one single-frame call per frame;
* ``use_previous_frame_init=False``: every frame starts from the same initial parameters, so
  the frames are independent and are fitted in TWO launches: frame 0
  (``num_iters_first``, no preserve term) and frames 1..T-1 as one batch
  (``num_iters_followup``, preserve term towards the shared initial pose) + ONE final forward.  When a
  ``torch.distributed`` process group is initialised (one process per GPU, ``torchrun``), the T frames are cut
  into contiguous blocks, one per rank (``parallel.fit_forward_exchange``: no collective during the iterations;
  the all-gather of the fitted parameters is enqueued under the rank's final forward over ITS block, the joints
  follow).  Every rank returns parameters, joints and loss of all frames; vertices stay on the rank that produced
  them (``vertices=None`` elsewhere) unless ``gather_vertices=True``.  Frame 0 is fitted once, by
  the rank that owns it.  ``bench.py`` times this very function.
"""
from __future__ import annotations

import dataclasses
from typing import Callable, Optional

import numpy as np
import torch

from ..core.config import ModelType, SequenceOptimizeConfig, sequence_config_from
from ..core.engine import (OptimizeEngine, default_init_params, load_mean_pose_shape, optimize_shape_pass,
                           optimize_shape_pass_batched, upgrade_smpl_family_init_params)
from ..core.joints.adapters import normalize_sequence_observations
from ..models.smpl_data import BodyModelFitResult, BodyModelParams, SMPLData, param_rows
from . import common
from .frame import _with_root_aligned_transl, ikgat_init_params, ikgat_prev_params


def _process_group():
    """The ``torch.distributed`` module when this process is one rank of an initialised group of > 1, else None."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        return dist
    return None


def _packed_widths(est, prev: BodyModelParams):
    """Columns of the kernel-layout pose / shape vectors the fitter returns: for packed 52- / 55-joint models ALL non-root
    joints and betas | expression (162 / 153 and 20 values), else the widths of `prev` (63 / 69 and 10)."""
    smpl = getattr(est.fitter, "smpl", None)
    if smpl is not None and getattr(smpl, "packed", False):
        return 3 * (int(smpl.num_joints) - 1), int(smpl.num_shape)
    return int(prev.body_pose.shape[-1]), int(prev.betas.shape[-1])


def _fit_independent_frames(est, prev: BodyModelParams, xyz, conf, model_indices, dist, gather_vertices: bool = False):
    """The frame loop of ``api/sequence.py:214-281`` with ``use_previous_frame_init=False``: every frame starts from
    `prev`; frame 0 with ``seq_ind == 0`` semantics (``num_iters_first``, no preserve term), frames 1..T-1 with
    ``seq_ind >= 1`` semantics.  The T frames are cut into contiguous blocks, one per rank (one block = everything without a
    process group); a rank fits ITS block (frame 0 on the rank that owns it: one launch for it, one for the others), runs the
    final forward over ITS block only, and the ranks exchange the fitted parameters (enqueued under the forward) and the
    joints (``parallel.fit_forward_exchange``).  Vertices stay on the rank that produced them - ``vertices=None`` in the
    results of other ranks' frames - unless ``gather_vertices`` asks for the second exchange.

    Returns ``(params dict over all T frames, joints (T, .), vertex_of(i) -> (1, V, 3) | None, loss (T,))``."""
    from ..parallel import fit_forward_exchange, rows_per_rank, shard_bounds, unpack_outputs, valid_rows
    T = xyz.shape[0]
    world, rank = (dist.get_world_size(), dist.get_rank()) if dist is not None else (1, 0)
    start, stop = shard_bounds(T, world, rank)
    per = rows_per_rank(T, world)
    pose_dim, num_shape = _packed_widths(est, prev)
    device = xyz.device

    def fit_block():
        parts = []
        if start == 0 and stop > 0:
            o, _, _, _ = est.fit_batch(_repeat_params(prev, 1), xyz[0:1], conf[0], seq_ind=0,
                                       target_model_indices=model_indices, per_frame_conf=False, run_forward=False)
            parts.append(o)
        lo = max(start, 1)
        if stop > lo:
            o, _, _, _ = est.fit_batch(_repeat_params(prev, stop - lo), xyz[lo:stop], conf[lo:stop], seq_ind=1,
                                       target_model_indices=model_indices, per_frame_conf=True, run_forward=False)
            parts.append(o)
        if not parts:                                     # more ranks than frames: this rank has no frame - zero rows of the right widths
            e = lambda c: torch.zeros((0, c), dtype=torch.float32, device=device)
            return {"global_orient": e(3), "body_pose": e(pose_dim), "betas": e(num_shape), "transl": e(3),
                    "loss": torch.zeros((0,), dtype=torch.float32, device=device)}
        if len(parts) == 1:
            return parts[0]
        return {k: torch.cat([p[k] for p in parts], dim=0).contiguous() for k in parts[0]}

    def forward_block(out):
        # (also for a rank without frames: the forward of zero rows returns zero-row joints / vertices, and the rank enters
        #  every collective of the exchange with padding only - never branch a collective on what a block holds)
        return est.fitter.final_forward(out)

    ex = fit_forward_exchange(fit_block, forward_block, dist, pad_to=per, gather_vertices=gather_vertices)
    if world == 1:
        out, joints, verts = ex["local"], ex["joints"], ex["vertices"]
        return out, joints, (lambda i: verts[i: i + 1]), out["loss"]
    keep = valid_rows(T, world, device)
    out = unpack_outputs(ex["packed"].index_select(0, keep), num_shape, pose_dim)
    joints, verts = ex["joints"], ex["vertices"]
    joints = joints.index_select(0, keep)
    if ex["vertices_gathered"]:
        verts = verts.index_select(0, keep)
        vertex_of = lambda i: verts[i: i + 1]
    else:
        vertex_of = lambda i: verts[i - start: i - start + 1] if start <= i < stop else None
    return out, joints, vertex_of, out["loss"]


def _preprocess_sequence(joints_seq, joint_layout, body_model, seq_cfg: SequenceOptimizeConfig, device):
    """Observations of one sequence as both entry points fit them: layout adaptation (which sets the config's joints category,
    as the reference does), ``limit_frames`` and the ``fix_foot`` confidences (api/sequence.py:96-128).
    Returns ``(xyz (T, K, 3), conf (T, K), model_indices or None)`` on `device`."""
    xyz, conf, model_indices, in_layout = normalize_sequence_observations(joints_seq, layout=joint_layout,
                                                                         body_model=body_model)
    xyz, conf, model_indices = common.canonicalize(xyz, conf, model_indices, in_layout, joint_layout, body_model,
                                                   seq_cfg.frame, device)
    if seq_cfg.limit_frames is not None and seq_cfg.limit_frames > 0:
        xyz, conf = xyz[: seq_cfg.limit_frames], conf[: seq_cfg.limit_frames]
    if seq_cfg.fix_foot and xyz.shape[1] > 11:       # api/sequence.py:124-128
        conf = conf.clone()
        conf[:, [7, 8, 10, 11]] = 1.5
    return xyz, conf, model_indices


def _repeat_params(p: BodyModelParams, n: int) -> BodyModelParams:
    """`p` (one row) as the start of n frames, every array field repeated and the data class kept - the reference hands
    `prev` itself (``SMPLHData`` / ``SMPLXData`` with hands, jaw, eyes, expression) to every frame (api/sequence.py:270-281)."""
    return dataclasses.replace(p, **{k: t.expand(n, -1).contiguous() for k, t in param_rows(p)})


def optimize_params_sequence(joints_seq, *, init_params: Optional[BodyModelParams] = None,
                             body_model: ModelType = "smpl", joint_layout: Optional[str] = None, model=None,
                             config: Optional[SequenceOptimizeConfig | dict] = None, device=None,
                             pose_prior=None, mean_params: Optional[tuple] = None,
                             gather_vertices: bool = False) -> list[BodyModelFitResult]:
    """Optimise body parameters for a motion sequence; results in temporal order.

    ``gather_vertices`` only matters for independent frames under a ``torch.distributed`` process group: every rank
    returns parameters, joints and loss of ALL frames, but the vertices of its own block only (``vertices=None``
    elsewhere) unless this asks for the second all-gather (82.7 KB per frame)."""
    device = common.resolve_device(device)
    seq_cfg = sequence_config_from(config)
    frame_cfg = seq_cfg.frame
    common.check_request(frame_cfg, body_model)
    xyz, conf, model_indices = _preprocess_sequence(joints_seq, joint_layout, body_model, seq_cfg, device)

    if frame_cfg.estimator_type == "ikgat":
        return _ikgat_sequence(xyz, init_params, body_model, model, seq_cfg, device)
    model = common.obtain_model(model, body_model, device)
    mean_pose, mean_shape = mean_params if mean_params is not None else load_mean_pose_shape(
        common.DEFAULT_MEAN_FILE, device)
    mean_pose, mean_shape = mean_pose.to(device), mean_shape.to(device)
    betas_opt = mean_shape
    if frame_cfg.joints_category != "GENERIC":
        betas_opt = optimize_shape_pass(model=model, seq_config=seq_cfg, init_mean_shape=mean_shape,
                                        init_mean_pose=mean_pose, data_tensor=xyz, confidence_input=conf[0],
                                        device=device, pose_prior=pose_prior)
    engine = OptimizeEngine(model=model, frame_config=frame_cfg, device=device, model_type=body_model,
                            pose_prior=pose_prior)
    if xyz.shape[0] == 0:
        return []

    if init_params is None:
        prev = common.default_start(model, body_model, frame_cfg.joints_category, frame_cfg.coordinate_mode, xyz[0:1],
                                    (mean_pose, mean_shape), device, betas=betas_opt)
    else:
        common.check_param_type(init_params, body_model, "init_params")
        prev = init_params.to(device)

    results: list[BodyModelFitResult] = []
    T = xyz.shape[0]
    est = engine.estimator
    if (seq_cfg.use_previous_frame_init and T > 1
            and hasattr(est.fitter, "chain_supported") and est.fitter.chain_supported(model_indices)):
        # world mode: the whole chain is one launch (Adam: k2b_fit_sequence, L-BFGS: k2b_fit_sequence_lbfgs); camera mode: the
        # stages are enqueued frame by frame, the reported loss and the final forward once for all frames
        if frame_cfg.coordinate_mode == "world" and prev.transl is None:
            prev = _with_root_aligned_transl(prev, xyz[0:1], model, frame_cfg, device)
        out, joints, verts, loss = est.fit_chain(prev, xyz, conf, model_indices)
        return _batched_results(est.fitter, out, joints, verts, loss, prev, T)
    if seq_cfg.use_previous_frame_init or T == 1:
        for idx in range(T):
            frame = xyz[idx: idx + 1]
            if frame_cfg.coordinate_mode == "world" and prev.transl is None:
                prev = _with_root_aligned_transl(prev, frame, model, frame_cfg, device)
            res = engine.fit_frame(init_params=prev, j3d=frame, conf_3d=conf[idx], seq_ind=idx,
                                   target_model_indices=model_indices)
            results.append(res)
            if seq_cfg.use_previous_frame_init:
                prev = res.params
        return results

    # independent frames: all start from `prev` (api/sequence.py:214-281 with use_previous_frame_init=False)
    if frame_cfg.coordinate_mode == "world" and prev.transl is None:
        prev = _with_root_aligned_transl(prev, xyz[0:1], model, frame_cfg, device)
    if not hasattr(est.fitter, "fit_batch"):          # (a plug-in estimator without a batched entry point: one call per frame)
        for idx in range(T):
            results.append(engine.fit_frame(init_params=prev, j3d=xyz[idx: idx + 1], conf_3d=conf[idx], seq_ind=idx,
                                            target_model_indices=model_indices))
        return results
    out, joints, vertex_of, loss = _fit_independent_frames(est, prev, xyz, conf, model_indices, _process_group(),
                                                           gather_vertices)
    return [BodyModelFitResult(params=est.fitter.result_params(out, prev, slice(i, i + 1)), vertices=vertex_of(i),
                               joints=joints[i: i + 1], loss=loss[i]) for i in range(T)]


def _ikgat_sequence(xyz, init_params, body_model, model, seq_cfg, device) -> list[BodyModelFitResult]:
    """IK-GAT over a sequence (reference ``api/sequence.py:90,130-137,167-176,214-281``): no model, no mean parameters, no
    shape pass.  The one start object is carried through every frame, so every result's params equal it (frame 0's
    ``transl`` included).  ONE launch and one device-to-host copy of the (T, J, 4) quaternions: independent frames run
    batched; the pos-rot6 network with ``use_previous_frame_init=True`` runs as one in-kernel chain, frame t reading frame
    t-1's prediction.  Under a process group every rank runs all frames (no sharding)."""
    from ..core.estimators.ikgat import IKGATEstimator, result_for
    frame_cfg = seq_cfg.frame
    est = IKGATEstimator(frame_cfg, device=device)
    T = xyz.shape[0]
    if T == 0:
        return []
    if init_params is None:
        prev = ikgat_init_params(xyz[0:1], frame_cfg, device)
    else:
        prev = ikgat_prev_params(init_params, xyz[0:1], body_model, model, frame_cfg, device, "init_params")
    chain = est.needs_quaternions and seq_cfg.use_previous_frame_init and T > 1
    quats = est.predict(est._positions(xyz), est._quaternions(prev), chain=chain)
    return [result_for(prev, quats[t], xyz[t: t + 1]) for t in range(T)]


def _batched_results(fitter, out, joints, verts, loss, init, n) -> list[BodyModelFitResult]:
    """Per-frame result objects (the data class the reference returns for the model / input type) of a batched fit."""
    return [BodyModelFitResult(params=fitter.result_params(out, init, slice(i, i + 1)), vertices=verts[i: i + 1],
                               joints=joints[i: i + 1], loss=loss[i]) for i in range(n)]


def pack_ragged(seqs):
    """Sequences of (T_s, ...) tensors -> ``(packed (sum T, ...), lengths (S,) int32, offsets (S,) int32)``: sequence s owns
    rows ``offsets[s] .. offsets[s] + lengths[s] - 1`` (offsets = exclusive prefix sums of the lengths)."""
    from ..native import ragged_offsets
    lengths = np.asarray([int(s.shape[0]) for s in seqs], dtype=np.int32)
    return torch.cat(list(seqs), dim=0), lengths, ragged_offsets(lengths)


@dataclasses.dataclass
class SequenceBatch:
    """Result of ``optimize_params_sequences``: S fitted sequences in packed form - no per-frame objects, no vertices.

    ``params``: ``global_orient``, ``body_pose``, ``betas``, ``transl`` as (sum T, .) tensors in the layout of the reference's
    result objects; ``joints`` (sum T, J, 3); ``loss`` (sum T,); sequence s owns rows ``offsets[s] .. offsets[s] + lengths[s]``.
    ``results(s)`` is what ``optimize_params_sequence`` returns for sequence s (vertices from one LBS launch for it);
    ``pose(s)`` is its (T, 3 + body pose) axis-angle pose, what the eval consumes."""
    params: dict
    joints: torch.Tensor
    loss: torch.Tensor
    lengths: np.ndarray
    offsets: np.ndarray
    _result_fn: Optional[Callable[[int], list]] = dataclasses.field(default=None, repr=False)

    def __len__(self) -> int:
        return int(len(self.lengths))

    @property
    def num_frames(self) -> int:
        return int(np.asarray(self.lengths, dtype=np.int64).sum())

    def _rows(self, s: int) -> slice:
        if not 0 <= s < len(self):
            raise IndexError(f"sequence {s} of {len(self)}")
        o = int(self.offsets[s])
        return slice(o, o + int(self.lengths[s]))

    def pose(self, s: int) -> torch.Tensor:
        rows = self._rows(s)
        return torch.cat([self.params["global_orient"][rows], self.params["body_pose"][rows]], dim=1)

    def loss_of(self, s: int) -> torch.Tensor:
        return self.loss[self._rows(s)]

    def joints_of(self, s: int) -> torch.Tensor:
        return self.joints[self._rows(s)]

    def results(self, s: int) -> list[BodyModelFitResult]:
        self._rows(s)
        return self._result_fn(s)


def _batch_from_results(per_seq: list[list[BodyModelFitResult]], device) -> SequenceBatch:
    """Packed view of per-sequence result lists (the loop path)."""
    lengths = np.asarray([len(r) for r in per_seq], dtype=np.int32)
    from ..native import ragged_offsets
    flat = [r for rs in per_seq for r in rs]
    keys = ("global_orient", "body_pose", "betas", "transl")
    if flat:
        params = {k: torch.cat([torch.as_tensor(getattr(r.params, k), dtype=torch.float32, device=device).reshape(1, -1)
                                for r in flat]) for k in keys}
        joints = torch.cat([r.joints for r in flat], dim=0)
        loss = torch.stack([torch.as_tensor(r.loss, dtype=torch.float32, device=device).reshape(()) for r in flat])
    else:
        params = {k: torch.zeros((0, 0), device=device) for k in keys}
        joints, loss = torch.zeros((0, 0, 3), device=device), torch.zeros((0,), device=device)
    return SequenceBatch(params=params, joints=joints, loss=loss, lengths=lengths, offsets=ragged_offsets(lengths),
                         _result_fn=lambda s: per_seq[s])


def _packed_batch(fitter, out, joints, loss, lengths, offsets, starts) -> SequenceBatch:
    """``SequenceBatch`` of a packed fit `out` over all frames: `starts` holds one start per sequence; ``results(s)`` cuts
    sequence s out and runs the final forward for its vertices."""
    ref = fitter.result_params(out, starts[0])                # reference layout (SMPL-H / SMPL-X: hands and face unpacked)
    params = {k: getattr(ref, k) for k in ("global_orient", "body_pose", "betas", "transl")}

    def result_fn(s):
        n, o = int(lengths[s]), int(offsets[s])
        if n == 0:
            return []
        part = {k: v[o:o + n].contiguous() for k, v in out.items()}
        j, v = fitter.final_forward(part)
        return _batched_results(fitter, part, j, v, part["loss"], starts[s], n)

    return SequenceBatch(params=params, joints=joints, loss=loss, lengths=lengths, offsets=offsets, _result_fn=result_fn)


def _stack_starts(starts: list[BodyModelParams], device) -> BodyModelParams:
    """One-row starts of the same data class -> one object with a row per start (kernel inputs of ``fit_chains``)."""
    rows = [dict(param_rows(p)) for p in starts]
    return dataclasses.replace(starts[0], **{k: torch.cat([r[k].to(device) for r in rows], dim=0).contiguous() for k in rows[0]})


def optimize_params_sequences(joints_seqs, *, init_params: Optional[list] = None, body_model: ModelType = "smpl",
                              joint_layout: Optional[str] = None, model=None,
                              config: Optional[SequenceOptimizeConfig | dict] = None, device=None, pose_prior=None,
                              mean_params: Optional[tuple] = None) -> SequenceBatch:
    """``optimize_params_sequence`` for many sequences in one call; returns a packed ``SequenceBatch``.

    ``joints_seqs``: a list of whatever ``optimize_params_sequence`` accepts; ``init_params``: None or one start (one row)
    per sequence.  Every sequence is preprocessed exactly as the single call does it (layout adaptation, ``limit_frames``,
    ``fix_foot``, the shape pre-pass, the default start); with the shape pre-pass off its result equals the single call's bit
    for bit.

    Which path runs:
    * world mode, ``use_previous_frame_init=True``, a fitter whose ``chain_supported`` holds, one target set for all
      sequences: ONE launch for all chains (``k2b_fit_sequences``: Adam, SMPL / SMPL-H / SMPL-X; ``k2b_fit_sequences_lbfgs``:
      L-BFGS, 24-joint model), the sequences longest first inside, results in the caller's order.  The shape pre-pass (when
      enabled and the joints category is not GENERIC) runs for all sequences together on the device
      (``optimize_shape_pass_batched``: agrees with the single call's ``optimize_shape_pass`` within 1e-5, not bit for bit -
      the chains are then bit-identical to the single call started from those betas); the default starts of all sequences
      come from one batched forward;
    * everything else (camera mode, independent frames, IK-GAT, surface targets, L-BFGS on SMPL-H / SMPL-X): a loop of
      ``optimize_params_sequence``, correct by construction.
    Errors are the single call's, raised before anything is launched.  Under a ``torch.distributed`` process group every rank
    fits all sequences."""
    from ..core.estimators.optimization import OptimizationEstimator
    if not isinstance(joints_seqs, (list, tuple)):
        raise TypeError("joints_seqs must be a list of sequences")
    if len(joints_seqs) == 0:
        raise ValueError("joints_seqs is empty")
    S = len(joints_seqs)
    if init_params is not None:
        if not isinstance(init_params, (list, tuple)) or len(init_params) != S:
            raise ValueError("init_params must be None or a list with one start per sequence")
    seq_cfg = sequence_config_from(config)
    frame_cfg = seq_cfg.frame
    common.check_request(frame_cfg, body_model)
    if init_params is not None:
        for p in init_params:
            common.check_param_type(p, body_model, "init_params")
    if (frame_cfg.estimator_type != "ikgat" and seq_cfg.use_shape_optimization and not frame_cfg.use_lbfgs
            and frame_cfg.joints_category != "GENERIC"):
        raise RuntimeError(
            "use_shape_optimization=True with use_lbfgs=False: the reference's Adam branch of the shape "
            "pre-pass raises (core/shape.py:10,110-113); set use_shape_optimization=False or use_lbfgs=True")
    device = common.resolve_device(device)

    def by_loop(model_obj, prior):
        per_seq = [optimize_params_sequence(j, init_params=None if init_params is None else init_params[s], body_model=body_model,
                                            joint_layout=joint_layout, model=model_obj, config=seq_cfg, device=device,
                                            pose_prior=prior, mean_params=mean_params)
                   for s, j in enumerate(joints_seqs)]
        return _batch_from_results(per_seq, device)

    if frame_cfg.estimator_type == "ikgat" or frame_cfg.coordinate_mode != "world" or not seq_cfg.use_previous_frame_init:
        return by_loop(model, pose_prior)

    # per-sequence preprocessing: the single call's own helper
    xs, cs, idx_sets = [], [], []
    for j in joints_seqs:
        xyz, conf, model_indices = _preprocess_sequence(j, joint_layout, body_model, seq_cfg, device)
        xs.append(xyz)
        cs.append(conf)
        idx_sets.append(None if model_indices is None else tuple(int(i) for i in model_indices.reshape(-1).tolist()))
    model = common.obtain_model(model, body_model, device)
    if pose_prior is None:
        from ..prior import MaxMixturePrior
        pose_prior = MaxMixturePrior(prior_folder="./data/models/", num_gaussians=frame_cfg.pose_prior_num_gaussians,
                                     device=device)
    engine = OptimizeEngine(model=model, frame_config=frame_cfg, device=device, model_type=body_model, pose_prior=pose_prior)
    est = engine.estimator
    model_indices = None if idx_sets[0] is None else torch.tensor(idx_sets[0], dtype=torch.long)
    # the route is decided before any shape pass runs (the native entries' own support rules, mirrored by chains_supported)
    if (not isinstance(est, OptimizationEstimator) or len(set(idx_sets)) != 1 or not hasattr(est.fitter, "fit_chains")
            or not est.fitter.chains_supported(model_indices)):
        return by_loop(model, pose_prior)

    mean_pose, mean_shape = mean_params if mean_params is not None else load_mean_pose_shape(common.DEFAULT_MEAN_FILE, device)
    mean_pose, mean_shape = mean_pose.to(device), mean_shape.to(device)
    live = [s for s in range(S) if xs[s].shape[0] > 0]
    need_default = [s for s in live if init_params is None]
    betas_of = {s: mean_shape for s in need_default}
    if need_default and seq_cfg.use_shape_optimization and frame_cfg.joints_category != "GENERIC":
        # the shape pre-pass of every sequence that needs a default start, all together on the device (a given start makes
        # the single call's pass result unused: it is not run)
        betas = optimize_shape_pass_batched(model, seq_cfg, mean_shape, mean_pose, [xs[s] for s in need_default],
                                            [cs[s][0] for s in need_default], device, pose_prior=pose_prior)
        betas_of = {s: betas[i:i + 1] for i, s in enumerate(need_default)}
    starts = {}
    if need_default:                                  # the default starts of all sequences: ONE batched forward
        n = len(need_default)
        base = default_init_params(mean_pose.expand(n, -1), torch.cat([betas_of[s].reshape(1, -1) for s in need_default]),
                                   torch.cat([xs[s][0:1] for s in need_default]), model,
                                   joints_category=frame_cfg.joints_category, coordinate_mode=frame_cfg.coordinate_mode)
        for i, s in enumerate(need_default):
            one = SMPLData(betas=base.betas[i:i + 1], global_orient=base.global_orient[i:i + 1],
                           body_pose=base.body_pose[i:i + 1], transl=base.transl[i:i + 1])
            starts[s] = upgrade_smpl_family_init_params(one, model_type=body_model, model=model, device=device)
    if init_params is not None:
        for s in live:
            starts[s] = init_params[s].to(device)
    for s in live:
        if starts[s].transl is None:
            starts[s] = _with_root_aligned_transl(starts[s], xs[s][0:1], model, frame_cfg, device)
    if not live:
        return _batch_from_results([[] for _ in range(S)], device)

    j3d, lengths, offsets = pack_ragged(xs)
    conf = torch.cat(cs, dim=0).contiguous()
    # one start row per sequence (an empty sequence's row is never read: any live start stands in)
    starts = [starts.get(s, starts[live[0]]) for s in range(S)]
    try:
        out = est.fit_chains(_stack_starts(starts, device), j3d, conf, lengths, model_indices)
    except NotImplementedError:                       # (L-BFGS on SMPL-H / SMPL-X): sequence by sequence
        return by_loop(model, pose_prior)
    joints, _ = est.fitter.final_forward(out, want_vertices=False)
    return _packed_batch(est.fitter, out, joints, out["loss"], lengths, offsets, starts)


def optimize_shape_sequence(joints_seq, *, body_model: ModelType = "smpl", joint_layout: Optional[str] = None,
                            model=None, config: Optional[SequenceOptimizeConfig | dict] = None, device=None,
                            pose_prior=None, mean_params: Optional[tuple] = None) -> BodyModelParams:
    """Run the sequence optimisation and return the last frame's parameters."""
    results = optimize_params_sequence(joints_seq, init_params=None, body_model=body_model, joint_layout=joint_layout,
                                       model=model, config=config, device=device, pose_prior=pose_prior,
                                       mean_params=mean_params)
    if not results:
        raise ValueError("No frames were optimized")
    return results[-1].params
