"""The learned IK-GAT estimator (reference ``keypoints2body/core/estimators/ikgat/``) on the HIP engine.

The reference runs its graph-attention regressor one frame at a time through PyTorch and PyG.  Here the
checkpoint is read on the host, checked against the network the config describes and packed into the layout
of ``k2b_ikgat_create`` (include/k2b.h; the one table of that order is ``ikgat_segment`` in csrc/k2b_ikgat_plan.h, and
``expected_shapes`` below is held to it by tests/test_ikgat_plan_host.py); inference is the HIP kernel ``k2b_ikgat_kernel``
(csrc/k2b_ikgat.hip), which also does the reference's pre- and post-processing (root subtraction, quaternion
-> 6-D, 6-D -> quaternion).  The uploaded network is cached per checkpoint file (path, size, mtime) and
network shape, so a per-frame loop of ``optimize_params_frame`` reads and uploads it once.

Differences from the reference, all at its failure boundaries:

* the checkpoint is loaded with ``torch.load(weights_only=True)``; anything but tensors (optionally inside a
  ``{"model_state": ...}`` wrapper) is refused with ``ValueError``;
* a missing, extra or mis-shaped state-dict entry raises ``ValueError`` naming the key (the reference's
  ``load_state_dict`` raises ``RuntimeError``);
* a frame whose joint count differs from ``len(ikgat_parent_ids)`` raises ``ValueError`` before any launch
  (the reference fails later with a broadcasting ``RuntimeError``);
* input quaternions of the wrong shape raise ``ValueError``.

PyG's ``GATConv`` is restated, not imported (``torch_geometric`` is not a dependency), so parity with it is
unpinned at that boundary; the goldens under ``tests/golden/ikgat_*.npz`` come from the reference's own code
with only ``GATConv`` restated (``tools/gen_golden_ikgat.py``).
"""
from __future__ import annotations

import dataclasses as _dc
import json
import logging
import os
import pickle
from collections import OrderedDict
from pathlib import Path
from typing import Optional

import numpy as np
import torch

from ...models.smpl_data import BodyModelFitResult, BodyModelParams

logger = logging.getLogger(__name__)

SUPPORTED_FORMATS = ("manny", "smplx")
MODEL_TYPES = {"pos_to_rot6": 3, "pos-rot6_to_rot6": 9}     # model_type -> input width (inference.py:22-24, 150-153)
_SHAPE_KEYS = ("hidden_dim", "num_layers", "num_heads")
# keyword arguments of the reference's GATRotationRegressor that config.json may carry besides the three above;
# input_format / output_format are overwritten by create_rotation_regressor (inference.py:166-174)
_CTOR_KEYS = ("dropout", "input_format", "output_format")
_CACHE_SIZE = 8


@_dc.dataclass(frozen=True)
class IkgatSpec:
    """What a ``FrameOptimizeConfig`` resolves to: the checkpoint and the network it must hold."""

    path: Path
    model_type: str
    input_dim: int
    parents: tuple
    hidden_dim: int
    num_layers: int
    num_heads: int

    @property
    def num_joints(self) -> int:
        return len(self.parents)


def _detect_config(config_path: Path) -> dict:
    """``config.json`` next to the checkpoint, used only when it names all three shape keys (inference.py:126-143)."""
    default = {"hidden_dim": 128, "num_layers": 3, "num_heads": 4}
    if not config_path.exists():
        return default
    try:
        with config_path.open("r", encoding="utf-8") as f:
            cfg = json.load(f)
    except Exception as exc:
        logger.warning("Failed to load IKGAT config at %s: %s", config_path, exc)
        return default
    if not isinstance(cfg, dict) or any(k not in cfg for k in _SHAPE_KEYS):
        return default
    return cfg


def resolve(frame_config) -> IkgatSpec:
    """Checks, path and config.json resolution in the reference's order (inference.py:146-177, 62-63)."""
    fmt, mtype, parents = frame_config.ikgat_model_format, frame_config.ikgat_model_type, frame_config.ikgat_parent_ids
    if fmt not in SUPPORTED_FORMATS:
        raise ValueError(f"Unsupported model_format: {fmt}. Supported: {sorted(SUPPORTED_FORMATS)}")
    if mtype not in MODEL_TYPES:
        raise ValueError(f"Unsupported model_type: {mtype}. Supported: {sorted(MODEL_TYPES)}")
    if not parents:
        raise ValueError("ikgat_parent_ids must be provided for estimator_type='ikgat'")
    path = Path(frame_config.ikgat_model_dir) / "ikgat" / mtype / f"{fmt}.pth"
    model_cfg = _detect_config(path.parent / "config.json")
    if not path.exists():
        raise FileNotFoundError(f"IKGAT model file not found: {path}")
    # the shape keys are overwritten by the frame config; every other key reaches the network constructor
    unknown = sorted(k for k in model_cfg if k not in _SHAPE_KEYS and k not in _CTOR_KEYS)
    if unknown:
        raise TypeError(f"GATRotationRegressor.__init__() got an unexpected keyword argument '{unknown[0]}' "
                        f"(from {path.parent / 'config.json'})")
    return IkgatSpec(path=path, model_type=mtype, input_dim=MODEL_TYPES[mtype], parents=tuple(int(p) for p in parents),
                     hidden_dim=int(frame_config.ikgat_hidden_dim), num_layers=int(frame_config.ikgat_num_layers),
                     num_heads=int(frame_config.ikgat_num_heads))


def expected_shapes(spec: IkgatSpec) -> "OrderedDict[str, tuple]":
    """State-dict keys of the reference's GATRotationRegressor (recent PyG spelling) in the packing order of
    ``k2b_ikgat_create``, with their shapes."""
    J, IN, H, L, NH = spec.num_joints, spec.input_dim, spec.hidden_dim, spec.num_layers, spec.num_heads
    if NH < 1 or H % NH:
        raise ValueError(f"ikgat_num_heads={NH} does not divide ikgat_hidden_dim={H}")
    C, H2 = H // NH, H // 2
    s = OrderedDict()
    s["input_proj.weight"], s["input_proj.bias"] = (H, IN), (H,)
    s["joint_pos_embed.weight"] = (J, H)
    s["residual_proj.weight"], s["residual_proj.bias"] = (H, IN), (H,)
    for l in range(L):
        s[f"gat_layers.{l}.lin.weight"] = (NH * C, H)
        s[f"gat_layers.{l}.att_src"] = (1, NH, C)
        s[f"gat_layers.{l}.att_dst"] = (1, NH, C)
        s[f"gat_layers.{l}.bias"] = (NH * C,)
        s[f"layer_norms.{l}.weight"], s[f"layer_norms.{l}.bias"] = (H,), (H,)
    s["output_head.0.weight"], s["output_head.0.bias"] = (H2, H), (H2,)
    s["output_head.2.weight"], s["output_head.2.bias"] = (H2,), (H2,)
    s["output_head.4.weight"], s["output_head.4.bias"] = (6, H2), (6,)
    return s


def read_checkpoint(path: Path) -> dict:
    """``torch.load(weights_only=True)`` of a state dict, ``{"model_state": ...}`` unwrapped; tensors only."""
    try:
        obj = torch.load(str(path), map_location="cpu", weights_only=True)
    except (pickle.UnpicklingError, RuntimeError, AttributeError, TypeError, EOFError) as exc:
        raise ValueError(f"{path}: not a weights-only checkpoint (only tensors in a state dict are loaded): {exc}") from None
    if isinstance(obj, dict) and "model_state" in obj:
        obj = obj["model_state"]
    if not isinstance(obj, dict):
        raise ValueError(f"{path}: expected a state dict, got {type(obj).__name__}")
    for k, v in obj.items():
        if not isinstance(v, torch.Tensor):
            raise ValueError(f"{path}: state-dict entry {k!r} is a {type(v).__name__}, not a tensor")
    return obj


def pack_state(state: dict, spec: IkgatSpec) -> np.ndarray:
    """The state dict as one float32 vector in ``k2b_ikgat_create``'s order.  Accepts both PyG spellings of the GAT
    projection: ``lin.weight`` (recent) or ``lin_src.weight`` + ``lin_dst.weight`` holding the same tensor (older)."""
    shapes = expected_shapes(spec)
    state = dict(state)
    for l in range(spec.num_layers):
        src, dst, lin = (f"gat_layers.{l}.{n}.weight" for n in ("lin_src", "lin_dst", "lin"))
        if lin not in state and (src in state or dst in state):
            if src not in state or dst not in state:
                raise ValueError(f"state dict has only one of {src!r} and {dst!r}")
            a, b = state.pop(src), state.pop(dst)
            if a.shape != b.shape or not torch.equal(a, b):
                raise ValueError(f"{src!r} and {dst!r} differ: the regressor's GAT layers share one projection")
            state[lin] = a
    missing = [k for k in shapes if k not in state]
    if missing:
        raise ValueError(f"state dict is missing {missing[0]!r}" + (f" (and {len(missing) - 1} more)" if len(missing) > 1 else ""))
    extra = sorted(k for k in state if k not in shapes)
    if extra:
        raise ValueError(f"unexpected key in state dict: {extra[0]!r}")
    parts = []
    for k, shp in shapes.items():
        v = state[k]
        if tuple(v.shape) != shp:
            raise ValueError(f"state-dict entry {k!r} has shape {tuple(v.shape)}, the network needs {shp}")
        if not v.is_floating_point():
            raise ValueError(f"state-dict entry {k!r} has dtype {v.dtype}, expected a floating-point tensor")
        parts.append(v.detach().to(torch.float32).reshape(-1).numpy())
    return np.ascontiguousarray(np.concatenate(parts), dtype=np.float32)


def cache_key(spec: IkgatSpec, device) -> tuple:
    st = os.stat(spec.path)
    return (str(spec.path.resolve()), st.st_size, st.st_mtime_ns, spec.input_dim, spec.hidden_dim, spec.num_layers,
            spec.num_heads, spec.parents, str(device))


_networks: "OrderedDict[tuple, object]" = OrderedDict()


def network(spec: IkgatSpec, device):
    """The uploaded network of `spec` on `device`, read and uploaded once per checkpoint file state."""
    from ...native import NativeIkgat, require_device
    device = require_device(device)
    key = cache_key(spec, device)
    net = _networks.get(key)
    if net is not None:
        _networks.move_to_end(key)
        return net
    packed = pack_state(read_checkpoint(spec.path), spec)
    net = NativeIkgat(np.asarray(spec.parents, np.int32), packed, spec.input_dim, spec.hidden_dim, spec.num_layers,
                      spec.num_heads, device=device)
    for k in [k for k in _networks if k[0] == key[0] and k[-1] == key[-1]]:
        del _networks[k]                       # older states of the same file on this device
    _networks[key] = net
    while len(_networks) > _CACHE_SIZE:
        _networks.popitem(last=False)
    return net


def clear_cache() -> None:
    _networks.clear()


class IKGATEstimator:
    """Learned IK estimator: per-joint quaternions from 3D joints (reference ``inference.py:180-226``)."""

    def __init__(self, frame_config, device=None):
        self.spec = resolve(frame_config)
        self.net = network(self.spec, device)
        self.device = self.net.device

    @property
    def needs_quaternions(self) -> bool:
        return self.spec.input_dim == 9

    def _positions(self, j3d: torch.Tensor) -> torch.Tensor:
        J = self.spec.num_joints
        if j3d.dim() != 3 or j3d.shape[-1] != 3 or j3d.shape[1] != J:
            raise ValueError(f"IK-GAT: the joints have shape {tuple(j3d.shape)}, the network has {J} joints "
                             f"(len(ikgat_parent_ids)); expected (T, {J}, 3)")
        return j3d.detach().to(device=self.device, dtype=torch.float32).contiguous()

    def _quaternions(self, init_params: BodyModelParams) -> Optional[np.ndarray]:
        if not self.needs_quaternions:
            return None
        q = (getattr(init_params, "metadata", {}) or {}).get("ikgat_quaternions")
        if q is None:
            raise ValueError("ikgat model_type='pos-rot6_to_rot6' requires init_params.metadata['ikgat_quaternions']")
        q = q.detach().cpu().numpy() if isinstance(q, torch.Tensor) else np.asarray(q)
        if q.shape != (self.spec.num_joints, 4):
            raise ValueError(f"ikgat_quaternions has shape {q.shape}, expected ({self.spec.num_joints}, 4)")
        return np.ascontiguousarray(q, dtype=np.float32)

    def predict(self, positions: torch.Tensor, quats: Optional[np.ndarray], chain: bool = False) -> np.ndarray:
        """(T, J, 3) positions and (J, 4) input quaternions (broadcast over the frames; chain: frame 0's only) -> (T, J, 4)
        host float32 quaternions: one launch, one device-to-host copy."""
        T, J = positions.shape[0], self.spec.num_joints
        q = None
        if quats is not None:
            q = torch.as_tensor(quats).to(self.device)[None]
            q = q if chain else q.expand(T, J, 4).contiguous()
        return self.net.predict(positions, q, chain=chain).cpu().numpy()

    def predict_frames(self, positions: torch.Tensor, quats: Optional[torch.Tensor], chain: bool = False) -> torch.Tensor:
        """Device-level entry: (T, J, 3) positions and (T, J, 4) input quaternions -> (T, J, 4) device quaternions."""
        return self.net.predict(self._positions(positions), quats, chain=chain)

    def fit_frame(self, init_params: BodyModelParams, j3d: torch.Tensor, conf_3d: Optional[torch.Tensor], seq_ind: int,
                  target_model_indices: Optional[torch.Tensor] = None) -> BodyModelFitResult:
        del conf_3d, seq_ind, target_model_indices
        pos = self._positions(j3d[:1] if j3d.dim() == 3 else j3d)
        pred = self.predict(pos, self._quaternions(init_params))[0]
        return result_for(init_params, pred, j3d)


def result_for(init_params: BodyModelParams, quats: np.ndarray, j3d: torch.Tensor) -> BodyModelFitResult:
    """The reference's result object: params = init_params.detach() with a NEW metadata dict holding the predicted
    (J, 4) float32 quaternions; joints = vertices = the input frame; no loss (inference.py:216-226)."""
    meta = dict(getattr(init_params, "metadata", {}) or {})
    meta["ikgat_quaternions"] = quats
    params = init_params.detach()
    params.metadata = meta
    return BodyModelFitResult(params=params, joints=j3d.detach(), vertices=j3d.detach(), loss=None)
