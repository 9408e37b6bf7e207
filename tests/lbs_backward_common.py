"""Shared by the ``k2b_lbs_backward`` tests: small synthetic models with their CPU oracles (``oracle/smpl_torch.py`` in float64
and float32, ``torch.autograd.grad``), packed parameter sets with the two edge frames, and the gate.

Gate (per parameter group and frame): ``max|g_dev - g_64| <= tol * max|g_64|`` with ``tol = max(2e-5, 4 * e32)``: 2e-5 is the
project's analytic-gradient gate (``test_fit_gradient_matches_autograd``), e32 the same oracle's own float32-autograd error
against float64 on the case (the same statistic, its maximum over groups and frames), the factor 4 for another summation order
over up to 3 V terms."""
import functools
import re
from pathlib import Path

import numpy as np
import torch

from keypoints2body_amd import native, synthetic

REPO = Path(__file__).resolve().parents[1]
GROUPS = ("global_orient", "body_pose", "betas", "transl")
NUM_BETAS = {"smplx20": 10, "smplx26": 16}         # betas of the SMPL-X layouts (the rest: 10 expression coefficients)


def kernel_chunk() -> int:
    """Vertices per chunk of the dense backward kernel, read from its source."""
    src = (REPO / "keypoints2body_amd" / "csrc" / "k2b_lbs_backward.hip").read_text()
    return int(re.search(r"constexpr int kBwdChunk = (\d+);", src).group(1))


@functools.lru_cache(maxsize=None)
def consts(kind: str, V: int):
    if kind == "smpl":
        return synthetic.make_body_model(3, num_vertices=V)
    if kind == "smplh":
        return synthetic.make_body_model_h(3, num_vertices=V)
    return synthetic.make_body_model_x(3, num_vertices=V, num_shape=int(kind[5:]))


@functools.lru_cache(maxsize=None)
def landmarks(kind: str, V: int):
    """(vertex_ids [L,3], bary [L,3]) of the SMPL-X models, None for the others."""
    return synthetic.make_landmarks(num_vertices=V) if kind.startswith("smplx") else None


@functools.lru_cache(maxsize=None)
def oracle(kind: str, V: int, double: bool):
    from oracle.smpl_torch import TorchSMPL, TorchSMPLH, TorchSMPLX
    dt = torch.float64 if double else torch.float32
    c = consts(kind, V)
    if kind == "smpl":
        return TorchSMPL(c, dtype=dt)
    if kind == "smplh":
        return TorchSMPLH(c, dtype=dt)
    return TorchSMPLX(c, dtype=dt, num_betas=NUM_BETAS[kind])


@functools.lru_cache(maxsize=None)
def native_model(kind: str, V: int):
    c = consts(kind, V)
    return native.NativeModel(c.v_template, c.shapedirs, c.posedirs, c.J_regressor, c.lbs_weights, c.parents, c.extra_vertex_ids,
                              landmarks=landmarks(kind, V))


def fields(kind: str, B: int, seed: int) -> dict:
    """smplx keyword -> float32 array of B frames (``make_poses`` / ``make_poses_h`` / ``make_poses_x``)."""
    if kind == "smpl":
        p = synthetic.make_poses(B, seed)
        return dict(global_orient=p.global_orient, body_pose=p.body_pose, betas=p.betas, transl=p.transl)
    if kind == "smplh":
        p = synthetic.make_poses_h(B, seed)
        return dict(global_orient=p.global_orient, body_pose=p.body_pose, left_hand_pose=p.left_hand_pose,
                    right_hand_pose=p.right_hand_pose, betas=p.betas, transl=p.transl)
    p = synthetic.make_poses_x(B, seed)
    betas = p.betas if kind == "smplx20" else (0.5 * synthetic.normalish(47, (B, 16), seed)).astype(np.float32)
    return dict(global_orient=p.global_orient, body_pose=p.body_pose, jaw_pose=p.jaw_pose, leye_pose=p.leye_pose,
                reye_pose=p.reye_pose, left_hand_pose=p.left_hand_pose, right_hand_pose=p.right_hand_pose, betas=betas,
                expression=p.expression, transl=p.transl)


POSE_ORDER = ("body_pose", "jaw_pose", "leye_pose", "reye_pose", "left_hand_pose", "right_hand_pose")


def packed(kind: str, B: int, seed: int):
    """(global_orient, pose of all non-root joints, betas | expression, transl) as float32 arrays.  From three frames on, frame 1
    has an all-zero pose (the Rodrigues limit) and frame 2 a rotation of 2 rad (> pi / 2) about a seeded axis on every joint."""
    f = fields(kind, B, seed)
    go = f["global_orient"].copy()
    pose = np.concatenate([f[k] for k in POSE_ORDER if k in f], axis=1)
    shape = np.concatenate([f[k] for k in ("betas", "expression") if k in f], axis=1)
    if B >= 3:
        go[1] = 0.0
        pose[1] = 0.0
        axes = synthetic.normalish(60, (1 + pose.shape[1] // 3, 3), seed)
        axes = 2.0 * axes / np.sqrt((axes * axes).sum(axis=1, keepdims=True))
        go[2] = axes[0]
        pose[2] = axes[1:].reshape(-1)
    return go.astype(np.float32), pose.astype(np.float32), shape.astype(np.float32), f["transl"].copy()


def oracle_forward(kind: str, V: int, module, go, pose, shape, tr):
    """(joints (B,J+E+L,3), vertices (B,V,3)) of the oracle, the landmark rows combined from the translated vertices as
    ``k2b_lbs`` defines them."""
    joints, verts = module._lbs(torch.cat([go, pose], dim=1), shape, tr)
    lm = landmarks(kind, V)
    if lm is not None:
        ids = torch.as_tensor(lm[0].astype(np.int64))
        w = torch.as_tensor(lm[1]).to(verts.dtype)
        joints = torch.cat([joints, (verts[:, ids] * w[None, :, :, None]).sum(dim=2)], dim=1)
    return joints, verts


def oracle_grads(kind: str, V: int, params, cot_joints, cot_verts, double: bool, with_transl: bool = True):
    """``torch.autograd.grad`` of <cot_joints, joints> + <cot_verts, vertices> in the oracle; `params` as ``packed``.  Without
    a translation the forward gets none, and its gradient is that of a zero translation."""
    dt = torch.float64 if double else torch.float32
    leaves = [torch.tensor(np.asarray(p), dtype=dt, requires_grad=True) for p in params[:3]]
    tr = torch.tensor(np.asarray(params[3]) if with_transl else np.zeros_like(params[3]), dtype=dt, requires_grad=True)
    joints, verts = oracle_forward(kind, V, oracle(kind, V, double), *leaves, tr)
    loss = 0.0
    if cot_joints is not None:
        loss = loss + (torch.as_tensor(cot_joints).to(dt) * joints).sum()
    if cot_verts is not None:
        loss = loss + (torch.as_tensor(cot_verts).to(dt) * verts).sum()
    return dict(zip(GROUPS, torch.autograd.grad(loss, leaves + [tr])))


def group_error(got: dict, ref: dict) -> dict:
    """Per group: the largest ``max|got - ref| / max|ref|`` over the frames (a frame whose reference group is all zero
    counts its absolute error)."""
    out = {}
    for k in GROUPS:
        g, r = got[k].detach().cpu().double(), ref[k].detach().cpu().double()
        num = (g - r).abs().amax(dim=1)
        den = r.abs().amax(dim=1)
        out[k] = float(torch.where(den > 0, num / den.clamp_min(1e-300), num).max())
    return out


def gate(name: str, got: dict, g64: dict, g32: dict):
    """Print the measured figures, then assert the gate."""
    e32 = max(group_error(g32, g64).values())
    tol = max(2e-5, 4.0 * e32)
    err = group_error(got, g64)
    print(f"{name}: " + " ".join(f"{k}={v:.2e}" for k, v in err.items()) + f" max={max(err.values()):.2e} e32={e32:.2e} tol={tol:.2e}")
    for k, v in err.items():
        assert v <= tol, (name, k, v, tol)
