"""ORACLE (test infrastructure, not product code): CPU restatement of the IK-GAT rotation regressor in plain
PyTorch, float32 or float64, with every stage exposed.

Only ``tests/`` and ``tools/`` may import this module.  Pinned by ``tests/golden/ikgat_*.npz`` (the reference's own
public API on its demo motion, ``tools/gen_golden_ikgat.py``); ``tests/test_oracle_ikgat.py`` checks this restatement
against them, which is what lets ``tests/test_gpu_ikgat_oracle.py`` compare the HIP kernel with it on new inputs.

Written from the published formulations, one citation per step:

* graph            reference ``core/estimators/ikgat/gan_regressor.py:16-36``: both directions per parent link, the
                   ``i <-> i+1`` chain when no joint has a parent;
* GATConv          Velickovic et al., "Graph Attention Networks" (ICLR 2018), eq. 1-4, in PyG's ``GATConv`` form
                   (eval mode, ``concat=True``, ``add_self_loops=True``, no edge features): self loops removed then one
                   added per node, duplicates kept (no coalescing), ``softmax`` = exp(e - max) / (sum + 1e-16);
* network          ``gan_regressor.py:39-126``: input projection + joint embedding, L x (GAT, ELU, LayerNorm,
                   ``+ prev`` for l > 0), residual projection, head Linear - ReLU - LayerNorm - Linear(6);
* preprocess       ``inference.py:83-105`` and ``utils.py:8-26``: positions minus joint 0, quaternion xyzw -> 6-D (the
                   first two columns of its rotation matrix) after ``F.normalize`` (eps 1e-12);
* 6-D -> quat      Zhou et al., "On the Continuity of Rotation Representations in Neural Networks" (CVPR 2019),
                   eq. 15-16 (Gram-Schmidt), then the trace branch of Shepperd's matrix -> quaternion method (J. Guidance
                   and Control 1(3), 1978).  Follows what ``inference.py:39-43`` and ``utils.py:29-47`` compute: two
                   orthonormalisations, and 1e-8 both as the floor of 1 + trace and added to the divisor 4 w.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

NEGATIVE_SLOPE = 0.2        # PyG GATConv default
SOFTMAX_EPS = 1e-16         # torch_geometric.utils.softmax
LN_EPS = 1e-5               # nn.LayerNorm default
QUAT_EPS = 1e-8             # rot6_to_quat_torch's eps


# ---- graph ---------------------------------------------------------------------------------------------------------------
def skeleton_edges(parents: Sequence[int]) -> torch.Tensor:
    """(2, E) source/target pairs as the regressor builds them: parent -> child and child -> parent for every joint with
    a parent >= 0 (a self-parent gives two self loops), or the chain i <-> i+1 when there is no such joint."""
    edges = []
    for child, parent in enumerate(parents):
        if int(parent) >= 0:
            edges.append((int(parent), child))
            edges.append((child, int(parent)))
    if not edges:
        for i in range(len(parents) - 1):
            edges.append((i, i + 1))
            edges.append((i + 1, i))
    return torch.tensor(edges, dtype=torch.long).reshape(-1, 2).t().contiguous()


def with_self_loops(edge_index: torch.Tensor, num_nodes: int) -> torch.Tensor:
    """PyG's ``remove_self_loops`` then ``add_self_loops``: every i -> i edge dropped, one appended per node; duplicates of
    other edges stay (GATConv does not coalesce)."""
    src, dst = edge_index
    keep = src != dst
    loops = torch.arange(num_nodes, device=edge_index.device)
    return torch.stack([torch.cat([src[keep], loops]), torch.cat([dst[keep], loops])])


def message_edges(parents: Sequence[int]) -> torch.Tensor:
    """(2, E') edges one frame's GAT layers aggregate over."""
    return with_self_loops(skeleton_edges(parents), len(parents))


# ---- GATConv -------------------------------------------------------------------------------------------------------------
def gat_conv(x, edge_index, weight, att_src, att_dst, bias, heads: int, negative_slope: float = NEGATIVE_SLOPE,
             return_attention: bool = False):
    """x (N, H_in), weight (heads * C, H_in), att_* (1, heads, C), bias (heads * C) -> (N, heads * C)."""
    N, Hh = x.shape[0], heads
    C = weight.shape[0] // Hh
    xp = F.linear(x, weight).view(N, Hh, C)
    a_src = (xp * att_src).sum(-1)
    a_dst = (xp * att_dst).sum(-1)
    src, dst = with_self_loops(edge_index, N)
    e = F.leaky_relu(a_src[src] + a_dst[dst], negative_slope)
    emax = torch.full((N, Hh), -float("inf"), dtype=e.dtype).scatter_reduce(0, dst[:, None].expand(-1, Hh), e, "amax")
    ex = (e - emax[dst]).exp()
    den = torch.zeros((N, Hh), dtype=e.dtype).index_add(0, dst, ex) + SOFTMAX_EPS
    alpha = ex / den[dst]
    out = torch.zeros((N, Hh, C), dtype=x.dtype).index_add(0, dst, alpha[..., None] * xp[src])
    out = out.reshape(N, Hh * C) + bias
    return (out, (src, dst, alpha)) if return_attention else out


class GATConv(nn.Module):
    """PyG ``GATConv`` restated (eval mode) with its parameter names, so the reference's ``load_state_dict`` fills it:
    x' = x W^T; a_src / a_dst = <x'_h, att_h>; self loops removed then one added per node;
    e_ji = LeakyReLU_0.2(a_src[j] + a_dst[i]); softmax over the edges entering i with PyG's exp(e - max) / (sum + 1e-16);
    out_i = sum_j alpha_ji x'_j, heads concatenated, + bias."""

    def __init__(self, in_channels, out_channels, heads=1, dropout=0.0, concat=True, negative_slope=NEGATIVE_SLOPE):
        super().__init__()
        assert concat
        self.heads, self.out_channels, self.negative_slope = heads, out_channels, negative_slope
        self.lin = nn.Linear(in_channels, heads * out_channels, bias=False)
        self.att_src = nn.Parameter(torch.empty(1, heads, out_channels))
        self.att_dst = nn.Parameter(torch.empty(1, heads, out_channels))
        self.bias = nn.Parameter(torch.empty(heads * out_channels))

    def forward(self, x, edge_index):
        return gat_conv(x, edge_index, self.lin.weight, self.att_src, self.att_dst, self.bias, self.heads, self.negative_slope)


# ---- rotations -----------------------------------------------------------------------------------------------------------
def quat_to_rot6(q: torch.Tensor) -> torch.Tensor:
    """(..., 4) xyzw, any norm -> (..., 6): columns 1 and 2 of the rotation matrix of q / max(|q|, 1e-12)."""
    x, y, z, w = F.normalize(q, p=2.0, dim=-1).unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y + z * w), 2 * (x * z - y * w),
                        2 * (x * y - z * w), 1 - 2 * (x * x + z * z), 2 * (y * z + x * w)], dim=-1)


def _unit(v: torch.Tensor) -> torch.Tensor:
    """v / max(|v|, 1e-12) along the last axis (``F.normalize``'s clamp)."""
    return F.normalize(v, p=2.0, dim=-1, eps=1e-12)


def axes_to_rot6(raw: torch.Tensor) -> torch.Tensor:
    """(..., 6) two raw axes u, v -> the Gram-Schmidt pair (e1, e2) of Zhou et al. eq. 15-16:
    e1 = N(u), e2 = N(v - <e1, v> e1), N = ``_unit``."""
    u, v = raw.split(3, dim=-1)
    e1 = _unit(u)
    proj = (e1 * v).sum(dim=-1, keepdim=True)
    return torch.cat([e1, _unit(v - proj * e1)], dim=-1)


def rot6_to_quat(rot6: torch.Tensor) -> torch.Tensor:
    """(..., 6) -> unit quaternion xyzw with qw >= 0.  The pair is orthonormalised once more (the reference does it in both
    of its steps), e3 = e1 x e2 completes the rotation matrix with e1, e2, e3 as COLUMNS, and the quaternion follows from
    the trace branch of the matrix -> quaternion conversion alone (Shepperd's w-branch, no switch on the largest diagonal
    term):  w = sqrt(max(1 + tr, 1e-8)) / 2,  (x, y, z) = (e2z - e3y, e3x - e1z, e1y - e2x) / (4 w + 1e-8),  then
    normalised.  Written per component, like ``rot6_to_quat`` in csrc/k2b_ikgat.hip."""
    e = axes_to_rot6(rot6)
    e1x, e1y, e1z, e2x, e2y, e2z = e.unbind(-1)
    # the library's cross product, not three written-out differences of products: it rounds differently in the last bit
    # (fused multiply-add), and with it the float32 oracle reproduces the reference's recorded float32 run bit for bit
    e3x, e3y, e3z = torch.linalg.cross(e[..., :3], e[..., 3:], dim=-1).unbind(-1)
    tr = e1x + e2y + e3z
    w = 0.5 * (1.0 + tr).clamp_min(QUAT_EPS).sqrt()
    scale = 4.0 * w + QUAT_EPS
    return _unit(torch.stack([(e2z - e3y) / scale, (e3x - e1z) / scale, (e1y - e2x) / scale, w], dim=-1))


def raw_to_quat(raw: torch.Tensor) -> torch.Tensor:
    """The head's 6 outputs -> quaternion: ``axes_to_rot6`` then ``rot6_to_quat`` (so two orthonormalisations, as the reference)."""
    return rot6_to_quat(axes_to_rot6(raw))


# ---- the regressor -------------------------------------------------------------------------------------------------------
class IkgatOracle:
    """The regressor with the weights of a ``synthetic.make_ikgat_state`` state dict (numpy arrays or tensors; the GAT
    projection as ``lin.weight`` or as older PyG's ``lin_src.weight`` + ``lin_dst.weight``), evaluated in ``dtype``.
    The weights are the float32 values cast to ``dtype``: float64 adds precision of evaluation, not of the constants."""

    def __init__(self, state: dict, parents: Sequence[int], dtype: torch.dtype = torch.float64):
        self.dtype = dtype
        self.parents = [int(p) for p in parents]
        self.J = len(self.parents)
        w = {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in state.items()}
        self.L = 1 + max(int(k.split(".")[1]) for k in w if k.startswith("layer_norms."))
        for l in range(self.L):
            src, dst, lin = (f"gat_layers.{l}.{n}.weight" for n in ("lin_src", "lin_dst", "lin"))
            if lin not in w:
                if not torch.equal(w[src], w[dst]):
                    raise ValueError(f"{src!r} and {dst!r} differ: the regressor's GAT layers share one projection")
                w[lin] = w[src]
        self.w = w
        self.heads = int(w["gat_layers.0.att_src"].shape[1])
        self.H = int(w["input_proj.weight"].shape[0])
        self.IN = int(w["input_proj.weight"].shape[1])
        self.edge_index = skeleton_edges(self.parents)

    # -- stages
    def preprocess(self, positions, quaternions=None) -> torch.Tensor:
        """(B, J, 3) [+ (B, J, 4) xyzw] -> network input (B, J, IN): root-relative positions [| 6-D rotation]."""
        pos = torch.as_tensor(np.asarray(positions)).to(self.dtype)
        x = pos - pos[:, 0:1]
        if self.IN == 9:
            if quaternions is None:
                raise ValueError("quaternions are required for the pos-rot6 network")
            x = torch.cat([x, quat_to_rot6(torch.as_tensor(np.asarray(quaternions)).to(self.dtype))], dim=-1)
        return x

    def embed(self, x: torch.Tensor) -> torch.Tensor:
        w = self.w
        return F.linear(x, w["input_proj.weight"], w["input_proj.bias"]) + w["joint_pos_embed.weight"][None]

    def batch_edges(self, B: int) -> torch.Tensor:
        return torch.cat([self.edge_index + b * self.J for b in range(B)], dim=1)

    def gat_layer(self, l: int, nodes: torch.Tensor, edges: torch.Tensor) -> Dict[str, torch.Tensor]:
        """One block on flattened nodes (B * J, H): ``conv`` (GATConv incl. bias), ``elu``, ``norm``, ``out`` (+ prev)."""
        w = self.w
        conv = gat_conv(nodes, edges, w[f"gat_layers.{l}.lin.weight"], w[f"gat_layers.{l}.att_src"],
                        w[f"gat_layers.{l}.att_dst"], w[f"gat_layers.{l}.bias"], self.heads)
        elu = F.elu(conv)
        norm = F.layer_norm(elu, (self.H,), w[f"layer_norms.{l}.weight"], w[f"layer_norms.{l}.bias"], LN_EPS)
        return {"conv": conv, "elu": elu, "norm": norm, "out": norm + nodes if l > 0 else norm}

    def head(self, h: torch.Tensor) -> Dict[str, torch.Tensor]:
        w = self.w
        hid = F.relu(F.linear(h, w["output_head.0.weight"], w["output_head.0.bias"]))
        ln = F.layer_norm(hid, (self.H // 2,), w["output_head.2.weight"], w["output_head.2.bias"], LN_EPS)
        return {"hidden": hid, "hidden_norm": ln, "raw": F.linear(ln, w["output_head.4.weight"], w["output_head.4.bias"])}

    # -- end to end
    @torch.no_grad()
    def stages(self, positions, quaternions=None) -> Dict[str, torch.Tensor]:
        """Every intermediate of B independent frames, (B, J, ...) each; ``quat`` is the result."""
        x = self.preprocess(positions, quaternions)
        B = x.shape[0]
        out = {"x": x, "h0": self.embed(x)}
        nodes, edges = out["h0"].reshape(B * self.J, self.H), self.batch_edges(B)
        for l in range(self.L):
            st = self.gat_layer(l, nodes, edges)
            nodes = st["out"]
            for k, v in st.items():
                out[f"gat{l}.{k}"] = v.view(B, self.J, self.H)
        out["residual"] = F.linear(x, self.w["residual_proj.weight"], self.w["residual_proj.bias"])
        out["trunk"] = nodes.view(B, self.J, self.H) + out["residual"]
        out.update(self.head(out["trunk"]))
        out["rot6"] = axes_to_rot6(out["raw"])
        out["quat"] = rot6_to_quat(out["rot6"])
        return out

    def forward(self, positions, quaternions=None) -> np.ndarray:
        """(B, J, 3) [+ (B, J, 4)] -> (B, J, 4) xyzw, as a numpy array of ``dtype``."""
        if len(positions) == 0:
            return np.zeros((0, self.J, 4), dtype=torch.empty(0, dtype=self.dtype).numpy().dtype)
        return self.stages(positions, quaternions)["quat"].numpy()

    __call__ = forward

    def chain(self, positions, q0) -> np.ndarray:
        """Warm-started sequence: frame 0 reads ``q0`` (J, 4), frame t + 1 reads frame t's output quaternions."""
        q, out = np.asarray(q0), []
        for t in range(len(positions)):
            q = self.forward(np.asarray(positions)[t: t + 1], q[None])[0]
            out.append(q)
        return np.stack(out) if out else np.zeros((0, self.J, 4))


def forward_pair(state: dict, parents: Sequence[int], positions, quaternions=None) -> Tuple[np.ndarray, np.ndarray]:
    """(q64, q32): the same inputs through the float64 and the float32 oracle."""
    return (IkgatOracle(state, parents, torch.float64)(positions, quaternions),
            IkgatOracle(state, parents, torch.float32)(positions, quaternions))
