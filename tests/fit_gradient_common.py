"""Shared by the fit kernels' gradient tests (``k2b_fit.hip``, ``k2b_fit_tree.hip``): small synthetic models with their CPU oracles
(``oracle/smpl_torch.py`` forward and ``oracle.fit_torch.frame_losses`` in float64 and float32, ``torch.autograd.grad``, plus the
translation prior ``w_t^2 |transl - target|^2`` of ``k2b.h``), the cases, the evaluate-only device call and the gate.

Gate, per parameter group and frame: ``max|g_dev - g_64| <= tol_k * max|g_64|``, both maxima over that group in that frame, with
``tol_k = max(2e-5, 4 * e32_k)``: 2e-5 is the project's analytic-gradient gate (``test_fit_gradient_matches_autograd``), ``e32_k``
the same statistic of the float32 oracle against the float64 one for that group (its maximum over the case's frames), the factor 4
the one ``tests/lbs_backward_common.py`` allows for another summation order.  A group that is identically zero in float64 (a term
that does not touch it, fingers without targets) is measured against the largest entry of that frame's whole float64 gradient;
a group outside the optimiser (``optimize_mask``, ``freeze_betas``) must be exactly zero.  The loss per frame:
``|loss_dev - loss_64| <= max(2e-6, 4 * e32_loss) * |loss_64|``.

Conditions on the inputs (asserted, so that a badly chosen case cannot loosen its own gate, and computed from the oracle alone):
``e32_k <= 1e-4`` for every group of every case, and one float32 rounding of the target coordinates moves no group of the float64
gradient by more than an eighth of 2e-5 (ROUNDING_LIMIT below).  ``tests/test_fit_gradient_conditions.py`` checks both for all
cases without a GPU.

Root rotations of several turns (``turn_case``, TURNS = 6.5 .. 5000 rad) have a gate of their own, ``turn_gate``: the group gate per
frame, widened by what two ulp of the float32 angle do to the float64 gradient.

Groups: global_orient, body_pose, betas, transl; SMPL-H and SMPL-X split the pose into body | (face) | hands and SMPL-X the shape
coefficients into betas | expression."""
import copy
import functools
from dataclasses import dataclass, field, replace
from typing import Optional

import numpy as np
import torch

from keypoints2body_amd import synthetic
from tests import helpers as H

GRAD_GATE = 2e-5           # tests/test_gpu_parity.py::test_fit_gradient_matches_autograd
LOSS_GATE = 2e-6
ORDER_FACTOR = 4.0         # tests/lbs_backward_common.py
E32_LIMIT = 1e-4           # condition on the inputs
# Second condition on the inputs.  A float32 forward rounds every coordinate it forms (joint, joint + transl, minus target) to
# half an ulp of that coordinate, and the joint term's gradient is the residual times a constant: a case whose targets lie
# close to the joints but far from the origin turns those roundings into gradient error whatever the kernel does.  So, in
# float64 alone: moving every target coordinate by half its float32 ulp may change no group by more than an eighth of the gate
# (a forward chain, the translation, the residual and the backward sums are a handful of such roundings).  TRANSL_SCALE and
# TARGET_OFFSET are chosen for it: coordinates within about a metre (ulp 6e-8 .. 1.2e-7), residuals of about 12 cm per axis.
ROUNDING_LIMIT = GRAD_GATE / 8.0
TRANSL_SCALE, TARGET_OFFSET = 0.2, 0.12
MODEL_SEED = 3
SMPLX_BETAS = {20: 10, 32: 22}                    # shape coefficients -> betas (the rest: 10 expression coefficients)
LADDER = (0.0, 1e-6, 1e-3, 1.0, 2.0, 3.0, 3.1415, 3.3)
# Rotation vectors of several turns (legal input; optimisers produce them), on the root only: it is outside the pose prior, so
# every group keeps the scale of the joint term.  999 / 1001 straddle the branch of ``sincos_small`` (csrc/k2b_device.h) that hands
# angles above 1e3 rad to the library functions.  ``turn_case``, ``turn_gate``.
TURNS = (6.5, 20.0, 100.0, 999.0, 1001.0, 5000.0)
TURN_SHARP = 20.0          # up to this angle a turned frame is held as sharply as every other frame
TURN_ULPS = 2.0            # a float32 kernel forms the angle with a sum of squares and a square root: two roundings
GMOF_SIGMA = 0.05
GMOF_RESIDUALS = (0.01, 0.03, 0.05, 0.1, 0.3, 1.0)       # metres: below, at and far above sigma
CONF_PATTERN = (0.0, 0.5, 1.0, 2.5, 1.5)
TERMS = ("joint", "mixture", "bending", "shape", "preserve", "transl")
# every loss weight of k2b_fit_config (sigma is the GMoF scale); "transl" is the translation prior, built for 24 joints only
ALL_ON = dict(sigma=100.0, joint=600.0, mixture=4.78 * 1.5, bending=15.2, shape=5.0, preserve=5.0, transl=100.0)

# Odd trees for the tree kernel.  Its entry (k2b_fit_rules.h, shared_path) takes up to 63 joints, targeted joints down to depth 15
# (four pointer-doubling rounds) and a prior over the first 3..63 pose dimensions that hold the bending prior's indices (up to 55).
TREES = {
    # 21 joints, 60 pose dimensions (all of them under the prior), junctions at the root, inside limbs and a three-way one at 7
    "tree21": [-1, 0, 0, 1, 1, 2, 2, 3, 4, 5, 6, 7, 7, 7, 8, 9, 10, 11, 12, 13, 14],
    # 26 joints: a chain 0 .. 15 (depth 15, the limit) with side branches, one of them ending at depth 15 too
    "tree26": [-1] + list(range(15)) + [3, 16, 7, 18, 19, 11, 0, 22, 14, 5],
    # the same with a joint at depth 16: refused when that joint is targeted
    "tree27": [-1] + list(range(15)) + [3, 16, 7, 18, 19, 11, 0, 22, 14, 5, 15],
    # one joint more than the entry takes (the model itself may have up to 64), three children per joint: refused
    "tree64": [-1] + [(j - 1) // 3 for j in range(1, 64)],
}
TREE_DEPTH_LIMIT, TREE_JOINT_LIMIT, TREE_PRIOR_LIMIT = 15, 63, 63


def tree_limits_in_source():
    """(joints, depth, prior dimensions) the tree kernel's entry accepts, read from its own checks."""
    import re
    from pathlib import Path
    src = (Path(__file__).resolve().parents[1] / "keypoints2body_amd" / "csrc" / "k2b_fit_rules.h").read_text()
    m = re.search(r"\(f\.J > (\d+) \|\| rounds_for_depth\(max_depth\) > (\d+)\)", src)
    p = re.search(r"prior_dims < 3 \|\| el\.prior_dims > (\d+) \|\| el\.prior_dims % 3 != 0", src)
    return int(m.group(1)), 2 ** int(m.group(2)) - 1, int(p.group(1)) // 3 * 3


def tree_depth(parents) -> int:
    d = [0] * len(parents)
    for j in range(1, len(parents)):
        d[j] = d[parents[j]] + 1
    return max(d)


@dataclass(frozen=True)
class Layout:
    kernel: str             # "fused" (k2b_fit.hip) or "tree" (k2b_fit_tree.hip)
    J: int
    NB: int
    prior_dims: int         # pose dimensions the mixture, the bending prior and the preserve term see
    betas_prior: int        # coefficients under the shape prior and freeze_betas
    cfg_prior_dims: int     # k2b_fit_config.prior_pose_dims / num_betas_prior that say so
    cfg_betas_prior: int
    groups: tuple           # (name, first column, end column) in the packed row [global_orient | pose | shape | transl]

    @property
    def D(self):
        return 3 * (self.J - 1)

    @property
    def P(self):
        return 3 + self.D + self.NB + 3


@functools.lru_cache(maxsize=None)
def layout(kind: str) -> Layout:
    if kind.startswith("smplx"):
        NB = int(kind[5:])
        nb = SMPLX_BETAS[NB]
        s = 3 + 162
        groups = (("global_orient", 0, 3), ("body", 3, 66), ("face", 66, 75), ("hands", 75, 165), ("betas", s, s + nb),
                  ("expression", s + nb, s + NB), ("transl", s + NB, s + NB + 3))
        return Layout("tree", 55, NB, 63, nb, 63, nb, groups)
    if kind == "smplh":
        s = 3 + 153
        groups = (("global_orient", 0, 3), ("body", 3, 66), ("hands", 66, 156), ("betas", s, s + 10), ("transl", s + 10, s + 13))
        return Layout("tree", 52, 10, 63, 10, 63, 10, groups)
    J, NB = (len(TREES[kind]), 10) if kind in TREES else (24, int(kind[4:]))
    D = 3 * (J - 1)
    groups = (("global_orient", 0, 3), ("body_pose", 3, 3 + D), ("betas", 3 + D, 3 + D + NB), ("transl", 3 + D + NB, 3 + D + NB + 3))
    if kind in TREES:
        return Layout("tree", J, NB, min(D, 63), NB, 0 if D <= 63 else 63, 0, groups)
    return Layout("fused", J, NB, D, NB, 0, 0, groups)


def tree_rest(kind: str) -> np.ndarray:
    parents = TREES[kind]
    step = synthetic.normalish(78, (len(parents), 3), MODEL_SEED)
    step = 0.12 * step / np.sqrt((step * step).sum(axis=1, keepdims=True))
    rest = np.zeros((len(parents), 3))
    rest[0] = (0.0, -0.2, 0.0)
    for j in range(1, len(parents)):
        rest[j] = rest[parents[j]] + step[j]
    return rest


@functools.lru_cache(maxsize=None)
def consts(kind: str):
    """A few hundred vertices: the fit kernels never read vertices, only the oracle's forward does."""
    if kind.startswith("smplx"):
        return synthetic.make_body_model_x(MODEL_SEED, num_vertices=660, num_shape=int(kind[5:]))
    if kind == "smplh":
        return synthetic.make_body_model_h(MODEL_SEED, num_vertices=624)
    if kind in TREES:
        parents = np.asarray(TREES[kind], dtype=np.int32)
        return synthetic.make_body_model(MODEL_SEED, num_vertices=12 * len(parents), num_betas=10, parents=parents, rest=tree_rest(kind),
                                         num_extra=0)
    return synthetic.make_body_model(MODEL_SEED, num_vertices=512, num_betas=int(kind[4:]))


@functools.lru_cache(maxsize=None)
def oracle(kind: str, double: bool):
    from oracle.smpl_torch import TorchSMPL, TorchSMPLH, TorchSMPLX
    dt = torch.float64 if double else torch.float32
    if kind.startswith("smplx"):
        return TorchSMPLX(consts(kind), dtype=dt, num_betas=SMPLX_BETAS[int(kind[5:])])
    if kind == "smplh":
        return TorchSMPLH(consts(kind), dtype=dt)
    return TorchSMPL(consts(kind), dtype=dt)


@functools.lru_cache(maxsize=None)
def prior(double: bool):
    """The fixture prior, its buffers cast to the oracle's type."""
    p = H.oracle_prior()
    if double:
        p = copy.copy(p)
        p.means, p.precisions, p.nll_weights = p.means.double(), p.precisions.double(), p.nll_weights.double()
    return p


@functools.lru_cache(maxsize=None)
def native_model(kind: str):
    from keypoints2body_amd.native import NativeModel
    c = consts(kind)
    return NativeModel(c.v_template, c.shapedirs, c.posedirs, c.J_regressor, c.lbs_weights, c.parents, c.extra_vertex_ids)


# ---- cases -------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True, eq=False)
class Case:
    name: str
    kind: str
    idx: tuple                          # model joint per target
    j3d: np.ndarray                     # [B][K][3]
    go: np.ndarray
    pose: np.ndarray                    # all non-root joints
    shape: np.ndarray                   # betas | expression
    tr: np.ndarray
    weights: dict = field(default_factory=lambda: dict(ALL_ON))
    conf: Optional[np.ndarray] = None   # None, [K] or [B][K] (then conf_per_frame = 1)
    preserve: Optional[np.ndarray] = None
    tr_target: Optional[np.ndarray] = None
    mask: int = 15
    freeze: int = 0

    @property
    def frames(self):
        return self.j3d.shape[0]


def only(term: str, **more) -> dict:
    """Every loss weight zero but one."""
    w = {k: 0.0 for k in ALL_ON}
    w["sigma"] = ALL_ON["sigma"]
    w[term] = ALL_ON[term]
    w.update(more)
    return w


def all_on(kind: str, **more) -> dict:
    w = dict(ALL_ON)
    if layout(kind).kernel == "tree":
        w["transl"] = 0.0                # not built there
    w.update(more)
    return w


def joints64(kind: str, go, pose, shape, tr) -> np.ndarray:
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    with torch.no_grad():
        j, _ = oracle(kind, True)._lbs(torch.cat([t(go), t(pose)], dim=1), t(shape), t(tr))
    return j[:, :layout(kind).J].numpy()


@functools.lru_cache(maxsize=None)
def base(kind: str, B: int = 17, seed: int = 11, num_targets: int = 0) -> Case:
    """B seeded frames: pose ~ 0.2 rad (root 0.3, fingers and face 0.15), shape ~ 0.5, transl ~ 0.2 m, targets 12 cm off the model's joints, a
    preserve pose 0.05 rad and (24-joint kernel) a translation-prior centre about 0.1 m off.  `num_targets`: the first joints (0 = all)."""
    lay = layout(kind)
    f = lambda stream, cols, scale: (scale * synthetic.normalish(stream, (B, cols), seed)).astype(np.float32)
    go, pose, shape, tr = f(70, 3, 0.3), f(71, lay.D, 0.2), f(72, lay.NB, 0.5), f(73, 3, TRANSL_SCALE)
    pose[:, 63:] *= 0.75
    K = num_targets or lay.J
    j3d = (joints64(kind, go, pose, shape, tr)[:, :K] + TARGET_OFFSET * synthetic.normalish(74, (B, K, 3), seed)).astype(np.float32)
    # (the tree kernel's entry refuses a translation-prior centre as it refuses the weight)
    return Case(f"{kind}/base{K}", kind, tuple(range(K)), j3d, go, pose, shape, tr, all_on(kind), preserve=pose + f(75, lay.D, 0.05),
                tr_target=tr + f(76, 3, 0.06) if lay.kernel == "fused" else None)


def term_case(kind: str, term: str, num_targets: int = 0) -> Case:
    b = base(kind, num_targets=num_targets)
    return replace(b, name=f"{b.name}/{term}", weights=all_on(kind) if term == "all" else only(term))


@functools.lru_cache(maxsize=None)
def ladder_case(kind: str) -> Case:
    """Frame 0: the joints, root included, cycle through the angles of LADDER about seeded axes; frame 1: all zero."""
    lay = layout(kind)
    b = base(kind, B=2, seed=13)
    axes = synthetic.normalish(77, (lay.J, 3), 13)
    axes = axes / np.sqrt((axes * axes).sum(axis=1, keepdims=True))
    full = np.zeros((2, lay.J, 3))
    full[0] = axes * np.asarray([LADDER[j % len(LADDER)] for j in range(lay.J)])[:, None]
    go, pose = full[:, 0].astype(np.float32), full[:, 1:].reshape(2, -1).astype(np.float32)
    j3d = (joints64(kind, go, pose, b.shape, b.tr) + TARGET_OFFSET * synthetic.normalish(74, (2, lay.J, 3), 13)).astype(np.float32)
    return replace(b, name=f"{kind}/ladder", j3d=j3d, go=go, pose=pose, preserve=pose + (b.preserve - b.pose))


@functools.lru_cache(maxsize=None)
def gmof_case(kind: str, term: str) -> Case:
    """Sigma 0.05 m and residuals of 0.01 .. 1 m, both signs; target 5 of frame 0 sits exactly on its joint.  The body is centred
    on the origin and the residuals grow with the joint's distance from it (the three components of a joint take three
    neighbouring sizes): a residual of 1 cm on a coordinate of a metre would be lost in that coordinate's float32 rounding."""
    lay = layout(kind)
    b = base(kind, B=3, seed=17)
    tr = (b.tr - joints64(kind, b.go, b.pose, b.shape, b.tr).mean(axis=1)).astype(np.float32)
    now = joints64(kind, b.go, b.pose, b.shape, tr)
    rank = np.argsort(np.argsort(np.abs(now).max(axis=2), axis=1), axis=1)                    # [3][J]: 0 = nearest to the origin
    size = rank[:, :, None] * (len(GMOF_RESIDUALS) - 2) // lay.J + np.arange(3)[None, None, :]               # 0 .. 5
    f, k, c = np.meshgrid(np.arange(3), np.arange(lay.J), np.arange(3), indexing="ij")
    r = np.asarray(GMOF_RESIDUALS)[size] * np.where((f + k + c) % 2 == 0, 1.0, -1.0)
    r[0, 5] = 0.0
    w = all_on(kind, sigma=GMOF_SIGMA) if term == "all" else only(term, sigma=GMOF_SIGMA)
    return replace(b, name=f"{kind}/gmof/{term}", j3d=(now - r).astype(np.float32), tr=tr, tr_target=None if b.tr_target is None else tr + (b.tr_target - b.tr),
                   weights=w)


@functools.lru_cache(maxsize=None)
def conf_case(kind: str, per_frame: bool, removed: bool = False) -> Case:
    """Confidences with zeros and values above 1, shared ([K]) or a per-frame table ([B][K]) whose rows differ.  Every target of
    confidence zero is moved a metre off: it must contribute nothing.  `removed`: the same call without the targets whose
    confidence is zero in every frame (the oracle's result is the same)."""
    lay = layout(kind)
    b = base(kind, B=3, seed=19)
    K = lay.J
    pat = np.asarray(CONF_PATTERN, dtype=np.float32)
    conf = np.stack([pat[(np.arange(K) + 2 * r) % len(pat)] for r in range(3)]) if per_frame else pat[np.arange(K) % len(pat)]
    if per_frame:
        conf[:, 3] = 0.0
    table = conf if per_frame else np.broadcast_to(conf, (3, K))
    j3d = b.j3d.copy()
    j3d[table == 0.0] += np.float32(1.0)
    keep = np.arange(K)
    if removed:
        keep = np.flatnonzero((table != 0.0).any(axis=0))
        assert 0 < len(keep) < K
    return replace(b, name=f"{kind}/conf/{'table' if per_frame else 'shared'}{'/removed' if removed else ''}", idx=tuple(int(k) for k in keep),
                   j3d=np.ascontiguousarray(j3d[:, keep]), conf=np.ascontiguousarray(conf[..., keep]))


@functools.lru_cache(maxsize=None)
def turn_case(kind: str) -> Case:
    """Frame f: the root turned by TURNS[f] rad about a seeded axis, everything else as ``base``."""
    n = len(TURNS)
    b = base(kind, B=n, seed=37)
    axes = synthetic.normalish(81, (n, 3), 37)
    axes = axes / np.sqrt((axes * axes).sum(axis=1, keepdims=True))
    go = (axes * np.asarray(TURNS)[:, None]).astype(np.float32)
    j3d = (joints64(kind, go, b.pose, b.shape, b.tr) + TARGET_OFFSET * synthetic.normalish(74, (n, layout(kind).J, 3), 37)).astype(np.float32)
    return replace(b, name=f"{kind}/turns", j3d=j3d, go=go)


def member_case(kind: str, mask: int, freeze: int) -> Case:
    b = base(kind, B=3, seed=23)
    return replace(b, name=f"{kind}/mask{mask}{'/frozen' if freeze else ''}", mask=mask, freeze=freeze)


@functools.lru_cache(maxsize=None)
def mixture_case(kind: str, term: str) -> Case:
    """Frame m sits near the mean of component m of the fixture prior (its first prior dimensions), 0.02 rad of seeded noise."""
    lay = layout(kind)
    means = H.gmm_fixture()["ref_means"]
    M = means.shape[0]
    b = base(kind, B=M, seed=29)
    pose = b.pose.copy()
    pose[:, :lay.prior_dims] = means[:, :lay.prior_dims] + (0.02 * synthetic.normalish(79, (M, lay.prior_dims), 29)).astype(np.float32)
    j3d = (joints64(kind, b.go, pose, b.shape, b.tr) + TARGET_OFFSET * synthetic.normalish(74, (M, lay.J, 3), 29)).astype(np.float32)
    return replace(b, name=f"{kind}/mixture/{term}", j3d=j3d, pose=pose, preserve=pose + (b.preserve - b.pose),
                   weights=all_on(kind) if term == "all" else only(term))


def mixture_selection(case: Case):
    """(component selected per frame, gap between the best two values / |best|) in float64."""
    lay = layout(case.kind)
    with torch.no_grad():
        vals = prior(True).per_component(torch.tensor(case.pose[:, :lay.prior_dims], dtype=torch.float64))
    two = torch.topk(vals, 2, dim=1, largest=False).values
    return vals.argmin(dim=1).numpy(), ((two[:, 1] - two[:, 0]) / two[:, 0].abs()).numpy()


# ---- oracle ------------------------------------------------------------------------------------------------------------------
def excluded_columns(case: Case) -> np.ndarray:
    """[P] bool: columns of the packed gradient outside the optimiser."""
    lay = layout(case.kind)
    D, NB = lay.D, lay.NB
    out = np.zeros(lay.P, dtype=bool)
    out[0:3] = not case.mask & 1
    out[3:3 + D] = not case.mask & 2
    out[3 + D:3 + D + NB] = not case.mask & 4
    if case.freeze:
        out[3 + D:3 + D + lay.betas_prior] = True
    out[3 + D + NB:] = not case.mask & 8
    return out


def oracle_eval(case: Case, double: bool):
    """(loss [B], gradient [B][P]) of the fit loss by autograd through the oracle, as float64 arrays; excluded columns zero.
    On one thread: the float32 sums, and with them e32 and the gate, do not depend on how many cores the machine offers."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return _oracle_eval(case, double)
    finally:
        torch.set_num_threads(threads)


def _oracle_eval(case: Case, double: bool):
    from oracle.fit_torch import FitWeights, frame_losses
    lay = layout(case.kind)
    dt = torch.float64 if double else torch.float32
    t = lambda a: torch.tensor(np.asarray(a), dtype=dt)
    w = {k: float(np.float32(v)) for k, v in case.weights.items()}          # the values the device reads from its float config
    go, pose, shape, tr = leaves = [t(a).requires_grad_() for a in (case.go, case.pose, case.shape, case.tr)]
    joints, _ = oracle(case.kind, double)._lbs(torch.cat([go, pose], dim=1), shape, tr)
    fw = FitWeights(sigma=w["sigma"], pose_prior_weight=w["mixture"], shape_prior_weight=w["shape"], angle_prior_weight=w["bending"],
                    joint_loss_weight=w["joint"], pose_preserve_weight=w["preserve"])
    Dp = lay.prior_dims
    preserve = t(case.pose if case.preserve is None else case.preserve)[:, :Dp]
    conf = torch.ones(len(case.idx), dtype=dt) if case.conf is None else t(case.conf)
    lf = frame_losses(pose[:, :Dp], preserve, shape[:, :lay.betas_prior], joints[:, list(case.idx)], t(case.j3d), prior(double), conf, fw,
                      preserve_on=True)
    target = t(case.tr if case.tr_target is None else case.tr_target)
    lf = lf + (w["transl"] ** 2) * ((tr - target) ** 2).sum(dim=-1)         # k2b.h: w_t^2 |transl - transl_prior_target|^2
    grads = torch.autograd.grad(lf.sum(), leaves)
    g = torch.cat(grads, dim=1).double().numpy()
    g[:, excluded_columns(case)] = 0.0
    return lf.detach().double().numpy(), g


def group_errors(got: np.ndarray, ref: np.ndarray, lay: Layout) -> dict:
    """Per group: [B] values ``max|got - ref| / max|ref|`` over the group; where the reference group is all zero, over the largest
    entry of that frame's whole reference gradient (and the absolute error where that is zero too)."""
    whole = np.abs(ref).max(axis=1)
    out = {}
    for name, a, b in lay.groups:
        num = np.abs(got[:, a:b] - ref[:, a:b]).max(axis=1)
        den = np.abs(ref[:, a:b]).max(axis=1)
        den = np.where(den > 0, den, whole)
        out[name] = np.where(den > 0, num / np.where(den > 0, den, 1.0), num)
    return out


def rounding_sensitivity(case: Case, g64: np.ndarray) -> dict:
    """Per group: the largest change (``group_errors``' statistic) of the float64 gradient when every target coordinate moves by
    half its float32 ulp, seeded signs."""
    sign = np.where(synthetic.uniform(80, case.j3d.size, 31).reshape(case.j3d.shape) < 0.5, -1.0, 1.0)
    moved = replace(case, j3d=case.j3d.astype(np.float64) + 0.5 * np.spacing(np.abs(case.j3d)).astype(np.float64) * sign)
    return {k: float(v.max()) for k, v in group_errors(oracle_eval(moved, True)[1], g64, layout(case.kind)).items()}


@dataclass(frozen=True, eq=False)
class Reference:
    loss64: np.ndarray
    g64: np.ndarray
    e32: dict               # group -> e32_k
    e32_loss: float
    rounding: dict          # group -> what one float32 rounding of the targets does to it


_references = {}


def reference(case: Case) -> Reference:
    """The case's oracle results, computed once; asserts the condition on the inputs."""
    if case.name not in _references:
        loss64, g64 = oracle_eval(case, True)
        loss32, g32 = oracle_eval(case, False)
        e32 = {k: float(v.max()) for k, v in group_errors(g32, g64, layout(case.kind)).items()}
        e32_loss = float((np.abs(loss32 - loss64) / np.abs(loss64)).max())
        _references[case.name] = Reference(loss64, g64, e32, e32_loss, rounding_sensitivity(case, g64))
    r = _references[case.name]
    for k, v in r.rounding.items():
        assert v <= ROUNDING_LIMIT, f"{case.name}: one float32 rounding of the targets moves {k} by {v:.2e} (limit {ROUNDING_LIMIT:.1e}): badly conditioned"
    for k, v in r.e32.items():
        assert v <= E32_LIMIT, f"{case.name}: float32 autograd is off by {v:.2e} in {k}: the case is badly conditioned (limit {E32_LIMIT:.0e})"
    assert r.e32_loss <= E32_LIMIT, (case.name, r.e32_loss)
    return r


# ---- several turns -----------------------------------------------------------------------------------------------------------
def turn_rescaled(go: np.ndarray, sign: float) -> np.ndarray:
    """The root vectors in float64, rescaled so that every angle moves by `sign` * TURN_ULPS ulp of the float32 angle."""
    go = np.asarray(go, dtype=np.float64)
    angle = np.sqrt((go * go).sum(axis=1))
    return go * ((angle + sign * TURN_ULPS * np.spacing(angle.astype(np.float32)).astype(np.float64)) / angle)[:, None]


@dataclass(frozen=True, eq=False)
class TurnReference:
    loss64: np.ndarray
    g64: np.ndarray
    e32: dict               # group -> [B]: the float32 oracle's error per frame
    e32_loss: np.ndarray    # [B]
    widen: dict             # group -> [B]: d_f, what TURN_ULPS ulp of the float32 angle do to the float64 gradient, either way
    widen_loss: np.ndarray  # [B]


@functools.lru_cache(maxsize=None)
def turn_reference(kind: str) -> TurnReference:
    """From the oracle alone.  Conditions, asserted: up to TURN_SHARP rad the float32 oracle stays within E32_LIMIT per frame
    (``reference``'s condition), and one float32 rounding of the targets moves no group by more than ROUNDING_LIMIT.  Unlike
    the positions of the LBS forward, where two ulp of a 20 rad angle stay below the gate, the gradient's d_f does not: a group's
    gradient is a sum of partly cancelling torques while a change of the root angle moves every joint coherently, so two ulp of
    6.5 rad (1e-6 rad) already move the root group by 1e-4 of its largest entry and the others by up to 4e-5 (20 rad: 6e-4
    and 7e-5; the float32 oracle itself is off by up to 1e-4 there).  d_f is therefore not capped; it comes from float64 alone."""
    case, lay = turn_case(kind), layout(kind)
    loss64, g64 = oracle_eval(case, True)
    loss32, g32 = oracle_eval(case, False)
    rel = lambda l: np.abs(l - loss64) / np.abs(loss64)
    moved = [oracle_eval(replace(case, go=turn_rescaled(case.go, sign)), True) for sign in (1.0, -1.0)]
    widen = {k: np.maximum(*(group_errors(g, g64, lay)[k] for _, g in moved)) for k, _, _ in lay.groups}
    ref = TurnReference(loss64, g64, group_errors(g32, g64, lay), rel(loss32), widen, np.maximum(*(rel(l) for l, _ in moved)))
    sharp = np.asarray(TURNS) <= TURN_SHARP
    for k, v in rounding_sensitivity(case, g64).items():
        assert v <= ROUNDING_LIMIT, f"{case.name}: one float32 rounding of the targets moves {k} by {v:.2e}"
    for k in ref.e32:
        assert (ref.e32[k][sharp] <= E32_LIMIT).all(), (case.name, k, ref.e32[k])
    assert (ref.e32_loss[sharp] <= E32_LIMIT).all(), (case.name, ref.e32_loss)
    return ref


def turn_gate(kind: str, loss: np.ndarray, grad: np.ndarray, what: str = ""):
    """The group gate of ``gate`` per frame, widened by d_f: ``max|g - g64| <= (max(2e-5, 4 e32_kf) + d_kf) max|g64|`` over group k of
    frame f, the loss within ``max(2e-6, 4 e32_loss_f) + d_loss_f`` of itself; e32 per frame, so that the large angles do not loosen
    the small ones.  Up to TURN_SHARP rad the gate stays within a few 1e-4 of the group's largest entry (``turn_reference``);
    above it d_f dominates - the float32 angle itself is uncertain by an ulp or two, which at 5000 rad is a milliradian - and
    the test catches a wrong quadrant, a broken reduction or a broken library branch there, not an ulp.
    Prints the measured figures per angle first."""
    case, lay, ref = turn_case(kind), layout(kind), turn_reference(kind)
    err = group_errors(grad, ref.g64, lay)
    tol = {k: np.maximum(GRAD_GATE, ORDER_FACTOR * ref.e32[k]) + ref.widen[k] for k in err}
    e_loss = np.abs(loss - ref.loss64) / np.abs(ref.loss64)
    tol_loss = np.maximum(LOSS_GATE, ORDER_FACTOR * ref.e32_loss) + ref.widen_loss
    for f, a in enumerate(TURNS):
        print(f"turn gate {lay.kernel} {case.name}{what} {a:g} rad: loss={e_loss[f]:.2e}/{ref.e32_loss[f]:.2e}/{tol_loss[f]:.2e} " +
              " ".join(f"{k}={v[f]:.2e}/{ref.e32[k][f]:.2e}/{tol[k][f]:.2e}" for k, v in err.items()) + "  (error/e32/tol)")
    assert np.isfinite(grad).all() and np.isfinite(loss).all(), case.name
    for k, v in err.items():
        assert (v <= tol[k]).all(), f"{case.name}{what}: {k} off by {v} of the group's largest entry per frame, gate {tol[k]}"
    assert (e_loss <= tol_loss).all(), f"{case.name}{what}: loss off by {e_loss}, gate {tol_loss}"


# ---- device ------------------------------------------------------------------------------------------------------------------
def fit_config(case: Case, launch_shape: int = 0, prior_pose_dims: Optional[int] = None):
    from keypoints2body_amd import native
    lay, w = layout(case.kind), case.weights
    cfg = native.default_fit_config()
    cfg.num_iters, cfg.step_size = 1, 0.0                      # one evaluate-only closure
    cfg.sigma, cfg.joint_loss_weight, cfg.pose_prior_weight = w["sigma"], w["joint"], w["mixture"]
    cfg.angle_prior_weight, cfg.shape_prior_weight, cfg.pose_preserve_weight = w["bending"], w["shape"], w["preserve"]
    cfg.transl_prior_weight = w["transl"]
    cfg.freeze_betas, cfg.optimize_mask = int(case.freeze), int(case.mask)
    cfg.conf_per_frame = int(case.conf is not None and case.conf.ndim == 2)
    cfg.debug_launch_shape = int(launch_shape)
    cfg.prior_pose_dims, cfg.num_betas_prior = lay.cfg_prior_dims, lay.cfg_betas_prior
    if prior_pose_dims is not None:
        cfg.prior_pose_dims = int(prior_pose_dims)
    return cfg


def device_eval(case: Case, launch_shape: int = 0, frames: int = 0, prior_pose_dims: Optional[int] = None):
    """(loss [n], gradient [n][P]) as float64 arrays of one evaluate-only closure through ``native.fit_world`` on the first
    `frames` frames (0 = all); asserts that the closure returns the parameters unchanged."""
    from keypoints2body_amd import native
    n = frames or case.frames
    rows = lambda a: None if a is None else H.cuda(a[:n])
    conf = None if case.conf is None else (rows(case.conf) if case.conf.ndim == 2 else H.cuda(case.conf))
    ins = [rows(a) for a in (case.go, case.pose, case.shape, case.tr)]
    out = native.fit_world(native_model(case.kind), H.native_prior(), fit_config(case, launch_shape, prior_pose_dims), list(case.idx), rows(case.j3d), conf,
                           *ins, preserve_pose=rows(case.preserve), want_grad=True, transl_prior_target=rows(case.tr_target))
    for k, x in zip(native.PARAM_KEYS, ins):
        assert torch.equal(out[k], x), f"{case.name}: an evaluate-only closure moved {k}"
    return out["loss"].cpu().double().numpy(), out["grad"].cpu().double().numpy()


def gate(case: Case, loss: np.ndarray, grad: np.ndarray, ref: Optional[Reference] = None, what: str = ""):
    """Print the measured figures, then assert the gate on the first ``len(loss)`` frames of the case."""
    lay = layout(case.kind)
    ref = ref or reference(case)
    n = loss.shape[0]
    g64, loss64 = ref.g64[:n], ref.loss64[:n]
    excluded = excluded_columns(case)
    err = group_errors(grad, g64, lay)
    tol = {k: max(GRAD_GATE, ORDER_FACTOR * ref.e32[k]) for k in err}
    e_loss = float((np.abs(loss - loss64) / np.abs(loss64)).max())
    tol_loss = max(LOSS_GATE, ORDER_FACTOR * ref.e32_loss)
    print(f"gate {lay.kernel} {case.name}{what} frames={n} loss={e_loss:.2e}/{ref.e32_loss:.2e}/{tol_loss:.2e} " +
          " ".join(f"{k}={v.max():.2e}/{ref.e32[k]:.2e}/{tol[k]:.2e}" for k, v in err.items()) + "  (error/e32/tol)")
    assert np.isfinite(grad).all() and np.isfinite(loss).all(), case.name
    assert (grad[:, excluded] == 0.0).all(), f"{case.name}: a group outside the optimiser has a gradient"
    for k, v in err.items():
        assert (v <= tol[k]).all(), f"{case.name}{what}: {k} off by {v.max():.2e} of the group's largest entry (frame {int(v.argmax())}), gate {tol[k]:.2e}"
    assert e_loss <= tol_loss, f"{case.name}{what}: loss off by {e_loss:.2e}, gate {tol_loss:.2e}"


# ---- the cases by name, for the check of the input conditions ------------------------------------------------------------------
FUSED_BETAS = (1, 10, 11, 16)
TREE_KINDS = ("smplh", "smplx20", "smplx32")
BOTH = ("smpl10", "smplx20")


def all_cases():
    """Every case the GPU tests gate (the refusals have no oracle)."""
    out = [term_case("smpl10", t) for t in TERMS + ("all",)]
    out += [term_case(f"smpl{nb}", t) for nb in FUSED_BETAS if nb != 10 for t in ("shape", "joint")]
    out += [term_case(kind, t) for kind in TREE_KINDS for t in TERMS[:-1] + ("all",)]
    out += [term_case("smplx20", "all", num_targets=22)]
    out += [ladder_case(kind) for kind in BOTH + ("smplh",)]
    out += [gmof_case(kind, t) for kind in BOTH for t in ("joint", "all")]
    out += [conf_case(kind, per_frame) for kind in BOTH for per_frame in (False, True)]
    out += [member_case(kind, mask, 0) for kind in BOTH for mask in (15, 9, 2, 4)]
    out += [member_case(kind, 15, 1) for kind in BOTH]
    out += [mixture_case(kind, t) for kind in BOTH + ("smplh",) for t in ("mixture", "all")]
    out += [term_case(kind, "all") for kind in ("tree21", "tree26")]
    return out
