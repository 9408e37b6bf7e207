"""Shared by the tests of PROJECTED SURFACE TARGETS (``k2b_surface_term_image``, ``k2b_fit_image``: vertex-selected joints and
barycentric landmarks under the perspective joint term of ``k2b_fit_config.projection``, ``include/k2b.h``).

Built on tests/lbs_layouts_common.py (the landmark layout, ``surface_term_case``, ``_output_joints``, ``oracle``, ``term_groups``),
tests/reproj_common.py (``projected``, ``pixel_rows``, ``trajectory_gate``, ``FOCAL_UNEQUAL``) and tests/fit_gradient_common.py.  The
oracle is float64 autograd of

    (X, Y, Z) = output joint t (smplx's: sum_k b_tk v_u, translated),   e = (fx X / Z - u', fy Y / Z - v'),
    loss_t = w_j^2 c_t^2 (gmof(e_x, sigma) + gmof(e_y, sigma))

through the oracle forward plus ``_output_joints``, in float64 and in float32 on one thread.  The term has NO counterpart in the
reference (its 2D input raises): the oracle is this formula, nothing else.

No gate number is new: gradient per group and frame ``max(GRAD_GATE = 2e-5, 4 e32)``, loss ``max(LOSS_GATE = 2e-6, 4 e32_loss)``,
parameters ``trajectory_gate``; the conditions on the inputs are ``E32_LIMIT``, ``ROUNDING_LIMIT`` and, for the stand-alone term's
loss, ``TERM_ROUNDING_LIMIT_LOSS`` (tests/test_reproj_surface_conditions.py asserts them from the oracle alone)."""
import dataclasses
import functools
from dataclasses import replace
from typing import Optional

import numpy as np
import torch

from keypoints2body_amd import synthetic
from tests import fit_gradient_common as G
from tests import helpers as H
from tests import lbs_layouts_common as L
from tests import reproj_common as R

FOCAL = R.FOCAL_UNEQUAL
SIGMA, WEIGHT = R.SIGMA, R.JOINT_WEIGHT
V = L.V_SMALL


# ---- the stand-alone term ----------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True, eq=False)
class TermCase:
    name: str
    J: int
    NB: int
    params: tuple                 # (go, pose, shape, tr) float32
    rows: tuple                   # output joints = what the entry takes as model joint indices
    targets: np.ndarray           # [B][T][3] float32 rows (u', v', junk)
    conf: np.ndarray              # [B][T]
    skip: Optional[np.ndarray] = None   # [B][T] bool: targets the ORACLE leaves out (the device gets them with confidence 0)
    focal: tuple = FOCAL


def _points64(J, NB, p, rows):
    j64, _ = L._forward(J, NB, V, "landmarks", p, True, True)
    return j64[:, list(rows)].numpy()


def _on_axis(J, NB, p, rows, depth):
    """The parameters with the selected points' mean x and y on the optical axis, `depth` metres along it ([B] or a number)."""
    go, pose, shape, tr = (a.copy() for a in p)
    tr[:, 2] += np.asarray(depth, dtype=np.float32)
    tr[:, :2] = (tr[:, :2] - _points64(J, NB, (go, pose, shape, tr), rows).mean(axis=1)[:, :2]).astype(np.float32)
    return go, pose, shape, tr


def _term_case(name, rows, depth, seed):
    J, NB = L.LANDMARK_LAYOUT
    b = L.surface_term_case(3)
    cols = [b.rows.index(r) for r in rows]
    p = _on_axis(J, NB, b.params, rows, depth)
    x = _points64(J, NB, p, rows)
    B, T = x.shape[:2]
    uv = np.stack([FOCAL[0] * x[..., 0] / x[..., 2], FOCAL[1] * x[..., 1] / x[..., 2]], axis=-1)
    uv = uv + R.PIXEL_OFFSET * synthetic.normalish(74, (B, T, 2), seed)
    conf = np.ascontiguousarray(b.conf[:, cols])
    conf[1, min(3, T - 1)] = 0.0
    return TermCase(name, J, NB, p, tuple(rows), R.pixel_targets(uv, seed), conf)


@functools.lru_cache(maxsize=None)
def base() -> TermCase:
    """The 20 targets of ``surface_term_case`` (extras J, J+2, J+4 and every third landmark) on the landmark layout, B = 3, on the
    optical axis at 3 m, targets 20 px off, FOCAL_UNEQUAL, sigma 100 px, weight 1, per-frame confidences with conf[1, 3] = 0."""
    return _term_case("proj surface/base", L.surface_term_case(3).rows, R.DEPTH, 43)


@functools.lru_cache(maxsize=None)
def extras_only() -> TermCase:
    """Vertex-selected joints alone: under projection they take the surface kernel as well."""
    return _term_case("proj surface/extras", L.surface_term_case(3).rows[:3], R.DEPTH, 47)


@functools.lru_cache(maxsize=None)
def behind() -> TermCase:
    """Frame 1 stands 3 m BEHIND the camera (every Z < 0): legal, finite, the same gates."""
    c = _term_case("proj surface/behind", L.surface_term_case(3).rows, np.asarray([R.DEPTH, -R.DEPTH, R.DEPTH]), 53)
    z = _points64(c.J, c.NB, c.params, c.rows)[..., 2]
    assert (z[1] < -1.0).all() and (z[0] > 1.0).all() and (z[2] > 1.0).all()
    return c


@functools.lru_cache(maxsize=None)
def conf_zero_moved() -> TermCase:
    """The target of confidence 0 moved by CONF_OFF px: the oracle evaluates the call WITHOUT that target."""
    b = base()
    tgt = b.targets.copy()
    tgt[b.conf == 0.0] += np.float32(R.CONF_OFF)
    return replace(b, name="proj surface/conf0", targets=tgt, skip=b.conf == 0.0)


def term_cases():
    return [base(), extras_only(), behind(), conf_zero_moved()]


def term_oracle(case: TermCase, double: bool, targets=None):
    """(loss [B], gradient [B][P] in the packed layout) by autograd, as float64 arrays.  One thread."""
    from oracle.fit_torch import gmof
    dt = torch.float64 if double else torch.float32
    leaves = [torch.tensor(a, dtype=dt, requires_grad=True) for a in case.params]
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        joints, verts = L.oracle(case.J, case.NB, V, "landmarks", double)._lbs(torch.cat(leaves[:2], dim=1), leaves[2], leaves[3])
        pts = L._output_joints(joints, verts, L.landmarks(case.J, V))[:, list(case.rows)]
        c = torch.tensor(case.conf, dtype=dt)
        w = float(np.float32(WEIGHT))
        tgt = R.pixel_rows(torch.tensor(case.targets if targets is None else targets, dtype=dt))
        per = (w * w) * (c * c) * gmof(R.projected(pts, case.focal) - tgt, float(np.float32(SIGMA))).sum(dim=-1)
        if case.skip is not None:
            per = torch.where(torch.as_tensor(case.skip), torch.zeros_like(per), per)
        lf = per.sum(dim=1)
        grads = torch.autograd.grad(lf.sum(), leaves)
    finally:
        torch.set_num_threads(threads)
    return lf.detach().double().numpy(), torch.cat(grads, dim=1).double().numpy()


_term_references = {}


def term_figures(case: TermCase) -> L.TermReference:
    """The oracle's results and the figures of the input conditions, computed once, nothing asserted."""
    if case.name not in _term_references:
        lay = L.term_groups(case.J, case.NB)
        loss64, g64 = term_oracle(case, True)
        loss32, g32 = term_oracle(case, False)
        sign = np.where(synthetic.uniform(80, case.targets.size, 31).reshape(case.targets.shape) < 0.5, -1.0, 1.0)
        moved = case.targets.astype(np.float64) + 0.5 * np.spacing(np.abs(case.targets)).astype(np.float64) * sign
        loss_m, g_m = term_oracle(case, True, targets=moved)
        rel = lambda a: float((np.abs(a - loss64) / np.abs(loss64)).max())
        _term_references[case.name] = L.TermReference(
            loss64, g64, {k: float(v.max()) for k, v in G.group_errors(g32, g64, lay).items()}, rel(loss32),
            {k: float(v.max()) for k, v in G.group_errors(g_m, g64, lay).items()}, rel(loss_m))
    return _term_references[case.name]


def term_reference(case: TermCase) -> L.TermReference:
    """``term_figures`` with the conditions on the inputs asserted."""
    r = term_figures(case)
    assert np.isfinite(r.g64).all() and np.isfinite(r.loss64).all(), case.name
    for k, v in r.rounding.items():
        assert v <= G.ROUNDING_LIMIT, f"{case.name}: one float32 rounding of the targets moves {k} by {v:.2e} (limit {G.ROUNDING_LIMIT:.1e})"
    assert r.rounding_loss <= L.TERM_ROUNDING_LIMIT_LOSS, f"{case.name}: one float32 rounding of the targets moves the loss by {r.rounding_loss:.2e}"
    for k, v in dict(r.e32, loss=r.e32_loss).items():
        assert v <= G.E32_LIMIT, f"{case.name}: the float32 oracle is off by {v:.2e} in {k} (limit {G.E32_LIMIT:.0e})"
    return r


def term_gate(case: TermCase, loss, grad):
    ref = term_reference(case)
    lay = L.term_groups(case.J, case.NB)
    loss, grad = loss.detach().cpu().double().numpy(), grad.detach().cpu().double().numpy()
    err = G.group_errors(grad, ref.g64, lay)
    tol = {k: max(G.GRAD_GATE, G.ORDER_FACTOR * ref.e32[k]) for k in err}
    e_loss = float((np.abs(loss - ref.loss64) / np.abs(ref.loss64)).max())
    tol_loss = max(G.LOSS_GATE, G.ORDER_FACTOR * ref.e32_loss)
    print(f"term {case.name}: loss={e_loss:.2e}/{ref.e32_loss:.2e}/{tol_loss:.2e} " +
          " ".join(f"{k}={v.max():.2e}/{ref.e32[k]:.2e}/{tol[k]:.2e}" for k, v in err.items()) + "  (error/e32/tol)")
    assert np.isfinite(grad).all() and np.isfinite(loss).all(), case.name
    for k, v in err.items():
        assert (v <= tol[k]).all(), f"{case.name}: {k} off by {v.max():.2e} of the group's largest entry (frame {int(v.argmax())}), gate {tol[k]:.2e}"
    assert e_loss <= tol_loss, f"{case.name}: loss off by {e_loss:.2e}, gate {tol_loss:.2e}"


def term_device(case: TermCase, rows=None):
    """``native.surface_term_image`` on the case (on the frames `rows`)."""
    from keypoints2body_amd import native
    sel = slice(None) if rows is None else list(rows)
    take = lambda a: H.cuda(np.ascontiguousarray(a[sel]))
    return native.surface_term_image(L.native_model(case.J, case.NB, V, "landmarks"), list(case.rows), take(case.targets), take(case.conf),
                                     SIGMA, WEIGHT, case.focal, *(take(a) for a in case.params))


# ---- the whole loss: kinematic joints and surface targets in one k2b_fit_image call -----------------------------------------------
FUSED, TREE = "smpl10", "smplx20"
LMK_KIND = "smplx20"              # the landmark-bearing model: smplx20's constants with a landmark table of its own


@dataclasses.dataclass(frozen=True, eq=False)
class Case(R.Case):
    """``reproj_common.Case`` whose ``idx`` may name output joints beyond the kinematic ones; `lmk`: the model's landmark table."""
    lmk: Optional[tuple] = None


@functools.lru_cache(maxsize=None)
def lmk_table():
    c = G.consts(LMK_KIND)
    return synthetic.make_landmarks(c.v_template.shape[0], G.layout(LMK_KIND).J, 51, seed=0)


def num_outputs(kind: str, lmk) -> int:
    return G.layout(kind).J + len(G.consts(kind).extra_vertex_ids) + (0 if lmk is None else lmk[0].shape[0])


def outputs(kind, lmk, double, go, pose, shape, tr):
    joints, verts = G.oracle(kind, double)._lbs(torch.cat([go, pose], dim=1), shape, tr)
    return L._output_joints(joints, verts, lmk)


def surface_rows(kind: str, lmk) -> tuple:
    """Extras J, J+2, J+4, J+7 and, on a landmark model, every fifth landmark."""
    J, E = G.layout(kind).J, len(G.consts(kind).extra_vertex_ids)
    return (J, J + 2, J + 4, J + 7) + (() if lmk is None else tuple(range(J + E, J + E + lmk[0].shape[0], 5)))


@functools.lru_cache(maxsize=None)
def fit_case(kind: str, landmarks: bool = False, B: int = 3, seed: int = 23, mask: int = 15, freeze: int = 0, kinematic: int = 0) -> Case:
    """``reproj_common.base`` (every kinematic joint - or the first `kinematic` -, all priors on, on the optical axis at 3 m) with
    the surface targets of ``surface_rows`` beside them, 20 px off their float64 projection, per-frame confidences with one zero on
    a surface target moved by CONF_OFF px."""
    b = R.base(kind, B=B, seed=seed, focal=FOCAL)
    lmk = lmk_table() if landmarks else None
    K = kinematic or len(b.idx)
    rows = surface_rows(kind, lmk)
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    with torch.no_grad():
        x = outputs(kind, lmk, True, t(b.go), t(b.pose), t(b.shape), t(b.tr))[:, list(rows)].numpy()
    uv = np.stack([FOCAL[0] * x[..., 0] / x[..., 2], FOCAL[1] * x[..., 1] / x[..., 2]], axis=-1)
    uv = uv + R.PIXEL_OFFSET * synthetic.normalish(77, uv.shape, seed)
    j3d = np.concatenate([b.j3d[:, :K], R.pixel_targets(uv, seed + 1)], axis=1)
    conf = (0.5 + synthetic.uniform(96, B * j3d.shape[1], seed).reshape(B, -1)).astype(np.float32)
    conf[1 % B, K + 1] = 0.0
    j3d[1 % B, K + 1] += np.float32(R.CONF_OFF)
    name = f"proj surface fit/{kind}{'+lmk' if landmarks else ''}/B{B}s{seed}k{K}/mask{mask}{'/frozen' if freeze else ''}"
    return Case(name, kind, tuple(b.idx[:K]) + rows, np.ascontiguousarray(j3d), b.go, b.pose, b.shape, b.tr, b.weights, conf=conf,
                preserve=b.preserve, tr_target=b.tr_target, mask=mask, freeze=freeze, focal=FOCAL, lmk=lmk)


def frame_loss(case: Case, double: bool, go, pose, shape, tr):
    """``reproj_common.frame_loss`` over the model's OUTPUT joints (kinematic, vertex-selected, landmarks)."""
    from oracle.fit_torch import FitWeights, frame_losses
    lay = G.layout(case.kind)
    dt = torch.float64 if double else torch.float32
    t = lambda a: torch.tensor(np.asarray(a), dtype=dt)
    w = {k: float(np.float32(v)) for k, v in case.weights.items()}
    pts = outputs(case.kind, case.lmk, double, go, pose, shape, tr)[:, list(case.idx)]
    fw = FitWeights(sigma=w["sigma"], pose_prior_weight=w["mixture"], shape_prior_weight=w["shape"], angle_prior_weight=w["bending"],
                    joint_loss_weight=w["joint"], pose_preserve_weight=w["preserve"])
    Dp = lay.prior_dims
    preserve = t(case.pose if case.preserve is None else case.preserve)[:, :Dp]
    conf = torch.ones(len(case.idx), dtype=dt) if case.conf is None else t(case.conf)
    lf = frame_losses(pose[:, :Dp], preserve, shape[:, :lay.betas_prior], R.projected(pts, case.focal), R.pixel_rows(t(case.j3d)),
                      G.prior(double), conf, fw, preserve_on=True)
    target = t(case.tr if case.tr_target is None else case.tr_target)
    return lf + (w["transl"] ** 2) * ((tr - target) ** 2).sum(dim=-1)


def oracle_eval(case: Case, double: bool):
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        dt = torch.float64 if double else torch.float32
        leaves = [torch.tensor(np.asarray(a), dtype=dt).requires_grad_() for a in (case.go, case.pose, case.shape, case.tr)]
        lf = frame_loss(case, double, *leaves)
        g = torch.cat(torch.autograd.grad(lf.sum(), leaves), dim=1).double().numpy()
        g[:, G.excluded_columns(case)] = 0.0
        return lf.detach().double().numpy(), g
    finally:
        torch.set_num_threads(threads)


_references = {}


def figures(case: Case) -> G.Reference:
    if case.name not in _references:
        loss64, g64 = oracle_eval(case, True)
        loss32, g32 = oracle_eval(case, False)
        lay = G.layout(case.kind)
        e32 = {k: float(v.max()) for k, v in G.group_errors(g32, g64, lay).items()}
        sign = np.where(synthetic.uniform(80, case.j3d.size, 31).reshape(case.j3d.shape) < 0.5, -1.0, 1.0)
        moved = replace(case, j3d=case.j3d.astype(np.float64) + 0.5 * np.spacing(np.abs(case.j3d)).astype(np.float64) * sign)
        rounding = {k: float(v.max()) for k, v in G.group_errors(oracle_eval(moved, True)[1], g64, lay).items()}
        _references[case.name] = G.Reference(loss64, g64, e32, float((np.abs(loss32 - loss64) / np.abs(loss64)).max()), rounding)
    return _references[case.name]


def reference(case: Case) -> G.Reference:
    r = figures(case)
    assert np.isfinite(r.g64).all() and np.isfinite(r.loss64).all(), case.name
    for k, v in r.rounding.items():
        assert v <= G.ROUNDING_LIMIT, f"{case.name}: one float32 rounding of the targets moves {k} by {v:.2e} (limit {G.ROUNDING_LIMIT:.1e})"
    for k, v in dict(r.e32, loss=r.e32_loss).items():
        assert v <= G.E32_LIMIT, f"{case.name}: the float32 oracle is off by {v:.2e} in {k} (limit {G.E32_LIMIT:.0e})"
    return r


def fit_cases():
    """Every whole-loss case the GPU tests gate."""
    out = [fit_case(FUSED), fit_case(TREE), fit_case(LMK_KIND, True)] + [c for c, _ in adam_cases()]
    return [c for i, c in enumerate(out) if c not in out[:i]]


def adam_cases():
    """(case, iterations): optimize_mask 15 and 9 on both routes, freeze_betas once."""
    return [(fit_case(k, mask=m), 12) for k in (FUSED, TREE) for m in (15, 9)] + [(fit_case(TREE, freeze=1), 12)]


_native_lmk = {}


def native_model(case):
    lmk = getattr(case, "lmk", None)
    if lmk is None:
        return G.native_model(case.kind)
    if case.kind not in _native_lmk:             # built here, as tests/test_gpu_landmarks.py::native_lmk builds its own
        from keypoints2body_amd.native import NativeModel
        c = G.consts(case.kind)
        _native_lmk[case.kind] = NativeModel(c.v_template, c.shapedirs, c.posedirs, c.J_regressor, c.lbs_weights, c.parents,
                                             c.extra_vertex_ids, landmarks=case.lmk)
    return _native_lmk[case.kind]


def device_call(case: Case, cfg, rows=None, want_grad: bool = True, entry: str = "fit_image", edit=None):
    """``native.fit_image`` (or `entry`) on the case's frames (or on the frames `rows`) under `cfg`; `edit(name, array)` changes an
    input on its way to the device.  Returns (outputs, the start tensors)."""
    from keypoints2body_amd import native
    sel = slice(None) if rows is None else list(rows)
    edit = edit or (lambda name, a: a)
    take = lambda name, a: None if a is None else H.cuda(np.ascontiguousarray(edit(name, a.copy())[sel]))
    ins = [take(k, a) for k, a in zip(("go", "pose", "shape", "tr"), (case.go, case.pose, case.shape, case.tr))]
    out = getattr(native, entry)(native_model(case), H.native_prior(), cfg, list(case.idx), take("j3d", case.j3d), take("conf", case.conf), *ins,
                                 preserve_pose=take("preserve", case.preserve), want_grad=want_grad,
                                 transl_prior_target=take("tr_target", case.tr_target))
    return out, ins


def adam_config(case: Case, iters: int):
    cfg = R.fit_config(case)
    cfg.num_iters, cfg.step_size = int(iters), R.ADAM["lr"]
    return cfg


def packed_row(out) -> torch.Tensor:
    from keypoints2body_amd import native
    return torch.cat([out[k] for k in native.PARAM_KEYS], dim=1)


# ---- Adam loops and warm-start chains over the output joints -----------------------------------------------------------------------
def oracle_adam(case: Case, double: bool, iters: int):
    """``reproj_common.oracle_adam`` over ``frame_loss`` above (landmarks included): ([B][P] parameters after `iters` iterations,
    [B] loss before the last step).  ``case.mask`` / ``case.freeze`` say what the optimiser holds."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        lay = G.layout(case.kind)
        dt = torch.float64 if double else torch.float32
        go, pose, shape, tr = (torch.tensor(np.asarray(a), dtype=dt).requires_grad_() for a in (case.go, case.pose, case.shape, case.tr))
        head, tail = shape.detach()[:, :lay.betas_prior].clone().requires_grad_(), shape.detach()[:, lay.betas_prior:].clone().requires_grad_()
        opt_params = ([go] if case.mask & 1 else []) + ([pose] if case.mask & 2 else []) + ([tr] if case.mask & 8 else [])
        if case.mask & 4:
            opt_params += ([] if case.freeze else [head]) + ([tail] if tail.shape[1] else [])
        opt = torch.optim.Adam(opt_params, **R.ADAM)
        for _ in range(iters):
            opt.zero_grad()
            lf = frame_loss(case, double, go, pose, torch.cat([head, tail], dim=1), tr)
            lf.sum().backward()
            opt.step()
        return torch.cat([go, pose, head, tail, tr], dim=1).detach().double().numpy().copy(), lf.detach().double().numpy().copy()
    finally:
        torch.set_num_threads(threads)


def oracle_chain(kind: str, lmk, idx, targets, start, weights: dict, focal, first: int, follow: int, freeze: bool, double: bool):
    """One video as ``reproj_chain_common.oracle_chain`` runs it, over the output joints `idx`: `targets` [T][K][3] centred rows,
    `start` (go, pose, shape, tr) rows of one frame.  Frame 0: `first` iterations without the preserve term; frame t > 0 from frame
    t - 1's result, that result's pose preserved, `follow` iterations, a fresh optimiser, the betas held under `freeze`.  Per frame
    ([1][P] parameters, [1] loss, [1][P] float64 gradient at the frame's start)."""
    lay = G.layout(kind)
    cur = [np.asarray(a, dtype=np.float64 if double else np.float32) for a in start]
    edges = (0, 3, 3 + lay.D, 3 + lay.D + lay.NB, lay.P)
    steps = []
    for t in range(targets.shape[0]):
        w = dict(weights, preserve=weights["preserve"] if t > 0 else 0.0, transl=0.0)
        case = Case(f"chain step {t}", kind, tuple(idx), np.ascontiguousarray(targets[t:t + 1]), *cur, w, preserve=cur[1], mask=15,
                    freeze=int(freeze and t > 0), focal=tuple(focal), lmk=lmk)
        params, loss = oracle_adam(case, double, first if t == 0 else follow)
        steps.append((params, loss, oracle_eval(case, True)[1] if double else None))
        cur = [params[:, a:b] if double else params[:, a:b].astype(np.float32) for a, b in zip(edges, edges[1:])]
    return steps
