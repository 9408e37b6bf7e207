"""Shared by the tests of the multi-view joint term (``k2b_fit_multiview``, ABI 1.10: the perspective reprojection of
``k2b_fit_config.projection = 1`` summed over C calibrated cameras, ``include/k2b.h``).  Built on tests/reproj_common.py and
tests/fit_gradient_common.py: their models, layouts, ``group_errors``, ``gate``, ``trajectory_gate`` and the limits on the inputs.
The oracle is ``oracle.fit_torch.frame_losses`` fed with the C views' projected points concatenated along the joint axis, the
targets ``(u', v', 0)`` and the confidences likewise concatenated, in float64 and in float32 on one thread.  The term has no
counterpart in the reference: the oracle is this formula, nothing else.

No gate number is new: gradient per group and frame ``max(2e-5, 4 e32_k)``, loss ``max(2e-6, 4 e32_loss)``, trajectories
``trajectory_gate``; ``E32_LIMIT`` and ``ROUNDING_LIMIT`` are asserted from the oracle alone (tests/test_multiview_conditions.py).

The rig: the body centred on the world origin; camera c of C has ``R_c = Rx(+-0.25) Ry(2 pi c / C + 0.3)`` and
``t_c = (0.02 c, -0.03 c, 3 + 0.2 c)``, the focals alternate between (500, 500) and (500, 430); the targets are 20 px x
``normalish`` off the projections and the third target column is seeded junk that the kernel must not read."""
import functools
from dataclasses import dataclass, replace

import numpy as np
import torch

from keypoints2body_amd import synthetic
from tests import fit_gradient_common as G
from tests import helpers as H
from tests import reproj_common as R

VIEWS = (1, 2, 3, 8)
KINDS = R.KINDS_FUSED + R.KINDS_TREE
BOTH = R.BOTH
TILT = 0.25


@dataclass(frozen=True, eq=False)
class Case(G.Case):
    """``j3d`` holds [B][C][K] rows (u', v', ignored); ``conf`` None, [C][K] or [B][C][K]; ``cams`` C rows (R (3,3), t (3,),
    focal (2,)) in float64 holding float32 values: what the device reads."""
    cams: tuple = ()

    @property
    def views(self):
        return len(self.cams)


def _rx(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])


def _ry(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def rig(C: int, behind=None) -> tuple:
    """The C cameras of the rig; `behind`: that camera looks AWAY from the body (its ``t_z`` negated: every q_z < 0)."""
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    cams = []
    for c in range(C):
        t = np.array([0.02 * c, -0.03 * c, 3.0 + 0.2 * c])
        if c == behind:
            t[2] = -t[2]
        cams.append((f32(_rx(TILT if c % 2 == 0 else -TILT) @ _ry(2.0 * np.pi * c / C + 0.3)), f32(t),
                     f32(R.FOCAL if c % 2 == 0 else R.FOCAL_UNEQUAL)))
    return tuple(cams)


def project64(kind: str, go, pose, shape, tr, cams) -> np.ndarray:
    """[B][C][J][2] centred pixel coordinates of the model's joints in every view, float64; also returns the depths [B][C][J]."""
    p = G.joints64(kind, go, pose, shape, tr)
    uv, z = [], []
    for Rc, tc, fc in cams:
        q = p @ Rc.T + tc
        uv.append(np.stack([fc[0] * q[..., 0] / q[..., 2], fc[1] * q[..., 1] / q[..., 2]], axis=-1))
        z.append(q[..., 2])
    return np.stack(uv, axis=1), np.stack(z, axis=1)


@functools.lru_cache(maxsize=None)
def base(kind: str, C: int, B: int = 3, seed: int = 11, behind=None) -> Case:
    """``fit_gradient_common.base`` centred on the world origin and seen by the rig's C cameras."""
    b = G.base(kind, B=B, seed=seed)
    tr = (b.tr - G.joints64(kind, b.go, b.pose, b.shape, b.tr).mean(axis=1)).astype(np.float32)
    cams = rig(C, behind)
    K = G.layout(kind).J
    uv, z = project64(kind, b.go, b.pose, b.shape, tr, cams)
    for c in range(C):
        assert (z[:, c] < -1.0).all() if c == behind else (z[:, c] > 1.0).all(), (kind, C, c)
    uv = uv + R.PIXEL_OFFSET * synthetic.normalish(74, (B, C, K, 2), seed)
    tag = "" if behind is None else f"/behind{behind}"
    return Case(f"views/{kind}/C{C}/base{B}s{seed}{tag}", kind, b.idx, R.pixel_targets(uv, seed), b.go, b.pose, b.shape, tr,
                R.weights(kind, "all"), preserve=b.preserve, tr_target=None if b.tr_target is None else tr + (b.tr_target - b.tr), cams=cams)


def term_case(kind: str, C: int, term: str, B: int = 3) -> Case:
    b = base(kind, C, B=B)
    return replace(b, name=f"{b.name}/{term}", weights=R.weights(kind, term))


@functools.lru_cache(maxsize=None)
def conf_case(kind: str, C: int, per_frame: bool) -> Case:
    """Zeros and values above 1, shared [C][K] or per frame [B][C][K]; a pair of confidence zero is CONF_OFF px off and must
    contribute nothing."""
    b = base(kind, C, B=3, seed=19)
    K = G.layout(kind).J
    pat = np.asarray(G.CONF_PATTERN, dtype=np.float32)
    shared = np.stack([pat[(np.arange(K) + c) % len(pat)] for c in range(C)])
    conf = np.stack([np.roll(shared, 2 * r, axis=1) for r in range(3)]) if per_frame else shared
    if per_frame:
        conf[:, :, 3] = 0.0
    table = conf if per_frame else np.broadcast_to(conf, (3, C, K))
    j3d = b.j3d.copy()
    j3d[table == 0.0] += np.float32(R.CONF_OFF)
    return replace(b, name=f"{b.name}/conf/{'table' if per_frame else 'shared'}", j3d=j3d, conf=np.ascontiguousarray(conf))


@functools.lru_cache(maxsize=None)
def blind_view_case(kind: str, C: int) -> Case:
    """The whole of view 1 has confidence 0 (its targets CONF_OFF px off): the call is the fit to the other views."""
    b = base(kind, C, B=3, seed=29)
    conf = np.ones((C, G.layout(kind).J), dtype=np.float32)
    conf[1] = 0.0
    j3d = b.j3d.copy()
    j3d[:, 1] += np.float32(R.CONF_OFF)
    return replace(b, name=f"{b.name}/blind1", j3d=j3d, conf=conf)


def behind_case(kind: str, C: int) -> Case:
    """Camera 1 has the body behind it: every q_z < 0 there, legal, finite, gated like the rest."""
    b = base(kind, C, B=3, seed=41, behind=1)
    return replace(b, name=f"{b.name}/all")


def member_case(kind: str, C: int, mask: int, freeze: int) -> Case:
    b = base(kind, C, B=3, seed=23)
    return replace(b, name=f"{b.name}/mask{mask}{'/frozen' if freeze else ''}", mask=mask, freeze=freeze)


# ---- oracle ------------------------------------------------------------------------------------------------------------------
def frame_loss(case: Case, double: bool, go, pose, shape, tr):
    """[B] loss of the case at the given leaves (tensors of the oracle's type)."""
    from oracle.fit_torch import FitWeights, frame_losses
    lay = G.layout(case.kind)
    dt = torch.float64 if double else torch.float32
    t = lambda a: torch.tensor(np.asarray(a), dtype=dt)
    w = {k: float(np.float32(v)) for k, v in case.weights.items()}
    joints, _ = G.oracle(case.kind, double)._lbs(torch.cat([go, pose], dim=1), shape, tr)
    pts = joints[:, list(case.idx)]
    views = [R.projected(pts @ t(Rc).T + t(tc), fc) for Rc, tc, fc in case.cams]
    B, C, K = case.j3d.shape[:3]
    fw = FitWeights(sigma=w["sigma"], pose_prior_weight=w["mixture"], shape_prior_weight=w["shape"], angle_prior_weight=w["bending"],
                    joint_loss_weight=w["joint"], pose_preserve_weight=w["preserve"])
    Dp = lay.prior_dims
    preserve = t(case.pose if case.preserve is None else case.preserve)[:, :Dp]
    conf = torch.ones(C * K, dtype=dt) if case.conf is None else t(case.conf).reshape((B, C * K) if case.conf.ndim == 3 else (C * K,))
    lf = frame_losses(pose[:, :Dp], preserve, shape[:, :lay.betas_prior], torch.cat(views, dim=1), R.pixel_rows(t(case.j3d)).reshape(B, C * K, 3),
                      G.prior(double), conf, fw, preserve_on=True)
    target = t(case.tr if case.tr_target is None else case.tr_target)
    return lf + (w["transl"] ** 2) * ((tr - target) ** 2).sum(dim=-1)


def oracle_eval(case: Case, double: bool):
    """(loss [B], gradient [B][P]) by autograd through the oracle, float64 arrays; excluded columns zero.  One thread."""
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


def rounding_sensitivity(case: Case, g64: np.ndarray) -> dict:
    """Per group: the largest change of the float64 gradient when every target coordinate moves by half its float32 ulp."""
    sign = np.where(synthetic.uniform(80, case.j3d.size, 31).reshape(case.j3d.shape) < 0.5, -1.0, 1.0)
    moved = replace(case, j3d=case.j3d.astype(np.float64) + 0.5 * np.spacing(np.abs(case.j3d)).astype(np.float64) * sign)
    return {k: float(v.max()) for k, v in G.group_errors(oracle_eval(moved, True)[1], g64, G.layout(case.kind)).items()}


_references = {}


def reference(case: Case) -> G.Reference:
    """The case's oracle results, computed once; asserts the conditions on the inputs."""
    if case.name not in _references:
        loss64, g64 = oracle_eval(case, True)
        loss32, g32 = oracle_eval(case, False)
        assert np.isfinite(g64).all() and np.isfinite(loss64).all() and np.isfinite(g32).all(), case.name
        e32 = {k: float(v.max()) for k, v in G.group_errors(g32, g64, G.layout(case.kind)).items()}
        e32_loss = float((np.abs(loss32 - loss64) / np.abs(loss64)).max())
        _references[case.name] = G.Reference(loss64, g64, e32, e32_loss, rounding_sensitivity(case, g64))
    r = _references[case.name]
    for k, v in r.rounding.items():
        assert v <= G.ROUNDING_LIMIT, f"{case.name}: one float32 rounding of the targets moves {k} by {v:.2e} (limit {G.ROUNDING_LIMIT:.1e})"
    for k, v in r.e32.items():
        assert v <= G.E32_LIMIT, f"{case.name}: float32 autograd is off by {v:.2e} in {k} (limit {G.E32_LIMIT:.0e})"
    assert r.e32_loss <= G.E32_LIMIT, (case.name, r.e32_loss)
    return r


# ---- device ------------------------------------------------------------------------------------------------------------------
def fit_config(case: Case, launch_shape: int = 0):
    cfg = G.fit_config(case, launch_shape)
    cfg.projection = 1
    cfg.conf_per_frame = int(case.conf is not None and case.conf.ndim == 3)
    return cfg


def device_call(case: Case, cfg, want_grad: bool = True, rows=None, model=None, prior=None, j3d=None):
    """``native.fit_multiview`` on the frames `rows` (None = all) under `cfg`; `j3d` replaces the case's targets."""
    from keypoints2body_amd import native
    sel = slice(0, case.frames) if rows is None else list(rows)
    take = lambda a: None if a is None else H.cuda(np.ascontiguousarray(a[sel]))
    conf = None if case.conf is None else (take(case.conf) if case.conf.ndim == 3 else H.cuda(case.conf))
    ins = [take(a) for a in (case.go, case.pose, case.shape, case.tr)]
    out = native.fit_multiview(model or G.native_model(case.kind), prior or H.native_prior(), cfg, list(case.cams), list(case.idx),
                               take(case.j3d if j3d is None else j3d), conf, *ins, preserve_pose=take(case.preserve), want_grad=want_grad,
                               transl_prior_target=take(case.tr_target))
    return out, ins


def device_eval(case: Case, launch_shape: int = 0, rows=None, finite: bool = True, j3d=None):
    """(loss [n], gradient [n][P]) as float64 arrays of one evaluate-only closure; the closure moves no parameter."""
    from keypoints2body_amd import native
    out, ins = device_call(case, fit_config(case, launch_shape), rows=rows, j3d=j3d)
    for k, x in zip(native.PARAM_KEYS, ins):
        assert not finite or torch.equal(out[k], x), f"{case.name}: an evaluate-only closure moved {k}"
    return out["loss"].cpu().double().numpy(), out["grad"].cpu().double().numpy()


def gate(case: Case, loss, grad, what: str = ""):
    G.gate(case, loss, grad, reference(case), what)


# ---- Adam trajectories -------------------------------------------------------------------------------------------------------
def oracle_adam(case: Case, double: bool, checkpoints):
    """``reproj_common.oracle_adam`` with the multi-view loss: {iteration: ([B][P] parameters after it, [B] loss before its
    step)}, every group in the optimiser."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        dt = torch.float64 if double else torch.float32
        go, pose, shape, tr = (torch.tensor(np.asarray(a), dtype=dt).requires_grad_() for a in (case.go, case.pose, case.shape, case.tr))
        opt = torch.optim.Adam([go, pose, tr, shape], **R.ADAM)
        out = {}
        for it in range(1, max(checkpoints) + 1):
            opt.zero_grad()
            lf = frame_loss(case, double, go, pose, shape, tr)
            lf.sum().backward()
            opt.step()
            if it in checkpoints:
                out[it] = (torch.cat([go, pose, shape, tr], dim=1).detach().double().numpy().copy(), lf.detach().double().numpy().copy())
        return out
    finally:
        torch.set_num_threads(threads)


def device_adam(case: Case, iters: int, launch_shape: int = 0, rows=None, model=None, prior=None, j3d=None):
    """([n][P] parameters, [n] loss) after `iters` Adam iterations on the device, as float32 tensors' exact values."""
    from keypoints2body_amd import native
    cfg = fit_config(case, launch_shape)
    cfg.num_iters, cfg.step_size = int(iters), R.ADAM["lr"]
    out, _ = device_call(case, cfg, want_grad=False, rows=rows, model=model, prior=prior, j3d=j3d)
    return torch.cat([out[k] for k in native.PARAM_KEYS], dim=1).cpu().numpy(), out["loss"].cpu().numpy()


# ---- the cases by name, for the check of the input conditions ------------------------------------------------------------------
def term_cases():
    """(kind, C) of the closure cases: every kind with C = 3, ``BOTH`` with every C."""
    return [(kind, 3) for kind in KINDS] + [(kind, C) for kind in BOTH for C in VIEWS if C != 3]


def trajectory_case(kind: str, C: int) -> Case:
    return base(kind, C, B=3, seed=11)


def all_cases():
    """Every case the GPU tests gate."""
    out = [term_case(kind, C, t) for kind, C in term_cases() for t in ("joint", "all")]
    out += [conf_case(kind, 3, per_frame) for kind in BOTH for per_frame in (False, True)]
    out += [blind_view_case(kind, 3) for kind in BOTH]
    out += [behind_case(kind, 3) for kind in BOTH]
    out += [member_case(kind, 2, mask, 0) for kind in BOTH for mask in (15, 9, 2, 4)]
    out += [member_case(kind, 2, 15, 1) for kind in BOTH]
    out += [trajectory_case(kind, C) for kind in BOTH for C in (2, 4)]
    return out
