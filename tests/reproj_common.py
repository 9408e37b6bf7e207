"""Shared by the tests of the projected joint term (``k2b_fit_config.projection = 1``: perspective reprojection of centred
pixel targets, ``include/k2b.h``).  Built on tests/fit_gradient_common.py: its models, layouts, ``group_errors``, ``gate`` and the
limits on the inputs; the oracle is ``oracle.fit_torch.frame_losses`` fed with the projected points ``(fx X / Z, fy Y / Z, 0)``
and the targets ``(u', v', 0)``, in float64 and in float32 on one thread.  The term has no counterpart in the reference: the
oracle is this formula, nothing else.

No gate number is new.  Gradient per group and frame ``max(2e-5, 4 e32_k)``, loss ``max(2e-6, 4 e32_loss)``, and the two
conditions on the inputs, ``E32_LIMIT`` and ``ROUNDING_LIMIT``, asserted from the oracle alone
(tests/test_reproj_conditions.py, no GPU).  The inputs that meet them: targets with the principal point subtracted (a pixel
coordinate is a few hundred times its residual, so its float32 rounding counts), fx = fy = 500 px, bodies about 3 m in front
of the camera, residuals of about 15 px.

A target's third column is ignored by the kernel; the cases fill it with a seeded value, the oracle with zero."""
import functools
from dataclasses import dataclass, replace

import numpy as np
import torch

from keypoints2body_amd import synthetic
from tests import fit_gradient_common as G
from tests import helpers as H

FOCAL = (500.0, 500.0)
FOCAL_UNEQUAL = (500.0, 430.0)
DEPTH = 3.0                    # metres in front of the camera
PIXEL_OFFSET = 20.0            # scale of the seeded residuals, px: their mean size is about 15 px
SIGMA = 100.0                  # px
JOINT_WEIGHT = 1.0             # pixel residuals are two orders above metric ones: weight 1 keeps the priors in the gradient
GMOF_SIGMA = 20.0
GMOF_RESIDUALS = (2.0, 7.0, 20.0, 60.0, 150.0, 400.0)      # px: below, at and far above sigma
CONF_OFF = 100.0               # px by which a target of confidence 0 is moved
KINDS_FUSED, KINDS_TREE = ("smpl10", "smpl16"), ("smplh", "smplx20", "smplx32")
BOTH = ("smpl10", "smplx20")


@dataclass(frozen=True, eq=False)
class Case(G.Case):
    """``j3d`` holds (u', v', ignored) per target."""
    focal: tuple = FOCAL


def weights(kind: str, term: str, sigma: float = SIGMA) -> dict:
    w = G.all_on(kind) if term == "all" else G.only(term)
    w["sigma"] = sigma
    if w["joint"]:
        w["joint"] = JOINT_WEIGHT
    return w


def project64(kind: str, go, pose, shape, tr, focal) -> np.ndarray:
    """[B][J][2] pixel coordinates (centred) of the model's joints, float64."""
    p = G.joints64(kind, go, pose, shape, tr)
    return np.stack([focal[0] * p[..., 0] / p[..., 2], focal[1] * p[..., 1] / p[..., 2]], axis=-1)


def pixel_targets(uv: np.ndarray, seed: int) -> np.ndarray:
    """float32 target rows (u', v', seeded junk the kernel must not read)."""
    junk = 3.0 + synthetic.normalish(83, uv.shape[:-1] + (1,), seed)
    return np.concatenate([uv, junk], axis=-1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def base(kind: str, B: int = 17, seed: int = 11, focal: tuple = FOCAL, depth: float = DEPTH) -> Case:
    """``fit_gradient_common.base`` moved onto the optical axis (the joints' mean x and y at the principal point, which keeps the
    pixel coordinates and with them their float32 ulp small), `depth` metres from the camera; targets PIXEL_OFFSET px off."""
    b = G.base(kind, B=B, seed=seed)
    tr = b.tr.copy()
    tr[:, 2] += np.float32(depth)
    tr[:, :2] = (tr[:, :2] - G.joints64(kind, b.go, b.pose, b.shape, tr).mean(axis=1)[:, :2]).astype(np.float32)
    K = G.layout(kind).J
    uv = project64(kind, b.go, b.pose, b.shape, tr, focal) + PIXEL_OFFSET * synthetic.normalish(74, (B, K, 2), seed)
    return Case(f"proj/{kind}/base{B}s{seed}f{focal[0]:g}x{focal[1]:g}d{depth:g}", kind, b.idx, pixel_targets(uv, seed), b.go, b.pose, b.shape, tr,
                weights(kind, "all"), preserve=b.preserve, tr_target=None if b.tr_target is None else tr + (b.tr_target - b.tr), focal=focal)


def term_case(kind: str, term: str, focal: tuple = FOCAL) -> Case:
    b = base(kind, focal=focal)
    return replace(b, name=f"{b.name}/{term}", weights=weights(kind, term))


@functools.lru_cache(maxsize=None)
def conf_case(kind: str, per_frame: bool) -> Case:
    """As ``fit_gradient_common.conf_case``: zeros and values above 1, shared or a per-frame table; a target of confidence zero
    is CONF_OFF px off and must contribute nothing."""
    b = base(kind, B=3, seed=19)
    K = G.layout(kind).J
    pat = np.asarray(G.CONF_PATTERN, dtype=np.float32)
    conf = np.stack([pat[(np.arange(K) + 2 * r) % len(pat)] for r in range(3)]) if per_frame else pat[np.arange(K) % len(pat)]
    if per_frame:
        conf[:, 3] = 0.0
    table = conf if per_frame else np.broadcast_to(conf, (3, K))
    j3d = b.j3d.copy()
    j3d[table == 0.0] += np.float32(CONF_OFF)
    return replace(b, name=f"{b.name}/conf/{'table' if per_frame else 'shared'}", j3d=j3d, conf=np.ascontiguousarray(conf))


def member_case(kind: str, mask: int, freeze: int) -> Case:
    b = base(kind, B=3, seed=23)
    return replace(b, name=f"{b.name}/mask{mask}{'/frozen' if freeze else ''}", mask=mask, freeze=freeze)


@functools.lru_cache(maxsize=None)
def gmof_case(kind: str, term: str) -> Case:
    """Sigma 20 px and residuals of 2 .. 400 px, both signs; target 5 of frame 0 sits on its projection.  As in
    ``fit_gradient_common.gmof_case`` the body is centred (``base``: on the optical axis) and the residuals grow with the pixel
    coordinate: a residual of 2 px on a coordinate of 300 px would be lost in that coordinate's float32 rounding."""
    lay = G.layout(kind)
    b = base(kind, B=3, seed=17)
    tr = b.tr
    uv = project64(kind, b.go, b.pose, b.shape, tr, b.focal)
    rank = np.argsort(np.argsort(np.abs(uv).max(axis=2), axis=1), axis=1)                     # [3][J]: 0 = nearest to the principal point
    size = rank[:, :, None] * (len(GMOF_RESIDUALS) - 1) // lay.J + np.arange(2)[None, None, :]              # 0 .. 5
    f, k, c = np.meshgrid(np.arange(3), np.arange(lay.J), np.arange(2), indexing="ij")
    r = np.asarray(GMOF_RESIDUALS)[size] * np.where((f + k + c) % 2 == 0, 1.0, -1.0)
    r[0, 5] = 0.0
    return replace(b, name=f"{b.name}/gmof/{term}", j3d=pixel_targets(uv - r, 17), weights=weights(kind, term, GMOF_SIGMA))


@functools.lru_cache(maxsize=None)
def behind_case(kind: str) -> Case:
    """Frame 1 of three stands DEPTH metres BEHIND the camera (every Z < 0): legal input, finite, gated like the others."""
    b = base(kind, B=3, seed=41)
    tr = b.tr.copy()
    tr[1, 2] -= np.float32(2.0 * DEPTH)
    p = G.joints64(kind, b.go, b.pose, b.shape, tr)
    assert (p[1, :, 2] < -1.0).all() and (p[0, :, 2] > 1.0).all() and (p[2, :, 2] > 1.0).all()
    uv = project64(kind, b.go, b.pose, b.shape, tr, b.focal) + PIXEL_OFFSET * synthetic.normalish(74, (3, G.layout(kind).J, 2), 41)
    return replace(b, name=f"{b.name}/behind", j3d=pixel_targets(uv, 41), tr=tr, tr_target=None if b.tr_target is None else tr + (b.tr_target - b.tr))


# ---- the root on the plane Z = 0 ---------------------------------------------------------------------------------------------
Z0_MIN_DEPTH = 0.5             # metres: the targeted joints of the trap's cases lie at least this far from the plane Z = 0


def rest_root_z(kind: str) -> np.float32:
    """float32 z of the rest root at shape 0, contracted on the host (the GPU tests take the device's own value,
    ``native_root_z``: the kernel's root must land on Z = 0 exactly)."""
    c = G.consts(kind)
    return np.float32((np.asarray(c.J_regressor, dtype=np.float64)[0] @ np.asarray(c.v_template, dtype=np.float64)[:, 2]))


def native_root_z(kind: str) -> np.float32:
    return np.float32(G.native_model(kind).joint_basis()[0][0, 2])


def z0_case(kind: str, targeted: bool, root_z: np.float32, conf_root: float = 0.0, frames: int = 3, bad=(1,)) -> Case:
    """Betas 0 and ``transl_z = -root_z`` in the frames `bad`: their root sits on the camera's plane Z = 0, where X / Z is
    infinite.  The body lies along the optical axis (root turned a quarter about x), and the targets are the joints at least
    Z0_MIN_DEPTH from the plane in every frame - before or behind the camera - so the other joints near the plane, like the
    root, are lanes WITHOUT a target.  `targeted`: the root is a target as well, with confidence `conf_root` in the frames `bad` and 0
    in the others (0: the lane must still contribute nothing; non-zero: the frame is non-finite,
    tests/test_gpu_reproj_isolation.py).  The other frames
    are `base` frames at DEPTH."""
    lay = G.layout(kind)
    b = base(kind, B=frames, seed=43)
    go, shape, tr = b.go.copy(), b.shape.copy(), b.tr.copy()
    for f in bad:
        go[f] = (np.float32(np.pi / 2), 0.0, 0.0)
        shape[f] = 0.0
        tr[f] = (0.05, -0.03, -root_z)
    p = G.joints64(kind, go, b.pose, shape, tr)
    far = (np.abs(p[:, :, 2]) >= Z0_MIN_DEPTH).all(axis=0)
    far[0] = False
    idx = [int(j) for j in np.flatnonzero(far)]
    assert len(idx) >= 6, (kind, len(idx))
    uv = project64(kind, go, b.pose, shape, tr, b.focal)[:, idx] + PIXEL_OFFSET * synthetic.normalish(74, (frames, len(idx), 2), 43)
    j3d, conf = pixel_targets(uv, 43), None
    if targeted:
        idx = [0] + idx
        j3d = np.concatenate([np.asarray([[[12.0, -9.0, 1.0]]] * frames, dtype=np.float32), j3d], axis=1)
        conf = np.ones((frames, len(idx)), dtype=np.float32)      # per frame: the root counts in the frames `bad` alone
        conf[:, 0] = 0.0
        conf[list(bad), 0] = conf_root
    w = weights(kind, "all")
    w["transl"] = 0.0          # (its centre would sit on the plane as well; the term is covered by the other cases)
    tag = f"root{'_c%g' % conf_root if targeted else '_free'}/{frames}/{','.join(map(str, bad))}"
    return replace(b, name=f"{b.name}/z0/{tag}", idx=tuple(idx), j3d=j3d, go=go, shape=shape, tr=tr, conf=conf, weights=w, tr_target=None)


def without_root(case: Case) -> Case:
    """The same call without the root's target: what the oracle evaluates where the root's confidence is zero (0 x inf)."""
    assert case.idx[0] == 0 and case.conf is not None and not case.conf[:, 0].any()
    return replace(case, name=case.name + "/dropped", idx=case.idx[1:], j3d=np.ascontiguousarray(case.j3d[:, 1:]), conf=np.ascontiguousarray(case.conf[:, 1:]))


# ---- oracle ------------------------------------------------------------------------------------------------------------------
def oracle_eval(case: Case, double: bool):
    """(loss [B], gradient [B][P]) by autograd through the oracle, float64 arrays; excluded columns zero.  One thread."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return _oracle_eval(case, double)
    finally:
        torch.set_num_threads(threads)


def projected(points: torch.Tensor, focal) -> torch.Tensor:
    """(fx X / Z, fy Y / Z, 0) of [..][3] points: no clamp on Z."""
    fx, fy = (float(np.float32(f)) for f in focal)                       # the values the device reads from its float config
    return torch.stack([fx * points[..., 0] / points[..., 2], fy * points[..., 1] / points[..., 2], torch.zeros_like(points[..., 0])], dim=-1)


def pixel_rows(j3d: torch.Tensor) -> torch.Tensor:
    return torch.cat([j3d[..., :2], torch.zeros_like(j3d[..., :1])], dim=-1)


def frame_loss(case: Case, double: bool, go, pose, shape, tr):
    """[B] loss of the case at the given leaves (tensors of the oracle's type)."""
    from oracle.fit_torch import FitWeights, frame_losses
    lay = G.layout(case.kind)
    dt = torch.float64 if double else torch.float32
    t = lambda a: torch.tensor(np.asarray(a), dtype=dt)
    w = {k: float(np.float32(v)) for k, v in case.weights.items()}
    joints, _ = G.oracle(case.kind, double)._lbs(torch.cat([go, pose], dim=1), shape, tr)
    fw = FitWeights(sigma=w["sigma"], pose_prior_weight=w["mixture"], shape_prior_weight=w["shape"], angle_prior_weight=w["bending"],
                    joint_loss_weight=w["joint"], pose_preserve_weight=w["preserve"])
    Dp = lay.prior_dims
    preserve = t(case.pose if case.preserve is None else case.preserve)[:, :Dp]
    conf = torch.ones(len(case.idx), dtype=dt) if case.conf is None else t(case.conf)
    lf = frame_losses(pose[:, :Dp], preserve, shape[:, :lay.betas_prior], projected(joints[:, list(case.idx)], case.focal), pixel_rows(t(case.j3d)),
                      G.prior(double), conf, fw, preserve_on=True)
    target = t(case.tr if case.tr_target is None else case.tr_target)
    return lf + (w["transl"] ** 2) * ((tr - target) ** 2).sum(dim=-1)


def _oracle_eval(case: Case, double: bool):
    dt = torch.float64 if double else torch.float32
    leaves = [torch.tensor(np.asarray(a), dtype=dt).requires_grad_() for a in (case.go, case.pose, case.shape, case.tr)]
    lf = frame_loss(case, double, *leaves)
    g = torch.cat(torch.autograd.grad(lf.sum(), leaves), dim=1).double().numpy()
    g[:, G.excluded_columns(case)] = 0.0
    return lf.detach().double().numpy(), g


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
    cfg.focal[0], cfg.focal[1] = case.focal
    return cfg


def device_call(case: Case, cfg, frames: int = 0, want_grad: bool = True, rows=None):
    """``native.fit_world`` on the first `frames` frames (0 = all) or on the frames `rows`, under `cfg`."""
    from keypoints2body_amd import native
    sel = slice(0, frames or case.frames) if rows is None else list(rows)
    take = lambda a: None if a is None else H.cuda(np.ascontiguousarray(a[sel]))
    conf = None if case.conf is None else (take(case.conf) if case.conf.ndim == 2 else H.cuda(case.conf))
    ins = [take(a) for a in (case.go, case.pose, case.shape, case.tr)]
    out = native.fit_world(G.native_model(case.kind), H.native_prior(), cfg, list(case.idx), take(case.j3d), conf, *ins,
                           preserve_pose=take(case.preserve), want_grad=want_grad, transl_prior_target=take(case.tr_target))
    return out, ins


def device_eval(case: Case, launch_shape: int = 0, frames: int = 0, rows=None, finite: bool = True):
    """(loss [n], gradient [n][P]) as float64 arrays of one evaluate-only closure; the closure moves no parameter (`finite` =
    False: a frame of the call is non-finite, and the parameters it returns for that frame are unspecified)."""
    from keypoints2body_amd import native
    out, ins = device_call(case, fit_config(case, launch_shape), frames, rows=rows)
    for k, x in zip(native.PARAM_KEYS, ins):
        assert not finite or torch.equal(out[k], x), f"{case.name}: an evaluate-only closure moved {k}"
    return out["loss"].cpu().double().numpy(), out["grad"].cpu().double().numpy()


def shapes_of(kind: str):
    return (1, 2, 3, 4) if G.layout(kind).kernel == "fused" else (1, 2)


def gate(case: Case, loss, grad, ref=None, what: str = ""):
    G.gate(case, loss, grad, ref or reference(case), what)


# ---- Adam trajectories -------------------------------------------------------------------------------------------------------
ADAM = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8)
PARAM_GATE = 1e-4              # tests/test_gpu_parity.py: PARAM_TOL


def oracle_adam(case: Case, double: bool, checkpoints, mask: int = 15, freeze: int = 0):
    """``torch.optim.Adam`` over the case's loss for max(checkpoints) iterations: {iteration: ([B][P] parameters after it,
    [B] loss before its step)}.  Groups outside the optimiser (``mask``, ``freeze``) are not handed to it."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        lay = G.layout(case.kind)
        dt = torch.float64 if double else torch.float32
        go, pose, shape, tr = (torch.tensor(np.asarray(a), dtype=dt).requires_grad_() for a in (case.go, case.pose, case.shape, case.tr))
        # betas | expression: freeze_betas holds the first betas_prior coefficients
        head, tail = shape.detach()[:, :lay.betas_prior].clone().requires_grad_(), shape.detach()[:, lay.betas_prior:].clone().requires_grad_()
        opt_params = ([go] if mask & 1 else []) + ([pose] if mask & 2 else []) + ([tr] if mask & 8 else [])
        if mask & 4:
            opt_params += ([] if freeze else [head]) + ([tail] if tail.shape[1] else [])
        opt = torch.optim.Adam(opt_params, **ADAM)
        out = {}
        for it in range(1, max(checkpoints) + 1):
            opt.zero_grad()
            lf = frame_loss(case, double, go, pose, torch.cat([head, tail], dim=1), tr)
            lf.sum().backward()
            opt.step()
            if it in checkpoints:
                out[it] = (torch.cat([go, pose, head, tail, tr], dim=1).detach().double().numpy().copy(), lf.detach().double().numpy().copy())
        return out
    finally:
        torch.set_num_threads(threads)


def device_adam(case: Case, iters: int, launch_shape: int = 0, frames: int = 0, mask: int = 15, freeze: int = 0):
    """([n][P] parameters, [n] loss) after `iters` Adam iterations on the device."""
    from keypoints2body_amd import native
    cfg = fit_config(replace(case, mask=mask, freeze=freeze), launch_shape)
    cfg.num_iters, cfg.step_size = int(iters), ADAM["lr"]
    out, _ = device_call(case, cfg, frames, want_grad=False)
    return torch.cat([out[k] for k in native.PARAM_KEYS], dim=1).cpu().double().numpy(), out["loss"].cpu().double().numpy()


def trajectory_gate(what: str, got: np.ndarray, ref64: np.ndarray, ref32: np.ndarray, first_grad: np.ndarray):
    """Per parameter ``|got - ref64| <= max(1e-4, 4 |ref32 - ref64|)``, the widening taken per frame as the largest deviation of the
    float32 oracle loop in that frame.  An entry whose first-step gradient is zero in float64 takes no part (Adam's first step
    is lr * sign(g): rounding decides its sign; tests/test_gpu_parity.py starts off such points for the same reason) - the
    cases here have none outside the excluded groups, which must not move at all."""
    dev32 = np.abs(ref32 - ref64).max(axis=1, keepdims=True)
    tol = np.maximum(PARAM_GATE, G.ORDER_FACTOR * dev32)
    live = first_grad != 0.0
    err = np.abs(got - ref64)
    print(f"trajectory {what}: max error {err[live].max():.2e}, float32 oracle loop {dev32.max():.2e}, gate {tol.min():.2e} .. {tol.max():.2e}")
    assert np.isfinite(got).all(), what
    bad = np.argwhere(live & (err > tol))
    assert not len(bad), f"{what}: {len(bad)} parameters off by up to {err[live].max():.2e} (gate {tol.max():.2e}), the first at (frame, column) {bad[:6].tolist()}"


# ---- the cases by name, for the check of the input conditions ------------------------------------------------------------------
def all_cases():
    """Every case the GPU tests gate."""
    out = [term_case(kind, t) for kind in KINDS_FUSED + KINDS_TREE for t in ("joint", "all")]
    out += [term_case(kind, t, FOCAL_UNEQUAL) for kind in BOTH for t in ("joint", "all")]
    out += [conf_case(kind, per_frame) for kind in BOTH for per_frame in (False, True)]
    out += [member_case(kind, mask, 0) for kind in BOTH for mask in (15, 9, 2, 4)]
    out += [member_case(kind, 15, 1) for kind in BOTH]
    out += [gmof_case(kind, t) for kind in BOTH for t in ("joint", "all")]
    out += [behind_case(kind) for kind in BOTH]
    for kind in BOTH:
        out += [z0_case(kind, False, rest_root_z(kind)), without_root(z0_case(kind, True, rest_root_z(kind)))]
    return out
