"""Shared by the tests of the multi-view warm-start chains (``k2b_fit_multiview_sequences``, ABI 1.11, ``include/k2b.h``).  Built on
tests/multiview_common.py - its rig, its bodies (``base``: centred on the world origin, seen by C cameras), its loss
(``frame_loss``) - and on tests/reproj_chain_common.py and tests/reproj_common.py (``PRESERVE``, ``refused``, ``trajectory_gate``,
``F32_LOOP_LIMIT``), all unchanged.  No gate number is new.

A sequence is ONE ``base`` body seen in T frames by the same rig: frame t's targets are the body's projections into the C views
plus its own seeded residuals of PIXEL_OFFSET px (frame 0: the base case's own targets).

The chain, restated (k2b.h): frame 0 of a sequence runs `first` Adam iterations from the sequence's start without a preserve
term; frame t > 0 starts from frame t - 1's result, preserves that result's pose with the configured weight, runs `follow`
iterations with a fresh optimiser and, with `freeze`, holds the first ``betas_prior`` shape coefficients."""
import functools
from dataclasses import dataclass, replace
from typing import Optional

import numpy as np
import torch

from keypoints2body_amd import synthetic
from tests import fit_gradient_common as G
from tests import helpers as H
from tests import multiview_common as MV
from tests import reproj_chain_common as RC
from tests import reproj_common as R

PRESERVE = RC.PRESERVE
KEYS = RC.KEYS
ORACLE_KINDS = ("smpl10", "smplx20")                # one fused kind, one tree kind
ORACLE_VIEWS = (2, 4)
ORACLE_S, ORACLE_T, ORACLE_FIRST, ORACLE_FOLLOW = 3, 3, 10, 5
ORACLE_SEED = 59


@dataclass(frozen=True, eq=False)
class Chain:
    """S sequences, packed: ``targets`` [sum T][C][K][3] rows (u', v', ignored), ``conf`` None, [C][K] or [sum T][C][K], one start
    row per sequence (``base``, which also holds the rig), ``lengths`` [S]."""
    name: str
    kind: str
    base: MV.Case
    targets: np.ndarray
    conf: Optional[np.ndarray]
    lengths: np.ndarray

    @property
    def offsets(self):
        return np.concatenate(([0], np.cumsum(self.lengths)[:-1])).astype(np.int64)

    def rows(self, s):
        return slice(int(self.offsets[s]), int(self.offsets[s] + self.lengths[s]))

    @property
    def per_frame_conf(self):
        return self.conf is not None and self.conf.ndim == 3


def weights(kind):
    w = R.weights(kind, "all")
    w["transl"], w["preserve"] = 0.0, PRESERVE      # (a chain takes no translation prior)
    return w


@functools.lru_cache(maxsize=None)
def chain(kind: str, C: int, lengths: tuple, seed: int = 11, conf: str = "") -> Chain:
    """`conf`: "" (none), "shared" ([C][K]) or "frame" ([sum T][C][K]); values in 0.5 .. 1.5."""
    S, T = len(lengths), max(max(lengths), 1)
    b = MV.base(kind, C, B=S, seed=seed)
    b = replace(b, weights=weights(kind), preserve=None, tr_target=None)
    K = G.layout(kind).J
    uv, _ = MV.project64(kind, b.go, b.pose, b.shape, b.tr, b.cams)
    frames = [b.j3d] + [R.pixel_targets(uv + R.PIXEL_OFFSET * synthetic.normalish(74, (S, C, K, 2), seed + 101 * t), seed + t) for t in range(1, T)]
    per_seq = np.stack(frames, axis=1)                                                      # [S][T][C][K][3]
    targets = np.concatenate([per_seq[s, :lengths[s]] for s in range(S)], axis=0)
    table = None
    if conf == "shared":
        table = (0.5 + synthetic.uniform(81, C * K, seed).reshape(C, K)).astype(np.float32)
    elif conf == "frame":
        table = (0.5 + synthetic.uniform(81, targets.shape[0] * C * K, seed).reshape(targets.shape[0], C, K)).astype(np.float32)
    return Chain(f"mvchain/{kind}/C{C}/{'-'.join(map(str, lengths)) if len(lengths) < 8 else f'{len(lengths)}x{lengths[0]}'}s{seed}{conf}", kind, b,
                 np.ascontiguousarray(targets), table, np.asarray(lengths, dtype=np.int32))


def select(c: Chain, seqs) -> Chain:
    """The sequences `seqs` of `c`, in that order, as a chain of their own."""
    seqs = list(seqs)
    take = lambda a: np.ascontiguousarray(a[seqs])
    b = replace(c.base, go=take(c.base.go), pose=take(c.base.pose), shape=take(c.base.shape), tr=take(c.base.tr), j3d=take(c.base.j3d))
    cat = lambda a: np.concatenate([a[c.rows(s)] for s in seqs], axis=0) if seqs else a[:0]
    conf = np.ascontiguousarray(cat(c.conf)) if c.per_frame_conf else c.conf
    return Chain(f"{c.name}/{','.join(map(str, seqs))}", c.kind, b, np.ascontiguousarray(cat(c.targets)), conf, c.lengths[seqs])


def drop_view(c: Chain, view: int) -> Chain:
    """`c` without camera `view`: its rig, target rows and confidences."""
    keep = [v for v in range(c.base.views) if v != view]
    b = replace(c.base, cams=tuple(c.base.cams[v] for v in keep), j3d=np.ascontiguousarray(c.base.j3d[:, keep]))
    conf = None if c.conf is None else np.ascontiguousarray(c.conf[..., keep, :])
    return Chain(f"{c.name}/without{view}", c.kind, b, np.ascontiguousarray(c.targets[:, keep]), conf, c.lengths)


def blind_view(c: Chain, view: int) -> Chain:
    """`c` with confidence 0 in the whole of camera `view`, whose targets are CONF_OFF px off; the other pairs keep theirs (ones
    where `c` has none)."""
    K = G.layout(c.kind).J
    conf = np.ones((c.base.views, K), dtype=np.float32) if c.conf is None else c.conf.copy()
    conf[..., view, :] = 0.0
    targets = c.targets.copy()
    targets[:, view] += np.float32(R.CONF_OFF)
    return Chain(f"{c.name}/blind{view}", c.kind, c.base, targets, conf, c.lengths)


# ---- device ------------------------------------------------------------------------------------------------------------------
def config(c: Chain, first: int, launch_shape: int = 0):
    cfg = MV.fit_config(c.base, launch_shape)
    cfg.num_iters, cfg.step_size = int(first), R.ADAM["lr"]
    cfg.conf_per_frame = int(c.per_frame_conf)
    return cfg


def starts(c: Chain):
    return [H.cuda(a) for a in (c.base.go, c.base.pose, c.base.shape, c.base.tr)]


def device_chain(c: Chain, first: int, follow: int, freeze: bool, launch_shape: int = 0, cfg=None, idx=None, offsets=None, model=None, prior=None,
                 cams=None, targets=None):
    """``native.fit_multiview_sequences``: a dict of packed [sum T][.] tensors."""
    from keypoints2body_amd import native
    cfg = cfg or config(c, first, launch_shape)
    return native.fit_multiview_sequences(model or G.native_model(c.kind), prior or H.native_prior(), cfg, follow, freeze,
                                          list(c.base.cams) if cams is None else cams, list(c.base.idx) if idx is None else idx, c.lengths,
                                          H.cuda(c.targets if targets is None else targets), None if c.conf is None else H.cuda(c.conf), *starts(c),
                                          offsets=offsets)


def device_loop(c: Chain, first: int, follow: int, freeze: bool, launch_shape: int):
    """The same chains driven from the host: one ``k2b_fit_multiview`` launch per step over the sequences that still have a frame,
    in the forced launch shape.  Frame 0 has preserve weight 0; frame t starts from frame t - 1's result, gets that result's body
    pose as ``preserve_pose`` and ``freeze_betas`` for the follow-up freeze."""
    from keypoints2body_amd import native
    n = int(c.lengths.sum())
    model = G.native_model(c.kind)
    out = None
    cur = starts(c)
    off = torch.as_tensor(c.offsets, device="cuda")
    targets, conf = H.cuda(c.targets), None if c.conf is None else H.cuda(c.conf)
    for t in range(int(c.lengths.max()) if len(c.lengths) else 0):
        live = torch.as_tensor(np.flatnonzero(c.lengths > t), device="cuda")
        rows = off[live] + t
        cfg = config(c, first if t == 0 else follow, launch_shape)
        cfg.pose_preserve_weight = 0.0 if t == 0 else PRESERVE
        cfg.freeze_betas = int(freeze and t > 0)
        cf = conf[rows].contiguous() if c.per_frame_conf else conf
        begin = [a[live].contiguous() for a in cur]
        o = native.fit_multiview(model, H.native_prior(), cfg, list(c.base.cams), list(c.base.idx), targets[rows].contiguous(), cf, *begin,
                                 preserve_pose=None if t == 0 else begin[1])
        if out is None:
            out = {k: torch.full((n,) + tuple(v.shape[1:]), float("nan"), device="cuda") for k, v in o.items()}
        for k in o:
            out[k][rows] = o[k]
        cur = [a.clone() for a in cur]
        for a, k in zip(cur, KEYS):
            a[live] = o[k]
    return out


assert_equal = RC.assert_equal
assert_shape_held = RC.assert_shape_held          # (reads name, kind, lengths, rows)


# ---- oracle ------------------------------------------------------------------------------------------------------------------
def oracle_cases():
    """(kind, C) of every chain the GPU oracle test gates."""
    return [(kind, C) for kind in ORACLE_KINDS for C in ORACLE_VIEWS]


@functools.lru_cache(maxsize=None)
def oracle_case(kind: str, C: int) -> Chain:
    return chain(kind, C, (ORACLE_T,) * ORACLE_S, seed=ORACLE_SEED)


def _split(lay, p):
    e = (0, 3, 3 + lay.D, 3 + lay.D + lay.NB, lay.P)
    return [p[:, a:b] for a, b in zip(e, e[1:])]


def step_case(c: Chain, t: int, params, freeze: bool, tag: str) -> MV.Case:
    """Step t of every sequence of `c` (equal lengths) as a ``multiview_common.Case``: started from `params` (go, pose, shape, tr),
    whose pose is also the preserve pose handed on at t > 0."""
    go, pose, shape, tr = params
    w = dict(c.base.weights, preserve=0.0 if t == 0 else PRESERVE)
    T = int(c.lengths[0])
    return replace(c.base, name=f"{c.name}/{tag}/step{t}", j3d=np.ascontiguousarray(c.targets[t::T]), go=go, pose=pose, shape=shape, tr=tr,
                   preserve=pose, weights=w, freeze=int(freeze and t > 0))


def oracle_adam(case: MV.Case, double: bool, iters: int, freeze: int):
    """``torch.optim.Adam`` over ``multiview_common.frame_loss`` for `iters` iterations: ([B][P] parameters after them, [B] loss
    before the last step).  With `freeze` the first ``betas_prior`` shape coefficients are not handed to the optimiser."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        lay = G.layout(case.kind)
        dt = torch.float64 if double else torch.float32
        go, pose, shape, tr = (torch.tensor(np.asarray(a), dtype=dt).requires_grad_() for a in (case.go, case.pose, case.shape, case.tr))
        head, tail = shape.detach()[:, :lay.betas_prior].clone().requires_grad_(), shape.detach()[:, lay.betas_prior:].clone().requires_grad_()
        opt = torch.optim.Adam([go, pose, tr] + ([] if freeze else [head]) + ([tail] if tail.shape[1] else []), **R.ADAM)
        lf = None
        for _ in range(iters):
            opt.zero_grad()
            lf = MV.frame_loss(case, double, go, pose, torch.cat([head, tail], dim=1), tr)
            lf.sum().backward()
            opt.step()
        return torch.cat([go, pose, head, tail, tr], dim=1).detach().double().numpy().copy(), lf.detach().double().numpy().copy()
    finally:
        torch.set_num_threads(threads)


@functools.lru_cache(maxsize=None)
def oracle_chain(kind: str, C: int, freeze: bool, double: bool):
    """The whole chain of ``oracle_case`` frame after frame: per step ([S][P] parameters, [S] loss before the last step, [S][P]
    float64 gradient at the step's start with the columns outside the optimiser zero - float64 chain only)."""
    c, lay = oracle_case(kind, C), G.layout(kind)
    cur = [np.asarray(a, dtype=np.float64 if double else np.float32) for a in (c.base.go, c.base.pose, c.base.shape, c.base.tr)]
    steps = []
    for t in range(ORACLE_T):
        case = step_case(c, t, cur, freeze, f"{'f64' if double else 'f32'}{'/frozen' if freeze else ''}")
        params, loss = oracle_adam(case, double, ORACLE_FIRST if t == 0 else ORACLE_FOLLOW, case.freeze)
        g0 = MV.oracle_eval(case, True)[1] if double else None
        steps.append((params, loss, g0))
        cur = [a if double else a.astype(np.float32) for a in _split(lay, params)]
    return steps


def f32_loop_deviation(kind: str, C: int, freeze: bool) -> float:
    """max |float32 chain - float64 chain| over every step and parameter."""
    d64, d32 = oracle_chain(kind, C, freeze, True), oracle_chain(kind, C, freeze, False)
    return max(float(np.abs(a[0] - b[0]).max()) for a, b in zip(d64, d32))
