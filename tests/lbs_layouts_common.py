"""Shared by the layout tests of ``k2b_lbs`` / ``k2b_lbs_backward`` (``tests/test_lbs_layouts_host.py``, ``tests/test_gpu_lbs_layouts.py``,
``tests/test_gpu_lbs_layouts_backward.py``); importable without a GPU.

``k2b.h`` promises the LBS pair for 17-24 and 49-56 joints with 1-32 shape coefficients, and the code branches on exactly those two
numbers: the forward's route (``k2b_model_create``: tile, stream, stream_x, stream_xw, from the number of 16-deep k-steps
``KX = 2 ceil((9 (J - 1) + NB + 2) / 32)``), the capacity of the pose set-up's shape loop, the fill of the last k-step, the
backward's feature row ``16 ceil(9 (J - 1) / 16) + (NB <= 16 ? 16 : 32)`` and the instantiation of ``k2b_vertex_term``.  TABLE
below holds one layout per branch and per fill pattern; ``expected_route`` restates the host's rule with the constants read from
the sources.

Models: prefixes of the synthetic SMPL / SMPL-X trees (valid trees: ``parents[i] < i``), 56 joints = the SMPL-X tree plus one
leaf on joint 20; V = 333 vertices (two full 128-vertex groups and a partial one with a partial 16-vertex tile and empty waves),
five vertex-selected joints.  B = 37 frames: one full 32-frame tile and five frames.

Forward gate, per frame f: ``max|dev - ref64| <= max(5e-6 * max(1, S_f), 4 * e32_f)`` over the frame's vertices and output joints,
with ref64 the float64 oracle (``oracle.smpl_torch.TorchSMPL._lbs``), S_f the largest |coordinate| of the frame's float64
vertices and e32_f the float32 oracle's own error on the frame.  5e-6 m and the scale factor are the project's forward gate
(``test_lbs_ragged_sizes_match_oracle``), the factor 4 the one ``tests/lbs_backward_common.py`` allows for
another summation order.  Condition on the inputs, from the oracle alone (so that a case cannot loosen its own gate):
``e32 <= 1.25e-6`` (a quarter of the gate) for the benign and wide regimes, ``<= 4e-6`` for the far one, where the final rounding
at 50 m is 1.9e-6 by itself.  The backward's gate is ``lbs_backward_common.gate``, the loss terms' that of
``tests/fit_gradient_common.py``.

Regime "turns" (TURN_LAYOUTS): the benign parameters with rotation vectors of several turns - TURNS = 6.5 .. 5000 rad, the pair
999 / 1001 on both sides of the branch of ``sincos_small`` to the library functions - on the root, on joint 3, and 999 / 1001 rad
on two consecutive joints of a chain (``turn_frames``).  Its gate is the one above widened per frame by d_f: the largest change
of the float64 result when every turned rotation vector is rescaled so that its angle moves by +-2 ulp of the float32 angle (a
float32 kernel forms the angle with a sum of squares and a square root: two roundings), from the float64 oracle alone.
Conditions up to 20 rad: ``e32 <= 1.25e-6`` and d_f at most the unchanged gate, so those frames are held as sharply as every
other frame.  Above 20 rad d_f dominates (the float32 oracle alone is off by 4e-6 m at 100 rad, 5e-5 m at 999 rad, 2e-4 m at
5000 rad): there the test catches a wrong quadrant, a broken reduction or a broken library branch, not an ulp."""
import dataclasses
import functools
import re
from pathlib import Path
from types import SimpleNamespace
from typing import Optional

import numpy as np
import torch

from keypoints2body_amd import synthetic
from tests import fit_gradient_common as F
from tests import lbs_backward_common as C

REPO = Path(__file__).resolve().parents[1]
CSRC = REPO / "keypoints2body_amd" / "csrc"

V_SMALL, FRAMES, NUM_EXTRA = 333, 37, 5
MODEL_SEED = 3
FORWARD_GATE = 5e-6                    # metres
E32_LIMIT = {"benign": 1.25e-6, "wide": 1.25e-6, "far": 4e-6, "turns": 1.25e-6}
REGIMES = ("benign", "wide", "far")
# Rotation vectors of several turns (legal input; optimisers produce them): the pair 999 / 1001 straddles the branch of
# ``sincos_small`` (csrc/k2b_device.h) that hands angles above 1e3 rad to the library functions.  See ``turn_frames``.
TURNS, TURN_SHARP, TURN_ULPS = F.TURNS, F.TURN_SHARP, F.TURN_ULPS
TURN_JOINT, TURN_CHAIN = 3, (1, 4)     # the single non-root joint; two consecutive joints of a chain (4's parent is 1)
TURN_LAYOUTS = ((23, 10), (24, 17), (55, 21), (56, 32))
TURN_BACKWARD_LAYOUT = (24, 17)

# (J, NB, features F = 9 (J - 1) + NB + 2, 16-deep k-steps KX, route)
TABLE = (
    (17, 1, 147, 10, "tile"),          # smallest J and NB; 9 (J - 1) = 144: no pad column in the backward
    (21, 10, 192, 12, "tile"),         # last 32-deep k-step exactly full
    (21, 11, 193, 14, "stream"),       # one feature into a new k-step; capacity 16 with NB 11; stream kernel with 21 joints
    (23, 10, 210, 14, "stream"),       # one idle joint lane
    (20, 32, 205, 14, "stream"),       # stream kernel with capacity 32
    (24, 15, 224, 14, "stream"),       # every k column of the stream kernel in use
    (23, 24, 224, 14, "stream"),       # the only e4m3 layout with capacity 32 (pose set-up <32, 3, true>); last k-step exactly full
    (24, 16, 225, 16, "tile"),         # its boundary partner; backward row with NB = 16
    (24, 17, 226, 16, "tile"),         # capacity 32; the backward's row switch; vertex_term<64, 32>
    (24, 32, 241, 16, "tile"),
    (49, 1, 435, 32, "stream_x"),      # 28 k-steps padded to 32: four all-zero ones; 9 (J - 1) = 432: no pad column
    (53, 20, 490, 32, "stream_x"),
    (55, 21, 509, 32, "stream_x"),     # capacity 32 on the 16-k-step kernel
    (55, 24, 512, 32, "stream_x"),     # exactly full
    (56, 15, 512, 32, "stream_x"),     # exactly full, no padded joint
    (56, 16, 513, 34, "stream_xw"),    # the wide kernel reached by the joint count; capacity 20
    (56, 32, 529, 34, "stream_xw"),    # the documented maximum
)
LAYOUTS = tuple((J, NB) for J, NB, _, _, _ in TABLE)
FAR_LAYOUTS = ((23, 10), (24, 16), (55, 24), (56, 32))
STREAM_LAYOUTS = tuple((J, NB) for J, NB, _, _, route in TABLE if route != "tile")
REPEAT_LAYOUTS = ((23, 10), (24, 17), (49, 1), (56, 16))
EXTRA_ROUTE_LAYOUTS = ((24, 10), (55, 21))
LANDMARK_LAYOUT = (56, 16)
PRODUCT_CASES = ((23, 10, 6890), (56, 32, 10475))            # (J, NB, V) with B = 3, benign
BACKWARD_LAYOUTS = ((17, 1), (21, 11), (24, 16), (24, 17), (49, 1), (55, 24), (56, 15), (56, 32))
BACKWARD_ALL_COTANGENTS = ((17, 1), (56, 32))                # these also run "joints" alone and "no_transl"
VERTEX_TERM_LAYOUTS = ((20, 16), (24, 17), (56, 32))         # <24, 16> with J < 24; <64, 32> by NB; <64, 32> at the maximum


def forward_cases():
    """(J, NB, regime) of every forward case at V_SMALL x FRAMES."""
    return [(J, NB, r) for J, NB in LAYOUTS for r in ("benign", "wide")] + [(J, NB, "far") for J, NB in FAR_LAYOUTS]


# ---- the host's rule ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def route_constants_in_source() -> dict:
    """kStreamKSteps, kStreamXKSteps, kStreamXWKSteps (32-deep k-steps of the three stream kernels) and kMaxXSteps (16-deep
    k-steps the pose set-up can stage), all in ``k2b_lbs_plan.h``."""
    plan = (CSRC / "k2b_lbs_plan.h").read_text()
    return {name: int(re.search(rf"constexpr int {name} = (\d+);", plan).group(1))
            for name in ("kStreamKSteps", "kStreamXKSteps", "kStreamXWKSteps", "kMaxXSteps")}


def expected_route(J: int, NB: int, constants=None):
    """(F, KX, route) as ``k2b_model_create`` decides them: 17-24 joints take the stream kernel only at its own k-step count;
    49-56 joints are padded up to the 16-k-step stream kernel or take the 17-k-step one."""
    c = constants or route_constants_in_source()
    feats = 9 * (J - 1) + NB + 2
    kx = 2 * ((feats + 31) // 32)
    groups = (J + 7) // 8
    if groups == 3:
        route = "stream" if kx == 2 * c["kStreamKSteps"] else "tile"
    elif groups == 7:
        kx = max(kx, 2 * c["kStreamXKSteps"])
        route = "stream_x" if kx == 2 * c["kStreamXKSteps"] else "stream_xw" if kx == 2 * c["kStreamXWKSteps"] else "tile"
    else:
        raise ValueError(f"{J} joints: k2b_lbs is built for 17-24 and 49-56")
    if kx > c["kMaxXSteps"]:
        raise ValueError(f"{J} joints / {NB} coefficients: {kx} k-steps, the pose set-up stages {c['kMaxXSteps']}")
    return feats, kx, route


# ---- models ---------------------------------------------------------------------------------------------------------------------
def tree(J: int):
    """(parents [J] int32, rest joints [J][3])."""
    if 17 <= J <= 24:
        return synthetic.SMPL_PARENTS[:J].copy(), synthetic._REST_JOINTS[:J].copy()
    if 49 <= J <= 55:
        return synthetic.SMPLX_PARENTS[:J].copy(), synthetic._smplx_rest_joints()[:J]
    if J == 56:                          # one leaf more on the left wrist, 5 cm off it
        rest = synthetic._smplx_rest_joints()
        leaf = rest[20] + np.array([0.03, 0.04, 0.0])
        return np.append(synthetic.SMPLX_PARENTS, np.int32(20)).astype(np.int32), np.concatenate([rest, leaf[None]], axis=0)
    raise ValueError(J)


@functools.lru_cache(maxsize=None)
def landmarks(J: int, V: int):
    """The landmark table of the LANDMARK_LAYOUT model: 51 triangles on the vertices of the joints 15 and 22."""
    return synthetic.make_landmarks(num_vertices=V, num_joints=J, joints=(15, 22))


@functools.lru_cache(maxsize=None)
def consts(J: int, NB: int, V: int = V_SMALL, variant: str = "tagged"):
    """`variant`: "tagged" (five extra joints on distinct vertices: they ride in the W image), "gather" (two of them on one vertex:
    the gather launch), "none" (no extra joints), "landmarks" (as tagged; the native model also gets ``landmarks(J, V)``)."""
    parents, rest = tree(J)
    c = synthetic.make_body_model(MODEL_SEED, num_vertices=V, num_betas=NB, parents=parents, rest=rest,
                                  num_extra=0 if variant == "none" else NUM_EXTRA)
    if variant == "gather":
        ids = c.extra_vertex_ids.copy()
        ids[2] = ids[0]
        c = dataclasses.replace(c, extra_vertex_ids=ids)
    return c


@functools.lru_cache(maxsize=None)
def oracle(J: int, NB: int, V: int, variant: str, double: bool):
    from oracle.smpl_torch import TorchSMPL
    return TorchSMPL(consts(J, NB, V, variant), dtype=torch.float64 if double else torch.float32)


_native = {}


def native_model(J: int, NB: int, V: int = V_SMALL, variant: str = "tagged", env=None):
    """The device model; `env` = (monkeypatch, name, value): created with that variable set (read at creation, per model)."""
    from keypoints2body_amd.native import NativeModel
    key = (J, NB, V, variant, None if env is None else env[1:])
    if key not in _native:
        c = consts(J, NB, V, variant)
        make = lambda: NativeModel(c.v_template, c.shapedirs, c.posedirs, c.J_regressor, c.lbs_weights, c.parents, c.extra_vertex_ids,
                                   landmarks=landmarks(J, V) if variant == "landmarks" else None)
        if env is None:
            _native[key] = make()
        else:
            with env[0].context() as mp:
                mp.setenv(env[1], env[2])
                _native[key] = make()
    return _native[key]


# ---- parameters -----------------------------------------------------------------------------------------------------------------
def _unit(a):
    return a / np.sqrt((a * a).sum(axis=-1, keepdims=True))


@functools.lru_cache(maxsize=None)
def params(J: int, NB: int, regime: str, B: int = FRAMES):
    """(global_orient, pose of all non-root joints, shape, transl) as float32 arrays, seeded per layout and regime.  Frame 1: all-zero
    pose and root; frame 2: the angles of ``fit_gradient_common.LADDER`` about seeded axes on the joints 0..7; frame 3: 2 rad about
    seeded axes on every joint.  Regime "turns": the benign parameters with the frames of ``turn_frames`` changed."""
    if regime == "turns":
        return _turn_params(J, NB, B)
    rng = np.random.default_rng([J, NB, REGIMES.index(regime)])
    D = 3 * (J - 1)
    if regime == "benign":              # the scales of tests/test_gpu_smplx_wide.py
        go, pose = 0.2 * rng.standard_normal((B, 3)), 0.15 * rng.standard_normal((B, D))
        shape, tr = 0.3 * rng.standard_normal((B, NB)), rng.standard_normal((B, 3))
    else:                               # the regime of test_lbs_ragged_sizes_match_oracle; far: 50 m off the origin
        go, pose = rng.uniform(-3.0, 3.0, (B, 3)), 0.6 * rng.standard_normal((B, D))
        shape = rng.uniform(-2.5, 2.5, (B, NB))
        reach = 50.0 if regime == "far" else 5.0
        tr = rng.uniform(-reach, reach, (B, 3))
    full = np.concatenate([go, pose], axis=1).reshape(B, J, 3)
    axes = _unit(rng.standard_normal((2, J, 3)))
    if B > 1:
        full[1] = 0.0
    if B > 2:
        full[2, :len(F.LADDER)] = axes[0, :len(F.LADDER)] * np.asarray(F.LADDER)[:, None]
    if B > 3:
        full[3] = 2.0 * axes[1]
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return f32(full[:, 0]), f32(full[:, 1:].reshape(B, D)), f32(shape), f32(tr)


@functools.lru_cache(maxsize=None)
def backward_params(J: int, NB: int, B: int = 3, scales=(0.3, 0.2, 0.5, 1.0)):
    """As ``lbs_backward_common.packed``: seeded frames at the scales of ``synthetic.make_poses`` (root 0.3, pose 0.2, shape 0.5,
    translation 1), frame 1 an all-zero pose, frame 2 a rotation of 2 rad about a seeded axis on every joint."""
    D = 3 * (J - 1)
    seed = 100 * J + NB
    f = lambda stream, cols, scale: scale * synthetic.normalish(stream, (B, cols), seed)
    go, pose, shape, tr = f(90, 3, scales[0]), f(91, D, scales[1]), f(92, NB, scales[2]), f(93, 3, scales[3])
    if B >= 3:
        go[1] = 0.0
        pose[1] = 0.0
        axes = 2.0 * _unit(synthetic.normalish(94, (J, 3), seed))
        go[2] = axes[0]
        pose[2] = axes[1:].reshape(-1)
    return tuple(np.ascontiguousarray(a, dtype=np.float32) for a in (go, pose, shape, tr))


# ---- several turns ----------------------------------------------------------------------------------------------------------------
TURN_FRAMES = 4 + 2 * len(TURNS) + 1   # frames a batch needs to hold every turned frame


def turn_frames() -> dict:
    """frame -> ((joint, angle), ...): from frame 4 on one frame per angle of TURNS with the angle on the root, one per angle with
    it on TURN_JOINT, and one frame with 999 and 1001 rad on the two joints of TURN_CHAIN."""
    n = len(TURNS)
    out = {4 + i: ((0, a),) for i, a in enumerate(TURNS)}
    out.update({4 + n + i: ((TURN_JOINT, a),) for i, a in enumerate(TURNS)})
    out[4 + 2 * n] = ((TURN_CHAIN[0], 999.0), (TURN_CHAIN[1], 1001.0))
    return out


def turn_angle(B: int = FRAMES) -> np.ndarray:
    """[B]: the largest turned angle of the frame (0 for the frames left benign)."""
    out = np.zeros(B)
    for f, turned in turn_frames().items():
        out[f] = max(a for _, a in turned)
    return out


def _turn_params(J: int, NB: int, B: int):
    assert B >= TURN_FRAMES
    go, pose, shape, tr = (a.copy() for a in params(J, NB, "benign", B))
    full = np.concatenate([go, pose], axis=1).reshape(B, J, 3).astype(np.float64)
    axes = _unit(np.random.default_rng([J, NB, 1000]).standard_normal((B, 2, 3)))
    for f, turned in turn_frames().items():
        for i, (joint, angle) in enumerate(turned):
            full[f, joint] = angle * axes[f, i]
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return f32(full[:, 0]), f32(full[:, 1:].reshape(B, 3 * (J - 1))), shape, tr


def turn_rescaled(p: tuple, sign: float) -> tuple:
    """The parameters in float64 with every turned rotation vector rescaled so that its angle moves by `sign` * TURN_ULPS ulp of
    the float32 angle."""
    go, pose, shape, tr = (np.asarray(a, dtype=np.float64).copy() for a in p)
    B, J = go.shape[0], 1 + pose.shape[1] // 3
    full = np.concatenate([go, pose], axis=1).reshape(B, J, 3)
    for f, turned in turn_frames().items():
        for joint, _ in turned:
            angle = float(np.sqrt((full[f, joint] ** 2).sum()))
            full[f, joint] *= (angle + sign * TURN_ULPS * float(np.spacing(np.float32(angle)))) / angle
    return np.ascontiguousarray(full[:, 0]), np.ascontiguousarray(full[:, 1:].reshape(B, 3 * (J - 1))), shape, tr


def turn_summary(ref, joints, vertices) -> str:
    """The worst error per turned angle (its frames together), for the log and DESIGN.md."""
    err = np.maximum(frame_error(joints, ref.joints), frame_error(vertices, ref.vertices) if vertices is not None else 0.0)
    angle = turn_angle(len(err))
    return " ".join(f"{a:g}:{err[angle == a].max():.2e}/{ref.tol[angle == a].min():.2e}" for a in sorted(set(angle[angle > 0])))


# ---- forward reference and gate -------------------------------------------------------------------------------------------------
def _output_joints(joints, verts, lmk):
    """smplx's output joints: J kinematic, E vertex-selected, then the landmark rows combined from the (translated) vertices."""
    if lmk is None:
        return joints
    ids = torch.as_tensor(lmk[0].astype(np.int64))
    w = torch.as_tensor(lmk[1]).to(verts.dtype)
    return torch.cat([joints, (verts[:, ids] * w[None, :, :, None]).sum(dim=2)], dim=1)


def _forward(J, NB, V, variant, p, double: bool, with_transl: bool):
    dt = torch.float64 if double else torch.float32
    go, pose, shape, tr = (torch.tensor(a, dtype=dt) for a in p)
    with torch.no_grad():
        joints, verts = oracle(J, NB, V, variant, double)._lbs(torch.cat([go, pose], dim=1), shape, tr if with_transl else None)
        joints = _output_joints(joints, verts, landmarks(J, V) if variant == "landmarks" else None)
    return joints.double(), verts.double()


@dataclasses.dataclass(frozen=True, eq=False)
class Reference:
    name: str
    params: tuple                 # float32 arrays
    joints: torch.Tensor          # float64 (B, J + E (+ L), 3)
    vertices: torch.Tensor        # float64 (B, V, 3)
    scale: np.ndarray             # [B]: S_f
    e32: np.ndarray               # [B]: e32_f
    widen: Optional[np.ndarray] = None   # [B]: d_f of the "turns" regime

    @property
    def base_tol(self):
        return np.maximum(FORWARD_GATE * np.maximum(1.0, self.scale), 4.0 * self.e32)

    @property
    def tol(self):
        return self.base_tol if self.widen is None else self.base_tol + self.widen


def frame_error(got: torch.Tensor, ref: torch.Tensor) -> np.ndarray:
    """[B]: max|got - ref| per frame; a frame with a value that is not finite counts as infinitely off."""
    d = (got.detach().cpu().double() - ref).abs().flatten(1)
    return torch.where(torch.isfinite(d), d, torch.full_like(d, float("inf"))).amax(dim=1).numpy()


@functools.lru_cache(maxsize=None)
def reference(J: int, NB: int, regime: str, V: int = V_SMALL, B: int = FRAMES, variant: str = "tagged", with_transl: bool = True) -> Reference:
    """The float64 forward of ``params(J, NB, regime, B)``, computed once, with the float32 oracle's error per frame (on one
    thread: the float32 sums, and with them the gate, do not depend on how many cores the machine offers)."""
    p = params(J, NB, regime, B)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        j64, v64 = _forward(J, NB, V, variant, p, True, with_transl)
        j32, v32 = _forward(J, NB, V, variant, p, False, with_transl)
        widen = None
        if regime == "turns":             # d_f: what TURN_ULPS ulp of the float32 angle do to the float64 result, either way
            moved = [_forward(J, NB, V, variant, turn_rescaled(p, sign), True, with_transl) for sign in (1.0, -1.0)]
            widen = np.max([np.maximum(frame_error(j, j64), frame_error(v, v64)) for j, v in moved], axis=0)
    finally:
        torch.set_num_threads(threads)
    e32 = np.maximum(frame_error(j32, j64), frame_error(v32, v64))
    name = f"{J}/{NB} {regime} V={V} B={B}" + ("" if variant == "tagged" else f" {variant}") + ("" if with_transl else " no transl")
    return Reference(name, p, j64, v64, v64.abs().flatten(1).amax(dim=1).numpy(), e32, widen)


def check_inputs(ref: Reference, regime: str):
    """The condition on the inputs: the float32 oracle itself stays within its share of the gate."""
    if regime == "turns":
        # the frames turned by more than TURN_SHARP rad are held to d_f (the float32 angle itself is 2 ulp uncertain); up to it
        # the widening stays within the unchanged gate, and every frame's float32 oracle within the benign limit
        sharp = turn_angle(len(ref.e32)) <= TURN_SHARP
        assert (ref.widen[turn_angle(len(ref.e32)) == 0] == 0).all()
        assert (ref.widen[sharp] <= ref.base_tol[sharp]).all(), f"{ref.name}: d_f {ref.widen[sharp].max():.2e} above the gate at an angle <= {TURN_SHARP}"
        worst = float(ref.e32[sharp].max())
        assert worst <= E32_LIMIT[regime], f"{ref.name}: the float32 oracle is off by {worst:.2e} m at an angle <= {TURN_SHARP} (limit {E32_LIMIT[regime]:.2e})"
        return
    worst = float(ref.e32.max())
    assert worst <= E32_LIMIT[regime], (f"{ref.name}: the float32 oracle is off by {worst:.2e} m (frame {int(ref.e32.argmax())}, limit "
                                        f"{E32_LIMIT[regime]:.2e}): badly conditioned, change the seed or the scale")


def forward_gate(ref: Reference, joints, vertices, what: str = ""):
    """Print the measured maxima, then assert the per-frame gate; `vertices` may be None (a joints-only call)."""
    tol = ref.tol
    ej = frame_error(joints, ref.joints)
    ev = frame_error(vertices, ref.vertices) if vertices is not None else np.zeros_like(ej)
    err = np.maximum(ej, ev)
    worst = int((err / tol).argmax())
    print(f"forward {ref.name}{what}: vertices {ev.max():.3e} joints {ej.max():.3e} e32 {ref.e32.max():.3e} S {ref.scale.max():.2f} "
          f"worst frame {worst}: {err[worst]:.3e} of {tol[worst]:.3e}")
    assert (err <= tol).all(), (f"{ref.name}{what}: frame {worst} is off by {err[worst]:.3e} m (vertices {ev[worst]:.3e}, joints {ej[worst]:.3e}), "
                                f"gate {tol[worst]:.3e} (S {ref.scale[worst]:.2f}, e32 {ref.e32[worst]:.2e})")


# ---- backward: autograd through the oracle ------------------------------------------------------------------------------------------
def oracle_grads(J, NB, V, variant, p, cot_joints, cot_verts, double: bool, with_transl: bool = True):
    """``torch.autograd.grad`` of <cot_joints, joints> + <cot_verts, vertices> (``lbs_backward_common.oracle_grads`` for these models)."""
    dt = torch.float64 if double else torch.float32
    leaves = [torch.tensor(a, dtype=dt, requires_grad=True) for a in p[:3]]
    tr = torch.tensor(p[3] if with_transl else np.zeros_like(p[3]), dtype=dt, requires_grad=True)
    joints, verts = oracle(J, NB, V, variant, double)._lbs(torch.cat(leaves[:2], dim=1), leaves[2], tr)
    joints = _output_joints(joints, verts, landmarks(J, V) if variant == "landmarks" else None)
    loss = 0.0
    if cot_joints is not None:
        loss = loss + (torch.as_tensor(cot_joints).to(dt) * joints).sum()
    if cot_verts is not None:
        loss = loss + (torch.as_tensor(cot_verts).to(dt) * verts).sum()
    return dict(zip(C.GROUPS, torch.autograd.grad(loss, leaves + [tr])))


def _frame_group_error(got: dict, ref: dict) -> dict:
    """``lbs_backward_common.group_error``'s statistic per frame: group -> [B]."""
    out = {}
    for k in C.GROUPS:
        g, r = got[k].detach().cpu().double(), ref[k].detach().cpu().double()
        num, den = (g - r).abs().amax(dim=1), r.abs().amax(dim=1)
        num = torch.where(torch.isfinite(num), num, torch.full_like(num, float("inf")))
        out[k] = torch.where(den > 0, num / den.clamp_min(1e-300), num).numpy()
    return out


@functools.lru_cache(maxsize=None)
def turn_backward_reference(J: int, NB: int, B: int = TURN_FRAMES):
    """(parameters, cotangents (joints, vertices), float64 gradients, e32 [B], d group -> [B]) of the "turns" frames for
    ``k2b_lbs_backward``, from the oracle alone: e32_f the float32 autograd's error on frame f (``lbs_backward_common``'s statistic,
    the largest over the groups), d_f the largest change of the float64 gradient when every turned angle moves by TURN_ULPS ulp
    of the float32 angle, either way.  Asserted: up to TURN_SHARP rad d_f stays within the unchanged gate 2e-5."""
    p = params(J, NB, "turns", B)
    rng = np.random.default_rng([J, NB, 77])
    gj = rng.standard_normal((B, J + NUM_EXTRA, 3)).astype(np.float32)
    gv = rng.standard_normal((B, V_SMALL, 3)).astype(np.float32)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        g64 = oracle_grads(J, NB, V_SMALL, "tagged", p, gj, gv, True)
        g32 = oracle_grads(J, NB, V_SMALL, "tagged", p, gj, gv, False)
        moved = [oracle_grads(J, NB, V_SMALL, "tagged", turn_rescaled(p, sign), gj, gv, True) for sign in (1.0, -1.0)]
    finally:
        torch.set_num_threads(threads)
    e32 = np.max(list(_frame_group_error(g32, g64).values()), axis=0)
    a, b = (_frame_group_error(m, g64) for m in moved)
    widen = {k: np.maximum(a[k], b[k]) for k in C.GROUPS}
    sharp = turn_angle(B) <= TURN_SHARP
    for k, v in widen.items():
        assert (v[sharp] <= F.GRAD_GATE).all(), f"backward turns {J}/{NB}: d_f of {k} is {v[sharp].max():.2e} at an angle <= {TURN_SHARP}"
    assert (e32[sharp] <= F.E32_LIMIT).all(), (J, NB, e32)
    return p, (gj, gv), g64, e32, widen


def turn_backward_gate(J: int, NB: int, got: dict):
    """``lbs_backward_common.gate`` per frame, widened by d_f: ``max|g - g64| <= (max(2e-5, 4 e32_f) + d_kf) max|g64|`` over group k
    of frame f.  Above TURN_SHARP rad d_f dominates: there the test catches a wrong quadrant, a broken reduction or a broken
    library branch, not an ulp."""
    _, _, g64, e32, widen = turn_backward_reference(J, NB)
    err = _frame_group_error(got, g64)
    angle = turn_angle(len(e32))
    for a in sorted(set(angle)):
        rows = angle == a
        print(f"backward turns {J}/{NB} {a:g} rad: " + " ".join(f"{k}={err[k][rows].max():.2e}" for k in C.GROUPS) +
              f" e32={e32[rows].max():.2e} d={max(widen[k][rows].max() for k in C.GROUPS):.2e}")
    for k in C.GROUPS:
        tol = np.maximum(F.GRAD_GATE, 4.0 * e32) + widen[k]
        worst = int((err[k] / tol).argmax())
        assert (err[k] <= tol).all(), f"backward turns {J}/{NB}: {k} of frame {worst} ({angle[worst]:g} rad) off by {err[k][worst]:.2e}, gate {tol[worst]:.2e}"


# ---- the stand-alone loss terms (k2b_vertex_term, k2b_surface_term) ---------------------------------------------------------------
TERM_SIGMA, TERM_WEIGHT = 100.0, 600.0
# Residuals of the terms' targets.  These calls have three to twenty targets per frame, so nothing averages out: a float32 forward
# rounds a coordinate of about a metre by up to 6e-8 m, which moves a quadratic loss of residual r by 2 * 6e-8 / r of itself.  For
# that to stay below an eighth of the loss gate (fit_gradient_common's rule for one rounding: a forward makes a handful of them) r
# has to be at least 16 * 6e-8 / 2e-6 = 0.48 m.  (Sigma is 100 m: the GMoF stays quadratic.)  Asserted per case in float64 alone,
# for the loss and for every gradient group (``term_reference``).
TERM_OFFSET = 0.5
TERM_ROUNDING_LIMIT_LOSS = F.LOSS_GATE / 8.0


def term_groups(J: int, NB: int):
    D = 3 * (J - 1)
    return SimpleNamespace(groups=(("global_orient", 0, 3), ("body_pose", 3, 3 + D), ("betas", 3 + D, 3 + D + NB),
                                   ("transl", 3 + D + NB, 3 + D + NB + 3)))


def term_params(J: int, NB: int, B: int = 3):
    """The scales of ``fit_gradient_common.base`` (coordinates within about a metre), frames 1 and 2 as ``backward_params``."""
    return backward_params(J, NB, B, scales=(0.3, 0.2, 0.5, F.TRANSL_SCALE))


def term_targets(J, NB, V, variant, p, rows, conf_seed: int):
    """(targets [B][T][3] float32: the float64 output joints `rows` and TERM_OFFSET of seeded noise; confidences [B][T] float32 in
    0.5 .. 1.5 with one zero)."""
    j64, _ = _forward(J, NB, V, variant, p, True, True)
    B, T = j64.shape[0], len(rows)
    tgt = (j64[:, list(rows)].numpy() + TERM_OFFSET * synthetic.normalish(95, (B, T, 3), conf_seed)).astype(np.float32)
    conf = (0.5 + synthetic.uniform(96, B * T, conf_seed).reshape(B, T)).astype(np.float32)
    conf[1, min(3, T - 1)] = 0.0
    return tgt, conf


@dataclasses.dataclass(frozen=True, eq=False)
class TermCase:
    name: str
    J: int
    NB: int
    variant: str
    params: tuple
    index: tuple                  # what the entry takes: indices into the extra joints (vertex term) or model joint rows (surface term)
    rows: tuple                   # rows of the output joints
    targets: np.ndarray
    conf: np.ndarray              # [T] or [B][T]


@functools.lru_cache(maxsize=None)
def vertex_term_case(J: int, NB: int, B: int = 3) -> TermCase:
    """Four of the five extra joints, one confidence per target (the entry takes no table), one of them zero."""
    p = term_params(J, NB, B)
    sel = (0, 2, 3, 4)
    rows = tuple(J + e for e in sel)
    tgt, conf = term_targets(J, NB, V_SMALL, "tagged", p, rows, conf_seed=41)
    conf = conf[0].copy()
    conf[1] = 0.0
    return TermCase(f"vertex term {J}/{NB}", J, NB, "tagged", p, sel, rows, tgt, conf)


@functools.lru_cache(maxsize=None)
def surface_term_case(B: int = 3) -> TermCase:
    """The landmark model: three extra joints and every third landmark, per-frame confidences."""
    J, NB = LANDMARK_LAYOUT
    p = term_params(J, NB, B)
    first = J + NUM_EXTRA
    rows = (J, J + 2, J + 4) + tuple(range(first, first + landmarks(J, V_SMALL)[0].shape[0], 3))
    tgt, conf = term_targets(J, NB, V_SMALL, "landmarks", p, rows, conf_seed=43)
    return TermCase(f"surface term {J}/{NB}", J, NB, "landmarks", p, rows, rows, tgt, conf)


def term_oracle(case: TermCase, double: bool, targets=None):
    """(loss [B], gradient [B][P] in the packed layout) of ``w^2 conf^2 sum gmof(joint - target)`` by autograd, as float64 arrays."""
    from oracle.fit_torch import gmof
    dt = torch.float64 if double else torch.float32
    leaves = [torch.tensor(a, dtype=dt, requires_grad=True) for a in case.params]
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        joints, verts = oracle(case.J, case.NB, V_SMALL, case.variant, double)._lbs(torch.cat(leaves[:2], dim=1), leaves[2], leaves[3])
        joints = _output_joints(joints, verts, landmarks(case.J, V_SMALL) if case.variant == "landmarks" else None)[:, list(case.rows)]
        c = torch.tensor(case.conf, dtype=dt)
        c = c[None] if c.dim() == 1 else c
        w = float(np.float32(TERM_WEIGHT))
        tgt = torch.tensor(case.targets if targets is None else targets, dtype=dt)
        lf = ((w * w) * (c * c)[..., None] * gmof(joints - tgt, float(np.float32(TERM_SIGMA)))).sum(dim=(1, 2))
        grads = torch.autograd.grad(lf.sum(), leaves)
    finally:
        torch.set_num_threads(threads)
    return lf.detach().double().numpy(), torch.cat(grads, dim=1).double().numpy()


@dataclasses.dataclass(frozen=True, eq=False)
class TermReference:
    loss64: np.ndarray
    g64: np.ndarray
    e32: dict
    e32_loss: float
    rounding: dict                # group -> what one float32 rounding of the targets does to it
    rounding_loss: float


_term_references = {}


def term_reference(case: TermCase) -> TermReference:
    """The case's oracle results, computed once; asserts the conditions on the inputs (``fit_gradient_common.reference``'s, and
    the same for the loss)."""
    if case.name not in _term_references:
        lay = term_groups(case.J, case.NB)
        loss64, g64 = term_oracle(case, True)
        loss32, g32 = term_oracle(case, False)
        sign = np.where(synthetic.uniform(80, case.targets.size, 31).reshape(case.targets.shape) < 0.5, -1.0, 1.0)
        moved = case.targets.astype(np.float64) + 0.5 * np.spacing(np.abs(case.targets)).astype(np.float64) * sign
        loss_m, g_m = term_oracle(case, True, targets=moved)
        _term_references[case.name] = TermReference(
            loss64, g64, {k: float(v.max()) for k, v in F.group_errors(g32, g64, lay).items()},
            float((np.abs(loss32 - loss64) / np.abs(loss64)).max()),
            {k: float(v.max()) for k, v in F.group_errors(g_m, g64, lay).items()}, float((np.abs(loss_m - loss64) / np.abs(loss64)).max()))
    r = _term_references[case.name]
    for k, v in r.rounding.items():
        assert v <= F.ROUNDING_LIMIT, f"{case.name}: one float32 rounding of the targets moves {k} by {v:.2e} (limit {F.ROUNDING_LIMIT:.1e}): badly conditioned"
    assert r.rounding_loss <= TERM_ROUNDING_LIMIT_LOSS, f"{case.name}: one float32 rounding of the targets moves the loss by {r.rounding_loss:.2e}"
    for k, v in dict(r.e32, loss=r.e32_loss).items():
        assert v <= F.E32_LIMIT, f"{case.name}: the float32 oracle is off by {v:.2e} in {k}: badly conditioned"
    return r


def term_gate(case: TermCase, loss, grad):
    """The gate of ``tests/fit_gradient_common.py``: per parameter group and frame ``max|g - g64| <= max(2e-5, 4 e32_k) max|g64|``, the
    loss per frame within ``max(2e-6, 4 e32_loss)`` of itself."""
    ref = term_reference(case)
    lay = term_groups(case.J, case.NB)
    loss, grad = loss.detach().cpu().double().numpy(), grad.detach().cpu().double().numpy()
    err = F.group_errors(grad, ref.g64, lay)
    tol = {k: max(F.GRAD_GATE, F.ORDER_FACTOR * ref.e32[k]) for k in err}
    e_loss = float((np.abs(loss - ref.loss64) / np.abs(ref.loss64)).max())
    tol_loss = max(F.LOSS_GATE, F.ORDER_FACTOR * ref.e32_loss)
    print(f"term {case.name}: loss={e_loss:.2e}/{ref.e32_loss:.2e}/{tol_loss:.2e} " +
          " ".join(f"{k}={v.max():.2e}/{ref.e32[k]:.2e}/{tol[k]:.2e}" for k, v in err.items()) + "  (error/e32/tol)")
    assert np.isfinite(grad).all() and np.isfinite(loss).all(), case.name
    for k, v in err.items():
        assert (v <= tol[k]).all(), f"{case.name}: {k} off by {v.max():.2e} of the group's largest entry (frame {int(v.argmax())}), gate {tol[k]:.2e}"
    assert e_loss <= tol_loss, f"{case.name}: loss off by {e_loss:.2e}, gate {tol_loss:.2e}"
