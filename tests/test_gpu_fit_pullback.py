"""Gates for a future attempt at the pull-back of the fused fit kernel's tree pass (``k2b_fit.hip``): the subtree torque and
force of a joint, expressed in its PARENT's frame, ``Rgp^T v``.  Nothing in the tree pass changed with this file: the kernel forms
the pull-back as ``R (Rg^T v)`` from the lane's own two rotations, and fetching the parent's global rotation from the parent's lane
instead was measured and is slower ("Rejected": wide rows 5).  Whoever tries again starts from these gates.  The
poses put the rotation where a wrong parent frame shows: on the root alone (every joint's parent frame is turned, the root's own
is the identity), along one arm chain (a parent frame that differs from joint to joint), and on the spine with the only live
target on the head (the gradient of 3, 6 and 9 is the torque of one force, pulled back through one, two and three turned
parents).  Oracle, gate and the evaluate-only device call are those of tests/fit_gradient_common.py, unchanged.

The one test that runs code changed together with this file is the second: the row waves of the 16-wave shape change their
priority several times per iteration, which cannot change a bit, and the launch shapes are held to each other over
100 iterations on the same poses.

Lanes beyond the tree: the fused kernel's entry takes the 24-joint tree only, so there they are lanes 24..31 of every 32-lane
half, and the whole upper half in the one-tree-per-wave shape.  A 17-joint model, the smallest the model handle takes, goes to
``k2b_fit_tree.hip`` (same two-rotation pull-back, its own code), with the bending prior's indices moved inside its 48 pose
dimensions: the defaults (52, 55) lie beyond them, the entry refuses them and the oracle cannot index them."""
import functools

import numpy as np
import pytest
import torch

from keypoints2body_amd import synthetic
from tests import fit_gradient_common as F
from tests import helpers as H

pytestmark = pytest.mark.gpu

POSES = ("root", "arm", "spine_head")
TARGETS = (22, 24)                       # 22: deepest target at depth 7, three doubling rounds; 24: the hands at depth 8, four
BETAS = (10, 16)                         # the kernel's two instantiations by shape coefficients
ARM = (13, 16, 18, 20)                   # left collar, shoulder, elbow, wrist
SPINE, HEAD = (3, 6, 9), 15
SEED = 41
OUT_KEYS = ("global_orient", "body_pose", "betas", "transl", "loss", "grad")
SWITCH = "K2B_FIT_SCAN64"


def _unit(stream, rows):
    a = synthetic.normalish(stream, (rows, 3), SEED)
    return a / np.sqrt((a * a).sum(axis=1, keepdims=True))


@functools.lru_cache(maxsize=None)
def _case(pose_name: str, K: int, nb: int) -> F.Case:
    """Two frames of ``fit_gradient_common.base`` (shape, translation, preserve offset, translation-prior centre) with every
    rotation zero but the named ones; frame 1 turns about other axes by other angles than frame 0."""
    kind = f"smpl{nb}"
    b = F.base(kind, B=2, seed=SEED)
    full = np.zeros((2, 24, 3))
    if pose_name == "root":
        full[:, 0] = _unit(90, 2) * np.asarray([2.0, -1.9])[:, None]
    elif pose_name == "arm":
        for i, j in enumerate(ARM):
            full[:, j] = _unit(91 + i, 2) * np.asarray([0.9 + 0.1 * i, -(0.7 + 0.15 * i)])[:, None]
    else:
        for i, j in enumerate(SPINE):
            full[:, j] = _unit(95 + i, 2) * np.asarray([0.6 + 0.1 * i, -(0.8 - 0.1 * i)])[:, None]
    go, pose = full[:, 0].astype(np.float32), full[:, 1:].reshape(2, -1).astype(np.float32)
    j3d = (F.joints64(kind, go, pose, b.shape, b.tr)[:, :K] + F.TARGET_OFFSET * synthetic.normalish(74, (2, K, 3), SEED)).astype(np.float32)
    conf = None
    if pose_name == "spine_head":
        # every target but the head's has confidence zero and lies a metre off: it must contribute nothing (the number of
        # doubling rounds still follows the deepest joint among the K targets)
        conf = np.zeros(K, dtype=np.float32)
        conf[HEAD] = 1.0
        j3d[:, conf == 0.0] += np.float32(1.0)
    return F.replace(b, name=f"{kind}/pullback/{pose_name}{K}", idx=tuple(range(K)), j3d=j3d, go=go, pose=pose, conf=conf,
                     preserve=pose + (b.preserve - b.pose))


def _native(kind: str):
    from keypoints2body_amd.native import NativeModel
    c = F.consts(kind)
    return NativeModel(c.v_template, c.shapedirs, c.posedirs, c.J_regressor, c.lbs_weights, c.parents, c.extra_vertex_ids)


def _closure(case: F.Case, model, shape: str = "auto"):
    """``fit_gradient_common.device_eval`` on a given model handle."""
    from keypoints2body_amd import native
    ins = [H.cuda(a) for a in (case.go, case.pose, case.shape, case.tr)]
    out = native.fit_world(model, H.native_prior(), F.fit_config(case, H.LAUNCH_SHAPES[shape]), list(case.idx), H.cuda(case.j3d),
                           None if case.conf is None else H.cuda(case.conf), *ins, preserve_pose=H.cuda(case.preserve), want_grad=True,
                           transl_prior_target=H.cuda(case.tr_target))
    for k, x in zip(native.PARAM_KEYS, ins):
        assert torch.equal(out[k], x), f"{case.name}: an evaluate-only closure moved {k}"
    return out["loss"].cpu().double().numpy(), out["grad"].cpu().double().numpy()


# ---- 1. gradient after one iteration against the float64 oracle -----------------------------------------------------------------
@pytest.mark.parametrize("nb", BETAS)
@pytest.mark.parametrize("K", TARGETS)
@pytest.mark.parametrize("pose_name", POSES)
def test_gradient_meets_the_oracle_gate(pose_name, K, nb):
    case = _case(pose_name, K, nb)
    assert case.frames == 2
    F.gate(case, *F.device_eval(case))


# ---- 2. the launch shapes agree bit for bit after 100 iterations ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _batch(K: int, nb: int):
    """16 frames: the six frames of the three poses, repeated (CPU arrays, never changed)."""
    cases = [_case(p, K, nb) for p in POSES]
    rows = lambda get: np.concatenate([get(c) for c in cases])[np.arange(16) % 6]
    # (one confidence row per frame: the head-only frames keep theirs, the others have every target live)
    conf = np.concatenate([np.broadcast_to(np.ones(K, np.float32) if c.conf is None else c.conf, (2, K)) for c in cases])[np.arange(16) % 6]
    return dict(j3d=rows(lambda c: c.j3d), go=rows(lambda c: c.go), pose=rows(lambda c: c.pose), shape=rows(lambda c: c.shape),
                tr=rows(lambda c: c.tr), conf=np.ascontiguousarray(conf))


def _fit100(K, nb, n, shape):
    from keypoints2body_amd import native
    q = _batch(K, nb)
    cfg = native.default_fit_config()
    cfg.num_iters = 100
    cfg.conf_per_frame = 1
    cfg.debug_launch_shape = H.LAUNCH_SHAPES[shape]
    c = lambda k: H.cuda(q[k][:n])
    return native.fit_world(F.native_model(f"smpl{nb}"), H.native_prior(), cfg, list(range(K)), c("j3d"), c("conf"), c("go"), c("pose"),
                            c("shape"), c("tr"), want_grad=True)


@pytest.mark.parametrize("K,nb", [(22, 10), (24, 16)])
@pytest.mark.parametrize("n", [9, 16])
def test_launch_shapes_are_bit_identical_after_100_iterations(n, K, nb):
    wide = _fit100(K, nb, n, "wide")
    for k in OUT_KEYS:
        assert wide[k].shape[0] == n and torch.isfinite(wide[k]).all(), f"{n} frames: {k} of the wide shape is not finite"
    assert not torch.equal(wide["body_pose"], H.cuda(_batch(K, nb)["pose"][:n])), "the fit did not move"
    for shape in ("paired", "split", "split_paired"):
        other = _fit100(K, nb, n, shape)
        for k in OUT_KEYS:
            assert torch.equal(wide[k], other[k]), f"{n} frames, {K} targets, {nb} betas: {k} of the wide shape differs from the {shape} shape"


# ---- 3. a tree without a scan plan: the fp64 instantiation ------------------------------------------------------------------------
_twins = {}


def _twin(monkeypatch, kind):
    """The model created under K2B_FIT_SCAN64=1 (set around the creation only: the switch is read there, per model)."""
    if kind not in _twins:
        with monkeypatch.context() as mp:
            mp.setenv(SWITCH, "1")
            _twins[kind] = _native(kind)
    return _twins[kind]


@pytest.mark.parametrize("K", TARGETS)
@pytest.mark.parametrize("pose_name", POSES)
def test_fp64_scan_instantiation_meets_the_same_gate(monkeypatch, pose_name, K):
    case = _case(pose_name, K, 10)
    F.gate(case, *_closure(case, _twin(monkeypatch, case.kind)), what=" fp64 scans")


# ---- 4. lanes beyond the tree ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ("split", "split_paired", "paired", "wide"))
def test_lanes_beyond_the_tree_stay_identities(shape):
    """The root's parent frame and that of every lane beyond the 24 joints is the identity: the root's gradient (a wrong parent
    frame turns it) passes the gate in every shape - one tree per wave, with an empty upper half, and two - and every fitted
    parameter is finite after 10 iterations from the 2 rad root."""
    from keypoints2body_amd import native
    case = _case("root", 24, 10)
    F.gate(case, *_closure(case, F.native_model(case.kind), shape), what=f" {shape}")
    cfg = F.fit_config(case, H.LAUNCH_SHAPES[shape])
    cfg.num_iters, cfg.step_size = 10, native.default_fit_config().step_size
    out = native.fit_world(F.native_model(case.kind), H.native_prior(), cfg, list(case.idx), H.cuda(case.j3d), None,
                           *(H.cuda(a) for a in (case.go, case.pose, case.shape, case.tr)), preserve_pose=H.cuda(case.preserve),
                           want_grad=True, transl_prior_target=H.cuda(case.tr_target))
    for k in OUT_KEYS:
        assert torch.isfinite(out[k]).all(), f"{shape}: {k} is not finite after 10 iterations"
    assert not torch.equal(out["global_orient"], H.cuda(case.go)), "the fit did not move"


# ---- 4b. a 17-joint model, on the tree kernel ---------------------------------------------------------------------------------------
TREE17 = "tree17"
TREE17_ANGLE_IDX = (40, 43, 9, 12)       # the bending prior's four indices inside 3 * 16 = 48 pose dimensions (defaults: 52, 55, 9, 12)


def _tree17(monkeypatch):
    """The first 17 joints of the SMPL tree as a model of ``fit_gradient_common`` (registered for this test only) and the oracle's
    bending prior on TREE17_ANGLE_IDX."""
    import oracle.fit_torch as O
    monkeypatch.setitem(F.TREES, TREE17, [int(p) for p in synthetic.SMPL_PARENTS[:17]])
    monkeypatch.setattr(O, "ANGLE_IDX", TREE17_ANGLE_IDX)
    assert F.layout(TREE17).kernel == "tree" and F.layout(TREE17).J == 17 and F.layout(TREE17).D == 48


def _tree17_fit(case, num_iters):
    from keypoints2body_amd import native
    cfg = F.fit_config(case)
    for i, a in enumerate(TREE17_ANGLE_IDX):
        cfg.angle_prior_index[i] = a
    if num_iters > 1:
        cfg.num_iters, cfg.step_size = num_iters, native.default_fit_config().step_size
    ins = [H.cuda(a) for a in (case.go, case.pose, case.shape, case.tr)]
    out = native.fit_world(F.native_model(TREE17), H.native_prior(), cfg, list(case.idx), H.cuda(case.j3d), None, *ins,
                           preserve_pose=H.cuda(case.preserve), want_grad=True)
    return out, ins


def test_seventeen_joint_model_meets_the_gate_and_stays_finite(monkeypatch):
    """2 frames, every loss term the tree kernel has, targets on all 17 joints: the gradient of one evaluate-only closure passes
    the oracle gate, and every fitted parameter, the loss and the gradient are finite after 10 iterations."""
    from keypoints2body_amd import native
    _tree17(monkeypatch)
    case = F.base(TREE17, B=2, seed=SEED)
    assert case.tr_target is None and case.weights["transl"] == 0.0 and case.weights["bending"] > 0.0
    out, ins = _tree17_fit(case, 1)
    for k, x in zip(native.PARAM_KEYS, ins):
        assert torch.equal(out[k], x), f"{case.name}: an evaluate-only closure moved {k}"
    F.gate(case, out["loss"].cpu().double().numpy(), out["grad"].cpu().double().numpy())
    out, ins = _tree17_fit(case, 10)
    for k in OUT_KEYS:
        assert torch.isfinite(out[k]).all(), f"{k} is not finite after 10 iterations"
    assert not torch.equal(out["body_pose"], ins[1]), "the fit did not move"
