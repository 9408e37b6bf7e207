"""GPU: every entry keeps to the header's rules for the caller's buffers (``include/k2b.h``, Conventions; arena,
guards and batch sizes: ``tests/caller_buffers_common.py``, held to their premises by ``tests/test_caller_buffers_conditions.py``).

A. Every call runs twice: once with the binding's own allocation - the path the other GPU tests hold to float64 oracles - and
once with every output carved out of one guarded arena (``native.outputs_from``).  Then: every guard float still has the sentinel's
bits (nothing was written in front of, behind or a row away from an output), no output element has them (every element was
written), every input - device tensors and host index arrays - has the bits of its snapshot, and the two results are
``torch.equal``.  No tolerance anywhere.

B. The in-place fits: the provider hands ``k2b_fit_world`` / ``k2b_fit_image`` / ``k2b_fit_multiview`` / ``k2b_fit_world_lbfgs`` the input
tensors themselves as the four fitted parameters; ``preserve_pose`` and ``transl_prior_target`` NULL (their defaults are the initial
parameters, which the call overwrites), or the ``body_pose`` / ``transl`` tensor itself.  Gate: bit equality with the out-of-place
call on clones taken before.

Shapes are the smallest with a partial tail: odd batches (a half-filled slot pair), 17 frames (one more than a workgroup holds),
6890 vertices (430 tiles of 16 and 10), 255 / 257 elements around a 256-thread block, ragged chains with a one-frame sequence and
an empty one.  Two Adam iterations keep the moments live; two L-BFGS iterations reach the history."""
from pathlib import Path

import numpy as np
import pytest
import torch

from keypoints2body_amd import native, synthetic
from tests import call_history_common as C
from tests import caller_buffers_common as A
from tests import fit_gradient_common as F
from tests import helpers as H
from tests import isolation_common as I
from tests import lbs_layouts_common as L
from tests import multiview_common as MV
from tests import reproj_chain_common as RC
from tests import reproj_common as R
from tests import reproj_surface_common as RS

pytestmark = pytest.mark.gpu

ITERS = 2
LBFGS = dict(max_iter=2, lr=1.0, tolerance_grad=0.0, tolerance_change=0.0)
P = native.PARAM_KEYS
TILE_SWITCH = "K2B_LBS_TILE"


def _cus() -> int:
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- the two protocols -----------------------------------------------------------------------------------------------------------
def _held(call, inputs: dict, what: str) -> dict:
    """A: `call()` -> dict of result tensors under the names of ``native.outputs_from``; `inputs`: everything the call reads."""
    torch.cuda.synchronize()
    want_dev = call()
    want = C.to_host(want_dev)
    C.assert_finite(want, what)
    arena = A.Arena(A.requests_like(want_dev), device="cuda")
    snap = A.snapshot(inputs)
    with native.outputs_from(arena.provider):
        got = call()
    torch.cuda.synchronize()
    views = arena.outputs()
    assert {k for k, v in got.items() if v is not None} == set(views), (what, sorted(got), sorted(views))
    for k, v in views.items():
        assert got[k].data_ptr() == v.data_ptr(), f"{what}: {k} did not come from the provider"
    arena.check(what)
    A.assert_inputs_unwritten(inputs, snap, what)
    C.assert_same(C.to_host(got), want, f"{what}, into the caller's arena,")
    return want


IN_PLACE_VARIANTS = ("defaults", "preserve_is_body_pose", "transl_target_is_transl")


def _in_place(call, inputs: dict, what: str, variant: str):
    """B: `call(go, pose, shape, tr, preserve_pose, transl_prior_target)` -> the fit's result dict; `inputs` holds the four start
    tensors under PARAM_KEYS and every other device input of the call."""
    start = [inputs[k].clone() for k in P]
    ref_in = [t.clone() for t in start]
    pick = lambda params: (params[1] if variant == "preserve_is_body_pose" else None, params[3] if variant == "transl_target_is_transl" else None)
    torch.cuda.synchronize()
    want_dev = call(*ref_in, *pick([t.clone() for t in start]))
    want = C.to_host(want_dev)
    C.assert_finite(want, what)
    for k, a, b in zip(P, ref_in, start):
        assert torch.equal(a, b), f"{what}: the out-of-place call wrote its input {k}"
    live = dict(zip(P, start))
    others = {k: v for k, v in inputs.items() if k not in live}
    snap = A.snapshot(others)
    arena = A.Arena([(k, tuple(v.shape)) for k, v in want_dev.items() if k not in live], device="cuda")
    with native.outputs_from(lambda name, shape: live[name] if name in live else arena.provider(name, shape)):
        got = call(*start, *pick(start))
    torch.cuda.synchronize()
    for k in P:
        assert got[k].data_ptr() == live[k].data_ptr(), f"{what}: {k} is not the input buffer"
    arena.check(what)
    A.assert_inputs_unwritten(others, snap, what)
    C.assert_same(C.to_host(got), want, f"{what}, in place ({variant}),")
    assert not torch.equal(want["body_pose"], inputs["body_pose"].cpu()), f"{what}: the fit did not move the pose"
    # the control: the centre matters in this case - preserving the FITTED pose (what a call that lost the initial one would do
    # from its second iteration on) gives another result, so the equality above is not one of a term that is switched off
    moved = C.to_host(call(*[t.clone() for t in ref_in], want_dev["body_pose"].clone(), None))
    assert not torch.equal(moved["body_pose"], want["body_pose"]), f"{what}: the preserve centre does not reach the result"
    if variant == "transl_target_is_transl":
        moved = C.to_host(call(*[t.clone() for t in ref_in], None, want_dev["transl"].clone()))
        assert not torch.equal(moved["transl"], want["transl"]), f"{what}: the translation prior's centre does not reach the result"


# ---- fit inputs ----------------------------------------------------------------------------------------------------------------------
def _fit_inputs(case: F.Case, shared_conf: bool = False) -> dict:
    dev = lambda a: None if a is None else H.cuda(np.ascontiguousarray(a))
    conf = case.conf[0] if shared_conf else case.conf              # one row for every frame, or the case's own table
    out = dict(zip(P, (dev(a) for a in (case.go, case.pose, case.shape, case.tr))))
    out.update(idx=np.asarray(case.idx, dtype=np.int32), j3d=dev(case.j3d), conf=dev(conf), preserve=dev(case.preserve), tr_target=dev(case.tr_target))
    return out


def _adam(cfg, iters: int = ITERS):
    cfg.num_iters, cfg.step_size = iters, native.default_fit_config().step_size
    return cfg


def _world_call(entry, model, cfg, a: dict, want_grad: bool, head=(), **kw):
    """The out-of-place call of A on the inputs `a` (preserve pose and prior centre as tensors of their own)."""
    return lambda: entry(model, H.native_prior(), cfg, *head, list(a["idx"]), a["j3d"], a["conf"], *(a[k] for k in P), preserve_pose=a["preserve"],
                         want_grad=want_grad, transl_prior_target=a["tr_target"], **kw)


def _world_in_place(entry, model, cfg, a: dict, head=(), **kw):
    return lambda go, pose, shape, tr, preserve, target: entry(model, H.native_prior(), cfg, *head, list(a["idx"]), a["j3d"], a["conf"], go, pose, shape, tr,
                                                               preserve_pose=preserve, want_grad=True, transl_prior_target=target, **kw)


def _without_centres(a: dict) -> dict:
    return {k: v for k, v in a.items() if k not in ("preserve", "tr_target")}


# ---- A.1 k2b_fit_world, the fused kernel -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", A.FUSED_BATCHES)
@pytest.mark.parametrize("shape", (0, 1, 2, 3, 4))
@pytest.mark.parametrize("kind", ("smpl10", "smpl16"))
def test_fused_fit_writes_its_outputs_and_nothing_else(kind, shape, B):
    """The automatic shape and the four forced ones at 1, 5 and 17 frames (half-filled slot pairs; 17: one frame in a second
    workgroup of the paired and wide shapes), with 10 shape coefficients and in the 16-wide instantiation; ``grad_out`` on and
    off, one confidence row for all frames and one per frame."""
    assert F.layout(kind).kernel == "fused" and B < _cus()
    case = C.fit_case(kind, B)
    for shared_conf in (False, True):
        a = _fit_inputs(case, shared_conf)
        cfg = _adam(F.fit_config(case, shape))
        cfg.conf_per_frame = int(not shared_conf)
        for want_grad in (True, False):
            out = _held(_world_call(native.fit_world, F.native_model(kind), cfg, a, want_grad), a,
                        f"k2b_fit_world {kind} shape {shape} B={B} grad={want_grad} shared_conf={shared_conf}")
            assert ("grad" in out) == want_grad and not torch.equal(out["body_pose"], a["body_pose"].cpu())


# ---- A.2 the tree kernel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("shape", (1, 2), ids=("plain", "comp_waves"))
@pytest.mark.parametrize("kind", ("smplh", "smplx20"))
def test_tree_fit_writes_its_outputs_and_nothing_else(kind, shape, B):
    assert kind in F.TREE_KINDS and F.layout(kind).kernel == "tree"
    case = C.fit_case(kind, B)
    a = _fit_inputs(case)
    _held(_world_call(native.fit_world, F.native_model(kind), _adam(F.fit_config(case, shape)), a, True), a, f"k2b_fit_world {kind} tree shape {shape} B={B}")


# ---- A.3 surface targets ---------------------------------------------------------------------------------------------------------------
def _surface_problem(route: str, B: int):
    idx, tgt, conf, p = C.surface_inputs(route, B)
    J = L.LANDMARK_LAYOUT[0]
    surface = [j for j in idx if j >= J]
    assert len(surface) <= 32 and (any(j >= J + L.NUM_EXTRA for j in surface) == (route == "landmarks"))       # vertex-term route / surface kernel
    a = dict(zip(P, (H.cuda(x) for x in p)))
    a.update(idx=np.asarray(idx, dtype=np.int32), j3d=H.cuda(tgt), conf=H.cuda(conf), preserve=None, tr_target=None)
    cfg = native.default_fit_config()
    cfg.num_iters, cfg.prior_pose_dims, cfg.conf_per_frame, cfg.pose_preserve_weight = ITERS, 63, 1, 5.0
    return L.native_model(*L.LANDMARK_LAYOUT, variant="landmarks"), cfg, a


@pytest.mark.parametrize("route", C.SURFACE_ROUTES)
def test_surface_target_fit_writes_its_outputs_and_nothing_else(route):
    model, cfg, a = _surface_problem(route, 3)
    _held(_world_call(native.fit_world, model, cfg, a, True), a, f"k2b_fit_world surface targets ({route})")


# ---- A.4 k2b_fit_image, A.5 k2b_fit_multiview ------------------------------------------------------------------------------------------
def _image_case(which: str, B: int):
    if which == "kinematic/fused":
        return R.base(RS.FUSED, B=B)
    if which == "kinematic/tree":
        return R.base(RS.TREE, B=B)
    return RS.fit_case({"surface/fused": RS.FUSED, "surface/tree": RS.TREE, "surface/landmarks": RS.LMK_KIND}[which], which == "surface/landmarks", B=B)


@pytest.mark.parametrize("which", ("kinematic/fused", "kinematic/tree", "surface/fused", "surface/tree", "surface/landmarks"))
def test_fit_image_writes_its_outputs_and_nothing_else(which):
    case = _image_case(which, 3)
    a = _fit_inputs(case)
    _held(_world_call(native.fit_image, RS.native_model(case), _adam(R.fit_config(case)), a, True), a, f"k2b_fit_image {which}")


def _multiview_problem(kind: str, B: int):
    case = MV.base(kind, 2, B=B)
    a = _fit_inputs(case)
    table = native.camera_table(list(case.cams))
    a["cameras"] = np.frombuffer(table, dtype=np.uint8)               # the host camera table, as bytes
    return case, a, table


@pytest.mark.parametrize("B", (1, 5))
@pytest.mark.parametrize("kind", MV.BOTH)
def test_fit_multiview_writes_its_outputs_and_nothing_else(kind, B):
    case, a, table = _multiview_problem(kind, B)
    _held(_world_call(native.fit_multiview, F.native_model(kind), _adam(MV.fit_config(case)), a, True, head=(table,)), a, f"k2b_fit_multiview {kind} C=2 B={B}")


# ---- A.6 k2b_fit_world_lbfgs -----------------------------------------------------------------------------------------------------------
def _lbfgs_problem(name: str):
    lc, cus = I.CASE[name], _cus()
    assert I.lbfgs_scheme(lc, cus) == lc.scheme and I.workgroup_frames(lc, cus)[0] >= 2
    case = C.fit_case(lc.kind, lc.frames(cus))
    return lc, case, _fit_inputs(case)


@pytest.mark.parametrize("name", C.LBFGS_CASES)
def test_device_lbfgs_writes_its_outputs_and_nothing_else(name):
    """The three launch schemes and the wide driver at ``isolation_common``'s batches (a multiple of the compute units less one:
    the last workgroup is ragged)."""
    lc, case, a = _lbfgs_problem(name)
    _held(_world_call(native.fit_world_lbfgs, F.native_model(lc.kind), F.fit_config(case), a, True, **LBFGS), a, f"k2b_fit_world_lbfgs {name} B={case.frames}")


# ---- A.7 chains ------------------------------------------------------------------------------------------------------------------------
def _chain_cfg(case: F.Case, shape: int, lbfgs: bool = False):
    cfg = F.fit_config(case) if lbfgs else _adam(F.fit_config(case, shape))
    cfg.transl_prior_weight = 0.0                                    # (not built into a chain)
    return cfg


def _ragged_problem(kind: str, lengths):
    lengths = np.asarray(lengths, dtype=np.int32)
    off = native.ragged_offsets(lengths)
    case = C.fit_case(kind, int(lengths.sum()))
    a = _without_centres(_fit_inputs(case))
    a.update({k: H.cuda(np.ascontiguousarray(x[off])) for k, x in zip(P, (case.go, case.pose, case.shape, case.tr))})
    a.update(lengths=lengths, offsets=off)
    return case, a


@pytest.mark.parametrize("kernel", tuple(C.CHAIN_KINDS))
def test_fit_sequence_writes_its_outputs_and_nothing_else(kernel):
    kind, shape = C.CHAIN_KINDS[kernel]
    S = T = 3
    case = C.fit_case(kind, S * T)
    K = case.j3d.shape[1]
    a = _without_centres(_fit_inputs(case))
    a.update(j3d=H.cuda(case.j3d.reshape(S, T, K, 3)), conf=H.cuda(case.conf.reshape(S, T, K)))
    a.update({k: H.cuda(np.ascontiguousarray(x[::T])) for k, x in zip(P, (case.go, case.pose, case.shape, case.tr))})
    cfg = _chain_cfg(case, shape)
    out = _held(lambda: native.fit_sequence(F.native_model(kind), H.native_prior(), cfg, ITERS, list(a["idx"]), a["j3d"], a["conf"], *(a[k] for k in P)), a,
                f"k2b_fit_sequence {kernel} S=3 T=3")
    assert tuple(out["body_pose"].shape[:2]) == (S, T)


@pytest.mark.parametrize("lengths", ((3, 1, 2), (1,)), ids=str)
@pytest.mark.parametrize("kernel", tuple(C.CHAIN_KINDS))
def test_fit_sequences_writes_its_outputs_and_nothing_else(kernel, lengths):
    kind, shape = C.CHAIN_KINDS[kernel]
    case, a = _ragged_problem(kind, lengths)
    cfg = _chain_cfg(case, shape)
    _held(lambda: native.fit_sequences(F.native_model(kind), H.native_prior(), cfg, ITERS, list(a["idx"]), a["lengths"], a["j3d"], a["conf"], *(a[k] for k in P),
                                       offsets=a["offsets"]), a, f"k2b_fit_sequences {kernel} {lengths}")


@pytest.mark.parametrize("lengths", ((3, 1, 2), (1,)), ids=str)
@pytest.mark.parametrize("kernel", tuple(C.CHAIN_KINDS))
def test_fit_image_sequences_writes_its_outputs_and_nothing_else(kernel, lengths):
    kind, shape = C.CHAIN_KINDS[kernel]
    c = RC.chain(kind, tuple(lengths), per_frame_conf=True)
    a = dict(zip(P, RC.starts(c)))
    a.update(idx=np.asarray(c.base.idx, dtype=np.int32), j3d=H.cuda(c.targets), conf=H.cuda(c.conf), lengths=np.array(c.lengths, dtype=np.int32),
             offsets=native.ragged_offsets(c.lengths))
    cfg = RC.config(c, ITERS, shape)
    _held(lambda: native.fit_image_sequences(F.native_model(kind), H.native_prior(), cfg, ITERS, True, list(a["idx"]), a["lengths"], a["j3d"], a["conf"],
                                             *(a[k] for k in P), offsets=a["offsets"]), a, f"k2b_fit_image_sequences {kernel} {lengths}")


def test_fit_sequence_lbfgs_writes_its_outputs_and_nothing_else():
    kind, T = "smpl10", 3
    case = C.fit_case(kind, T)
    a = _without_centres(_fit_inputs(case))
    a.update({k: H.cuda(np.ascontiguousarray(x[:1])) for k, x in zip(P, (case.go, case.pose, case.shape, case.tr))})
    cfg = _chain_cfg(case, 0, lbfgs=True)
    kw = {k: v for k, v in LBFGS.items() if k != "max_iter"}
    _held(lambda: native.fit_sequence_lbfgs(F.native_model(kind), H.native_prior(), cfg, LBFGS["max_iter"], LBFGS["max_iter"], list(a["idx"]), a["j3d"], a["conf"],
                                            *(a[k] for k in P), **kw), a, "k2b_fit_sequence_lbfgs T=3")


def test_fit_sequences_lbfgs_writes_its_outputs_and_nothing_else():
    kind, lengths = "smpl10", (2, 1, 3)
    case, a = _ragged_problem(kind, lengths)
    cfg = _chain_cfg(case, 0, lbfgs=True)
    kw = {k: v for k, v in LBFGS.items() if k != "max_iter"}
    _held(lambda: native.fit_sequences_lbfgs(F.native_model(kind), H.native_prior(), cfg, LBFGS["max_iter"], LBFGS["max_iter"], list(a["idx"]), a["lengths"], a["j3d"],
                                             a["conf"], *(a[k] for k in P), offsets=a["offsets"], **kw), a, f"k2b_fit_sequences_lbfgs {lengths}")


# ---- A.8 k2b_shape_pass_lbfgs ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, free", (("smpl10", 10), ("smpl16", 10), ("smpl16", 16)), ids=str)
def test_shape_pass_writes_its_rows_at_the_output_pitch(kind, free):
    """Three sequences, the middle one empty (it returns its start).  ("smpl16", 10): fewer free coefficients than the model has,
    so a row of the optimiser's state (pitch NB = 16) is longer than a row of ``betas_out`` (pitch 10)."""
    lengths = (3, 0, 2)
    N, S = sum(lengths), len(lengths)
    assert F.layout(kind).NB >= free and ((kind, free) != ("smpl16", 10) or F.layout(kind).NB > free)
    case = C.fit_case(kind, N)
    a = dict(j3d=H.cuda(case.j3d), conf=H.cuda(case.conf), global_orient=H.cuda(case.go), body_pose=H.cuda(case.pose),
             root_targets=H.cuda(np.ascontiguousarray(case.j3d[:, 0])), betas_in=H.cuda(np.ascontiguousarray(case.shape[:S, :free])),
             seq_offsets=torch.tensor(np.concatenate(([0], np.cumsum(lengths))), dtype=torch.int32, device="cuda"), idx=np.asarray(case.idx, dtype=np.int32))
    cfg = native.default_fit_config()
    out = _held(lambda: {"betas": native.shape_pass_lbfgs(F.native_model(kind), H.native_prior(), cfg, a["seq_offsets"], list(a["idx"]), a["j3d"], a["conf"],
                                                          a["global_orient"], a["body_pose"], a["root_targets"], 0, a["betas_in"], **LBFGS)}, a,
                f"k2b_shape_pass_lbfgs {kind} free={free}")
    start = a["betas_in"].cpu()
    assert torch.equal(out["betas"][1], start[1]) and not torch.equal(out["betas"][0], start[0]) and not torch.equal(out["betas"][2], start[2])


# ---- A.9 k2b_lbs, A.10 k2b_lbs_backward ------------------------------------------------------------------------------------------------
V_SMPL = L.PRODUCT_CASES[0][2]
# (J, NB, V, variant): the SMPL-sized model (430 full 16-vertex tiles and one of 10), every small-V layout of the layout table
# (333 vertices: 20 full tiles and one of 13) and the landmark model; the tile twins of the layouts a stream kernel takes
_SMPL_SIZED = L.PRODUCT_CASES[0][:2] + (V_SMPL, "tagged")
_LANDMARKS = L.LANDMARK_LAYOUT + (L.V_SMALL, "landmarks")
LBS_LAYOUTS = (_SMPL_SIZED,) + tuple((J, NB, L.V_SMALL, "tagged") for J, NB in L.LAYOUTS) + (_LANDMARKS,)
BACKWARD_LAYOUTS = (_SMPL_SIZED,) + tuple((J, NB, L.V_SMALL, "tagged") for J, NB in L.BACKWARD_LAYOUTS) + (_LANDMARKS,)
_streamed = lambda layouts: tuple(lay for lay in layouts if lay[3] == "tagged" and L.expected_route(lay[0], lay[1])[2] != "tile")
LBS_TWINS, BACKWARD_TWINS = _streamed(LBS_LAYOUTS), _streamed(BACKWARD_LAYOUTS)


def _lbs_model(lay, monkeypatch=None):
    J, NB, V, variant = lay
    return L.native_model(J, NB, V, variant, env=None if monkeypatch is None else (monkeypatch, TILE_SWITCH, "1"))


def _lbs_check(lay, model, B: int, what: str):
    J, NB, V, _ = lay
    p = dict(zip(P, (H.cuda(x) for x in L.params(J, NB, "benign", B))))
    for want_vertices in (True, False):
        for with_transl in (True, False):
            def call():
                joints, verts = model.lbs(p["global_orient"], p["body_pose"], p["betas"], p["transl"] if with_transl else None, want_vertices=want_vertices)
                return {"joints": joints, "vertices": verts} if want_vertices else {"joints": joints}
            out = _held(call, p, f"k2b_lbs {what} B={B} vertices={want_vertices} transl={with_transl}")
            assert tuple(out["joints"].shape) == (B, model.num_output_joints, 3)


def test_the_smpl_sized_model_ends_in_a_partial_tile():
    assert V_SMPL == 6890 and V_SMPL % 16 == 10 and L.V_SMALL % 16 != 0


@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("lay", LBS_LAYOUTS, ids=str)
def test_lbs_writes_its_outputs_and_nothing_else(lay, B):
    _lbs_check(lay, _lbs_model(lay), B, str(lay))


@pytest.mark.parametrize("lay", LBS_TWINS, ids=str)
def test_lbs_tile_twin_writes_its_outputs_and_nothing_else(lay, monkeypatch):
    for B in (1, 3):
        _lbs_check(lay, _lbs_model(lay, monkeypatch), B, f"{lay} under {TILE_SWITCH}")


WANT_MASKS = tuple(tuple(i != off for i in range(4)) for off in range(4)) + ((True, True, True, True),)


def _backward_check(lay, model, what: str):
    J, NB, V, _ = lay
    B = 3
    rng = np.random.default_rng([J, NB, V, 7])
    a = dict(zip(P, (H.cuda(x) for x in L.backward_params(J, NB, B))))
    a.update(grad_joints=H.cuda(rng.standard_normal((B, model.num_output_joints, 3)).astype(np.float32)),
             grad_vertices=H.cuda(rng.standard_normal((B, V, 3)).astype(np.float32)))
    for want in WANT_MASKS:
        def call():
            grads = model.lbs_backward(*(a[k] for k in P), a["grad_joints"], a["grad_vertices"], want=want)
            return {f"grad_{k}": g for k, g in zip(P, grads) if g is not None}
        out = _held(call, a, f"k2b_lbs_backward {what} want={want}")
        assert set(out) == {f"grad_{k}" for k, w in zip(P, want) if w}


@pytest.mark.parametrize("lay", BACKWARD_LAYOUTS, ids=str)
def test_lbs_backward_writes_the_wanted_gradients_and_nothing_else(lay):
    _backward_check(lay, _lbs_model(lay), str(lay))


@pytest.mark.parametrize("lay", BACKWARD_TWINS, ids=str)
def test_lbs_backward_on_the_tile_twin(lay, monkeypatch):
    _backward_check(lay, _lbs_model(lay, monkeypatch), f"{lay} under {TILE_SWITCH}")


# ---- A.11 the stand-alone terms --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("term", ("vertex", "surface", "surface_image"))
def test_stand_alone_terms_write_their_outputs_and_nothing_else(term):
    case = {"vertex": lambda: L.vertex_term_case(24, 17, 3), "surface": lambda: L.surface_term_case(3), "surface_image": RS.base}[term]()
    assert case.targets.shape[0] == 3
    variant = "landmarks" if term == "surface_image" else case.variant
    model = L.native_model(case.J, case.NB, L.V_SMALL, variant)
    index = case.rows if term == "surface_image" else case.index
    a = dict(zip(P, (H.cuda(x) for x in case.params)))
    a.update(targets=H.cuda(case.targets), conf=H.cuda(case.conf), index=np.asarray(index, dtype=np.int32))
    if term == "surface_image":
        run = lambda: native.surface_term_image(model, list(a["index"]), a["targets"], a["conf"], RS.SIGMA, RS.WEIGHT, case.focal, *(a[k] for k in P))
    else:
        entry = native.vertex_term if term == "vertex" else native.surface_term
        run = lambda: entry(model, list(a["index"]), a["targets"], a["conf"], L.TERM_SIGMA, L.TERM_WEIGHT, *(a[k] for k in P))
    _held(lambda: dict(zip(("loss", "grad"), run())), a, f"k2b_{term}_term")


# ---- A.12 .. A.15 the entries with 256-thread blocks over n, and the IK-GAT net -------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 255, 257))
def test_adam_step_updates_its_three_blocks_and_nothing_else(n):
    """``params``, ``m`` and ``v`` are views of an arena (the entry updates in place); ``grad`` is an input."""
    rng = np.random.default_rng([5, n])
    x0, g, m0, v0 = (H.cuda(rng.standard_normal(n).astype(np.float32)) for _ in range(4))
    v0 = v0.abs()
    want = {"params": x0.clone(), "m": m0.clone(), "v": v0.clone()}
    native.adam_step(want["params"], g, want["m"], want["v"], 3, 1e-2)
    arena = A.Arena([(k, (n,)) for k in want], device="cuda")
    views = arena.outputs()
    for k, t in (("params", x0), ("m", m0), ("v", v0)):
        views[k].copy_(t)
    snap = A.snapshot({"grad": g})
    native.adam_step(views["params"], g, views["m"], views["v"], 3, 1e-2)
    torch.cuda.synchronize()
    arena.check(f"k2b_adam_step n={n}")
    A.assert_inputs_unwritten({"grad": g}, snap, f"k2b_adam_step n={n}")
    C.assert_same(C.to_host(views), C.to_host(want), f"k2b_adam_step n={n}")
    assert not torch.equal(views["params"], x0)


@pytest.mark.parametrize("n", (1, 257))
def test_angular_error_writes_its_output_and_nothing_else(n):
    rng = np.random.default_rng([13, n])
    a = {k: H.cuda(rng.standard_normal((n, 3)).astype(np.float32)) for k in ("pred", "gt")}
    _held(lambda: {"deg": native.angular_error_deg(a["pred"], a["gt"])}, a, f"k2b_angular_error_deg n={n}")


@pytest.mark.parametrize("N", (5, 70))
@pytest.mark.parametrize("align", tuple(native.POINT_ALIGN_MODES))
def test_point_error_writes_its_outputs_and_nothing_else(align, N):
    rng = np.random.default_rng([9, N])
    a = {k: H.cuda(rng.standard_normal((3, N, 3)).astype(np.float32)) for k in ("pred", "gt")}
    a["weights"] = H.cuda((0.5 + rng.random((3, N))).astype(np.float32))
    assert N == 5 or N > 64                                          # five points, and more than one wave of them
    _held(lambda: dict(zip(("err", "per_point", "transform"), native.point_error(a["pred"], a["gt"], weights=a["weights"], align=align, per_point=True, transform=True))),
          a, f"k2b_point_error {align} N={N}")


_nets = {}


def _ikgat(IN: int):
    """The small nets of ``tests/test_gpu_ikgat_oracle.py`` (TAIL_NETS F5 / F12), created once."""
    if IN not in _nets:
        from keypoints2body_amd.core.estimators import ikgat
        J, HID, NL, NH = (24, 64, 2, 2) if IN == 9 else (22, 32, 1, 2)
        parents = [int(p) for p in synthetic.SMPL_PARENTS[:J]]
        state = synthetic.make_ikgat_state(J, IN, HID, NL, NH, seed=3)
        spec = ikgat.IkgatSpec(path=Path("."), model_type="pos_to_rot6" if IN == 3 else "pos-rot6_to_rot6", input_dim=IN, parents=tuple(parents), hidden_dim=HID,
                               num_layers=NL, num_heads=NH)
        packed = ikgat.pack_state({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in state.items()}, spec)
        _nets[IN] = native.NativeIkgat(parents, packed, IN, HID, NL, NH)
    return _nets[IN]


@pytest.mark.parametrize("chain", (False, True), ids=("independent", "chain"))
@pytest.mark.parametrize("IN", (3, 9))
def test_ikgat_predict_writes_its_output_and_nothing_else(IN, chain):
    net, T = _ikgat(IN), 3
    rng = np.random.default_rng([17, IN])
    a = {"positions": H.cuda((0.5 * rng.standard_normal((T, net.num_joints, 3))).astype(np.float32))}
    if IN == 9:
        a["quat_in"] = H.cuda(rng.standard_normal((T, net.num_joints, 4)).astype(np.float32))
    _held(lambda: {"quaternions": net.predict(a["positions"], a.get("quat_in"), chain=chain)}, a, f"k2b_ikgat_predict input_dim={IN} chain={chain}")


# ---- B. in-place fits ----------------------------------------------------------------------------------------------------------------
IN_PLACE_B = 5


def _variants(takes_transl_prior: bool):
    return IN_PLACE_VARIANTS if takes_transl_prior else IN_PLACE_VARIANTS[:2]


@pytest.mark.parametrize("variant", IN_PLACE_VARIANTS)
@pytest.mark.parametrize("shape", (0, 1, 2, 3, 4))
def test_fused_fit_in_place(shape, variant):
    case = C.fit_case("smpl10", IN_PLACE_B)
    assert case.weights["preserve"] > 0 and case.weights["transl"] > 0
    a = _without_centres(_fit_inputs(case))
    _in_place(_world_in_place(native.fit_world, F.native_model("smpl10"), _adam(F.fit_config(case, shape)), a), a, f"k2b_fit_world fused shape {shape}", variant)


@pytest.mark.parametrize("variant", _variants(False))
@pytest.mark.parametrize("shape", (1, 2), ids=("plain", "comp_waves"))
def test_tree_fit_in_place(shape, variant):
    """(The tree kernel takes no translation prior: the entry refuses the weight and the centre.)"""
    case = C.fit_case("smplx20", IN_PLACE_B)
    assert case.weights["preserve"] > 0 and case.weights["transl"] == 0
    a = _without_centres(_fit_inputs(case))
    _in_place(_world_in_place(native.fit_world, F.native_model("smplx20"), _adam(F.fit_config(case, shape)), a), a, f"k2b_fit_world tree shape {shape}", variant)


@pytest.mark.parametrize("variant", _variants(False))
@pytest.mark.parametrize("route", C.SURFACE_ROUTES)
def test_surface_target_fit_in_place(route, variant):
    """Both routes run the Adam loop as pairs of launches that step the OUTPUT buffers in place: ``host::start_in_place`` skips the
    copy of a parameter whose output is its input, and keeps copies of the preserve pose for the later iterations."""
    model, cfg, a = _surface_problem(route, IN_PLACE_B)
    assert cfg.pose_preserve_weight > 0
    _in_place(_world_in_place(native.fit_world, model, cfg, _without_centres(a)), _without_centres(a), f"k2b_fit_world surface targets ({route})", variant)


@pytest.mark.parametrize("which, variant", [("surface/fused", v) for v in _variants(True)] + [("surface/landmarks", v) for v in _variants(False)])
def test_fit_image_with_surface_targets_in_place(which, variant):
    case = _image_case(which, IN_PLACE_B)
    takes = F.layout(case.kind).kernel == "fused"
    assert takes == (which == "surface/fused")                       # (the landmark model runs the tree kernel: no translation prior to alias)
    assert case.weights["preserve"] > 0 and (case.weights["transl"] > 0) == takes
    a = _without_centres(_fit_inputs(case))
    _in_place(_world_in_place(native.fit_image, RS.native_model(case), _adam(R.fit_config(case)), a), a, f"k2b_fit_image {which}", variant)


@pytest.mark.parametrize("variant", IN_PLACE_VARIANTS)
def test_fit_multiview_in_place(variant):
    case, a, table = _multiview_problem("smpl10", IN_PLACE_B)
    assert case.weights["preserve"] > 0 and case.weights["transl"] > 0
    a = _without_centres(a)
    _in_place(_world_in_place(native.fit_multiview, F.native_model("smpl10"), _adam(MV.fit_config(case)), a, head=(table,)), a, "k2b_fit_multiview C=2", variant)


@pytest.mark.parametrize("name, variant", [(n, v) for n in C.LBFGS_CASES for v in _variants(n != "lbfgs/wide")])
def test_device_lbfgs_in_place(name, variant):
    """Every scheme needs its own frames per compute unit, so these run at ``isolation_common``'s batches, not at five frames."""
    lc, case, a = _lbfgs_problem(name)
    takes = F.layout(lc.kind).kernel == "fused"
    assert takes == (name != "lbfgs/wide")                           # (the wide driver runs the tree kernel: no translation prior)
    assert case.weights["preserve"] > 0 and (case.weights["transl"] > 0) == takes
    a = _without_centres(a)
    kw = dict(LBFGS)
    call = lambda go, pose, shape, tr, preserve, target: native.fit_world_lbfgs(F.native_model(lc.kind), H.native_prior(), F.fit_config(case), list(a["idx"]), a["j3d"],
                                                                                 a["conf"], go, pose, shape, tr, preserve_pose=preserve, transl_prior_target=target,
                                                                                 want_grad=True, **kw)
    _in_place(call, a, f"k2b_fit_world_lbfgs {name} B={case.frames}", variant)
