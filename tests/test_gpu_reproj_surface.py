"""Projected surface targets on the device: ``k2b_surface_term_image`` (the perspective form of the surface-point kernel) and
``k2b_fit_image`` (kinematic joints and surface targets of 2D keypoints in one Adam fit), against the float64 oracle of
tests/reproj_surface_common.py.  There is no reference counterpart (the reference raises for 2D input): the oracle is the formula
of ``include/k2b.h``, the gates are ``fit_gradient_common``'s (``max(2e-5, 4 e32)`` per gradient group and frame, ``max(2e-6, 4
e32_loss)`` for the loss) and ``reproj_common.trajectory_gate`` for fitted parameters."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

from keypoints2body_amd import native
from tests import fit_gradient_common as G
from tests import helpers as H
from tests import reproj_common as R
from tests import reproj_surface_common as S

pytestmark = pytest.mark.gpu


# ---- 1-3: the stand-alone term -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.term_cases(), ids=lambda c: c.name)
def test_surface_term_image_matches_the_oracle(case):
    """The base case, an extras-only selection, frame 1 behind the camera (finite, the same gates) and the target of confidence 0
    moved by 100 px (gated against the oracle WITHOUT that target)."""
    loss, grad = S.term_device(case)
    S.term_gate(case, loss, grad)


def test_surface_term_image_frames_do_not_depend_on_the_batch():
    case = S.base()
    loss, grad = S.term_device(case)
    for f in range(3):
        l1, g1 = S.term_device(case, rows=[f])
        assert torch.equal(l1[0], loss[f]) and torch.equal(g1[0], grad[f]), f


# ---- 4: the whole loss, evaluate-only ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", (S.fit_case(S.FUSED), S.fit_case(S.TREE), S.fit_case(S.LMK_KIND, True)), ids=lambda c: c.name)
def test_fit_image_evaluate_only_matches_the_oracle_of_the_whole_loss(case):
    """Kinematic and surface targets together, every prior on: the fused kernel (24 joints with extras), the tree kernel (smplx20)
    and a landmark-bearing model built here.  ``num_iters = 1``, ``step_size = 0``: loss and gradient, parameters unmoved."""
    out, ins = S.device_call(case, R.fit_config(case))
    for k, x in zip(native.PARAM_KEYS, ins):
        assert torch.equal(out[k], x), f"{case.name}: an evaluate-only call moved {k}"
    G.gate(case, out["loss"].cpu().double().numpy(), out["grad"].cpu().double().numpy(), S.reference(case))


# ---- 5: Adam trajectories ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_loops(case, iters):
    assert case.lmk is None                                   # (reproj_common's loop reads the oracle's joints and extras)
    kw = dict(mask=case.mask, freeze=case.freeze)
    return R.oracle_adam(case, True, (iters,), **kw)[iters], R.oracle_adam(case, False, (iters,), **kw)[iters], S.oracle_eval(case, True)[1]


@pytest.mark.parametrize("case,iters", S.adam_cases(), ids=lambda c: getattr(c, "name", str(c)))
def test_fit_image_adam_matches_the_oracle_loop(case, iters):
    """12 iterations against ``torch.optim.Adam`` in float64 and float32: optimize_mask 15 and 9 on both routes, freeze_betas once."""
    ref64, ref32, g0 = _oracle_loops(case, iters)
    out, _ = S.device_call(case, S.adam_config(case, iters), want_grad=False)
    params = S.packed_row(out).cpu().double().numpy()
    R.trajectory_gate(f"{case.name} after {iters}", params, ref64[0], ref32[0], g0)
    start = np.concatenate([case.go, case.pose, case.shape, case.tr], axis=1).astype(np.float64)
    excluded = G.excluded_columns(case)
    assert np.array_equal(params[:, excluded], start[:, excluded]), "a group outside the optimiser moved"
    if case.freeze:
        assert not np.array_equal(params[:, ~excluded], start[:, ~excluded])
    loss = out["loss"].cpu().double().numpy()
    rel = np.abs(loss - ref64[1]) / np.abs(ref64[1])
    print(f"loss before step {iters}: device off by {rel.max():.2e}")
    assert np.isfinite(loss).all()


# ---- 6: kinematic targets only = k2b_fit_world under projection ----------------------------------------------------------------
@pytest.mark.parametrize("kind", R.BOTH)
def test_kinematic_targets_only_equal_fit_world_bit_for_bit(kind):
    case = R.base(kind, B=3, seed=23)
    for cfg in (R.fit_config(case), S.adam_config(case, 7)):
        a, _ = R.device_call(case, cfg, want_grad=True)
        b, _ = S.device_call(dataclasses.replace(case), cfg, want_grad=True)
        for k in a:
            assert torch.equal(a[k], b[k]), (kind, k)


# ---- 7: batch independence -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", (S.fit_case(S.FUSED), S.fit_case(S.LMK_KIND, True)), ids=lambda c: c.name)
def test_a_frame_fitted_alone_equals_the_frame_inside_the_batch(case):
    cfg = S.adam_config(case, 6)
    whole, _ = S.device_call(case, cfg)
    for f in range(case.frames):
        alone, _ = S.device_call(case, cfg, rows=[f])
        for k in whole:
            assert torch.equal(alone[k][0], whole[k][f]), (f, k)


# ---- 8: isolation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ("nan_target", "inf_transl"))
@pytest.mark.parametrize("case", (S.fit_case(S.FUSED), S.fit_case(S.TREE)), ids=lambda c: c.name)
def test_a_non_finite_frame_stays_in_its_own_frame(case, what):
    """An input test (non-finite VALUES, no fault): a NaN coordinate of a surface target, or an Inf translation, in frame 1."""
    K = len([i for i in case.idx if i < G.layout(case.kind).J])

    def edit(name, a):
        if what == "nan_target" and name == "j3d":
            a[1, K, 0] = np.nan                               # (the first surface target; its confidence is not 0)
        if what == "inf_transl" and name == "tr":
            a[1, 0] = np.inf                                  # (x: an infinite depth alone projects to a finite pixel)
        return a
    assert case.conf[1, K] != 0.0
    for cfg in (R.fit_config(case), S.adam_config(case, 4)):
        clean, _ = S.device_call(case, cfg)
        dirty, _ = S.device_call(case, cfg, edit=edit)
        for k in clean:
            for f in (0, 2):
                assert torch.equal(clean[k][f], dirty[k][f]), (what, k, f)
        assert not torch.isfinite(dirty["loss"][1]), what
        assert not torch.isfinite(dirty["grad"][1]).all(), what


def test_surface_term_image_keeps_a_non_finite_frame_to_itself():
    term = S.base()
    for arr, at in (("targets", (1, 0, 0)), ("tr", (1, 0))):
        bad = {"targets": term.targets.copy(), "tr": term.params[3].copy()}
        bad[arr][at] = np.nan if arr == "targets" else np.inf
        assert term.conf[1, 0] != 0.0
        dirty = dataclasses.replace(term, targets=bad["targets"], params=term.params[:3] + (bad["tr"],))
        l0, g0 = S.term_device(term)
        l1, g1 = S.term_device(dirty)
        for f in (0, 2):
            assert torch.equal(l0[f], l1[f]) and torch.equal(g0[f], g1[f]), (arr, f)
        assert not torch.isfinite(l1[1]) and not torch.isfinite(g1[1]).all(), arr


# ---- 9: refusals ---------------------------------------------------------------------------------------------------------------
SENTINEL = 7.25


class _Outputs:
    """Every float tensor ``torch.empty`` hands out while active is filled with SENTINEL and remembered: the wrappers of
    keypoints2body_amd.native allocate a call's outputs that way, so a refused call must leave them all at SENTINEL."""

    def __init__(self, monkeypatch):
        self.made, real = [], torch.empty

        def empty(*a, **k):
            t = real(*a, **k)
            if t.is_floating_point():
                t.fill_(SENTINEL)
                self.made.append(t)
            return t
        monkeypatch.setattr(torch, "empty", empty)

    def untouched(self):
        torch.cuda.synchronize()
        return len(self.made) > 0 and all(bool((t == SENTINEL).all()) for t in self.made)


def _refused(monkeypatch, exc, match, call, entry):
    outs = _Outputs(monkeypatch)
    with pytest.raises(exc, match=match):
        call()
    assert outs.untouched(), "a refused call wrote to its outputs"
    monkeypatch.undo()
    assert entry in native.load_library().k2b_last_error().decode()


def test_fit_image_refusals_come_before_any_launch(monkeypatch):
    case = S.fit_case(S.FUSED)
    call = lambda c, cfg: (lambda: S.device_call(c, cfg))
    cfg = R.fit_config(case)
    cfg.projection = 0
    _refused(monkeypatch, ValueError, "projection=0 must be 1", call(case, cfg), "k2b_fit_image")
    for focal in ((0.0, 500.0), (500.0, -1.0), (float("nan"), 500.0), (500.0, float("inf"))):
        cfg = R.fit_config(case)
        cfg.focal[0], cfg.focal[1] = focal
        _refused(monkeypatch, ValueError, "finite and positive", call(case, cfg), "k2b_fit_image")
    J = G.layout(case.kind).J
    surf = [k for k, i in enumerate(case.idx) if i >= J]
    only = dataclasses.replace(case, idx=tuple(case.idx[k] for k in surf), j3d=np.ascontiguousarray(case.j3d[:, surf]),
                               conf=np.ascontiguousarray(case.conf[:, surf]))
    _refused(monkeypatch, NotImplementedError, "at least one kinematic joint", call(only, R.fit_config(only)), "k2b_fit_image")
    # more surface targets than the kernel takes (kSurfMaxTargets = 128): a model with 72 extras + 64 landmarks
    from keypoints2body_amd import synthetic
    cx = G.consts(S.TREE)
    big = native.NativeModel(cx.v_template, cx.shapedirs, cx.posedirs, cx.J_regressor, cx.lbs_weights, cx.parents, cx.extra_vertex_ids,
                             landmarks=synthetic.make_landmarks(cx.v_template.shape[0], 55, 64, seed=1))
    limit = 128
    tree = S.fit_case(S.TREE)
    many = dataclasses.replace(tree, idx=(0,) + tuple(range(55, 55 + limit + 1)), j3d=np.zeros((3, limit + 2, 3), np.float32), conf=None)
    monkeypatch.setattr(S, "native_model", lambda _case: big)
    _refused(monkeypatch, NotImplementedError, f"at most {limit}", call(many, R.fit_config(many)), "k2b_fit_image")
    # the fp64 scan twin
    monkeypatch.setenv("K2B_FIT_SCAN64", "1")
    c = G.consts(case.kind)
    twin = native.NativeModel(c.v_template, c.shapedirs, c.posedirs, c.J_regressor, c.lbs_weights, c.parents, c.extra_vertex_ids)
    monkeypatch.delenv("K2B_FIT_SCAN64")
    monkeypatch.setattr(S, "native_model", lambda _case: twin)
    _refused(monkeypatch, NotImplementedError, "fp32 scans", call(case, R.fit_config(case)), "k2b_fit_image")


def test_surface_term_image_refusals(monkeypatch):
    case = S.base()
    for focal in ((0.0, 430.0), (500.0, float("nan"))):
        _refused(monkeypatch, ValueError, "finite and positive", lambda: S.term_device(dataclasses.replace(case, focal=focal)),
                 "k2b_surface_term_image")
    kin = dataclasses.replace(case, rows=(3,) + case.rows[1:])
    _refused(monkeypatch, ValueError, "outside", lambda: S.term_device(kin), "k2b_surface_term_image")


def test_the_old_entries_refuse_what_they_refused():
    """``k2b_fit_world`` under projection keeps refusing a surface target; the 3D surface term is what it was (bit-equal with or
    without the projected form having run on the same selection and model)."""
    case = S.fit_case(S.TREE)
    with pytest.raises(NotImplementedError, match="surface targets"):
        S.device_call(case, R.fit_config(case), entry="fit_world")
    term = S.base()
    from tests import lbs_layouts_common as L
    model = L.native_model(term.J, term.NB, S.V, "landmarks")
    args = (model, list(term.rows), H.cuda(term.targets), H.cuda(term.conf), 100.0, 600.0, *(H.cuda(a) for a in term.params))
    before = native.surface_term(*args)
    S.term_device(term)
    after = native.surface_term(*args)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
