"""The Adam loop of ``k2b_fit_multiview``: trajectories against the float64 oracle loop (``torch.optim.Adam`` over
tests/multiview_common.py's loss, the same hyper-parameters; gate ``reproj_common.trajectory_gate``), the launch shapes bit for
bit, a frame alone and inside a batch, the call's independence of what its handles served before, and the refusals that need a
model."""
import functools

import numpy as np
import pytest
import torch

from keypoints2body_amd import native
from tests import call_history_common as CH
from tests import fit_gradient_common as G
from tests import helpers as H
from tests import multiview_common as MV
from tests import reproj_common as R

pytestmark = pytest.mark.gpu

CHECKPOINTS = (1, 10, 30)


@functools.lru_cache(maxsize=None)
def _oracle_loops(kind, C):
    case = MV.trajectory_case(kind, C)
    return MV.oracle_adam(case, True, CHECKPOINTS), MV.oracle_adam(case, False, CHECKPOINTS), MV.oracle_eval(case, True)[1]


@pytest.mark.parametrize("iters", CHECKPOINTS)
@pytest.mark.parametrize("C", (2, 4))
@pytest.mark.parametrize("kind", MV.BOTH)
def test_adam_trajectory_matches_the_oracle_loop(kind, C, iters):
    case = MV.trajectory_case(kind, C)
    ref64, ref32, g0 = _oracle_loops(kind, C)
    params, loss = MV.device_adam(case, iters)
    R.trajectory_gate(f"{case.name} after {iters}", params.astype(np.float64), ref64[iters][0], ref32[iters][0], g0)
    start = np.concatenate([case.go, case.pose, case.shape, case.tr], axis=1).astype(np.float64)
    assert np.array_equal(params.astype(np.float64)[g0 == 0.0], start[g0 == 0.0])
    rel = np.abs(loss - ref64[iters][1]) / np.abs(ref64[iters][1])
    print(f"loss before step {iters}: device off by {rel.max():.2e}")
    assert np.isfinite(loss).all()


@pytest.mark.parametrize("frames", (5, 17))
@pytest.mark.parametrize("kind", MV.BOTH)
def test_launch_shapes_agree_bit_for_bit_over_a_fit(kind, frames):
    """Fused kernel: split, split-paired, paired, wide; 5 and 17 frames leave the paired shapes a half-empty wavefront.  Tree kernel:
    plain and component waves."""
    case = MV.base(kind, 3, B=frames, seed=13)
    shapes = R.shapes_of(kind)
    first = MV.device_adam(case, 10, shapes[0])
    for s in shapes[1:]:
        params, loss = MV.device_adam(case, 10, s)
        assert np.array_equal(params, first[0]) and np.array_equal(loss, first[1]), f"{case.name}: shape {s} differs from shape {shapes[0]}"
    auto = MV.device_adam(case, 10, 0)
    assert np.array_equal(auto[0], first[0]) and np.array_equal(auto[1], first[1])
    assert np.isfinite(first[0]).all()


@pytest.mark.parametrize("kind", MV.BOTH)
def test_a_frame_alone_equals_its_row_in_a_batch(kind):
    case = MV.base(kind, 3, B=17, seed=13)
    params, loss = MV.device_adam(case, 10)
    for row in (0, 6, 16):
        p1, l1 = MV.device_adam(case, 10, rows=[row])
        assert np.array_equal(p1[0], params[row]) and l1[0] == loss[row], (case.name, row)


def _fit(case, handles, rows=None, j3d=None, iters=10):
    model, prior = handles
    cfg = MV.fit_config(case)
    cfg.num_iters, cfg.step_size = iters, R.ADAM["lr"]
    return MV.device_call(case, cfg, want_grad=True, rows=rows, model=model, prior=prior, j3d=j3d)[0]


@pytest.mark.parametrize("kind", MV.BOTH)
def test_the_call_does_not_depend_on_the_calls_before_it(kind):
    """The same 3-frame call after a larger batch, after a refused call and after a batch of NaN keypoints, and on a second set of
    fresh handles: the bits of the first call on fresh handles."""
    big = MV.base(kind, 3, B=17, seed=13)
    rows = [4, 5, 6]

    def refused(handles):
        cfg = MV.fit_config(big)
        cfg.projection = 0
        with pytest.raises(ValueError, match="projection=0"):
            MV.device_call(big, cfg, rows=rows, model=handles[0], prior=handles[1])

    CH.run_protocol(lambda: (CH.fresh_model(kind), CH.fresh_prior()), lambda h: _fit(big, h, rows=rows),
                    [("larger batch", lambda h: _fit(big, h), None),
                     ("non-finite batch", lambda h: _fit(big, h, j3d=np.full_like(big.j3d, np.nan)), CH.all_rows_nonfinite("loss", big.name))],
                    f"k2b_fit_multiview {big.name}", between=refused)


# ---- refusals that need a model ------------------------------------------------------------------------------------------------
SENTINEL = 7.25


def _refused(monkeypatch, exc, match, call):
    """A refused call leaves every output tensor as ``torch.empty`` handed it out (filled with SENTINEL here)."""
    made, real = [], torch.empty

    def empty(*a, **k):
        t = real(*a, **k)
        if t.is_floating_point():
            t.fill_(SENTINEL)
            made.append(t)
        return t
    monkeypatch.setattr(torch, "empty", empty)
    with pytest.raises(exc, match=match):
        call()
    torch.cuda.synchronize()
    assert made and all(bool((t == SENTINEL).all()) for t in made), "a refused call wrote to its outputs"
    monkeypatch.undo()


def test_surface_targets_are_refused(monkeypatch):
    kind = "smplx20"
    case = MV.base(kind, 2, B=3)
    model, J = G.native_model(kind), G.layout(kind).J
    assert model.num_extra > 0
    bad = MV.replace(case, idx=tuple(case.idx[:8]) + (J,), j3d=np.ascontiguousarray(case.j3d[:, :, :9]))
    _refused(monkeypatch, NotImplementedError, "surface targets", lambda: MV.device_call(bad, MV.fit_config(bad)))
    assert "k2b_fit_multiview" in native.load_library().k2b_last_error().decode()


def test_the_fp64_scan_twin_is_refused(monkeypatch):
    case = MV.base("smpl10", 2, B=3)
    monkeypatch.setenv("K2B_FIT_SCAN64", "1")
    c = G.consts("smpl10")
    model = native.NativeModel(c.v_template, c.shapedirs, c.posedirs, c.J_regressor, c.lbs_weights, c.parents, c.extra_vertex_ids)
    monkeypatch.delenv("K2B_FIT_SCAN64")
    _refused(monkeypatch, NotImplementedError, "fp32 scans", lambda: MV.device_call(case, MV.fit_config(case), model=model))


def test_the_tree_kernel_refuses_a_translation_prior_as_ever(monkeypatch):
    case = MV.base("smplx20", 2, B=3)
    cfg = MV.fit_config(case)
    cfg.transl_prior_weight = 10.0
    _refused(monkeypatch, NotImplementedError, "translation prior", lambda: MV.device_call(case, cfg))


@pytest.mark.parametrize("kind", MV.BOTH)
def test_bad_views_are_invalid_arguments_with_real_handles(kind, monkeypatch):
    case = MV.base(kind, 2, B=3)
    cams = list(case.cams)
    nan_cam = (cams[1][0].copy(), cams[1][1].copy(), cams[1][2])
    nan_cam[0][1, 1] = np.nan
    _refused(monkeypatch, ValueError, r"cameras\[1\].rotation\[4\]", lambda: MV.device_call(MV.replace(case, cams=(cams[0], nan_cam)), MV.fit_config(case)))
    cfg = MV.fit_config(case)
    cfg.projection = 0
    _refused(monkeypatch, ValueError, "projection=0", lambda: MV.device_call(case, cfg))
