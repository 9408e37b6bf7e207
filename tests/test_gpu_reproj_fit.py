"""The Adam loop of ``k2b_fit_world`` under the projected joint term: trajectories against the float64 oracle loop
(``torch.optim.Adam`` over tests/reproj_common.py's loss, the same hyper-parameters), the launch shapes bit for bit, the 3D term
untouched by the new fields, and every refusal of the host layer.  Gate per parameter: ``max(1e-4, 4 x the float32 oracle
loop's deviation from the float64 one)``; 1e-4 is the project's parameter gate (tests/test_gpu_parity.py)."""
import functools

import numpy as np
import pytest
import torch

from keypoints2body_amd import native
from tests import fit_gradient_common as G
from tests import helpers as H
from tests import reproj_common as R

pytestmark = pytest.mark.gpu

CHECKPOINTS = (1, 2, 10, 50)
TRAJECTORY_FRAMES = {"smpl10": 17, "smplx20": 5}


@functools.lru_cache(maxsize=None)
def _trajectory_case(kind):
    b = R.base(kind, B=TRAJECTORY_FRAMES[kind], seed=11 if kind == "smpl10" else 47)
    return R.replace(b, name=b.name + "/adam")


@functools.lru_cache(maxsize=None)
def _oracle_loops(kind):
    case = _trajectory_case(kind)
    return R.oracle_adam(case, True, CHECKPOINTS), R.oracle_adam(case, False, CHECKPOINTS), R.oracle_eval(case, True)[1]


@pytest.mark.parametrize("iters", CHECKPOINTS)
@pytest.mark.parametrize("kind", tuple(TRAJECTORY_FRAMES))
def test_adam_trajectory_matches_the_oracle_loop(kind, iters):
    case = _trajectory_case(kind)
    ref64, ref32, g0 = _oracle_loops(kind)
    params, loss = R.device_adam(case, iters)
    R.trajectory_gate(f"{case.name} after {iters}", params, ref64[iters][0], ref32[iters][0], g0)
    # (entries whose gradient is identically zero - the rotation of a leaf joint outside the prior moves no joint - never move)
    start = np.concatenate([case.go, case.pose, case.shape, case.tr], axis=1)[:len(params)].astype(np.float64)
    assert np.array_equal(params[g0 == 0.0], start[g0 == 0.0])
    rel = np.abs(loss - ref64[iters][1]) / np.abs(ref64[iters][1])
    rel32 = np.abs(ref32[iters][1] - ref64[iters][1]) / np.abs(ref64[iters][1])
    print(f"loss before step {iters}: device off by {rel.max():.2e}, float32 oracle loop by {rel32.max():.2e}")
    assert np.isfinite(loss).all()


@pytest.mark.parametrize("frames", (3, 17))
@pytest.mark.parametrize("kind", R.BOTH)
def test_launch_shapes_agree_bit_for_bit_over_a_fit(kind, frames):
    case = R.term_case(kind, "all")
    shapes = R.shapes_of(kind)
    first = R.device_adam(case, 10, shapes[0], frames)
    for s in shapes[1:]:
        params, loss = R.device_adam(case, 10, s, frames)
        assert np.array_equal(params, first[0]) and np.array_equal(loss, first[1]), f"{case.name}: shape {s} differs from shape {shapes[0]} at {frames} frames"
    auto = R.device_adam(case, 10, 0, frames)
    assert np.array_equal(auto[0], first[0]) and np.array_equal(auto[1], first[1])


@pytest.mark.parametrize("kind", R.BOTH)
def test_the_3d_term_does_not_read_the_focal_lengths(kind):
    """``projection = 0`` with arbitrary ``focal`` values: bit-equal to ``focal = 0``, gradient and fit."""
    case = G.term_case(kind, "all")
    rows = lambda a: None if a is None else H.cuda(a)
    ins = [rows(a) for a in (case.go, case.pose, case.shape, case.tr)]
    results = []
    for focal in ((0.0, 0.0), (123.5, float("nan"))):
        for iters, step in ((1, 0.0), (5, 1e-2)):
            cfg = G.fit_config(case)
            cfg.num_iters, cfg.step_size = iters, step
            assert cfg.projection == 0
            cfg.focal[0], cfg.focal[1] = focal
            results.append(native.fit_world(G.native_model(kind), H.native_prior(), cfg, list(case.idx), rows(case.j3d), None, *ins,
                                            preserve_pose=rows(case.preserve), want_grad=True, transl_prior_target=rows(case.tr_target)))
    for a, b in ((results[0], results[2]), (results[1], results[3])):
        for k in a:
            assert torch.equal(a[k], b[k]), k


# ---- refusals ----------------------------------------------------------------------------------------------------------------
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


def _refused(monkeypatch, exc, match, call):
    outs = _Outputs(monkeypatch)
    with pytest.raises(exc, match=match):
        call()
    assert outs.untouched(), "a refused call wrote to its outputs"
    monkeypatch.undo()


def _world_args(case, n=3):
    take = lambda a: H.cuda(a[:n])
    return [list(case.idx), take(case.j3d), None] + [take(a) for a in (case.go, case.pose, case.shape, case.tr)]


@pytest.mark.parametrize("kind", R.BOTH)
def test_bad_projection_fields_are_invalid_arguments(kind, monkeypatch):
    case = R.term_case(kind, "joint")
    model, prior, args = G.native_model(kind), H.native_prior(), _world_args(R.term_case(kind, "joint"))
    for projection, focal, match in ((2, (500.0, 500.0), "projection=2"), (-1, (500.0, 500.0), "projection=-1"), (1, (0.0, 500.0), r"focal\[0\]"),
                                     (1, (500.0, -3.0), r"focal\[1\]"), (1, (float("inf"), 500.0), r"focal\[0\]"),
                                     (1, (500.0, float("nan")), r"focal\[1\]")):
        cfg = R.fit_config(case)
        cfg.projection = projection
        cfg.focal[0], cfg.focal[1] = focal
        _refused(monkeypatch, ValueError, match, lambda: native.fit_world(model, prior, cfg, *args, want_grad=True))


def test_surface_targets_are_refused_under_projection(monkeypatch):
    kind = "smplx20"
    model, case = G.native_model(kind), R.term_case(kind, "joint")
    J = G.layout(kind).J
    assert model.num_extra > 0
    idx, j3d = list(case.idx[:8]) + [J], H.cuda(case.j3d[:3, :9])
    args = [idx, j3d, None] + [H.cuda(a[:3]) for a in (case.go, case.pose, case.shape, case.tr)]
    cfg = R.fit_config(case)
    _refused(monkeypatch, NotImplementedError, "surface targets", lambda: native.fit_world(model, H.native_prior(), cfg, *args))
    cfg.projection = 0                                        # (the same call with the 3D term is taken)
    native.fit_world(model, H.native_prior(), cfg, *args)


def test_the_fp64_scan_twin_is_refused_under_projection(monkeypatch):
    case = R.term_case("smpl10", "joint")
    monkeypatch.setenv("K2B_FIT_SCAN64", "1")
    c = G.consts("smpl10")
    model = native.NativeModel(c.v_template, c.shapedirs, c.posedirs, c.J_regressor, c.lbs_weights, c.parents, c.extra_vertex_ids)
    monkeypatch.delenv("K2B_FIT_SCAN64")
    cfg, args = R.fit_config(case), _world_args(case)
    _refused(monkeypatch, NotImplementedError, "fp32 scans", lambda: native.fit_world(model, H.native_prior(), cfg, *args))
    cfg.projection = 0
    native.fit_world(model, H.native_prior(), cfg, *args)


@pytest.mark.parametrize("kind", R.BOTH)
def test_every_other_fit_entry_refuses_projection(kind, monkeypatch):
    """k2b_fit_sequence (a chain of one frame included), k2b_fit_sequences, k2b_fit_world_lbfgs, k2b_fit_sequence_lbfgs,
    k2b_fit_sequences_lbfgs and k2b_shape_pass_lbfgs: K2B_ERR_UNSUPPORTED before any launch."""
    case = R.term_case(kind, "joint")
    model, prior = G.native_model(kind), H.native_prior()
    cfg = R.fit_config(case)
    cfg.transl_prior_weight = 0.0
    idx = list(case.idx)
    T = 3
    j3d = H.cuda(case.j3d[:T])
    one = [H.cuda(a[:1]) for a in (case.go, case.pose, case.shape, case.tr)]
    rows = [H.cuda(a[:T]) for a in (case.go, case.pose, case.shape, case.tr)]
    match = "projected joint term"
    calls = {
        "k2b_fit_sequence": lambda: native.fit_sequence(model, prior, cfg, 2, idx, j3d[None], None, *one),
        "k2b_fit_sequence/1": lambda: native.fit_sequence(model, prior, cfg, 2, idx, j3d[:, None], None, *rows),
        "k2b_fit_sequences": lambda: native.fit_sequences(model, prior, cfg, 2, idx, [2, 1], j3d, None, *[a[:2] for a in rows]),
        "k2b_fit_world_lbfgs": lambda: native.fit_world_lbfgs(model, prior, cfg, idx, j3d, None, *rows, max_iter=3, lr=1.0),
        "k2b_fit_sequence_lbfgs": lambda: native.fit_sequence_lbfgs(model, prior, cfg, 3, 2, idx, j3d, None, *one, lr=1.0),
        "k2b_fit_sequences_lbfgs": lambda: native.fit_sequences_lbfgs(model, prior, cfg, 3, 2, idx, [2, 1], j3d, None, *[a[:2] for a in rows], lr=1.0),
        "k2b_shape_pass_lbfgs": lambda: native.shape_pass_lbfgs(
            model, prior, cfg, torch.tensor([0, 2, 3], dtype=torch.int32, device="cuda"), idx, j3d, torch.ones((T, len(idx)), device="cuda"),
            rows[0], rows[1], j3d[:, 0].contiguous(), 0, rows[2][:2, :min(10, rows[2].shape[1])].contiguous(), max_iter=3, lr=1.0),
    }
    for name, call in calls.items():
        _refused(monkeypatch, NotImplementedError, match, call)
        assert name.split("/")[0] in native.load_library().k2b_last_error().decode()
