"""GPU: the 2D entry points with hand, face and foot keypoints - ``optimize_params_frame_2d`` / ``optimize_params_sequence_2d`` /
``optimize_params_sequences_2d`` with a dict of blocks or surface indices among ``target_model_indices``, and
``ImageSpaceFitter``'s lockstep chain.  No reference counterpart (the reference raises for 2D input): the chains are held to the
float64 oracle chain of tests/reproj_surface_common.py (``reproj_chain_common``'s, over the model's output joints) with
``reproj_common.trajectory_gate``."""
import functools

import numpy as np
import pytest
import torch

import keypoints2body_amd as k2b
from keypoints2body_amd import native, synthetic
from keypoints2body_amd.core.config import FrameOptimizeConfig, SequenceOptimizeConfig
from keypoints2body_amd.core.fitters import image_space
from keypoints2body_amd.core.fitters.image_space import ImageSpaceFitter
from tests import fit_gradient_common as G
from tests import helpers as H
from tests import reproj_chain_common as RC
from tests import reproj_common as R
from tests import reproj_surface_common as S

pytestmark = pytest.mark.gpu

FOCAL, PP = 500.0, (320.5, 240.25)
NOISE = 2.0                                     # px
FIRST, FOLLOW = 12, 5
KEYS = ("global_orient", "body_pose", "betas", "transl")
T = 3


# ---- a frame with all four blocks on the 55-joint landmark model ---------------------------------------------------------------
def _project(j):
    j = j.detach().cpu().double().numpy()
    return FOCAL * j[..., :2] / j[..., 2:3]


def test_frame_with_body_hands_and_face_blocks():
    from tests.test_gpu_landmarks import BLOCKS, body_model_lmk, packed
    model, prior = body_model_lmk(), RC.assets("smplx20")[1]
    p = synthetic.make_poses_x(1, seed=61)
    pose, shape = packed(p)
    tr = np.asarray([[0.1, -0.05, 3.0]], dtype=np.float32)
    j, _ = model.native.lbs(H.cuda(p.global_orient), H.cuda(pose), H.cuda(shape), H.cuda(tr), want_vertices=False)
    assert tuple(j.shape) == (1, 127, 3)
    uv = _project(j)[0] + NOISE * synthetic.normalish(95, (127, 2), 61)
    blocks = {name: uv[lo:hi] + np.asarray(PP) for name, lo, hi in BLOCKS}
    assert [v.shape[0] for v in blocks.values()] == [22, 21, 21, 51]
    idx = [i for _, lo, hi in BLOCKS for i in range(lo, hi)]
    off = lambda n, a, s: (a + s * synthetic.normalish(n, a.shape, 61)).astype(np.float32)
    start = RC.init_params("smplx20", model, off(90, p.global_orient, 0.1), off(91, pose, 0.1), off(92, shape, 0.3))
    cfg = FrameOptimizeConfig(use_lbfgs=False, num_iters=10)
    kw = dict(focal=FOCAL, principal_point=PP, body_model="smplx", model=model, pose_prior=prior, config=cfg, init_params=start)
    res = k2b.optimize_params_frame_2d(blocks, **kw)
    assert tuple(res.joints.shape) == (1, 127, 3) and torch.isfinite(res.joints).all() and torch.isfinite(res.loss)
    assert all(torch.isfinite(getattr(res.params, f)).all() for f in KEYS + ("expression", "jaw_pose", "left_hand_pose", "right_hand_pose"))

    # the same fit through ImageSpaceFitter.fit_batch, and its start
    fitter = ImageSpaceFitter(model, step_size=cfg.step_size, num_iters=10, joints_category="GENERIC", pose_prior=prior)
    all_uv = np.concatenate(list(blocks.values()), axis=0)
    out, joints, _, loss = fitter.fit_batch(start, all_uv[None], FOCAL, PP, np.ones(len(idx), np.float32), target_model_indices=idx)
    ref = fitter.result_params(out, start)
    for f in KEYS + ("expression", "jaw_pose", "left_hand_pose", "right_hand_pose"):
        assert torch.equal(getattr(res.params, f), getattr(ref, f)), f
    assert torch.equal(res.joints, joints) and torch.equal(res.loss, loss.sum())

    # arrays + target_model_indices: the same bits
    arr = k2b.optimize_params_frame_2d(all_uv, target_model_indices=idx, **kw)
    for f in KEYS + ("expression", "jaw_pose"):
        assert torch.equal(getattr(arr.params, f), getattr(res.params, f)), f

    # hands and face end nearer their detections than they start
    go0, bp0, be0 = fitter._start_rows(start)
    surf = [k for k, i in enumerate(idx) if i >= 22]
    cols = torch.as_tensor(idx, device="cuda")[surf]
    centred = all_uv[surf] - np.asarray(PP)
    err = lambda go, bp, be, t: float(np.linalg.norm(
        _project(model.native.lbs(go, bp, be, t, want_vertices=False)[0].index_select(1, cols))[0] - centred, axis=-1).mean())
    begin = err(go0, bp0, be0, fitter.last_init_cam_t)
    end = err(out["global_orient"], out["body_pose"], out["betas"], out["transl"])
    print(f"mean pixel error of the hand and face blocks: {begin:.2f} -> {end:.2f}")
    assert end < begin


# ---- videos on the small landmark-bearing SMPL-X model -----------------------------------------------------------------------
KIND = S.LMK_KIND


@functools.lru_cache(maxsize=None)
def _lmk_assets():
    from keypoints2body_amd.models.body_model import BodyModel
    c = G.consts(KIND)
    model = BodyModel(c.v_template, c.shapedirs, c.posedirs, c.J_regressor, c.lbs_weights, c.parents, c.extra_vertex_ids,
                      model_type="smplx", num_betas=10, landmarks=S.lmk_table())
    return model, RC.assets(KIND)[1]


@functools.lru_cache(maxsize=None)
def _video(surface: bool):
    """Body 22 and, with `surface`, the surface targets of ``surface_rows`` (four vertex-selected joints, every fifth landmark):
    a drifting body 3 m away, detections = its float64 projection + 2 px of noise; the start 0.1 rad / 0.3 off frame 0."""
    lmk = S.lmk_table()
    idx = list(range(22)) + (list(S.surface_rows(KIND, lmk)) if surface else [])
    b = R.base(KIND, B=1, seed=61)
    step = lambda stream, a, scale: scale * synthetic.normalish(stream, a.shape, 61)
    go = np.concatenate([b.go + t * step(93, b.go, 0.03) for t in range(T)]).astype(np.float64)
    pose = np.concatenate([b.pose + t * step(94, b.pose, 0.05) for t in range(T)]).astype(np.float64)
    rep = lambda a: torch.tensor(np.repeat(a, T, axis=0), dtype=torch.float64)
    with torch.no_grad():
        x = S.outputs(KIND, lmk, True, torch.tensor(go), torch.tensor(pose), rep(b.shape), rep(b.tr))[:, idx].numpy()
    uv = FOCAL * x[..., :2] / x[..., 2:3] + NOISE * synthetic.normalish(95, (T, len(idx), 2), 61)
    start = tuple((a + s * synthetic.normalish(n, a.shape, 61)).astype(np.float32) for n, a, s in ((90, b.go, 0.1), (91, b.pose, 0.1), (92, b.shape, 0.3)))
    return uv + np.asarray(PP), idx, start


def _kw(surface, freeze=True):
    model, prior = _lmk_assets()
    _, idx, start = _video(surface)
    cfg = SequenceOptimizeConfig(frame=FrameOptimizeConfig(use_lbfgs=False, num_iters=FIRST, num_iters_followup=FOLLOW, freeze_betas=freeze))
    return dict(focal=FOCAL, principal_point=PP, body_model="smplx", model=model, config=cfg, target_model_indices=idx,
                init_params=RC.init_params(KIND, model, *start), pose_prior=prior)


class _Stage1:
    """Records what ``ImageSpaceFitter._fit`` returns: the first call of a fit is stage 1, whose result starts the chain."""

    def __init__(self, monkeypatch):
        self.results, real = [], ImageSpaceFitter._fit

        def fit(fitter, *a, **k):
            out = real(fitter, *a, **k)
            self.results.append({key: v.clone() for key, v in out.items()})
            return out
        monkeypatch.setattr(ImageSpaceFitter, "_fit", fit)

    def start(self):
        return [self.results[0][k].cpu().numpy() for k in KEYS]


def _weights(fitter, freeze):
    assert FrameOptimizeConfig().pose_preserve_weight == RC.PRESERVE
    cfg = fitter.stage_configs((FOCAL, FOCAL), 0, 100.0, 1.0, RC.PRESERVE, freeze)[1]
    return dict(sigma=cfg.sigma, joint=cfg.joint_loss_weight, mixture=cfg.pose_prior_weight, bending=cfg.angle_prior_weight,
                shape=cfg.shape_prior_weight, preserve=RC.PRESERVE, transl=0.0)


def _gate_chain(what, packed, pixels, idx, start, freeze, frames):
    model, prior = _lmk_assets()
    fitter = ImageSpaceFitter(model, step_size=1e-2, num_iters=FIRST, joints_category="GENERIC", pose_prior=prior, num_iters_followup=FOLLOW)
    targets = image_space.centred_keypoints(pixels, PP)
    args = (KIND, S.lmk_table(), idx, targets, start, _weights(fitter, freeze), (FOCAL, FOCAL), FIRST, FOLLOW, freeze)
    d64, d32 = S.oracle_chain(*args, True), S.oracle_chain(*args, False)
    for t in frames:
        R.trajectory_gate(f"{what} frame {t}", packed[t:t + 1], d64[t][0], d32[t][0], d64[t][2])


def _packed(results):
    model = _lmk_assets()[0]
    rows = []
    for r in results:
        p = r.params
        pose = model.pack_pose(1, body_pose=p.body_pose, jaw_pose=p.jaw_pose, leye_pose=p.leye_pose, reye_pose=p.reye_pose,
                               left_hand_pose=p.left_hand_pose, right_hand_pose=p.right_hand_pose)
        rows.append(torch.cat([p.global_orient, pose, model.pack_shape(1, p.betas, p.expression), p.transl], dim=1))
    return torch.cat(rows).cpu().double().numpy()


@pytest.mark.parametrize("freeze", (True, False))
def test_a_short_video_with_surface_targets(monkeypatch, freeze):
    pixels, idx, _ = _video(True)
    kw = _kw(True, freeze)
    spy = _Stage1(monkeypatch)
    res = k2b.optimize_params_sequence_2d(pixels, **kw)
    start = spy.start()
    monkeypatch.undo()
    assert len(res) == T and all(torch.isfinite(r.joints).all() and torch.isfinite(r.loss) for r in res)
    one = k2b.optimize_params_frame_2d(pixels[0], **dict(kw, config=kw["config"].frame))
    for f in KEYS + ("expression", "jaw_pose", "left_hand_pose"):
        assert torch.equal(getattr(res[0].params, f), getattr(one.params, f)), f
    _gate_chain(f"video{'/frozen' if freeze else ''}", _packed(res), pixels, idx, start, freeze, (0, 1, 2))
    held = all(torch.equal(r.params.betas, res[0].params.betas) for r in res[1:])
    assert held == freeze
    assert not torch.equal(res[1].params.expression, res[0].params.expression)


def test_many_videos_with_surface_targets_equal_the_single_calls():
    pixels, _, _ = _video(True)
    kw = _kw(True)
    videos = [pixels, pixels[2:3], pixels[:0]]
    batch = k2b.optimize_params_sequences_2d(videos, **dict(kw, init_params=[kw["init_params"]] * 3))
    assert isinstance(batch, k2b.SequenceBatch) and list(batch.lengths) == [3, 1, 0] and batch.num_frames == 4
    assert len(batch.results(2)) == 0
    for s, v in enumerate(videos[:2]):
        single = k2b.optimize_params_sequence_2d(v, **kw)
        got = batch.results(s)
        assert len(got) == len(single) == len(v)
        for a, b in zip(got, single):
            for f in KEYS + ("expression", "left_hand_pose"):
                assert torch.equal(getattr(a.params, f), getattr(b.params, f)), (s, f)
            assert torch.equal(a.joints, b.joints) and torch.equal(a.loss, b.loss)


def test_a_dict_video_equals_the_arrays_with_indices():
    """Body and both hand blocks on SMPL-X (the hands' fingertips are vertex-selected joints): the dict and the arrays with the
    blocks' indices give the same bits."""
    model, prior = _lmk_assets()
    rng = np.random.default_rng(3)
    pixels, _, start = _video(False)
    blocks = {"body": pixels, "left_hand": pixels[:, :21] + rng.normal(size=(T, 21, 2)), "right_hand": pixels[:, 1:22] + rng.normal(size=(T, 21, 2))}
    idx = list(range(22)) + list(range(25, 67))
    kw = dict(_kw(False), target_model_indices=None)
    a = k2b.optimize_params_sequence_2d(blocks, **kw)
    b = k2b.optimize_params_sequence_2d(np.concatenate(list(blocks.values()), axis=1), **dict(kw, target_model_indices=idx))
    for x, y in zip(a, b):
        for f in KEYS + ("expression", "left_hand_pose"):
            assert torch.equal(getattr(x.params, f), getattr(y.params, f)), f
        assert torch.isfinite(x.joints).all()


def test_the_lockstep_route_on_kinematic_targets_agrees_with_the_one_launch_chain(monkeypatch):
    """3 frames at 12 / 5 iterations: both routes against the same oracle chain (no bit equality is asked: the one-launch chain
    keeps its state in registers across frames, the lockstep route goes through memory and separate launches)."""
    pixels, idx, start = _video(False)
    model, prior = _lmk_assets()
    fitter = ImageSpaceFitter(model, step_size=1e-2, num_iters=FIRST, joints_category="GENERIC", pose_prior=prior, num_iters_followup=FOLLOW)
    init = RC.init_params(KIND, model, *start)
    spy = _Stage1(monkeypatch)
    one, _, _, _ = fitter.fit_sequences(init, pixels, [T], FOCAL, PP, target_model_indices=idx, run_forward=False)
    s1 = spy.start()
    assert len(spy.results) == 1
    lock, _, _, loss = fitter.fit_sequences(init, pixels, [T], FOCAL, PP, target_model_indices=idx, run_forward=False, _one_launch=False)
    assert len(spy.results) == 2 + T                           # stage 1 again, then one call per frame index
    monkeypatch.undo()
    for k in KEYS:
        assert torch.equal(spy.results[1][k], spy.results[0][k]), k
    assert torch.isfinite(loss).all()
    for name, out in (("one launch", one), ("lockstep", lock)):
        _gate_chain(name, S.packed_row(out).cpu().double().numpy(), pixels, idx, s1, True, (0, 1, 2))
    print(f"lockstep vs one launch: max difference {float((S.packed_row(lock) - S.packed_row(one)).abs().max()):.2e}")
