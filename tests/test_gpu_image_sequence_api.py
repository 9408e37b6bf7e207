"""GPU: ``optimize_params_sequence_2d`` / ``optimize_params_sequences_2d`` and ``ImageSpaceFitter.fit_sequences`` end to end on a
synthetic SMPL and a synthetic SMPL-X model: a 6-frame motion projected at f = 500 px from 3 m with 2 px of noise."""
import functools

import numpy as np
import pytest
import torch

import keypoints2body_amd as k2b
from keypoints2body_amd import native, synthetic
from keypoints2body_amd.core.config import FrameOptimizeConfig, SequenceOptimizeConfig
from keypoints2body_amd.core.fitters.image_space import ImageSpaceFitter
from tests import fit_gradient_common as G
from tests import reproj_common as R
from tests import reproj_chain_common as RC

pytestmark = pytest.mark.gpu

T, K = 6, 22
FOCAL, PP = 500.0, (320.5, 240.25)
NOISE = 2.0                                     # px
FIRST, FOLLOW = 12, 5
KINDS = ("smpl10", "smplx20")
KEYS = ("global_orient", "body_pose", "betas", "transl")


@functools.lru_cache(maxsize=None)
def _motion(kind):
    """A body 3 m in front of the camera whose pose drifts 0.05 rad per frame (the root 0.03); detections = its projection + 2 px
    of seeded noise, in pixels with the principal point added; the start is the first frame's pose 0.1 rad / 0.3 off."""
    b = R.base(kind, B=1, seed=61)
    step = lambda stream, a, scale: scale * synthetic.normalish(stream, a.shape, 61)
    go = np.concatenate([b.go + t * step(93, b.go, 0.03) for t in range(T)]).astype(np.float32)
    pose = np.concatenate([b.pose + t * step(94, b.pose, 0.05) for t in range(T)]).astype(np.float32)
    rep = lambda a: np.repeat(a, T, axis=0)
    uv = R.project64(kind, go, pose, rep(b.shape), rep(b.tr), (FOCAL, FOCAL))[:, :K] + NOISE * synthetic.normalish(95, (T, K, 2), 61)
    start = tuple((a + s * synthetic.normalish(n, a.shape, 61)).astype(np.float32) for n, a, s in ((90, b.go, 0.1), (91, b.pose, 0.1), (92, b.shape, 0.3)))
    return uv + np.asarray(PP), uv, start


def _kw(kind, freeze=True):
    model, prior = RC.assets(kind)
    cfg = SequenceOptimizeConfig(frame=FrameOptimizeConfig(use_lbfgs=False, num_iters=FIRST, num_iters_followup=FOLLOW, freeze_betas=freeze))
    return dict(focal=FOCAL, principal_point=PP, body_model="smplx" if kind.startswith("smplx") else "smpl", model=model, config=cfg,
                init_params=RC.init_params(kind, model, *_motion(kind)[2]), pose_prior=prior)


def _mean_pixel_error(kind, params, uv):
    """[n] mean pixel distance between the projected joints of packed float64 parameter rows and centred detections."""
    lay = G.layout(kind)
    go, pose, shape, tr = (params[:, a:b] for a, b in ((0, 3), (3, 3 + lay.D), (3 + lay.D, 3 + lay.D + lay.NB), (3 + lay.D + lay.NB, lay.P)))
    return np.linalg.norm(R.project64(kind, go, pose, shape, tr, (FOCAL, FOCAL))[:, :K] - uv, axis=-1).mean(axis=1)


def _spied(fn):
    """`fn()` with the fit launches of keypoints2body_amd.native counted by entry."""
    calls = {"fit_world": 0, "fit_image_sequences": 0}
    orig = {k: getattr(native, k) for k in calls}

    def spy(k):
        def f(*a, **kw):
            calls[k] += 1
            return orig[k](*a, **kw)
        return f
    for k in calls:
        setattr(native, k, spy(k))
    try:
        return fn(), calls
    finally:
        for k in calls:
            setattr(native, k, orig[k])


@pytest.mark.parametrize("kind", KINDS)
def test_a_video_is_one_stage_one_launch_and_one_chain_launch(kind):
    pixels, uv, start = _motion(kind)
    kw = _kw(kind)
    res, calls = _spied(lambda: k2b.optimize_params_sequence_2d(pixels, **kw))
    assert calls == {"fit_world": 1, "fit_image_sequences": 1}
    assert len(res) == T and all(isinstance(r, k2b.BodyModelFitResult) for r in res)
    assert all(tuple(r.vertices.shape) == (1, G.consts(kind).v_template.shape[0], 3) and tuple(r.params.transl.shape) == (1, 3) for r in res)
    # frame 0 is the frame entry's fit of that frame, bit for bit
    one = k2b.optimize_params_frame_2d(pixels[0], **dict(kw, config=kw["config"].frame))
    for f in ("global_orient", "body_pose", "betas", "transl") + (("expression", "jaw_pose", "left_hand_pose") if kind.startswith("smplx") else ()):
        assert torch.equal(getattr(res[0].params, f), getattr(one.params, f)), f
    assert torch.equal(res[0].joints, one.joints)
    # every frame ends nearer its detections than it starts (frame t starts from frame t - 1's result; frame 0 from stage 1's)
    model, prior = RC.assets(kind)
    fitter = ImageSpaceFitter(model, step_size=1e-2, num_iters=FIRST, joints_category="AMASS", pose_prior=prior, num_iters_followup=FOLLOW)
    out, _, _, loss = fitter.fit_sequences(kw["init_params"], pixels, [T], FOCAL, PP, np.ones((T, K), np.float32), run_forward=False)
    packed = torch.cat([out[k] for k in KEYS], dim=1).cpu().double().numpy()
    assert torch.equal(out["transl"], torch.cat([r.params.transl for r in res])) and torch.equal(out["global_orient"], torch.cat([r.params.global_orient for r in res]))
    lay = G.layout(kind)
    start0 = np.concatenate([start[0], start[1], start[2], fitter.last_init_cam_t.cpu().numpy()], axis=1).astype(np.float64)
    begins = np.concatenate([start0, packed[:-1]], axis=0)
    end, begin = _mean_pixel_error(kind, packed, uv), _mean_pixel_error(kind, begins, uv)
    print(f"{kind}: mean pixel error per frame {begin} -> {end}")
    assert (end < begin).all() and bool(torch.isfinite(loss).all())
    # the shape is the first frame's
    nb = lay.betas_prior
    assert torch.equal(out["betas"][1:, :nb], out["betas"][:1, :nb].expand(T - 1, -1))


@pytest.mark.parametrize("kind", KINDS)
def test_many_videos_equal_the_single_calls_bit_for_bit(kind):
    pixels, _, start = _motion(kind)
    model, prior = RC.assets(kind)
    kw = _kw(kind)
    conf = (0.5 + synthetic.uniform(96, T * K, 61).reshape(T, K, 1)).astype(np.float64)
    videos = [np.concatenate([pixels, conf], axis=2)[:4], pixels[5:6], pixels[2:5]]
    init = [kw["init_params"]] * 3
    batch, calls = _spied(lambda: k2b.optimize_params_sequences_2d(videos, **dict(kw, init_params=init)))
    assert calls == {"fit_world": 1, "fit_image_sequences": 1}
    assert isinstance(batch, k2b.SequenceBatch) and list(batch.lengths) == [4, 1, 3] and batch.num_frames == 8
    for s, v in enumerate(videos):
        single = k2b.optimize_params_sequence_2d(v, **kw)
        got = batch.results(s)
        assert len(got) == len(single) == len(v)
        for a, b in zip(got, single):
            for f in KEYS:
                assert torch.equal(getattr(a.params, f), getattr(b.params, f)), (s, f)
            assert torch.equal(a.joints, b.joints) and torch.equal(a.vertices, b.vertices) and torch.equal(a.loss, b.loss)
        assert torch.equal(batch.joints_of(s), torch.cat([r.joints for r in single])) and torch.equal(batch.loss_of(s), torch.stack([r.loss for r in single]))


@pytest.mark.parametrize("kind", KINDS)
def test_independent_frames_are_the_batched_frame_fit(kind):
    pixels, _, start = _motion(kind)
    model, prior = RC.assets(kind)
    kw = _kw(kind)
    cfg = SequenceOptimizeConfig(frame=kw["config"].frame, use_previous_frame_init=False)
    res, calls = _spied(lambda: k2b.optimize_params_sequence_2d(pixels[:3], **dict(kw, config=cfg)))
    assert calls["fit_image_sequences"] == 0 and len(res) == 3
    fitter = ImageSpaceFitter(model, step_size=1e-2, num_iters=FIRST, joints_category="AMASS", pose_prior=prior)
    rows = RC.init_params(kind, model, *(np.repeat(a, 3, axis=0) for a in start))
    out, joints, _, loss = fitter.fit_batch(rows, pixels[:3], FOCAL, PP, np.ones((3, K), np.float32), per_frame_conf=True)
    ref = fitter.result_params(out, rows)
    for i, r in enumerate(res):
        for f in KEYS:
            assert torch.equal(getattr(r.params, f), getattr(ref, f)[i:i + 1]), (i, f)
        assert torch.equal(r.joints, joints[i:i + 1]) and torch.equal(r.loss, loss[i])


def test_an_empty_video_writes_nothing_and_changes_nothing():
    kind = "smpl10"
    pixels, _, start = _motion(kind)
    model, prior = RC.assets(kind)
    fitter = ImageSpaceFitter(model, step_size=1e-2, num_iters=FIRST, joints_category="AMASS", pose_prior=prior, num_iters_followup=FOLLOW)
    rows = lambda n: RC.init_params(kind, model, *(np.repeat(a, n, axis=0) for a in start))
    with_gap, _, _, _ = fitter.fit_sequences(rows(3), pixels[:3], [2, 0, 1], FOCAL, PP, run_forward=False)
    without, _, _, _ = fitter.fit_sequences(rows(2), pixels[:3], [2, 1], FOCAL, PP, run_forward=False)
    for k in KEYS + ("loss",):
        assert torch.equal(with_gap[k], without[k]), k
    none, joints, verts, loss = fitter.fit_sequences(rows(1), pixels[:0], [0], FOCAL, PP)
    assert tuple(none["body_pose"].shape) == (0, 69) and tuple(loss.shape) == (0,) and joints.shape[0] == 0


def test_lbfgs_is_refused_and_the_old_entries_keep_refusing_2d_input():
    kind = "smpl10"
    pixels, _, _ = _motion(kind)
    kw = _kw(kind)
    lb = SequenceOptimizeConfig(frame=FrameOptimizeConfig(use_lbfgs=True))
    with pytest.raises(NotImplementedError, match="L-BFGS"):
        k2b.optimize_params_sequence_2d(pixels, **dict(kw, config=lb))
    with pytest.raises(NotImplementedError, match="L-BFGS"):
        k2b.optimize_params_sequences_2d([pixels], **dict(kw, config=lb, init_params=[kw["init_params"]]))
    with pytest.raises(NotImplementedError, match="joints2d"):
        k2b.optimize_params_sequence(np.zeros((2, 22, 3), np.float32), model=kw["model"], pose_prior=kw["pose_prior"],
                                     config={"frame": {"input_type": "joints2d"}})
