"""GPU: ``optimize_params_sequence_multiview`` / ``optimize_params_sequences_multiview`` end to end on a synthetic SMPL model.

* many videos side by side equal each video alone, bit for bit;
* a video's first frame has the parameters of ``optimize_params_frame_multiview`` on that frame;
* ``use_previous_frame_init=False`` is ``optimize_params_frames_multiview`` on the same frames from the same starts;
* on a seeded smooth motion seen by four cameras with exact projections the chain ends its last frame no worse than independent
  frames fitted with the follow-up iteration count from the mean pose - the order only, as tests/test_gpu_multiview_api.py
  asserts it: no absolute number is fixed here."""
import functools

import numpy as np
import pytest
import torch

import keypoints2body_amd as k2b
from keypoints2body_amd.core.config import FrameOptimizeConfig, SequenceOptimizeConfig
from keypoints2body_amd.models.smpl_data import SMPLData
from tests import fit_gradient_common as G
from tests import multiview_chain_common as MC
from tests import multiview_common as MV
from tests import reproj_chain_common as RC

pytestmark = pytest.mark.gpu

KIND, FIRST, FOLLOW = "smpl10", 40, 10
LENGTHS = (3, 1, 2)
KEYS = ("global_orient", "body_pose", "betas", "transl")


def _start():
    z = lambda n: torch.zeros((1, n))
    return SMPLData(betas=z(10), global_orient=z(3), body_pose=z(69), transl=None)


def _config(**kw):
    return SequenceOptimizeConfig(frame=FrameOptimizeConfig(use_lbfgs=False, num_iters=FIRST, num_iters_followup=FOLLOW, freeze_betas=True), **kw)


def _kw():
    model, prior = RC.assets(KIND)
    return dict(body_model="smpl", model=model, pose_prior=prior)


def _cameras(cams, pp):
    return [k2b.Camera(Rc, tc, tuple(fc), p) for (Rc, tc, fc), p in zip(cams, pp)]


@functools.lru_cache(maxsize=None)
def _videos():
    """Three videos of lengths (3, 1, 2) seen by two cameras: the packed chain targets of tests/multiview_chain_common.py with every
    camera's principal point added, cut into videos (T, C, K, 2)."""
    c = MC.chain(KIND, 2, LENGTHS, seed=43)
    pp = ((320.5, 240.25), (300.0, 250.0))
    pixels = c.targets[..., :2].astype(np.float64) + np.asarray(pp)[None, :, None, :]
    return [pixels[c.rows(s)] for s in range(len(LENGTHS))], _cameras(c.base.cams, pp)


def _same(a, b, what):
    for key in KEYS:
        assert torch.equal(getattr(a.params, key), getattr(b.params, key)), (what, key)
    assert torch.equal(a.joints, b.joints) and torch.equal(a.vertices, b.vertices) and float(a.loss) == float(b.loss), what


@functools.lru_cache(maxsize=None)
def _alone(s):
    videos, cams = _videos()
    return k2b.optimize_params_sequence_multiview(videos[s], cameras=cams, init_params=_start(), config=_config(), **_kw())


def test_many_videos_side_by_side_equal_each_video_alone():
    videos, cams = _videos()
    batch = k2b.optimize_params_sequences_multiview(videos, cameras=cams, init_params=[_start() for _ in videos], config=_config(), **_kw())
    assert isinstance(batch, k2b.SequenceBatch) and batch.lengths.tolist() == list(LENGTHS) and batch.num_frames == sum(LENGTHS)
    for s, n in enumerate(LENGTHS):
        got, want = batch.results(s), _alone(s)
        assert len(got) == len(want) == n
        for t in range(n):
            _same(got[t], want[t], (s, t))
        assert all(bool(torch.isfinite(getattr(r.params, k)).all()) for r in want for k in KEYS)


def test_the_first_frame_has_the_parameters_of_the_frame_entry():
    videos, cams = _videos()
    for s in range(len(LENGTHS)):
        one = k2b.optimize_params_frame_multiview(videos[s][0], cameras=cams, init_params=_start(),
                                                  config=FrameOptimizeConfig(use_lbfgs=False, num_iters=FIRST), **_kw())
        for key in KEYS:
            assert torch.equal(getattr(_alone(s)[0].params, key), getattr(one.params, key)), (s, key)
    # the later frames moved on from it, under the follow-up freeze of the shape
    first, second = _alone(0)[0].params, _alone(0)[1].params
    assert torch.equal(first.betas, second.betas) and not torch.equal(first.body_pose, second.body_pose)


def test_without_the_warm_start_the_frames_are_the_independent_ones():
    videos, cams = _videos()
    got = k2b.optimize_params_sequence_multiview(videos[0], cameras=cams, init_params=_start(), config=_config(use_previous_frame_init=False), **_kw())
    want = k2b.optimize_params_frames_multiview(videos[0], cameras=cams, init_params=[_start() for _ in range(LENGTHS[0])],
                                                config=FrameOptimizeConfig(use_lbfgs=False, num_iters=FIRST), **_kw())
    assert len(got) == len(want) == LENGTHS[0]
    for t in range(LENGTHS[0]):
        _same(got[t], want[t], t)


def test_limit_frames_cuts_the_video():
    videos, cams = _videos()
    got = k2b.optimize_params_sequence_multiview(videos[0], cameras=cams, init_params=_start(), config=_config(limit_frames=2), **_kw())
    assert len(got) == 2
    for t in range(2):
        _same(got[t], _alone(0)[t], t)


# ---- a smooth motion ---------------------------------------------------------------------------------------------------------------
MOTION_T, MOTION_C = 4, 4
MOTION_PP = ((320.5, 240.25), (300.0, 250.0), (310.0, 236.5), (330.25, 244.0))


@functools.lru_cache(maxsize=None)
def _motion():
    """Four frames on the straight line (in axis-angle, translation and all) from one seeded pose a third of the way towards
    another, the shape of the first; exact pixels in the four views of the rig."""
    ends = MV.base(KIND, MOTION_C, B=2, seed=61)
    w = np.linspace(0.0, 1.0 / 3.0, MOTION_T)[:, None]
    mix = lambda a: ((1.0 - w) * a[0:1].astype(np.float64) + w * a[1:2].astype(np.float64)).astype(np.float32)
    go, pose, tr = mix(ends.go), mix(ends.pose), mix(ends.tr)
    shape = np.repeat(ends.shape[0:1], MOTION_T, axis=0)
    uv, z = MV.project64(KIND, go, pose, shape, tr, ends.cams)
    assert (z > 1.0).all()
    K = G.layout(KIND).J
    return uv[:, :, :K] + np.asarray(MOTION_PP)[None, :, None, :], _cameras(ends.cams, MOTION_PP)


def _residual(result, cams, pixels):
    """Mean pixel distance over the views and joints of one frame's fitted world-space joints from `pixels` (C, K, 2)."""
    joints = result.joints[0, :pixels.shape[1]].cpu().double().numpy()
    out = []
    for cam, px in zip(cams, pixels):
        q = joints @ cam.rotation.T + cam.translation
        proj = q[:, :2] / q[:, 2:3] * np.asarray(cam.focal) + np.asarray(cam.principal_point)
        out.append(np.linalg.norm(proj - px, axis=1).mean())
    return float(np.mean(out))


def test_the_chain_ends_no_worse_than_independent_frames_at_the_followup_count():
    pixels, cams = _motion()
    chain = k2b.optimize_params_sequence_multiview(pixels, cameras=cams, init_params=_start(), config=_config(), **_kw())
    apart = k2b.optimize_params_frames_multiview(pixels, cameras=cams, init_params=[_start() for _ in range(MOTION_T)],
                                                 config=FrameOptimizeConfig(use_lbfgs=False, num_iters=FOLLOW), **_kw())
    assert len(chain) == len(apart) == MOTION_T
    last = MOTION_T - 1
    r_chain, r_apart = _residual(chain[last], cams, pixels[last]), _residual(apart[last], cams, pixels[last])
    print(f"last frame: mean reprojection residual {r_chain:.3f} px (chain, {FIRST} / {FOLLOW} iterations) / {r_apart:.3f} px (independent, "
          f"{FOLLOW} iterations from the mean pose)")
    assert np.isfinite(r_chain) and r_chain <= r_apart
