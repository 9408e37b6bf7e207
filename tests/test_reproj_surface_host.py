"""Host side of the projected surface targets (no GPU): the two new symbols of ABI 1.9, the dict-of-blocks input of the 2D entry
points, and the argument errors that must come before any device call.  (Without a device every call that reaches the device
layer raises ``RuntimeError``; a ``ValueError`` here therefore came first.)"""
import numpy as np
import pytest
import torch

import keypoints2body_amd as k2b
from keypoints2body_amd import native
from keypoints2body_amd.api import image
from keypoints2body_amd.core.joints import adapters


def test_the_new_entries_are_exported_at_abi_1_9():
    lib = native.load_library()
    assert lib.k2b_version() >> 16 == 1 and (lib.k2b_version() & 0xffff) >= 9
    for name in ("k2b_fit_image", "k2b_surface_term_image"):
        assert name in native.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert len(lib.k2b_fit_image.argtypes) == len(lib.k2b_fit_world.argtypes) == 21
    assert len(lib.k2b_surface_term_image.argtypes) == len(lib.k2b_surface_term.argtypes) + 1


def test_the_new_entries_refuse_bad_calls_on_the_host():
    """NULL handles are refused by name before anything is touched (the pointers are never followed)."""
    lib = native.load_library()
    cfg = native.default_fit_config()
    assert lib.k2b_fit_image(None, None, cfg, 1, 1, *([None] * 16)) == native.K2B_ERR_INVALID_ARGUMENT
    assert b"k2b_fit_image" in lib.k2b_last_error()
    assert lib.k2b_surface_term_image(None, 1, 1, None, None, None, 0, 100.0, 1.0, *([None] * 8)) == native.K2B_ERR_INVALID_ARGUMENT
    assert b"k2b_surface_term_image" in lib.k2b_last_error()


def _blocks(counts, frames=None, cols=2):
    rng = np.random.default_rng(5)
    lead = () if frames is None else (frames,)
    return {name: rng.normal(size=lead + (k, cols)) for name, k in counts.items()}


@pytest.mark.parametrize("body_model,counts", (("smplx", dict(body=22, left_hand=21, right_hand=21, face=51)),
                                               ("smplx", dict(body=24, face=17)),
                                               ("smplh", dict(body=22, right_hand=21))))
@pytest.mark.parametrize("frames", (None, 3))
def test_dict_blocks_map_to_the_indices_of_the_3d_dict_input(body_model, counts, frames):
    b2 = _blocks(counts, frames, cols=3)
    kp, idx = image._blocks_2d(b2, body_model, frames is not None, None)
    b3 = {k: np.concatenate([v, np.ones(v.shape[:-1] + (1,))], axis=-1).astype(np.float32) for k, v in b2.items()}   # (x, y, z, conf)
    _, _, idx3, _ = adapters._normalize_blocks(b3, body_model, sequence=frames is not None)
    assert idx == idx3.tolist()
    K = sum(counts.values())
    assert kp.shape == (() if frames is None else (frames,)) + (K, 3)
    order = [n for n, _, _ in adapters._BLOCKS if n in counts]
    assert np.array_equal(kp, np.concatenate([b2[n] for n in order], axis=-2))
    if "face" in counts:
        assert idx[-counts["face"]] == 67                      # the face block at 67 ..
    # two columns: the confidence is one
    kp2, _ = image._blocks_2d({k: v[..., :2] for k, v in b2.items()}, body_model, frames is not None, None)
    assert np.array_equal(kp2[..., :2], kp[..., :2]) and (kp2[..., 2] == 1.0).all()


def test_argument_errors_come_before_any_device_call():
    kw = dict(focal=500.0, principal_point=(0.0, 0.0))
    seq = _blocks(dict(body=22, face=51), frames=3)
    seq["face"] = seq["face"][:2]
    with pytest.raises(ValueError, match="share same T"):
        k2b.optimize_params_sequence_2d(seq, body_model="smplx", **kw)
    with pytest.raises(ValueError, match="share same T"):
        k2b.optimize_params_sequences_2d([seq], body_model="smplx", **kw)
    with pytest.raises(ValueError, match="face block requires body_model='smplx'"):
        k2b.optimize_params_frame_2d(_blocks(dict(body=22, face=51)), body_model="smplh", **kw)
    with pytest.raises(ValueError, match="requires body_model='smplh' or 'smplx'"):
        k2b.optimize_params_frame_2d(_blocks(dict(body=22, left_hand=21)), body_model="smpl", **kw)
    with pytest.raises(ValueError, match="torso joints"):                        # hands alone: no hips, no shoulders
        k2b.optimize_params_frame_2d(_blocks(dict(left_hand=21, right_hand=21)), body_model="smplx", **kw)
    with pytest.raises(ValueError, match="torso joints"):
        k2b.optimize_params_sequence_2d(_blocks(dict(face=51), frames=2), body_model="smplx", **kw)
    with pytest.raises(ValueError, match="target_model_indices must be None"):
        k2b.optimize_params_frame_2d(_blocks(dict(body=22)), body_model="smplx", target_model_indices=list(range(22)), **kw)
    with pytest.raises(ValueError, match="unknown keypoint blocks"):
        k2b.optimize_params_frame_2d(dict(_blocks(dict(body=22)), feet=np.zeros((6, 2))), body_model="smplx", **kw)
    with pytest.raises(ValueError, match="must have 21 joints"):
        k2b.optimize_params_frame_2d(_blocks(dict(body=22, left_hand=20)), body_model="smplx", **kw)
    with pytest.raises(ValueError, match="every sequence is a dict"):
        k2b.optimize_params_sequences_2d([_blocks(dict(body=22), frames=2), torch.zeros(2, 22, 2)], body_model="smplx", **kw)
    with pytest.raises(ValueError, match="the same blocks"):
        k2b.optimize_params_sequences_2d([_blocks(dict(body=22), frames=2), _blocks(dict(body=24), frames=2)], body_model="smplx", **kw)
