"""Host (no GPU): the float64 oracle of the positional-error tests is itself right and its cases are well conditioned, and
``k2b_point_error`` is declared, exported, prototyped and refuses bad calls before any HIP call."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from tests import point_error_common as P

REPO = Path(__file__).resolve().parents[1]


def test_oracle_recovers_a_known_similarity():
    for scale, mode in ((True, 3), (False, 2)):
        pred, _, s, R, t = P.known_transform_case(scale=scale)
        x = pred.astype(np.float64)
        y = s[:, None, None] * np.einsum("bij,bnj->bni", R, x) + t[:, None, :]          # exact in float64: not rounded to float32
        o = P.oracle(x, y, None, mode)
        L = P.frame_scale(x, y)
        assert np.all(o["err"] <= 1e-12 * L), o["err"]
        assert np.allclose(o["transform"][:, 0], s, rtol=0, atol=1e-12)
        assert np.allclose(o["transform"][:, 1:10].reshape(-1, 3, 3), R, rtol=0, atol=1e-12)
        assert np.allclose(o["transform"][:, 10:], t, rtol=0, atol=1e-12)
        assert np.all(P.oracle_horn_err(x, y, None, scale) <= 1e-12 * L)


def test_oracle_keeps_a_proper_rotation_for_a_mirrored_copy():
    pred, gt = P.mirrored_case()
    for mode in (2, 3):
        o = P.oracle(pred, gt, None, mode)
        R = o["transform"][:, 1:10].reshape(-1, 3, 3)
        assert np.allclose(np.linalg.det(R), 1.0, atol=1e-12)
        assert np.allclose(R @ R.transpose(0, 2, 1), np.eye(3), atol=1e-12)
        assert np.all(o["err"] > 0.05), o["err"]                     # a 1 x 1.8 x 3.2 m cloud mirrored: far from aligned
        assert np.all(o["gap"] > 1e-2)                               # and the best proper rotation is still unique
    free = P.oracle(pred, gt * np.array([-1.0, 1.0, 1.0], np.float32), None, 2)         # un-mirrored: aligns to float32 rounding
    assert np.all(free["err"] < 1e-6)


def _all_cases():
    yield from P.parity_cases()
    pred, gt = P.mirrored_case()
    yield "mirrored", pred, gt, None
    for scale in (True, False):
        pred, gt, *_ = P.known_transform_case(scale=scale)
        yield f"known-scale{int(scale)}", pred, gt, None


def test_every_gpu_case_is_well_conditioned():
    """The SVD and the quaternion formulation agree on every frame's error to 1e-12 L: the optimum the GPU test compares against is
    determined to far below its tolerance.  No case is excluded."""
    for name, pred, gt, w in _all_cases():
        L = P.frame_scale(pred, gt)
        for mode, scale in ((2, False), (3, True)):
            a, b = P.oracle(pred, gt, w, mode)["err"], P.oracle_horn_err(pred, gt, w, scale)
            assert np.all(np.abs(a - b) <= 1e-12 * L), (name, mode, np.abs(a - b).max())


def test_entry_is_declared_exported_and_versioned():
    from keypoints2body_amd import native
    header = (REPO / "include" / "k2b.h").read_text()
    assert "k2b_point_error" in set(re.findall(r"\b(k2b_[a-z_]+)\s*\(", header))
    assert "k2b_point_error" in native.EXPORTED_SYMBOLS
    lib = native.load_library()
    assert hasattr(lib, "k2b_point_error")
    assert lib.k2b_version() >> 16 == 1 and (lib.k2b_version() & 0xffff) >= 6


def test_prototype_matches_the_header_argument_by_argument():
    from keypoints2body_amd import native
    header = re.sub(r"/\*.*?\*/", " ", (REPO / "include" / "k2b.h").read_text(), flags=re.S)
    (result, args), = re.findall(r"([\w \*]+?)\bk2b_point_error\s*\(([^()]*)\)\s*K2B_SINCE\(1, 6\)\s*;", header)
    want = ["pointer" if "*" in a else re.search(r"\b(int32_t)\b", a).group(1) for a in args.split(",")]
    fn = native.load_library().k2b_point_error
    got = ["pointer" if t is C.c_void_p else {C.c_int32: "int32_t"}[t] for t in fn.argtypes]
    assert len(want) == 11 and got == want, (want, got)
    assert want == ["int32_t", "int32_t", "pointer", "pointer", "pointer", "int32_t", "int32_t", "pointer", "pointer", "pointer",
                    "pointer"]
    assert result.strip() == "int" and fn.restype is C.c_int


def test_bad_calls_are_refused_on_the_host_before_any_hip_call():
    """No device is needed for a refusal, and the pointers below are never followed."""
    from keypoints2body_amd import native
    lib = native.load_library()
    buf = (C.c_float * 16)()
    ptr = C.c_void_p(C.addressof(buf))
    good = dict(B=4, N=22, pred=ptr, gt=ptr, w=None, per_frame=0, mode=3, err=ptr, pp=None, tf=None, stream=None)

    def call(**kw):
        rc = lib.k2b_point_error(*{**good, **kw}.values())
        return rc, lib.k2b_last_error().decode()
    inv, uns = native.K2B_ERR_INVALID_ARGUMENT, native.K2B_ERR_UNSUPPORTED
    for kw, code, text in (
            (dict(N=0), inv, "num_points=0"), (dict(N=-3), inv, "num_points=-3"), (dict(B=-1), inv, "num_frames=-1"),
            (dict(mode=-1), inv, "align_mode=-1"), (dict(mode=4), inv, "align_mode=4"),
            (dict(pred=None), inv, "NULL"), (dict(gt=None), inv, "NULL"), (dict(err=None), inv, "NULL"),
            (dict(B=0, N=0), inv, "num_points=0"), (dict(B=0, mode=7), inv, "align_mode=7"),
            (dict(N=2 ** 20 + 1), uns, "num_points=1048577"),
            (dict(B=2 ** 24, N=257), uns, "exceeds one launch"), (dict(B=2 ** 26, N=256), uns, "exceeds one launch")):
        rc, msg = call(**kw)
        assert rc == code and text in msg and msg.startswith("k2b_point_error:"), (kw, rc, msg)
    # nothing to do: OK whatever the buffers (checked before the NULL pointers, as k2b_angular_error_deg does)
    assert call(B=0)[0] == native.K2B_OK
    assert call(B=0, pred=None, gt=None, err=None)[0] == native.K2B_OK


def test_python_wrappers_check_their_arguments_before_the_library():
    import torch
    from keypoints2body_amd import evaluation
    if not torch.cuda.is_available():                                # there is no CPU path: the siblings' refusal
        with pytest.raises(RuntimeError, match="HIP device"):
            evaluation.compute_position_error(np.zeros((2, 4, 3), np.float32), np.zeros((2, 4, 3), np.float32))
    with pytest.raises(ValueError, match="align must be one of"):
        evaluation.compute_position_error(np.zeros((2, 4, 3), np.float32), np.zeros((2, 4, 3), np.float32), align="affine")
