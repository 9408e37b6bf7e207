"""No GPU: the surface of the multi-view fit (``k2b_fit_multiview`` and ``k2b_camera_size``, ABI 1.10; ``Camera``,
``optimize_params_frame_multiview`` / ``optimize_params_frames_multiview``), the refusals that follow no handle, and the host
triangulation.  (Without a device every call that reaches the device layer raises ``RuntimeError``; a ``ValueError`` here
therefore came first.)"""
import ctypes
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import keypoints2body_amd as k2b
from keypoints2body_amd import native
from keypoints2body_amd.core.fitters import multiview
from tests import multiview_common as MV

REPO = Path(__file__).resolve().parents[1]
NAME = "k2b_fit_multiview"
IDENTITY = ([1, 0, 0, 0, 1, 0, 0, 0, 1], [0, 0, 3], [500, 430])


def _declaration(name=NAME):
    header = re.sub(r"/\*.*?\*/", " ", (REPO / "include" / "k2b.h").read_text(), flags=re.S)
    decls = re.findall(rf"([\w \*]+?)\b({name})\s*\(([^()]*)\)\s*K2B_SINCE\(1, 10\)\s*;", header)
    assert [n for _, n, _ in decls] == [name], "declared once, with K2B_SINCE(1, 10) behind the argument list"
    return decls[0]


def test_the_header_declares_the_entry_since_1_10():
    result, _, args = _declaration()
    assert result.strip() == "int"
    names = [a.split()[-1].lstrip("*") for a in args.split(",")]
    assert names == ["model", "prior", "cfg", "num_frames", "num_views", "cameras", "num_targets", "model_joint_index", "keypoints", "conf",
                     "global_orient_in", "body_pose_in", "betas_in", "transl_in", "preserve_pose", "transl_prior_target",
                     "global_orient_out", "body_pose_out", "betas_out", "transl_out", "loss_out", "grad_out", "stream"]
    result, _, args = _declaration("k2b_camera_size")
    assert result.strip() == "uint32_t" and args.strip() == "void"


def test_the_symbols_are_exported_and_versioned():
    lib = native.load_library()
    for name in (NAME, "k2b_camera_size"):
        assert name in native.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.k2b_version() >> 16 == 1 and (lib.k2b_version() & 0xffff) >= 10
    assert callable(native.fit_multiview)


def test_the_ctypes_prototype_and_the_camera_mirror_match_the_header():
    _, name, args = _declaration()
    lib = native.load_library()
    kinds = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double}
    want = ["pointer" if "*" in a else next(k for k in kinds if re.search(rf"\b{k}\b", a)) for a in args.split(",")]
    got = ["pointer" if t is ctypes.c_void_p or issubclass(t, ctypes._Pointer) else next(k for k, c in kinds.items() if c is t)
           for t in getattr(lib, name).argtypes]
    assert got == want, (name, want, got)
    assert getattr(lib, name).restype is ctypes.c_int
    # k2b_fit_world's arguments with num_views and cameras behind num_frames
    world = list(lib.k2b_fit_world.argtypes)
    assert list(getattr(lib, name).argtypes) == world[:4] + [ctypes.c_int32, ctypes.POINTER(native.CameraC)] + world[4:]
    # the struct: the header's fields in the header's order, the size the library reports
    header = (REPO / "include" / "k2b.h").read_text()
    body = re.search(r"typedef struct k2b_camera \{(.*?)\} k2b_camera;", header, flags=re.S).group(1)
    fields = re.findall(r"float (\w+)\[(\d+)\];", re.sub(r"/\*.*?\*/", " ", body, flags=re.S))
    assert fields == [("rotation", "9"), ("translation", "3"), ("focal", "2")]
    assert [(n, t._length_) for n, t in native.CameraC._fields_] == [(n, int(k)) for n, k in fields]
    assert lib.k2b_camera_size() == ctypes.sizeof(native.CameraC) == 56
    assert lib.k2b_fit_config_size() == ctypes.sizeof(native.FitConfigC)          # (the configuration did not grow)


def test_the_public_functions_are_exported_with_keyword_only_cameras():
    for fn_name in ("optimize_params_frame_multiview", "optimize_params_frames_multiview"):
        assert fn_name in k2b.__all__
        p = inspect.signature(getattr(k2b, fn_name)).parameters
        assert p["cameras"].kind is inspect.Parameter.KEYWORD_ONLY and p["cameras"].default is inspect.Parameter.empty, fn_name
        assert list(p)[0] in ("keypoints2d", "keypoints") and "config" in p
    assert "Camera" in k2b.__all__ and "warm-start" in k2b.optimize_params_frames_multiview.__doc__


def _call(cfg, views, table, model=None):
    lib = native.load_library()
    return lib.k2b_fit_multiview(model, None, cfg, 1, views, table, 1, *([None] * 16)), lib.k2b_last_error().decode()


def test_what_concerns_the_views_is_refused_before_any_handle_is_followed():
    """NULL handles throughout: each refusal names its cause, so it came before the check of the handles - and before any HIP
    call, which this machine could not answer.  (Surface targets and the scan plan need a model: tests/test_gpu_multiview_fit.py.)"""
    cfg = native.default_fit_config()
    cfg.projection = 1
    good = native.camera_table([IDENTITY])
    for views in (0, -1, 9):
        code, msg = _call(cfg, views, good)
        assert code == native.K2B_ERR_INVALID_ARGUMENT and f"num_views={views}" in msg, msg
    code, msg = _call(cfg, 1, None)
    assert code == native.K2B_ERR_INVALID_ARGUMENT and "cameras is NULL" in msg
    for projection in (0, 2):
        cfg.projection = projection
        code, msg = _call(cfg, 1, good)
        assert code == native.K2B_ERR_INVALID_ARGUMENT and f"projection={projection}" in msg, msg
    cfg.projection = 1
    for field, slot, value in (("rotation", 4, np.nan), ("rotation", 8, np.inf), ("translation", 2, -np.inf), ("translation", 0, np.nan)):
        table = native.camera_table([IDENTITY, IDENTITY])
        getattr(table[1], field)[slot] = value
        code, msg = _call(cfg, 2, table)
        assert code == native.K2B_ERR_INVALID_ARGUMENT and f"cameras[1].{field}[{slot}]" in msg, msg
    for value in (0.0, -500.0, np.nan, np.inf):
        table = native.camera_table([IDENTITY])
        table[0].focal[1] = value
        code, msg = _call(cfg, 1, table)
        assert code == native.K2B_ERR_INVALID_ARGUMENT and "focal[1]" in msg and NAME in msg, msg
    cfg.focal[0] = cfg.focal[1] = float("nan")                      # cfg->focal is not read: the cameras carry theirs
    code, msg = _call(cfg, 1, good)
    assert code == native.K2B_ERR_INVALID_ARGUMENT and "model, prior and cfg are required" in msg, msg
    assert native.load_library().k2b_fit_multiview(None, None, None, 1, 1, good, 1, *([None] * 16)) == native.K2B_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("C", (2, 4, 8))
def test_the_triangulation_recovers_seeded_points(C):
    rng = np.random.default_rng(C)
    cams = MV.rig(C)
    Rm, t, f = (np.stack([c[i] for c in cams]) for i in range(3))
    X = 0.4 * rng.normal(size=(5, 4, 3))
    q = np.einsum("cij,bnj->bcni", Rm, X) + t[None, :, None, :]
    uv = q[..., :2] / q[..., 2:] * f[None, :, None, :]
    assert np.abs(multiview.triangulate_dlt(uv, np.ones((5, C, 4), bool), Rm, t, f) - X).max() < 1e-9
    # a view that does not see a point takes no part, whatever its row holds
    usable = np.ones((5, C, 4), bool)
    usable[1, 0, 2] = usable[3, C - 1, 0] = False
    uv[1, 0, 2], uv[3, C - 1, 0] = np.nan, 1e9
    if C > 2:
        assert np.abs(multiview.triangulate_dlt(uv, usable, Rm, t, f) - X).max() < 1e-9
    usable[1, 1:, 2] = False
    with pytest.raises(ValueError, match="fewer than two views"):
        multiview.triangulate_dlt(uv, usable, Rm, t, f)


def test_camera_rejects_what_is_no_rotation():
    Rc, tc, fc = MV.rig(3)[1]
    cam = k2b.Camera(Rc, tc, tuple(fc), (320.0, 240.0))
    assert cam.focal == (500.0, 430.0) and cam.rotation.shape == (3, 3)
    assert k2b.Camera(Rc, tc, 500.0, (0, 0)).focal == (500.0, 500.0)
    for bad in (1.001 * Rc, Rc @ np.diag([1.0, 1.0, -1.0]), Rc + 1e-3, Rc[:2], np.full((3, 3), np.nan)):
        with pytest.raises(ValueError, match="rotation"):
            k2b.Camera(bad, tc, 500.0, (0, 0))
    with pytest.raises(ValueError, match="translation"):
        k2b.Camera(Rc, [0.0, np.inf, 1.0], 500.0, (0, 0))
    with pytest.raises(ValueError, match="focal"):
        k2b.Camera(Rc, tc, -1.0, (0, 0))
    with pytest.raises(ValueError, match="principal_point"):
        k2b.Camera(Rc, tc, 500.0, (0, np.nan))


def test_argument_errors_of_the_public_functions_come_before_any_device_call():
    cams = [k2b.Camera(Rc, tc, tuple(fc), (0.0, 0.0)) for Rc, tc, fc in MV.rig(2)]
    with pytest.raises(ValueError, match="C = 2 cameras"):
        k2b.optimize_params_frame_multiview(np.zeros((3, 22, 2)), cameras=cams)
    with pytest.raises(ValueError, match="between 1 and 8 cameras"):
        k2b.optimize_params_frame_multiview(np.zeros((9, 22, 2)), cameras=cams * 5)[0]
    with pytest.raises(ValueError, match="Camera objects"):
        k2b.optimize_params_frame_multiview(np.zeros((1, 22, 2)), cameras=[MV.rig(1)[0]])
    with pytest.raises(NotImplementedError, match="kinematic targets only"):
        k2b.optimize_params_frame_multiview({"body": np.zeros((22, 2))}, cameras=cams)
    with pytest.raises(NotImplementedError, match="Adam only"):
        k2b.optimize_params_frame_multiview(np.zeros((2, 22, 2)), cameras=cams, config={"use_lbfgs": True})
    with pytest.raises(ValueError, match="conf must be"):
        k2b.optimize_params_frame_multiview(np.zeros((2, 22, 2)), cameras=cams, conf=np.ones(22))
    with pytest.raises(ValueError, match=r"\(T,C,K,2\)"):
        k2b.optimize_params_frames_multiview(np.zeros((2, 22, 2)), cameras=cams)
