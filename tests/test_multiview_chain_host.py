"""No GPU: the surface of the multi-view warm-start chains (``k2b_fit_multiview_sequences``, ABI 1.11;
``optimize_params_sequence_multiview`` / ``optimize_params_sequences_multiview``), what the entry refuses (the stand-alone program
``tests/host/multiview_chain_rules_check.cpp`` over csrc/k2b_fit_rules.h, built with the address and undefined-behaviour sanitizers
as tests/test_fit_rules_host.py builds its own), and the argument checks of the Python layers.  (Without a device every call that
reaches the device layer raises ``RuntimeError``; a ``ValueError`` or ``NotImplementedError`` here therefore came first.)"""
import ctypes
import inspect
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import keypoints2body_amd as k2b
from keypoints2body_amd import native
from tests import multiview_common as MV

REPO = Path(__file__).resolve().parents[1]
CSRC = REPO / "keypoints2body_amd" / "csrc"
NAME = "k2b_fit_multiview_sequences"
IDENTITY = ([1, 0, 0, 0, 1, 0, 0, 0, 1], [0, 0, 3], [500, 430])


def _declaration():
    header = re.sub(r"/\*.*?\*/", " ", (REPO / "include" / "k2b.h").read_text(), flags=re.S)
    decls = re.findall(rf"([\w \*]+?)\b({NAME})\s*\(([^()]*)\)\s*K2B_SINCE\(1, 11\)\s*;", header)
    assert [n for _, n, _ in decls] == [NAME], "declared once, with K2B_SINCE(1, 11) behind the argument list"
    return decls[0]


def test_the_header_declares_the_entry_since_1_11():
    result, _, args = _declaration()
    assert result.strip() == "int"
    names = [a.split()[-1].lstrip("*") for a in args.split(",")]
    assert names == ["model", "prior", "cfg", "num_sequences", "lengths", "offsets", "followup_iters", "followup_freeze_betas", "num_views", "cameras",
                     "num_targets", "model_joint_index", "keypoints", "conf", "global_orient_in", "body_pose_in", "betas_in", "transl_in",
                     "global_orient_out", "body_pose_out", "betas_out", "transl_out", "loss_out", "stream"]
    header = (REPO / "include" / "k2b.h").read_text()
    # the Conventions lists that enumerate the entries with a frame or sequence dimension name it, and the guarantees stand next to it
    assert header.count(NAME) >= 4
    for phrase in ("bit-identical to that sequence fitted alone", "host loop of k2b_fit_multiview calls", "summed in the order 0 .. C - 1",
                   "stays in its own SEQUENCE"):
        assert phrase in header, phrase


def test_the_symbol_is_exported_and_the_minor_version_is_bumped():
    lib = native.load_library()
    assert NAME in native.EXPORTED_SYMBOLS and hasattr(lib, NAME)
    assert lib.k2b_version() >> 16 == 1 and (lib.k2b_version() & 0xffff) >= 11
    assert callable(native.fit_multiview_sequences)


def test_the_ctypes_prototype_matches_the_header_argument_by_argument():
    result, name, args = _declaration()
    lib = native.load_library()
    kinds = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double}
    want = ["pointer" if "*" in a else next(k for k in kinds if re.search(rf"\b{k}\b", a)) for a in args.split(",")]
    got = ["pointer" if t is ctypes.c_void_p or issubclass(t, ctypes._Pointer) else next(k for k, c in kinds.items() if c is t)
           for t in getattr(lib, name).argtypes]
    assert got == want, (name, want, got)
    assert getattr(lib, name).restype is ctypes.c_int
    # k2b_fit_image_sequences' arguments with num_views and cameras behind followup_freeze_betas
    image = list(lib.k2b_fit_image_sequences.argtypes)
    assert list(getattr(lib, name).argtypes) == image[:8] + [ctypes.c_int32, ctypes.POINTER(native.CameraC)] + image[8:]
    assert lib.k2b_fit_config_size() == ctypes.sizeof(native.FitConfigC) and lib.k2b_camera_size() == ctypes.sizeof(native.CameraC)


def test_the_public_functions_are_exported_with_keyword_only_cameras():
    for fn_name in ("optimize_params_sequence_multiview", "optimize_params_sequences_multiview"):
        assert fn_name in k2b.__all__
        p = inspect.signature(getattr(k2b, fn_name)).parameters
        assert p["cameras"].kind is inspect.Parameter.KEYWORD_ONLY and p["cameras"].default is inspect.Parameter.empty, fn_name
        assert list(p)[0] in ("keypoints", "keypoints_seqs") and "config" in p
    from keypoints2body_amd.core.fitters.multiview import MultiViewFitter
    assert "num_iters_followup" in inspect.signature(MultiViewFitter.__init__).parameters
    assert callable(MultiViewFitter.fit_sequences)
    # the three places that said the chain is missing no longer do
    for text in (inspect.getsource(k2b.api.multiview), (REPO / "DESIGN.md").read_text()):
        assert "multi-view videos is not built" not in text and "is not built: ``optimize_params_frames_multiview``" not in text


# ---- the rules, without a device -------------------------------------------------------------------------------------------------
def _host_compiler():
    """The HIP toolchain's clang (the header is the one the library compiles), else the system's."""
    for c in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++", "clang++"):
        if shutil.which(c):
            return c
    return None


def test_the_rules_of_the_entry_and_of_the_other_ten(tmp_path):
    cxx = _host_compiler()
    assert cxx is not None, "the host check needs the clang++ of the HIP toolchain that builds libk2b.so"
    exe = tmp_path / "multiview_chain_rules_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", str(CSRC),
                    str(REPO / "tests" / "host" / "multiview_chain_rules_check.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout + run.stderr)
    assert run.returncode == 0, run.stdout[-6000:] + run.stderr[-4000:]
    assert run.stdout.splitlines()[-1] == "0 failures"


def _call(cfg, views, table, lengths=(2, 1), offsets=(0, 2), followup=5):
    lib = native.load_library()
    L, O = np.asarray(lengths, dtype=np.int32), np.asarray(offsets, dtype=np.int32)
    code = lib.k2b_fit_multiview_sequences(None, None, cfg, len(L), L.ctypes.data_as(ctypes.c_void_p), O.ctypes.data_as(ctypes.c_void_p), followup, 1,
                                           views, table, 1, *([None] * 13))
    return code, lib.k2b_last_error().decode()


def test_the_library_refuses_what_follows_no_handle_under_the_entrys_name():
    """NULL handles throughout: the table of sequences and the views are judged before the handles are followed - and before any
    HIP call, which this machine could not answer.  (Everything that needs a model: the host program above, and
    tests/test_gpu_multiview_chain.py.)"""
    cfg = native.default_fit_config()
    cfg.projection = 1
    good = native.camera_table([IDENTITY])
    code, msg = _call(cfg, 1, good, offsets=(0, 3))
    assert code == native.K2B_ERR_INVALID_ARGUMENT and f"{NAME}: offsets[1]=3, expected 2" in msg, msg
    code, msg = _call(cfg, 1, good, lengths=(2, -1))
    assert code == native.K2B_ERR_INVALID_ARGUMENT and f"{NAME}: lengths[1]=-1" in msg, msg
    for views in (0, 9):
        code, msg = _call(cfg, views, good)
        assert code == native.K2B_ERR_INVALID_ARGUMENT and f"{NAME}: num_views={views}" in msg, msg
    code, msg = _call(cfg, 1, None)
    assert code == native.K2B_ERR_INVALID_ARGUMENT and f"{NAME}: cameras is NULL" in msg, msg
    cfg.projection = 0
    code, msg = _call(cfg, 1, good)
    assert code == native.K2B_ERR_INVALID_ARGUMENT and f"{NAME}: projection=0" in msg, msg
    cfg.projection = 1
    table = native.camera_table([IDENTITY, IDENTITY])
    table[1].translation[2] = float("nan")
    code, msg = _call(cfg, 2, table)
    assert code == native.K2B_ERR_INVALID_ARGUMENT and f"{NAME}: cameras[1].translation[2]" in msg, msg
    table = native.camera_table([IDENTITY])
    table[0].focal[0] = 0.0
    code, msg = _call(cfg, 1, table)
    assert code == native.K2B_ERR_INVALID_ARGUMENT and f"{NAME}: focal[0]" in msg, msg
    code, msg = _call(cfg, 1, good)
    assert code == native.K2B_ERR_INVALID_ARGUMENT and f"{NAME}: model, prior and cfg are required" in msg, msg


# ---- the Python layers, without a device --------------------------------------------------------------------------------------------
def _cams(C=2):
    return [k2b.Camera(Rc, tc, tuple(fc), (0.0, 0.0)) for Rc, tc, fc in MV.rig(C)]


ADAM = {"frame": {"use_lbfgs": False}}


def test_argument_errors_of_the_public_functions_come_before_any_device_call():
    cams = _cams()
    with pytest.raises(ValueError, match=r"\(T,C,K,2\)"):
        k2b.optimize_params_sequence_multiview(np.zeros((2, 22, 2)), cameras=cams, config=ADAM)
    with pytest.raises(ValueError, match="C = 2 cameras"):
        k2b.optimize_params_sequence_multiview(np.zeros((4, 3, 22, 2)), cameras=cams, config=ADAM)
    with pytest.raises(ValueError, match="between 1 and 8 cameras"):
        k2b.optimize_params_sequence_multiview(np.zeros((4, 10, 22, 2)), cameras=cams * 5, config=ADAM)
    with pytest.raises(ValueError, match="Camera objects"):
        k2b.optimize_params_sequence_multiview(np.zeros((4, 1, 22, 2)), cameras=[MV.rig(1)[0]], config=ADAM)
    with pytest.raises(NotImplementedError, match="kinematic targets only"):
        k2b.optimize_params_sequence_multiview({"body": np.zeros((4, 2, 22, 2))}, cameras=cams, config=ADAM)
    with pytest.raises(NotImplementedError, match="kinematic targets only"):
        k2b.optimize_params_sequences_multiview([np.zeros((4, 2, 22, 2)), {"body": np.zeros((4, 2, 22, 2))}], cameras=cams, config=ADAM)
    with pytest.raises(NotImplementedError, match="Adam only"):
        k2b.optimize_params_sequence_multiview(np.zeros((4, 2, 22, 2)), cameras=cams, config={"frame": {"use_lbfgs": True}})
    with pytest.raises(NotImplementedError, match="Adam only"):
        k2b.optimize_params_sequences_multiview([np.zeros((4, 2, 22, 2))], cameras=cams, config=k2b.core.config.SequenceOptimizeConfig())
    with pytest.raises(TypeError, match="list of sequences"):
        k2b.optimize_params_sequences_multiview(np.zeros((4, 2, 22, 2)), cameras=cams, config=ADAM)
    with pytest.raises(ValueError, match="is empty"):
        k2b.optimize_params_sequences_multiview([], cameras=cams, config=ADAM)
    with pytest.raises(ValueError, match="same number of keypoints"):
        k2b.optimize_params_sequences_multiview([np.zeros((4, 2, 22, 2)), np.zeros((4, 2, 24, 2))], cameras=cams, config=ADAM)
    with pytest.raises(ValueError, match="one start per sequence"):
        k2b.optimize_params_sequences_multiview([np.zeros((4, 2, 22, 2))] * 2, cameras=cams, config=ADAM, init_params=[None])
    with pytest.raises(ValueError, match="Unsupported body_model"):
        k2b.optimize_params_sequence_multiview(np.zeros((4, 2, 22, 2)), cameras=cams, config=ADAM, body_model="mano")


def test_argument_errors_of_the_ctypes_mirror_come_before_any_device_call():
    import torch
    table = native.camera_table([IDENTITY, IDENTITY])
    z = torch.zeros
    with pytest.raises(ValueError, match=r"\(sum T, C, K, 3\)"):
        native.fit_multiview_sequences(None, None, native.default_fit_config(), 5, True, table, [0, 1], [2], z(2, 2, 3), None, z(1, 3), z(1, 69),
                                       z(1, 10), z(1, 3))
    with pytest.raises(ValueError, match="3 views for 2 cameras"):
        native.fit_multiview_sequences(None, None, native.default_fit_config(), 5, True, table, [0, 1], [2], z(2, 3, 2, 3), None, z(1, 3), z(1, 69),
                                       z(1, 10), z(1, 3))
    with pytest.raises(ValueError, match="2 entries for 4 targets"):
        native.fit_multiview_sequences(None, None, native.default_fit_config(), 5, True, table, [0, 1], [2], z(2, 2, 4, 3), None, z(1, 3), z(1, 69),
                                       z(1, 10), z(1, 3))
    with pytest.raises(ValueError, match="lengths sum to 3"):
        native.fit_multiview_sequences(None, None, native.default_fit_config(), 5, True, table, [0, 1], [2, 1], z(2, 2, 2, 3), None, z(2, 3), z(2, 69),
                                       z(2, 10), z(2, 3))
