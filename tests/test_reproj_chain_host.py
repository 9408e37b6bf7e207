"""No GPU: the surface of the projected warm-start chains (``k2b_fit_image_sequences``, ABI 1.8; ``optimize_params_sequence_2d`` /
``optimize_params_sequences_2d``) and the condition on the oracle chain that tests/test_gpu_reproj_chain.py gates against."""
import ctypes
import inspect
import re
from pathlib import Path

import pytest

import keypoints2body_amd as k2b
from keypoints2body_amd import native
from tests import reproj_chain_common as RC

REPO = Path(__file__).resolve().parents[1]
NAME = "k2b_fit_image_sequences"


def _declaration():
    header = re.sub(r"/\*.*?\*/", " ", (REPO / "include" / "k2b.h").read_text(), flags=re.S)
    decls = re.findall(rf"([\w \*]+?)\b({NAME})\s*\(([^()]*)\)\s*K2B_SINCE\(1, 8\)\s*;", header)
    assert [name for _, name, _ in decls] == [NAME], "declared once, with K2B_SINCE(1, 8) behind the argument list"
    return decls[0]


def test_the_header_declares_the_entry_since_1_8():
    result, _, args = _declaration()
    assert result.strip() == "int"
    names = [a.split()[-1].lstrip("*") for a in args.split(",")]
    assert names == ["model", "prior", "cfg", "num_sequences", "lengths", "offsets", "followup_iters", "followup_freeze_betas", "num_targets",
                     "model_joint_index", "keypoints", "conf", "global_orient_in", "body_pose_in", "betas_in", "transl_in", "global_orient_out",
                     "body_pose_out", "betas_out", "transl_out", "loss_out", "stream"]


def test_the_symbol_is_exported_and_versioned():
    lib = native.load_library()
    assert NAME in native.EXPORTED_SYMBOLS and hasattr(lib, NAME)
    assert lib.k2b_version() >> 16 == 1 and (lib.k2b_version() & 0xffff) >= 8
    assert callable(native.fit_image_sequences)


def test_the_ctypes_prototype_matches_the_header_argument_by_argument():
    result, name, args = _declaration()
    lib = native.load_library()
    kinds = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double}
    want = ["pointer" if "*" in a else next(k for k in kinds if re.search(rf"\b{k}\b", a)) for a in args.split(",")]
    got = ["pointer" if t is ctypes.c_void_p or issubclass(t, ctypes._Pointer) else next(k for k, c in kinds.items() if c is t)
           for t in getattr(lib, name).argtypes]
    assert got == want, (name, want, got)
    assert getattr(lib, name).restype is ctypes.c_int
    # k2b_fit_sequences' arguments with followup_freeze_betas behind followup_iters
    seqs = list(lib.k2b_fit_sequences.argtypes)
    assert list(getattr(lib, name).argtypes) == seqs[:7] + [ctypes.c_int32] + seqs[7:]


def test_the_public_functions_are_exported_with_keyword_only_intrinsics():
    for fn_name in ("optimize_params_sequence_2d", "optimize_params_sequences_2d"):
        assert fn_name in k2b.__all__
        p = inspect.signature(getattr(k2b, fn_name)).parameters
        for key in ("focal", "principal_point"):
            assert p[key].kind is inspect.Parameter.KEYWORD_ONLY and p[key].default is inspect.Parameter.empty, (fn_name, key)
        assert list(p)[0] in ("keypoints_seq", "keypoints_seqs") and "config" in p
    assert "num_iters_followup" in inspect.signature(k2b.core.fitters.image_space.ImageSpaceFitter.__init__).parameters


@pytest.mark.parametrize("freeze", (False, True))
@pytest.mark.parametrize("kind", RC.ORACLE_KINDS)
def test_the_float32_oracle_chain_stays_within_a_quarter_of_the_gate(kind, freeze):
    """From the oracle alone: over the whole gated chain (3 sequences x 3 frames, 10 / 5 iterations) the float32
    ``torch.optim.Adam`` loop sits within 2.5e-5 of the float64 one, so ``trajectory_gate``'s widening ``4 x deviation`` never
    exceeds its floor of 1e-4 and the device is held to 1e-4 throughout."""
    dev = RC.f32_loop_deviation(kind, freeze)
    print(f"{kind}{' frozen' if freeze else ''}: float32 oracle chain off the float64 one by {dev:.2e} (limit {RC.F32_LOOP_LIMIT:.1e})")
    assert dev <= RC.F32_LOOP_LIMIT
