"""Host (no GPU): ``k2b_lbs_backward`` is declared, exported, in the ctypes table, and answers a NULL model before any HIP call."""
import ctypes as C
import re
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]


def test_entry_is_declared_exported_and_versioned():
    from keypoints2body_amd import native
    header = (REPO / "include" / "k2b.h").read_text()
    declared = set(re.findall(r"\b(k2b_[a-z_]+)\s*\(", header))
    assert "k2b_lbs_backward" in declared and "k2b_lbs_backward" in native.EXPORTED_SYMBOLS
    lib = native.load_library()
    assert hasattr(lib, "k2b_lbs_backward")
    assert lib.k2b_version() >> 16 == 1 and (lib.k2b_version() & 0xffff) >= 4      # the minor version grew with the entry


def _abi_call(model, num_frames):
    """The entry with every buffer NULL (as ``_abi_call`` of tests/test_sequences_host.py: the checks come before any HIP call)."""
    from keypoints2body_amd import native
    lib = native.load_library()
    return lib.k2b_lbs_backward(model, num_frames, *([None] * 10), None)


def test_null_model_is_refused_before_any_hip_call():
    from keypoints2body_amd import native
    lib = native.load_library()
    assert _abi_call(None, 4) == native.K2B_ERR_INVALID_ARGUMENT
    assert b"model" in lib.k2b_last_error()
    assert _abi_call(None, 0) == native.K2B_ERR_INVALID_ARGUMENT                  # a NULL model even with nothing to do


def test_prototype_matches_the_header_argument_by_argument():
    """The entry's declaration carries the ``K2B_SINCE(1, 4)`` marker behind its argument list, so it is checked here: the
    number of arguments and each one's kind (pointer = the declaration has a ``*``, else ``int32_t``), and the result."""
    from keypoints2body_amd import native
    header = re.sub(r"/\*.*?\*/", " ", (REPO / "include" / "k2b.h").read_text(), flags=re.S)
    (result, args), = re.findall(r"([\w \*]+?)\bk2b_lbs_backward\s*\(([^()]*)\)\s*K2B_SINCE\(1, 4\)\s*;", header)
    want = ["pointer" if "*" in a else re.search(r"\b(int32_t)\b", a).group(1) for a in args.split(",")]
    fn = native.load_library().k2b_lbs_backward
    got = ["pointer" if t is C.c_void_p else {C.c_int32: "int32_t"}[t] for t in fn.argtypes]
    assert len(want) == 13 and got == want, (want, got)
    assert result.strip() == "int" and fn.restype is C.c_int
