"""The model handle's host tables (csrc/k2b_tree.h, k2b_scan_plan.h, k2b_model_tables.h) without a GPU: the stand-alone program
``tests/host/model_tables_check.cpp`` builds every lane, ancestor and prior-column table for the SMPL, SMPL-H and SMPL-X trees and
the odd trees of ``tests/fit_gradient_common.py``, the vertex-set images of a toy model, the surface index and the LBS backward's
item image, and checks each against a brute-force definition.  Built with the address and undefined-behaviour sanitizers: the
builders index by lane, joint and fragment, and a wrong index should stop here, not on the GPU."""
import shutil
import subprocess
from pathlib import Path

from keypoints2body_amd import synthetic
from tests import fit_gradient_common as F

REPO = Path(__file__).resolve().parents[1]
CSRC = REPO / "keypoints2body_amd" / "csrc"


def _host_compiler():
    """A host C++ compiler with ``_Float16`` (the images are f16): the HIP toolchain's clang, else the system's."""
    for c in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++", "clang++"):
        if shutil.which(c):
            return c
    return None


def test_model_tables_match_their_brute_force_definitions(tmp_path):
    cxx = _host_compiler()
    assert cxx is not None, "the host check needs the clang++ of the HIP toolchain that builds libk2b.so"
    exe = tmp_path / "model_tables_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", str(CSRC),
                    str(REPO / "tests" / "host" / "model_tables_check.cpp"), "-o", str(exe)], check=True)
    trees = {"smpl": synthetic.SMPL_PARENTS, "smplh": synthetic.SMPLH_PARENTS, "smplx": synthetic.SMPLX_PARENTS}
    trees.update({k: F.TREES[k] for k in ("tree21", "tree26", "tree64")})
    # a second tree with a scan plan (tests/test_fit_scan_plan.py): longer and shorter limbs, a second spine branch
    trees["limbs24"] = [-1, 0, 1, 2, 3, 4, 5, 6, 0, 8, 0, 10, 11, 12, 13, 12, 15, 16, 17, 18, 19, 12, 21, 22]
    args = [f"{name}={','.join(str(int(p)) for p in parents)}" for name, parents in trees.items()]
    run = subprocess.run([str(exe)] + args, capture_output=True, text=True)
    print(run.stdout + run.stderr)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    for name in trees:
        assert any(line.startswith(name) and line.endswith(": ok") for line in run.stdout.splitlines()), name
    assert run.stdout.splitlines()[-1] == "0 failures"
