"""The host decisions of the LBS pair (csrc/k2b_lbs_plan.h) without a GPU: the stand-alone program ``tests/host/lbs_plan_check.cpp``
walks every layout of 2-64 joints and 1-32 shape coefficients, ten batch sizes, five CU counts, six vertex counts and four landmark
counts, and holds the route and the padding of KX, the pose set-up's capacity, the workspace counts, the padded frames, the pose
grid, the persistent grids, the passes of a forward call (every requested output row written by exactly one pass, nothing else
written, sources before their readers) and the backward's plan (groups, workspace split, dense LDS within 160 KiB, frame rows of
one launch) to the rules as ``k2b_internal.h`` and DESIGN.md word them, restated in the program.  Its ``(J, NB, F, KX, route)`` lines
are the library's own rule: every row of ``lbs_layouts_common.TABLE`` has to be among them.  Built with the address and
undefined-behaviour sanitizers, as ``tests/test_launch_plan_host.py``."""
import shutil
import subprocess
from pathlib import Path

from tests import lbs_layouts_common as L

REPO = Path(__file__).resolve().parents[1]
CSRC = REPO / "keypoints2body_amd" / "csrc"
SECTIONS = ["route table and padding of KX", "pose capacity", "padded frames", "workspace", "pose grid", "persistent grids",
            "forward passes", "backward"]


def _host_compiler():
    """The HIP toolchain's clang (the header is the one the kernels compile), else the system's."""
    for c in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++", "clang++"):
        if shutil.which(c):
            return c
    return None


def test_lbs_plans_match_the_rules_written_out_independently(tmp_path):
    cxx = _host_compiler()
    assert cxx is not None, "the host check needs the clang++ of the HIP toolchain that builds libk2b.so"
    exe = tmp_path / "lbs_plan_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", str(CSRC),
                    str(REPO / "tests" / "host" / "lbs_plan_check.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    lines = run.stdout.splitlines()
    print("\n".join(l for l in lines if not l.startswith("(")) + run.stderr)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    for section in SECTIONS:
        assert f"{section}: ok" in lines, section
    assert lines[-1] == "0 failures"
    # the library's own rule against the table the GPU layout tests are written for
    layouts = {l for l in lines if l.startswith("(")}
    assert len(layouts) == 16 * 32                       # 17-24 and 49-56 joints, 1-32 coefficients
    for J, NB, feats, kx, route in L.TABLE:
        assert f"({J}, {NB}, {feats}, {kx}, {route})" in layouts, (J, NB)
