"""The launch policy of the fit kernels and the device L-BFGS (csrc/k2b_launch_plan.h) without a GPU: the stand-alone program
``tests/host/launch_plan_check.cpp`` plans every batch size from 0 to three full-width launches and a bit, for five CU counts, every
forced shape, every L-BFGS mode, chains on and off, and holds each plan to the rules as DESIGN.md words them, restated in the
program: shapes by frames per CU, the split into whole rounds plus a remainder, the chain and L-BFGS slot counts, the agreement
of ``lbfgs_scheme_for`` with the plans, the tree kernel's plan, the staged history pairs against a brute-force count and the LDS
layout's sum.  Built with the address and undefined-behaviour sanitizers, as ``tests/test_model_tables_host.py``."""
import shutil
import subprocess
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
CSRC = REPO / "keypoints2body_amd" / "csrc"
SECTIONS = [f"{what} C={c}" for c in (1, 8, 64, 256, 304) for what in ("fit_world", "schemes", "fit_tree")] + [
    "pinned rows", "LDS layout and staged pairs", "persistent_grid"]


def _host_compiler():
    """The HIP toolchain's clang (the header is the one the kernels compile), else the system's."""
    for c in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++", "clang++"):
        if shutil.which(c):
            return c
    return None


def test_launch_plans_match_the_rules_written_out_independently(tmp_path):
    cxx = _host_compiler()
    assert cxx is not None, "the host check needs the clang++ of the HIP toolchain that builds libk2b.so"
    exe = tmp_path / "launch_plan_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", str(CSRC),
                    str(REPO / "tests" / "host" / "launch_plan_check.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout + run.stderr)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    lines = run.stdout.splitlines()
    for section in SECTIONS:
        assert f"{section}: ok" in lines, section
    assert lines[-1] == "0 failures"
