"""The host driver of the device L-BFGS (csrc/k2b_lbfgs_plan.h) without a GPU: the stand-alone program
``tests/host/lbfgs_plan_check.cpp`` replays the schedule of launches for the three schemes and ``max_iter`` 1 to 40 and 10000 (launch
counts, every step on the result of the closure before it, no launch reading the buffer it writes, the rounds consumed and then one
finalise, where the last loss lands), holds the iteration counts to torch's rule, the state layout to a sum made frame by frame, every
workspace map to the pointer arithmetic the entries used to do by hand, and the step kernel's plan to a count of the history pairs
that fit in 48 KiB.  Built with the address and undefined-behaviour sanitizers, as ``tests/test_launch_plan_host.py``."""
import shutil
import subprocess
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
CSRC = REPO / "keypoints2body_amd" / "csrc"
SECTIONS = ["schedule", "counts", "state layout", "workspace maps", "step plan"]


def _host_compiler():
    """The HIP toolchain's clang (the header is the one the kernels compile), else the system's."""
    for c in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++", "clang++"):
        if shutil.which(c):
            return c
    return None


def test_lbfgs_plans_match_the_rules_written_out_independently(tmp_path):
    cxx = _host_compiler()
    assert cxx is not None, "the host check needs the clang++ of the HIP toolchain that builds libk2b.so"
    exe = tmp_path / "lbfgs_plan_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", str(CSRC),
                    str(REPO / "tests" / "host" / "lbfgs_plan_check.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout + run.stderr)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    lines = run.stdout.splitlines()
    for section in SECTIONS:
        assert f"{section}: ok" in lines, section
    assert lines[-1] == "0 failures"
