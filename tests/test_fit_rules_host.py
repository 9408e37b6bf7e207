"""What the ten fit entries refuse (csrc/k2b_fit_rules.h) without a GPU: the stand-alone program ``tests/host/fit_rules_check.cpp``
includes the header alone and is fed the table of bad calls (``tests/fit_refusal_cases.py``) in a plain line format, with the facts
of the handles written out as integers.  Every row must come back with the code and the message that the entries themselves gave
before the header existed (``tests/golden/fit_refusals.json``, recorded on an MI355X), exactly.  The program also sweeps the
accepting side and holds it to a table of what is built, written out independently.  Built with the address and
undefined-behaviour sanitizers, as ``tests/test_launch_plan_host.py``."""
import json
import shutil
import subprocess
from pathlib import Path

import pytest

from keypoints2body_amd import native
from tests import fit_refusal_cases as T

REPO = Path(__file__).resolve().parents[1]
CSRC = REPO / "keypoints2body_amd" / "csrc"
GOLDEN = json.loads((REPO / "tests" / "golden" / "fit_refusals.json").read_text())


def _host_compiler():
    """The HIP toolchain's clang (the header is the one the library compiles), else the system's."""
    for c in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++", "clang++"):
        if shutil.which(c):
            return c
    return None


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = _host_compiler()
    assert cxx is not None, "the host check needs the clang++ of the HIP toolchain that builds libk2b.so"
    exe = tmp_path_factory.mktemp("fit_rules") / "fit_rules_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", str(CSRC),
                    str(REPO / "tests" / "host" / "fit_rules_check.cpp"), "-o", str(exe)], check=True)
    return exe


def test_the_table_and_the_recording_name_the_same_rows():
    assert [c["id"] for c in T.CASES] == list(GOLDEN)
    assert {c["entry"] for c in T.CASES} == set(T.ENTRIES)
    for case in T.CASES:
        row = GOLDEN[case["id"]]
        assert row["entry"] == "k2b_" + case["entry"] and row["code"] in (native.K2B_ERR_INVALID_ARGUMENT, native.K2B_ERR_UNSUPPORTED), row


def test_every_refusal_is_the_recorded_one(program, tmp_path):
    cfg = native.default_fit_config()
    defaults = {k: (tuple(getattr(cfg, k)) if hasattr(getattr(cfg, k), "__len__") else getattr(cfg, k)) for k in T.CFG_FIELDS}
    lines = tmp_path / "cases.txt"
    lines.write_text("".join(T.host_line(case, defaults) + "\n" for case in T.CASES))
    run = subprocess.run([str(program), "cases", str(lines)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    got = {}
    for row in run.stdout.splitlines():
        id, code, message = row.split("\t", 2)
        got[id] = (int(code), message)
    want = {id: (row["code"], row["message"]) for id, row in GOLDEN.items()}
    wrong = {id: (got.get(id), want[id]) for id in want if got.get(id) != want[id]}
    assert not wrong, "\n".join(f"{id}: rules {g}, recorded {w}" for id, (g, w) in wrong.items())
    assert len(got) == len(want)


def test_what_is_built_matches_the_table_written_out_independently(program):
    run = subprocess.run([str(program), "sweep"], capture_output=True, text=True)
    print(run.stdout + run.stderr)
    assert run.returncode == 0, run.stdout[-6000:] + run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert lines[-1] == "0 failures"
    rows = [row for row in lines[1:-1] if not row.startswith("FAIL")]
    assert len(rows) == 44 * 3 and {row.split()[0] for row in rows} == {"k2b_" + e for e in T.ENTRIES}
