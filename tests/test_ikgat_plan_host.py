"""The IK-GAT set-up (csrc/k2b_ikgat_plan.h) without a GPU: the stand-alone program ``tests/host/ikgat_plan_check.cpp`` includes
the header alone, packs the weight image of every net of the shape sweep of DESIGN.md 4.8 and holds it, the graph, the LDS map and
the launch to expectations written out independently.  Here its figures are compared with the recordings: the image and graph
hashes with ``tests/golden/ikgat_plan_parent.json`` (the packing code of the commit before the header existed, compiled into a
scratch program over the same nets and the same integer weights), the refusals with ``tests/golden/ikgat_refusals.json`` (that
commit's library), the caller's layout with ``core/estimators/ikgat.py``.  Built with the address and undefined-behaviour
sanitizers, as ``tests/test_fit_rules_host.py``; nothing is loaded into Python."""
import json
import shutil
import subprocess
from pathlib import Path

import pytest
import torch

from keypoints2body_amd import native, synthetic
from keypoints2body_amd.core.estimators import ikgat
from tests import ikgat_cases as T

REPO = Path(__file__).resolve().parents[1]
CSRC = REPO / "keypoints2body_amd" / "csrc"
PARENT = json.loads((REPO / "tests" / "golden" / "ikgat_plan_parent.json").read_text())
REFUSALS = json.loads((REPO / "tests" / "golden" / "ikgat_refusals.json").read_text())


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
    exe = tmp_path_factory.mktemp("ikgat_plan") / "ikgat_plan_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", str(CSRC),
                    str(REPO / "tests" / "host" / "ikgat_plan_check.cpp"), "-o", str(exe)], check=True)
    return exe


@pytest.fixture(scope="module")
def sweep(program):
    run = subprocess.run([str(program), "sweep"], capture_output=True, text=True)
    print(run.stdout + run.stderr)
    assert run.returncode == 0, run.stdout[-6000:] + run.stderr[-4000:]
    return run.stdout.splitlines()


def test_image_graph_lds_map_and_launch_meet_the_independent_expectations(sweep):
    assert sweep[-1] == "0 failures"
    assert sweep[-5:-1] == ["image and graph: ok", "values worked by hand: ok", "LDS map: ok", "launch: ok"]


def test_image_and_graph_are_the_parents_bit_for_bit(sweep):
    got = {}
    for row in sweep:
        if row.startswith("case "):
            t = row.split()
            got[t[1]] = dict(dims=[int(x) for x in t[2:7]], nedges=int(t[7]), LDX=int(t[8]), KC=int(t[9]), F=int(t[10]),
                             image_fnv1a64=t[11], csr_fnv1a64=t[12])
    assert list(got) == list(PARENT)
    wrong = {k: (got[k], PARENT[k]) for k in PARENT if got[k] != PARENT[k]}
    assert not wrong, wrong
    # the sweep of DESIGN.md 4.8 is all there
    dims = {tuple(v["dims"]) for v in PARENT.values()}
    assert {(2, 9, 16, 1, 16), (64, 9, 256, 8, 8), (22, 9, 192, 3, 192), (1, 3, 16, 1, 1), (22, 9, 128, 3, 4), (24, 9, 48, 3, 3),
            (64, 9, 256, 2, 8)} <= dims and {144, 192, 208, 256} <= {d[2] for d in dims}
    assert PARENT["default"]["F"] == 2 and PARENT["J64_H256_L2"]["F"] == 1 and PARENT["J2_H16_h16"]["F"] == 16


def test_callers_layout_is_the_one_python_packs(program):
    for row in PARENT.values():
        J, IN, H, L, NH = row["dims"]
        run = subprocess.run([str(program), "layout", str(J), str(IN), str(H), str(L)], capture_output=True, text=True)
        assert run.returncode == 0, run.stdout + run.stderr
        *segments, total = run.stdout.splitlines()
        spec = T.spec(J, IN, H, L, NH)
        shapes = ikgat.expected_shapes(spec)
        assert len(segments) == len(shapes)
        for line, (key, shape) in zip(segments, shapes.items()):
            name, layer, rows, cols = line.split()
            assert name.replace(".l.", f".{layer}.") == key, (line, key)
            size = 1
            for s in shape:
                size *= s
            assert int(rows) * int(cols) == size and (len(shape) != 2 or (int(rows), int(cols)) == shape), (line, key, shape)
        state = {k: torch.from_numpy(v) for k, v in synthetic.make_ikgat_state(J, IN, H, L, NH).items()}
        assert total == f"total {ikgat.pack_state(state, spec).size}"
    assert PARENT["default"]["dims"] == [22, 9, 128, 3, 4]      # whose total tests/test_ikgat_host.py pins at 65222


def test_the_table_and_the_recording_name_the_same_rows():
    assert [c["id"] for c in T.CREATE_CASES] == list(REFUSALS["create"])
    assert T.PREDICT_CASES == list(REFUSALS["predict"])
    for id, row in REFUSALS["create"].items():
        assert (row["code"] == native.K2B_OK) == (id == "accepted"), row
        assert row["code"] in (native.K2B_OK, native.K2B_ERR_INVALID_ARGUMENT, native.K2B_ERR_UNSUPPORTED) and bool(row["message"]) == (id != "accepted")


def test_the_header_refuses_what_the_entry_was_recorded_to_refuse(program, tmp_path):
    lines = tmp_path / "cases.txt"
    lines.write_text("".join(T.host_line(c) + "\n" for c in T.CREATE_CASES))
    run = subprocess.run([str(program), "refusals", str(lines)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    got = {}
    for row in run.stdout.splitlines():
        id, code, message = row.split("\t", 2)
        got[id] = {"code": int(code), "message": message}
    assert got == REFUSALS["create"]


def test_the_entry_refuses_what_it_was_recorded_to_refuse():
    """Every create refusal comes before the device query; the accepted row then finds a device or says that there is none."""
    for case in T.CREATE_CASES:
        code, message = T.run_create(case)
        if case["id"] == "accepted":
            assert (code, message) in ((native.K2B_OK, ""), (native.K2B_ERR_NO_DEVICE, "k2b_ikgat_create: no HIP device visible (this engine has no CPU path)"))
        else:
            assert {"code": code, "message": message} == REFUSALS["create"][case["id"]], case["id"]
