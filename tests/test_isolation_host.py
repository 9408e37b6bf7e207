"""The isolation tests' own premises, without a GPU (``tests/isolation_common.py``).

Launch side: the stand-alone program ``tests/host/isolation_plan.cpp`` (includes ``csrc/k2b_launch_plan.h`` alone; built with the
address and undefined-behaviour sanitizers as ``tests/test_launch_plan_host.py`` builds its program) prints the header's plan of
every case for 64, 256 and 304 compute units.  Every case must put at least two frames (sequences) into a workgroup, have a ragged
last workgroup, land in the L-BFGS scheme it names, and ``isolation_common.workgroup_frames`` - from which the GPU tests place their
poisoned frames - must say what the header says.

Oracle side: for every model and poison kind the float64 oracle itself makes the poisoned frame non-finite and leaves the clean
one finite, so that no GPU case demands what the reference does not do; and ``assert_isolated`` raises on fabricated leaks."""
import subprocess

import numpy as np
import pytest
import torch

from tests import fit_gradient_common as F
from tests import isolation_common as I
from tests import lbs_layouts_common as L
from tests.test_launch_plan_host import CSRC, REPO, _host_compiler

FIT_KINDS = ("smpl10", "smplx20", "smplx32", "tree21")
LBS_ROUTE_LAYOUTS = ((24, 16, "tagged"), (23, 10, "tagged"), (55, 21, "tagged"), (56, 16, "landmarks"))


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    cxx = _host_compiler()
    assert cxx is not None, "the host check needs the clang++ of the HIP toolchain that builds libk2b.so"
    exe = tmp_path_factory.mktemp("isolation") / "isolation_plan"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", str(CSRC),
                    str(REPO / "tests" / "host" / "isolation_plan.cpp"), "-o", str(exe)], check=True)
    args = []
    for cus in I.HOST_CU_COUNTS:
        for c in I.CASES:
            args += [c.name, c.entry, str(c.frames(cus)), str(cus), str(c.shape), str(F.layout(c.kind).NB)]
    run = subprocess.run([str(exe)] + args, capture_output=True, text=True)
    print(run.stdout + run.stderr)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    out = {}
    for line in run.stdout.splitlines():
        name, *fields = line.split()
        row = dict(f.split("=") for f in fields)
        out[name, int(row["cus"])] = row
    assert len(out) == len(I.CASES) * len(I.HOST_CU_COUNTS)
    return out


@pytest.mark.parametrize("cus", I.HOST_CU_COUNTS)
@pytest.mark.parametrize("case", I.CASES, ids=lambda c: c.name)
def test_every_case_shares_workgroups_where_it_says(plans, case, cus):
    row = plans[case.name, cus]
    n = case.frames(cus)
    W, pairs = I.workgroup_frames(case, cus)
    assert int(row["frames"]) == n and int(row["launches"]) == 1, row
    assert int(row["frames_per_wg"]) == W >= 2, (row, W)
    assert (int(row["frames_per_wave"]) == 2) == pairs, (row, pairs)
    if case.entry == "fused":
        assert int(row["shape"]) == case.shape - 1 and W == I.FUSED_CAPACITY[case.shape] and n == 2 * W + 1, row
    if case.entry in ("tree", "chain_tree"):
        assert int(row["comp_waves"]) == (4 if case.shape == 2 else 0) and W == (4 if case.shape == 2 else 5), row
    if case.scheme:
        assert row["scheme"] == case.scheme == I.lbfgs_scheme(case, cus), row
    for variant in ("body", "tail"):
        p = I.case_positions(case, cus, variant)            # (asserts check_positions)
        assert p.grid == int(row["grid"]) and p.W == W and 1 <= p.tail < W, (variant, p, row)
        assert all(0 <= f < n for f in p.frames)
        if variant == "tail":
            assert p.frames == (n - p.tail,)
            continue
        # slot 0 (the first half of a wave pair), an odd slot (the second half), the last slot of a full workgroup
        assert [f % W for f in p.frames] == list(p.slots) and [f // W for f in p.frames] == list(p.workgroups)
        assert p.slots[0] == 0 and p.slots[-1] == W - 1 and any(s % 2 for s in p.slots)
        if W >= 6:
            assert len(p.slots) == 3 and p.slots[1] % 2 == 1 and 1 < p.slots[1] < W - 1
        clean_wgs = set(range(p.grid - 1)) - set(p.workgroups)
        assert clean_wgs, "no full workgroup is entirely clean"


def test_positions_are_refused_where_nothing_is_shared():
    with pytest.raises(AssertionError):
        I.check_positions(I.positions(1, 9, "body"), False, "body")
    with pytest.raises(AssertionError):
        I.check_positions(I.positions(4, 8, "tail"), False, "tail")              # the last workgroup is full
    with pytest.raises(AssertionError):
        I.check_positions(I.Positions((0, 1), (0, 1), (0, 0), 8, 3, 1), True, "body")   # wave partners


# ---- the oracle side -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", I.FIT_POISONS)
@pytest.mark.parametrize("kind", FIT_KINDS)
def test_float64_oracle_makes_the_poisoned_frame_non_finite(kind, poison):
    case = I.poison_fit_case(I.fit_case(kind, 3), poison, [1])
    loss, grad = F.oracle_eval(case, True)
    assert np.isfinite(loss[[0, 2]]).all() and np.isfinite(grad[[0, 2]]).all(), (kind, poison, loss)
    assert not np.isfinite(loss[1]), (kind, poison, loss)
    masks = I.fit_oracle_masks(case, [1])
    assert masks["loss"].all() and masks["grad"].any()


def test_float64_oracle_with_a_group_outside_the_optimiser():
    case = I.poison_fit_case(I.fit_case("smpl10", 3, mask=11), "j3d_nan", [1])
    masks = I.fit_oracle_masks(case, [1])
    lay = F.layout("smpl10")
    assert masks["grad"].any() and not masks["grad"][:, 3 + lay.D:3 + lay.D + lay.NB].any()


@pytest.mark.parametrize("poison", I.LBS_POISONS)
@pytest.mark.parametrize("J, NB, variant", LBS_ROUTE_LAYOUTS)
def test_float64_lbs_oracle_is_non_finite_where_the_poison_reaches(J, NB, variant, poison):
    p = I.poison_lbs_params(L.params(J, NB, "benign"), poison, [0, 31, 36])
    m = I.lbs_oracle_masks(J, NB, variant, p, [0, 1, 31, 36])
    assert not m["joints"][1].any() and not m["vertices"][1].any()               # frame 1 is clean
    for r in (0, 2, 3):
        assert m["joints"][r].any() and m["vertices"][r].any(), (poison, r)
    if poison == "transl_ninf":                                                  # transl[., 0]: at least every x coordinate
        assert m["vertices"][[0, 2, 3], :, 0].all() and m["joints"][[0, 2, 3], :, 0].all()


@pytest.mark.parametrize("poison", I.TERM_POISONS)
def test_float64_term_oracles_make_the_poisoned_frame_non_finite(poison):
    for case in (L.vertex_term_case(24, 17, 5), L.surface_term_case(5)):
        m = I.term_oracle_masks(I.poison_term_case(case, poison, [3]), [2, 3])
        assert not m["loss"][0] and not m["grad"][0].any() and m["loss"][1] and m["grad"][1].any(), (case.name, poison)


# ---- assert_isolated raises on fabricated outputs ------------------------------------------------------------------------------
def _fabricated():
    g = torch.Generator().manual_seed(5)
    clean = {"body_pose": torch.randn(9, 69, generator=g), "loss": torch.rand(9, generator=g) + 1.0}
    bad = {k: v.clone() for k, v in clean.items()}
    bad["loss"][[0, 3]] = float("nan")
    bad["body_pose"][0] = float("nan")
    bad["body_pose"][3, :5] = float("inf")
    return clean, bad


def test_assert_isolated_accepts_an_isolated_result():
    clean, bad = _fabricated()
    mask = np.zeros((2, 69), dtype=bool)
    mask[0] = True
    mask[1, :5] = True
    I.assert_isolated(clean, bad, [0, 3], dict(I.loss_nonfinite(2), body_pose=mask))


def test_assert_isolated_raises_on_one_changed_bit_in_a_clean_frame():
    clean, bad = _fabricated()
    bits = bad["body_pose"].view(torch.int32)
    bits[4, 17] ^= 1
    assert bad["body_pose"][4, 17] != clean["body_pose"][4, 17]
    with pytest.raises(AssertionError, match=r"clean frames \[4\]"):
        I.assert_isolated(clean, bad, [0, 3], I.loss_nonfinite(2))


def test_assert_isolated_raises_on_a_finite_loss_of_a_poisoned_frame():
    clean, bad = _fabricated()
    bad["loss"][3] = 2.5
    with pytest.raises(AssertionError, match="poisoned frame 3 is finite"):
        I.assert_isolated(clean, bad, [0, 3], I.loss_nonfinite(2))


def test_assert_isolated_raises_on_a_nan_in_a_clean_frame_and_on_a_missed_mask_element():
    clean, bad = _fabricated()
    both = {k: v.clone() for k, v in clean.items()}
    both["loss"][5] = float("nan")                                              # the same NaN in both calls is still a leak
    with pytest.raises(AssertionError, match=r"clean frames \[5\]"):
        I.assert_isolated(both, dict(bad, loss=torch.where(torch.isnan(both["loss"]), both["loss"], bad["loss"])), [0, 3], I.loss_nonfinite(2))
    mask = np.zeros((2, 69), dtype=bool)
    mask[1, 5] = True                                                           # element 5 of frame 3 is finite in the fabrication
    with pytest.raises(AssertionError, match="body_pose of the poisoned frame 3 is finite"):
        I.assert_isolated(clean, bad, [0, 3], {"body_pose": mask})
