"""No GPU: the premises of ``tests/test_gpu_caller_buffers.py`` (``tests/caller_buffers_common.py``), so that a pass there means what
DESIGN.md 4.4e says it means - the arena reports a float written directly behind, directly in front of and a full row away from an
output, its views are aligned and share nothing, the hook of ``keypoints2body_amd.native`` validates what a provider hands it, and
the batch sizes of the fused fit kernel leave half-filled slot pairs and a spilled frame under the header's own launch plans."""
import subprocess
import threading

import numpy as np
import pytest
import torch

from keypoints2body_amd import native
from tests import caller_buffers_common as A
from tests import fit_gradient_common as F
from tests import isolation_common as I
from tests.test_launch_plan_host import CSRC, REPO, _host_compiler

# a scalar-per-frame output, a row shorter than the 4 KiB floor, a row longer than it (2000 floats = 8000 bytes), a 0-d output
REQUESTS = [("loss", (5,)), ("body_pose", (5, 69)), ("grad", (3, 2000)), ("betas", (5, 10)), ("one", ())]


def _written(arena, skip=()):
    """Fill every output as an entry would (finite values), so that only the planted float is wrong."""
    for name, v in arena.outputs().items():
        if name not in skip:
            v.copy_(torch.arange(v.numel(), dtype=torch.float32).reshape(v.shape))
    return arena


def _span(arena, name):
    return next(s for s in arena.spans if s.name == name)


def test_an_untouched_arena_passes_once_every_output_is_written():
    arena = _written(A.Arena(REQUESTS))
    arena.check("clean")
    assert set(arena.outputs()) == {n for n, _ in REQUESTS}
    for name, shape in REQUESTS:
        v = arena.outputs()[name]
        assert tuple(v.shape) == tuple(shape) and v.is_contiguous() and v.dtype == torch.float32


def test_the_sentinel_is_a_quiet_nan_compared_as_bits():
    arena = A.Arena(REQUESTS)
    assert bool(torch.isnan(arena.flat).all())
    assert int(arena.bits[0]) & 0xFFFFFFFF == A.SENTINEL_BITS == 0x7FC5A5A5
    other_nan = torch.tensor([float("nan")]).view(torch.int32)
    assert int(other_nan[0]) & 0xFFFFFFFF != A.SENTINEL_BITS         # a NaN an entry computes is not the sentinel


@pytest.mark.parametrize("name", [n for n, _ in REQUESTS])
def test_a_float_directly_behind_an_output_is_reported(name):
    arena = _written(A.Arena(REQUESTS))
    arena.flat[_span(arena, name).stop] = 1.5
    with pytest.raises(AssertionError, match=rf"back guard of {name} .*offsets \+1 \.\. \+1 "):
        arena.check("planted")


@pytest.mark.parametrize("name", [n for n, _ in REQUESTS])
def test_a_float_directly_in_front_of_an_output_is_reported(name):
    arena = _written(A.Arena(REQUESTS))
    arena.flat[_span(arena, name).start - 1] = float("nan")          # a NaN of other bits than the sentinel's
    with pytest.raises(AssertionError, match=rf"front guard of {name} .*offsets -1 \.\. -1 "):
        arena.check("planted")


@pytest.mark.parametrize("name", ("body_pose", "grad", "loss"))
def test_a_float_a_full_row_away_is_reported(name):
    """The element a kernel writes when it handles one frame too many (behind) or starts one frame early (in front): the same
    column, one row of the leading index away - also where the row is longer than the 4 KiB floor."""
    shape = dict(REQUESTS)[name]
    row = int(np.prod(shape[1:], dtype=np.int64))
    for side in ("back", "front"):
        arena = _written(A.Arena(REQUESTS))
        s = _span(arena, name)
        if side == "back":
            arena.flat[s.stop - 1 + row] = 0.0
            want = rf"back guard of {name} .*offsets \+{row} \.\. \+{row} "
        else:
            arena.flat[s.start - row] = 0.0
            want = rf"front guard of {name} .*offsets -{row} \.\. -{row} "
        with pytest.raises(AssertionError, match=want):
            arena.check("planted")
    arena = _written(A.Arena(REQUESTS))
    s = _span(arena, name)
    arena.flat[s.stop:s.stop + row] = 2.0                              # the whole phantom row: first and last offsets
    with pytest.raises(AssertionError, match=rf"{row} floats of the back guard of {name} .*offsets \+1 \.\. \+{row} "):
        arena.check("planted")


def test_an_element_that_was_never_written_is_reported():
    arena = _written(A.Arena(REQUESTS), skip=("betas",))
    with pytest.raises(AssertionError, match=r"50 elements of betas .*never written.*rows 0 \.\. 4"):
        arena.check("unwritten")
    arena.check("unwritten, allowed", unwritten_ok=("betas",))
    arena = _written(A.Arena(REQUESTS))
    arena.bits[_span(arena, "body_pose").start + 4 * 69 + 68] = int(np.array(A.SENTINEL_BITS, np.uint32).view(np.int32))
    with pytest.raises(AssertionError, match=r"1 elements of body_pose .*rows 4 \.\. 4"):
        arena.check("last element of the last row")


def test_views_are_aligned_and_share_nothing_with_each_other_or_a_guard():
    spans, total = A.layout(REQUESTS)
    arena = A.Arena(REQUESTS)
    assert arena.flat.numel() == total and arena.flat.data_ptr() % A.ALIGN_BYTES == 0
    owner = np.zeros(total, dtype=np.int32)                              # how many guards / views claim each float
    for s in spans:
        n = int(np.prod(s.shape, dtype=np.int64))
        row = int(np.prod(s.shape[1:], dtype=np.int64))
        g = max(A.MIN_GUARD_BYTES // 4, row)
        assert A.guard_floats(s.shape) == g
        assert s.stop - s.start == n and (s.start * 4) % A.ALIGN_BYTES == 0
        assert s.start - s.front >= g and s.back_stop - s.stop == g     # the back guard begins at the first float behind the view
        assert 0 <= s.front <= s.start <= s.stop <= s.back_stop <= total
        v = arena.outputs()[s.name]
        assert v.data_ptr() == arena.flat.data_ptr() + 4 * s.start and v.data_ptr() % A.ALIGN_BYTES == 0
        for a, b in ((s.front, s.start), (s.start, s.stop), (s.stop, s.back_stop)):
            owner[a:b] += 1
    assert (owner == 1).all(), "a float belongs to two views or guards, or to none"
    assert [s.front for s in spans[1:]] == [s.back_stop for s in spans[:-1]] and spans[0].front == 0 and spans[-1].back_stop == total
    # every guard float is looked at
    seen = np.zeros(total, dtype=bool)
    for _, _, a, b in arena.guards():
        seen[a:b] = True
    for s in spans:
        assert not seen[s.start:s.stop].any()
        seen[s.start:s.stop] = True
    assert seen.all()


def test_inputs_are_compared_bit_for_bit_host_arrays_too():
    ins = {"j3d": torch.tensor([[1.0, float("nan"), -0.0]]), "offsets": torch.tensor([0, 3, 5], dtype=torch.int32), "idx": np.arange(4, dtype=np.int32),
           "lengths": [3, 1, 2], "conf": None}
    snap = A.snapshot(ins)
    A.assert_inputs_unwritten(ins, snap, "untouched")                   # the NaN equals itself as bits
    ins["j3d"][0, 2] = 0.0                                              # -0.0 -> +0.0: equal as floats, another bit pattern
    with pytest.raises(AssertionError, match="input j3d .*was written: 1 elements, flat offsets 2 .. 2"):
        A.assert_inputs_unwritten(ins, snap, "sign of zero")
    ins["j3d"][0, 2] = -0.0
    ins["offsets"][1] = 4
    with pytest.raises(AssertionError, match="input offsets"):
        A.assert_inputs_unwritten(ins, snap, "device index array")
    ins["offsets"][1] = 3
    ins["idx"][3] = 7
    with pytest.raises(AssertionError, match="host array idx"):
        A.assert_inputs_unwritten(ins, snap, "host index array")
    ins["idx"][3] = 3
    ins["lengths"][1] = 2
    with pytest.raises(AssertionError, match="host array lengths"):
        A.assert_inputs_unwritten(ins, snap, "host list")


# ---- the hook ------------------------------------------------------------------------------------------------------------------
CPU = torch.device("cpu")


def test_the_hook_uses_what_the_provider_hands_it_and_allocates_otherwise():
    arena = A.Arena([("loss", (4,))])
    with native.outputs_from(arena.provider):
        got = native._output("loss", (4,), CPU)
        other = native._output("grad", (4, 7), CPU)                       # the arena does not know it: allocated as before
    assert got.data_ptr() == arena.outputs()["loss"].data_ptr() and arena.asked == ["loss", "grad"]
    assert tuple(other.shape) == (4, 7) and other.dtype == torch.float32
    plain = native._output("loss", (4,), CPU)
    assert plain.data_ptr() != got.data_ptr() and arena.asked == ["loss", "grad"]      # outside the block nobody is asked


@pytest.mark.parametrize("given, match", [
    (lambda: torch.zeros(5), r"provided output loss has shape \(5,\), expected \(4,\)"),
    (lambda: torch.zeros(4, 1), r"provided output loss has shape \(4, 1\), expected \(4,\)"),
    (lambda: torch.zeros(4, dtype=torch.float64), "provided output loss must be a contiguous float32 torch tensor"),
    (lambda: torch.zeros(4, dtype=torch.int32), "provided output loss must be a contiguous float32 torch tensor"),
    (lambda: torch.zeros(8)[::2], "provided output loss must be a contiguous float32 torch tensor"),
    (lambda: np.zeros(4, np.float32), "provided output loss must be a contiguous float32 torch tensor"),
    (lambda: torch.zeros(4, device="meta"), "provided output loss is on meta, expected cpu"),
], ids=("longer", "rank", "float64", "int32", "strided", "numpy", "device"))
def test_the_hook_refuses_a_wrong_provider_tensor_before_any_launch(given, match):
    with native.outputs_from(lambda name, shape: given()):
        with pytest.raises(ValueError, match=match):
            native._output("loss", (4,), CPU)


def test_the_hook_nests_and_is_restored_on_exit_and_on_exceptions():
    a, b = torch.zeros(2), torch.ones(2)
    current = lambda: getattr(native._outputs, "provider", None)
    assert current() is None
    with native.outputs_from(lambda n, s: a):
        with native.outputs_from(lambda n, s: b):
            assert native._output("x", (2,), CPU) is b                  # the innermost provider is asked
        assert native._output("x", (2,), CPU) is a
        with native.outputs_from(None):                                 # an outer provider switched off
            assert native._output("x", (2,), CPU) is not a
        with pytest.raises(KeyError):
            with native.outputs_from(lambda n, s: b):
                raise KeyError("inside")
        assert native._output("x", (2,), CPU) is a
    assert current() is None
    with pytest.raises(ValueError):
        with native.outputs_from(lambda n, s: torch.zeros(3)):
            native._output("x", (2,), CPU)
    assert current() is None


def test_the_hook_is_per_thread():
    a = torch.zeros(2)
    seen = {}

    def worker():
        seen["inside"] = native._output("x", (2,), CPU) is a
        with native.outputs_from(lambda n, s: None):
            pass
    with native.outputs_from(lambda n, s: a):
        t = threading.Thread(target=worker)
        t.start()
        t.join()
        assert native._output("x", (2,), CPU) is a                      # the worker's block did not end this one
    assert seen == {"inside": False}


def test_every_result_of_the_binding_goes_through_the_hook():
    """``torch.empty`` appears once in ``native.py``: in the hook (the L-BFGS development state is ``torch.zeros``, an input)."""
    src = (REPO / "keypoints2body_amd" / "native.py").read_text()
    code = [line.split("#")[0] for line in src.splitlines() if "``torch.empty``" not in line]
    assert sum(line.count("torch.empty(") for line in code) == 1
    assert sum(line.count("torch.full(") + line.count("torch.empty_like(") + line.count("torch.zeros_like(") for line in code) == 0


# ---- the batch sizes of the fused fit kernel -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """``plan_fit_world`` of ``csrc/k2b_launch_plan.h`` for every forced shape, batch and CU count, printed by the stand-alone
    program of the isolation tests (built as ``tests/test_isolation_host.py`` builds it)."""
    cxx = _host_compiler()
    assert cxx is not None, "the host check needs the clang++ of the HIP toolchain that builds libk2b.so"
    exe = tmp_path_factory.mktemp("caller_buffers") / "isolation_plan"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", str(CSRC),
                    str(REPO / "tests" / "host" / "isolation_plan.cpp"), "-o", str(exe)], check=True)
    args = []
    for cus in A.HOST_CU_COUNTS:
        for shape in I.FUSED_CAPACITY:
            for B in A.FUSED_BATCHES:
                for nb in (10, 16):
                    args += [f"fused/{shape}/{B}/{nb}", "fused", str(B), str(cus), str(shape), str(nb)]
    run = subprocess.run([str(exe)] + args, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    out = {}
    for line in run.stdout.splitlines():
        name, *fields = line.split()
        row = {k: (v if k == "scheme" else int(v)) for k, v in (f.split("=") for f in fields)}
        _, shape, B, nb = name.split("/")
        out[int(shape), int(B), int(nb), row["cus"]] = row
    assert len(out) == len(args) // 6
    return out


def _workgroups(row):
    """Frames of every workgroup of a plan row."""
    W, n, grid = row["frames_per_wg"], row["frames"], row["grid"]
    assert row["launches"] == 1 and grid == -(-n // W)
    return [W] * (grid - 1) + [n - (grid - 1) * W]


@pytest.mark.parametrize("cus", A.HOST_CU_COUNTS)
def test_every_forced_shape_carries_a_partly_filled_slot_pair(plans, cus):
    """Every batch of FUSED_BATCHES is odd, so under every plan some workgroup holds an odd number of frames: in the three shapes
    that carry two frames per wave (split-paired, paired, wide) the last wave of that workgroup has one half without a frame.
    The split shape carries one frame per wave: there the partly filled unit is the workgroup (fewer frames than its four
    slots).  Held to the header's plans, and to ``isolation_common.workgroup_frames`` where that restatement applies (fewer
    frames than compute units)."""
    assert all(B % 2 == 1 for B in A.FUSED_BATCHES)
    for shape, capacity in I.FUSED_CAPACITY.items():
        partly = False
        for B in A.FUSED_BATCHES:
            for nb in (10, 16):
                row = plans[shape, B, nb, cus]
                assert row["shape"] == shape - 1 and row["frames"] == B and 1 <= row["frames_per_wg"] <= capacity, row
                wgs = _workgroups(row)
                assert sum(wgs) == B and all(1 <= w <= capacity for w in wgs)
                if B < cus:
                    W, pairs = I.workgroup_frames(I.LaunchCase("caller", "fused", "smpl10", shape, 0, B), cus)
                    assert W == row["frames_per_wg"] and pairs == (row["frames_per_wave"] == 2), (row, W, pairs)
                if row["frames_per_wave"] == 2:
                    assert shape >= 2 and any(w % 2 == 1 for w in wgs), row       # a wave with one frame on one half only
                    partly = True
                else:
                    assert shape == 1
                    partly = partly or any(w < capacity for w in wgs)
        assert partly, (shape, cus)


@pytest.mark.parametrize("cus", A.HOST_CU_COUNTS)
def test_seventeen_frames_spill_one_frame_into_a_second_workgroup(plans, cus):
    """B = 17 in the paired and the wide shape (sixteen slots): a full workgroup and one with a single frame - wherever the plan
    fills the slots, which it does with fewer frames than compute units (the devices this runs on: 256, 304) and with one compute
    unit.  At 8 compute units the same plan spreads the frames, three to a workgroup: six workgroups, every one with a half-filled
    pair, the last with two frames - still more than one workgroup and an odd one."""
    assert A.SPILL_BATCH in A.FUSED_BATCHES
    for shape in (3, 4):
        assert I.FUSED_CAPACITY[shape] == A.SPILL_BATCH - 1
        for nb in (10, 16):
            wgs = _workgroups(plans[shape, A.SPILL_BATCH, nb, cus])
            if cus > A.SPILL_BATCH or cus == 1:
                assert wgs == [16, 1], (shape, cus, wgs)
            else:
                assert len(wgs) > 1 and any(w % 2 == 1 for w in wgs), (shape, cus, wgs)
    # the two smaller batches stay in one workgroup where the slots are filled: 1 frame, and 5 (4 + 1 in the split shape)
    if cus > A.SPILL_BATCH:
        assert _workgroups(plans[1, 5, 10, cus]) == [4, 1] and _workgroups(plans[2, 5, 10, cus]) == [5] and _workgroups(plans[4, 1, 10, cus]) == [1]


@pytest.mark.parametrize("cus", [c for c in A.HOST_CU_COUNTS if c > 1])
def test_the_lbfgs_batches_land_in_the_scheme_they_name(cus):
    """The L-BFGS cases run at ``isolation_common``'s own batch (a multiple of the compute units less one: an odd, ragged batch);
    with a single compute unit those counts collapse into the persistent scheme, which is why 1 is left out here."""
    for name in ("lbfgs/persistent", "lbfgs/fused_rounds", "lbfgs/two_launches", "lbfgs/wide"):
        lc = I.CASE[name]
        assert I.lbfgs_scheme(lc, cus) == lc.scheme, (name, cus)
        assert lc.frames(cus) % cus == cus - 1
        assert F.layout(lc.kind).kernel == ("tree" if name == "lbfgs/wide" else "fused")
