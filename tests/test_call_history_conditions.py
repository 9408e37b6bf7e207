"""No GPU: the sizes of the call-history tests (``tests/call_history_common.py``) against the plan headers and their restatements,
so that a pass of ``tests/test_gpu_call_history.py`` means what DESIGN.md 4.4e says it means."""
import pytest

from tests import call_history_common as C
from tests import fit_gradient_common as F
from tests import isolation_common as I
from tests import lbs_layouts_common as L


def test_the_lbs_batches_address_the_workspace_with_different_row_strides():
    """5, 133, 40 and 200 frames pad to pairwise different row counts; the polluter spans two 128-frame groups; 40 fits inside
    the buffer the polluter grew, 200 does not, and the reserve is beyond all of them."""
    pad = {B: C.lbs_frames_padded(B) for B in set(C.LBS_SEQUENCE)}
    assert pad == {5: 32, 133: 160, 40: 64, 200: 224}
    assert len(set(pad.values())) == len(pad)
    assert C.LBS_POLLUTER > 128 and pad[C.LBS_X] < pad[C.LBS_STRIDE] < pad[C.LBS_POLLUTER] < pad[C.LBS_REGROW] < C.lbs_frames_padded(C.LBS_RESERVE)
    assert C.LBS_SEQUENCE[0] == C.LBS_SEQUENCE[2] == C.LBS_X and C.LBS_SEQUENCE[1] == C.LBS_POLLUTER


def test_one_lbs_layout_per_route():
    routes = {name: L.expected_route(J, NB)[2] for name, (J, NB, _, _) in C.LBS_ROUTES.items()}
    assert routes == {name: route for name, (_, _, _, route) in C.LBS_ROUTES.items()}
    assert set(routes.values()) == {r for _, _, _, _, r in L.TABLE}
    assert all((J, NB) in L.LAYOUTS for J, NB, _, _ in C.LBS_ROUTES.values())
    J, NB, _, _ = C.LBS_ROUTES["stream_xw"]
    assert 25 <= NB <= 32                                            # the wide stream kernel by its coefficient count


def test_every_polluter_batch_exceeds_its_x():
    assert C.LBS_POLLUTER > C.LBS_X and C.BACKWARD_POLLUTER > C.BACKWARD_X and C.ADAM_POLLUTER > C.ADAM_X
    assert C.SURFACE_POLLUTER > C.SURFACE_X and C.CHAIN_POLLUTER > C.CHAIN_X and min(C.RAGGED_POLLUTERS) > C.CHAIN_X
    assert C.RAGGED_POLLUTERS[0] < C.RAGGED_POLLUTERS[1]             # the staging grows twice
    assert C.ADAM_ITERS_OTHER > C.ADAM_ITERS and C.LBFGS_OTHER["max_iter"] > C.LBFGS["max_iter"]
    # iteration n >= 2 pushes pair n - 1: max_iter leaves room to wrap the ring (measured on the device by the GPU tests), the
    # follow-up frames of a chain (max_iter // 2) to fill it
    assert C.LBFGS_OTHER["history_size"] + 2 <= C.LBFGS_OTHER["max_iter"] // 2, "the polluter's history ring cannot wrap"
    assert C.LBFGS["max_iter"] < 100                                 # X: most of its (max_iter-cut) history is never written
    for cus in I.HOST_CU_COUNTS:
        for name in C.LBFGS_CASES:
            n, big = C.lbfgs_sizes(name, cus)
            assert big > n == I.CASE[name].frames(cus)
        for name in C.SHARED_CHAIN_CASES:
            n, big = C.chain_sizes(name, cus)
            assert big > n == I.CASE[name].frames(cus)


@pytest.mark.parametrize("cus", I.HOST_CU_COUNTS)
def test_x_batches_where_frames_share_a_workgroup(cus):
    """The fused kernel's forced shapes at 5 frames, the L-BFGS schemes and ``isolation_common``'s tree and chain cases put several
    frames (sequences) into one workgroup.  (The tree kernel at 5 frames and a chain of three sequences run one per workgroup by
    the same rules, which is why the cases at 4 CUs + 3 frames and 4 / 2 CUs + 1 sequences stand beside them.)"""
    for kind, shapes in C.ADAM_KINDS.items():
        for shape in shapes:
            if F.layout(kind).kernel == "fused" and shape:
                W, _ = I.workgroup_frames(C.adam_launch_case(kind, shape, C.ADAM_X), cus)
                assert W >= 2, (kind, shape, W)
    for name in C.LBFGS_CASES + C.SHARED_CHAIN_CASES + ("tree/smplx20/plain", "tree/smplx20/comp_waves"):
        lc = I.CASE[name]
        assert I.workgroup_frames(lc, cus)[0] >= 2, name
        if name.startswith("lbfgs"):
            assert I.lbfgs_scheme(lc, cus) == lc.scheme
    assert I.workgroup_frames(C.adam_launch_case("smplx20", 1, C.ADAM_X), cus)[0] == 1


def test_the_filler_selections_exceed_the_cache():
    size = C.surface_cache_size()
    J, NB = L.LANDMARK_LAYOUT
    nl = L.landmarks(J, L.V_SMALL)[0].shape[0]
    keep = (J + 1, J + L.NUM_EXTRA + 2)
    schedule = C.cache_schedule(size)
    (evicting,), (before, after) = schedule["evicted"], schedule["kept"]
    # "evicted": S0 and the fillers are more tables than the cache holds, and S0 is the oldest: it leaves
    assert evicting >= size
    # "kept": behind the touch S0 is the most recent of 1 + before tables; `after` more distinct ones evict the oldest
    # 1 + before + after - size of them, which must be at least one and at most the `before` fillers in front of S0
    evictions = 1 + before + after - size
    assert after <= size - 1 < before + after and 1 <= evictions <= before, (before, after, size)
    need = max(evicting, before + after)
    sel = C.filler_selections(J, L.NUM_EXTRA, nl, need, keep)
    assert size >= 2 and len(sel) == need and len(set(sel)) == need
    assert keep not in sel and tuple(reversed(keep)) not in sel
    assert all(J <= e < J + L.NUM_EXTRA <= l < J + L.NUM_EXTRA + nl for e, l in sel)       # a landmark in each: the cached route


def test_inputs_build_without_a_device():
    x = C.fit_case("smpl10", C.ADAM_X)
    bad = C.poison_all(C.fit_case("smpl10", C.ADAM_POLLUTER))
    other = C.fit_case("smpl10", C.ADAM_POLLUTER, seed=C.SEED_OTHER)
    assert x.frames == C.ADAM_X and bad.frames == other.frames == C.ADAM_POLLUTER
    import numpy as np
    assert not np.isfinite(bad.j3d).all(axis=(1, 2)).any() and not np.isfinite(bad.tr).all(axis=1).any() and not np.isfinite(bad.pose).all(axis=1).any()
    assert np.isfinite(other.j3d).all() and not np.array_equal(other.j3d[:C.ADAM_X], x.j3d)
    p = C.poison_all_lbs(L.params(23, 10, "benign", C.LBS_POLLUTER))
    assert all(not np.isfinite(a).all(axis=1).any() for a in p)
