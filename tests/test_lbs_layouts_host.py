"""Host (no GPU): the layout table of ``tests/lbs_layouts_common.py`` against the route rule of ``k2b_model_create`` (constants read
from the sources), the table's coverage of every branch the LBS kernels take on J and NB, the trees, and the condition on the
inputs of every forward case the GPU tests gate (float64 and float32 oracle alone)."""
import numpy as np
import pytest

from tests import lbs_layouts_common as L


def test_every_row_agrees_with_the_route_rule():
    for J, NB, feats, kx, route in L.TABLE:
        assert feats == 9 * (J - 1) + NB + 2, (J, NB)
        assert L.expected_route(J, NB) == (feats, kx, route), (J, NB, L.expected_route(J, NB))
    assert len(set(L.LAYOUTS)) == len(L.TABLE) == 17


def test_the_route_constants_are_the_ones_the_table_was_written_for():
    c = L.route_constants_in_source()
    assert c == {"kStreamKSteps": 7, "kStreamXKSteps": 16, "kStreamXWKSteps": 17, "kMaxXSteps": 34}
    # the rule reacts to each of them: one k-step more or fewer moves a row of the table
    for name in ("kStreamKSteps", "kStreamXKSteps", "kStreamXWKSteps"):
        for delta in (-1, 1):
            wrong = dict(c, **{name: c[name] + delta})
            moved = []
            for J, NB, feats, kx, route in L.TABLE:
                try:
                    moved.append(L.expected_route(J, NB, wrong) != (feats, kx, route))
                except ValueError:
                    moved.append(True)
            assert any(moved), (name, delta)
    with pytest.raises(ValueError):
        L.expected_route(56, 32, dict(c, kMaxXSteps=c["kMaxXSteps"] - 2))
    with pytest.raises(ValueError):
        L.expected_route(30, 10)


def test_the_table_covers_every_branch():
    rows = {(J, NB): (feats, kx, route) for J, NB, feats, kx, route in L.TABLE}
    small = {r[2] for (J, _), r in rows.items() if J <= 24}
    large = {r[2] for (J, _), r in rows.items() if J >= 49}
    assert small == {"tile", "stream"} and large == {"stream_x", "stream_xw"}
    feats = {r[0] for r in rows.values()}
    assert {192, 193, 224, 225, 512, 513} <= feats                     # exactly full at 32 and at 16, and one over
    assert sum(f == 512 for f, _, _ in rows.values()) >= 2             # 55 / 24 and 56 / 15
    assert {J for J, _ in rows if 9 * (J - 1) % 16 == 0} == {17, 49}   # the backward's row without a pad column
    assert (24, 16) in rows and (24, 17) in rows                       # both sides of the backward's / the vertex term's switch
    assert rows[(56, 32)][0] == 529 and max(feats) == 529              # the documented maximum
    assert rows[(49, 1)][1] == 32 and 2 * ((435 + 31) // 32) == 28     # padded up to the 16-k-step kernel
    assert rows[(56, 16)][2] == "stream_xw"                            # the wide kernel by joint count, not by 25-32 coefficients
    # pose set-up capacities: NB equal to none of 10 / 16 / 20 / 32 in both joint families, and the smallest
    assert {NB for J, NB in rows if J <= 24} >= {1, 11, 15, 17} and {NB for J, NB in rows if J >= 49} >= {1, 15, 21, 24}
    assert 23 in {J for J, _ in rows} and 56 in {J for J, _ in rows}   # an idle joint lane; no padded joint in the last group
    for sub in (L.FAR_LAYOUTS, L.STREAM_LAYOUTS, L.REPEAT_LAYOUTS, L.BACKWARD_LAYOUTS, L.BACKWARD_ALL_COTANGENTS, (L.LANDMARK_LAYOUT,)):
        assert set(sub) <= set(rows), sub
    assert len(L.STREAM_LAYOUTS) == 12
    assert rows[(23, 24)] == (224, 14, "stream")                         # capacity 32 on the e4m3 form (pose set-up <32, 3, true>), last k-step full
    assert set(L.BACKWARD_LAYOUTS) == {(17, 1), (21, 11), (24, 16), (24, 17), (49, 1), (55, 24), (56, 15), (56, 32)}


@pytest.mark.parametrize("J", sorted({J for J, _ in L.LAYOUTS} | {J for J, _ in L.EXTRA_ROUTE_LAYOUTS + L.VERTEX_TERM_LAYOUTS}))
def test_trees_are_valid(J):
    parents, rest = L.tree(J)
    assert parents.shape == (J,) and rest.shape == (J, 3) and parents[0] == -1
    assert all(0 <= parents[i] < i for i in range(1, J))
    assert len({tuple(r) for r in rest.round(6)}) == J                 # no two joints on one spot
    if J == 56:
        assert parents[55] == 20 and abs(np.linalg.norm(rest[55] - rest[20]) - 0.05) < 1e-12
    c = L.consts(J, 10)
    assert c.num_joints == J and c.num_vertices == L.V_SMALL and len(set(c.extra_vertex_ids.tolist())) == L.NUM_EXTRA


def test_model_variants():
    for J, NB in L.EXTRA_ROUTE_LAYOUTS:
        ids = L.consts(J, NB, variant="gather").extra_vertex_ids
        assert len(ids) == L.NUM_EXTRA and len(set(ids.tolist())) == L.NUM_EXTRA - 1        # one vertex named twice
        assert len(L.consts(J, NB, variant="none").extra_vertex_ids) == 0
        assert L.expected_route(J, NB)[2] in ("stream", "stream_x")                         # the tag sits in the stream kernels' W image
    ids, bary = L.landmarks(L.LANDMARK_LAYOUT[0], L.V_SMALL)
    assert ids.shape == bary.shape == (51, 3) and ids.min() >= 0 and ids.max() < L.V_SMALL
    assert all(len(set(t)) == 3 for t in ids.tolist()) and np.allclose(bary.sum(axis=1), 1.0, atol=1e-6)


def test_special_frames_are_where_the_docstring_says():
    go, pose, shape, tr = L.params(23, 10, "wide")
    full = np.concatenate([go, pose], axis=1).reshape(L.FRAMES, 23, 3).astype(np.float64)
    angle = np.sqrt((full * full).sum(axis=2))
    assert not full[1].any()
    np.testing.assert_allclose(angle[2, :8], L.F.LADDER, rtol=1e-6, atol=1e-12)
    np.testing.assert_allclose(angle[3], 2.0, rtol=1e-6)
    assert np.abs(tr).max() <= 5.0 and np.abs(L.params(23, 10, "far")[3]).max() > 25.0
    assert all(a.dtype == np.float32 for a in (go, pose, shape, tr))
    bgo, bpose, _, _ = L.backward_params(17, 1)
    assert not bgo[1].any() and not bpose[1].any()
    np.testing.assert_allclose(np.sqrt((bpose[2].reshape(-1, 3).astype(np.float64) ** 2).sum(axis=1)), 2.0, rtol=1e-6)


@pytest.mark.parametrize("J, NB, regime", L.forward_cases())
def test_forward_inputs_are_well_conditioned(J, NB, regime):
    """e32 <= a quarter of the gate (benign, wide) or 4e-6 (far), with and without the translation."""
    for with_transl in (True, False):
        ref = L.reference(J, NB, regime, with_transl=with_transl)
        print(f"{ref.name}: e32 {ref.e32.max():.3e} S {ref.scale.max():.2f}")
        L.check_inputs(ref, regime if with_transl else "benign" if regime == "benign" else "wide")
        assert np.isfinite(ref.scale).all() and (ref.tol >= L.FORWARD_GATE).all()


def test_turn_frames_are_where_the_docstring_says():
    assert L.TURNS == (6.5, 20.0, 100.0, 999.0, 1001.0, 5000.0) and set(L.TURN_LAYOUTS) <= set(L.LAYOUTS) and L.TURN_BACKWARD_LAYOUT in L.BACKWARD_LAYOUTS
    for J, NB in L.TURN_LAYOUTS:
        go, pose, shape, tr = L.params(J, NB, "turns")
        benign = L.params(J, NB, "benign")
        full = np.concatenate([go, pose], axis=1).reshape(L.FRAMES, J, 3).astype(np.float64)
        same = np.concatenate([benign[0], benign[1]], axis=1).reshape(L.FRAMES, J, 3)
        angle = np.sqrt((full * full).sum(axis=2))
        frames = L.turn_frames()
        assert sorted(frames) == list(range(4, L.TURN_FRAMES)) and L.TURN_FRAMES <= L.FRAMES
        for f in range(L.FRAMES):
            turned = dict(frames.get(f, ()))
            for joint in range(J):
                if joint in turned:
                    np.testing.assert_allclose(angle[f, joint], turned[joint], rtol=1e-6)
                else:
                    assert np.array_equal(full[f, joint].astype(np.float32), same[f, joint])
        assert np.array_equal(shape, benign[2]) and np.array_equal(tr, benign[3])
        parents, _ = L.tree(J)
        assert parents[L.TURN_CHAIN[1]] == L.TURN_CHAIN[0] and dict(frames[L.TURN_FRAMES - 1]) == {L.TURN_CHAIN[0]: 999.0, L.TURN_CHAIN[1]: 1001.0}
        assert [frames[4 + i] for i in range(6)] == [((0, a),) for a in L.TURNS]
        assert [frames[10 + i] for i in range(6)] == [((L.TURN_JOINT, a),) for a in L.TURNS]


@pytest.mark.parametrize("J, NB", L.TURN_LAYOUTS)
def test_turn_inputs_meet_their_conditions(J, NB):
    """Up to 20 rad: e32 <= 1.25e-6 (the benign limit) and d_f at most the unchanged gate, so those frames are held as sharply as
    every other frame; above it d_f dominates (the float32 oracle alone is off by micrometres at 100 rad and more beyond)."""
    ref = L.reference(J, NB, "turns")
    L.check_inputs(ref, "turns")
    angle = L.turn_angle()
    for a in sorted(set(angle[angle > 0])):
        rows = angle == a
        print(f"{ref.name} {a:g} rad: e32 {ref.e32[rows].max():.2e} d_f {ref.widen[rows].max():.2e} gate {ref.tol[rows].min():.2e}")
    assert np.isfinite(ref.widen).all() and (ref.widen[angle == 0] == 0).all()
    assert ref.widen[angle == 5000.0].max() > 10 * L.FORWARD_GATE               # there the widening is what gates


def test_backward_turn_inputs_meet_their_conditions():
    J, NB = L.TURN_BACKWARD_LAYOUT
    p, _, g64, e32, widen = L.turn_backward_reference(J, NB)                    # (asserts the conditions up to 20 rad)
    assert all(a.shape[0] == L.TURN_FRAMES and a.dtype == np.float32 for a in p)
    angle = L.turn_angle(L.TURN_FRAMES)
    for a in sorted(set(angle)):
        rows = angle == a
        print(f"backward turns {J}/{NB} {a:g} rad: e32 {e32[rows].max():.2e} d_f {max(v[rows].max() for v in widen.values()):.2e}")
    assert all(np.isfinite(v.numpy()).all() for v in g64.values()) and all(np.isfinite(v).all() for v in widen.values())


@pytest.mark.parametrize("J, NB, V", L.PRODUCT_CASES)
def test_product_size_inputs_are_well_conditioned(J, NB, V):
    ref = L.reference(J, NB, "benign", V=V, B=3)
    print(f"{ref.name}: e32 {ref.e32.max():.3e} S {ref.scale.max():.2f}")
    L.check_inputs(ref, "benign")


def test_variant_inputs_are_well_conditioned():
    for J, NB in L.EXTRA_ROUTE_LAYOUTS:
        for variant in ("gather", "none"):
            L.check_inputs(L.reference(J, NB, "wide", variant=variant), "wide")
    L.check_inputs(L.reference(*L.LANDMARK_LAYOUT, "wide", variant="landmarks"), "wide")


def test_loss_term_inputs_are_well_conditioned():
    """The float32 oracle's error and the effect of one float32 rounding of the targets, on the loss and on every gradient group."""
    for case in [L.vertex_term_case(J, NB) for J, NB in L.VERTEX_TERM_LAYOUTS] + [L.surface_term_case()]:
        r = L.term_reference(case)
        print(f"{case.name}: e32 loss {r.e32_loss:.2e} groups {max(r.e32.values()):.2e}; one rounding: loss {r.rounding_loss:.2e} groups {max(r.rounding.values()):.2e}")
        assert (case.conf == 0.0).any() and np.isfinite(r.g64).all() and (r.loss64 > 0).all()
