"""GPU: warm-start chains under the projected joint term (``k2b_fit_image_sequences``, ABI 1.8).

* the in-kernel chain against the same engine driven frame by frame from the host (``k2b_fit_world`` with ``projection = 1``
  per step, in the same forced launch shape): bit for bit, on the fused kernel and on both shapes of the tree kernel, with the
  follow-up shape freeze on and off;
* a sequence does not depend on its neighbours, their number or their order;
* the whole chain against ``torch.optim.Adam`` loops in float64 (``reproj_common.trajectory_gate`` unchanged; the float32 loop's
  own deviation is asserted without a GPU in tests/test_reproj_chain_host.py);
* a non-finite keypoint stays in its own sequence;
* every refusal comes before any launch and leaves the outputs untouched."""
import numpy as np
import pytest
import torch

from keypoints2body_amd import native
from tests import fit_gradient_common as G
from tests import helpers as H
from tests import reproj_chain_common as RC
from tests import reproj_common as R

pytestmark = pytest.mark.gpu

SPLIT = H.LAUNCH_SHAPES["split"]
FUSED_CASES = [((6,), 12, 5, False), ((4,) * 5, 8, 3, True), ((3,) * 301, 6, 8, False), ((4, 0, 1, 3, 2), 7, 4, False)]
TREE_CASES = [((4,), 8, 3), ((3,) * 9, 6, 4), ((3, 1, 0, 2), 6, 4)]
_id = lambda v: f"{len(v)}x{v[0]}" if isinstance(v, tuple) and len(set(v)) == 1 else ("-".join(map(str, v)) if isinstance(v, tuple) else None)


@pytest.mark.parametrize("freeze", (False, True))
@pytest.mark.parametrize("lengths,first,follow,per_frame", FUSED_CASES, ids=_id)
@pytest.mark.parametrize("kind", R.KINDS_FUSED)
def test_fused_chain_equals_the_frame_loop_bit_for_bit(kind, lengths, first, follow, per_frame, freeze):
    c = RC.chain(kind, lengths, seed=len(lengths), per_frame_conf=per_frame)
    got = RC.device_chain(c, first, follow, freeze)
    RC.assert_equal(got, RC.device_loop(c, first, follow, freeze, SPLIT), c.name)
    RC.assert_shape_held(c, got, freeze)
    assert all(bool(torch.isfinite(v).all()) for v in got.values())


@pytest.mark.parametrize("freeze", (False, True))
@pytest.mark.parametrize("shape", (1, 2))
@pytest.mark.parametrize("lengths,first,follow", TREE_CASES, ids=_id)
@pytest.mark.parametrize("kind", R.KINDS_TREE)
def test_tree_chain_equals_the_frame_loop_bit_for_bit(kind, lengths, first, follow, shape, freeze):
    c = RC.chain(kind, lengths, seed=len(lengths))
    got = RC.device_chain(c, first, follow, freeze, launch_shape=shape)
    RC.assert_equal(got, RC.device_loop(c, first, follow, freeze, shape), f"{c.name} shape {shape}")
    RC.assert_shape_held(c, got, freeze)
    assert all(bool(torch.isfinite(v).all()) for v in got.values())


@pytest.mark.parametrize("kind", R.BOTH)
def test_a_sequence_does_not_depend_on_its_neighbours_or_their_order(kind):
    c = RC.chain(kind, (3, 1, 4, 0, 2, 4, 1), seed=7, per_frame_conf=True)
    first, follow = 6, 3
    whole = RC.device_chain(c, first, follow, True)
    alone = {}
    for s in range(len(c.lengths)):
        alone[s] = RC.device_chain(RC.select(c, [s]), first, follow, True)
        RC.assert_equal({k: v[c.rows(s)] for k, v in whole.items()}, alone[s], f"{c.name}: sequence {s} alone")
    order = [5, 3, 0, 6, 2, 1, 4]
    p = RC.select(c, order)
    mixed = RC.device_chain(p, first, follow, True)
    for i, s in enumerate(order):
        RC.assert_equal({k: v[p.rows(i)] for k, v in mixed.items()}, alone[s], f"{c.name}: sequence {s} at position {i}")


@pytest.mark.parametrize("freeze", (False, True))
@pytest.mark.parametrize("kind", RC.ORACLE_KINDS)
def test_the_whole_chain_matches_the_float64_oracle_chain(kind, freeze):
    c = RC.oracle_case(kind)
    ref64, ref32 = RC.oracle_chain(kind, freeze, True), RC.oracle_chain(kind, freeze, False)
    got = RC.device_chain(c, RC.ORACLE_FIRST, RC.ORACLE_FOLLOW, freeze)
    packed = torch.cat([got[k] for k in RC.KEYS], dim=1).cpu().double().numpy()
    loss = got["loss"].cpu().double().numpy()
    lay = G.layout(kind)
    for t in range(RC.ORACLE_T):
        p64, l64, g0 = ref64[t]
        R.trajectory_gate(f"{c.name}{' frozen' if freeze else ''} frame {t}", packed[t::RC.ORACLE_T], p64, ref32[t][0], g0)
        rel = np.abs(loss[t::RC.ORACLE_T] - l64) / np.abs(l64)
        print(f"loss before the last step of frame {t}: device off by {rel.max():.2e}")
        assert rel.max() <= 1e-3
    if freeze:
        s = 3 + lay.D
        held = packed[:, s:s + lay.betas_prior].reshape(RC.ORACLE_S, RC.ORACLE_T, -1)
        assert np.array_equal(held[:, 1:], np.broadcast_to(held[:, :1], held[:, 1:].shape))


@pytest.mark.parametrize("kind", R.BOTH)
def test_a_bad_frame_stays_in_its_own_sequence(kind):
    c = RC.chain(kind, (3, 3, 3), seed=29)
    first, follow = 6, 3
    clean = RC.device_chain(c, first, follow, True)
    targets = c.targets.copy()
    targets[c.rows(1)][1, 4, 0] = np.nan                          # sequence 1, frame 1, one keypoint
    bad = RC.device_chain(RC.Chain(c.name + "/nan", c.kind, c.base, targets, c.conf, c.lengths), first, follow, True)
    without = RC.device_chain(RC.select(c, [0, 2]), first, follow, True)
    for i, s in enumerate((0, 2)):
        RC.assert_equal({k: v[c.rows(s)] for k, v in bad.items()}, {k: v[3 * i:3 * i + 3] for k, v in without.items()}, f"{c.name}: sequence {s}")
    r = c.rows(1)
    RC.assert_equal({k: v[r][:1] for k, v in bad.items()}, {k: v[r][:1] for k, v in clean.items()}, f"{c.name}: frame 0 of the bad sequence")
    assert not bool(torch.isfinite(bad["loss"][r][1])), "the frame whose keypoint is NaN reports a non-finite loss"


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def _call(c, cfg, **kw):
    return lambda: RC.device_chain(c, 0, 3, True, cfg=cfg, **kw)


@pytest.mark.parametrize("kind", R.BOTH)
def test_refusals_come_before_any_launch(kind, monkeypatch):
    c = RC.chain(kind, (3, 2), seed=31)
    good = lambda: RC.config(c, 5)
    cfg = good()
    cfg.projection = 0
    RC.refused(monkeypatch, ValueError, "projection=0", _call(c, cfg))
    for focal, match in (((0.0, 500.0), r"focal\[0\]"), ((500.0, float("nan")), r"focal\[1\]"), ((float("inf"), 500.0), r"focal\[0\]")):
        cfg = good()
        cfg.focal[0], cfg.focal[1] = focal
        RC.refused(monkeypatch, ValueError, match, _call(c, cfg))
    cfg = good()
    cfg.transl_prior_weight = 1.0
    RC.refused(monkeypatch, ValueError, "transl_prior_weight", _call(c, cfg))
    RC.refused(monkeypatch, ValueError, "offsets", _call(c, good(), offsets=[0, 2]))
    RC.refused(monkeypatch, ValueError, "followup_iters", lambda: RC.device_chain(c, 5, 0, True))
    assert "k2b_fit_image_sequences" in native.load_library().k2b_last_error().decode()
    RC.device_chain(c, 5, 3, True)                                # (the same call, in order, is taken)


def test_a_surface_target_is_refused(monkeypatch):
    kind = "smplx20"
    c = RC.chain(kind, (3, 2), seed=31)
    assert G.native_model(kind).num_extra > 0
    idx = list(c.base.idx[:-1]) + [G.layout(kind).J]
    RC.refused(monkeypatch, NotImplementedError, "surface targets", _call(c, RC.config(c, 5), idx=idx))


def test_the_fp64_scan_twin_is_refused(monkeypatch):
    kind = "smpl10"
    c = RC.chain(kind, (3, 2), seed=31)
    monkeypatch.setenv("K2B_FIT_SCAN64", "1")
    k = G.consts(kind)
    model = native.NativeModel(k.v_template, k.shapedirs, k.posedirs, k.J_regressor, k.lbs_weights, k.parents, k.extra_vertex_ids)
    monkeypatch.delenv("K2B_FIT_SCAN64")
    RC.refused(monkeypatch, NotImplementedError, "fp32 scans", _call(c, RC.config(c, 5), model=model))
