"""GPU: warm-start chains over the videos of a calibrated rig (``k2b_fit_multiview_sequences``, ABI 1.11).

* the in-kernel chain against the same engine driven frame by frame from the host (``k2b_fit_multiview`` per step, in the same
  forced launch shape, the preserve pose handed on): bit for bit, on the fused kernel and on both shapes of the tree kernel, with
  the follow-up shape freeze on and off, at 1, 2, 3 and 8 views;
* a sequence does not depend on its neighbours, their number or their order;
* the whole chain against ``torch.optim.Adam`` loops over ``multiview_common.frame_loss`` in float64
  (``reproj_common.trajectory_gate`` unchanged; the float32 loop's own deviation is asserted without a GPU in
  tests/test_multiview_chain_conditions.py);
* a view of confidence 0 changes nothing: the chain without that view, bit for bit;
* a non-finite keypoint stays in its own sequence;
* every refusal comes before any launch and leaves the outputs untouched;
* the outputs are fully written and nothing beside them is, and the call does not depend on what its handles served before."""
import numpy as np
import pytest
import torch

from keypoints2body_amd import native
from tests import call_history_common as CH
from tests import caller_buffers_common as CB
from tests import fit_gradient_common as G
from tests import helpers as H
from tests import multiview_chain_common as MC
from tests import reproj_chain_common as RC
from tests import reproj_common as R

pytestmark = pytest.mark.gpu

SPLIT = H.LAUNCH_SHAPES["split"]
# lengths, first iterations, follow-up iterations, confidences, view counts
FUSED_CASES = [((6,), 12, 5, "shared", (2, 8)), ((4,) * 5, 8, 3, "frame", (2, 8)), ((3,) * 301, 6, 8, "", (3,)), ((4, 0, 1, 3, 2), 7, 4, "", (3,)),
               ((3, 2), 6, 3, "", (1,))]
TREE_CASES = [((4,), 8, 3, 3), ((3,) * 9, 6, 4, 3), ((3, 1, 0, 2), 6, 4, 3), ((3, 2), 6, 3, 1)]
_lengths_id = lambda v: f"{len(v)}x{v[0]}" if len(set(v)) == 1 else "-".join(map(str, v))
FUSED = [pytest.param(lengths, first, follow, conf, C, id=f"{_lengths_id(lengths)}-C{C}") for lengths, first, follow, conf, views in FUSED_CASES for C in views]
TREE = [pytest.param(lengths, first, follow, C, id=f"{_lengths_id(lengths)}-C{C}") for lengths, first, follow, C in TREE_CASES]


def _finite(out):
    return all(bool(torch.isfinite(v).all()) for v in out.values())


@pytest.mark.parametrize("freeze", (False, True))
@pytest.mark.parametrize("lengths,first,follow,conf,C", FUSED)
@pytest.mark.parametrize("kind", R.KINDS_FUSED)
def test_fused_chain_equals_the_frame_loop_bit_for_bit(kind, lengths, first, follow, conf, C, freeze):
    c = MC.chain(kind, C, lengths, seed=len(lengths), conf=conf)
    got = MC.device_chain(c, first, follow, freeze)
    MC.assert_equal(got, MC.device_loop(c, first, follow, freeze, SPLIT), c.name)
    MC.assert_shape_held(c, got, freeze)
    assert _finite(got)


@pytest.mark.parametrize("freeze", (False, True))
@pytest.mark.parametrize("shape", (1, 2))
@pytest.mark.parametrize("lengths,first,follow,C", TREE)
@pytest.mark.parametrize("kind", R.KINDS_TREE)
def test_tree_chain_equals_the_frame_loop_bit_for_bit(kind, lengths, first, follow, C, shape, freeze):
    c = MC.chain(kind, C, lengths, seed=len(lengths))
    got = MC.device_chain(c, first, follow, freeze, launch_shape=shape)
    MC.assert_equal(got, MC.device_loop(c, first, follow, freeze, shape), f"{c.name} shape {shape}")
    MC.assert_shape_held(c, got, freeze)
    assert _finite(got)


@pytest.mark.parametrize("kind", R.BOTH)
def test_a_sequence_does_not_depend_on_its_neighbours_or_their_order(kind):
    c = MC.chain(kind, 2, (3, 1, 4, 0, 2, 4, 1), seed=7, conf="frame")
    first, follow = 6, 3
    whole = MC.device_chain(c, first, follow, True)
    alone = {}
    for s in range(len(c.lengths)):
        alone[s] = MC.device_chain(MC.select(c, [s]), first, follow, True)
        MC.assert_equal({k: v[c.rows(s)] for k, v in whole.items()}, alone[s], f"{c.name}: sequence {s} alone")
    order = [5, 3, 0, 6, 2, 1, 4]
    p = MC.select(c, order)
    mixed = MC.device_chain(p, first, follow, True)
    for i, s in enumerate(order):
        MC.assert_equal({k: v[p.rows(i)] for k, v in mixed.items()}, alone[s], f"{c.name}: sequence {s} at position {i}")


@pytest.mark.parametrize("freeze", (False, True))
@pytest.mark.parametrize("kind,C", MC.oracle_cases())
def test_the_whole_chain_matches_the_float64_oracle_chain(kind, C, freeze):
    c = MC.oracle_case(kind, C)
    ref64, ref32 = MC.oracle_chain(kind, C, freeze, True), MC.oracle_chain(kind, C, freeze, False)
    got = MC.device_chain(c, MC.ORACLE_FIRST, MC.ORACLE_FOLLOW, freeze)
    packed = torch.cat([got[k] for k in MC.KEYS], dim=1).cpu().double().numpy()
    loss = got["loss"].cpu().double().numpy()
    lay = G.layout(kind)
    for t in range(MC.ORACLE_T):
        p64, l64, g0 = ref64[t]
        R.trajectory_gate(f"{c.name}{' frozen' if freeze else ''} frame {t}", packed[t::MC.ORACLE_T], p64, ref32[t][0], g0)
        rel = np.abs(loss[t::MC.ORACLE_T] - l64) / np.abs(l64)
        print(f"loss before the last step of frame {t}: device off by {rel.max():.2e}")
        assert rel.max() <= 1e-3
    if freeze:
        s = 3 + lay.D
        held = packed[:, s:s + lay.betas_prior].reshape(MC.ORACLE_S, MC.ORACLE_T, -1)
        assert np.array_equal(held[:, 1:], np.broadcast_to(held[:, :1], held[:, 1:].shape))


@pytest.mark.parametrize("conf", ("", "frame"))
@pytest.mark.parametrize("kind", R.BOTH)
def test_a_view_of_confidence_zero_changes_nothing(kind, conf):
    """View 1 of 3 has confidence 0 everywhere and its targets CONF_OFF px off: the chain over views 0 and 2 alone, bit for bit."""
    c = MC.chain(kind, 3, (3, 1, 2), seed=37, conf=conf)
    first, follow = 6, 3
    blind = MC.device_chain(MC.blind_view(c, 1), first, follow, True)
    MC.assert_equal(blind, MC.device_chain(MC.drop_view(c, 1), first, follow, True), f"{c.name}: view 1 blind against view 1 absent")
    assert _finite(blind)


@pytest.mark.parametrize("kind", R.BOTH)
def test_a_bad_frame_stays_in_its_own_sequence(kind):
    c = MC.chain(kind, 2, (3, 3, 3), seed=29)
    first, follow = 6, 3
    clean = MC.device_chain(c, first, follow, True)
    targets = c.targets.copy()
    targets[c.rows(1)][1, 0, 4, 0] = np.nan                       # sequence 1, frame 1, view 0, one keypoint
    bad = MC.device_chain(c, first, follow, True, targets=targets)
    without = MC.device_chain(MC.select(c, [0, 2]), first, follow, True)
    for i, s in enumerate((0, 2)):
        MC.assert_equal({k: v[c.rows(s)] for k, v in bad.items()}, {k: v[3 * i:3 * i + 3] for k, v in without.items()}, f"{c.name}: sequence {s}")
        MC.assert_equal({k: v[c.rows(s)] for k, v in bad.items()}, {k: v[c.rows(s)] for k, v in clean.items()}, f"{c.name}: sequence {s} against the clean call")
    r = c.rows(1)
    MC.assert_equal({k: v[r][:1] for k, v in bad.items()}, {k: v[r][:1] for k, v in clean.items()}, f"{c.name}: frame 0 of the bad sequence")
    assert not bool(torch.isfinite(bad["loss"][r][1])), "the frame whose keypoint is NaN reports a non-finite loss"


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def _call(c, cfg, **kw):
    return lambda: MC.device_chain(c, 0, 3, True, cfg=cfg, **kw)


NAME = "k2b_fit_multiview_sequences"


def _refused(monkeypatch, exc, match, call):
    """``RC.refused`` (the exception, and every output that was handed out still holds its fill), with the code and the name: the
    wrapper raises ``ValueError`` for K2B_ERR_INVALID_ARGUMENT and ``NotImplementedError`` for K2B_ERR_UNSUPPORTED with the text
    "<entry>: <k2b_last_error>", and the library's own message starts with the entry's name."""
    RC.refused(monkeypatch, exc, rf"^{NAME}: {NAME}: .*{match}", call)
    assert native.load_library().k2b_last_error().decode().startswith(NAME + ": ")


def _spoilt(cams, view, field, slot, value):
    cams = [(Rc.copy(), tc.copy(), fc.copy()) for Rc, tc, fc in cams]
    cams[view][field].reshape(-1)[slot] = value
    return cams


@pytest.mark.parametrize("kind", R.BOTH)
def test_refusals_come_before_any_launch(kind, monkeypatch):
    c = MC.chain(kind, 2, (3, 2), seed=31)
    good = lambda: MC.config(c, 5)
    cams = list(c.base.cams)
    # (num_views = 0 cannot be said through the wrapper, which reads the view count off the keypoints: the raw call below)
    _refused(monkeypatch, ValueError, "num_views=9", _call(c, good(), cams=(cams * 5)[:9], targets=np.ascontiguousarray(np.tile(c.targets, (1, 5, 1, 1))[:, :9])))
    _refused(monkeypatch, ValueError, r"cameras\[1\].rotation\[4\]", _call(c, good(), cams=_spoilt(cams, 1, 0, 4, np.nan)))
    _refused(monkeypatch, ValueError, r"cameras\[0\].translation\[2\]", _call(c, good(), cams=_spoilt(cams, 0, 1, 2, np.inf)))
    for value in (0.0, -500.0, np.nan, np.inf):
        _refused(monkeypatch, ValueError, r"focal\[1\]", _call(c, good(), cams=_spoilt(cams, 1, 2, 1, value)))
    for projection in (0, 2):
        cfg = good()
        cfg.projection = projection
        _refused(monkeypatch, ValueError, f"projection={projection}", _call(c, cfg))
    cfg = good()
    cfg.transl_prior_weight = 1.0
    _refused(monkeypatch, ValueError, "transl_prior_weight", _call(c, cfg))
    _refused(monkeypatch, ValueError, "offsets", _call(c, good(), offsets=[0, 2]))
    for follow in (0, -3, (1 << 20) + 1):
        _refused(monkeypatch, ValueError, "followup_iters", lambda: MC.device_chain(c, 5, follow, True))
    got = MC.device_chain(c, 5, 3, True)                          # (the same call, in order, is taken)
    assert _finite(got)


@pytest.mark.parametrize("kind", R.BOTH)
def test_no_views_is_refused_with_real_handles(kind):
    """``num_views = 0`` through the library itself, on real handles and device buffers: K2B_ERR_INVALID_ARGUMENT under the entry's
    name, the outputs - pre-filled with a pattern - untouched; the same call with the rig's two views is taken and gives the
    wrapper's bits."""
    import ctypes
    c = MC.chain(kind, 2, (3, 2), seed=31)
    lib, model, prior, cfg = native.load_library(), G.native_model(kind), H.native_prior(), MC.config(c, 5)
    want = MC.device_chain(c, 5, 3, True)
    outs = {k: torch.full_like(v, RC.SENTINEL) for k, v in want.items()}
    table = native.camera_table(list(c.base.cams))
    L, O = c.lengths.astype(np.int32), c.offsets.astype(np.int32)
    idx = np.asarray(c.base.idx, dtype=np.int32)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    targets, ins = H.cuda(c.targets), MC.starts(c)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def raw(views):
        return lib.k2b_fit_multiview_sequences(model.handle, prior.handle, ctypes.byref(cfg), len(L), L.ctypes.data_as(ctypes.c_void_p),
                                               O.ctypes.data_as(ctypes.c_void_p), 3, 1, views, table, len(idx), idx.ctypes.data_as(ctypes.c_void_p),
                                               ptr(targets), None, *[ptr(t) for t in ins], *[ptr(outs[k]) for k in MC.KEYS + ("loss",)], stream)
    assert raw(0) == native.K2B_ERR_INVALID_ARGUMENT
    assert lib.k2b_last_error().decode().startswith(f"{NAME}: num_views=0 must be 1..8")
    torch.cuda.synchronize()
    assert all(bool((t == RC.SENTINEL).all()) for t in outs.values()), "a refused call wrote to its outputs"
    assert raw(2) == native.K2B_OK
    torch.cuda.synchronize()
    MC.assert_equal(outs, want, f"{c.name}: the raw call")


def test_negative_lengths_are_refused(monkeypatch):
    c = MC.chain("smpl10", 2, (3, 2), seed=31)
    bad = MC.Chain(c.name + "/neg", c.kind, c.base, c.targets, c.conf, np.asarray([6, -1], dtype=np.int32))
    _refused(monkeypatch, ValueError, r"lengths\[1\]=-1", _call(bad, MC.config(c, 5)))


def test_a_surface_target_is_refused(monkeypatch):
    kind = "smplx20"
    c = MC.chain(kind, 2, (3, 2), seed=31)
    assert G.native_model(kind).num_extra > 0
    idx = list(c.base.idx[:-1]) + [G.layout(kind).J]
    _refused(monkeypatch, NotImplementedError, "surface targets", _call(c, MC.config(c, 5), idx=idx))


def test_the_fp64_scan_twin_is_refused(monkeypatch):
    """A 24-joint model created under K2B_FIT_SCAN64=1 runs the fp64 scans, as one without a scan plan does: one fact to the rules
    (``Facts::fit_scan64``; tests/host/multiview_chain_rules_check.cpp), which the multi-view form is not built for."""
    kind = "smpl10"
    c = MC.chain(kind, 2, (3, 2), seed=31)
    k = G.consts(kind)
    monkeypatch.setenv("K2B_FIT_SCAN64", "1")
    model = native.NativeModel(k.v_template, k.shapedirs, k.posedirs, k.J_regressor, k.lbs_weights, k.parents, k.extra_vertex_ids)
    monkeypatch.delenv("K2B_FIT_SCAN64")
    _refused(monkeypatch, NotImplementedError, "fp32 scans", _call(c, MC.config(c, 5), model=model))


# ---- the caller's buffers and the call's history ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.BOTH)
def test_the_outputs_are_fully_written_and_nothing_beside_them(kind):
    """The five outputs lie in one arena between guard bands, all of it pre-filled with a NaN pattern: afterwards every element of
    every output is written (the empty sequence owns none), no guard float is, and the result is that of the plain call."""
    c = MC.chain(kind, 3, (4, 0, 1, 3, 2), seed=5, conf="frame")
    plain = MC.device_chain(c, 7, 4, True)
    arena = CB.Arena(CB.requests_like(plain), device="cuda")
    inputs = dict(targets=H.cuda(c.targets), conf=H.cuda(c.conf), **dict(zip(MC.KEYS, MC.starts(c))))
    snap = CB.snapshot(inputs)
    with native.outputs_from(arena.provider):
        got = native.fit_multiview_sequences(G.native_model(kind), H.native_prior(), MC.config(c, 7), 4, True, list(c.base.cams), list(c.base.idx),
                                             c.lengths, inputs["targets"], inputs["conf"], *[inputs[k] for k in MC.KEYS])
    torch.cuda.synchronize()
    assert sorted(arena.asked) == sorted(plain)
    for k in plain:
        assert got[k].data_ptr() == arena.views[k].data_ptr()
    arena.check(c.name)
    CB.assert_inputs_unwritten(inputs, snap, c.name)
    MC.assert_equal(got, plain, f"{c.name}: in the arena against the plain call")


@pytest.mark.parametrize("kind", R.BOTH)
def test_the_call_does_not_depend_on_the_calls_before_it(kind):
    """The same call after a larger call (more and longer sequences, more views: the slot table's pinned staging grows), after a
    refused call and after a call whose keypoints are all NaN, and on a second set of fresh handles: the bits of the first call
    on fresh handles."""
    c = MC.chain(kind, 2, (3, 1, 2), seed=13, conf="shared")
    big = MC.chain(kind, 3, (5,) * 40, seed=17)

    def refused(handles):
        cfg = MC.config(c, 6)
        cfg.projection = 0
        with pytest.raises(ValueError, match="projection=0"):
            MC.device_chain(c, 6, 3, True, cfg=cfg, model=handles[0], prior=handles[1])

    run = lambda ch, **kw: (lambda h: MC.device_chain(ch, 6, 3, True, model=h[0], prior=h[1], **kw))
    CH.run_protocol(lambda: (CH.fresh_model(kind), CH.fresh_prior()), run(c),
                    [("larger call", run(big), None),
                     ("non-finite call", run(big, targets=np.full_like(big.targets, np.nan)), CH.all_rows_nonfinite("loss", big.name))],
                    f"k2b_fit_multiview_sequences {c.name}", between=refused)
