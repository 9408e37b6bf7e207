"""GPU: a bad frame stays in its own frame (``include/k2b.h``, Conventions; ``tests/isolation_common.py``).

Every test is a pair of calls with the same batch, positions and config - one clean, one with a few frames carrying a NaN or an
infinity in one input - at batch sizes (functions of the CU count, planned by ``isolation_common.workgroup_frames`` and pinned to
``csrc/k2b_launch_plan.h`` by ``tests/test_isolation_host.py``) at which frames really share a wave, a workgroup, an MFMA tile.  The
gates are exact: every tensor of every clean frame is bit-equal between the two calls; every poisoned frame reports a non-finite
loss, or is non-finite wherever the float64 oracle of that frame is.  Three iterations (four of L-BFGS) are enough: a leak needs
one."""
import numpy as np
import pytest
import torch

from keypoints2body_amd import native, synthetic
from tests import fit_gradient_common as F
from tests import helpers as H
from tests import isolation_common as I
from tests import lbs_layouts_common as L

pytestmark = pytest.mark.gpu
ITERS = 3
LBFGS = dict(max_iter=4, lr=1.0)
VARIANTS = ("body", "tail")


def _cus() -> int:
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- k2b_fit_world -----------------------------------------------------------------------------------------------------------
def _fit_inputs(case: F.Case):
    dev = lambda a: None if a is None else H.cuda(a)
    return dict(j3d=dev(case.j3d), conf=dev(case.conf), params=[dev(a) for a in (case.go, case.pose, case.shape, case.tr)],
                preserve=dev(case.preserve), tr_target=dev(case.tr_target))


def _adam_config(case: F.Case, launch_shape: int, evaluate: bool):
    cfg = F.fit_config(case, launch_shape)                       # (one evaluate-only closure)
    if not evaluate:
        cfg.num_iters, cfg.step_size = ITERS, native.default_fit_config().step_size
    return cfg


def run_fit(case: F.Case, launch_shape: int, evaluate: bool = False) -> dict:
    a = _fit_inputs(case)
    out = native.fit_world(F.native_model(case.kind), H.native_prior(), _adam_config(case, launch_shape, evaluate), list(case.idx), a["j3d"],
                           a["conf"], *a["params"], preserve_pose=a["preserve"], want_grad=evaluate, transl_prior_target=a["tr_target"])
    torch.cuda.synchronize()
    return out


def run_lbfgs(case: F.Case) -> dict:
    a = _fit_inputs(case)
    out = native.fit_world_lbfgs(F.native_model(case.kind), H.native_prior(), F.fit_config(case), list(case.idx), a["j3d"], a["conf"], *a["params"],
                                 preserve_pose=a["preserve"], transl_prior_target=a["tr_target"], tolerance_grad=0.0, tolerance_change=0.0, **LBFGS)
    torch.cuda.synchronize()
    return out


_clean = {}


def _clean_result(key, make):
    """The clean call of a case, made once and shared by the poison kinds (never written to)."""
    if key not in _clean:
        _clean[key] = make()
    return _clean[key]


def _check_fit(lc: I.LaunchCase, poison: str, evaluate: bool, run, what: str):
    cus = _cus()
    case = I.fit_case(lc.kind, lc.frames(cus), mask=11 if evaluate else 15)          # evaluate-only: the betas outside the optimiser
    clean = _clean_result((what, evaluate), lambda: run(case))
    for k, v in clean.items():
        assert torch.isfinite(v).all(), (what, k)
    for variant in VARIANTS:
        pos = I.case_positions(lc, cus, variant)
        bad = I.poison_fit_case(case, poison, pos.frames)
        out = run(bad)
        need = I.fit_oracle_masks(bad, pos.frames) if evaluate else I.loss_nonfinite(len(pos.frames))
        I.assert_isolated(clean, out, pos.frames, need, f"{what} {poison} {variant} W={pos.W} frames {pos.frames}")
        if evaluate:
            assert bool((out["grad"][:, torch.as_tensor(F.excluded_columns(case))] == 0.0).all()), f"{what} {poison}: a group outside the optimiser has a gradient"


@pytest.mark.parametrize("poison", I.FIT_POISONS)
@pytest.mark.parametrize("shape", (1, 2, 3, 4), ids=lambda s: I.FUSED_SHAPE_NAMES[s])
def test_fused_kernel_adam_keeps_a_bad_frame_to_itself(shape, poison):
    """2 capacity + 1 frames in the forced shape: two full workgroups (4, 8, 16, 16 slots) and a lone frame whose wave partner
    reads strips nobody wrote.  Three Adam iterations, then evaluate-only, where the gradient must be non-finite wherever the
    float64 autograd gradient of that frame is, and the betas (outside the optimiser) keep an exactly zero gradient."""
    lc = I.CASE[f"fused/{I.FUSED_SHAPE_NAMES[shape]}"]
    for evaluate in (False, True):
        _check_fit(lc, poison, evaluate, lambda c: run_fit(c, shape, evaluate), lc.name)


@pytest.mark.parametrize("poison", I.FIT_POISONS)
@pytest.mark.parametrize("shape", (1, 2), ids=("plain", "comp_waves"))
@pytest.mark.parametrize("kind", ("smplx20", "smplx32", "tree21"))
def test_tree_kernel_adam_keeps_a_bad_frame_to_itself(kind, shape, poison):
    """4 CUs + 3 frames: five frame waves per workgroup (plain), resp. four plus the component waves that take the mixture off
    all four of them."""
    lc = I.CASE[f"tree/{kind}/{'plain' if shape == 1 else 'comp_waves'}"]
    _check_fit(lc, poison, False, lambda c: run_fit(c, shape), lc.name)


@pytest.mark.parametrize("poison", I.FIT_POISONS)
@pytest.mark.parametrize("name", ("lbfgs/persistent", "lbfgs/fused_rounds", "lbfgs/two_launches", "lbfgs/wide"))
def test_device_lbfgs_keeps_a_bad_frame_to_itself(name, poison):
    """2 / 3 / 5 CUs - 1 frames: the optimisers of a workgroup's two frames on its idle waves (persistent), the step as a prologue
    of a four-frame workgroup (fused rounds), the step kernel of its own (two launches; on smplx32, P = 200, the wide one).  The
    loss of a poisoned frame is a fresh evaluation at its result: non-finite."""
    lc = I.CASE[name]
    assert I.lbfgs_scheme(lc, _cus()) == lc.scheme
    _check_fit(lc, poison, False, run_lbfgs, lc.name)


# ---- chains ------------------------------------------------------------------------------------------------------------------
def _chain_config(case: F.Case, launch_shape: int):
    cfg = _adam_config(case, launch_shape, False)
    cfg.transl_prior_weight = 0.0                                # (not built into a chain)
    return cfg


def _chain_start(case: F.Case, first_rows):
    return [H.cuda(a[first_rows]) for a in (case.go, case.pose, case.shape, case.tr)]


@pytest.mark.parametrize("name", ("chain/fused", "chain/tree"))
def test_fit_sequence_poison_stays_in_its_sequence_and_does_not_travel_back(name):
    """4 CUs + 1 sequences of three frames, four chain slots per workgroup; ``j3d`` of frame 1 of a few sequences is NaN.  Every
    other sequence and frame 0 of the poisoned ones are bit-equal; their frames 1 and 2 report a non-finite loss."""
    lc, cus, T = I.CASE[name], _cus(), I.CHAIN_FRAMES
    S = lc.frames(cus)
    case = I.fit_case(lc.kind, S * T)
    K = case.j3d.shape[1]
    run = lambda j3d: native.fit_sequence(F.native_model(lc.kind), H.native_prior(), _chain_config(case, lc.shape), 2, list(case.idx),
                                          H.cuda(j3d.reshape(S, T, K, 3)), H.cuda(case.conf.reshape(S, T, K)),
                                          *_chain_start(case, np.arange(S) * T))
    clean = I.flatten_chain(run(case.j3d))
    for variant in VARIANTS:
        pos = I.case_positions(lc, cus, variant)
        first = [s * T + 1 for s in pos.frames]
        out = I.flatten_chain(run(I.poisoned(case.j3d, first, I.POISONS["j3d_nan"].element, I.NAN)))
        later = [s * T + t for s in pos.frames for t in range(1, T)]
        I.assert_isolated(clean, out, later, I.loss_nonfinite(len(later)), f"{name} {variant} sequences {pos.frames}")


@pytest.mark.parametrize("name", ("chain/fused", "chain/tree"))
def test_fit_sequences_ragged_chains_keep_a_bad_sequence_to_itself(name):
    """The same slots with ragged lengths 1 .. 3 and three empty sequences among them: the slots are the sequences with frames,
    longest first, so slot 0 is a long sequence (frame 1 poisoned) and the tail slot a sequence of one frame (that frame)."""
    lc, cus = I.CASE[name], _cus()
    slots = lc.frames(cus)
    lengths = [(3, 1, 2, 3, 2)[i % 5] for i in range(slots)]
    for at in (slots, 7, 0):
        lengths.insert(at, 0)
    S, N = len(lengths), sum(lengths)
    off = native.ragged_offsets(lengths)
    order = native.sequence_order(lengths)
    assert len(order) == slots
    case = I.fit_case(lc.kind, N)
    nonempty = [s for s in range(S) if lengths[s] > 0]
    start = np.asarray([off[s] if lengths[s] else 0 for s in range(S)])
    run = lambda j3d: native.fit_sequences(F.native_model(lc.kind), H.native_prior(), _chain_config(case, lc.shape), 2, list(case.idx), lengths,
                                           H.cuda(j3d), H.cuda(case.conf), *_chain_start(case, start))
    clean = run(case.j3d)
    assert all(torch.isfinite(v).all() for v in clean.values()) and len(nonempty) == slots
    for variant in VARIANTS:
        pos = I.case_positions(lc, cus, variant)
        seqs = [int(order[s]) for s in pos.frames]
        first = [int(off[s]) + min(1, lengths[s] - 1) for s in seqs]
        later = [f for s, a in zip(seqs, first) for f in range(a, int(off[s]) + lengths[s])]
        if variant == "tail":
            assert lengths[seqs[0]] == 1
        out = run(I.poisoned(case.j3d, first, I.POISONS["j3d_nan"].element, I.NAN))
        I.assert_isolated(clean, out, later, I.loss_nonfinite(len(later)), f"{name} ragged {variant} sequences {seqs}")


def test_fit_sequences_lbfgs_keeps_a_bad_sequence_to_itself():
    """2 CUs + 1 sequences of three frames in the persistent launch: two chain slots, each with its optimiser, per workgroup.
    The poisoned frame (frame 1) reports a non-finite loss, a fresh evaluation at its result.  Its fitted parameters are
    unspecified - the device optimiser, handed a NaN loss at its first evaluation, stops at its finite start, where
    ``torch.optim.LBFGS`` walks into NaN - and frame 2 starts from them: nothing is asserted about frame 2 (measured: a finite
    loss).  Every other sequence and frame 0 are bit-equal."""
    lc, cus, T = I.CASE["lbfgs/chain"], _cus(), I.CHAIN_FRAMES
    S = lc.frames(cus)
    case = I.fit_case(lc.kind, S * T)
    cfg = F.fit_config(case)
    cfg.transl_prior_weight = 0.0
    run = lambda j3d: native.fit_sequences_lbfgs(F.native_model(lc.kind), H.native_prior(), cfg, LBFGS["max_iter"], 2, list(case.idx), [T] * S,
                                                 H.cuda(j3d), H.cuda(case.conf), *_chain_start(case, np.arange(S) * T), lr=LBFGS["lr"],
                                                 tolerance_grad=0.0, tolerance_change=0.0)
    clean = run(case.j3d)
    for variant in VARIANTS:
        pos = I.case_positions(lc, cus, variant)
        first = [s * T + 1 for s in pos.frames]
        later = [s * T + t for s in pos.frames for t in range(1, T)]
        out = run(I.poisoned(case.j3d, first, I.POISONS["j3d_nan"].element, I.NAN))
        hit = np.asarray([f % T == 1 for f in sorted(later)])
        I.assert_isolated(clean, out, later, {"loss": hit}, f"lbfgs/chain {variant} sequences {pos.frames}")


def test_shape_pass_keeps_a_bad_sequence_to_itself():
    """Five sequences of 3, 1, 4, 2, 3 frames, one frame of sequence 2 poisoned: the other sequences' betas are bit-equal.  Nothing
    is asserted about sequence 2 (its optimiser may legitimately stop at its finite start)."""
    lengths = (3, 1, 4, 2, 3)
    N, S = sum(lengths), len(lengths)
    case = I.fit_case("smpl10", N)
    off = torch.tensor(np.concatenate(([0], np.cumsum(lengths))), dtype=torch.int32, device="cuda")
    betas = H.cuda(case.shape[:S])
    cfg = native.default_fit_config()
    run = lambda j3d: {"betas": native.shape_pass_lbfgs(F.native_model("smpl10"), H.native_prior(), cfg, off, list(case.idx), H.cuda(j3d), H.cuda(case.conf),
                                                        H.cuda(case.go), H.cuda(case.pose), H.cuda(np.ascontiguousarray(case.j3d[:, 0])), 0, betas,
                                                        tolerance_grad=0.0, tolerance_change=0.0, **LBFGS)}
    clean = run(case.j3d)
    assert torch.isfinite(clean["betas"]).all() and not torch.equal(clean["betas"], betas)
    out = run(I.poisoned(case.j3d, [5], I.POISONS["j3d_nan"].element, I.NAN))
    torch.cuda.synchronize()
    I.assert_isolated(clean, out, [2], {}, "shape pass")


# ---- the surface path --------------------------------------------------------------------------------------------------------
SURFACE_B, SURFACE_BAD = 5, 2


def _surface_fit(route: str):
    """(model, joint index, targets [B][K][3], confidences [B][K], parameters) on the landmark model: every kinematic joint and
    three extra joints (the vertex kernel's route), with `route` "landmarks" every third landmark too (the surface kernel's)."""
    J, NB = L.LANDMARK_LAYOUT
    p = L.term_params(J, NB, SURFACE_B)
    idx = list(range(J)) + [J, J + 2, J + 4]
    if route == "landmarks":
        first = J + L.NUM_EXTRA
        idx += list(range(first, first + L.landmarks(J, L.V_SMALL)[0].shape[0], 3))
    j64, _ = L._forward(J, NB, L.V_SMALL, "landmarks", p, True, True)
    K = len(idx)
    tgt = (j64[:, idx].numpy() + F.TARGET_OFFSET * synthetic.normalish(98, (SURFACE_B, K, 3), 53)).astype(np.float32)
    conf = (0.5 + synthetic.uniform(99, SURFACE_B * K, 53).reshape(SURFACE_B, K)).astype(np.float32)
    return L.native_model(J, NB, variant="landmarks"), idx, tgt, conf, p


@pytest.mark.parametrize("poison", I.FIT_POISONS)
@pytest.mark.parametrize("route", ("extras", "landmarks"))
def test_fit_world_with_surface_targets_keeps_a_bad_frame_to_itself(route, poison):
    """Five frames, three iterations of [evaluate-only fit launch, surface kernel with the Adam tail]; a target poison sits on
    the last (a surface) target."""
    model, idx, tgt, conf, p = _surface_fit(route)
    cfg = native.default_fit_config()
    cfg.num_iters, cfg.prior_pose_dims, cfg.conf_per_frame = ITERS, 63, 1

    def run(tgt, conf, p):
        out = native.fit_world(model, H.native_prior(), cfg, idx, H.cuda(tgt), H.cuda(conf), *map(H.cuda, p))
        torch.cuda.synchronize()
        return out

    clean = _clean_result(("surface fit", route), lambda: run(tgt, conf, p))
    assert all(torch.isfinite(v).all() for v in clean.values())
    ps, bad = I.POISONS[poison], [SURFACE_BAD]
    K = len(idx)
    if ps.field == "j3d":
        out = run(I.poisoned(tgt, bad, (K - 1, 1), ps.value), conf, p)
    elif ps.field == "conf":
        out = run(tgt, I.poisoned(conf, bad, (K - 1,), ps.value), p)
    else:
        out = run(tgt, conf, I.poison_lbs_params(p, poison, bad))
    I.assert_isolated(clean, out, bad, I.loss_nonfinite(1), f"surface fit {route} {poison}")


@pytest.mark.parametrize("poison", I.TERM_POISONS)
@pytest.mark.parametrize("term", ("vertex", "surface"))
def test_stand_alone_terms_keep_a_bad_frame_to_itself(term, poison):
    case = L.vertex_term_case(24, 17, SURFACE_B) if term == "vertex" else L.surface_term_case(SURFACE_B)
    model = L.native_model(case.J, case.NB, variant=case.variant)
    entry = native.vertex_term if term == "vertex" else native.surface_term

    def run(c):
        loss, grad = entry(model, list(c.index), H.cuda(c.targets), H.cuda(c.conf), L.TERM_SIGMA, L.TERM_WEIGHT, *map(H.cuda, c.params))
        torch.cuda.synchronize()
        return {"loss": loss, "grad": grad}

    clean = run(case)
    assert all(torch.isfinite(v).all() for v in clean.values())
    bad = I.poison_term_case(case, poison, [3])
    I.assert_isolated(clean, run(bad), [3], I.term_oracle_masks(bad, [3]), f"{case.name} {poison}")


# ---- k2b_lbs, k2b_lbs_backward -----------------------------------------------------------------------------------------------
LBS_BAD = (0, 31, 36)                                            # first and last frame of the 32-frame tile, last of the five beyond


@pytest.mark.parametrize("poison", I.LBS_POISONS)
@pytest.mark.parametrize("J, NB, variant", ((24, 16, "tagged"), (23, 10, "tagged"), (55, 21, "tagged"), (56, 16, "landmarks")),
                         ids=("tile", "stream", "stream_x", "stream_xw"))
def test_lbs_keeps_a_bad_frame_to_itself(J, NB, variant, poison):
    """37 frames - one 32-frame MFMA tile and five - on each route, with vertices and joints-only.  The poisoned frames are
    non-finite wherever the float64 oracle is: a NaN in ``transl[., 0]``, say, at least in every x coordinate."""
    model = L.native_model(J, NB, variant=variant)
    p = L.params(J, NB, "benign")
    bad = I.poison_lbs_params(p, poison, LBS_BAD)
    for want_vertices in (True, False):
        def run(q):
            joints, verts = model.lbs(*map(H.cuda, q), want_vertices=want_vertices)
            torch.cuda.synchronize()
            return {"joints": joints, "vertices": verts} if want_vertices else {"joints": joints}
        clean = run(p)
        assert all(torch.isfinite(v).all() for v in clean.values())
        I.assert_isolated(clean, run(bad), LBS_BAD, I.lbs_oracle_masks(J, NB, variant, bad, LBS_BAD, want_vertices),
                          f"lbs {J}/{NB} {poison} vertices={want_vertices}")


@pytest.mark.parametrize("poison", ("pose_nan", "cot_nan"))
@pytest.mark.parametrize("J, NB", ((24, 17), (56, 32)))
def test_lbs_backward_keeps_a_bad_frame_to_itself(J, NB, poison):
    """37 frames, frame 31 poisoned: a parameter, or an entry of ``grad_vertices``."""
    B, bad = L.FRAMES, [31]
    model = L.native_model(J, NB)
    p = L.backward_params(J, NB, B)
    rng = np.random.default_rng([J, NB, 7])
    gj = rng.standard_normal((B, J + L.NUM_EXTRA, 3)).astype(np.float32)
    gv = rng.standard_normal((B, L.V_SMALL, 3)).astype(np.float32)

    def run(q, cv):
        out = model.lbs_backward(*map(H.cuda, q), H.cuda(gj), H.cuda(cv))
        torch.cuda.synchronize()
        return dict(zip(native.PARAM_KEYS, out))

    clean = run(p, gv)
    assert all(torch.isfinite(v).all() for v in clean.values())
    ps = I.POISONS[poison]
    q, cv = (p, I.poisoned(gv, bad, ps.element, ps.value)) if poison == "cot_nan" else (I.poison_lbs_params(p, poison, bad), gv)
    I.assert_isolated(clean, run(q, cv), bad, I.lbs_backward_oracle_masks(J, NB, q, gj, cv, bad), f"lbs backward {J}/{NB} {poison}")
