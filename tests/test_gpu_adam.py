"""The Adam update of every fit path away from the default hyper-parameters, against a float64 twin of ``torch.optim.Adam`` (Tier A:
problems with an exactly known gradient) and against the oracle's fitters (Tier B: the full problem): the fused kernel in its
four launch shapes, the tree kernel in its two, the Adam tails of the vertex-term and surface-term kernels, the chain entries
with a follow-up count above and below the first, and ``k2b_adam_step`` alone; the coefficient-table cache past its 64 tables; the
refusal of an ``adam_eps`` that is no normal positive float32.  Twin, cases, references and gates: tests/adam_common.py; the
conditions on the inputs: tests/test_adam_conditions.py (no GPU)."""
import numpy as np
import pytest
import torch

from tests import adam_common as A
from tests import fit_gradient_common as F
from tests import helpers as H

pytestmark = pytest.mark.gpu

RUNS = [(r, it) for r in A.ROWS for it in A.ITERS] + [(A.LONG_ROW, A.LONG_ITERS)]
RUN_IDS = [f"{r}-{it}" for r, it in RUNS]
FUSED_SHAPES, TREE_SHAPES = (1, 2, 3, 4), (1, 2)
NON_DEFAULT = A.TIER_B_ROWS["b.8_.99_eps_1e-6"]
F_SHAPE = {1: "split", 2: "split_paired", 3: "paired", 4: "wide"}


def _cus() -> int:
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- Tier A --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row,iters", RUNS, ids=RUN_IDS)
@pytest.mark.parametrize("term", A.terms_of("smpl10"))
def test_fused_kernel_affine_gradients(term, row, iters):
    """Split, split-paired, paired and wide at 9, 17, 33 and 33 frames: each within the gate of the twin, what the term does not
    reach unchanged, and every shape bit-equal to the 33 frames of the wide one on the frames it has (second slots and the ragged
    workgroups included)."""
    a, b = A.active_columns("smpl10", term)
    ref = A.reference_a(term, b - a, row, iters)
    A.check_conditions(f"{term}/{row}/{iters}", ref.e32, ref.floor, ref.moved)
    got = {}
    for shape in FUSED_SHAPES:
        inp = A.tier_a_inputs("smpl10", term, row, A.FUSED_FRAMES[shape])
        got[shape], _ = A.fit(inp.case, A.tier_a_row(row, iters), iters, shape)
        A.gate_a(inp, ref, got[shape], f"fused/{F_SHAPE[shape]} {term} {row} {iters} iterations")
    longest = got[FUSED_SHAPES[-1]]                          # wide, 33 frames: every other call is a prefix of it
    assert all(longest.shape[0] >= g.shape[0] for g in got.values())
    for shape in FUSED_SHAPES[:-1]:
        assert torch.equal(got[shape], longest[:got[shape].shape[0]]), f"{term} {row} {iters}: {F_SHAPE[shape]} differs from wide"


@pytest.mark.parametrize("row,iters", RUNS, ids=RUN_IDS)
@pytest.mark.parametrize("term", A.terms_of("smplx20"))
@pytest.mark.parametrize("kind", A.TREE_KINDS)
def test_tree_kernel_affine_gradients(kind, term, row, iters):
    """Plain and component waves on four frames per compute unit plus three (several waves per workgroup, a ragged last one)."""
    a, b = A.active_columns(kind, term)
    ref = A.reference_a(term, b - a, row, iters)
    A.check_conditions(f"{term}/{row}/{iters}", ref.e32, ref.floor, ref.moved)
    inp = A.tier_a_inputs(kind, term, row, 4 * _cus() + 3)
    for shape in TREE_SHAPES:
        packed, _ = A.fit(inp.case, A.tier_a_row(row, iters), iters, shape)
        A.gate_a(inp, ref, packed, f"tree/{kind}/{'plain' if shape == 1 else 'comp_waves'} {term} {row} {iters} iterations")


# ---- k2b_adam_step alone -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", A.STEP_ROWS, ids=lambda r: r.name)
@pytest.mark.parametrize("n", A.STEP_SIZES)
def test_adam_step_alone_on_recorded_gradients(n, row):
    """40 consecutive steps, one of them with an all-zero gradient, entries of 1e-20 and 1e+15: both moments after every step and
    the parameters after the last against the twin.  (The row with both betas zero is the one that showed ``k2b_adam_kernel`` losing a
    gradient behind a first moment of 1e15: torch's lerp has a second form from a weight of 0.5 on)"""
    from keypoints2body_amd import native
    x0, g = A.step_problem()
    ref = A.reference_step(row)
    A.check_conditions(f"adam_step/{row.name}", ref.e32)
    gate_m, gate_v = A.moment_gates(row)
    x, m, v = H.cuda(x0[:n]), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    grads = H.cuda(g[:, :n])
    worst = {"m": 0.0, "v": 0.0}
    for t in range(A.STEP_COUNT):
        native.adam_step(x, grads[t], m, v, t + 1, row.lr, row.b1, row.b2, row.eps)
        for name, got, want, gate in (("m", m, ref.m64[t, :n], gate_m[t, :n]), ("v", v, ref.v64[t, :n], gate_v[t, :n])):
            err = np.abs(got.cpu().double().numpy() - want)
            worst[name] = max(worst[name], float((err / gate).max()))
            assert (err <= gate).all(), f"n={n} {row.name}: {name} after step {t + 1} off by {err.max():.3e} (element {int((err / gate).argmax())})"
    err = float(np.abs(x.cpu().double().numpy() - ref.x64[-1, :n]).max())
    print(f"adam gate adam_step n={n} {row.name}: deviation {err:.2e}  e32 {ref.e32:.2e}  floor {ref.floor:.2e}  gate {ref.tol:.2e}  "
          f"moments at {worst['m']:.2f} / {worst['v']:.2f} of their gates")
    assert err <= ref.tol, f"n={n} {row.name}: parameters {err:.2e} off the twin, gate {ref.tol:.2e}"


# ---- Tier B --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", list(A.TIER_B_ROWS))
def test_fused_kernel_full_problem_matches_the_oracle(row):
    """Every term on, 24 iterations: within the project's gates of ``fit_world_adam`` with the same hyper-parameters, in every
    launch shape, and the shapes bit-equal."""
    ref = A.reference_b("smpl10", row)
    A.check_conditions(f"smpl10/{row}", ref.e32)
    case = A.tier_b_case("smpl10")
    first = None
    for shape in FUSED_SHAPES:
        packed, loss = A.fit(case, A.TIER_B_ROWS[row], A.TIER_B_ITERS, shape)
        first = (packed, loss) if first is None else first
        assert torch.equal(packed, first[0]) and torch.equal(loss, first[1]), f"{row}: shape {shape} differs from shape {FUSED_SHAPES[0]}"
    A.gate_b(ref, *first, f"fused full problem {row}")


@pytest.mark.parametrize("row", list(A.TIER_B_ROWS))
def test_tree_kernel_full_problem_matches_the_oracle(row):
    ref = A.reference_b("smplx20", row)
    A.check_conditions(f"smplx20/{row}", ref.e32)
    for shape in TREE_SHAPES:
        A.gate_b(ref, *A.fit(A.tier_b_case("smplx20"), A.TIER_B_ROWS[row], A.TIER_B_ITERS, shape), f"tree/{shape} full problem {row}")


@pytest.mark.parametrize("row", list(A.B_ROWS))
@pytest.mark.parametrize("which", ("vertex", "landmark"))
def test_surface_target_tails_match_the_oracle(which, row):
    """One vertex-selected joint behind 22 kinematic targets (the Adam tail of ``k2b_vertex_term_kernel``, one launch pair per
    iteration, ``coef + it``) and one landmark (the tail of ``k2b_surface_term_kernel``): 12 iterations, also at an eps of 10, which
    is among the gradients' magnitudes."""
    ref = A.reference_b(which, row)
    A.check_conditions(f"{which}/{row}", ref.e32)
    model = A.native_landmark_model() if which == "landmark" else None
    A.gate_b(ref, *A.fit(A.surface_case(which), A.B_ROWS[row], A.SURFACE_ITERS, model=model), f"{which} tail {row}")


@pytest.mark.parametrize("counts", A.CHAIN_COUNTS, ids=lambda c: f"{c[0]}_{c[1]}")
@pytest.mark.parametrize("kind", A.CHAIN_KINDS)
def test_chains_match_the_oracles_frame_loop(kind, counts):
    """3 sequences of 4 frames with 3 first and 7 follow-up iterations (the chain's table is longer than ``num_iters``), and
    swapped: ``k2b_fit_sequence`` against the oracle's frame loop, ``k2b_fit_sequences`` bit-equal to it."""
    row = NON_DEFAULT
    ref = A.reference_b(f"chain/{kind}/{counts[0]}_{counts[1]}", row.name)
    A.check_conditions(f"chain/{kind}", ref.e32)
    one = A.fit_chain(A.chain_case(kind), row, *counts, ragged=False)
    A.gate_b(ref, *one, f"chain {kind} {counts}")
    many = A.fit_chain(A.chain_case(kind), row, *counts, ragged=True)
    assert torch.equal(one[0], many[0]) and torch.equal(one[1], many[1])


# ---- exact gates ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ragged", (False, True), ids=("fit_sequence", "fit_sequences"))
@pytest.mark.parametrize("counts", A.CHAIN_COUNTS, ids=lambda c: f"{c[0]}_{c[1]}")
@pytest.mark.parametrize("kind", A.CHAIN_KINDS)
def test_chain_with_the_preserve_term_alone_never_moves(kind, counts, ragged):
    """Frame 0 has no preserve term, so every gradient is zero and it ends where it started; every later frame preserves its
    predecessor's result and starts there: fresh optimiser state plus preserve reference, at no tolerance."""
    case = F.replace(A.chain_case(kind), weights=F.only("preserve"))
    packed, _ = A.fit_chain(case, NON_DEFAULT, *counts, ragged=ragged)
    heads = np.arange(A.CHAIN_S) * A.CHAIN_T
    start = torch.cat([H.cuda(a[heads]) for a in (case.go, case.pose, case.shape, case.tr)], dim=1)
    for t in range(A.CHAIN_T):
        assert torch.equal(packed[:, t], start), f"{kind} {counts}: frame {t} moved"


MEMBERS = [(9, 0), (2, 0), (4, 0), (8, 0), (15, 1)]


def _with_negative_zeros(case):
    go, pose, shape, tr = (a.copy() for a in (case.go, case.pose, case.shape, case.tr))
    go[0, 1], pose[0, 5], pose[1, 70 % pose.shape[1]], shape[0, 0], shape[1, 3], tr[1, 2] = (np.float32(-0.0),) * 6
    return F.replace(case, go=go, pose=pose, shape=shape, tr=tr)


EVERY_ROW = list({**A.ROWS, **A.B_ROWS}.values())             # the seven rows of Tier A, the two of Tier B, the surface routes' own


@pytest.mark.parametrize("row", EVERY_ROW, ids=lambda r: r.name)
@pytest.mark.parametrize("mask,freeze", MEMBERS)
@pytest.mark.parametrize("route", ("fused", "tree", "vertex", "landmark"))
def test_parameters_outside_the_optimiser_come_back_unchanged(route, mask, freeze, row):
    """optimize_mask 9, 2, 4, 8 and freeze_betas (SMPL-X: the first 10 of 20 coefficients) on the full problem at every
    hyper-parameter row, starts of -0.0 among them: what is outside the optimiser is ``torch.equal`` to its input, what is inside
    has moved."""
    base = {"fused": lambda: A.tier_b_case("smpl10"), "tree": lambda: A.tier_b_case("smplx20"), "vertex": lambda: A.surface_case("vertex"),
            "landmark": lambda: A.surface_case("landmark")}[route]()
    case = F.replace(_with_negative_zeros(base), mask=mask, freeze=freeze)
    model = A.native_landmark_model() if route == "landmark" else None
    shapes = {"fused": FUSED_SHAPES, "tree": TREE_SHAPES}.get(route, (0,))
    excluded = torch.as_tensor(F.excluded_columns(case))
    start = torch.cat([H.cuda(a) for a in (case.go, case.pose, case.shape, case.tr)], dim=1).cpu()
    for shape in shapes:
        packed = A.fit(case, row, 5, shape, model=model)[0].cpu()
        assert torch.isfinite(packed).all()
        assert torch.equal(packed[:, excluded], start[:, excluded]), f"{route} shape {shape} mask {mask} freeze {freeze} {row.name}: a parameter outside the optimiser moved"
        moved = (packed != start)[:, ~excluded]
        assert moved.float().mean() > 0.25, f"{route} shape {shape} mask {mask}: the optimiser's own parameters did not move"


@pytest.mark.parametrize("row", EVERY_ROW, ids=lambda r: r.name)
@pytest.mark.parametrize("mask,freeze", MEMBERS)
@pytest.mark.parametrize("ragged", (False, True), ids=("fit_sequence", "fit_sequences"))
@pytest.mark.parametrize("kind", A.CHAIN_KINDS)
def test_chains_carry_parameters_outside_the_optimiser_unchanged(kind, ragged, mask, freeze, row):
    """The same members in the chain entries (3 sequences of 4 frames, 3 + 5 iterations): a value outside the optimiser is handed
    from frame to frame, so every such column of every frame is ``torch.equal`` to the sequence's start, starts of -0.0 among
    them; what is inside has moved by the last frame."""
    base = A.chain_case(kind)
    heads = np.arange(A.CHAIN_S) * A.CHAIN_T
    go, pose, shape, tr = (a.copy() for a in (base.go, base.pose, base.shape, base.tr))
    h0, h1 = heads[0], heads[1]
    go[h0, 1], pose[h0, 5], pose[h1, 70 % pose.shape[1]], shape[h0, 0], shape[h1, 3], tr[h1, 2] = (np.float32(-0.0),) * 6
    case = F.replace(base, go=go, pose=pose, shape=shape, tr=tr, mask=mask, freeze=freeze)
    packed = A.fit_chain(case, row, 3, 5, ragged=ragged)[0].cpu()
    start = torch.cat([torch.as_tensor(a[heads]) for a in (go, pose, shape, tr)], dim=1)
    excluded = torch.as_tensor(F.excluded_columns(case))
    what = f"{kind} {'fit_sequences' if ragged else 'fit_sequence'} mask {mask} freeze {freeze} {row.name}"
    assert torch.isfinite(packed).all(), what
    for t in range(A.CHAIN_T):
        assert torch.equal(packed[:, t][:, excluded], start[:, excluded]), f"{what}: a parameter outside the optimiser moved in frame {t}"
    assert (packed[:, -1] != start)[:, ~excluded].float().mean() > 0.25, f"{what}: the optimiser's own parameters did not move"


def _fresh_model():
    from keypoints2body_amd.native import NativeModel
    c = F.consts("smpl10")
    return NativeModel(c.v_template, c.shapedirs, c.posedirs, c.J_regressor, c.lbs_weights, c.parents, c.extra_vertex_ids)


@pytest.mark.parametrize("order", ("evicted", "kept"))
def test_result_does_not_depend_on_the_coefficient_table_cache(order):
    """One model handle keeps 64 tables.  "evicted": case X, 70 one-iteration fits with 70 step sizes (X's table, the least
    recently used, leaves), X again.  "kept": X, 35 such fits, X (its table is now the most recent), 60 more (the others leave), X."""
    from keypoints2body_amd import native
    model = _fresh_model()
    inp = A.tier_a_inputs("smpl10", "preserve", NON_DEFAULT.name, 9)
    run_x = lambda: A.fit(inp.case, NON_DEFAULT, 37, model=model)[0]
    small = A.tier_a_inputs("smpl10", "preserve", NON_DEFAULT.name, 2)
    steps = iter(1e-3 * (1.0 + np.arange(200)))

    def fill(count):
        for _ in range(count):
            out, _ = A.fit(small.case, F.replace(NON_DEFAULT, lr=float(next(steps))), 1, model=model)
            assert torch.isfinite(out).all()

    first = run_x()
    if order == "evicted":
        fill(70)
    else:
        fill(35)
        assert torch.equal(run_x(), first)
        fill(60)
    assert torch.equal(run_x(), first)
    assert not torch.equal(first, torch.as_tensor(inp.x0).cuda())


# ---- the eps contract ----------------------------------------------------------------------------------------------------------
BAD_EPS = (-1e-8, float("nan"), 0.0, 1e-45)


def _adam_entries():
    """name -> call(eps): every Adam entry on a small problem."""
    from keypoints2body_amd import native

    def world(kind):
        case = A.tier_b_case(kind, 3)
        return lambda eps: A.fit(case, F.replace(NON_DEFAULT, eps=eps), 2)

    def chain(kind, ragged):
        return lambda eps: A.fit_chain(A.chain_case(kind), F.replace(NON_DEFAULT, eps=eps), 2, 2, ragged=ragged)

    def step(eps):
        x = torch.ones(5, device="cuda")
        native.adam_step(x, torch.ones_like(x), torch.zeros_like(x), torch.zeros_like(x), 1, 1e-2, 0.9, 0.999, eps)
        return x

    return {"fit_world/fused": world("smpl10"), "fit_world/tree": world("smplx20"), "fit_world/vertex": lambda eps: A.fit(
        A.surface_case("vertex"), F.replace(NON_DEFAULT, eps=eps), 2), "fit_world/landmark": lambda eps: A.fit(
        A.surface_case("landmark"), F.replace(NON_DEFAULT, eps=eps), 2, model=A.native_landmark_model()), "fit_sequence/fused": chain("smpl10", False),
        "fit_sequence/tree": chain("smplx20", False), "fit_sequences/fused": chain("smpl10", True), "fit_sequences/tree": chain("smplx20", True),
        "adam_step": step}


@pytest.mark.parametrize("eps", BAD_EPS, ids=str)
@pytest.mark.parametrize("entry", ("fit_world/fused", "fit_world/tree", "fit_world/vertex", "fit_world/landmark", "fit_sequence/fused", "fit_sequence/tree",
                                   "fit_sequences/fused", "fit_sequences/tree", "adam_step"))
def test_adam_entries_refuse_an_eps_that_is_no_normal_positive_float32(entry, eps):
    """Negative, NaN, zero and a float32 denormal: K2B_ERR_INVALID_ARGUMENT naming eps, from every Adam entry (with zero the update
    of a parameter with gradient zero would be 0 * rcp(0))."""
    with pytest.raises(ValueError, match="eps"):
        _adam_entries()[entry](eps)


def test_smallest_normal_eps_is_accepted_and_keeps_frozen_parameters():
    case = F.replace(A.tier_b_case("smpl10", 3), mask=2)
    packed = A.fit(case, F.replace(NON_DEFAULT, eps=1.2e-38), 3)[0].cpu()
    start = torch.cat([torch.as_tensor(a) for a in (case.go, case.pose, case.shape, case.tr)], dim=1)
    excluded = torch.as_tensor(F.excluded_columns(case))
    assert torch.isfinite(packed).all() and torch.equal(packed[:, excluded], start[:, excluded])


def test_lbfgs_entries_still_accept_the_default_config():
    """``k2b_fit_world_lbfgs``, ``k2b_fit_sequence_lbfgs``, ``k2b_fit_sequences_lbfgs`` and ``k2b_shape_pass_lbfgs`` take the config."""
    from keypoints2body_amd import native
    case = A.tier_b_case("smpl10", 3)
    cfg = F.fit_config(case)
    dev = [H.cuda(a) for a in (case.go, case.pose, case.shape, case.tr)]
    assert cfg.adam_eps == 1e-8
    out = native.fit_world_lbfgs(F.native_model("smpl10"), H.native_prior(), cfg, list(case.idx), H.cuda(case.j3d), None, *dev, max_iter=2, lr=1.0)
    assert torch.isfinite(out["loss"]).all()
    seq = native.fit_sequence_lbfgs(F.native_model("smpl10"), H.native_prior(), cfg, 2, 2, list(case.idx), H.cuda(case.j3d), None,
                                    *[d[:1].contiguous() for d in dev], lr=1.0)
    assert torch.isfinite(seq["loss"]).all()
    many = native.fit_sequences_lbfgs(F.native_model("smpl10"), H.native_prior(), cfg, 2, 2, list(case.idx), [2, 1], H.cuda(case.j3d), None,
                                      *[d[:2].contiguous() for d in dev], lr=1.0)
    assert torch.isfinite(many["loss"]).all()
    off = torch.tensor([0, 2, 3], dtype=torch.int32, device="cuda")
    betas = native.shape_pass_lbfgs(F.native_model("smpl10"), H.native_prior(), cfg, off, list(case.idx), H.cuda(case.j3d),
                                    torch.ones(3, len(case.idx), device="cuda"), dev[0], dev[1], H.cuda(np.ascontiguousarray(case.j3d[:, 0])), 0,
                                    dev[2][:2].contiguous(), max_iter=2, lr=1.0)
    assert torch.isfinite(betas).all()
