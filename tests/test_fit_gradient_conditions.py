"""The conditions on the inputs of the fit kernels' gradient gate (tests/fit_gradient_common.py), checked on the CPU oracle alone:
float32 autograd stays within 1e-4 of float64 autograd in every group of every case, one float32 rounding of the targets moves
no group by more than an eighth of the gate, the mixture cases select every component
with a clear margin, and the odd trees sit where the tree kernel's entry draws its limits.  Also the size of every loss term's
gradient on a reference golden: what a gate scaled by the largest entry of the whole gradient cannot see."""
import numpy as np
import pytest
import torch

from tests import fit_gradient_common as F
from tests import helpers as H

CASES = {c.name: c for c in F.all_cases()}


def test_case_names_are_distinct():
    assert len(CASES) == len(F.all_cases())


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_case_meets_the_input_conditions(name):
    case = CASES[name]
    ref = F.reference(case)                       # asserts e32_k <= E32_LIMIT
    assert np.isfinite(ref.g64).all() and np.abs(ref.g64).max() > 0.0
    print(f"{name}: loss e32 {ref.e32_loss:.2e} " + " ".join(f"{k}={v:.2e}" for k, v in ref.e32.items()) +
          " | one rounding of the targets: " + " ".join(f"{k}={v:.1e}" for k, v in ref.rounding.items()))
    assert max(ref.e32.values()) <= F.E32_LIMIT and max(ref.rounding.values()) <= F.ROUNDING_LIMIT


@pytest.mark.parametrize("kind", F.BOTH + ("smplh",))
def test_mixture_cases_select_every_component_with_a_margin(kind):
    case = F.mixture_case(kind, "mixture")
    chosen, gap = F.mixture_selection(case)
    print(f"{kind}: components {chosen.tolist()}, smallest gap {gap.min():.2e} of the best value")
    assert sorted(set(chosen.tolist())) == list(range(H.gmm_fixture()["ref_means"].shape[0]))
    assert (gap > 1e-3).all()


def test_ladder_holds_every_angle_on_both_kernels():
    for kind in F.BOTH:
        c = F.ladder_case(kind)
        full = np.concatenate([c.go, c.pose], axis=1).reshape(2, -1, 3)
        angles = np.linalg.norm(full[0].astype(np.float64), axis=1)
        for a in F.LADDER:
            assert np.isclose(angles, a, rtol=1e-6, atol=1e-12).any(), (kind, a)
        assert np.isclose(angles[0], F.LADDER[0]) and not full[1].any()


@pytest.mark.parametrize("kind", F.BOTH)
def test_turn_case_meets_its_conditions(kind):
    """The root turned by 6.5 .. 5000 rad: up to 20 rad the float32 oracle stays within E32_LIMIT per frame (asserted by
    ``turn_reference``, which also says why d_f is not capped by the gate here); above it d_f dominates."""
    c = F.turn_case(kind)
    np.testing.assert_allclose(np.linalg.norm(c.go.astype(np.float64), axis=1), F.TURNS, rtol=1e-6)
    ref = F.turn_reference(kind)
    for f, a in enumerate(F.TURNS):
        print(f"{c.name} {a:g} rad: e32 loss {ref.e32_loss[f]:.2e} groups {max(v[f] for v in ref.e32.values()):.2e}; "
              f"d_f loss {ref.widen_loss[f]:.2e} groups {max(v[f] for v in ref.widen.values()):.2e}")
    assert np.isfinite(ref.g64).all() and all(np.isfinite(v).all() for v in ref.widen.values())
    assert max(v[-1] for v in ref.widen.values()) > F.GRAD_GATE             # at 5000 rad the widening is what gates


def test_gmof_case_spans_sigma_and_has_a_target_on_its_joint():
    for kind in F.BOTH:
        c = F.gmof_case(kind, "joint")
        r = np.abs(F.joints64(kind, c.go, c.pose, c.shape, c.tr) - c.j3d)
        assert r[0, 5].max() < 1e-6 and r.min() < 0.5 * F.GMOF_SIGMA and r.max() > 10 * F.GMOF_SIGMA
        assert (np.abs(r - F.GMOF_SIGMA) < 1e-6).any()


def test_confidence_cases_hold_zeros_and_values_above_one_and_differing_rows():
    for kind in F.BOTH:
        shared, table = F.conf_case(kind, False), F.conf_case(kind, True)
        assert (shared.conf == 0).any() and (shared.conf > 1).any() and shared.conf.ndim == 1
        assert (table.conf == 0).any() and (table.conf > 1).any() and not np.array_equal(table.conf[0], table.conf[1])
        assert len(F.conf_case(kind, True, removed=True).idx) == len(table.idx) - 1


def test_odd_trees_sit_at_the_entry_limits():
    joints, depth, dims = F.tree_limits_in_source()
    assert (joints, depth, dims) == (F.TREE_JOINT_LIMIT, F.TREE_DEPTH_LIMIT, F.TREE_PRIOR_LIMIT)
    assert F.tree_depth(F.TREES["tree21"]) < depth and len(F.TREES["tree21"]) != 24
    assert F.tree_depth(F.TREES["tree26"]) == depth and F.tree_depth(F.TREES["tree27"]) == depth + 1
    assert len(F.TREES["tree64"]) == joints + 1 and F.tree_depth(F.TREES["tree64"]) < depth
    for kind, parents in F.TREES.items():
        assert all(0 <= p < j for j, p in enumerate(parents) if j)
        lay = F.layout(kind)
        assert lay.prior_dims <= dims and lay.prior_dims % 3 == 0 and lay.prior_dims > 55        # the bending prior's indices


def test_term_magnitudes_on_a_reference_golden():
    """Largest gradient entry of every term alone at the start of golden ``amass_noisy_conf`` (default weights, float64 autograd;
    preserve pose 0.05 rad off, translation prior of weight 100 centred 0.1 m off per axis).  The joint term's entries are
    orders above every prior's, and the shape prior and the preserve term lie wholly below 2e-5 of the largest entry: a gate
    scaled by the whole gradient cannot see them, which is why the gate is per group and every term is also run alone."""
    from oracle.fit_torch import FitWeights, frame_losses
    d = H.load_case("amass_noisy_conf")
    t = lambda k: torch.tensor(d[k], dtype=torch.float64)
    idx = H.case_indices(d)
    model = H.oracle_model(double=True)
    rng = np.random.default_rng(0)
    off = lambda shape, size: torch.tensor(size * rng.choice([-1.0, 1.0], size=shape))
    preserve, target = t("init_body_pose") + off(d["init_body_pose"].shape, 0.05), t("init_transl") + off(d["init_transl"].shape, 0.1)
    zero = dict(pose_prior_weight=0.0, shape_prior_weight=0.0, angle_prior_weight=0.0, joint_loss_weight=0.0, pose_preserve_weight=0.0)
    terms = {"all": ({}, 100.0), "joint": (dict(zero, joint_loss_weight=600.0), 0.0), "mixture": (dict(zero, pose_prior_weight=4.78 * 1.5), 0.0),
             "bending": (dict(zero, angle_prior_weight=15.2), 0.0), "shape": (dict(zero, shape_prior_weight=5.0), 0.0),
             "preserve": (dict(zero, pose_preserve_weight=5.0), 0.0), "transl": (zero, 100.0)}
    largest = {}
    for name, (weights, w_t) in terms.items():
        go, bp, be, tr = (t(k).requires_grad_() for k in ("init_global_orient", "init_body_pose", "init_betas", "init_transl"))
        joints = model(global_orient=go, body_pose=bp, betas=be, transl=tr).joints
        lf = frame_losses(bp, preserve, be, joints[:, idx], t("j3d"), F.prior(True), t("conf"), FitWeights(**weights), True)
        lf = lf + w_t ** 2 * ((tr - target) ** 2).sum(dim=-1)
        largest[name] = float(torch.cat(torch.autograd.grad(lf.sum(), [go, bp, be, tr]), dim=1).abs().max())
    allowed = F.GRAD_GATE * largest["all"]
    print("largest gradient entry: " + " ".join(f"{k}={v:.3e}" for k, v in largest.items()) + f"; 2e-5 of the whole gradient's: {allowed:.1f}")
    assert largest["joint"] > 100.0 * max(v for k, v in largest.items() if k not in ("all", "joint"))
    assert largest["shape"] < allowed and largest["preserve"] < allowed          # invisible to a gate on the whole gradient
