"""The Adam tests' oracle and the conditions on their inputs (tests/adam_common.py), without a GPU: the float64 twin against
``torch.optim.Adam`` in float64, and for every case of tests/test_gpu_adam.py that (a) torch's float32 Adam stays within a quarter of
the parameter gate of the twin and (b) one ulp on every gradient moves no end state by more than half the floor of the gate - so that
a badly chosen case cannot loosen its own gate."""
import numpy as np
import pytest
import torch

from tests import adam_common as A


@pytest.mark.parametrize("row", list(A.ROWS.values()) + list(A.TIER_B_ROWS.values()) + [A.STEP_ROWS[2]], ids=lambda r: r.name)
def test_twin_is_torch_adam_in_float64(row):
    """On the recorded gradients of the stand-alone step (zeros, 1e-20 and 1e+15 among them): parameters and both moments after
    40 steps, to float64 rounding."""
    x0, g = A.step_problem()
    x64, m64, v64 = (a[-1] for a in A.twin_on_gradients(x0, g, row))
    xt, mt, vt = A.torch_on_gradients(x0, g, row, torch.float64)
    # (x and m are sums of both signs: a few ulp of their largest addend, |x| < 1 and max |g| per element; v has one sign)
    scale = {"x": 1.0, "m": np.abs(g.astype(np.float64)).max(axis=0), "v": 0.0}
    for name, a, b in (("x", x64, xt), ("m", m64, mt), ("v", v64, vt)):
        assert (np.abs(a - b) <= 1e-13 * np.abs(b) + 1e-15 * scale[name]).all(), f"{row.name}: {name} off by {np.abs(a - b).max():.3e}"


@pytest.mark.parametrize("row", [A.ROWS["defaults"], A.ROWS["b.5_.9"], A.ROWS["eps_1e-3"]], ids=lambda r: r.name)
def test_affine_twin_is_torch_adam_in_float64(row):
    """The closed loop x <- Adam(x, g(x)) of Tier A: the twin with its analytic gradient against torch's Adam with autograd."""
    centre, start = A.block("preserve", 69)
    x64 = A.twin_affine(start, centre, 5.0, row, 37)
    xt = A.torch_affine(start, centre, 5.0, row, 37, dtype=torch.float64)
    np.testing.assert_allclose(x64, xt, rtol=0, atol=1e-12)


def test_the_long_run_has_no_bias_terms_left_in_float32():
    row = A.ROWS[A.LONG_ROW]
    t = A.LONG_ITERS // 4
    assert np.float32(1.0 - row.b1 ** t) == 1.0 and np.float32(np.sqrt(1.0 - row.b2 ** t)) == 1.0
    d = A.ROWS["defaults"]
    assert np.float32(np.sqrt(1.0 - d.b2 ** A.LONG_ITERS)) != 1.0


@pytest.mark.parametrize("term,n,row,iters", A.tier_a_cases(), ids=lambda v: str(v))
def test_tier_a_cases_meet_the_conditions(term, n, row, iters):
    ref = A.reference_a(term, n, row, iters)
    print(f"tier A {term}/{n} {row} {iters} iterations: e32 {ref.e32:.2e} floor {ref.floor:.2e} one ulp moves {ref.moved:.2e}")
    A.check_conditions(f"{term}/{n}/{row}/{iters}", ref.e32, ref.floor, ref.moved)
    centre, start = A.block(term, n, A.offsets_of(row))
    assert ref.still.sum() == A.PERIOD and (ref.x64[ref.still] == start[ref.still]).all()      # one lane per frame never moves
    lo, hi = A.offsets_of(row)
    off = np.abs(start.astype(np.float64) - centre)[~ref.still]
    assert off.min() >= 0.99 * lo and off.max() <= 1.01 * hi and (start > centre).any() and (start < centre).any()


@pytest.mark.parametrize("row", A.STEP_ROWS, ids=lambda r: r.name)
def test_step_problem_meets_the_conditions(row):
    x0, g = A.step_problem()
    assert not g[7].any() and (g == np.float32(1e-20)).any() and (g == np.float32(1e15)).any()
    assert g[3, 0] == np.float32(1e15) and g[11, 0] == np.float32(1e-20)
    ref = A.reference_step(row)
    print(f"adam step {row.name}: e32 {ref.e32:.2e} floor {ref.floor:.2e}")
    A.check_conditions(f"adam_step/{row.name}", ref.e32)
    assert ref.floor <= A.STEP_COUNT * row.lr * 4.0 * A.ULP                  # no looser than Tier A's floor
    # the moment gates can tell a lost moment from a kept one: they stay below the moment itself wherever it is not tiny
    gate_m, gate_v = A.moment_gates(row)
    big_m, big_v = np.abs(ref.m64) > 1e-30, ref.v64 > 1e-30
    assert (gate_m[big_m] < 1e-3 * np.abs(ref.m64[big_m])).mean() > 0.99 and (gate_v[big_v] < 1e-3 * ref.v64[big_v]).all()


@pytest.mark.parametrize("row", list(A.TIER_B_ROWS))
@pytest.mark.parametrize("name", A.tier_b_names())
def test_tier_b_cases_meet_the_condition(name, row):
    ref = A.reference_b(name, row)
    print(f"tier B {name} {row}: e32 {ref.e32:.2e}")
    A.check_conditions(f"{name}/{row}", ref.e32)
    assert np.isfinite(ref.x32).all() and np.isfinite(ref.loss32).all()


@pytest.mark.parametrize("name", ("vertex", "landmark"))
def test_surface_row_is_one_at_which_eps_matters(name):
    """The surface-target routes are held to the oracle at SURFACE_ROW too: the condition (a), and the oracle's own result moves by
    many gates when eps is taken for 1e-8."""
    row = A.SURFACE_ROW
    ref = A.reference_b(name, row.name)
    A.check_conditions(f"{name}/{row.name}", ref.e32)
    case = A.surface_case(name)
    other, _ = A.oracle_fit(case, A.replace(row, eps=1e-8), A.SURFACE_ITERS, False, landmarks=name == "landmark")
    assert np.abs(other - ref.x32).max() > 10 * A.PARAM_TOL


def test_default_hyper_parameters_reproduce_the_oracle_unchanged():
    """The oracle's fitters with the new keywords left out and with the defaults written out: bit for bit the same."""
    case = A.tier_b_case("smpl10", 2)
    a = A.oracle_fit(case, A.Row("d", 1e-2, 0.9, 0.999, 1e-8), 5, False)
    from oracle.fit_torch import FitWeights, fit_world_adam
    w = case.weights
    p = A.oracle_params("smpl10", case.go, case.pose, case.shape, case.tr, torch.float32)
    with A.one_thread():
        o = fit_world_adam(A.oracle_model("smpl10", False), A.F.prior(False), p["global_orient"], p["body_pose"], p["betas"], p["transl"],
                           torch.as_tensor(case.j3d), None, num_iters=5, seq_ind=1, model_idx=list(case.idx),
                           weights=FitWeights(sigma=w["sigma"], pose_prior_weight=w["mixture"], shape_prior_weight=w["shape"],
                                              angle_prior_weight=w["bending"], joint_loss_weight=w["joint"], pose_preserve_weight=w["preserve"]))
    assert np.array_equal(a[0], torch.cat([o.global_orient, o.body_pose, o.betas, o.transl], dim=1).double().numpy())
