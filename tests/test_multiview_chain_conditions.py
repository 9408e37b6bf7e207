"""No GPU: the conditions on the inputs of the multi-view chain's oracle test, from the oracle alone.  For every chain that
tests/test_gpu_multiview_chain.py gates against the float64 ``torch.optim.Adam`` loops (3 sequences x 3 frames, 10 / 5 iterations,
C = 2 and 4, one fused and one tree kind, the follow-up freeze on and off):

* the float32 loop sits within ``reproj_chain_common.F32_LOOP_LIMIT`` (2.5e-5, a quarter of the parameter gate) of the float64
  one, so ``trajectory_gate``'s widening ``4 x deviation`` never exceeds its floor of 1e-4;
* every oracle value is finite, and the float64 gradient at every step's start - which tells ``trajectory_gate`` the entries to
  leave out (Adam's first step is lr * sign(g)) - is zero in the groups outside the optimiser and non-zero in most others;
* every camera of the rig sees every joint of every start in front of it.

A chain that leaves a limit is changed (its seed), never the limit."""
import numpy as np
import pytest

from tests import fit_gradient_common as G
from tests import multiview_chain_common as MC
from tests import multiview_common as MV
from tests import reproj_chain_common as RC


@pytest.mark.parametrize("freeze", (False, True))
@pytest.mark.parametrize("kind,C", MC.oracle_cases())
def test_the_float32_oracle_chain_stays_within_a_quarter_of_the_gate(kind, C, freeze):
    dev = MC.f32_loop_deviation(kind, C, freeze)
    print(f"{kind} C={C}{' frozen' if freeze else ''}: float32 oracle chain off the float64 one by {dev:.2e} (limit {RC.F32_LOOP_LIMIT:.1e})")
    assert dev <= RC.F32_LOOP_LIMIT


@pytest.mark.parametrize("freeze", (False, True))
@pytest.mark.parametrize("kind,C", MC.oracle_cases())
def test_every_step_is_finite_and_its_first_gradient_names_the_gated_entries(kind, C, freeze):
    c = MC.oracle_case(kind, C)
    for t, (params, loss, g0) in enumerate(MC.oracle_chain(kind, C, freeze, True)):
        case = MC.step_case(c, t, [c.base.go, c.base.pose, c.base.shape, c.base.tr], freeze, "columns")
        inside = ~G.excluded_columns(case)
        assert np.isfinite(params).all() and np.isfinite(loss).all() and np.isfinite(g0).all(), (c.name, t)
        # (a zero gradient inside the optimiser - an untargeted leaf rotation beyond the prior - takes no part in the gate and must
        #  not move; what the gate reads is that the groups outside the optimiser are zero and that something is gated at all)
        assert (g0[:, ~inside] == 0.0).all() and (g0[:, inside] != 0.0).mean() > 0.5, (c.name, t)
    for params, loss, _ in MC.oracle_chain(kind, C, freeze, False):
        assert np.isfinite(params).all() and np.isfinite(loss).all()


@pytest.mark.parametrize("kind,C", MC.oracle_cases())
def test_the_chain_is_three_by_three_and_the_rig_sees_it(kind, C):
    c = MC.oracle_case(kind, C)
    assert c.lengths.tolist() == [MC.ORACLE_T] * MC.ORACLE_S and c.targets.shape[:2] == (MC.ORACLE_S * MC.ORACLE_T, C)
    assert c.base.weights["preserve"] == MC.PRESERVE and c.base.weights["transl"] == 0.0
    _, z = MV.project64(kind, c.base.go, c.base.pose, c.base.shape, c.base.tr, c.base.cams)
    assert (z > 1.0).all()
    assert np.isfinite(c.targets).all()
