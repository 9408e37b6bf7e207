"""The input conditions of the projected-surface-target tests (tests/reproj_surface_common.py), asserted from the float64 / float32
oracle alone, no GPU - as tests/test_reproj_conditions.py does for the kinematic term: a case whose float32 oracle is off by
more than ``E32_LIMIT = 1e-4``, or whose gradient (loss) moves by more than ``ROUNDING_LIMIT = 2.5e-6``
(``TERM_ROUNDING_LIMIT_LOSS = 2.5e-7``) under one float32 rounding of its targets, would make the GPU gates a test of the inputs.
The term has no counterpart in the reference: the oracle is the formula of ``include/k2b.h`` (``k2b_fit_image``)."""
import numpy as np
import pytest

from tests import fit_gradient_common as G
from tests import lbs_layouts_common as L
from tests import reproj_surface_common as S


def test_the_limits_are_the_existing_ones():
    assert (G.E32_LIMIT, G.ROUNDING_LIMIT, L.TERM_ROUNDING_LIMIT_LOSS) == (1e-4, 2.5e-6, 2.5e-7)
    assert (G.GRAD_GATE, G.LOSS_GATE, G.ORDER_FACTOR) == (2e-5, 2e-6, 4.0)


@pytest.mark.parametrize("case", S.term_cases(), ids=lambda c: c.name)
def test_term_cases_meet_the_conditions(case):
    r = S.term_figures(case)
    print(f"{case.name}: e32 {min(r.e32.values()):.1e} .. {max(r.e32.values()):.1e}, e32 loss {r.e32_loss:.1e}, rounding "
          f"{min(r.rounding.values()):.1e} .. {max(r.rounding.values()):.1e}, rounding loss {r.rounding_loss:.1e}")
    S.term_reference(case)
    assert (r.loss64 > 0).all() and all(np.abs(r.g64[:, a:b]).max() > 0 for _, a, b in L.term_groups(case.J, case.NB).groups)


def test_base_case_is_the_one_described():
    c = S.base()
    J, NB = L.LANDMARK_LAYOUT
    assert (c.J, c.NB) == (J, NB) and c.targets.shape == (3, 20, 3) and c.focal == (500.0, 430.0)
    assert c.rows == L.surface_term_case(3).rows and c.rows[:3] == (J, J + 2, J + 4)
    assert c.conf[1, 3] == 0.0 and np.count_nonzero(c.conf == 0.0) == 1 and c.conf[c.conf > 0].min() >= 0.5 and c.conf.max() <= 1.5
    z = S._points64(J, NB, c.params, c.rows)[..., 2]
    print(f"depth of the points {z.min():.2f} .. {z.max():.2f} m")
    assert 2.0 < z.min() and z.max() < 4.5
    xy = S._points64(J, NB, c.params, c.rows)[..., :2].mean(axis=1)
    assert np.abs(xy).max() < 1e-6                     # on the optical axis


def test_a_skipped_target_is_what_confidence_zero_leaves():
    """The oracle WITHOUT the moved target equals the oracle with it at confidence 0 (finite depth: 0 . finite = 0)."""
    c = S.conf_zero_moved()
    import dataclasses
    with_it = S.term_oracle(dataclasses.replace(c, skip=None), True)
    without = S.term_oracle(c, True)
    assert np.array_equal(with_it[0], without[0]) and np.array_equal(with_it[1], without[1])


@pytest.mark.parametrize("case", S.fit_cases(), ids=lambda c: c.name)
def test_whole_loss_cases_meet_the_conditions(case):
    r = S.figures(case)
    print(f"{case.name}: e32 {min(r.e32.values()):.1e} .. {max(r.e32.values()):.1e}, e32 loss {r.e32_loss:.1e}, rounding "
          f"{min(r.rounding.values()):.1e} .. {max(r.rounding.values()):.1e}")
    S.reference(case)
    J = G.layout(case.kind).J
    assert any(i >= J for i in case.idx) and any(i < J for i in case.idx)
    assert max(case.idx) < S.num_outputs(case.kind, case.lmk)
