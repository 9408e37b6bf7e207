"""Host logic: every branch of the lock-step L-BFGS twin (``core/lbfgs_batched.py``) pinned to ``torch.optim.LBFGS`` in float64,
and the conditions under which the scripted cases of ``tests/lbfgs_scripts.py`` may serve as the device's yardstick
(``tests/test_gpu_lbfgs_branches.py``).

``tests/test_lbfgs_batched.py`` compares twin and torch on one mild family (quadratic + quartic at lr 1e-2), which never enters the
zoom phase, never rejects a curvature pair and ends on max_eval only.  Here the closure is SCRIPTED (its results come from a
table, whatever the point), so there is no feedback through x to amplify rounding, and the tables are wild enough to take every
branch.  The twin's branch record (``record=True``, filled from the masks it branches on) says which.

One deliberate difference from torch: a frame whose ACCEPTED loss is not finite stops in the twin (and on the device).  torch
has no such rule - it either dies on ``bracket[low_pos]`` of a one-point bracket (a NaN loss that satisfies Wolfe at once) or
goes on with NaN directions until the budget is spent - so frames that record ``fin_non_finite`` have no torch counterpart
and are held to the device only.
"""
import numpy as np
import pytest

from keypoints2body_amd.core.lbfgs_batched import EVENTS, BatchedLBFGS
from tests import lbfgs_scripts as S

_IDS = [c.name for c in S.CASES]


@pytest.mark.parametrize("c", S.CASES, ids=_IDS)
def test_float64_twin_equals_torch_frame_by_frame_on_the_script(c):
    twin = S.finished(c, 64)
    xt, calls = S.run_torch(c, range(c.B))
    stopped = np.array(["fin_non_finite" in ev for ev in twin.events])
    assert stopped.any() == (c.group == "nonfinite")
    held = ~stopped
    assert held.sum() >= c.B // 2
    assert np.array_equal(twin.calls[held], calls[held])                       # as many closure calls, frame by frame
    assert np.all((calls[stopped] == -1) | (calls[stopped] >= twin.calls[stopped]))
    # (an Inf loss in the bracket can make a NaN step that both then take: the same elements are non-finite in both)
    finite = np.isfinite(xt[held])
    assert np.array_equal(np.isfinite(twin.x[held]), finite) and (finite.all() or c.group == "nonfinite")
    diff = np.where(finite, np.abs(np.where(finite, twin.x[held], 0.0) - np.where(finite, xt[held], 0.0)), 0.0)
    err = diff.max(axis=1) / np.maximum(1.0, np.where(finite, np.abs(xt[held]), 0.0).max(axis=1))
    print(f"{c.name}: {held.sum()} frames ({int((~finite.all(axis=1)).sum())} not finite), twin - torch {err.max():.2e} relative")
    assert err.max() < 1e-9


@pytest.mark.parametrize("c", S.CASES, ids=_IDS)
def test_margin_condition_float32_and_float64_twins_take_the_same_branches(c):
    """Per case at most 2 % of the frames may part ways (a decision within float32 rounding of its threshold); they are named in
    the case (``exclude``) and left out of the device's numeric gate.  The seeds were chosen on the twins alone."""
    parted = S.parted(c)
    assert len(parted) <= 0.02 * c.B, parted
    assert parted == tuple(c.exclude), parted
    a, b = S.finished(c, 64), S.finished(c, 32)
    same = [i for i in range(c.B) if i not in parted]
    assert np.array_equal(a.calls[same], b.calls[same]) and np.array_equal(a.n_iter[same], b.n_iter[same])
    assert b.x.dtype == np.float32 and a.x.dtype == np.float64


def _coverage():
    """event -> {case name: frames that take it}, counting only frames whose float32 twin takes the same event sequence."""
    cov = {e: {} for e in EVENTS}
    for c in S.CASES:
        parted, twin = set(S.parted(c)), S.finished(c, 64)
        for i, ev in enumerate(twin.events):
            if i not in parted:
                for e in set(ev):
                    cov[e][c.name] = cov[e].get(c.name, 0) + 1
    return cov


def test_coverage_condition_every_branch_is_taken_by_the_cases_of_the_gpu_tests():
    cov = _coverage()
    for e in EVENTS:
        groups = sorted({S.BY_NAME[n].group for n in cov[e]})
        print(f"{e:22s} {sum(cov[e].values()):5d} frames  groups {', '.join(groups)}  e.g. {max(cov[e], key=cov[e].get) if cov[e] else '-'}")
    assert [e for e in EVENTS if not cov[e]] == []
    for ev in (ev for c in S.CASES for ev in S.finished(c, 64).events):
        assert set(ev) <= set(EVENTS)
    # what single cases are there for
    starts = S.finished(S.BY_NAME["starts-64"], 64).events
    assert all(ev == ["init_done"] for ev in starts[0:8])
    assert all("fin_t0" in ev for ev in starts[8:16])
    assert all(ev[-1] == "fin_flat" and "fin_small_step" not in ev and "fin_t0" not in ev for ev in starts[16:24])
    assert all("pair_rejected" in ev and "pair_accepted" in ev for ev in starts[24:32])          # the pair with 0 < y . s <= 1e-10
    assert all(ev[-1] == "fin_tol_grad" for ev in S.finished(S.BY_NAME["quadratic-63"], 64).events)
    assert all(ev[1] in ("br_exhausted_keep0", "br_exhausted_take_t") for ev in S.finished(S.BY_NAME["one-iter-8"], 64).events)
    assert any(ev[-1] == "gtd_exit" for ev in S.finished(S.BY_NAME["tolc-129"], 64).events)
    # more pairs than the 23 that fit the step kernel's 48 KiB of LDS at P = 256
    deep = S.finished(S.BY_NAME["descent-256"], 64)
    assert (deep.nold > 23).sum() >= deep.B // 4 and deep.H == 30
    wrap = S.finished(S.BY_NAME["descent-70"], 64)                              # the ring of three wraps several times
    assert min(ev.count("ring_drop") for ev in wrap.events) >= 6


def test_line_search_uses_its_own_tolerance_change_like_torch():
    """``LBFGS.step`` does not hand its tolerance_change to ``_strong_wolfe``: the "bracket is so small" stop of the zoom phase
    always compares with 1e-9.  (Found by the ``tolc`` script: with the optimiser's own 1e-3 there the twin stopped line searches
    that torch went on with, and made 2 closure calls where torch made 3 to 5.)"""
    c = S.BY_NAME["tolc-129"]
    twin = S.finished(c, 64)
    _, calls = S.run_torch(c, range(c.B))
    assert np.array_equal(twin.calls, calls) and calls.max() > 2
    assert any("zoom_enter_low0" in ev and "zn_width_stop" not in ev for ev in twin.events)


def test_record_changes_no_arithmetic():
    for c in (S.BY_NAME["iid-63"], S.BY_NAME["nonfinite-65"], S.BY_NAME["descent-70"]):
        for dt in (np.float32, np.float64):
            a, b = S.twin(c, dt, record=True), S.twin(c, dt, record=False)
            for r in range(c.rounds):
                a.advance(*S.result(c, r)), b.advance(*S.result(c, r))
                for k in ("x", "x_eval", "t", "loss", "d", "Y", "S", "RO", "br_t", "br_f"):
                    assert np.array_equal(getattr(a, k), getattr(b, k), equal_nan=True), (c.name, r, k)
                for k in ("phase", "n_iter", "evals", "nold", "ls_iter", "low", "insuf"):
                    assert np.array_equal(getattr(a, k), getattr(b, k)), (c.name, r, k)
            assert b.events is None and all(a.events)


def test_frames_of_a_script_are_independent():
    c = S.BY_NAME["walk-64"]
    sub = [3, 100, 255]
    full, part = S.finished(c, 32), S.twin(c, np.float32, frames=sub)
    for r in range(c.rounds):
        part.advance(*S.result(c, r, sub))
    assert np.array_equal(part.x, full.x[sub]) and part.events == [full.events[i] for i in sub]


# ---- point-dependent families: a smoke of the recorder, no numeric gate against torch (they amplify rounding: the float64 twin
# and torch part ways on a few frames in 16 by anything from 1e-8 to 20 relative) ------------------------------------------------
def _rosenbrock(X):
    a, b = X[:, :-1], X[:, 1:]
    f = (100.0 * (b - a * a) ** 2 + (1.0 - a) ** 2).sum(1)
    g = np.zeros_like(X)
    g[:, :-1] += -400.0 * a * (b - a * a) - 2.0 * (1.0 - a)
    g[:, 1:] += 200.0 * (b - a * a)
    return f, g


def _robust(X):                   # GMoF-like: sum r^2 / (r^2 + s^2)
    r2, s2 = X * X, 0.25
    return (r2 / (r2 + s2)).sum(1), 2.0 * X * s2 / (r2 + s2) ** 2


def _kink(X):
    return np.abs(X).sum(1) + 0.5 * (X * X).sum(1), np.sign(X) + X


def _step(X):                     # discontinuous: an ill-conditioned quadratic with a unit jump at |x| = 1/2
    c = (1.0 + np.arange(X.shape[1])) ** 2
    return 0.5 * (c * X * X).sum(1) + (np.abs(X) > 0.5).sum(1), c * X


@pytest.mark.parametrize("fg,H", [(_rosenbrock, 2), (_robust, 3), (_kink, 4), (_step, 2)], ids=["rosenbrock", "robust", "kink", "step"])
def test_recorder_on_point_dependent_functions(fg, H):
    x0 = np.random.default_rng(7).standard_normal((16, 6))
    runs = []
    for record in (True, False):
        opt = BatchedLBFGS(lambda X: tuple(np.asarray(v, np.float64) for v in fg(X)), x0, lr=1.0, max_iter=20, history_size=H,
                           record=record)
        runs.append((opt.run().copy(), opt))
    assert np.array_equal(runs[0][0], runs[1][0], equal_nan=True)
    events = runs[0][1].events
    assert all(ev and set(ev) <= set(EVENTS) for ev in events)
    assert all(ev[0] in ("first_step_lr", "first_step_scaled") for ev in events)
    assert any(e.startswith("zoom_enter") for ev in events for e in ev)          # at lr = 1 the line search has to work
    # a finished frame's record ends on a stop rule
    assert all(ev[-1].startswith("fin_") or ev[-1] == "gtd_exit" for ev in events)
