"""GPU: the device L-BFGS state machine (csrc/k2b_lbfgs_device.h) against the float64 twin, ROUND BY ROUND, on every branch.

The step kernel is driven through the development entry ``k2b_debug_lbfgs_step`` with SCRIPTED closure results
(``tests/lbfgs_scripts.py``: loss and gradient of (frame, round) from a table, whatever the point), so rounding cannot be
amplified through x and every decision of the state machine can be compared exactly: phase, iteration and evaluation counters,
history fill, line-search counter, the insufficient-progress flag and the low end of the bracket are EQUAL to the twin's after
every round; the next point and the step length stay within

    tol(frame, round) = (2 niter + 2) 2^-24 max(1, max|x|) + 4 |twin32 - twin64|

of the float64 twin's: the float32 roundings of ``x + t d`` over the accepted steps, plus the margin for the device and the
float32 twin differing in summation order (the gradient tests' rule).  ``tests/test_lbfgs_branches.py`` pins the twin to
``torch.optim.LBFGS`` on the same cases, shows that together they take every branch, and that float32 and float64 take the same
ones (frames that do not are named in the case and only printed here).
"""
from functools import lru_cache

import numpy as np
import pytest
import torch

from keypoints2body_amd import native
from tests import lbfgs_scripts as S

pytestmark = pytest.mark.gpu

_INTS = ("phase", "niter", "evals", "nold", "ls_iter", "insuf")
_ZOOM, _DONE = 2, 3


def _split(c, x):
    D, NB = c.split
    e = (0, 3, 3 + D, 3 + D + NB, c.P)
    return tuple(torch.from_numpy(np.ascontiguousarray(x[:, a:b])).cuda() for a, b in zip(e, e[1:]))


class Run:
    """Case `c` on the device and in both twins, one round at a time; what every round left is kept for the tests."""

    def __init__(self, c, cap=None, frames=None, finalize_at=None):
        self.c, self.frames = c, (list(range(c.B)) if frames is None else list(frames))
        f, g = S.tables(c)
        fr = self.frames
        loss = torch.from_numpy(np.ascontiguousarray(f[fr].T.astype(np.float32))).cuda()              # (R, B)
        grad = torch.from_numpy(np.ascontiguousarray(g[fr].transpose(1, 0, 2))).cuda()               # (R, B, P)
        self.dev = native.LbfgsDebug(*_split(c, S.start(c)[fr]), max_iter=c.max_iter, lr=c.lr, history_size=c.H, tolerance_grad=c.tol_g,
                                     tolerance_change=c.tol_c, max_staged_pairs=c.cap if cap is None else cap)
        self.t64, self.t32 = S.twin(c, np.float64, fr), S.twin(c, np.float32, fr)
        self.rounds, self.finalized = [], None
        for r in range(c.rounds):
            self.dev.step(loss[r], grad[r])
            st = self.dev.read_state()
            st["point"] = self.dev.point().cpu().numpy()
            for tw in (self.t64, self.t32):
                tw.advance(*S.result(c, r, fr))
            st["twin"] = {"phase": self.t64.phase.astype(np.int32), "niter": self.t64.n_iter.copy(), "evals": self.t64.evals.copy(),
                          "nold": self.t64.nold.copy(), "ls_iter": self.t64.ls_iter.copy(), "insuf": self.t64.insuf.astype(np.int32),
                          "low": self.t64.low.copy(), "t": self.t64.t.copy(), "point": self.t64.x_eval.copy(), "x": self.t64.x.copy(),
                          "t32": self.t32.t.copy(), "point32": self.t32.x_eval.astype(np.float64), "x32": self.t32.x.astype(np.float64)}
            self.rounds.append(st)
            if finalize_at == r:
                self.finalized = self.dev.finalized().cpu().numpy()
        assert (self.t64.phase == _DONE).all()


@lru_cache(maxsize=None)
def _run(name, cap=None):
    return Run(S.BY_NAME[name], cap)


def _tol(niter, ref, ref32):
    """The rule of the module docstring for a (B, n) quantity `ref` (float64 twin) with its float32 twin's value."""
    fin = np.isfinite(ref) & np.isfinite(ref32)
    scale = np.maximum(1.0, np.where(fin, np.abs(ref), 0.0).max(axis=1))
    return (2 * niter + 2) * 2.0 ** -24 * scale + 4.0 * np.where(fin, np.abs(np.where(fin, ref32 - ref, 0.0)), 0.0).max(axis=1)


def _hold(run):
    """Every gate of the module docstring on a finished run; returns the largest error / tol of the point and of t."""
    c = run.c
    held = np.array([i not in c.exclude for i in run.frames])
    worst_x = worst_t = 0.0
    for r, st in enumerate(run.rounds):
        tw = st["twin"]
        for k in _INTS:
            assert np.array_equal(st[k][held], tw[k][held]), (c.name, r, k, np.nonzero(st[k] != tw[k])[0][:8])
        zoom = held & (tw["phase"] == _ZOOM)
        assert np.array_equal(st["low"][zoom], tw["low"][zoom]), (c.name, r, "low")
        # frames whose float64 twin is finite: the numeric gate; the others: the same elements are not finite
        pattern = np.isfinite(tw["point"])
        assert np.array_equal(np.isfinite(st["point"])[held], pattern[held]), (c.name, r, "non-finite pattern of the point")
        assert np.array_equal(np.isfinite(st["t"])[held], np.isfinite(tw["t"])[held]), (c.name, r, "non-finite pattern of t")
        fin = held & pattern.all(axis=1) & np.isfinite(tw["t"]) & np.isfinite(tw["point32"]).all(axis=1) & np.isfinite(tw["t32"])
        assert c.group == "nonfinite" or fin[held].all(), (c.name, r)
        ex = np.abs(st["point"][fin].astype(np.float64) - tw["point"][fin]).max(axis=1) / _tol(tw["niter"][fin], tw["point"][fin], tw["point32"][fin])
        et = np.abs(st["t"][fin] - tw["t"][fin]) / _tol(tw["niter"][fin], tw["t"][fin, None], tw["t32"][fin, None])
        if ex.size:
            worst_x, worst_t = max(worst_x, float(ex.max())), max(worst_t, float(et.max()))
            assert ex.max() <= 1.0, (c.name, r, "point", int(np.nonzero(fin)[0][ex.argmax()]), float(ex.max()))
            assert et.max() <= 1.0, (c.name, r, "t", int(np.nonzero(fin)[0][et.argmax()]), float(et.max()))
    for i in np.nonzero(~held)[0]:
        print(f"{c.name}: frame {run.frames[i]} (twins part ways) - device phases {[int(st['phase'][i]) for st in run.rounds]}, "
              f"ls_iter {[int(st['ls_iter'][i]) for st in run.rounds]}")
    return worst_x, worst_t


@pytest.mark.parametrize("name", [c.name for c in S.CASES])
def test_device_state_machine_follows_the_float64_twin_round_by_round(name):
    run = _run(name)
    wx, wt = _hold(run)
    done = [next(r for r, st in enumerate(run.rounds) if st["twin"]["phase"][i] == _DONE) for i in range(run.c.B)]
    print(f"{name}: B {run.c.B} P {run.c.P} H {run.c.H} cap {run.c.cap}: largest error / tol: point {wx:.3f}, t {wt:.3f}; "
          f"frames finish in rounds {min(done)}..{max(done)}")
    assert max(done) > 0 or run.c.group == "starts"


def test_device_stops_in_the_twins_round_for_every_finish_rule():
    """Each stop rule and the evaluation budget: the frames that END on it (the twin's record, float32 and float64 agreeing) are
    DONE on the device after that very round and not before.  ``max_iter = 1`` and the tolerance variants are cases of their own."""
    rules = ("init_done", "gtd_exit", "fin_max_iter", "fin_max_eval", "fin_tol_grad", "fin_small_step", "fin_flat", "fin_non_finite")
    seen = dict.fromkeys(rules, 0)
    for name in ("one-iter-8", "tolc-129", "quadratic-63", "starts-64", "nonfinite-65", "walk-255", "descent-70"):
        run, c = _run(name), S.BY_NAME[name]
        events = S.finished(c, 64).events
        phases = np.stack([st["phase"] for st in run.rounds])                   # (R, B)
        first_done = (phases == _DONE).argmax(axis=0)
        assert (phases[-1] == _DONE).all()
        twin_done = (np.stack([st["twin"]["phase"] for st in run.rounds]) == _DONE).argmax(axis=0)
        for i in range(c.B):
            if i in c.exclude:
                continue
            last = [e for e in events[i] if e in rules]
            assert last, (name, i, events[i])
            assert first_done[i] == twin_done[i] == S.finished(c, 64).calls[i] - 1, (name, i, last)
            for e in last:
                seen[e] += 1
    print("frames held per finish rule:", seen)
    assert all(seen.values()), seen


def test_finalize_on_a_copy_leaves_every_frame_at_its_accepted_point_and_the_run_alone():
    """At a round where the twin has frames in the bracket phase, in zoom and finished at once: a finalize call on a COPY of the
    state and the parameter arrays holds every frame's accepted x; the run itself goes on as if nothing had happened."""
    c = S.BY_NAME["walk-64"]
    base = _run(c.name)
    want = {1, _ZOOM, _DONE}
    at = next(r for r, st in enumerate(base.rounds) if r >= 3 and want <= set(st["twin"]["phase"].tolist()))
    run = Run(c, finalize_at=at)
    tw = base.rounds[at]["twin"]
    assert {int(p) for p in tw["phase"]} >= want
    tol = _tol(tw["niter"], tw["x"], tw["x32"])
    err = np.abs(run.finalized.astype(np.float64) - tw["x"]).max(axis=1)
    print(f"finalize at round {at}: phases {np.bincount(tw['phase'], minlength=4)}, largest error / tol {np.max(err / tol):.3f}")
    assert (err <= tol).all()
    moving = tw["phase"] != _DONE                                              # (mid line search the arrays hold a TRIAL point, not x)
    assert (np.abs(base.rounds[at]["point"][moving] - tw["x"][moving]).max(axis=1) > 1e-6).any()
    for a, b in zip(run.rounds, base.rounds):
        assert np.array_equal(a["point"], b["point"], equal_nan=True)
        for k in native.LBFGS_STATE_INTS + ("t", "loss", "hdiag"):
            assert np.array_equal(a[k], b[k], equal_nan=True), k


def test_staged_pairs_cap_does_not_change_a_bit():
    """The ring of three wraps several times (P = 70, twelve iterations): with no history pair staged in LDS, with one, and with
    all of them, every round's point and state are bit-equal.  (At P = 256, H = 30 the uncapped kernel itself reads pairs 23..
    from global memory: ``descent-256`` above.)"""
    c = S.BY_NAME["descent-70"]
    assert min(ev.count("ring_drop") for ev in S.finished(c, 64).events) >= 6
    runs = [_run(c.name), _run(c.name, 0), _run(c.name, 1)]
    for other in runs[1:]:
        for a, b in zip(runs[0].rounds, other.rounds):
            assert np.array_equal(a["point"], b["point"])
            for k in native.LBFGS_STATE_INTS + native.LBFGS_STATE_DOUBLES:
                assert np.array_equal(a[k], b[k]), k
    deep = S.finished(S.BY_NAME["descent-256"], 64)
    assert (deep.nold > 23).sum() >= deep.B // 4


@pytest.mark.parametrize("name", ["iid-65", "walk-255", "descent-256"])
def test_frames_are_independent_of_their_batch(name):
    """A sub-batch of three frames gives the same bits as inside B (narrow and wide form, history in and beyond LDS)."""
    c = S.BY_NAME[name]
    sub = [1, c.B // 2, c.B - 1]
    full, part = _run(name), Run(c, frames=sub)
    for a, b in zip(full.rounds, part.rounds):
        assert np.array_equal(a["point"][sub], b["point"], equal_nan=True)
        for k in native.LBFGS_STATE_INTS + native.LBFGS_STATE_DOUBLES:
            assert np.array_equal(a[k][sub], b[k], equal_nan=True), k


def test_debug_entry_refuses_bad_calls_with_a_device_present():
    z = lambda *s: torch.zeros(*s, device="cuda")
    with pytest.raises(NotImplementedError, match="7 parameters"):
        native.LbfgsDebug(z(2, 3), z(2, 0), z(2, 1), z(2, 3), max_iter=5, lr=1.0)
    d = native.LbfgsDebug(z(2, 3), z(2, 1), z(2, 1), z(2, 3), max_iter=5, lr=1.0)
    with pytest.raises(ValueError, match="grad has shape"):
        d.step(z(2), z(2, 9))
    d.state = d.state[:-16]
    with pytest.raises(ValueError, match="state buffer of"):
        d.step(z(2), z(2, 8))
    e = native.LbfgsDebug(z(0, 3), z(0, 5), z(0, 2), z(0, 3), max_iter=5, lr=1.0)      # an empty batch is a no-op
    e.step(z(0), z(0, 13))
    assert e.point().shape == (0, 13)
