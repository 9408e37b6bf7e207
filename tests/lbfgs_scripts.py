"""Scripted closures for the L-BFGS tests: loss and gradient of (frame, round) come from a seeded table and do NOT depend on
the point the optimiser asks for.

Why: L-BFGS amplifies rounding because the closure depends on x (a one-ulp difference in a search direction moves the next
gradient, which moves the next decision).  With a table there is no such feedback: two implementations that differ in rounding
only can part ways solely where a decision lies within rounding of its threshold, and until then their iterates differ by the
accumulated rounding of ``x + t d`` alone.  That makes the table a sharp gate for every BRANCH of the state machine
(``tests/test_lbfgs_branches.py``: twin against ``torch.optim.LBFGS``; ``tests/test_gpu_lbfgs_branches.py``: device against
twin), on inputs wild enough to reach all of them.

Losses are float32-representable (the device reads them as float32), gradients float32.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from functools import lru_cache
from typing import Optional, Tuple

import numpy as np

from keypoints2body_amd.core.lbfgs_batched import BatchedLBFGS


@dataclass(frozen=True)
class Case:
    """One scripted run: the table's group and seed, the problem's shape and the optimiser's settings (``cap``: staged-pairs
    cap of the device's step kernel, -1 = none)."""
    name: str
    group: str                      # iid | walk | descent | nonfinite | starts | quadratic | tolc
    B: int
    P: int
    H: int
    lr: float
    max_iter: int
    seed: int
    tol_g: float = 1e-7
    tol_c: float = 1e-9
    cap: int = -1
    exclude: Tuple[int, ...] = field(default=())     # frames whose float32 and float64 twins part ways (margin condition)

    @property
    def max_eval(self) -> int:
        return self.max_iter * 5 // 4

    @property
    def rounds(self) -> int:        # the most closure results any frame consumes, + 1 idle round
        return self.max_eval + 2

    @property
    def split(self) -> Tuple[int, int]:
        """(D, NB) of the parameter arrays [3 | D | NB | 3] the device writes the point to: P = 3 + D + NB + 3."""
        nb = min(1 + self.P % 3, self.P - 7)
        return self.P - 6 - nb, nb


def _f32(a):
    return np.asarray(a, dtype=np.float32)


def _tables(c: Case) -> Tuple[np.ndarray, np.ndarray]:
    rng = np.random.default_rng(c.seed)
    B, P, R = c.B, c.P, c.rounds
    g = rng.standard_normal((B, R, P))
    if c.group == "iid":
        f = rng.standard_normal((B, R))
    elif c.group == "walk":                      # a drifting random walk: mostly downhill, with setbacks
        f = np.cumsum(rng.standard_normal((B, R)) - 0.3, axis=1)
    elif c.group == "descent":                   # steady descent: every trial is lower, its gradient a shrunk, jittered copy
        f = 10.0 - np.cumsum(rng.uniform(0.5, 1.5, (B, R)), axis=1)
        base = rng.standard_normal((B, 1, P))
        shrink = 0.85 ** np.arange(R)[None, :, None]
        g = (base + 0.05 * g) * shrink
    elif c.group == "nonfinite":                 # iid sprinkled with NaN / +Inf / -Inf losses; round 0 always finite
        f = rng.standard_normal((B, R))
        u = rng.uniform(size=(B, R))
        u[:, 0] = 1.0
        f = np.where(u < 0.04, np.nan, np.where(u < 0.07, np.inf, np.where(u < 0.09, -np.inf, f)))
    elif c.group == "starts":                    # special starts and a marginal curvature pair, eight frames each; the rest iid
        f = rng.standard_normal((B, R))
        g[0:8, 0] = 0.0                          # zero first gradient: INIT -> DONE
        f[8:16] = f[8:16, :1]                    # constant loss: the line search returns t = 0
        f[16:24] = -1e-12 * np.arange(R)[None]   # decrements below tolerance_change at small, shrinking gradients: flat loss
        g[16:24] = 1e-4 * g[16:24, :1] * (0.5 ** np.arange(R))[None, :, None]
        # a curvature pair with 0 < y . s <= 1e-10 (rejected; "> 0" would keep it): |g|^2 ~ 4e-9 passes the gtd rule, the first trial
        # at t = 1 rises by ~7e-8 so that zoom lands near t = 0.03, the next gradient is 0.8 g: y . s = 0.2 t |g|^2 ~ 2e-11
        f[24:32] = -1e-7 * np.arange(R)[None]
        f[24:32, 1] = 6.7e-8 * rng.uniform(0.5, 2.0, 8)
        g[24:32] = 7.9e-6 * g[24:32, :1] * (0.8 ** np.arange(R))[None, :, None]
    elif c.group == "tolc":                      # gradient scales over four decades against a coarse tolerance_change
        f = rng.standard_normal((B, R))
        g = g * 10.0 ** rng.uniform(-3.0, 1.0, (B, 1, 1))
    else:
        raise ValueError(c.group)
    return _f32(f).astype(np.float64), _f32(g)


def _quadratic_tables(c: Case) -> Tuple[np.ndarray, np.ndarray]:
    """A separable quadratic 0.5 sum a_i x_i^2 along the float64 twin's own path, recorded as a table (so that it, too, is a
    script: replayed it no longer depends on the point)."""
    rng = np.random.default_rng(c.seed)
    a = rng.uniform(0.5, 2.0, (c.B, c.P))
    x0 = start(c).astype(np.float64)
    F, G = [], []

    def fg(X):
        f, g = _f32(0.5 * (a * X * X).sum(1)).astype(np.float64), _f32(a * X)
        F.append(f), G.append(g)
        return f, g
    opt = BatchedLBFGS(fg, x0, lr=c.lr, max_iter=c.max_iter, tolerance_grad=c.tol_g, tolerance_change=c.tol_c, history_size=c.H)
    opt.run()
    while len(F) < c.rounds:
        F.append(F[-1]), G.append(G[-1])
    return np.stack(F, 1), np.stack(G, 1)


@lru_cache(maxsize=None)
def tables(c: Case) -> Tuple[np.ndarray, np.ndarray]:
    """(loss (B, R) float64 holding float32 values, gradient (B, R, P) float32), read-only."""
    f, g = _quadratic_tables(c) if c.group == "quadratic" else _tables(c)
    f.setflags(write=False), g.setflags(write=False)
    return f, g


def start(c: Case) -> np.ndarray:
    return _f32(np.random.default_rng(c.seed + 1000).standard_normal((c.B, c.P)))


def twin(c: Case, dtype, frames=None, record: bool = True) -> BatchedLBFGS:
    """The CPU twin of case `c` (vectors of `dtype`), to be driven with ``advance(*result(c, r, frames))``."""
    x0 = start(c) if frames is None else start(c)[frames]
    return BatchedLBFGS(None, x0.astype(dtype), lr=c.lr, max_iter=c.max_iter, tolerance_grad=c.tol_g, tolerance_change=c.tol_c,
                        history_size=c.H, record=record)


def result(c: Case, r: int, frames=None):
    f, g = tables(c)
    r = min(r, f.shape[1] - 1)
    return (f[:, r], g[:, r]) if frames is None else (f[frames, r], g[frames, r])


def run_twin(c: Case, dtype) -> BatchedLBFGS:
    """Case `c` to the end; ``opt.calls`` = closure results each frame consumed before it finished."""
    opt = twin(c, dtype)
    opt.calls = np.zeros(c.B, dtype=np.int64)
    r = 0
    while np.any(opt.phase != 3):
        opt.calls += opt.phase != 3
        opt.advance(*result(c, r))
        r += 1
    assert r <= c.rounds - 1, (c.name, r)
    return opt


@lru_cache(maxsize=None)
def finished(c: Case, bits: int) -> BatchedLBFGS:
    """``run_twin`` in float32 / float64 (`bits`), computed once and shared: treat it as read-only."""
    return run_twin(c, {32: np.float32, 64: np.float64}[bits])


def parted(c: Case):
    """Frames whose float32 and float64 twins record different event sequences: a decision within rounding of its threshold."""
    a, b = finished(c, 64), finished(c, 32)
    return tuple(i for i in range(c.B) if a.events[i] != b.events[i])


def run_torch(c: Case, frames) -> Tuple[np.ndarray, np.ndarray]:
    """``torch.optim.LBFGS`` in float64 on the frames `frames` of the script, one optimiser per frame: (final points, closure
    calls).  The closure ignores the point: call n returns row n of the frame's table."""
    import torch
    f, g = tables(c)
    x0 = start(c).astype(np.float64)
    xs, calls = [], []
    for i in frames:
        p = torch.tensor(x0[i:i + 1].copy(), requires_grad=True)
        n = [0]

        def closure():
            r = min(n[0], f.shape[1] - 1)
            n[0] += 1
            p.grad = torch.tensor(g[i:i + 1, r].astype(np.float64))
            return torch.tensor(f[i, r], dtype=torch.float64)
        try:
            torch.optim.LBFGS([p], max_iter=c.max_iter, lr=c.lr, tolerance_grad=c.tol_g, tolerance_change=c.tol_c, history_size=c.H,
                              line_search_fn="strong_wolfe").step(closure)
            xs.append(p.detach().numpy()[0])
            calls.append(n[0])
        except IndexError:        # torch's own end on a NaN loss that satisfies Wolfe at once: ``bracket[low_pos]`` of a one-point bracket
            xs.append(np.full(c.P, np.nan))
            calls.append(-1)
    return np.stack(xs), np.asarray(calls)


# ---- the cases of the GPU tests (tests/test_gpu_lbfgs_branches.py); the CPU tests hold the coverage and margin conditions on them.
# Vector lengths: one to three elements per lane around the 64-lane edges in the step kernel's narrow form (8 .. 192), four in
# its wide form (193 .. 256); history 1, 2, 3 and torch's 100; staged-pairs cap 0, 1 and none.
CASES = (
    Case("iid-8", "iid", 256, 8, 2, 1.0, 16, seed=1),
    Case("iid-63", "iid", 256, 63, 3, 0.3, 20, seed=2, cap=1),
    Case("iid-65", "iid", 256, 65, 100, 1.0, 30, seed=3),
    Case("iid-129", "iid", 256, 129, 1, 1e-2, 12, seed=4, cap=0),
    Case("iid-193", "iid", 256, 193, 3, 1.0, 16, seed=5),
    Case("walk-64", "walk", 256, 64, 2, 1.0, 20, seed=6, cap=0),
    Case("walk-128", "walk", 256, 128, 4, 0.3, 30, seed=7),
    Case("walk-192", "walk", 256, 192, 100, 1e-2, 16, seed=8, cap=1),
    Case("walk-255", "walk", 256, 255, 2, 1.0, 12, seed=9),
    Case("descent-191", "descent", 64, 191, 3, 1.0, 16, seed=10),
    Case("descent-256", "descent", 64, 256, 30, 1.0, 40, seed=11),
    Case("descent-70", "descent", 64, 70, 3, 1.0, 12, seed=12),
    Case("nonfinite-65", "nonfinite", 64, 65, 3, 1.0, 20, seed=13),
    Case("nonfinite-256", "nonfinite", 64, 256, 2, 0.3, 16, seed=14, cap=1),
    Case("starts-64", "starts", 64, 64, 3, 1.0, 12, seed=15),
    Case("quadratic-63", "quadratic", 64, 63, 100, 1.0, 30, seed=16, tol_g=1e-3),
    Case("tolc-129", "tolc", 64, 129, 2, 1e-2, 12, seed=17, tol_g=0.0, tol_c=1e-3),
    Case("one-iter-8", "iid", 256, 8, 1, 1.0, 1, seed=18),
)
BY_NAME = {c.name: c for c in CASES}
