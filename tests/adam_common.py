"""Shared by the Adam tests (``tests/test_adam_conditions.py`` without a GPU, ``tests/test_gpu_adam.py``): a float64 twin of
``torch.optim.Adam``'s single-tensor step, the hyper-parameter rows, the cases of both tiers, their references and the gates.

The update is written out five times in ``csrc/`` (``adam_update`` of k2b_fit.hip, the ``adam`` lambda of k2b_fit_tree.hip, the tails of
``k2b_vertex_term_kernel`` and ``k2b_surface_term_kernel``, ``k2b_adam_kernel``) and the host forms its coefficients (the table of
``adam_table``, one table for both counts of a chain, ``coef + it`` in the surface path, ``1 - beta`` in ``fill_call_fields``).

Tier A: problems whose gradient is known exactly per parameter, so that an error of the update cannot hide behind one of the
gradient.  Every loss weight is zero but one: the preserve term (``g = 2 w^2 (theta - theta0)`` on the body pose under the prior,
``optimize_mask`` 2), the shape prior (``g = 2 w^2 beta``, mask 4) or the translation prior (``g = 2 w^2 (t - t0)``, mask 8, 24-joint
models only).  The twin iterates ``x <- Adam(x, g(x))`` in float64; ``torch.optim.Adam`` on float32 CPU tensors with the same closure is
the yardstick.  Frame f of a device call is row ``f % PERIOD`` of a seeded block, so that one reference serves every frame count;
one lane per frame starts exactly at the centre (gradient identically zero).

Gate of Tier A, per case, on the maximum over frames and lanes: ``|x_dev - x_64| <= max(floor, ORDER_FACTOR * e32)``, e32 the same
statistic of torch's float32 Adam against the twin, ``floor = num_iters * lr * 4 * 2^-23``: the kernels form a step with two 1-ulp
hardware operations (``v_rcp_f32``, ``v_sqrt_f32``) and the reciprocal of sqrt(bc2) where torch rounds correctly, about four ulp of
a step of length at most about lr.

Conditions on the inputs, from the oracle alone (``check_conditions``; asserted for every case by the CPU test): (a) e32 is at
most a quarter of the project's parameter gate 1e-4; (b) multiplying the twin's gradient at every step by ``1 +- 2^-23``, seeded
signs, moves no end state by more than half the floor.  Rows with a short memory (beta1 = 0: the step is lr sign(g) at the centre; beta2 = 0 or 0.9: it is lr m / |g| with g near 0) fail
them where a lane reaches the centre within the run: every rounding of g is amplified there, torch's own float32 Adam ends up to
1e-2 off the twin.  Those rows keep their hyper-parameters and start further from the centre (``ROW_OFFSETS``); the long run takes a
smaller lr (``LONG_LR``).

Tier B: the full problem (every term on) against the oracle's fitters ``fit_world_adam`` / ``fit_world_adam_smplx`` with the same
hyper-parameters, at the project's gates (parameters 1e-4, loss 2e-4 relative); the float32 oracle must sit within a quarter of
the parameter gate of the float64 one."""
import contextlib
import functools
from dataclasses import dataclass, replace
from types import SimpleNamespace
from typing import Optional

import numpy as np
import torch

from keypoints2body_amd import synthetic
from tests import fit_gradient_common as F
from tests import helpers as H

PARAM_TOL = 1e-4           # tests/test_gpu_parity.py
LOSS_RTOL = 2e-4
ORDER_FACTOR = F.ORDER_FACTOR
E32_LIMIT = PARAM_TOL / 4.0
ULP = 2.0 ** -23
PERIOD = 13                # frames of the seeded block


@dataclass(frozen=True)
class Row:
    name: str
    lr: float
    b1: float
    b2: float
    eps: float

    def set(self, cfg, iters: int):
        cfg.num_iters, cfg.step_size, cfg.adam_beta1, cfg.adam_beta2, cfg.adam_eps = int(iters), self.lr, self.b1, self.b2, self.eps
        return cfg

    @property
    def kw(self):
        return dict(lr=self.lr, adam_betas=(self.b1, self.b2), adam_eps=self.eps)


ROWS = {r.name: r for r in (
    Row("defaults", 1e-2, 0.9, 0.999, 1e-8),
    Row("b.5_.9", 1e-2, 0.5, 0.9, 1e-8),
    Row("b1_0", 1e-2, 0.0, 0.999, 1e-8),
    Row("b2_0", 1e-2, 0.9, 0.0, 1e-8),
    Row("eps_1e-3", 1e-2, 0.9, 0.999, 1e-3),
    Row("b.99_.9999_eps_1e-12", 1e-2, 0.99, 0.9999, 1e-12),
    Row("lr_3e-2", 3e-2, 0.9, 0.999, 1e-8),
)}
ITERS = (1, 2, 37)
# The long run: both bias terms are exactly 1 in float32 long before its end (0.5^t and 0.9^t < 2^-25 from t = 165 on; with
# the default beta2 that takes 16 600 steps), and the table is far longer than any other in the suite.
LONG_ITERS, LONG_ROW = 1200, "b.5_.9"
TIER_B_ROWS = {r.name: r for r in (Row("b.8_.99_eps_1e-6", 1e-2, 0.8, 0.99, 1e-6), Row("eps_1e-3", 1e-2, 0.9, 0.999, 1e-3))}
# The surface-target routes have no Tier A, and the gradients of the full problem (up to 1e5) hide any eps up to 1e-3: their own
# row has an eps among the gradients' magnitudes (``test_adam_conditions.py`` asserts that the oracle's result depends on it).
SURFACE_ROW = Row("b.8_.99_eps_10", 1e-2, 0.8, 0.99, 10.0)
B_ROWS = {**TIER_B_ROWS, SURFACE_ROW.name: SURFACE_ROW}
STEP_ROWS = (ROWS["defaults"], ROWS["b.5_.9"], Row("b0_0_eps_1e-3", 3e-2, 0.0, 0.0, 1e-3))     # k2b_adam_step alone


# ---- the twin ------------------------------------------------------------------------------------------------------------------
def adam64(x, m, v, g, t: int, row: Row):
    """One step of ``torch/optim/adam.py::_single_tensor_adam`` (no weight decay, no amsgrad) on float64 arrays; the bias terms
    are Python floats, as there.  Returns the new (x, m, v)."""
    # exp_avg.lerp_(grad, 1 - beta1), as the weighted sum it stands for: the form m + (g - m) w loses a small g behind a large m
    # even in float64 (beta1 = 0 after a gradient of 1e15), where torch's lerp switches to g - (g - m) (1 - w)
    m = m * row.b1 + g * (1.0 - row.b1)
    v = v * row.b2 + (g * g) * (1.0 - row.b2)              # exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    bc1 = 1.0 - row.b1 ** t
    bc2 = 1.0 - row.b2 ** t
    step_size = row.lr / bc1
    denom = np.sqrt(v) / (bc2 ** 0.5) + row.eps
    return x - step_size * (m / denom), m, v


def twin_on_gradients(x0, grads, row: Row):
    """The twin on a recorded gradient sequence [T][n]: (x, m, v) after every step, each [T][n] float64."""
    x = np.asarray(x0, dtype=np.float64)
    m, v = np.zeros_like(x), np.zeros_like(x)
    out = []
    for t, g in enumerate(np.asarray(grads, dtype=np.float64), start=1):
        x, m, v = adam64(x, m, v, g, t, row)
        out.append((x, m, v))
    return tuple(np.stack([o[k] for o in out]) for k in range(3))


def torch_on_gradients(x0, grads, row: Row, dtype):
    """``torch.optim.Adam`` (single-tensor path) on the same gradients: (x, m, v) after the last step as float64 arrays."""
    x = torch.tensor(np.asarray(x0), dtype=dtype, requires_grad=True)
    opt = torch.optim.Adam([x], lr=row.lr, betas=(row.b1, row.b2), eps=row.eps, foreach=False)
    for g in grads:
        x.grad = torch.tensor(np.asarray(g), dtype=dtype)
        opt.step()
    st = opt.state[x]
    return tuple(a.detach().double().numpy() for a in (x, st["exp_avg"], st["exp_avg_sq"]))


@contextlib.contextmanager
def one_thread():
    """The float32 sums of the oracle, and with them e32, do not depend on how many cores the machine offers."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(threads)


def twin_affine(start, centre, weight: float, row: Row, iters: int, signs_seed: Optional[int] = None):
    """``x <- Adam(x, 2 w^2 (x - centre))`` in float64 from the float32 arrays `start`, `centre`.  `signs_seed`: every gradient is
    multiplied by ``1 +- 2^-23``, seeded signs (condition (b))."""
    x, c = np.asarray(start, dtype=np.float64), np.asarray(centre, dtype=np.float64)
    m, v = np.zeros_like(x), np.zeros_like(x)
    k = 2.0 * float(np.float32(weight)) ** 2
    rng = None if signs_seed is None else np.random.default_rng(signs_seed)
    for t in range(1, iters + 1):
        g = k * (x - c)
        if rng is not None:
            g = g * (1.0 + ULP * rng.choice((-1.0, 1.0), size=g.shape))
        x, m, v = adam64(x, m, v, g, t, row)
    return x


def torch_affine(start, centre, weight: float, row: Row, iters: int, dtype=torch.float32):
    """The yardstick: ``torch.optim.Adam`` on CPU tensors of `dtype` with the closure ``w^2 |x - centre|^2``."""
    with one_thread():
        x = torch.tensor(np.asarray(start), dtype=dtype, requires_grad=True)
        c = torch.tensor(np.asarray(centre), dtype=dtype)
        opt = torch.optim.Adam([x], lr=row.lr, betas=(row.b1, row.b2), eps=row.eps, foreach=False)
        w2 = float(np.float32(weight)) ** 2
        for _ in range(iters):
            opt.zero_grad()
            (w2 * ((x - c) ** 2).sum()).backward()
            opt.step()
        return x.detach().double().numpy()


# ---- Tier A --------------------------------------------------------------------------------------------------------------------
TERM_MASK = {"preserve": 2, "shape": 4, "transl": 8}
TERM_WEIGHT = {k: F.ALL_ON[k] for k in TERM_MASK}                  # 5, 5, 100
FUSED_FRAMES = {1: 9, 2: 17, 3: 33, 4: 33}                         # debug_launch_shape -> frames (tests/isolation_common.py)
TREE_KINDS = ("smplx20", "smplx32", "tree21")
KINDS = ("smpl10",) + TREE_KINDS
# Starts: |start - centre| log-uniform in OFFSETS, mixed signs.  The rows of ROW_OFFSETS fail the conditions near the centre (module
# docstring) and start further off, so far that no lane comes near the centre within 37 steps: a step is lr |m^| / sqrt(v^), at most
# about 1.3 lr there (measured with the twin), 0.5 in all.  The long run takes LONG_LR for the same reason: 1200 steps stay below 0.4.
OFFSETS = (1e-3, 1.0)
ROW_OFFSETS = {"b2_0": (1.0, 2.0), "b.5_.9": (0.5, 1.0), "b1_0": (0.5, 1.0)}
LONG_LR = 2.5e-4


def offsets_of(row_name: str):
    return ROW_OFFSETS.get(row_name, OFFSETS)


def terms_of(kind: str):
    return ("preserve", "shape", "transl") if F.layout(kind).kernel == "fused" else ("preserve", "shape")


def active_columns(kind: str, term: str):
    """(first, end) column of the packed row [global_orient | pose | shape | transl] that the term's gradient reaches."""
    lay = F.layout(kind)
    if term == "preserve":
        return 3, 3 + lay.prior_dims
    if term == "shape":
        return 3 + lay.D, 3 + lay.D + lay.betas_prior
    return 3 + lay.D + lay.NB, lay.P


def tier_a_row(row_name: str, iters: int) -> Row:
    """The row as the case runs it: the long run takes LONG_LR."""
    row = ROWS[row_name]
    return replace(row, lr=LONG_LR) if iters == LONG_ITERS else row


@functools.lru_cache(maxsize=None)
def block(term: str, n: int, span: tuple = OFFSETS):
    """(centre, start): [PERIOD][n] float32.  Lane r % n of frame r starts exactly at the centre; from six lanes on, the two
    lanes behind it start at the ends of the offset range."""
    lo, hi = span
    u = synthetic.uniform(90, PERIOD * n, 53).reshape(PERIOD, n)
    sign = np.where(synthetic.uniform(91, PERIOD * n, 53).reshape(PERIOD, n) < 0.5, -1.0, 1.0)
    off = sign * lo * (hi / lo) ** u
    centre = np.zeros((PERIOD, n)) if term == "shape" else 0.2 * synthetic.normalish(92, (PERIOD, n), 53)
    centre = centre.astype(np.float32)
    r = np.arange(PERIOD)
    if n >= 6:
        off[r, (r + 1) % n] = sign[r, (r + 1) % n] * lo
        off[r, (r + 2) % n] = sign[r, (r + 2) % n] * hi
    start = (centre + off).astype(np.float32)
    start[r, r % n] = centre[r, r % n]
    return centre, start


@dataclass(frozen=True, eq=False)
class ReferenceA:
    x64: np.ndarray         # [PERIOD][n]
    e32: float
    floor: float
    moved: float            # condition (b): what one ulp on every gradient does
    still: np.ndarray       # [PERIOD][n] bool: lanes whose gradient is identically zero

    @property
    def tol(self):
        return max(self.floor, ORDER_FACTOR * self.e32)


@functools.lru_cache(maxsize=None)
def reference_a(term: str, n: int, row_name: str, iters: int) -> ReferenceA:
    row = tier_a_row(row_name, iters)
    centre, start = block(term, n, offsets_of(row_name))
    w = TERM_WEIGHT[term]
    x64 = twin_affine(start, centre, w, row, iters)
    x32 = torch_affine(start, centre, w, row, iters)
    moved = max(float(np.abs(twin_affine(start, centre, w, row, iters, signs_seed=s) - x64).max()) for s in (1, 2))
    return ReferenceA(x64, float(np.abs(x32 - x64).max()), iters * row.lr * 4.0 * ULP, moved, start == centre)


def check_conditions(what: str, e32: float, floor: Optional[float] = None, moved: Optional[float] = None):
    assert e32 <= E32_LIMIT, f"{what}: torch's float32 Adam is {e32:.2e} off the float64 twin (limit {E32_LIMIT:.1e}): badly conditioned"
    if floor is not None:
        assert moved <= 0.5 * floor, f"{what}: one ulp on every gradient moves the end state by {moved:.2e}, more than half the floor {floor:.2e}"


def tier_a_cases():
    """(term, active lanes, row, iterations) of every Tier A reference the GPU tests use."""
    widths = sorted({(t, active_columns(k, t)[1] - active_columns(k, t)[0]) for k in KINDS for t in terms_of(k)})
    return [(t, n, r, it) for t, n in widths for r in ROWS for it in ITERS] + [(t, n, LONG_ROW, LONG_ITERS) for t, n in widths]


@functools.lru_cache(maxsize=None)
def passive_row(P: int) -> np.ndarray:
    """[PERIOD][P] float32 values for the columns the term does not reach, zeros of both signs among them."""
    a = (0.3 * synthetic.normalish(93, (PERIOD, P), 53)).astype(np.float32)
    pick = synthetic.uniform(94, PERIOD * P, 53).reshape(PERIOD, P)
    a[pick < 0.1] = 0.0
    a[pick < 0.05] = -0.0
    return a


@dataclass(frozen=True, eq=False)
class InputsA:
    case: F.Case
    x0: np.ndarray          # [B][P] packed start
    first: int              # active columns
    end: int


def tier_a_inputs(kind: str, term: str, row_name: str, frames: int) -> InputsA:
    """The device call's inputs: frame f is row f % PERIOD of the block in the term's columns and of ``passive_row`` elsewhere.
    One targeted joint (the root) with a finite target; its weight is zero."""
    lay = F.layout(kind)
    a, b = active_columns(kind, term)
    centre, start = block(term, b - a, offsets_of(row_name))
    rows = np.arange(frames) % PERIOD
    x0 = passive_row(lay.P)[rows].copy()
    x0[:, a:b] = start[rows]
    c = passive_row(lay.P)[rows].copy()              # centres for the whole row: outside the term's columns they are never read
    c[:, a:b] = centre[rows]
    cols = native_columns(lay)
    part = lambda arr, k: np.ascontiguousarray(arr[:, cols[k]])
    case = F.Case(f"adam/{kind}/{term}", kind, (0,), np.full((frames, 1, 3), 0.25, dtype=np.float32), part(x0, "global_orient"),
                  part(x0, "body_pose"), part(x0, "betas"), part(x0, "transl"), weights=F.only(term),
                  preserve=part(c, "body_pose") if term == "preserve" else None, tr_target=part(c, "transl") if term == "transl" else None,
                  mask=TERM_MASK[term])
    return InputsA(case, x0, a, b)


def native_columns(lay: F.Layout) -> dict:
    from keypoints2body_amd import native
    return native.param_columns(lay.D, lay.NB)


def fit(case: F.Case, row: Row, iters: int, launch_shape: int = 0, model=None):
    """``native.fit_world`` on the case with the row's hyper-parameters: the packed result [B][P] (device tensor) and the loss."""
    from keypoints2body_amd import native
    cfg = row.set(F.fit_config(case, launch_shape), iters)
    conf = None if case.conf is None else H.cuda(case.conf)
    out = native.fit_world(model or F.native_model(case.kind), H.native_prior(), cfg, list(case.idx), H.cuda(case.j3d), conf,
                           H.cuda(case.go), H.cuda(case.pose), H.cuda(case.shape), H.cuda(case.tr),
                           preserve_pose=None if case.preserve is None else H.cuda(case.preserve),
                           transl_prior_target=None if case.tr_target is None else H.cuda(case.tr_target))
    return torch.cat([out[k] for k in native.PARAM_KEYS], dim=1), out["loss"]


def gate_a(inp: InputsA, ref: ReferenceA, packed: torch.Tensor, what: str) -> float:
    """Prints the figures, then asserts: the term's columns within the gate of the twin, its still lanes and every other column
    ``torch.equal`` to the start.  Returns the deviation."""
    x0 = torch.as_tensor(inp.x0)
    got = packed.cpu()
    rows = np.arange(got.shape[0]) % PERIOD
    err = float(np.abs(got[:, inp.first:inp.end].double().numpy() - ref.x64[rows]).max())
    print(f"adam gate {what}: deviation {err:.2e}  e32 {ref.e32:.2e}  floor {ref.floor:.2e}  gate {ref.tol:.2e}")
    assert torch.isfinite(got).all(), what
    outside = torch.ones(got.shape[1], dtype=torch.bool)
    outside[inp.first:inp.end] = False
    assert torch.equal(got[:, outside], x0[:, outside]), f"{what}: a parameter that the term does not reach, or one outside the optimiser, moved"
    still = torch.as_tensor(ref.still[rows])
    assert torch.equal(got[:, inp.first:inp.end][still], x0[:, inp.first:inp.end][still]), f"{what}: a lane with gradient zero moved"
    assert err <= ref.tol, f"{what}: {err:.2e} off the float64 twin, gate {ref.tol:.2e} (e32 {ref.e32:.2e}, floor {ref.floor:.2e})"
    return err


# ---- k2b_adam_step alone -------------------------------------------------------------------------------------------------------
STEP_SIZES, STEP_COUNT, STEP_N = (1, 255, 256, 257, 1000), 40, 1000


@functools.lru_cache(maxsize=None)
def step_problem():
    """(x0 [n], gradients [T][n]) float32: seeded values, step 7 all zero, entries of 1e-20 and 1e+15 (the first elements among
    them, so that the one-element case sees both)."""
    x0 = (0.1 * synthetic.normalish(95, (STEP_N,), 59)).astype(np.float32)
    g = synthetic.normalish(96, (STEP_COUNT, STEP_N), 59).astype(np.float32)
    g[7] = 0.0
    tiny = synthetic.uniform(97, STEP_COUNT * STEP_N, 59).reshape(STEP_COUNT, STEP_N)
    g[tiny < 0.02] = 1e-20
    g[tiny > 0.98] = 1e+15
    g[3, 0], g[11, 0], g[12, 0] = 1e+15, 1e-20, -1e-20
    g[7] = 0.0
    return x0, g


@dataclass(frozen=True, eq=False)
class ReferenceStep:
    x64: np.ndarray         # [T][n] after every step
    m64: np.ndarray
    v64: np.ndarray
    e32: float              # x after the last step: torch float32 against the twin, over the whole problem
    floor: float

    @property
    def tol(self):
        return max(self.floor, ORDER_FACTOR * self.e32)


@functools.lru_cache(maxsize=None)
def reference_step(row: Row) -> ReferenceStep:
    """One reference for every n: the cases are prefixes of one 1000-element problem and e32 is taken over all of it, so that
    the one-element case does not gate on a single lane's luck (deliberate: it is looser than that lane's own e32, which can be
    zero by chance while the device's 1-ulp operations legitimately differ).  The floor is deliberately not Tier A's
    ``num_iters * lr * 4 * 2^-23``: a recorded gradient sequence with all-zero steps and outliers does not walk lr per step, so the
    floor is the same four ulp of the path the twin's longest-walking lane really walks (for all three rows that is less than
    ``num_iters * lr`` would give: ``test_adam_conditions.py`` asserts it)."""
    x0, g = step_problem()
    x64, m64, v64 = twin_on_gradients(x0, g, row)
    x32, _, _ = torch_on_gradients(x0, g, row, torch.float32)
    path = np.abs(np.diff(np.concatenate([x0[None].astype(np.float64), x64]), axis=0)).sum(axis=0).max()
    return ReferenceStep(x64, m64, v64, float(np.abs(x32 - x64[-1]).max()), float(4.0 * ULP * path))


MOMENT_MARGIN = 2.0         # on the worst-case count below, for what it leaves out (a contraction changes which intermediate rounds)


def moment_gates(row: Row):
    """[T][n] bounds for m and v from the twin's own moments, as recursions that decay like the moments do, so that a gate never
    outlives the gradient that widened it.  One float32 rounding is half an ulp (2^-24) of its result.

    m: ``m + w d`` below a weight w = 1 - beta1 of 0.5 and ``g - (1 - w) d`` from there on, d = g - m.  Rounded: d, its product
    with the coefficient u = min(w, 1 - w) (one ulp of u |d| together), the sum (half an ulp of the new m), and w itself where
    1 - beta1 is no float32 (half an ulp of w |d|); the error of the old m comes through times beta1.
    ``E_t = beta1 E_(t-1) + margin ulp (|m_t| / 2 + (u + w / 2) |d_t|)``; with beta1 = 0 that is an ulp of |g_t|.
    v: ``beta2 v + (1 - beta2) g g``: both coefficients, three products and the sum, at most two ulp of the new v.
    ``E_t = beta2 E_(t-1) + margin 2 ulp v_t``.  Both plus a few of the smallest normal float32, where a product (1e-20 squared)
    is flushed to zero."""
    _, g = step_problem()
    g = g.astype(np.float64)
    ref = reference_step(row)
    w = 1.0 - row.b1
    u = min(w, 1.0 - w)
    w_rounds = 0.0 if float(np.float32(w)) == w else 0.5 * w
    tiny = 4.0 * 2.0 ** -126
    gate_m, gate_v = np.zeros_like(g), np.zeros_like(g)
    em, ev, m_old = np.zeros(g.shape[1]), np.zeros(g.shape[1]), np.zeros(g.shape[1])
    for t in range(g.shape[0]):
        d = np.abs(g[t] - m_old)
        em = row.b1 * em + MOMENT_MARGIN * ULP * (0.5 * np.abs(ref.m64[t]) + (u + w_rounds) * d)
        ev = row.b2 * ev + MOMENT_MARGIN * 2.0 * ULP * ref.v64[t]
        gate_m[t], gate_v[t] = em + tiny, ev + tiny
        m_old = ref.m64[t]
    return gate_m, gate_v


# ---- Tier B --------------------------------------------------------------------------------------------------------------------
X_POSE_FIELDS = (("body_pose", 63), ("jaw_pose", 3), ("leye_pose", 3), ("reye_pose", 3), ("left_hand_pose", 45), ("right_hand_pose", 45))
TIER_B_ITERS = 24
TIER_B_FRAMES = 5
SURFACE_ITERS = 12
NUM_LANDMARKS = 5


@functools.lru_cache(maxsize=None)
def tier_b_case(kind: str, frames: int = TIER_B_FRAMES) -> F.Case:
    """``fit_gradient_common.base``: seeded frames, every term on, targets 12 cm off the start's joints; the preserve pose is the
    start (the oracle's fitters preserve the start) and there is no translation prior (the oracle's fitters have none)."""
    b = F.base(kind, B=frames, seed=61)
    return replace(b, name=f"adam/{kind}/full{frames}", weights=F.all_on(kind, transl=0.0), preserve=None, tr_target=None)


@functools.lru_cache(maxsize=None)
def landmark_table():
    return synthetic.make_landmarks(660, 55, NUM_LANDMARKS, seed=5)


class WithLandmarks:
    """The oracle's SMPL-X forward with the landmarks appended to its output joints (smplx: sum_k b_k v[ids_k])."""

    def __init__(self, model):
        self.model = model
        ids, bary = landmark_table()
        self.ids = torch.as_tensor(ids.reshape(-1), dtype=torch.long)
        self.bary = torch.as_tensor(bary, dtype=model.dtype)

    def __call__(self, **kw):
        out = self.model(**kw)
        tri = out.vertices[:, self.ids].reshape(out.vertices.shape[0], NUM_LANDMARKS, 3, 3)
        return SimpleNamespace(joints=torch.cat([out.joints, (tri * self.bary[None, :, :, None]).sum(dim=2)], dim=1), vertices=out.vertices)


@functools.lru_cache(maxsize=None)
def native_landmark_model():
    from keypoints2body_amd.native import NativeModel
    c = F.consts("smplx20")
    return NativeModel(c.v_template, c.shapedirs, c.posedirs, c.J_regressor, c.lbs_weights, c.parents, c.extra_vertex_ids, landmarks=landmark_table())


@functools.lru_cache(maxsize=None)
def surface_case(which: str) -> F.Case:
    """Tier B with one surface target behind the body's joints: "vertex" - SMPL, the first vertex-selected joint (the tail of
    ``k2b_vertex_term_kernel``); "landmark" - SMPL-X with a landmark table, its first landmark (``k2b_surface_term_kernel``)."""
    kind = "smpl10" if which == "vertex" else "smplx20"
    b = tier_b_case(kind, 3)
    lay = F.layout(kind)
    extras = len(F.consts(kind).extra_vertex_ids)
    j = lay.J if which == "vertex" else lay.J + extras
    model = oracle_model(kind, True, which == "landmark")
    with torch.no_grad():
        at = model(**oracle_params(kind, b.go, b.pose, b.shape, b.tr, torch.float64)).joints[:, j].numpy()
    tgt = (at + 0.05 * synthetic.normalish(98, (3, 3), 61)).astype(np.float32)
    K = 22
    return replace(b, name=f"adam/{which}", idx=tuple(range(K)) + (j,), j3d=np.ascontiguousarray(np.concatenate([b.j3d[:, :K], tgt[:, None]], axis=1)))


def oracle_model(kind: str, double: bool, landmarks: bool = False):
    m = F.oracle(kind, double)
    return WithLandmarks(m) if landmarks else m


def oracle_params(kind: str, go, pose, shape, tr, dtype) -> dict:
    t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)
    if not kind.startswith("smplx"):
        return dict(global_orient=t(go), body_pose=t(pose), betas=t(shape), transl=t(tr))
    p = dict(global_orient=t(go), transl=t(tr))
    at = 0
    for k, w in X_POSE_FIELDS:
        p[k] = t(pose)[:, at:at + w]
        at += w
    nb = F.layout(kind).betas_prior
    p["betas"], p["expression"] = t(shape)[:, :nb], t(shape)[:, nb:]
    return p


def oracle_fit(case: F.Case, row: Row, iters: int, double: bool, seq_ind: int = 1, landmarks: bool = False, start=None):
    """The oracle's fitter on the case: (packed parameters [B][P], loss [B]) as float64 arrays.  `start`: packed start [B][P]."""
    with one_thread():
        return _oracle_fit(case, row, iters, double, seq_ind, landmarks, start)


def _oracle_fit(case, row, iters, double, seq_ind, landmarks, start):
    from oracle.fit_torch import FitWeights, fit_world_adam, fit_world_adam_smplx
    kind, lay = case.kind, F.layout(case.kind)
    dt = torch.float64 if double else torch.float32
    w = case.weights
    fw = FitWeights(sigma=w["sigma"], pose_prior_weight=w["mixture"], shape_prior_weight=w["shape"], angle_prior_weight=w["bending"],
                    joint_loss_weight=w["joint"], pose_preserve_weight=w["preserve"])
    if start is None:
        go, pose, shape, tr = case.go, case.pose, case.shape, case.tr
    else:
        cols = native_columns(lay)
        go, pose, shape, tr = (np.asarray(start)[:, cols[k]] for k in ("global_orient", "body_pose", "betas", "transl"))
    p = oracle_params(kind, go, pose, shape, tr, dt)
    j3d = torch.as_tensor(case.j3d).to(dt)
    conf = None if case.conf is None else torch.as_tensor(case.conf).to(dt)
    model, prior = oracle_model(kind, double, landmarks), F.prior(double)
    if kind.startswith("smplx"):
        out, loss, _, _, _ = fit_world_adam_smplx(model, prior, p, j3d, conf, num_iters=iters, seq_ind=seq_ind, model_idx=list(case.idx), weights=fw,
                                                  **row.kw)
        pose_out = torch.cat([out[k] for k, _ in X_POSE_FIELDS], dim=1)
        packed = torch.cat([out["global_orient"], pose_out, out["betas"], out["expression"], out["transl"]], dim=1)
    else:
        o = fit_world_adam(model, prior, p["global_orient"], p["body_pose"], p["betas"], p["transl"], j3d, conf, num_iters=iters, seq_ind=seq_ind,
                           model_idx=list(case.idx), weights=fw, **row.kw)
        packed, loss = torch.cat([o.global_orient, o.body_pose, o.betas, o.transl], dim=1), o.loss
    return packed.double().numpy(), loss.double().numpy()


@dataclass(frozen=True, eq=False)
class ReferenceB:
    x32: np.ndarray         # the float32 oracle: what the device is gated against
    loss32: np.ndarray
    e32: float              # max |x32 - x64|


_references_b = {}


def reference_b(name: str, row_name: str) -> ReferenceB:
    """`name`: smpl10 | smplx20 | vertex | landmark | chain/smpl10/3_7 ... (``tier_b_names``)."""
    key = (name, row_name)
    if key not in _references_b:
        row = B_ROWS[row_name]
        if name.startswith("chain/"):
            _, kind, counts = name.split("/")
            first, follow = (int(c) for c in counts.split("_"))
            x32, l32 = oracle_chain(kind, row, first, follow, False)
            x64, _ = oracle_chain(kind, row, first, follow, True)
        else:
            surface = name in ("vertex", "landmark")
            case = surface_case(name) if surface else tier_b_case(name)
            iters = SURFACE_ITERS if surface else TIER_B_ITERS
            x32, l32 = oracle_fit(case, row, iters, False, landmarks=name == "landmark")
            x64, _ = oracle_fit(case, row, iters, True, landmarks=name == "landmark")
        _references_b[key] = ReferenceB(x32, l32, float(np.abs(x32 - x64).max()))
    return _references_b[key]


CHAIN_S, CHAIN_T = 3, 4
CHAIN_COUNTS = ((3, 7), (7, 3))                    # (num_iters, followup_iters): the follow-up count above the first, and swapped
CHAIN_KINDS = ("smpl10", "smplx20")


def tier_b_names():
    return ["smpl10", "smplx20", "vertex", "landmark"] + [f"chain/{k}/{a}_{b}" for k in CHAIN_KINDS for a, b in CHAIN_COUNTS]


@functools.lru_cache(maxsize=None)
def chain_case(kind: str) -> F.Case:
    """S sequences of T frames: the targets of S * T seeded frames (sequence s owns the frames s T .. s T + T - 1), the start of
    sequence s is that of its first frame."""
    return tier_b_case(kind, CHAIN_S * CHAIN_T)


def oracle_chain(kind: str, row: Row, first: int, follow: int, double: bool):
    """The oracle's frame loop: frame 0 from the start without the preserve term, every later frame from its predecessor's
    result with a fresh optimiser and the preserve term.  (packed [S][T][P], loss [S][T])."""
    case = chain_case(kind)
    heads = np.arange(CHAIN_S) * CHAIN_T
    x, losses, prev = [], [], None
    for t in range(CHAIN_T):
        one = F.replace(case, j3d=case.j3d[heads + t], go=case.go[heads], pose=case.pose[heads], shape=case.shape[heads], tr=case.tr[heads])
        prev, loss = oracle_fit(one, row, first if t == 0 else follow, double, seq_ind=t, start=prev)
        x.append(prev)
        losses.append(loss)
    return np.stack(x, axis=1), np.stack(losses, axis=1)


def fit_chain(case: F.Case, row: Row, first: int, follow: int, ragged: bool, start=None):
    """``native.fit_sequence`` (or ``fit_sequences`` with S equal lengths) on the chain case: (packed [S][T][P], loss [S][T])."""
    from keypoints2body_amd import native
    cfg = row.set(F.fit_config(case), first)
    heads = np.arange(CHAIN_S) * CHAIN_T
    ins = [H.cuda(a[heads]) for a in (case.go, case.pose, case.shape, case.tr)] if start is None else start
    K = case.j3d.shape[1]
    if ragged:
        out = native.fit_sequences(F.native_model(case.kind), H.native_prior(), cfg, follow, list(case.idx), [CHAIN_T] * CHAIN_S, H.cuda(case.j3d), None, *ins)
        out = {k: v.reshape((CHAIN_S, CHAIN_T) + tuple(v.shape[1:])) for k, v in out.items()}
    else:
        out = native.fit_sequence(F.native_model(case.kind), H.native_prior(), cfg, follow, list(case.idx),
                                  H.cuda(case.j3d.reshape(CHAIN_S, CHAIN_T, K, 3)), None, *ins)
    return torch.cat([out[k] for k in native.PARAM_KEYS], dim=2), out["loss"]


def gate_b(ref: ReferenceB, packed, loss, what: str) -> float:
    got = packed.detach().cpu().double().numpy()
    err = float(np.abs(got - ref.x32).max())
    print(f"adam gate {what}: deviation {err:.2e}  e32 {ref.e32:.2e}  gate {PARAM_TOL:.0e}")
    assert np.isfinite(got).all(), what
    assert err < PARAM_TOL, f"{what}: parameters {err:.2e} off the oracle's fitter"
    np.testing.assert_allclose(loss.detach().cpu().double().numpy(), ref.loss32, rtol=LOSS_RTOL, err_msg=what)
    return err
