"""Shared by the call-history tests (``tests/test_call_history_conditions.py``, ``tests/test_gpu_call_history.py``); importable
without a GPU (the device is touched inside functions only).

The contract (``include/k2b.h``, Conventions): what a call returns depends on its own arguments only, not on the
calls its handles, its thread or its stream served before.  The library keeps state between calls - grow-only LBS workspaces
addressed with the current call's padded frame count, LRU caches of Adam and surface tables, first-use tables, pinned staging per
thread, stream-ordered scratch of which only a part is cleared - and ``keypoints2body_amd.native`` hands every output out of
``torch.empty``.

The protocol, the same for every entry (``run_protocol``): R0 = X on fresh handles; then, per polluter, [polluter, NaN-filled and
freed tensors of the shapes of X's outputs, X again] on the same handles and stream with no host synchronisation of the test's
own in between (every device input is uploaded beforehand); then X on a second set of fresh handles.  Gate: every returned tensor
``torch.equal`` to R0.  Conditions, asserted: R0 finite; the NaN polluter's loss (or output) non-finite in every frame; the
polluter's batch larger than X's.

Polluters: "nan" - the same entry on a larger batch with a NaN in ``j3d`` / ``body_pose`` and ``-inf`` in ``transl`` of every
frame; "other" - the same entry on a larger batch of clean data from another seed, with more iterations (a longer, filled
L-BFGS history; more sequences) where the entry has them.  ``fminf`` / ``fmaxf`` / selects drop a NaN; a finite wrong value they
do not, and bit equality catches it.

Cases come from the existing commons: ``fit_gradient_common`` (F), ``isolation_common`` (I), ``lbs_layouts_common`` (L)."""
import re
from dataclasses import replace

import numpy as np
import torch

from keypoints2body_amd import synthetic
from tests import fit_gradient_common as F
from tests import helpers as H
from tests import isolation_common as I
from tests import lbs_layouts_common as L

NAN = float("nan")
ADAM_ITERS, ADAM_ITERS_OTHER = 3, 5
LBFGS = dict(max_iter=4, lr=1.0)                         # X: most history slots are never written
LBFGS_OTHER = dict(max_iter=12, lr=1.0, history_size=3)  # the polluter's ring of three is full after four iterations
SEED_X, SEED_OTHER = 47, 53                              # (47: the seed of isolation_common.fit_case)
FIT_POISONS = ("j3d_nan", "pose_nan", "transl_ninf")     # all three in every frame of the NaN polluter
LBS_POISONS = ("orient_nan", "pose_nan", "betas_nan", "transl_ninf")

# ---- sizes (tests/test_call_history_conditions.py holds them to the plan headers) ------------------------------------------------
# k2b_lbs: X, the polluter, X again, then two more row strides inside the grown buffer / a regrown one
LBS_X, LBS_POLLUTER, LBS_STRIDE, LBS_REGROW, LBS_RESERVE = 5, 133, 40, 200, 300
LBS_SEQUENCE = (LBS_X, LBS_POLLUTER, LBS_X, LBS_STRIDE, LBS_REGROW)
# one layout per route of lbs_layouts_common.TABLE: (J, NB, variant, route)
LBS_ROUTES = {"stream": (23, 10, "tagged", "stream"), "stream_x": (55, 21, "tagged", "stream_x"), "stream_xw": (56, 32, "tagged", "stream_xw"),
              "tile": (24, 16, "tagged", "tile")}
LBS_LANDMARKS = L.LANDMARK_LAYOUT + ("landmarks",)       # joints-only calls use the landmark workspace
BACKWARD_X, BACKWARD_POLLUTER = 3, 70
BACKWARD_LAYOUTS = ((24, 17, "tagged"), (56, 32, "tagged"), L.LANDMARK_LAYOUT + ("landmarks",))
ADAM_X, ADAM_POLLUTER = 5, 37
ADAM_KINDS = {"smpl10": (0, 1, 2, 3, 4), "smpl16": (0, 1, 2, 3, 4), "smplx20": (0, 1, 2), "tree21": (0, 1, 2)}   # kind -> debug_launch_shape
SURFACE_X, SURFACE_POLLUTER = 3, 9
SURFACE_ROUTES = ("extras", "landmarks")
SURFACE_FILLERS_EXTRA = 6                                # filler selections beyond the cache's size
LBFGS_CASES = ("lbfgs/persistent", "lbfgs/fused_rounds", "lbfgs/two_launches", "lbfgs/wide")
CHAIN_T, CHAIN_X, CHAIN_POLLUTER = I.CHAIN_FRAMES, 3, 37
RAGGED_POLLUTERS = (300, 700)                            # sequences: the pinned slot-table staging grows twice and is re-used once
CHAIN_KINDS = {"fused": ("smpl10", 0), "tree": ("smplx20", 2)}       # kernel -> (kind, debug_launch_shape)
SHARED_CHAIN_CASES = ("chain/fused", "chain/tree", "lbfgs/chain")     # isolation_common's: several chain slots per workgroup
PAIRS, POINTS = 257, 65                                  # no multiples of a block


def lbs_frames_padded(frames: int) -> int:
    """``k2b::lbs_frames_padded`` with its numbers read from ``csrc/k2b_lbs_plan.h``."""
    src = (L.CSRC / "k2b_lbs_plan.h").read_text()
    m = re.search(r"constexpr int lbs_frames_padded\(int num_frames\) \{ return \(num_frames \+ (\d+)\) / (\d+) \* (\d+); \}", src)
    add, div, mul = (int(g) for g in m.groups())
    return (frames + add) // div * mul


def surface_cache_size() -> int:
    """kMaxSurfaceTables of ``csrc/k2b_api_model.hip``: the surface tables a model handle keeps."""
    src = (L.CSRC / "k2b_api_model.hip").read_text()
    return int(re.search(r"constexpr size_t kMaxSurfaceTables = (\d+);", src).group(1))


def cache_schedule(size: int) -> dict:
    """Filler fits around the touches of S0 on a strict LRU cache of `size` tables.  "evicted": more fillers than the cache
    holds behind S0's only use, so its table leaves.  "kept": (before, after) the midway touch of S0 - together at least `size`,
    so that tables do leave, but at most `size` - 1 behind the touch, so that S0, the most recent entry then, never becomes the
    oldest of a full cache: the fillers in front of the touch leave, S0 stays and is re-used behind the evictions."""
    return {"evicted": (size + SURFACE_FILLERS_EXTRA,), "kept": (size // 2, size - 1)}


def surface_target_limit() -> int:
    src = (L.CSRC / "k2b_layout.h").read_text()
    return int(re.search(r"constexpr int kSurfMaxTargets = (\d+);", src).group(1))


def adam_launch_case(kind: str, shape: int, frames: int) -> I.LaunchCase:
    """The Adam X of `kind` in the forced shape as an ``isolation_common.LaunchCase`` (frames fixed, no CU term)."""
    return I.LaunchCase(f"history/{kind}/{shape}", F.layout(kind).kernel, kind, shape, 0, frames)


def lbfgs_sizes(name: str, cus: int):
    """(X frames, polluter frames): X at the case's own count (frames share a workgroup there), the polluter one frame per compute
    unit above it."""
    n = I.CASE[name].frames(cus)
    return n, n + cus


def chain_sizes(name: str, cus: int):
    """(X sequences, polluter sequences) of a chain case of ``isolation_common``: its own count, and one per compute unit more."""
    n = I.CASE[name].frames(cus)
    return n, n + cus


def filler_selections(J: int, E: int, num_landmarks: int, count: int, keep: tuple):
    """`count` distinct two-target selections (an extra joint, a landmark) as model joint indices, none of them `keep`."""
    out = []
    for l in range(num_landmarks):
        for e in range(E):
            s = (J + e, J + E + l)
            if s != tuple(keep) and s != tuple(reversed(keep)):
                out.append(s)
            if len(out) == count:
                return out
    raise ValueError(f"{E} extra joints x {num_landmarks} landmarks hold fewer than {count} selections")


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def fit_case(kind: str, frames: int, seed: int = SEED_X, mask: int = 15) -> F.Case:
    """``isolation_common.fit_case`` at another seed: every loss weight on, a per-frame confidence table."""
    b = F.base(kind, B=frames, seed=seed)
    K = b.j3d.shape[1]
    conf = (0.5 + synthetic.uniform(97, frames * K, seed).reshape(frames, K)).astype(np.float32)
    return replace(b, name=f"{kind}/history{frames}s{seed}", conf=conf, mask=mask)


def poison_all(case: F.Case) -> F.Case:
    for kind in FIT_POISONS:
        case = I.poison_fit_case(case, kind, range(case.frames))
    return case


def poison_all_lbs(params: tuple) -> tuple:
    for kind in LBS_POISONS:
        params = I.poison_lbs_params(params, kind, range(params[0].shape[0]))
    return params


def surface_inputs(route: str, frames: int, other: bool = False):
    """(joint index, targets [B][K][3], confidences [B][K], parameters) on the landmark layout as ``tests/test_gpu_isolation.py``
    builds them: every kinematic joint and three extra joints (the vertex kernel's route), with `route` "landmarks" every third
    landmark too (the surface kernel's).  `other`: the same at other scales (the polluter's clean data)."""
    J, NB = L.LANDMARK_LAYOUT
    p = L.backward_params(J, NB, frames, scales=(0.25, 0.15, 0.4, 0.25) if other else (0.3, 0.2, 0.5, F.TRANSL_SCALE))
    idx = list(range(J)) + [J, J + 2, J + 4]
    if route == "landmarks":
        first = J + L.NUM_EXTRA
        idx += list(range(first, first + L.landmarks(J, L.V_SMALL)[0].shape[0], 3))
    j64, _ = L._forward(J, NB, L.V_SMALL, "landmarks", p, True, True)
    K = len(idx)
    seed = 59 if other else 53
    tgt = (j64[:, idx].numpy() + F.TARGET_OFFSET * synthetic.normalish(98, (frames, K, 3), seed)).astype(np.float32)
    conf = (0.5 + synthetic.uniform(99, frames * K, seed).reshape(frames, K)).astype(np.float32)
    return idx, tgt, conf, p


def all_joint_targets(frames: int):
    """(targets [B][J + E + L][3] for every output joint of the landmark layout, confidences, parameters): the cache test picks
    its columns from them."""
    J, NB = L.LANDMARK_LAYOUT
    p = L.term_params(J, NB, frames)
    j64, _ = L._forward(J, NB, L.V_SMALL, "landmarks", p, True, True)
    n = j64.shape[1]
    tgt = (j64.numpy() + F.TARGET_OFFSET * synthetic.normalish(98, (frames, n, 3), 61)).astype(np.float32)
    conf = (0.5 + synthetic.uniform(99, frames * n, 61).reshape(frames, n)).astype(np.float32)
    return tgt, conf, p


def cotangents(J: int, NB: int, B: int, rows: int):
    rng = np.random.default_rng([J, NB, B, 7])
    return rng.standard_normal((B, rows, 3)).astype(np.float32), rng.standard_normal((B, L.V_SMALL, 3)).astype(np.float32)


# ---- fresh handles -----------------------------------------------------------------------------------------------------------
def fresh_model(kind: str):
    """A new ``NativeModel`` of ``fit_gradient_common.consts(kind)`` (not the cached one the other tests share)."""
    return F.native_model.__wrapped__(kind)


def fresh_lbs_model(J: int, NB: int, variant: str = "tagged", landmarks=None):
    from keypoints2body_amd.native import NativeModel
    c = L.consts(J, NB, L.V_SMALL, variant)
    if landmarks is None and variant == "landmarks":
        landmarks = L.landmarks(J, L.V_SMALL)
    return NativeModel(c.v_template, c.shapedirs, c.posedirs, c.J_regressor, c.lbs_weights, c.parents, c.extra_vertex_ids, landmarks=landmarks)


def fresh_prior():
    return H.native_prior.__wrapped__()


# ---- the protocol ------------------------------------------------------------------------------------------------------------
def to_host(out: dict) -> dict:
    return {k: v.detach().cpu() for k, v in out.items() if v is not None}


def nan_outputs(like: dict):
    """Allocate, fill with NaN and free tensors of exactly the shapes of `like`: the caching allocator hands the next
    ``torch.empty`` of such a shape one of these blocks (or another dirty one), so an element the entry does not write shows."""
    made = [torch.full(tuple(v.shape), NAN, dtype=v.dtype, device="cuda") if v.is_floating_point() else None for v in like.values()]
    del made


def assert_same(got: dict, want: dict, what: str):
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for k in sorted(want):
        a, b = got[k], want[k]
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k, tuple(a.shape), tuple(b.shape))
        if not torch.equal(a, b):
            bad = (a != b) | torch.isnan(a)
            rows = torch.nonzero(bad.reshape(bad.shape[0], -1).any(dim=1)).flatten().tolist() if a.dim() else [0]
            diff = float((a.double() - b.double()).abs().nan_to_num(nan=float("inf")).max())
            raise AssertionError(f"{what}: {k} differs from the first call on fresh handles in {int(bad.sum())} elements (rows {rows[:12]}, "
                                 f"by up to {diff:.3e}; NaN: {int(torch.isnan(a).sum())})")


def assert_finite(out: dict, what: str):
    for k, v in out.items():
        assert bool(torch.isfinite(v).all()), f"{what}: {k} of the first call is not finite"


def nonfinite_rows(t: torch.Tensor) -> torch.Tensor:
    """[rows] bool: the row holds a NaN or an infinity."""
    return (~torch.isfinite(t.reshape(t.shape[0], -1))).any(dim=1)


def run_protocol(make_handles, run_x, polluters, what: str, fresh_leg: bool = True, between=None):
    """`make_handles()` -> handles; `run_x(handles)` -> dict of device tensors, queued without a synchronisation of its own;
    `polluters`: (name, run(handles) -> dict, check(host dict) or None) - the check holds the polluter's own conditions.
    `between(handles)`: further calls between the polluter and X (refusals).  Returns R0 (host)."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    handles = make_handles()
    r0_dev = run_x(handles)                                          # kept alive: its blocks are not the ones X gets next
    r0 = to_host(r0_dev)
    assert_finite(r0, what)
    for name, pollute, check in polluters:
        p = pollute(handles)
        if between is not None:
            between(handles)
        nan_outputs(r0_dev)
        x = run_x(handles)
        torch.cuda.synchronize()
        assert_same(to_host(x), r0, f"{what} after the polluter '{name}'")
        if check is not None:
            check(to_host(p))
        del p, x
    if fresh_leg:                                                    # only the pool and the allocator are polluted here
        second = make_handles()
        nan_outputs(r0_dev)
        x = run_x(second)
        torch.cuda.synchronize()
        assert_same(to_host(x), r0, f"{what} on a second set of fresh handles")
    return r0


def all_rows_nonfinite(key: str, what: str):
    def check(out: dict):
        bad = nonfinite_rows(out[key])
        assert bool(bad.all()), f"{what}: {key} of the NaN polluter is finite in the rows {torch.nonzero(~bad).flatten().tolist()[:12]}: the poison did not go through"
    return check
