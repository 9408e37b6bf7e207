"""Shared by the isolation tests (``tests/test_isolation_host.py``, ``tests/test_gpu_isolation.py``); importable without a GPU.

The contract (``include/k2b.h``, Conventions): every output of a frame (of a sequence, in the chain entries) depends on that frame's
own inputs only, even when another frame's inputs are NaN or +-Inf; a frame whose loss depends on a non-finite input reports a
non-finite ``loss_out``; the stand-alone terms and the LBS pair are non-finite wherever the float64 oracle is.  The kernels share
hardware between frames (two frames on the halves of a wave, one arg-min reduction for both, sixteen frames as the columns of one
MFMA, component waves serving four frame waves, chain slots and L-BFGS instances in one workgroup, 32 frames in one LBS tile), so
a select written as a multiply by zero, a reduction that mixes the halves of a wave or a minimum that drops a NaN on one side only
would corrupt a clean neighbour without any finite-data test noticing.

A test is a pair of calls with the same batch, positions and config: one clean, one with a few frames poisoned.  The gates are
exact: every tensor of every clean frame ``torch.equal`` between the two calls; every poisoned frame non-finite where the case says
(its loss, or the elements where the float64 oracle of that frame is non-finite).  No tolerances.

Where the poisoned frames sit follows from the frames per workgroup W of the case's launch plan (``workgroup_frames``: the rules of
``csrc/k2b_launch_plan.h`` restated; ``tests/host/isolation_plan.cpp`` prints the header's own plans and the host test holds the
two together, so that a change of the launch policy cannot turn these tests into one workgroup per frame unnoticed): slot 0 of
workgroup 0, an odd slot in the middle, the last slot of a full workgroup - and, as a second variant, the first frame of the ragged
last workgroup.  No two poisoned frames share a wave; at least one full workgroup stays entirely clean.

``preserve_pose`` and ``transl_prior_target`` are never poisoned: with their weight at zero torch gives ``0 * nan = nan``, which is
no case worth a contract."""
import dataclasses
from dataclasses import dataclass, replace

import numpy as np
import torch

from tests import fit_gradient_common as F
from tests import lbs_layouts_common as L

NAN, INF = float("nan"), float("inf")


# ---- poison kinds ------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Poison:
    field: str              # attribute of fit_gradient_common.Case / position in the LBS parameter tuple / "cot"
    element: tuple          # index inside the frame
    value: float


POISONS = {
    "j3d_nan": Poison("j3d", (5, 1), NAN),
    "j3d_inf": Poison("j3d", (5, 1), INF),
    "conf_nan": Poison("conf", (7,), NAN),                 # conf_per_frame = 1
    "pose_nan": Poison("pose", (10,), NAN),
    "betas_nan": Poison("shape", (2,), NAN),
    "transl_ninf": Poison("tr", (0,), -INF),
    "orient_nan": Poison("go", (1,), NAN),                 # LBS only
    "cot_nan": Poison("cot", (40, 2), NAN),                # backward only: an entry of grad_vertices
}
FIT_POISONS = ("j3d_nan", "j3d_inf", "conf_nan", "pose_nan", "betas_nan", "transl_ninf")
LBS_POISONS = ("orient_nan", "pose_nan", "betas_nan", "transl_ninf")
TERM_POISONS = ("j3d_nan", "pose_nan", "transl_ninf")
LBS_FIELDS = {"go": 0, "pose": 1, "shape": 2, "tr": 3}


def poisoned(a: np.ndarray, frames, element: tuple, value: float) -> np.ndarray:
    """A copy of `a` with `value` at `element` of every frame of `frames`."""
    out = np.array(a, copy=True)
    for f in frames:
        out[(int(f),) + tuple(element)] = value
    return out


def poison_fit_case(case: F.Case, kind: str, frames) -> F.Case:
    p = POISONS[kind]
    return replace(case, name=f"{case.name}/{kind}", **{p.field: poisoned(getattr(case, p.field), frames, p.element, p.value)})


def poison_lbs_params(params: tuple, kind: str, frames) -> tuple:
    p = POISONS[kind]
    i = LBS_FIELDS[p.field]
    return tuple(poisoned(a, frames, p.element, p.value) if k == i else a for k, a in enumerate(params))


def poison_term_case(case: L.TermCase, kind: str, frames) -> L.TermCase:
    """A stand-alone term: `j3d` is its target array."""
    p = POISONS[kind]
    if p.field == "j3d":
        return replace(case, targets=poisoned(case.targets, frames, (1, 1), p.value))
    return replace(case, params=poison_lbs_params(case.params, kind, frames))


# ---- fit inputs --------------------------------------------------------------------------------------------------------------
def fit_case(kind: str, frames: int, mask: int = 15) -> F.Case:
    """`frames` distinct seeded frames of ``fit_gradient_common.base`` with every loss weight on (the tree kernel has no translation
    prior) and a per-frame confidence table in 0.5 .. 1.5."""
    from keypoints2body_amd import synthetic
    b = F.base(kind, B=frames, seed=47)
    K = b.j3d.shape[1]
    conf = (0.5 + synthetic.uniform(97, frames * K, 47).reshape(frames, K)).astype(np.float32)
    return replace(b, name=f"{kind}/isolation{frames}/mask{mask}", conf=conf, mask=mask)


def rows_of(case: F.Case, frames) -> F.Case:
    """The frames `frames` of a case as a case of their own (for the oracle)."""
    r = [int(f) for f in frames]
    pick = lambda a: None if a is None else a[r]
    return replace(case, name=f"{case.name}/rows", j3d=case.j3d[r], go=case.go[r], pose=case.pose[r], shape=case.shape[r], tr=case.tr[r],
                   conf=pick(case.conf) if case.conf is not None and case.conf.ndim == 2 else case.conf, preserve=pick(case.preserve),
                   tr_target=pick(case.tr_target))


def fit_oracle_masks(case: F.Case, frames) -> dict:
    """{"loss": [n] bool, "grad": [n][P] bool}: where the float64 oracle of the poisoned frames is non-finite (columns outside the
    optimiser are zero there, hence never in the mask)."""
    loss, grad = F.oracle_eval(rows_of(case, frames), True)
    return {"loss": ~np.isfinite(loss), "grad": ~np.isfinite(grad)}


def term_oracle_masks(case: L.TermCase, frames) -> dict:
    r = [int(f) for f in frames]
    sub = replace(case, params=tuple(a[r] for a in case.params), targets=case.targets[r], conf=case.conf[r] if case.conf.ndim == 2 else case.conf)
    loss, grad = L.term_oracle(sub, True)
    return {"loss": ~np.isfinite(loss), "grad": ~np.isfinite(grad)}


def lbs_oracle_masks(J, NB, variant, params, frames, want_vertices=True) -> dict:
    r = [int(f) for f in frames]
    joints, verts = L._forward(J, NB, L.V_SMALL, variant, tuple(a[r] for a in params), True, True)
    out = {"joints": ~np.isfinite(joints.numpy())}
    if want_vertices:
        out["vertices"] = ~np.isfinite(verts.numpy())
    return out


def lbs_backward_oracle_masks(J, NB, params, cot_joints, cot_verts, frames) -> dict:
    r = [int(f) for f in frames]
    g = L.oracle_grads(J, NB, L.V_SMALL, "tagged", tuple(a[r] for a in params), cot_joints[r], cot_verts[r], True)
    return {k: ~np.isfinite(v.numpy()) for k, v in g.items()}


# ---- launch cases ------------------------------------------------------------------------------------------------------------
FUSED_CAPACITY = {1: 4, 2: 8, 3: 16, 4: 16}              # frame slots of the forced shapes split, split-paired, paired, wide
FUSED_SHAPE_NAMES = {1: "split", 2: "split_paired", 3: "paired", 4: "wide"}
CHAIN_FRAMES = 3                                         # T of the k2b_fit_sequence cases
HOST_CU_COUNTS = (64, 256, 304)


@dataclass(frozen=True)
class LaunchCase:
    name: str
    entry: str            # fused | tree | chain_fused | chain_tree | lbfgs_fused | lbfgs_tree | chain_lbfgs
    kind: str             # model of fit_gradient_common
    shape: int            # k2b_fit_config.debug_launch_shape
    per_cu: int           # frames (sequences in a chain) = per_cu * CUs + extra
    extra: int
    scheme: str = ""      # the L-BFGS scheme the case names

    def frames(self, cus: int) -> int:
        return self.per_cu * cus + self.extra


def _cases():
    out = [LaunchCase(f"fused/{FUSED_SHAPE_NAMES[s]}", "fused", "smpl10", s, 0, 2 * FUSED_CAPACITY[s] + 1) for s in (1, 2, 3, 4)]
    out += [LaunchCase(f"tree/{kind}/{'plain' if s == 1 else 'comp_waves'}", "tree", kind, s, 4, 3)
            for kind in ("smplx20", "smplx32", "tree21") for s in (1, 2)]
    out += [LaunchCase("chain/fused", "chain_fused", "smpl10", 0, 4, 1), LaunchCase("chain/tree", "chain_tree", "smplx20", 2, 4, 1)]
    out += [LaunchCase("lbfgs/persistent", "lbfgs_fused", "smpl10", 0, 2, -1, "persistent"),
            LaunchCase("lbfgs/fused_rounds", "lbfgs_fused", "smpl10", 0, 3, -1, "fused_rounds"),
            LaunchCase("lbfgs/two_launches", "lbfgs_fused", "smpl10", 0, 5, -1, "two_launches"),
            LaunchCase("lbfgs/wide", "lbfgs_tree", "smplx32", 0, 2, -1, "two_launches"),
            LaunchCase("lbfgs/chain", "chain_lbfgs", "smpl10", 0, 2, 1, "persistent")]
    return tuple(out)


CASES = _cases()
CASE = {c.name: c for c in CASES}


def _ceil_div(a, b):
    return -(-a // b)


def workgroup_frames(case: LaunchCase, cus: int):
    """(frames per workgroup W, two frames per wave?) of the case's launch at `cus` compute units: ``plan_fit_world`` /
    ``plan_fit_tree`` / ``lbfgs_scheme_for`` of ``csrc/k2b_launch_plan.h`` restated for exactly these cases."""
    n = case.frames(cus)
    per = _ceil_div(n, cus)
    if case.entry == "fused":                            # a forced shape with fewer frames than CUs fills its slots
        assert n < cus
        return min(n, FUSED_CAPACITY[case.shape]), case.shape >= 2
    if case.entry in ("tree", "chain_tree", "lbfgs_tree"):
        tw = min(max(per, 1), 8)
        return (min(tw, 4) if case.shape == 2 else tw), False
    if case.entry == "chain_fused":                      # one split-shape slot per sequence
        return min(per, 4), False
    if case.entry == "chain_lbfgs":                      # the persistent launch: two optimisers per workgroup
        return min(per, 2), False
    if case.entry == "lbfgs_fused":
        if per <= 4:                                     # persistent (<= 2) and fused rounds (<= 4): the split shape
            return per, False
        return min(per, 8 if per <= 8 else 16), True     # two launches: the closure in the automatic shape (split-paired, wide)
    raise ValueError(case.entry)


def lbfgs_scheme(case: LaunchCase, cus: int) -> str:
    per = _ceil_div(case.frames(cus), cus)
    if case.entry == "lbfgs_tree":
        return "two_launches"
    if case.entry == "chain_lbfgs":                      # the frame loop runs inside the persistent launch, whatever the count
        return "persistent"
    return "persistent" if per <= 2 else "fused_rounds" if per <= 4 else "two_launches"


@dataclass(frozen=True)
class Positions:
    frames: tuple         # poisoned frames (sequences)
    slots: tuple          # their slot in their workgroup
    workgroups: tuple     # their workgroup
    W: int
    grid: int
    tail: int             # frames of the last workgroup


def positions(W: int, n: int, variant: str) -> Positions:
    """`variant` "body": slot 0, an odd slot in the middle and the last slot - in workgroup 0 where W >= 4 leaves them clean
    neighbours there, else in the workgroups 0, 1, 2; "tail": the first frame of the last workgroup."""
    grid = _ceil_div(n, W)
    tail = n - (grid - 1) * W
    if variant == "tail":
        wgs, slots = (grid - 1,), (0,)
    else:
        slots = tuple(sorted({0, min((W // 2) | 1, W - 1), W - 1}))
        wgs = tuple(0 for _ in slots) if W >= 4 else tuple(range(len(slots)))
    return Positions(tuple(w * W + s for w, s in zip(wgs, slots)), slots, wgs, W, grid, tail)


def check_positions(p: Positions, pairs: bool, variant: str):
    """What every case promises about its poisoned frames (asserted for three CU counts by the host test, and for the device's own
    by the GPU tests)."""
    n_full = p.grid - 1 if p.tail < p.W else p.grid
    assert p.W >= 2, "one frame per workgroup: nothing is shared"
    assert len(set(p.frames)) == len(p.frames)
    if variant == "tail":
        assert p.tail < p.W, f"the last workgroup is full ({p.tail} of {p.W})"
        assert p.frames == ((p.grid - 1) * p.W,) and n_full >= 1
        return
    assert 0 in p.slots and p.W - 1 in p.slots and any(s % 2 == 1 for s in p.slots)
    assert all(w < n_full for w in p.workgroups), "a poisoned frame of the body variant sits in the ragged workgroup"
    assert n_full > len(set(p.workgroups)), "no full workgroup is entirely clean"
    for w in set(p.workgroups):
        mine = [s for s, g in zip(p.slots, p.workgroups) if g == w]
        assert len(mine) < p.W, "a workgroup without a clean frame"
        if pairs:
            assert all((s ^ 1) not in mine for s in mine), "two poisoned frames are wave partners"


def case_positions(case: LaunchCase, cus: int, variant: str) -> Positions:
    W, pairs = workgroup_frames(case, cus)
    p = positions(W, case.frames(cus), variant)
    check_positions(p, pairs, variant)
    return p


# ---- the comparison ----------------------------------------------------------------------------------------------------------
def loss_nonfinite(count: int) -> dict:
    return {"loss": np.ones(count, dtype=bool)}


def assert_isolated(clean_out: dict, poisoned_out: dict, poisoned_frames, must_be_nonfinite: dict, what: str = ""):
    """`clean_out`, `poisoned_out`: name -> tensor with the frames in the leading dimension, results of two calls with the same batch,
    positions and config.  Every tensor of every frame outside `poisoned_frames` must be ``torch.equal`` between them (a NaN in a
    clean frame is unequal to itself: it fails).  `must_be_nonfinite`: name -> bool array [len(poisoned_frames), ...]; where it is
    true, that element of the poisoned frame must be NaN or +-Inf in `poisoned_out`.  Exact: no tolerances."""
    bad = sorted(int(f) for f in poisoned_frames)
    assert set(clean_out) == set(poisoned_out), (what, sorted(clean_out), sorted(poisoned_out))
    for k in sorted(clean_out):
        a, b = clean_out[k], poisoned_out[k]
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k, tuple(a.shape), tuple(b.shape))
        keep = torch.ones(a.shape[0], dtype=torch.bool)
        keep[bad] = False
        keep = keep.to(a.device)
        if torch.equal(a[keep], b[keep]):
            continue
        # which clean frame, for the message
        same = (a.reshape(a.shape[0], -1) == b.reshape(b.shape[0], -1)).all(dim=1).cpu()
        leaked = [int(f) for f in torch.nonzero(~same).flatten().tolist() if f not in bad]
        raise AssertionError(f"{what}: {k} of the clean frames {leaked[:12]} differs between the clean and the poisoned call "
                             f"(poisoned frames {bad})")
    for k, mask in must_be_nonfinite.items():
        got = poisoned_out[k][bad].detach().cpu()
        m = torch.as_tensor(np.asarray(mask)).reshape(got.shape)
        wrong = m & torch.isfinite(got)
        if bool(wrong.any()):
            where = torch.nonzero(wrong)[0].tolist()
            raise AssertionError(f"{what}: {k} of the poisoned frame {bad[where[0]]} is finite ({float(got[tuple(where)]):.6g}) at {where[1:]}, "
                                 f"where it has to be non-finite ({int(wrong.sum())} such elements)")


def flatten_chain(out: dict) -> dict:
    """(S, T, ...) results as (S * T, ...): frame s * T + t."""
    return {k: v.reshape((v.shape[0] * v.shape[1],) + tuple(v.shape[2:])) for k, v in out.items()}
