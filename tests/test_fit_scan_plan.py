"""The scan plan of the fused fit kernel (csrc/k2b_scan_plan.h), on the host: where every joint of a 24-joint tree sits in the 32
tree lanes and which of the two fp32 prefix scans yields its subtree sum.  Reached through the library's development entry
``k2b_dev_fit_scan_plan`` (no device needed, outside include/k2b.h).  The scans are replayed here lane by lane exactly as the
DPP steps move data - shifts inside rows of 16, sources outside the row read as zero, ``row_bcast:15`` into the odd rows - on
integer-valued inputs, where every sum is exact."""
import ctypes

import numpy as np

from keypoints2body_amd import native, synthetic

STEP1, STEP2, STEP4, END, CHAIN = 1, 2, 4, 8, 16      # k2b_scan_plan.h: kScan*


def _plan(parents):
    lib = native.load_library()
    fn = lib.k2b_dev_fit_scan_plan
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    par = np.ascontiguousarray(parents, np.int32)
    lane_of, flags = np.full(len(par), -1, np.int32), np.full(32, -1, np.int32)
    rc = fn(len(par), par.ctypes.data, lane_of.ctypes.data, flags.ctypes.data)
    return rc, lane_of, flags


def _subtrees(parents):
    J = len(parents)
    sub = [{j} for j in range(J)]
    for j in range(J - 1, 0, -1):
        sub[parents[j]] |= sub[j]
    return sub


def _shift_in_rows(x, s):
    """row_shr:s with bound_ctrl - lane l reads lane l - s of its own row of 16, zero from outside it"""
    out = np.zeros_like(x)
    for l in range(32):
        if (l & 15) >= s:
            out[l] = x[l - s]
    return out


def _replay(values_by_lane, flags):
    u = values_by_lane.copy()
    c = values_by_lane.copy()
    for s, bit in ((1, STEP1), (2, STEP2), (4, STEP4)):
        u = u + _shift_in_rows(u, s)
        c = c + _shift_in_rows(c, s) * ((flags & bit) != 0)
    u = u + _shift_in_rows(u, 8)
    u[16:] += u[15]                                     # row_bcast:15 into row 1
    return np.where((flags & END) != 0, u, c)


def test_smpl_plan_is_valid_and_its_scans_sum_every_subtree():
    parents = np.asarray(synthetic.SMPL_PARENTS)
    rc, lane_of, flags = _plan(parents)
    assert rc == 1
    J = len(parents)
    assert sorted(set(lane_of.tolist())) == sorted(lane_of.tolist()) and lane_of.min() >= 0
    assert lane_of.max() <= 30                          # lane 31 stays the identity source of the pointer-doubling rounds
    holes = sorted(set(range(32)) - set(lane_of.tolist()))
    assert all(flags[l] == 0 for l in holes)
    # the placement the tree pass is described with: right arm 0-4, left arm 5-9, head 10-11, spine 12-14, a hole, legs, root
    assert lane_of[[23, 21, 19, 17, 14]].tolist() == [0, 1, 2, 3, 4] and lane_of[[22, 20, 18, 16, 13]].tolist() == [5, 6, 7, 8, 9]
    assert lane_of[[15, 12]].tolist() == [10, 11] and lane_of[[9, 6, 3]].tolist() == [12, 13, 14] and 15 in holes
    assert lane_of[[11, 8, 5, 2]].tolist() == [16, 17, 18, 19] and lane_of[[10, 7, 4, 1]].tolist() == [20, 21, 22, 23] and lane_of[0] == 24
    sub = _subtrees(parents)
    for j in range(J):
        f = int(flags[lane_of[j]])
        assert f & (END | CHAIN), f"joint {j} is neither chain-type nor end-type"
        if f & CHAIN:                                   # a chain: consecutive lanes up to the joint's, inside one row of 16
            lanes = sorted(lane_of[k] for k in sub[j])
            assert lanes == list(range(lane_of[j] - len(lanes) + 1, lane_of[j] + 1)) and len(lanes) <= 8
            assert lanes[0] >> 4 == lanes[-1] >> 4, f"the chain of joint {j} crosses a row"
    rng = np.random.default_rng(0)
    for _ in range(8):
        x = rng.integers(-1000, 1000, J).astype(np.float64)
        by_lane = np.zeros(32)
        by_lane[lane_of] = x
        got = _replay(by_lane, flags)
        for j in range(J):
            assert got[lane_of[j]] == x[sorted(sub[j])].sum(), f"joint {j}"


def test_other_trees_with_a_plan_sum_every_subtree_too():
    """The plan is a function of the parent table, not of SMPL: a tree with longer and shorter limbs and a second spine branch."""
    parents = np.array([-1, 0, 1, 2, 3, 4, 5, 6, 0, 8, 0, 10, 11, 12, 13, 12, 15, 16, 17, 18, 19, 12, 21, 22])
    rc, lane_of, flags = _plan(parents)
    assert rc == 1 and lane_of.max() <= 30
    sub = _subtrees(parents)
    x = np.random.default_rng(1).integers(-1000, 1000, len(parents)).astype(np.float64)
    by_lane = np.zeros(32)
    by_lane[lane_of] = x
    got = _replay(by_lane, flags)
    for j in range(len(parents)):
        assert got[lane_of[j]] == x[sorted(sub[j])].sum(), f"joint {j}"
        if flags[lane_of[j]] & CHAIN:
            lanes = [lane_of[k] for k in sub[j]]
            assert min(lanes) >> 4 == max(lanes) >> 4


def test_trees_without_a_plan_are_refused():
    """They keep the DFS placement and the fp64 scans (k2b_model_create: no plan = fit_scan64)."""
    junction = np.asarray(synthetic.SMPL_PARENTS).copy()
    junction[7] = 1                                     # joint 1 has two children: a junction inside the left leg
    rc, lane_of, flags = _plan(junction)
    assert rc == 0 and (lane_of == -1).all() and (flags == -1).all()       # refused, nothing written
    long_chain = np.arange(-1, 23)                      # one chain of 24 joints: more than a masked scan covers
    assert _plan(long_chain)[0] == 0
    bad = np.asarray(synthetic.SMPL_PARENTS).copy()
    bad[5] = 9                                          # not a parent table (parent after child)
    assert _plan(bad)[0] == -1
