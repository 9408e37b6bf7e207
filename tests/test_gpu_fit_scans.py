"""Subtree sums of the fused fit kernel's tree pass: fp32 chain / end scans (csrc/k2b_lanes.h, chain_end_scans) against their
run-time twin, the fp64 prefix differences.  A model created under ``K2B_FIT_SCAN64=1`` keeps the DFS lane placement and the
fp64 instantiation; the variable is set around the creation only (the switch is read there, per model).

The failure mode the fp32 form must not have: a subtree sum formed as a DIFFERENCE of fp32 prefixes carries an absolute error of
eps x the largest prefix, so a small gradient beside large ones elsewhere in the tree drowns.  The case below has exactly that: one
arm sits on its targets (gradient ~ 0) while pelvis and legs are a metre off."""
import copy
import functools

import numpy as np
import pytest
import torch

from tests import helpers as H

pytestmark = pytest.mark.gpu

PARAM_TOL = 1e-4                    # tests/test_gpu_parity.py
GRAD_GATE = 2e-5                    # tests/test_gpu_parity.py::test_fit_gradient_matches_autograd, of the largest entry
CASE = "amass_noisy_conf"
QUIET_ARM = (13, 16, 18, 20, 22)    # left collar .. left hand: a chain in the middle of the lanes, not an end-type subtree
LOUD = (0, 1, 2, 4, 5, 7, 8, 10, 11)
SWITCH = "K2B_FIT_SCAN64"
EPS = 2.0 ** -24


def _native(consts):
    from keypoints2body_amd.native import NativeModel
    return NativeModel(consts.v_template, consts.shapedirs, consts.posedirs, consts.J_regressor, consts.lbs_weights, consts.parents,
                       consts.extra_vertex_ids)


_twins = {}


def _twin(monkeypatch):
    if "smpl" not in _twins:
        with monkeypatch.context() as mp:
            mp.setenv(SWITCH, "1")
            _twins["smpl"] = _native(H.body_consts())
    return _twins["smpl"]


def _fit(model, d, num_iters, want_grad=False, shape="auto", pose_priors=True):
    """tests.helpers.native_fit on a given model handle (pose_priors=False: mixture and angle prior weights zero)"""
    from keypoints2body_amd import native
    cfg = native.default_fit_config()
    if not pose_priors:
        cfg.pose_prior_weight = cfg.angle_prior_weight = 0.0
    cfg.debug_launch_shape = H.LAUNCH_SHAPES[shape]
    cfg.num_iters = int(num_iters)
    cfg.pose_preserve_weight = 5.0 if int(d["seq_ind"]) > 0 else 0.0
    cfg.freeze_betas = int(d["freeze_betas"])
    conf = H.cuda(d["conf"]) if int(d["has_conf"]) else None
    return native.fit_world(model, H.native_prior(), cfg, H.case_indices(d), H.cuda(d["j3d"]), conf, H.cuda(d["init_global_orient"]),
                            H.cuda(d["init_body_pose"]), H.cuda(d["init_betas"]), H.cuda(d["init_transl"]), want_grad=want_grad)


@functools.lru_cache(maxsize=None)
def _prior64():
    p = copy.copy(H.oracle_prior())
    p.means, p.precisions, p.nll_weights = p.means.double(), p.precisions.double(), p.nll_weights.double()
    return p


@functools.lru_cache(maxsize=None)
def _quiet_arm_case(n):
    """n frames from the golden case (its rows repeated, the later copies' poses nudged), the quiet arm's targets on the model's
    current joints, pelvis and leg targets about a metre off.  Returns the case, the float64 autograd gradients [n][3 + 69 + 10 + 3]
    of the whole loss and of the loss without the mixture and angle priors, and M per frame: the largest, over the arm's joints j,
    of sum over the subtree of j of |g_k| + |p_k - p_j| |g_k|."""
    from oracle.fit_torch import FitWeights, frame_losses
    g = H.load_case(CASE)
    rows = np.arange(n) % g["j3d"].shape[0]
    rng = np.random.default_rng(5)
    d = {k: g[k] for k in ("category", "num_iters", "seq_ind", "has_conf", "freeze_betas", "conf")}
    for k in ("j3d", "init_global_orient", "init_body_pose", "init_betas", "init_transl"):
        d[k] = g[k][rows].copy()
    d["init_body_pose"] += (0.05 * rng.standard_normal(d["init_body_pose"].shape) * (np.arange(n)[:, None] >= g["j3d"].shape[0])).astype(np.float32)
    idx = H.case_indices(d)
    assert idx == list(range(22)) and int(d["seq_ind"]) == 0 and not int(d["freeze_betas"])
    t64 = lambda k: torch.tensor(d[k], dtype=torch.float64)
    model = H.oracle_model(double=True)
    with torch.no_grad():
        now = model(global_orient=t64("init_global_orient"), body_pose=t64("init_body_pose"), betas=t64("init_betas"),
                    transl=t64("init_transl")).joints[:, :22].numpy()
    arm = [j for j in QUIET_ARM if j < 22]
    d["j3d"][:, arm] = now[:, arm].astype(np.float32)
    d["j3d"][:, LOUD] = (now[:, LOUD] + np.array([0.9, -0.4, 0.6]) + 0.1 * rng.standard_normal((n, len(LOUD), 3))).astype(np.float32)
    g_refs = []
    for w in (FitWeights(), FitWeights(pose_prior_weight=0.0, angle_prior_weight=0.0)):
        go, bp, be, tr = (t64(k).requires_grad_() for k in ("init_global_orient", "init_body_pose", "init_betas", "init_transl"))
        joints = model(global_orient=go, body_pose=bp, betas=be, transl=tr).joints
        joints.retain_grad()
        lf = frame_losses(bp, bp.detach().clone(), be, joints[:, idx], t64("j3d"), _prior64(), torch.tensor(d["conf"], dtype=torch.float64),
                          w, False)
        lf.sum().backward()
        g_refs.append(torch.cat([go.grad, bp.grad, be.grad, tr.grad], dim=1).numpy())
    gk = np.linalg.norm(joints.grad.numpy()[:, :24], axis=-1)                  # [n][24], zero where a joint has no target
    p = joints.detach().numpy()[:, :24]
    M = np.zeros(n)
    for i, j in enumerate(QUIET_ARM):
        sub = list(QUIET_ARM[i:])
        M = np.maximum(M, (gk[:, sub] * (1.0 + np.linalg.norm(p[:, sub] - p[:, j:j + 1], axis=-1))).sum(axis=1))
    return d, g_refs[0], g_refs[1], M


@pytest.mark.parametrize("n,shape", [(3, "auto"), (9, "wide"), (17, "wide")])
def test_small_gradient_beside_large_ones_is_as_good_as_the_fp64_twins(monkeypatch, n, shape):
    """One closure (num_iters = 1, want_grad) against float64 autograd on the oracle.  3 frames: one tree per wave (split shape);
    9 and 17 frames in the 16-wave shape: two trees per wave, a wave with a padding slot, a second workgroup.
    Gate 1: the project's gradient gate, 2e-5 of the largest entry, with every loss term on.
    Gate 2, on the quiet arm's entries alone: |error of the fp32 scans| <= |error of the fp64 twin| + 8 x 2^-24 x M.  A chain sum has
    at most 5 terms, so its error is <= 4 x 2^-24 x sum |terms| (doubled as margin); everything else is shared by the two builds.
    fp32 prefix differences fail gate 2: their error is 2^-24 x the leg-sized prefixes, orders above M.
    Gate 2 runs with the mixture and the angle prior switched off: their share of an arm entry is ~1e3, added to the tree's share in
    fp32 in both builds, and one rounding of that sum (6e-5) is a thousand times the bound - with them on the gate would compare
    roundings of the priors, not the scans."""
    d, g_all, g_tree, M = _quiet_arm_case(n)
    grad = lambda model, priors: _fit(model, d, 1, want_grad=True, shape=shape, pose_priors=priors)["grad"].cpu().numpy().astype(np.float64)
    scale = np.abs(g_all).max()
    e_all = np.abs(grad(H.native_model(), True) - g_all)
    e_fast, e_twin = np.abs(grad(H.native_model(), False) - g_tree), np.abs(grad(_twin(monkeypatch), False) - g_tree)
    cols = np.concatenate([3 + 3 * (j - 1) + np.arange(3) for j in QUIET_ARM])
    bound = 8.0 * EPS * M[:, None]
    print(f"{n} frames, {shape}: largest entry {scale:.3e}, error of the whole gradient {e_all.max() / scale:.2e} of it; quiet arm "
          f"without the pose priors: largest entry {np.abs(g_tree[:, cols]).max():.3e}, error fp32 scans {e_fast[:, cols].max():.3e}, "
          f"fp64 twin {e_twin[:, cols].max():.3e}, 8 eps M {bound.min():.3e}..{bound.max():.3e}, worst excess over the twin "
          f"{(e_fast[:, cols] - e_twin[:, cols]).max():.3e}")
    assert e_all.max() / scale < GRAD_GATE
    assert max(e_fast.max(), e_twin.max()) / np.abs(g_tree).max() < GRAD_GATE
    assert (e_fast[:, cols] <= e_twin[:, cols] + bound).all()


def test_fp64_twin_meets_the_golden_and_the_fp32_scans_stay_beside_it(monkeypatch):
    """100 Adam iterations on a reference golden: the twin within PARAM_TOL of the reference fitter's parameters, and the default
    model within PARAM_TOL of the twin (measured: DESIGN.md 4.1)."""
    d = H.load_case(CASE)
    fast, twin = _fit(H.native_model(), d, d["num_iters"]), _fit(_twin(monkeypatch), d, d["num_iters"])
    worst = 0.0
    for key in ("global_orient", "body_pose", "betas", "transl"):
        assert np.abs(twin[key].cpu().numpy() - d["out_" + key]).max() < PARAM_TOL, key
        assert np.abs(fast[key].cpu().numpy() - d["out_" + key]).max() < PARAM_TOL, key
        worst = max(worst, float((fast[key] - twin[key]).abs().max()))
    print(f"{CASE}, {int(d['num_iters'])} iterations: fp32 scans and fp64 twin differ by at most {worst:.3e}")
    assert worst < PARAM_TOL


def test_tree_without_a_scan_plan_fits_on_the_fp64_path():
    """A 24-joint tree with a junction inside a leg has no plan (tests/test_fit_scan_plan.py): its model keeps the DFS placement
    and the fp64 scans, in every shape bit for bit, and its gradient meets the autograd gate."""
    from keypoints2body_amd import native, synthetic
    from oracle.fit_torch import FitWeights, frame_losses
    from oracle.smpl_torch import TorchSMPL
    parents = np.asarray(synthetic.SMPL_PARENTS).copy()
    parents[7] = 1
    consts = synthetic.make_body_model(seed=3, num_vertices=512, parents=parents)
    oracle, model = TorchSMPL(consts), _native(consts)
    B = 3
    p = synthetic.make_poses(B, seed=11)
    t = lambda x: torch.as_tensor(np.asarray(x), dtype=torch.float32)
    with torch.no_grad():
        j3d = (oracle(global_orient=t(p.global_orient), body_pose=t(p.body_pose), betas=t(p.betas), transl=t(p.transl)).joints[:, :24] + 0.01).contiguous()
    start = dict(go=t(p.global_orient) * 0.9, bp=t(p.body_pose) * 0.9, be=t(p.betas) * 0.5, tr=t(p.transl) + 0.02)
    res = {}
    for shape in ("split", "split_paired", "paired", "wide"):
        cfg = native.default_fit_config()
        cfg.num_iters = 1
        cfg.debug_launch_shape = H.LAUNCH_SHAPES[shape]
        res[shape] = native.fit_world(model, H.native_prior(), cfg, list(range(24)), j3d.cuda(), None, *(start[k].cuda().contiguous() for k in ("go", "bp", "be", "tr")),
                                      want_grad=True)
        assert torch.equal(res[shape]["grad"], res["split"]["grad"]), shape
    go, bp, be, tr = (start[k].clone().requires_grad_() for k in ("go", "bp", "be", "tr"))
    mo = oracle(global_orient=go, body_pose=bp, betas=be, transl=tr)
    frame_losses(bp, bp.detach().clone(), be, mo.joints[:, :24], j3d, H.oracle_prior(), torch.ones(24), FitWeights(), False).sum().backward()
    g_ref = torch.cat([go.grad, bp.grad, be.grad, tr.grad], dim=1).numpy()
    err = np.abs(res["split"]["grad"].cpu().numpy() - g_ref).max() / np.abs(g_ref).max()
    print(f"junction tree: gradient error {err:.2e} of the largest entry")
    assert err < GRAD_GATE
