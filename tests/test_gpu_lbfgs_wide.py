"""GPU: the device-resident L-BFGS on models with more than 192 parameters per frame - the step kernel's wide form, four
vector elements per lane (``csrc/k2b_lbfgs_device.h``; ``k2b_lbfgs_step_kernel<4>``), for the 55-joint tree with 26 and 32 shape
coefficients: P = 3 + 162 + NB + 3 = 194 (the first size over the narrow form's 192; 16 betas | 10 expression coefficients is
the layout of the AMASS SMPL-X files) and 200 (the most the model layer takes).

What is pinned, as ``tests/test_gpu_lbfgs.py`` pins the narrow form: the CPU twin ``core/lbfgs_batched.py`` on the same closure
over the first iterations; independence of a frame from its batch; the history pairs beyond the staged ones (at P > 192 a pair is
2 KiB and the 48 KiB budget stages 23 of the 30 pairs of the reference's default ``max_iter = 30``: the two-loop recursion reads
the rest from global memory - compared against staging capped at 4 and at 0 pairs through ``K2B_LBFGS_STAGE_PAIRS``);
parameters outside the optimiser; loss and gradient at the result; the warm-start sequence; the fitter class with both drivers;
the batched shape pre-pass.

Targets come from the oracle's CPU forward of the same constants, not from ``NativeModel.lbs``: ``k2b_lbs`` stages at most 512
features (486 pose-corrective + NB + 2), so it skins a 55-joint model with up to 24 shape coefficients only.  For the same
reason the entries that end in the final forward (``fit_frame``, ``optimize_params_frame`` / ``_sequence`` / ``_sequences``) are
not exercised here; what is, runs without it (``fit_world_lbfgs``, ``fit_sequence_lbfgs``, ``fit_batch(run_forward=False)``,
the shape passes).

No 63-joint case: there is no forward to make targets from at that size either; P <= 256 covers it (P = 224 at most) by
construction.  Measured device - twin differences: DESIGN.md section 4.7."""
import os

import numpy as np
import pytest
import torch

from keypoints2body_amd import native, synthetic
from tests import helpers as H

pytestmark = pytest.mark.gpu

KEYS = ("global_orient", "body_pose", "betas", "transl")
NUM_BETAS = {26: 16, 32: 22}                 # shape coefficients -> betas (the rest: 10 expression coefficients)
MODEL_SEED = {26: 0, 32: 0}
STAGE_SWITCH = "K2B_LBFGS_STAGE_PAIRS"
_cache = {}


def _consts(nb):
    if ("consts", nb) not in _cache:
        _cache["consts", nb] = synthetic.make_body_model_x(MODEL_SEED[nb], num_vertices=1100, num_shape=nb)
    return _cache["consts", nb]


def _model(nb):
    if ("model", nb) not in _cache:
        c = _consts(nb)
        _cache["model", nb] = native.NativeModel(c.v_template, c.shapedirs, c.posedirs, c.J_regressor, c.lbs_weights, c.parents,
                                                 c.extra_vertex_ids)
    return _cache["model", nb]


def _oracle(nb):
    """The CPU forward of the same constants: ``k2b_lbs`` stages at most 512 features (486 pose-corrective + NB + 2), so it skins
    a 55-joint model up to 24 shape coefficients only - the targets of the wider models come from the oracle's forward."""
    if ("oracle", nb) not in _cache:
        from oracle.smpl_torch import TorchSMPLX
        _cache["oracle", nb] = TorchSMPLX(_consts(nb), num_betas=NUM_BETAS[nb])
    return _cache["oracle", nb]


def _joints(nb, go, pose, shape, tr):
    """(B, 55, 3) kinematic joints on the device; pose = the kernel's packed 162 values, shape = betas | expression."""
    t = lambda x: torch.as_tensor(np.asarray(x), dtype=torch.float32)
    go, pose, shape, tr = t(go), t(pose), t(shape), t(tr)
    k = NUM_BETAS[nb]
    with torch.no_grad():
        j = _oracle(nb)(global_orient=go, body_pose=pose[:, :63], jaw_pose=pose[:, 63:66], leye_pose=pose[:, 66:69], reye_pose=pose[:, 69:72],
                        left_hand_pose=pose[:, 72:117], right_hand_pose=pose[:, 117:162], betas=shape[:, :k], expression=shape[:, k:],
                        transl=tr, return_verts=False).joints[:, :55]
    return j.cuda().contiguous()


def _cfg(nb):
    cfg = native.default_fit_config()
    cfg.prior_pose_dims, cfg.num_betas_prior = 63, NUM_BETAS[nb]
    return cfg


def _problem(nb, B, seed=4):
    """55 kinematic joints of random parameters as targets; the start: zeros and the root-aligned translation."""
    if ("problem", nb, B, seed) in _cache:
        return _cache["problem", nb, B, seed]
    rng = np.random.default_rng(seed)
    go, pose, shape, tr = (0.2 * rng.standard_normal((B, 3)), 0.15 * rng.standard_normal((B, 162)), 0.3 * rng.standard_normal((B, nb)),
                           rng.standard_normal((B, 3)))
    j3d = _joints(nb, go, pose, shape, tr)
    z = lambda c: torch.zeros(B, c, device="cuda")
    tr0 = (j3d[:, 0] - _joints(nb, np.zeros((1, 3)), np.zeros((1, 162)), np.zeros((1, nb)), np.zeros((1, 3)))[:, 0]).contiguous()
    _cache["problem", nb, B, seed] = (j3d, (z(3), z(162), z(nb), tr0))
    return _cache["problem", nb, B, seed]


def _rows(init, sl):
    return [t[sl].contiguous() for t in init]


def _fit(nb, j3d, init, max_iter, cfg=None, **kw):
    return native.fit_world_lbfgs(_model(nb), H.native_prior(), cfg if cfg is not None else _cfg(nb), list(range(55)), j3d, None, *init,
                                  max_iter=max_iter, lr=1e-2, **kw)


def _evaluate(nb, cfg, j3d, point, preserve, want_grad=True):
    """One evaluate-only launch of the tree kernel: loss (and gradient) at `point`."""
    c = native.default_fit_config()
    for f, _ in native.FitConfigC._fields_:
        setattr(c, f, getattr(cfg, f))
    c.num_iters, c.step_size = 1, 0.0
    return native.fit_world(_model(nb), H.native_prior(), c, list(range(55)), j3d, None, *point, preserve_pose=preserve, want_grad=want_grad)


def _host_twin(nb, cfg, j3d, init, max_iter):
    """``BatchedLBFGS`` (numpy, float32 vectors) driving the same evaluate-only launches."""
    from keypoints2body_amd.core.lbfgs_batched import BatchedLBFGS
    preserve = init[1].clone()
    D = init[1].shape[1]

    def evaluate(x):
        xt = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
        r = _evaluate(nb, cfg, j3d, (xt[:, 0:3].contiguous(), xt[:, 3:3 + D].contiguous(), xt[:, 3 + D:3 + D + nb].contiguous(),
                                     xt[:, 3 + D + nb:].contiguous()), preserve)
        return r["loss"].cpu().numpy().astype(np.float64), r["grad"].cpu().numpy()

    opt = BatchedLBFGS(evaluate, torch.cat(init, dim=1).cpu().numpy(), lr=1e-2, max_iter=max_iter, history_size=100)
    return opt.run(), opt.rounds


def _cat(out):
    return torch.cat([out[k] for k in KEYS], dim=1)


# ---- 1. the CPU twin ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_iter", [1, 2, 3, 5])
@pytest.mark.parametrize("nb", [26, 32])
def test_wide_device_lbfgs_follows_the_cpu_twin_over_the_first_iterations(nb, max_iter):
    B = 12
    j3d, init = _problem(nb, B)
    assert 3 + 162 + nb + 3 > 192
    cfg = _cfg(nb)
    x_dev = _cat(_fit(nb, j3d, init, max_iter)).cpu().numpy()
    x_host, rounds = _host_twin(nb, cfg, j3d, init, max_iter)
    assert rounds <= max_iter * 5 // 4 + 2
    moved = np.abs(x_host - torch.cat(init, dim=1).cpu().numpy()).max()
    dev = np.abs(x_dev - x_host).max()
    print(f"NB {nb} (P {168 + nb}) max_iter {max_iter}: twin moved the start by {moved:.3e}, device - twin {dev:.3e}")
    assert moved > 1e-4                                   # the optimiser did something
    assert dev < 2e-5 * max(1.0, max_iter / 2), (nb, max_iter, dev)


# ---- 2. batch independence ------------------------------------------------------------------------------------------------------
def test_wide_device_lbfgs_frames_are_independent_of_their_batch():
    j3d, init = _problem(26, 40, seed=5)
    run = lambda sl: _fit(26, j3d[sl].contiguous(), _rows(init, sl), 30)
    full, again = run(slice(0, 40)), run(slice(0, 40))
    one, mid = run(slice(7, 8)), run(slice(20, 33))
    for k in KEYS + ("loss",):
        assert torch.equal(full[k], again[k]), k
        assert torch.equal(full[k][7:8], one[k]), k
        assert torch.equal(full[k][20:33], mid[k]), k
        assert torch.isfinite(full[k]).all(), k


# ---- 3. history beyond the staged pairs -----------------------------------------------------------------------------------------
def _with_stage_cap(cap, run):
    old = os.environ.get(STAGE_SWITCH)
    try:
        if cap is None:
            os.environ.pop(STAGE_SWITCH, None)
        else:
            os.environ[STAGE_SWITCH] = str(cap)
        return run()
    finally:
        if old is None:
            os.environ.pop(STAGE_SWITCH, None)
        else:
            os.environ[STAGE_SWITCH] = old


def _smpl_problem(B, seed=21, scale=0.8):
    m = H.native_model()
    p = synthetic.make_poses(B, seed=seed)
    go, bp, be, tr = map(H.cuda, (p.global_orient, p.body_pose, p.betas, p.transl))
    j, _ = m.lbs(go, bp, be, tr, want_vertices=False)
    return j[:, :22].contiguous(), (go * scale, bp * scale, be * 0.5, tr + 0.02)


@pytest.mark.parametrize("which", ["wide", "smpl"])
def test_staging_of_the_history_pairs_does_not_change_a_bit(which):
    """Default staging against at most 4 and 0 staged pairs: every pair of the two-loop recursion that is not staged is read
    through the global-memory branch of ``pair_y`` / ``pair_s``.  On the wide model the default run itself stages 23 of the 30
    pairs and reads the rest there; the fit is still moving when those pairs come into play (30 iterations against 24 differ).
    On the SMPL model TWO things change with the switch: the default run of 6 frames is the persistent launch of the fit kernel
    (every pair resident in LDS), a capped run goes through the step kernel, two launches per round.  The schemes are
    bit-identical (``tests/test_gpu_lbfgs.py``), so the comparison holds; a failure of the SMPL leg alone may be the scheme's,
    not the staging's."""
    B = 6
    if which == "wide":
        j3d, init = _problem(26, B, seed=8)
        run = lambda it=30: _fit(26, j3d, init, it, want_grad=True)
    else:
        j3d, init = _smpl_problem(B)
        run = lambda it=30: native.fit_world_lbfgs(H.native_model(), H.native_prior(), native.default_fit_config(), list(range(22)), j3d,
                                                   None, *init, max_iter=it, lr=1e-2, want_grad=True)
    before = os.environ.get(STAGE_SWITCH)
    default = _with_stage_cap(None, run)
    for cap in (4, 0):
        capped = _with_stage_cap(cap, run)
        for k in KEYS + ("loss", "grad"):
            assert torch.equal(default[k], capped[k]), (which, cap, k)
    assert os.environ.get(STAGE_SWITCH) == before
    for k in KEYS + ("loss", "grad"):
        assert torch.isfinite(default[k]).all(), k
    if which == "wide":
        shorter = _with_stage_cap(None, lambda: run(24))
        assert not torch.equal(_cat(default), _cat(shorter))       # iterations 25-30 (24 and more pairs) did something


# ---- 4. parameters outside the optimiser ----------------------------------------------------------------------------------------
def test_wide_device_lbfgs_respects_the_optimiser_membership():
    j3d, init = _problem(26, 12)
    cfg = _cfg(26)
    cfg.freeze_betas = 1
    fr = _fit(26, j3d, init, 10, cfg=cfg)
    assert torch.equal(fr["betas"][:, :16], init[2][:, :16]) and not torch.equal(fr["body_pose"], init[1])
    cfg.freeze_betas, cfg.optimize_mask = 0, 9            # global_orient + translation only
    s1 = _fit(26, j3d, init, 10, cfg=cfg)
    assert torch.equal(s1["betas"], init[2]) and torch.equal(s1["body_pose"], init[1]) and not torch.equal(s1["transl"], init[3])


# ---- 5. loss and gradient returned are those at the result ----------------------------------------------------------------------
def test_wide_device_lbfgs_returns_loss_and_gradient_at_the_result():
    j3d, init = _problem(26, 12)
    cfg = _cfg(26)
    out = _fit(26, j3d, init, 30, want_grad=True)
    start = _evaluate(26, cfg, j3d, init, init[1], want_grad=False)
    assert (out["loss"] < start["loss"]).all()
    again = _evaluate(26, cfg, j3d, tuple(out[k] for k in KEYS), init[1])
    assert torch.equal(again["loss"], out["loss"]) and torch.equal(again["grad"], out["grad"])
    assert tuple(out["grad"].shape) == (12, 194)


# ---- 6. warm-start sequence -----------------------------------------------------------------------------------------------------
def _motion(T, seed, joints=55):
    """(T, joints, 3) targets on the device: the NB = 26 model's kinematic joints along a small random walk of the pose."""
    rng = np.random.default_rng(seed)
    go = np.repeat(0.2 * rng.standard_normal((1, 3)), T, 0)
    pose = 0.15 * rng.standard_normal((1, 162)) + np.cumsum(0.02 * rng.standard_normal((T, 162)), axis=0)
    shape = np.repeat(0.3 * rng.standard_normal((1, 26)), T, 0)
    tr = np.repeat(rng.standard_normal((1, 3)), T, 0)
    return _joints(26, go, pose, shape, tr)[:, :joints].contiguous()


def _root0():
    return _joints(26, np.zeros((1, 3)), np.zeros((1, 162)), np.zeros((1, 26)), np.zeros((1, 3)))[:, 0]


def test_wide_sequence_mode_in_one_call_equals_the_frame_loop():
    """``k2b_fit_sequence_lbfgs`` through its frame-by-frame branch (``frame_prep`` + one device-driven fit per frame) against the
    same loop driven from here, one ``fit_world_lbfgs`` call per frame - the call ``WorldSpaceFitter.fit_frame`` makes (the start
    = the predecessor's result, which is also the preserve pose; frame 0 with 6 iterations and no preserve term, the others
    with 3 and the preserve term) - bit for bit, per-frame confidences included.  (``fit_frame`` itself ends in the final
    forward, which ``k2b_lbs`` does not run for this model: see ``_oracle``.)"""
    T = 5
    j = _motion(T, seed=2)
    conf = H.cuda(np.random.default_rng(3).uniform(0.5, 1.5, (T, 55)).astype(np.float32))
    z = lambda c: torch.zeros(1, c, device="cuda")
    start = (z(3), z(162), z(26), (j[:1, 0] - _root0()).contiguous())
    cfg = _cfg(26)
    cfg.pose_preserve_weight, cfg.conf_per_frame = 5.0, 1
    out = native.fit_sequence_lbfgs(_model(26), H.native_prior(), cfg, 6, 3, list(range(55)), j, conf, *start, lr=1e-2)
    prev = start
    for t in range(T):
        c = _cfg(26)
        c.pose_preserve_weight = 5.0 if t else 0.0
        one = native.fit_world_lbfgs(_model(26), H.native_prior(), c, list(range(55)), j[t:t + 1].contiguous(), conf[t].contiguous(), *prev,
                                     max_iter=3 if t else 6, lr=1e-2, preserve_pose=prev[1].clone())
        for k in KEYS + ("loss",):
            assert torch.equal(out[k][t:t + 1], one[k]), (t, k)
        prev = tuple(one[k] for k in KEYS)
    assert not torch.equal(out["body_pose"][0], out["body_pose"][T - 1]) and torch.isfinite(out["loss"]).all()


# ---- 7. the fitter class, both drivers ------------------------------------------------------------------------------------------
def _public():
    if "public" in _cache:
        return _cache["public"]
    from keypoints2body_amd.models.body_model import BodyModel
    from keypoints2body_amd.prior import MaxMixturePrior, MixtureBuffers
    g = H.gmm_fixture()
    c = _consts(26)
    model = BodyModel(c.v_template, c.shapedirs, c.posedirs, c.J_regressor, c.lbs_weights, c.parents, c.extra_vertex_ids, num_betas=16)
    assert model.model_type == "smplx" and model.num_betas == 16 and model.num_expression_coeffs == 10
    prior = MaxMixturePrior(MixtureBuffers(g["ref_means"], g["ref_precisions"], g["ref_nll_weights"].reshape(-1)))
    _cache["public"] = (model, prior, (torch.zeros(1, 66), torch.zeros(1, 16)))
    return _cache["public"]


def test_wide_model_through_the_fitter_with_the_host_driver_as_twin():
    """``WorldSpaceFitter`` on ``BodyModel(..., num_betas=16)`` in its default branch (L-BFGS): ``fit_batch`` without the final
    forward returns 16 betas | 10 expression coefficients, finite, at a lower loss than the start; ``lbfgs_driver = "host"`` over
    3 iterations agrees with the device driver within case 1's gate.  (The entries that end in the final forward -
    ``fit_frame``, ``optimize_params_frame`` / ``_sequence`` / ``_sequences`` - need ``k2b_lbs`` to skin this model: see ``_oracle``.)"""
    from keypoints2body_amd.core.fitters.world_space import WorldSpaceFitter
    from keypoints2body_amd.models.smpl_data import SMPLXData
    model, prior, _ = _public()
    j = _motion(1, seed=6).cpu()
    z = lambda c: torch.zeros(1, c)
    start = SMPLXData(betas=z(16), global_orient=z(3), body_pose=z(63), transl=(j[:, 0] - _root0().cpu()), left_hand_pose=z(45),
                      right_hand_pose=z(45), expression=z(10), jaw_pose=z(3), leye_pose=z(3), reye_pose=z(3))
    idx = torch.arange(55)
    run = lambda f: f.fit_batch(start, j, None, seq_ind=0, target_model_indices=idx, run_forward=False)[0]
    kw = dict(step_size=1e-2, joints_category="GENERIC", pose_prior=prior)
    at_start = run(WorldSpaceFitter(model, use_lbfgs=False, num_iters_first=1, **dict(kw, step_size=0.0)))     # a zero step: evaluate-only
    full = WorldSpaceFitter(model, use_lbfgs=True, num_iters_first=30, **kw)
    out = run(full)
    params = full.result_params(out, start)
    assert isinstance(params, SMPLXData) and tuple(params.betas.shape) == (1, 16) and tuple(params.expression.shape) == (1, 10)
    assert all(torch.isfinite(out[k]).all() for k in KEYS + ("loss",)) and float(out["loss"]) < float(at_start["loss"])
    dev_f, host_f = (WorldSpaceFitter(model, use_lbfgs=True, num_iters_first=3, **kw) for _ in range(2))
    host_f.lbfgs_driver = "host"
    a, b = _cat(run(dev_f)).cpu(), _cat(run(host_f)).cpu()
    moved = float((b - torch.cat([start.global_orient, torch.zeros(1, 162), torch.zeros(1, 26), start.transl], dim=1)).abs().max())
    diff = float((a - b).abs().max())
    print(f"fitter, 3 iterations: host driver moved the start by {moved:.3e}, device - host {diff:.3e}")
    assert moved > 1e-4 and diff < 2e-5 * max(1.0, 3 / 2), diff


# ---- 8. batched shape pre-pass --------------------------------------------------------------------------------------------------
def test_wide_batched_shape_pass_matches_the_single_pass():
    """``k2b_shape_pass_lbfgs`` (one optimiser instance of P = 194 per sequence; only the 16 betas move) against
    ``optimize_shape_pass`` (``torch.optim.LBFGS`` on the same closure) within DESIGN 4.7b's tolerance for the SMPL case, and a
    sequence alone against the same sequence inside the pair, bit for bit."""
    from keypoints2body_amd.core.config import SequenceOptimizeConfig
    from keypoints2body_amd.core.engine import optimize_shape_pass, optimize_shape_pass_batched
    model, prior, mean = _public()
    cfg = SequenceOptimizeConfig()
    cfg.frame.joints_category = "AMASS"
    xs = [_motion(8, seed=12, joints=22), _motion(8, seed=13, joints=22)]
    cs = [torch.ones(22), torch.tensor(np.random.default_rng(14).uniform(0.5, 1.5, 22).astype(np.float32))]
    pair = optimize_shape_pass_batched(model, cfg, mean[1], mean[0], xs, cs, "cuda", pose_prior=prior)
    assert tuple(pair.shape) == (2, 16) and torch.isfinite(pair).all() and float(pair.abs().max()) > 1e-3
    for s in range(2):
        one = optimize_shape_pass(model, cfg, mean[1], mean[0], xs[s], cs[s], model.device, pose_prior=prior)
        diff = float((pair[s:s + 1] - one.reshape(1, -1)).abs().max())
        print(f"sequence {s}: batched pass - single pass {diff:.3e}")
        assert diff < 1e-5, (s, diff)
        alone = optimize_shape_pass_batched(model, cfg, mean[1], mean[0], [xs[s]], [cs[s]], "cuda", pose_prior=prior)
        assert torch.equal(alone, pair[s:s + 1]), s
