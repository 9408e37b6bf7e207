"""GPU: the device-resident L-BFGS (``k2b_fit_world_lbfgs``, csrc/k2b_lbfgs.hip) - the reference's DEFAULT optimiser
(``core/config.py:29`` ``use_lbfgs=True``; ``core/fitters/world_space.py:231-247``) with the state machine itself on the device.

Gates, in the order of how sharply they pin the port:
* against its CPU twin ``core/lbfgs_batched.py`` (pinned to ``torch.optim.LBFGS`` iterate by iterate in float64 by
  ``tests/test_lbfgs_batched.py``) on the REAL closure, for the first iterations - while summation-order rounding (double
  accumulation on the device, float32 einsum in the twin) has not been amplified by the line search's branches yet;
* frames are independent and the result does not depend on the batch a frame sits in (bit for bit);
* end states at the reference's iteration counts statistically (``tests/test_gpu_api.py``: the world / camera L-BFGS goldens
  recorded with the real reference now run through this path);
* timing of the default-config single frame and of 256 frames, printed.
"""
import time

import numpy as np
import pytest
import torch

from keypoints2body_amd import native, synthetic
from tests import helpers as H

pytestmark = pytest.mark.gpu


def _problem(B, seed=21, scale=0.8):
    m = H.native_model()
    p = synthetic.make_poses(B, seed=seed)
    go, bp, be, tr = map(H.cuda, (p.global_orient, p.body_pose, p.betas, p.transl))
    j, _ = m.lbs(go, bp, be, tr, want_vertices=False)
    j3d = j[:, :22].contiguous()
    return j3d, (go * scale, bp * scale, be * 0.5, tr + 0.02)


def _host_twin(cfg, j3d, init, max_iter, lr=1e-2, history_size=100, opt_out=None, **kw):
    """``BatchedLBFGS`` (numpy, float32 vectors) driving the same evaluate-only launches (`opt_out`: a list that receives the
    finished optimiser, e.g. for its branch record with ``record=True``)."""
    from keypoints2body_amd.core.lbfgs_batched import BatchedLBFGS
    m, pr = H.native_model(), H.native_prior()
    c = native.default_fit_config()
    for f, _ in native.FitConfigC._fields_:
        setattr(c, f, getattr(cfg, f))
    c.num_iters, c.step_size = 1, 0.0
    go, bp, be, tr = init
    preserve = bp.clone()
    D, NB = bp.shape[1], be.shape[1]

    def evaluate(x):
        xt = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
        r = native.fit_world(m, pr, c, list(range(22)), j3d, None, xt[:, 0:3].contiguous(), xt[:, 3:3 + D].contiguous(),
                             xt[:, 3 + D:3 + D + NB].contiguous(), xt[:, 3 + D + NB:].contiguous(), preserve_pose=preserve, want_grad=True)
        return r["loss"].cpu().numpy().astype(np.float64), r["grad"].cpu().numpy()

    opt = BatchedLBFGS(evaluate, torch.cat(init, dim=1).cpu().numpy(), lr=lr, max_iter=max_iter, history_size=history_size, **kw)
    if opt_out is not None:
        opt_out.append(opt)
    return opt.run(), opt.rounds


@pytest.mark.parametrize("max_iter", [1, 2, 3, 5])
def test_device_lbfgs_follows_the_cpu_twin_over_the_first_iterations(max_iter):
    B = 12
    j3d, init = _problem(B)
    cfg = native.default_fit_config()
    out = native.fit_world_lbfgs(H.native_model(), H.native_prior(), cfg, list(range(22)), j3d, None, *init, max_iter=max_iter, lr=1e-2)
    x_dev = torch.cat([out[k] for k in ("global_orient", "body_pose", "betas", "transl")], dim=1).cpu().numpy()
    x_host, rounds = _host_twin(cfg, j3d, init, max_iter)
    assert rounds <= max_iter * 5 // 4 + 2
    moved = np.abs(x_host - torch.cat(init, dim=1).cpu().numpy()).max()
    dev = np.abs(x_dev - x_host).max()
    print(f"max_iter {max_iter}: twin moved the start by {moved:.3e}, device - twin {dev:.3e}")
    assert moved > 1e-4                                   # the optimiser did something
    assert dev < 2e-5 * max(1.0, max_iter / 2), (max_iter, dev)


def test_device_lbfgs_frames_are_independent_of_their_batch():
    j3d, init = _problem(40, seed=5)
    cfg = native.default_fit_config()
    run = lambda sl: native.fit_world_lbfgs(H.native_model(), H.native_prior(), cfg, list(range(22)), j3d[sl].contiguous(), None,
                                            *[t[sl].contiguous() for t in init], max_iter=30, lr=1e-2)
    full, again = run(slice(0, 40)), run(slice(0, 40))
    one, mid = run(slice(7, 8)), run(slice(20, 33))
    for k in ("global_orient", "body_pose", "betas", "transl", "loss"):
        assert torch.equal(full[k], again[k]), k
        assert torch.equal(full[k][7:8], one[k]), k       # a single frame takes the very same path (world-size independence)
        assert torch.equal(full[k][20:33], mid[k]), k
        assert torch.isfinite(full[k]).all()


def test_device_lbfgs_launch_schemes_agree_bitwise():
    """Three ways the rounds reach the device, chosen by the batch size: the whole fit in one persistent launch (at most two frames per
    CU), the step as a prologue of the closure's launch (at most four), and two launches per round (beyond).  The same frames must
    come out bit-identical whichever scheme their batch takes (the optimiser's code is inlined into three kernels: it is compiled
    without FMA contraction, and the tree pass keeps a single call site per kernel - either one left to the compiler cost a ulp in a
    few gradients of hundreds, and thirty L-BFGS iterations later the frames had parted ways)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    j3d, init = _problem(5 * cus, seed=13)
    cfg = native.default_fit_config()
    run = lambda n: native.fit_world_lbfgs(H.native_model(), H.native_prior(), cfg, list(range(22)), j3d[:n].contiguous(), None,
                                           *[t[:n].contiguous() for t in init], max_iter=30, lr=1e-2)
    small, mid, big = run(2 * cus), run(3 * cus), run(5 * cus)        # persistent | fused rounds | two launches per round
    for k in ("global_orient", "body_pose", "betas", "transl", "loss"):
        assert torch.equal(small[k], mid[k][:2 * cus]), k
        assert torch.equal(small[k], big[k][:2 * cus]), k
        assert torch.equal(mid[k], big[k][:3 * cus]), k
    # more history pairs than the staging LDS of any scheme holds (60 iterations, 85 parameters; lbfgs_staged_pairs of
    # csrc/k2b_launch_plan.h: 15 / 36 / 47 pairs fit at two frames per workgroup of the persistent launch, three of the fused
    # rounds and in the step kernel): the pairs beyond it are read from global memory, in the resident optimiser too
    long = lambda n: native.fit_world_lbfgs(H.native_model(), H.native_prior(), cfg, list(range(22)), j3d[:n].contiguous(), None,
                                            *[t[:n].contiguous() for t in init], max_iter=60, lr=1e-2, tolerance_grad=0.0,
                                            tolerance_change=0.0)
    a, b, c = long(2 * cus), long(3 * cus), long(5 * cus)
    for k in ("global_orient", "body_pose", "betas", "transl", "loss"):
        assert torch.equal(a[k], b[k][:2 * cus]), k
        assert torch.equal(a[k], c[k][:2 * cus]), k


# ---- the three inlined copies of the optimiser where the line search WORKS ------------------------------------------------------
# At lr = 1e-2 from a 20 % perturbation (everything above) the first trial step satisfies Wolfe nearly always: the zoom phase, the
# insufficient-progress rule and the ring's drop are compared with nothing in the fused copies.  Here: lr = 1, a history of 2 / 3,
# and an input on which the twin's branch record shows them taken (the condition in the scheme test).  What that needed, measured
# with the host-driven twin on the first 24 frames: at the default GMoF sigma of 100 the loss is so smooth that every zoom ends on
# its first evaluation whatever the start - `_problem`'s scale 0.8, 0.5, 0.2, 0, -0.5, -1, 1.5, 2: 13 to 46 zoom entries, 190 to
# 216 ring drops, NO insufficient-progress or flip event.  With a small sigma (0.05, the robust loss bites at 5 cm) and the start
# at the zero pose (scale 0) there are 81 / 78 zoom entries, 6 / 4 insufficient-progress and 4 / 3 flip events, 163 / 139 ring drops
# (history 2 / 3).  The copies must still agree bit for bit.
HARD = dict(max_iter=12, lr=1.0, tolerance_grad=0.0, tolerance_change=0.0)
HARD_SCALE, HARD_SIGMA = 0.0, 0.05


def _hard_cfg():
    cfg = native.default_fit_config()
    cfg.sigma = HARD_SIGMA
    return cfg


def _with_stage_pairs(cap, run):
    import os
    old = os.environ.get("K2B_LBFGS_STAGE_PAIRS")
    os.environ["K2B_LBFGS_STAGE_PAIRS"] = str(cap)
    try:
        return run()
    finally:
        if old is None:
            os.environ.pop("K2B_LBFGS_STAGE_PAIRS", None)
        else:
            os.environ["K2B_LBFGS_STAGE_PAIRS"] = old


@pytest.mark.parametrize("history", [2, 3])
def test_device_lbfgs_launch_schemes_agree_bitwise_where_the_line_search_works(history):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    j3d, init = _problem(5 * cus, seed=13, scale=HARD_SCALE)
    cfg = _hard_cfg()
    run = lambda n: native.fit_world_lbfgs(H.native_model(), H.native_prior(), cfg, list(range(22)), j3d[:n].contiguous(), None,
                                           *[t[:n].contiguous() for t in init], history_size=history, **HARD)
    small, mid, big = run(2 * cus), run(3 * cus), run(5 * cus)        # persistent | fused rounds | two launches per round
    for k in ("global_orient", "body_pose", "betas", "transl", "loss"):
        assert torch.equal(small[k], mid[k][:2 * cus]), k
        assert torch.equal(small[k], big[k][:2 * cus]), k
        assert torch.equal(mid[k], big[k][:3 * cus]), k
    unstaged = _with_stage_pairs(0, lambda: run(5 * cus))              # two launches per round, every pair from global memory
    for k in ("global_orient", "body_pose", "betas", "transl", "loss"):
        assert torch.equal(big[k], unstaged[k]), k

    # input condition, from the twin's record on the same closure launches (not from the code under test): the first 24 frames
    # enter the zoom phase, take an insufficient-progress or flip branch and drop a pair from the full ring
    n = 24
    sub = j3d[:n].contiguous(), tuple(t[:n].contiguous() for t in init)
    got = []
    _host_twin(cfg, *sub, HARD["max_iter"], lr=HARD["lr"], history_size=history, opt_out=got, record=True, tolerance_grad=0.0,
               tolerance_change=0.0)
    count = lambda *names: sum(ev.count(e) for ev in got[0].events for e in names)
    seen = {"zoom": count("zoom_enter_low0", "zoom_enter_low1"), "insuf / flip": count("zn_insuf_set", "zn_moved_insuf", "zr_flip"),
            "ring drop": count("ring_drop")}
    print(f"history {history}, start scale {HARD_SCALE}, sigma {HARD_SIGMA}: events over {n} frames {seen}")
    assert all(seen.values()), seen


@pytest.mark.parametrize("history", [2, 3])
@pytest.mark.parametrize("max_iter", [1, 2])
def test_device_lbfgs_follows_the_cpu_twin_where_the_line_search_works(max_iter, history):
    n = 24                                                             # the first 24 frames of the scheme test's batch
    j3d, init = _problem(5 * torch.cuda.get_device_properties(0).multi_processor_count, seed=13, scale=HARD_SCALE)
    j3d, init = j3d[:n].contiguous(), tuple(t[:n].contiguous() for t in init)
    cfg = _hard_cfg()
    kw = dict(HARD, max_iter=max_iter)
    out = native.fit_world_lbfgs(H.native_model(), H.native_prior(), cfg, list(range(22)), j3d, None, *init, history_size=history, **kw)
    x_dev = torch.cat([out[k] for k in ("global_orient", "body_pose", "betas", "transl")], dim=1).cpu().numpy()
    x_host, _ = _host_twin(cfg, j3d, init, max_iter, lr=kw["lr"], history_size=history, tolerance_grad=0.0, tolerance_change=0.0)
    dev = np.abs(x_dev - x_host).max(axis=1)
    print(f"lr 1, max_iter {max_iter}, history {history}: device - twin per frame, max {dev.max():.3e}")
    assert dev.max() < 2e-5 * max(1.0, max_iter / 2), (max_iter, dev)


def test_device_lbfgs_sixteen_beta_model_takes_the_same_schemes():
    """The 16-beta instantiations of the fused kernel (91 parameters per frame) through the persistent launch and through two
    launches per round: bit-identical, and the betas move."""
    from keypoints2body_amd import synthetic
    from keypoints2body_amd.native import NativeModel
    c = synthetic.make_body_model(seed=3, num_vertices=512, num_betas=16)
    model = NativeModel(c.v_template, c.shapedirs, c.posedirs, c.J_regressor, c.lbs_weights, c.parents, c.extra_vertex_ids)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = 5 * cus
    p = synthetic.make_poses(B, seed=21)
    t = lambda x: torch.as_tensor(np.asarray(x), dtype=torch.float32).cuda()
    go, bp, tr = t(p.global_orient), t(p.body_pose), t(p.transl)
    be = torch.linspace(-1.0, 1.0, 16).repeat(B, 1).cuda() * 0.5
    j, _ = model.lbs(go, bp, be, tr, want_vertices=False)
    j3d = j[:, :22].contiguous()
    init = (go * 0.8, bp * 0.8, torch.zeros_like(be), tr + 0.02)
    cfg = native.default_fit_config()
    run = lambda n: native.fit_world_lbfgs(model, H.native_prior(), cfg, list(range(22)), j3d[:n].contiguous(), None,
                                           *[x[:n].contiguous() for x in init], max_iter=10, lr=1e-2)
    small, big = run(8), run(B)
    for k in ("global_orient", "body_pose", "betas", "transl", "loss"):
        assert torch.equal(small[k], big[k][:8]), k
        assert torch.isfinite(big[k]).all()
    assert small["betas"].abs().max() > 1e-3


def test_device_lbfgs_minimises_and_respects_the_optimiser_membership():
    B = 64
    j3d, init = _problem(B, seed=9)
    m, pr = H.native_model(), H.native_prior()
    cfg = native.default_fit_config()
    cfg.num_iters, cfg.step_size = 1, 0.0
    start = native.fit_world(m, pr, cfg, list(range(22)), j3d, None, *init, preserve_pose=init[1])
    out = native.fit_world_lbfgs(m, pr, cfg, list(range(22)), j3d, None, *init, max_iter=30, lr=1e-2, want_grad=True)
    assert (out["loss"] < 0.5 * start["loss"]).all()      # thirty L-BFGS iterations from a 20 % perturbation (measured: 0.1-0.3)
    # loss / gradient returned ARE those at the result
    again = native.fit_world(m, pr, cfg, list(range(22)), j3d, None, out["global_orient"], out["body_pose"], out["betas"], out["transl"],
                             preserve_pose=init[1], want_grad=True)
    assert torch.equal(again["loss"], out["loss"]) and torch.equal(again["grad"], out["grad"])
    # frozen betas / a reduced optimiser: those parameters never move
    cfg.freeze_betas = 1
    fr = native.fit_world_lbfgs(m, pr, cfg, list(range(22)), j3d, None, *init, max_iter=10, lr=1e-2)
    assert torch.equal(fr["betas"], init[2]) and not torch.equal(fr["body_pose"], init[1])
    cfg.freeze_betas, cfg.optimize_mask = 0, 9            # camera stage 1: global_orient + translation only
    s1 = native.fit_world_lbfgs(m, pr, cfg, list(range(22)), j3d, None, *init, max_iter=10, lr=1e-2)
    assert torch.equal(s1["betas"], init[2]) and torch.equal(s1["body_pose"], init[1]) and not torch.equal(s1["transl"], init[3])


def test_device_lbfgs_timing_of_the_reference_default_path():
    """default-config single frame <= 1 ms (host-driven torch.optim.LBFGS: 6.9 ms), 256 independent frames
    <= 3 ms (lock-step host driver: 16 ms).  Wall time of the call + synchronise, median of several."""
    m, pr = H.native_model(), H.native_prior()
    cfg = native.default_fit_config()
    res = {}
    for B in (1, 256, 1024):
        j3d, init = _problem(B, seed=3)
        run = lambda: native.fit_world_lbfgs(m, pr, cfg, list(range(22)), j3d, None, *init, max_iter=30, lr=1e-2)
        for _ in range(3):
            run()
        torch.cuda.synchronize()
        ts = []
        for _ in range(7):
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        res[B] = 1e3 * float(np.median(ts))
    print("device L-BFGS (max_iter 30, 22 AMASS joints), ms per call:", {k: round(v, 3) for k, v in res.items()})
    assert res[1] < 2.0 and res[256] < 4.0


def test_smplx_device_lbfgs_runs_the_tree_kernel_as_its_closure():
    B = 6
    m, pr = H.native_model_x(), H.native_prior()
    rng = np.random.default_rng(4)
    go, pose, shape, tr = (0.2 * rng.standard_normal((B, 3)), 0.15 * rng.standard_normal((B, 162)), 0.3 * rng.standard_normal((B, 20)),
                           rng.standard_normal((B, 3)))
    j, _ = m.lbs(H.cuda(go), H.cuda(pose), H.cuda(shape), H.cuda(tr), want_vertices=False)
    j3d = j[:, :55].contiguous()
    cfg = native.default_fit_config(); cfg.prior_pose_dims, cfg.num_betas_prior = 63, 10
    z = lambda c: torch.zeros(B, c, device="cuda")
    tr0 = (j3d[:, 0] - m.lbs(z(3), z(162), z(20), None, want_vertices=False)[0][:, 0]).contiguous()
    cfg.num_iters, cfg.step_size = 1, 0.0
    start = native.fit_world(m, pr, cfg, list(range(55)), j3d, None, z(3), z(162), z(20), tr0)
    out = native.fit_world_lbfgs(m, pr, cfg, list(range(55)), j3d, None, z(3), z(162), z(20), tr0, max_iter=20, lr=1e-2)
    assert torch.isfinite(out["body_pose"]).all() and (out["loss"] < 0.6 * start["loss"]).all()


def test_device_lbfgs_history_ring_drops_the_oldest_pair_like_torch():
    """history_size smaller than the iteration count: torch pops the oldest (s, y) pair; the device keeps a ring.  Against the
    CPU twin with the same limit, frame by frame (and against an unlimited history, which must differ - the limit is really
    exercised).  A line search branches on rounding, so a frame either stays with its twin to ~1e-7 or leaves it by ~1e-3 at some
    iteration (tools/dev_lbfgs_diag.py: with an UNLIMITED history two of six frames have left by iteration 8, with this limit none
    by iteration 10): the gate is on the median frame."""
    B, it = 6, 10
    j3d, init = _problem(B, seed=13)
    cfg = native.default_fit_config()
    run = lambda h: native.fit_world_lbfgs(H.native_model(), H.native_prior(), cfg, list(range(22)), j3d, None, *init, max_iter=it, lr=1e-2,
                                           history_size=h)
    cat = lambda o: torch.cat([o[k] for k in ("global_orient", "body_pose", "betas", "transl")], dim=1).cpu().numpy()
    small, full = cat(run(2)), cat(run(100))
    twin, _ = _host_twin(cfg, j3d, init, it, history_size=2)
    per_frame = np.abs(small - twin).max(axis=1)
    print(f"history 2 against unlimited: {np.abs(small - full).max():.2e}; device - twin per frame {per_frame}")
    assert np.abs(small - full).max() > 1e-6
    assert np.median(per_frame) < 1e-5, per_frame


def test_device_lbfgs_empty_batch_and_argument_checks():
    m, pr = H.native_model(), H.native_prior()
    cfg = native.default_fit_config()
    e = lambda c: torch.zeros(0, c, device="cuda")
    out = native.fit_world_lbfgs(m, pr, cfg, list(range(22)), torch.zeros(0, 22, 3, device="cuda"), None, e(3), e(69), e(10), e(3), max_iter=5, lr=1e-2)
    assert out["body_pose"].shape == (0, 69)
    j3d, init = _problem(2)
    with pytest.raises(ValueError):
        native.fit_world_lbfgs(m, pr, cfg, list(range(22)), j3d, None, *init, max_iter=0, lr=1e-2)
    with pytest.raises(ValueError):
        native.fit_world_lbfgs(m, pr, cfg, list(range(22)), j3d, None, *init, max_iter=5, lr=0.0)
    with pytest.raises(NotImplementedError):
        native.fit_world_lbfgs(m, pr, cfg, list(range(22)), j3d, None, *init, max_iter=5, lr=1e-2, history_size=101)


def test_default_sequence_mode_in_one_call_equals_the_frame_loop():
    """``k2b_fit_sequence_lbfgs`` (the reference's DEFAULT sequence mode: warm start + L-BFGS, api/sequence.py:214-281 over
    world_space.py:231-247) against the same loop driven frame by frame through ``fit_frame`` - ``prev = res.params``, frame 0
    with ``num_iters_first`` and no preserve term, the others with ``num_iters_followup`` and the preserve term - bit for bit;
    per-frame confidences (``fix_foot``) included; and through the public ``optimize_params_sequence``."""
    import keypoints2body_amd as k2b
    from keypoints2body_amd.core.config import FrameOptimizeConfig, SequenceOptimizeConfig
    from keypoints2body_amd.core.fitters.world_space import WorldSpaceFitter
    from keypoints2body_amd.models.body_model import BodyModel
    from keypoints2body_amd.prior import MaxMixturePrior, MixtureBuffers
    g = H.gmm_fixture()
    prior = MaxMixturePrior(MixtureBuffers(g["ref_means"], g["ref_precisions"], g["ref_nll_weights"].reshape(-1)))
    model = BodyModel.synthetic(0)
    T = 9
    p = synthetic.make_poses(1, seed=17)
    rng = np.random.default_rng(2)
    walk = np.cumsum(0.03 * rng.standard_normal((T, 69)), axis=0).astype(np.float32)
    with torch.no_grad():
        j = H.oracle_model()(global_orient=torch.tensor(np.repeat(p.global_orient, T, 0)), body_pose=torch.tensor(p.body_pose + walk),
                             betas=torch.tensor(np.repeat(p.betas, T, 0)), transl=torch.tensor(np.repeat(p.transl, T, 0))).joints[:, :22]
    conf = torch.ones(T, 22)
    conf[:, [7, 8, 10, 11]] = 1.5
    fitter = WorldSpaceFitter(model, step_size=1e-2, num_iters_first=12, num_iters_followup=5, use_lbfgs=True, joints_category="AMASS",
                              pose_prior=prior)
    z = lambda c: torch.zeros(1, c)
    start = k2b.SMPLData(betas=z(10), global_orient=z(3), body_pose=z(69), transl=j[:1, 0].clone())
    assert fitter.chain_supported(None)
    out, joints, verts, loss = fitter.fit_chain(start, j, conf)
    prev = start
    for t in range(T):
        res = fitter.fit_frame(prev, j[t:t + 1], conf_3d=conf[t], seq_ind=t)
        for k in ("global_orient", "body_pose", "betas", "transl"):
            assert torch.equal(out[k][t:t + 1], getattr(res.params, k)), (t, k)
        assert torch.equal(joints[t:t + 1], res.joints) and float(loss[t]) == float(res.loss)
        prev = res.params
    # the public API takes this path for the reference's default configuration
    cfg = SequenceOptimizeConfig(frame=FrameOptimizeConfig(num_iters_first=12, num_iters_followup=5, joints_category="AMASS"),
                                 use_shape_optimization=False, fix_foot=True)
    assert cfg.frame.use_lbfgs and cfg.use_previous_frame_init
    seq = np.concatenate([j.numpy(), np.ones((T, 22, 1), np.float32)], axis=2)
    api = k2b.optimize_params_sequence(seq, init_params=start, joint_layout="AMASS", model=model, config=cfg, pose_prior=prior,
                                       mean_params=(torch.zeros(1, 72), torch.zeros(1, 10)))
    assert len(api) == T
    ref, _, _, _ = fitter.fit_chain(start, j, conf, joint_loss_weight=cfg.frame.joint_loss_weight,
                                    pose_preserve_weight=cfg.frame.pose_preserve_weight, freeze_betas=cfg.frame.freeze_betas)
    for t in (0, 1, T - 1):
        assert torch.equal(api[t].params.body_pose, ref["body_pose"][t:t + 1]) and torch.equal(api[t].params.betas, ref["betas"][t:t + 1])


def _refused_calls():
    """(id, entry, what is wrong with the call, exception class of the status, substring of the library's message).  One frame, three
    targets; ``cfg`` marks a non-zero translation prior weight, ``surface`` a target that is an extra joint."""
    bad, unsup = ValueError, NotImplementedError
    rows = []
    for entry, who, it in (("world", "k2b_fit_world_lbfgs", "max_iter"), ("sequence", "k2b_fit_sequence_lbfgs", "first_iters"),
                           ("sequences", "k2b_fit_sequences_lbfgs", "first_iters"), ("shape", "k2b_shape_pass_lbfgs", "max_iter")):
        rows += [(entry, {it: 0}, bad, f"{who}: max_iter=0"), (entry, {it: 10001}, bad, f"{who}: max_iter=10001"),
                 (entry, {"history_size": 101}, unsup, f"{who}: history_size=101 (at most 100)"),
                 (entry, {"lr": 0.0}, bad, f"{who}: lr must be positive"), (entry, {"lr": -1e-2}, bad, f"{who}: lr must be positive")]
    for entry, who in (("sequence", "k2b_fit_sequence_lbfgs"), ("sequences", "k2b_fit_sequences_lbfgs")):
        rows += [(entry, {"followup_iters": 0}, bad, f"{who}: followup_iters=0"),
                 (entry, {"followup_iters": 10001}, bad, f"{who}: followup_iters=10001"),
                 (entry, {"null": True}, bad, f"{who}: NULL parameter / target buffer")]
    rows += [("sequence", {"cfg": True}, unsup, "k2b_fit_sequence_lbfgs: no translation prior in a chain"),
             ("sequences", {"cfg": True}, bad, "k2b_fit_sequences_lbfgs: transl_prior_weight must be 0 in a chain"),
             ("world", {"null": True}, bad, "k2b_fit_world_lbfgs: NULL parameter buffer"),
             ("shape", {"null": True}, bad, "k2b_shape_pass_lbfgs: NULL buffer"),
             ("sequences", {"surface": True}, unsup,
              "k2b_fit_sequences_lbfgs: one launch needs the 24-joint model, the prior over the whole pose and kinematic targets")]
    return rows


def test_device_lbfgs_entries_refuse_bad_calls_with_their_status_and_message():
    """The argument checks of the four L-BFGS entries, call by call: the status class the binding raises and the text the library
    recorded (``k2b_last_error``).  Nothing is launched by a refused call."""
    m, pr = H.native_model(), H.native_prior()
    assert m.num_output_joints > m.num_joints              # the model has extra joints: a surface target exists
    j3d, (go, bp, be, tr) = _problem(1)
    j3d = j3d[:, :3].contiguous()
    off = torch.tensor([0, 1], dtype=torch.int32, device="cuda")

    def call(entry, max_iter=5, first_iters=5, followup_iters=3, history_size=100, lr=1e-2, null=False, cfg=False, surface=False):
        c = native.default_fit_config()
        c.transl_prior_weight = 1.0 if cfg else 0.0
        idx = [0, 1, m.num_joints] if surface else [0, 1, 2]
        g = None if null else go
        if entry == "world":
            return native.fit_world_lbfgs(m, pr, c, idx, j3d, None, g, bp, be, tr, max_iter=max_iter, lr=lr, history_size=history_size)
        if entry == "sequence":
            return native.fit_sequence_lbfgs(m, pr, c, first_iters, followup_iters, idx, j3d, None, g, bp, be, tr, lr=lr,
                                             history_size=history_size)
        if entry == "sequences":
            return native.fit_sequences_lbfgs(m, pr, c, first_iters, followup_iters, idx, [1], j3d, None, g, bp, be, tr, lr=lr,
                                              history_size=history_size)
        return native.shape_pass_lbfgs(m, pr, c, off, idx, j3d, None, g, bp, j3d[:, 0].contiguous(), 0, be, max_iter=max_iter, lr=lr,
                                       history_size=history_size)

    for entry, wrong, exc, text in _refused_calls():
        with pytest.raises(exc) as info:
            call(entry, **wrong)
        assert text in str(info.value), (entry, wrong, str(info.value))
    for entry in ("world", "sequence", "sequences", "shape"):                  # the same calls with nothing wrong go through
        call(entry)
    torch.cuda.synchronize()
