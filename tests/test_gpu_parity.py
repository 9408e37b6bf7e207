"""GPU parity tests proper: the HIP path (through the C ABI) against the oracle and
against the golden vectors the reference's own fitter produced.

Tolerances: the north star asks for pose/shape within 1e-4 abs of the reference CPU
path; the reference's own fp32-vs-fp64 spread on these inputs is ~3e-6
("noise floor"), so the gate below is 1e-4 and typical errors are ~1e-6.
"""
import numpy as np
import pytest
import torch

from tests import helpers as H

pytestmark = pytest.mark.gpu
PARAM_TOL = 1e-4


def test_library_loaded_and_device_present():
    from keypoints2body_amd import native
    lib = native.load_library()
    assert lib.k2b_version() >> 16 == 1
    assert torch.cuda.is_available()
    assert H.body_consts().fingerprint() == int(H.load_case("amass_zero_init")["model_fingerprint"])


def test_joint_basis_mfma_matches_regressor_contraction():
    c = H.body_consts()
    jt, jd = H.native_model().joint_basis()
    ref_t = c.J_regressor.astype(np.float64) @ c.v_template.astype(np.float64)
    ref_d = np.einsum("jv,vak->jak", c.J_regressor.astype(np.float64), c.shapedirs.astype(np.float64))
    assert np.abs(jt - ref_t).max() < 2e-6
    assert np.abs(jd - ref_d).max() < 2e-6


@pytest.mark.parametrize("with_transl", [True, False])
def test_lbs_matches_oracle_forward(with_transl):
    from keypoints2body_amd import synthetic
    B = 19   # not a multiple of the kernel's frame group
    p = synthetic.make_poses(B, seed=3)
    t = lambda a: torch.tensor(a)
    out = H.oracle_model()(global_orient=t(p.global_orient), body_pose=t(p.body_pose), betas=t(p.betas),
                           transl=t(p.transl) if with_transl else None)
    j, v = H.native_model().lbs(H.cuda(p.global_orient), H.cuda(p.body_pose), H.cuda(p.betas),
                                H.cuda(p.transl) if with_transl else None)
    torch.cuda.synchronize()
    assert np.abs(j.cpu().numpy() - out.joints.numpy()).max() < 5e-6
    assert np.abs(v.cpu().numpy() - out.vertices.numpy()).max() < 5e-6
    # joints-only path must agree with the full path bit for bit
    j2, v2 = H.native_model().lbs(H.cuda(p.global_orient), H.cuda(p.body_pose), H.cuda(p.betas),
                                  H.cuda(p.transl) if with_transl else None, want_vertices=False)
    assert v2 is None and torch.equal(j, j2)


@pytest.mark.parametrize("V,NB,B", [(64, 10, 1), (97, 10, 33), (500, 16, 129), (1000, 10, 257), (2049, 16, 31), (6890, 10, 130)])
def test_lbs_ragged_sizes_match_oracle(V, NB, B):
    """Mesh sizes and batches that are not multiples of the kernel's tiles (32-vertex / 32-frame MFMA tiles, 64 x 128
    workgroup tiles) and both beta counts, with large rotations; against the oracle's forward on the same arrays."""
    from keypoints2body_amd import synthetic
    from keypoints2body_amd.native import NativeModel
    from oracle.smpl_torch import TorchSMPL
    c = synthetic.make_body_model(seed=11, num_vertices=V, num_betas=NB)
    model = NativeModel(c.v_template, c.shapedirs, c.posedirs, c.J_regressor, c.lbs_weights, c.parents, c.extra_vertex_ids)
    rng = np.random.default_rng(V + B)
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32)
    go, bp = t(rng.uniform(-3.0, 3.0, (B, 3))), t(0.6 * rng.standard_normal((B, 69)))
    bp[0] = 0.0                                      # identity rotations in one frame
    be, tr = t(rng.uniform(-2.5, 2.5, (B, NB))), t(rng.uniform(-5.0, 5.0, (B, 3)))
    with torch.no_grad():
        want = TorchSMPL(c)(global_orient=go, body_pose=bp, betas=be, transl=tr)
    j, v = model.lbs(go.cuda(), bp.cuda().contiguous(), be.cuda(), tr.cuda())
    scale = max(1.0, float(want.vertices.abs().max()))
    assert v.shape == (B, V, 3) and j.shape[0] == B
    assert (v.cpu() - want.vertices).abs().max().item() < 5e-6 * scale
    assert (j.cpu() - want.joints).abs().max().item() < 5e-6 * scale
    j2, _ = model.lbs(go.cuda(), bp.cuda().contiguous(), be.cuda(), tr.cuda(), want_vertices=False)
    assert torch.equal(j, j2)


def test_lbs_against_float64_twin():
    from keypoints2body_amd import synthetic
    from oracle.smpl_torch import smpl_forward_np
    p = synthetic.make_poses(3, seed=5)
    j, v = H.native_model().lbs(H.cuda(p.global_orient), H.cuda(p.body_pose), H.cuda(p.betas), H.cuda(p.transl))
    for f in range(3):
        jr, vr = smpl_forward_np(H.body_consts(), p.global_orient[f], p.body_pose[f], p.betas[f], p.transl[f])
        assert np.abs(j[f].cpu().numpy() - jr).max() < 5e-6
        assert np.abs(v[f].cpu().numpy() - vr).max() < 5e-6


@pytest.mark.parametrize("case", ["amass_noisy_conf", "amass_followup", "smpl24_zero_init", "generic_indices"])
def test_fit_gradient_matches_autograd(case):
    """d loss / d params of the HIP analytic backward vs torch autograd on the oracle."""
    from oracle.fit_torch import FitWeights, frame_losses
    d = H.load_case(case)
    out = H.native_fit(d, num_iters=1, want_grad=True)
    g_hip = out["grad"].cpu().numpy()
    t = lambda k: torch.tensor(d[k])
    go, bp, be, tr = (t("init_global_orient").requires_grad_(), t("init_body_pose").requires_grad_(),
                      t("init_betas").requires_grad_(), t("init_transl").requires_grad_())
    idx = H.case_indices(d)
    conf = t("conf") if int(d["has_conf"]) else torch.ones(len(idx))
    mo = H.oracle_model()(global_orient=go, body_pose=bp, betas=be, transl=tr)
    lf = frame_losses(bp, bp.detach().clone() if int(d["seq_ind"]) == 0 else t("init_body_pose"), be,
                      mo.joints[:, idx], t("j3d"), H.oracle_prior(), conf, FitWeights(), int(d["seq_ind"]) > 0)
    lf.sum().backward()
    g_ref = torch.cat([go.grad, bp.grad, be.grad, tr.grad], dim=1).numpy()
    if int(d["freeze_betas"]):
        g_ref[:, 72:82] = 0
    scale = np.abs(g_ref).max(axis=1, keepdims=True)
    assert np.abs(g_hip - g_ref).max() / scale.max() < 2e-5
    np.testing.assert_allclose(out["loss"].cpu().numpy(), lf.detach().numpy(), rtol=2e-6)


@pytest.mark.parametrize("case", H.WORLD_CASES)
def test_fit_matches_reference_golden(case):
    """Fitted parameters after 1/2/10/50/100 Adam steps vs the reference fitter's."""
    d = H.load_case(case)
    worst = 0.0
    for ti, it in enumerate(d["trace_iters"]):
        out = H.native_fit(d, num_iters=int(it))
        for key, tk in (("global_orient", "trace_global_orient"), ("body_pose", "trace_body_pose"),
                        ("betas", "trace_betas"), ("transl", "trace_transl")):
            err = np.abs(out[key].cpu().numpy() - d[tk][ti]).max()
            worst = max(worst, err)
            assert err < PARAM_TOL, f"{case}: {key} after {it} iterations differs by {err}"
    out = H.native_fit(d)
    for key in ("global_orient", "body_pose", "betas", "transl"):
        assert np.abs(out[key].cpu().numpy() - d["out_" + key]).max() < PARAM_TOL
    # loss of the last iteration (before its step): the reference returns the batch sum
    loss = out["loss"].cpu().numpy().astype(np.float64)
    ref = d["out_loss"].astype(np.float64)
    if not int(d["per_frame_calls"]):
        loss = loss.sum(keepdims=True)
    np.testing.assert_allclose(loss, ref, rtol=1e-5)
    # final forward on the fitted parameters
    j, v = H.native_model().lbs(out["global_orient"], out["body_pose"], out["betas"], out["transl"])
    assert np.abs(j.cpu().numpy() - d["out_joints"]).max() < PARAM_TOL
    # matched final joint error: mean distance fitted joint - target equals the reference's to 1e-5 m
    idx = H.case_indices(d)
    jerr = lambda joints: np.linalg.norm(joints[:, idx] - d["j3d"], axis=-1).mean()     # target row k <-> model joint idx[k]
    assert abs(jerr(j.cpu().numpy()) - jerr(d["out_joints"])) < 1e-5, case
    vs = v[:, torch.as_tensor(d["sampled_vertex_ids"]).cuda()].cpu().numpy()
    assert np.abs(vs - d["out_verts_sampled"]).max() < PARAM_TOL
    assert np.abs(v.double().sum(dim=1).cpu().numpy() - d["out_verts_sum"]).max() < 6890 * 2e-5
    print(f"{case}: worst parameter deviation over the trace = {worst:.2e}")


@pytest.mark.parametrize("shape", ["split", "split_paired", "paired", "wide"])
def test_every_launch_shape_matches_reference_golden(shape):
    """The fit kernel has four launch shapes (row + tree wave per frame, row + tree wave per two frames, one wave for two
    frames, and the 16-wave shape of round 4: eight row waves with two frames + one component each, eight tree waves).  `k2b_fit_config.debug_launch_shape` forces a shape so that each one is pinned to the reference
    goldens, including a ragged batch that leaves half a paired wave and several MFMA columns empty."""
    for case in ("amass_batched", "amass_followup", "smpl24_zero_init"):
        d = H.load_case(case)
        out = H.native_fit(d, shape=shape)
        for key in ("global_orient", "body_pose", "betas", "transl"):
            err = np.abs(out[key].cpu().numpy() - d["out_" + key]).max()
            assert err < PARAM_TOL, f"{shape}/{case}: {key} differs by {err}"


def test_launch_shapes_agree_bitwise_on_a_ragged_batch():
    """Same arithmetic in every shape: loss and gradient of 37 frames (up to 10 workgroups with ragged tails) are bit-identical across shapes."""
    from keypoints2body_amd import native, synthetic
    B = 37
    m, pr = H.native_model(), H.native_prior()
    p = synthetic.make_poses(B, seed=11)
    go, bp, be, tr = map(H.cuda, (p.global_orient, p.body_pose, p.betas, p.transl))
    j, _ = m.lbs(go, bp, be, tr, want_vertices=False)
    j3d = (j[:, :22] + 0.01).contiguous()
    cfg = native.default_fit_config(); cfg.num_iters = 3
    res = {}
    for shape in ("split", "split_paired", "paired", "wide"):
        cfg.debug_launch_shape = H.LAUNCH_SHAPES[shape]
        res[shape] = native.fit_world(m, pr, cfg, list(range(22)), j3d, None, go * 0.9, bp * 0.9, be * 0.5, tr, want_grad=True)
    for shape in ("split_paired", "paired", "wide"):
        for k in ("global_orient", "body_pose", "betas", "transl", "loss", "grad"):
            assert torch.equal(res["split"][k], res[shape][k]), f"{shape}: {k}"


@pytest.mark.parametrize("shape", ["split", "split_paired", "paired", "wide"])
def test_sixteen_beta_model_matches_oracle(shape):
    """Models with more than 10 betas run the 16-beta instantiation of the fit kernel.  No reference golden
    exists for that size (the reference ships 10-beta SMPL); the oracle restatement - pinned to the reference
    on the 10-beta cases - is the checker here, on a 16-beta synthetic model with a small mesh."""
    from keypoints2body_amd import native, synthetic
    from keypoints2body_amd.native import NativeModel
    from oracle.fit_torch import fit_world_adam
    from oracle.smpl_torch import TorchSMPL
    c = synthetic.make_body_model(seed=3, num_vertices=512, num_betas=16)
    model = NativeModel(c.v_template, c.shapedirs, c.posedirs, c.J_regressor, c.lbs_weights, c.parents, c.extra_vertex_ids)
    oracle = TorchSMPL(c)
    B, iters = 3, 25
    p = synthetic.make_poses(B, seed=5)
    t = lambda x: torch.as_tensor(np.asarray(x), dtype=torch.float32)
    betas_true = torch.linspace(-1.0, 1.0, 16).repeat(B, 1) * 0.5
    with torch.no_grad():
        j3d = oracle(global_orient=t(p.global_orient), body_pose=t(p.body_pose), betas=betas_true, transl=t(p.transl)).joints[:, :22]
    go0, bp0, be0 = t(p.global_orient) * 0.8, t(p.body_pose) * 0.8, torch.zeros(B, 16)
    tr0 = t(p.transl) + 0.02
    ref = fit_world_adam(oracle, H.oracle_prior(), go0, bp0, be0, tr0, j3d, num_iters=iters)
    cfg = native.default_fit_config(); cfg.num_iters = iters
    cfg.debug_launch_shape = H.LAUNCH_SHAPES[shape]
    out = native.fit_world(model, H.native_prior(), cfg, list(range(22)), j3d.cuda().contiguous(), None,
                           go0.cuda(), bp0.cuda(), be0.cuda(), tr0.cuda())
    for key, want in (("global_orient", ref.global_orient), ("body_pose", ref.body_pose), ("betas", ref.betas), ("transl", ref.transl)):
        err = (out[key].cpu() - want).abs().max().item()
        assert err < PARAM_TOL, (shape, key, err)
    assert out["betas"].abs().max() > 1e-3          # the sixteen betas did move


def test_ill_conditioned_prior_matches_oracle():
    """The mixture prior runs on f16-split MFMA operands (two f16 terms per precision entry, power-of-two
    scale per component).  A prior far harsher than the goldens' - precision entries above 1e4, condition
    numbers above 1e4, components of very different scale, 5 components instead of 8 - must still reproduce the
    CPU float32 arithmetic of the reference's formulation (oracle) within the parity budget."""
    from keypoints2body_amd import native, synthetic
    from keypoints2body_amd.native import NativePrior
    from oracle.fit_torch import GMMPrior, fit_world_adam
    rng = np.random.default_rng(17)
    M = 5
    means = 0.3 * rng.standard_normal((M, 69))
    covars = np.zeros((M, 69, 69))
    for m in range(M):
        A = rng.standard_normal((69, 12)) * (0.02 * 1.4 ** m)
        covars[m] = A @ A.T + np.diag(10.0 ** rng.uniform(-5.0, -1.0, 69))
    prior_o = GMMPrior(means, covars, np.full(M, 1.0 / M))
    P = prior_o.precisions.numpy()
    assert np.abs(P).max() > 1e4 and np.linalg.cond(P[M - 1].astype(np.float64)) > 1e4 and (prior_o.nll_weights > 0).all()
    prior_n = NativePrior(prior_o.means.numpy(), P, prior_o.nll_weights.numpy().reshape(-1))
    B, iters = 4, 30
    p = synthetic.make_poses(B, seed=9)
    t = lambda x: torch.as_tensor(np.asarray(x), dtype=torch.float32)
    oracle = H.oracle_model()
    with torch.no_grad():
        j3d = oracle(global_orient=t(p.global_orient), body_pose=t(p.body_pose), betas=t(p.betas), transl=t(p.transl)).joints[:, :22]
    go0, bp0, be0, tr0 = t(p.global_orient) * 0.7, t(p.body_pose) * 0.7, torch.zeros(B, 10), t(p.transl) + 0.01
    ref = fit_world_adam(oracle, prior_o, go0, bp0, be0, tr0, j3d, num_iters=iters)
    cfg = native.default_fit_config(); cfg.num_iters = iters
    out = native.fit_world(H.native_model(), prior_n, cfg, list(range(22)), j3d.cuda().contiguous(), None,
                           go0.cuda(), bp0.cuda(), be0.cuda(), tr0.cuda())
    for key, want in (("global_orient", ref.global_orient), ("body_pose", ref.body_pose), ("betas", ref.betas), ("transl", ref.transl)):
        err = (out[key].cpu() - want).abs().max().item()
        assert err < PARAM_TOL, (key, err)
    np.testing.assert_allclose(out["loss"].cpu().numpy(), ref.loss.numpy(), rtol=2e-4)


@pytest.mark.parametrize("shape", [1, 2, 3, 4])
def test_rim_heavy_prior_matches_oracle_in_every_shape(shape):
    """Rows 64..68 of every precision matrix ride on the matrix cores as a fifth row tile whose f16 fragments share the
    component's power-of-two scale (k2b_api_prior.hip, k2b_fit.hip).  Here the last five pose dimensions are near-linear functions
    of the first 64 (x_B = C x_A + noise of variance 1e-4), so P_BA = -C / sigma^2 carries entries as large as anything in the
    core and P_BB = I / sigma^2 the largest of all: the fit must still follow the CPU float32 arithmetic of the reference's
    formulation (oracle) within the parity budget, in each launch shape."""
    from keypoints2body_amd import native, synthetic
    from keypoints2body_amd.native import NativePrior
    from oracle.fit_torch import GMMPrior, fit_world_adam
    rng = np.random.default_rng(23)
    M = 8
    means = 0.2 * rng.standard_normal((M, 69))
    covars = np.zeros((M, 69, 69))
    for m in range(M):
        A = rng.standard_normal((64, 10)) * 0.05
        S = A @ A.T + np.diag(10.0 ** rng.uniform(-3.0, -1.0, 64))
        C = 0.3 * rng.standard_normal((5, 64)) / 8.0
        covars[m, :64, :64] = S
        covars[m, 64:, :64] = C @ S
        covars[m, :64, 64:] = (C @ S).T
        covars[m, 64:, 64:] = C @ S @ C.T + 1e-4 * np.eye(5)
    prior_o = GMMPrior(means, covars, np.full(M, 1.0 / M))
    P = prior_o.precisions.numpy()
    assert np.abs(P[:, 64:, :64]).max() > 0.05 * np.abs(P[:, :64, :64]).max() and np.abs(P[:, 64:, 64:]).max() > 5e3
    prior_n = NativePrior(prior_o.means.numpy(), P, prior_o.nll_weights.numpy().reshape(-1))
    B, iters = 5, 25
    p = synthetic.make_poses(B, seed=11)
    t = lambda x: torch.as_tensor(np.asarray(x), dtype=torch.float32)
    oracle = H.oracle_model()
    with torch.no_grad():
        j3d = oracle(global_orient=t(p.global_orient), body_pose=t(p.body_pose), betas=t(p.betas), transl=t(p.transl)).joints[:, :22]
    go0, bp0, be0, tr0 = t(p.global_orient) * 0.8, t(p.body_pose) * 0.8, torch.zeros(B, 10), t(p.transl) + 0.01
    ref = fit_world_adam(oracle, prior_o, go0, bp0, be0, tr0, j3d, num_iters=iters)
    cfg = native.default_fit_config(); cfg.num_iters = iters; cfg.debug_launch_shape = shape
    out = native.fit_world(H.native_model(), prior_n, cfg, list(range(22)), j3d.cuda().contiguous(), None,
                           go0.cuda(), bp0.cuda(), be0.cuda(), tr0.cuda())
    worst = 0.0
    for key, want in (("global_orient", ref.global_orient), ("body_pose", ref.body_pose), ("betas", ref.betas), ("transl", ref.transl)):
        err = (out[key].cpu() - want).abs().max().item()
        worst = max(worst, err)
        assert err < PARAM_TOL, (shape, key, err)
    np.testing.assert_allclose(out["loss"].cpu().numpy(), ref.loss.numpy(), rtol=2e-4)
    print(f"rim-heavy prior, shape {shape}: worst parameter deviation {worst:.2e}")


def test_underflowed_mixture_weight_is_never_selected():
    """A mixture weight that underflows to 0 in float32 gives log(0) = -inf in the reference (prior.py:189):
    that component can never be the arg-min.  Same here: with component 0's weight set to 0 the result equals
    the fit with that component removed."""
    from keypoints2body_amd import native
    from keypoints2body_amd.native import NativePrior
    g = H.gmm_fixture()
    w = g["ref_nll_weights"].reshape(-1).copy()
    w0 = w.copy(); w0[0] = 0.0
    with_zero = NativePrior(g["ref_means"], g["ref_precisions"], w0)
    without = NativePrior(g["ref_means"][1:], g["ref_precisions"][1:], w[1:])
    d = H.load_case("amass_noisy_conf")
    dev = lambda k: H.cuda(d[k])
    cfg = native.default_fit_config(); cfg.num_iters = 20
    run = lambda pr: native.fit_world(H.native_model(), pr, cfg, list(range(22)), dev("j3d"), H.cuda(d["conf"]),
                                      dev("init_global_orient"), dev("init_body_pose"), dev("init_betas"), dev("init_transl"))
    a, b = run(with_zero), run(without)
    for k in ("global_orient", "body_pose", "betas", "transl", "loss"):
        assert torch.isfinite(a[k]).all()
        assert (a[k] - b[k]).abs().max() < 1e-6, k
    with pytest.raises(ValueError):
        NativePrior(g["ref_means"], g["ref_precisions"], -w)


def test_fit_is_deterministic_and_frames_are_independent():
    d = H.load_case("amass_noisy_conf")
    a = H.native_fit(d)
    b = H.native_fit(d)
    for k in ("global_orient", "body_pose", "betas", "transl", "loss"):
        assert torch.equal(a[k], b[k])
    sub = H.native_fit(d, rows=slice(2, 5))
    for k in ("global_orient", "body_pose", "betas", "transl", "loss"):
        assert torch.equal(a[k][2:5], sub[k])


def test_vertex_joint_targets_through_the_c_call_match_reference_golden():
    """k2b_fit_world with vertex-selected joints among the targets (two launches per iteration queued by the one call)
    against the reference's end state; a target list WITHOUT a kinematic joint is refused."""
    from keypoints2body_amd import native
    d = H.load_case("generic_vertex_joints")
    out = H.native_fit(d)
    for k in ("global_orient", "body_pose", "betas", "transl"):
        assert np.abs(out[k].cpu().numpy() - d["out_" + k]).max() < 1e-4, k
    np.testing.assert_allclose(out["loss"].cpu().numpy(), d["out_loss"], rtol=2e-5)
    idx = [i for i in H.case_indices(d) if i >= 24]
    cols = [k for k, i in enumerate(H.case_indices(d)) if i >= 24]
    cfg = native.default_fit_config()
    with pytest.raises(NotImplementedError):
        native.fit_world(H.native_model(), H.native_prior(), cfg, idx, H.cuda(d["j3d"][:, cols]), None,
                         H.cuda(d["init_global_orient"]), H.cuda(d["init_body_pose"]), H.cuda(d["init_betas"]), H.cuda(d["init_transl"]))


def test_vertex_joint_term_gradient_matches_autograd():
    """k2b_vertex_term: loss and analytic gradient of the joint loss on vertex-selected joints (blend shapes, LBS
    and chain differentiated by hand) against torch autograd through the oracle's SMPL forward."""
    from keypoints2body_amd import native, synthetic
    from oracle.fit_torch import gmof
    B = 3
    sel = [0, 1, 6, 13, 20]
    p = synthetic.make_poses(B, seed=21)
    t = lambda x: torch.as_tensor(np.asarray(x), dtype=torch.float32)
    go, bp, be, tr = (t(p.global_orient).requires_grad_(), t(p.body_pose).requires_grad_(), t(p.betas).requires_grad_(),
                      t(p.transl).requires_grad_())
    oracle = H.oracle_model()
    joints = oracle(global_orient=go, body_pose=bp, betas=be, transl=tr).joints
    gen = torch.Generator().manual_seed(3)
    tgt = (joints[:, [24 + e for e in sel]].detach() + 0.05 * torch.randn(B, len(sel), 3, generator=gen))
    conf = torch.tensor([1.0, 0.7, 1.5, 1.0, 0.9])
    lf = ((600.0 ** 2) * (conf ** 2).view(1, -1, 1) * gmof(joints[:, [24 + e for e in sel]] - tgt, 100.0)).sum(dim=(1, 2))
    lf.sum().backward()
    g_ref = torch.cat([go.grad, bp.grad, be.grad, tr.grad], dim=1).numpy()
    loss, grad = native.vertex_term(H.native_model(), sel, tgt.cuda().contiguous(), conf.cuda(), 100.0, 600.0,
                                    go.detach().cuda(), bp.detach().cuda(), be.detach().cuda(), tr.detach().cuda())
    np.testing.assert_allclose(loss.cpu().numpy(), lf.detach().numpy(), rtol=2e-5)
    g = grad.cpu().numpy()
    for name, sl in (("global_orient", slice(0, 3)), ("body_pose", slice(3, 72)), ("betas", slice(72, 82)), ("transl", slice(82, 85))):
        scale = np.abs(g_ref[:, sl]).max()
        assert np.abs(g[:, sl] - g_ref[:, sl]).max() / scale < 5e-5, name


def _random_configuration(seed):
    """One seeded fitting problem with everything the path branches on drawn at random: batch size, iteration
    count, target subset and order, confidences (zeros and values above 1), every loss weight (some zero), the
    GMoF sigma, frozen shape, first / follow-up frame, and the kind of start (zeros, a perturbed copy of the true
    pose, rotations of almost pi)."""
    from keypoints2body_amd import synthetic
    rng = np.random.default_rng(seed)
    B = int(rng.integers(1, 8))
    K = int(rng.integers(6, 25))
    model_idx = sorted(rng.choice(24, size=K, replace=False).tolist())
    model_idx = [model_idx[i] for i in rng.permutation(K)]
    if 0 not in model_idx:                      # keep the root observed so that the translation is determined
        model_idx[0] = 0
    p = synthetic.make_poses(B, seed=100 + seed)
    t = lambda x: torch.as_tensor(np.asarray(x), dtype=torch.float32)
    truth = dict(global_orient=t(p.global_orient), body_pose=t(p.body_pose), betas=t(p.betas), transl=t(p.transl))
    kind = ("zeros", "perturbed", "large")[seed % 3]
    if kind == "zeros":
        init = dict(global_orient=torch.zeros(B, 3), body_pose=torch.zeros(B, 69), betas=torch.zeros(B, 10))
    elif kind == "perturbed":
        init = dict(global_orient=truth["global_orient"] + 0.1, body_pose=truth["body_pose"] * 0.7 + 0.02,
                    betas=truth["betas"] * 0.3)
        init["body_pose"][:, 6:12] = 0.0        # a few joints exactly at the identity rotation
    else:
        axis = t(rng.standard_normal((B, 3))); axis = axis / axis.norm(dim=1, keepdim=True)
        init = dict(global_orient=axis * 3.1, body_pose=truth["body_pose"] * 1.5, betas=t(rng.uniform(-2, 2, (B, 10))))
    conf = t(rng.choice([0.0, 0.5, 1.0, 1.5], size=K, p=[0.15, 0.2, 0.45, 0.2]))
    conf[model_idx.index(0)] = 1.0
    pick = lambda *v: float(rng.choice(v))
    weights = dict(sigma=pick(30.0, 100.0, 300.0), pose_prior_weight=pick(0.0, 4.78 * 1.5, 12.0),
                   shape_prior_weight=pick(0.0, 5.0, 20.0), angle_prior_weight=pick(0.0, 15.2),
                   joint_loss_weight=pick(100.0, 600.0), pose_preserve_weight=pick(1.0, 5.0))
    return dict(B=B, iters=int(rng.integers(3, 31)), model_idx=model_idx, conf=conf if seed % 4 else None,
                truth=truth, init=init, weights=weights, seq_ind=int(seed % 2) * 3, freeze_betas=bool(seed % 5 == 0),
                noise=t(0.01 * rng.standard_normal((B, K, 3))), kind=kind)


@pytest.mark.parametrize("seed", list(range(1, 13)))
def test_random_configurations_match_oracle(seed):
    """Seeded sweep over the configuration space against the oracle (itself pinned to the reference on the golden
    cases), each case in one of the three launch shapes: parameters within 1e-4, last-iteration loss within 2e-4
    relative."""
    from keypoints2body_amd import native
    shape = ("split", "split_paired", "paired", "wide")[seed % 4]
    from oracle.fit_torch import FitWeights, fit_world_adam, guess_init_transl
    c = _random_configuration(seed)
    oracle = H.oracle_model()
    with torch.no_grad():
        joints = oracle(**c["truth"]).joints
    j3d = joints[:, c["model_idx"]] + c["noise"]
    init = c["init"]
    with torch.no_grad():
        j0 = oracle(global_orient=init["global_orient"], body_pose=init["body_pose"], betas=init["betas"]).joints
    root = c["model_idx"].index(0)
    tr0 = (j3d[:, root] - j0[:, 0]) + 0.01          # a start off the root-aligned one: no zero-gradient first step
    ref = fit_world_adam(oracle, H.oracle_prior(), init["global_orient"], init["body_pose"], init["betas"], tr0, j3d,
                         c["conf"], num_iters=c["iters"], seq_ind=c["seq_ind"], model_idx=c["model_idx"],
                         weights=FitWeights(**c["weights"]), freeze_betas=c["freeze_betas"])
    cfg = native.default_fit_config()
    cfg.num_iters = c["iters"]
    cfg.debug_launch_shape = H.LAUNCH_SHAPES[shape]
    for k, v in c["weights"].items():
        setattr(cfg, k, v)
    if c["seq_ind"] == 0:
        cfg.pose_preserve_weight = 0.0
    cfg.freeze_betas = int(c["freeze_betas"])
    out = native.fit_world(H.native_model(), H.native_prior(), cfg, c["model_idx"], j3d.cuda().contiguous(),
                           None if c["conf"] is None else c["conf"].cuda(), init["global_orient"].cuda(),
                           init["body_pose"].cuda().contiguous(), init["betas"].cuda(), tr0.cuda().contiguous())
    tag = (seed, shape, c["kind"], c["B"], c["iters"], len(c["model_idx"]))
    worst = 0.0
    for key, want in (("global_orient", ref.global_orient), ("body_pose", ref.body_pose), ("betas", ref.betas), ("transl", ref.transl)):
        err = (out[key].cpu() - want).abs().max().item()
        worst = max(worst, err)
        assert err < PARAM_TOL, (tag, key, err)
    print(f"random configuration {tag}: worst parameter deviation {worst:.2e}")
    np.testing.assert_allclose(out["loss"].cpu().numpy(), ref.loss.numpy(), rtol=2e-4, err_msg=str(tag))
    if c["freeze_betas"]:
        assert torch.equal(out["betas"].cpu(), init["betas"])
