"""GPU: autograd through ``BodyModel`` - ``k2b_lbs`` forward, ``k2b_lbs_backward`` backward - against the CPU oracle in float64
(gate: ``tests/lbs_backward_common.py``), the unchanged detached path, the fitters' detached results, and a dense mesh
registration written in torch."""
import numpy as np
import pytest
import torch

import keypoints2body_amd as k2b
from keypoints2body_amd.models.body_model import BodyModel
from keypoints2body_amd.prior import MaxMixturePrior, MixtureBuffers
from tests import helpers as H
from tests import lbs_backward_common as C

pytestmark = pytest.mark.gpu
V = 1100
POSE_KEYS = {"smpl": ("body_pose",), "smplh": ("body_pose", "left_hand_pose", "right_hand_pose"), "smplx20": C.POSE_ORDER}


@pytest.fixture(scope="module")
def models():
    cache = {}

    def get(kind):
        if kind not in cache:
            c = C.consts(kind, V)
            cache[kind] = BodyModel(c.v_template, c.shapedirs, c.posedirs, c.J_regressor, c.lbs_weights, c.parents,
                                    c.extra_vertex_ids, model_type=kind[:5], num_betas=C.NUM_BETAS.get(kind),
                                    landmarks=C.landmarks(kind, V))
        return cache[kind]
    return get


def _loss_weights(model, B, seed=21):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((B, model.num_output_joints, 3)).astype(np.float32),
            rng.standard_normal((B, V, 3)).astype(np.float32))


def _keyword_grads(kind, model, f, wj, wv):
    """Gradients of (w_v . vertices).sum() + (w_j . joints).sum() for every keyword of `f` through BodyModel."""
    leaves = {k: H.cuda(v).requires_grad_(True) for k, v in f.items()}
    out = model(**leaves)
    assert out.vertices.requires_grad and out.joints.requires_grad
    loss = (H.cuda(wv) * out.vertices).sum() + (H.cuda(wj) * out.joints).sum()
    return dict(zip(leaves, torch.autograd.grad(loss, list(leaves.values()))))


def _oracle_keyword_grads(kind, f, wj, wv, double):
    """The same through the oracle on packed parameters, split back into the keywords' slices (a one-row keyword broadcast
    over the batch receives the sum)."""
    B = max(v.shape[0] for v in f.values())
    full = {k: np.broadcast_to(v, (B, v.shape[1])) for k, v in f.items()}
    pose = np.concatenate([full[k] for k in POSE_KEYS[kind]], axis=1)
    shape = np.concatenate([full[k] for k in ("betas", "expression") if k in full], axis=1)
    g = C.oracle_grads(kind, V, (full["global_orient"], pose, shape, full["transl"]), wj, wv, double)
    out, o = {"global_orient": g["global_orient"], "transl": g["transl"]}, 0
    for k in POSE_KEYS[kind]:
        out[k] = g["body_pose"][:, o:o + f[k].shape[1]]
        o += f[k].shape[1]
    o = 0
    for k in ("betas", "expression"):
        if k in f:
            out[k] = g["betas"][:, o:o + f[k].shape[1]]
            o += f[k].shape[1]
    return {k: (v.sum(dim=0, keepdim=True) if f[k].shape[0] != B else v) for k, v in out.items()}


def _gate(name, got, g64, g32):
    err = lambda a, b: {k: float(((a[k].detach().cpu().double() - b[k].double()).abs().amax(dim=1)
                                  / b[k].double().abs().amax(dim=1)).max()) for k in b}
    e32 = max(err(g32, g64).values())
    tol = max(2e-5, 4.0 * e32)
    e = err(got, g64)
    print(f"{name}: " + " ".join(f"{k}={v:.2e}" for k, v in e.items()) + f" e32={e32:.2e} tol={tol:.2e}")
    for k, v in e.items():
        assert tuple(got[k].shape) == tuple(g64[k].shape), k
        assert v <= tol, (name, k, v, tol)


@pytest.mark.parametrize("kind", ["smpl", "smplh", "smplx20"])
def test_gradients_of_every_keyword_match_the_oracle(models, kind):
    B = 3
    model = models(kind)
    f = C.fields(kind, B, seed=13)
    if kind == "smplx20":
        f["betas"] = f["betas"][:1]                       # a (1, 10) betas broadcast over the three frames: receives the sum
    wj, wv = _loss_weights(model, B)
    got = _keyword_grads(kind, model, f, wj, wv)
    _gate(kind, got, _oracle_keyword_grads(kind, f, wj, wv, True), _oracle_keyword_grads(kind, f, wj, wv, False))


def test_only_transl_requires_grad(models):
    model = models("smpl")
    f = {k: H.cuda(v) for k, v in C.fields("smpl", 2, seed=3).items()}
    f["transl"].requires_grad_(True)
    out = model(**f)
    out.vertices.square().sum().backward()
    assert f["transl"].grad is not None and all(f[k].grad is None for k in ("global_orient", "body_pose", "betas"))
    ref = 2.0 * out.vertices.detach().sum(dim=1)
    assert torch.allclose(f["transl"].grad, ref, rtol=1e-4, atol=1e-4 * float(ref.abs().max()))


def test_without_a_gradient_the_path_is_the_detached_one(models):
    model = models("smpl")
    f = {k: H.cuda(v) for k, v in C.fields("smpl", 3, seed=4).items()}
    joints, verts = model.native.lbs(f["global_orient"], f["body_pose"], f["betas"], f["transl"])
    out = model(**f)
    assert out.vertices.requires_grad is False and out.vertices.grad_fn is None
    assert torch.equal(out.vertices, verts) and torch.equal(out.joints, joints)
    g = {k: v.clone().requires_grad_(True) for k, v in f.items()}
    with torch.no_grad():
        out = model(**g)
    assert out.vertices.requires_grad is False and out.joints.requires_grad is False
    assert torch.equal(out.vertices, verts) and torch.equal(out.joints, joints)


def test_fitter_results_stay_detached():
    g = H.gmm_fixture()
    prior = MaxMixturePrior(MixtureBuffers(g["ref_means"], g["ref_precisions"], g["ref_nll_weights"].reshape(-1)))
    model = BodyModel.synthetic(0)
    d = H.load_case("amass_zero_init")
    prev = k2b.SMPLData(betas=torch.tensor(d["init_betas"][:1], requires_grad=True),
                        global_orient=torch.tensor(d["init_global_orient"][:1], requires_grad=True),
                        body_pose=torch.tensor(d["init_body_pose"][:1], requires_grad=True), transl=None)
    res = k2b.optimize_params_frame(d["j3d"][0], prev_params=prev, joint_layout="AMASS", model=model, pose_prior=prior,
                                    config={"use_lbfgs": False, "num_iters_first": 5})
    for t in (res.params.betas, res.params.global_orient, res.params.body_pose, res.params.transl, res.joints, res.vertices):
        assert isinstance(t, torch.Tensor) and not t.requires_grad and t.grad_fn is None


def test_dense_registration_with_adam(models):
    """Fit BodyModel vertices to the mesh of a perturbed pose and shape: 20 Adam steps on the mean squared vertex distance, the
    identical loop on the CPU oracle in float32.  Measured on an MI355X: see DESIGN.md (LBS backward)."""
    kind, B, steps = "smpl", 2, 20
    model = models(kind)
    base = C.fields(kind, B, seed=17)
    rng = np.random.default_rng(5)
    target_f = {k: (v + 0.1 * rng.standard_normal(v.shape)).astype(np.float32) for k, v in base.items()}
    ref = C.oracle(kind, V, False)
    with torch.no_grad():
        target = ref(**{k: torch.tensor(v) for k, v in target_f.items()}).vertices

    def run(forward, to):
        leaves = {k: to(torch.tensor(v)).requires_grad_(True) for k, v in base.items()}
        opt = torch.optim.Adam(list(leaves.values()), lr=1e-2)
        tgt, losses = to(target), []
        for _ in range(steps + 1):                        # the last pass only evaluates the loss after `steps` steps
            opt.zero_grad()
            loss = (forward(**leaves).vertices - tgt).square().sum(dim=-1).mean()
            losses.append(float(loss.detach()))
            if len(losses) <= steps:
                loss.backward()
                opt.step()
        return losses

    dev = run(model, lambda t: t.cuda())
    cpu = run(ref, lambda t: t)
    print(f"dense registration: loss {dev[0]:.6e} -> {dev[-1]:.6e} (oracle loop {cpu[-1]:.6e}), ratio {dev[-1] / cpu[-1]:.5f}")
    assert dev[-1] < 0.5 * dev[0]
    assert dev[-1] <= 1.05 * cpu[-1]
