"""GPU: the forward (``k2b_lbs``) and every public entry that ends in it for 55-joint models with 25-32 shape coefficients -
9 x 54 + NB + 2 = 513..520 features, 34 sixteen-deep k-steps of the pose set-up, 17 thirty-two-deep ones of the skinning kernel
(``k2b_lbs_stream_xw_kernel``, the third description of ``csrc/k2b_lbs_stream.hip``).  16 betas | 10 expression coefficients
(NB = 26) is the layout of the AMASS SMPL-X files.

The model is that of ``tests/test_gpu_lbfgs_wide.py``: ``synthetic.make_body_model_x(0, num_vertices=1100, num_shape=nb)`` -
1100 vertices are 69 sixteen-vertex tiles padded to 72, nine vertex groups of which the last has empty waves (the partial-tile
wait counts).  The oracle is the CPU forward of the same constants, the gate the project's LBS gate (5e-6 m, DESIGN.md
section 3, ``tests/test_gpu_smplx.py``); parameter scales as ``_problem`` there (root 0.2, pose 0.15, shape 0.3, translation 1.0).

The tile kernel is the stream kernels' run-time twin: a model created under ``K2B_LBS_TILE=1`` is skinned by
``k2b_lbs_tile_kernel`` (``<7, 6>`` for 49-56 joints, ``<3, 12>`` for 17-24) whatever the stream kernels would take."""
import os

import numpy as np
import pytest
import torch

from keypoints2body_amd import native, synthetic
from tests import helpers as H

pytestmark = pytest.mark.gpu

GATE = 5e-6                                   # metres: the LBS gate
NUM_BETAS = {20: 10, 25: 15, 26: 16, 32: 22}  # shape coefficients -> betas (the rest: 10 expression coefficients)
TILE_SWITCH = "K2B_LBS_TILE"
_cache = {}


def _memo(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _consts(nb, V=1100):
    return _memo(("consts", nb, V), lambda: synthetic.make_body_model_x(0, num_vertices=V, num_shape=nb))


def _native(c, landmarks=None):
    return native.NativeModel(c.v_template, c.shapedirs, c.posedirs, c.J_regressor, c.lbs_weights, c.parents, c.extra_vertex_ids,
                              landmarks=landmarks)


def _model(nb, V=1100):
    return _memo(("model", nb, V), lambda: _native(_consts(nb, V)))


def _twin(monkeypatch, key, consts):
    """The model of `consts` created under the development switch: the tile kernel skins it.  The variable is set around the
    creation only (the switch is read there, per model)."""
    def make():
        with monkeypatch.context() as mp:
            mp.setenv(TILE_SWITCH, "1")
            return _native(consts)
    return _memo(("twin",) + key, make)


def _landmarks():
    return _memo("landmarks", lambda: synthetic.make_landmarks(num_vertices=1100))


def _params(nb, B, seed):
    """(global_orient, packed pose 162, betas | expression, transl) as float32 arrays."""
    rng = np.random.default_rng(seed)
    f = lambda x: x.astype(np.float32)
    return (f(0.2 * rng.standard_normal((B, 3))), f(0.15 * rng.standard_normal((B, 162))), f(0.3 * rng.standard_normal((B, nb))),
            f(rng.standard_normal((B, 3))))


def _oracle(nb, V, B, seed):
    """The oracle's forward of ``_params(nb, B, seed)``, computed once: (vertices (B, V, 3), joints (B, 127, 3)) on the CPU."""
    def make():
        from oracle.smpl_torch import TorchSMPLX
        m = _memo(("oracle", nb, V), lambda: TorchSMPLX(_consts(nb, V), num_betas=NUM_BETAS[nb]))
        go, pose, shape, tr = map(torch.from_numpy, _params(nb, B, seed))
        k = NUM_BETAS[nb]
        with torch.no_grad():
            o = m(global_orient=go, body_pose=pose[:, :63], jaw_pose=pose[:, 63:66], leye_pose=pose[:, 66:69], reye_pose=pose[:, 69:72],
                  left_hand_pose=pose[:, 72:117], right_hand_pose=pose[:, 117:162], betas=shape[:, :k], expression=shape[:, k:], transl=tr)
        return o.vertices, o.joints
    return _memo(("ref", nb, V, B, seed), make)


def _lbs(model, nb, B, seed, want_vertices=True):
    return model.lbs(*map(H.cuda, _params(nb, B, seed)), want_vertices=want_vertices)


def _err(a, b):
    return float((a.cpu() - b).abs().max())


def _check_forward(model, nb, V, B, seed, what):
    ref_v, ref_j = _oracle(nb, V, B, seed)
    j, v = _lbs(model, nb, B, seed)
    assert tuple(j.shape) == (B, 127, 3) and tuple(v.shape) == (B, V, 3)
    ev, ej = _err(v, ref_v), _err(j, ref_j)
    j2, none = _lbs(model, nb, B, seed, want_vertices=False)          # the 72 vertex-selected joints skinned alone
    ej2 = _err(j2, ref_j)
    print(f"{what}: NB {nb} V {V} B {B}: vertices {ev:.3e} joints {ej:.3e} joints alone {ej2:.3e}")
    assert none is None and torch.isfinite(v).all() and torch.isfinite(j).all()
    assert ev < GATE and ej < GATE and ej2 < GATE, (what, nb, V, B, ev, ej, ej2)
    return j, v


# ---- 1. forward against the oracle ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [25, 26, 32])
def test_wide_forward_matches_the_oracle(nb):
    """25: the first size over the 16-k-step kernel's 24 coefficients; 26 and 32: the sizes of the optimiser's tests.  B = 37 is one
    full and one partial 32-frame tile."""
    _check_forward(_model(nb), nb, 1100, 37, seed=4, what="forward")


def test_wide_forward_with_landmarks():
    """55 joints, 72 vertex-selected joints and 51 landmarks, with the mesh and from the 153 landmark vertices skinned alone."""
    nb, B = 26, 37
    ids, bary = _landmarks()
    m = _memo("lmk_model", lambda: _native(_consts(nb), landmarks=_landmarks()))
    ref_v, ref_j = _oracle(nb, 1100, B, 4)
    lmk = (ref_v[:, torch.as_tensor(ids.reshape(-1), dtype=torch.long)].reshape(B, -1, 3, 3) * torch.as_tensor(bary)[None, :, :, None]).sum(dim=2)
    ref = torch.cat([ref_j, lmk], dim=1)
    j, v = _lbs(m, nb, B, 4)
    j2, _ = _lbs(m, nb, B, 4, want_vertices=False)
    assert tuple(j.shape) == tuple(j2.shape) == (B, 127 + 51, 3)
    e = (_err(v, ref_v), _err(j, ref), _err(j2, ref))
    print(f"landmarks: vertices {e[0]:.3e} joints {e[1]:.3e} joints alone {e[2]:.3e}")
    assert max(e) < GATE, e


# ---- 2. the tile walk -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,B", [(1100, 1), (1100, 129), (1100, 300), (10475, 129)])
def test_wide_forward_walks_several_tiles(V, B):
    """More tiles than workgroups need at once / a ragged last frame group: a persistent workgroup walks more than one tile (the
    Pd buffers of the next tile's first two k-steps are handed over at the end of a tile) and the last frame group takes the
    predicated stores.  One case on the full-size mesh (82 vertex groups x 2 frame groups)."""
    _check_forward(_model(26, V), 26, V, B, seed=11, what="tile walk")


# ---- 3. the tile kernel as twin -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [26, 20])
def test_stream_and_tile_kernels_agree_with_the_oracle_smplx(nb, monkeypatch):
    """26: ``k2b_lbs_stream_xw_kernel`` against ``k2b_lbs_tile_kernel<7, 6>`` at 34 k-steps; 20: ``k2b_lbs_stream_x_kernel``
    against the same instantiation at 32.  Each route within the gate of the oracle (hence within twice the gate of each other)."""
    twin = _twin(monkeypatch, (nb,), _consts(nb))
    assert TILE_SWITCH not in os.environ
    for B, seed in ((37, 4), (300, 11)):
        a = _check_forward(_model(nb), nb, 1100, B, seed, what="default route")
        b = _check_forward(twin, nb, 1100, B, seed, what="tile twin")
        print(f"NB {nb} B {B}: default - twin: vertices {_err(a[1], b[1].cpu()):.3e} joints {_err(a[0], b[0].cpu()):.3e}")


def test_stream_and_tile_kernels_agree_with_the_oracle_smpl(monkeypatch):
    """SMPL: ``k2b_lbs_stream_kernel`` against ``k2b_lbs_tile_kernel<3, 12>`` on a 1100-vertex model of the 24-joint tree."""
    from oracle.smpl_torch import TorchSMPL
    c = _memo("smpl_consts", lambda: synthetic.make_body_model(0, num_vertices=1100))
    B = 161
    p = synthetic.make_poses(B, seed=5)
    t = lambda a: torch.tensor(np.asarray(a))
    with torch.no_grad():
        ref = TorchSMPL(c)(global_orient=t(p.global_orient), body_pose=t(p.body_pose), betas=t(p.betas), transl=t(p.transl))
    for what, m in (("default route", _memo("smpl_model", lambda: _native(c))), ("tile twin", _twin(monkeypatch, ("smpl",), c))):
        j, v = m.lbs(*map(H.cuda, (p.global_orient, p.body_pose, p.betas, p.transl)))
        j2, _ = m.lbs(*map(H.cuda, (p.global_orient, p.body_pose, p.betas, p.transl)), want_vertices=False)
        e = (_err(v, ref.vertices), _err(j, ref.joints), _err(j2, ref.joints))
        print(f"SMPL {what}: vertices {e[0]:.3e} joints {e[1]:.3e} joints alone {e[2]:.3e}")
        assert tuple(v.shape) == (B, 1100, 3) and max(e) < GATE, (what, e)


# ---- 4. determinism -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [20, 26])
def test_wide_forward_is_deterministic_and_frames_do_not_interact(nb):
    """The same call twice: bit-equal.  A frame's result does not depend on its batch: rows 0..36 of a 300-frame call equal the
    same 37 frames skinned alone, bit for bit.  This holds for ``k2b_lbs_stream_x_kernel`` on the 20-coefficient model (nb = 20:
    the kernel is the parent's, unchanged), so it is required of the 17-k-step kernel as well (nb = 26)."""
    m = _model(nb)
    j, v = _lbs(m, nb, 300, 11)
    j_again, v_again = _lbs(m, nb, 300, 11)
    assert torch.equal(j, j_again) and torch.equal(v, v_again)
    first = [H.cuda(x[:37]) for x in _params(nb, 300, 11)]
    j37, v37 = m.lbs(*first)
    assert torch.equal(v[:37], v37) and torch.equal(j[:37], j37)


# ---- 5. the fitter --------------------------------------------------------------------------------------------------------------
def _public():
    def make():
        from keypoints2body_amd.models.body_model import BodyModel
        from keypoints2body_amd.prior import MaxMixturePrior, MixtureBuffers
        g = H.gmm_fixture()
        c = _consts(26)
        model = BodyModel(c.v_template, c.shapedirs, c.posedirs, c.J_regressor, c.lbs_weights, c.parents, c.extra_vertex_ids, num_betas=16)
        assert model.model_type == "smplx" and model.num_betas == 16 and model.num_expression_coeffs == 10
        prior = MaxMixturePrior(MixtureBuffers(g["ref_means"], g["ref_precisions"], g["ref_nll_weights"].reshape(-1)))
        return model, prior, (torch.zeros(1, 66), torch.zeros(1, 16))
    return _memo("public", make)


def _motion(model, T, seed):
    """(T, 127, 3) output joints of the model's own forward along a small random walk of the pose, on the device."""
    rng = np.random.default_rng(seed)
    f = lambda x: H.cuda(x.astype(np.float32))
    go = np.repeat(0.2 * rng.standard_normal((1, 3)), T, 0)
    pose = 0.15 * rng.standard_normal((1, 162)) + np.cumsum(0.02 * rng.standard_normal((T, 162)), axis=0)
    shape = np.repeat(0.3 * rng.standard_normal((1, 26)), T, 0)
    tr = np.repeat(rng.standard_normal((1, 3)), T, 0)
    return model.native.lbs(f(go), f(pose), f(shape), f(tr), want_vertices=False)[0]


@pytest.mark.parametrize("use_lbfgs", [False, True])
def test_wide_model_through_fit_frame(use_lbfgs):
    """``WorldSpaceFitter.fit_frame`` on ``BodyModel(..., num_betas=16)`` with NB = 26, Adam and the default driver (device
    L-BFGS): ``SMPLXData`` out, the parameters those of ``fit_batch(run_forward=False)`` and joints / vertices those of
    ``k2b_lbs`` at them, bit for bit."""
    from keypoints2body_amd.core.fitters.world_space import WorldSpaceFitter
    from keypoints2body_amd.models.smpl_data import SMPLXData
    model, prior, _ = _public()
    j = _motion(model, 1, seed=6)[:, :55].cpu()
    z = lambda c: torch.zeros(1, c)
    with torch.no_grad():
        root0 = model(global_orient=z(3), body_pose=z(63), return_verts=False).joints[:, 0].cpu()
    start = SMPLXData(betas=z(16), global_orient=z(3), body_pose=z(63), transl=j[:, 0] - root0, left_hand_pose=z(45),
                      right_hand_pose=z(45), expression=z(10), jaw_pose=z(3), leye_pose=z(3), reye_pose=z(3))
    idx = torch.arange(55)
    kw = {} if use_lbfgs else {"use_lbfgs": False}                     # (the default: use_lbfgs=True on the device driver)
    fitter = WorldSpaceFitter(model, step_size=1e-2, num_iters_first=12, joints_category="GENERIC", pose_prior=prior, **kw)
    assert fitter.use_lbfgs == use_lbfgs and (not use_lbfgs or fitter.lbfgs_driver == "device")
    res = fitter.fit_frame(start, j, None, seq_ind=0, target_model_indices=idx)
    p = res.params
    assert isinstance(p, SMPLXData) and tuple(p.betas.shape) == (1, 16) and tuple(p.expression.shape) == (1, 10)
    assert tuple(res.vertices.shape) == (1, 1100, 3) and tuple(res.joints.shape) == (1, 127, 3)
    assert torch.isfinite(res.vertices).all() and torch.isfinite(res.joints).all() and torch.isfinite(res.loss)
    out = fitter.fit_batch(start, j, None, seq_ind=0, target_model_indices=idx, run_forward=False)[0]
    want = fitter.result_params(out, start)
    for k in ("global_orient", "body_pose", "transl", "left_hand_pose", "right_hand_pose", "expression", "jaw_pose", "leye_pose",
              "reye_pose", "betas"):
        assert torch.equal(getattr(p, k), getattr(want, k)), k
    assert float(p.body_pose.abs().max()) > 1e-4                      # the fit did something
    joints, verts = model.native.lbs(out["global_orient"], out["body_pose"], out["betas"], out["transl"])
    assert torch.equal(res.joints, joints) and torch.equal(res.vertices, verts)


# ---- 6. the public API in its default configuration -----------------------------------------------------------------------------
def test_wide_model_through_the_public_api_with_its_defaults():
    """``optimize_params_sequence`` with its defaults (shape pre-pass, L-BFGS per frame, warm start) on the NB = 26 model, 22
    AMASS targets from the model's own forward: every frame ``SMPLXData`` and finite; the pre-pass moves the 16 betas and leaves
    the expression at zero; the frames equal the frame-by-frame ``fit_frame`` chain from the same start, bit for bit; the fit
    explains the targets (factor 0.6 of the root-aligned zero pose's error: ``tests/test_gpu_smplx.py``)."""
    import keypoints2body_amd as k2b
    from keypoints2body_amd.api import sequence as S
    from keypoints2body_amd.models.smpl_data import SMPLXData
    model, prior, mean = _public()
    T = 4
    seq = _motion(model, T, seed=2)[:, :22].cpu().numpy()
    res = k2b.optimize_params_sequence(seq, body_model="smplx", joint_layout="AMASS", model=model, pose_prior=prior, mean_params=mean)
    assert len(res) == T and all(isinstance(r.params, SMPLXData) for r in res)
    fields = ("global_orient", "body_pose", "transl", "left_hand_pose", "right_hand_pose", "expression", "jaw_pose", "leye_pose",
              "reye_pose", "betas")
    for r in res:
        assert torch.isfinite(r.loss) and all(torch.isfinite(getattr(r.params, k)).all() for k in fields)
        assert tuple(r.params.betas.shape) == (1, 16) and tuple(r.params.expression.shape) == (1, 10)
        assert tuple(r.vertices.shape) == (1, 1100, 3) and tuple(r.joints.shape) == (1, 127, 3)
        assert torch.isfinite(r.vertices).all() and torch.isfinite(r.joints).all()
    assert float(res[0].params.betas.abs().max()) > 1e-3

    # the same start, then one fit_frame per frame: what the API runs as one chain
    dev = model.device
    seq_cfg = S.sequence_config_from(None)
    xyz, conf, idx = S._preprocess_sequence(seq, "AMASS", "smplx", seq_cfg, dev)
    betas = S.optimize_shape_pass(model=model, seq_config=seq_cfg, init_mean_shape=mean[1].to(dev), init_mean_pose=mean[0].to(dev),
                                  data_tensor=xyz, confidence_input=conf[0], device=dev, pose_prior=prior)
    # the pre-pass moved the 16 betas, every one of them, off the zero mean (by how much is the targets' business: the size test
    # is the one above, on the fitted frame, as for the 20-coefficient model)
    assert tuple(betas.reshape(1, -1).shape) == (1, 16) and torch.isfinite(betas).all() and bool((betas != 0).all())
    base = S.default_init_params(mean[0].to(dev), betas, xyz[0:1], model, joints_category=seq_cfg.frame.joints_category,
                                 coordinate_mode=seq_cfg.frame.coordinate_mode)
    prev = S.upgrade_smpl_family_init_params(base, model_type="smplx", model=model, device=dev)
    assert tuple(prev.expression.shape) == (1, 10) and float(prev.expression.abs().max()) == 0.0   # ... and left the expression at zero
    if prev.transl is None:
        prev = S._with_root_aligned_transl(prev, xyz[0:1], model, seq_cfg.frame, dev)
    engine = S.OptimizeEngine(model=model, frame_config=seq_cfg.frame, device=dev, model_type="smplx", pose_prior=prior)
    for i in range(T):
        want = engine.fit_frame(init_params=prev, j3d=xyz[i:i + 1], conf_3d=conf[i], seq_ind=i, target_model_indices=idx)
        for k in fields:
            assert torch.equal(getattr(res[i].params, k), getattr(want.params, k)), (i, k)
        assert torch.equal(res[i].vertices, want.vertices) and torch.equal(res[i].joints, want.joints), i
        prev = want.params

    with torch.no_grad():                                          # the zero pose, root aligned: where the fit starts
        j0 = model(global_orient=torch.zeros(1, 3), body_pose=torch.zeros(1, 63), return_verts=False).joints[:, :22].cpu()
    tgt = torch.tensor(seq[-1:])
    err0 = (j0 - j0[:, :1] + tgt[:, :1] - tgt).norm(dim=-1).mean()
    err = (res[-1].joints[:, :22].cpu() - tgt).norm(dim=-1).mean()
    print(f"last frame: mean joint error {float(err):.4f} m, root-aligned zero pose {float(err0):.4f} m")
    assert float(err) < 0.6 * float(err0), (float(err0), float(err))

    one = k2b.optimize_params_frame(seq[0], body_model="smplx", joint_layout="AMASS", model=model, pose_prior=prior, mean_params=mean)
    assert isinstance(one.params, SMPLXData) and tuple(one.params.betas.shape) == (1, 16)
    assert tuple(one.vertices.shape) == (1, 1100, 3) and tuple(one.joints.shape) == (1, 127, 3)
    assert torch.isfinite(one.loss) and torch.isfinite(one.joints).all() and torch.isfinite(one.vertices).all()


# ---- 7. several sequences -------------------------------------------------------------------------------------------------------
def test_wide_model_through_the_several_sequences_entry():
    """``optimize_params_sequences`` with two sequences of 3 and 5 frames in the default configuration: each equals
    ``optimize_params_sequence`` on it alone, bit for bit (the route a 20-coefficient SMPL-X model takes under L-BFGS: sequence
    by sequence)."""
    import keypoints2body_amd as k2b
    model, prior, mean = _public()
    seqs = [_motion(model, 3, seed=12)[:, :22].cpu().numpy(), _motion(model, 5, seed=13)[:, :22].cpu().numpy()]
    kw = dict(body_model="smplx", joint_layout="AMASS", model=model, pose_prior=prior, mean_params=mean)
    batch = k2b.optimize_params_sequences(seqs, **kw)
    assert len(batch) == 2 and batch.num_frames == 8 and tuple(batch.joints.shape) == (8, 127, 3)
    assert torch.isfinite(batch.joints).all() and torch.isfinite(batch.loss).all()
    for s, seq in enumerate(seqs):
        alone = k2b.optimize_params_sequence(seq, **kw)
        rows = slice(int(batch.offsets[s]), int(batch.offsets[s]) + int(batch.lengths[s]))
        assert len(alone) == int(batch.lengths[s])
        for k in ("global_orient", "body_pose", "betas", "transl"):
            want = torch.cat([getattr(r.params, k).reshape(1, -1) for r in alone]).to(batch.params[k].device)
            assert torch.equal(batch.params[k][rows], want), (s, k)
        assert torch.equal(batch.joints[rows], torch.cat([r.joints for r in alone]))
        assert torch.equal(batch.loss[rows], torch.stack([r.loss.reshape(()) for r in alone]).to(batch.loss.device))
        got = batch.results(s)
        assert len(got) == len(alone) and all(torch.equal(a.vertices, b.vertices) for a, b in zip(got, alone))
