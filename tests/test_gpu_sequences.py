"""GPU: many sequences of different lengths side by side (``optimize_params_sequences``; ``k2b_fit_sequences`` /
``k2b_fit_sequences_lbfgs``: ragged warm-start chains in ONE launch) and the eval CLI on top of it.

Every sequence must come out exactly as the single-sequence path makes it - ``optimize_params_sequence`` on that sequence
alone, bit for bit - whatever its neighbours, their number or their order."""
import pickle

import numpy as np
import pytest
import torch

import keypoints2body_amd as k2b
from keypoints2body_amd.models.body_model import BodyModel
from keypoints2body_amd.prior import MaxMixturePrior, MixtureBuffers
from tests import helpers as H

pytestmark = pytest.mark.gpu
LENGTHS = (1, 2, 5, 17, 30, 30, 64)
KEYS = ("global_orient", "body_pose", "betas", "transl")


@pytest.fixture(scope="module")
def assets():
    g = H.gmm_fixture()
    prior = MaxMixturePrior(MixtureBuffers(g["ref_means"], g["ref_precisions"], g["ref_nll_weights"].reshape(-1)))
    d = H.load_case("amass_noisy_conf")
    mean = (torch.tensor(np.concatenate([d["init_global_orient"][:1], d["init_body_pose"][:1]], axis=1)),
            torch.tensor(d["init_betas"][:1]))
    return BodyModel.synthetic(0), prior, mean


def make_sequences(lengths, seed=0):
    """AMASS-layout (T, 22, 4) arrays - joints of a synthetic motion plus noise, per-frame confidences in channel 4."""
    from keypoints2body_amd import synthetic
    rng = np.random.default_rng(seed)
    total = int(sum(lengths))
    p = synthetic.make_poses(max(total, 1), seed=seed + 1)
    model = H.oracle_model()
    with torch.no_grad():
        t = lambda a: torch.tensor(np.asarray(a, np.float32))
        j = model(global_orient=t(p.global_orient), body_pose=t(p.body_pose), betas=t(p.betas), transl=t(p.transl)).joints[:, :22]
    j = (j.numpy() + rng.normal(0, 0.01, j.shape)).astype(np.float32)
    # smooth motion inside a sequence: every frame of sequence s is a small step from its first frame
    out, o = [], 0
    for n in lengths:
        base = j[o: o + 1] + np.cumsum(rng.normal(0, 0.004, (n, 22, 3)), axis=0).astype(np.float32) if n else j[:0]
        conf = rng.uniform(0.5, 1.5, (n, 22, 1)).astype(np.float32)
        out.append(np.concatenate([base, conf], axis=2))
        o += n
    return out


def cfg_of(use_lbfgs, freeze, shape_pass=False):
    return {"frame": {"use_lbfgs": use_lbfgs, "freeze_betas": freeze, "num_iters_first": 14, "num_iters_followup": 6},
            "use_shape_optimization": shape_pass, "fix_foot": True}


def assert_same(batch, s, single):
    got = batch.results(s)
    assert len(got) == len(single) == int(batch.lengths[s])
    for i, (g, w) in enumerate(zip(got, single)):
        for k in KEYS:
            assert torch.equal(getattr(g.params, k), getattr(w.params, k)), (s, i, k)
        assert torch.equal(g.joints, w.joints) and torch.equal(g.vertices, w.vertices), (s, i)
        assert torch.equal(g.loss, w.loss), (s, i)
    if single:
        rows = slice(int(batch.offsets[s]), int(batch.offsets[s]) + len(single))
        for k in KEYS:
            assert torch.equal(batch.params[k][rows], torch.cat([getattr(w.params, k) for w in single])), (s, k)
        assert torch.equal(batch.loss[rows], torch.stack([w.loss for w in single])), s
        assert torch.equal(batch.joints[rows], torch.cat([w.joints for w in single])), s
        assert torch.equal(batch.pose(s), torch.cat([torch.cat([w.params.global_orient, w.params.body_pose], 1) for w in single]))


@pytest.mark.parametrize("use_lbfgs", [False, True], ids=["adam", "lbfgs"])
@pytest.mark.parametrize("freeze", [False, True], ids=["free", "frozen"])
def test_ragged_chains_equal_single_sequence_calls(assets, use_lbfgs, freeze):
    model, prior, mean = assets
    seqs = make_sequences(LENGTHS, seed=3)
    kw = dict(model=model, pose_prior=prior, mean_params=mean, config=cfg_of(use_lbfgs, freeze), joint_layout="AMASS")
    batch = k2b.optimize_params_sequences(seqs, **kw)
    assert batch.lengths.tolist() == list(LENGTHS) and batch.num_frames == sum(LENGTHS)
    for s, seq in enumerate(seqs):
        assert_same(batch, s, k2b.optimize_params_sequence(seq, **kw))
    if freeze:
        assert torch.equal(batch.params["betas"], mean[1].cuda().expand(sum(LENGTHS), -1))


@pytest.mark.parametrize("use_lbfgs", [False, True], ids=["adam", "lbfgs"])
def test_result_does_not_depend_on_order_or_neighbours(assets, use_lbfgs):
    """Reversed order, and the seven sequences among 1100 short ones: more than four per CU, so several waves of workgroups
    on both branches (Adam holds up to four sequences per workgroup, L-BFGS two)."""
    model, prior, mean = assets
    seqs = make_sequences(LENGTHS, seed=5)
    kw = dict(model=model, pose_prior=prior, mean_params=mean, config=cfg_of(use_lbfgs, False), joint_layout="AMASS")
    ref = k2b.optimize_params_sequences(seqs, **kw)
    rev = k2b.optimize_params_sequences(seqs[::-1], **kw)
    rng = np.random.default_rng(9)
    others = make_sequences(tuple(int(n) for n in rng.integers(1, 4, 1100)), seed=11)
    pos = sorted(rng.choice(1100 + len(seqs), len(seqs), replace=False).tolist())
    mixed_list, it_o = [], iter(others)
    it_s = iter(seqs)
    for i in range(1100 + len(seqs)):
        mixed_list.append(next(it_s) if i in pos else next(it_o))
    mixed = k2b.optimize_params_sequences(mixed_list, **kw)
    for s in range(len(seqs)):
        a = slice(int(ref.offsets[s]), int(ref.offsets[s]) + LENGTHS[s])
        r = len(seqs) - 1 - s
        b = slice(int(rev.offsets[r]), int(rev.offsets[r]) + LENGTHS[s])
        c = slice(int(mixed.offsets[pos[s]]), int(mixed.offsets[pos[s]]) + LENGTHS[s])
        for k in KEYS:
            assert torch.equal(ref.params[k][a], rev.params[k][b]), (s, k)
            assert torch.equal(ref.params[k][a], mixed.params[k][c]), (s, k)
        assert torch.equal(ref.loss[a], rev.loss[b]) and torch.equal(ref.loss[a], mixed.loss[c]), s


@pytest.mark.parametrize("S", [5, 300, 1100])
def test_smplx_ragged_chain_on_the_tree_kernel_equals_single_sequence_launches(S):
    """k2b_fit_sequences on the 55-joint tree kernel: every sequence equals k2b_fit_sequence on it alone, bit for bit.  S = 300
    puts two waves of different lengths in a workgroup (component-wave shape), S = 1100 five (plain shape)."""
    from keypoints2body_amd import native, synthetic
    from tests.test_gpu_smplx import POSE_FIELDS
    m, pr = H.native_model_x(), H.native_prior()
    rng = np.random.default_rng(S)
    lengths = (1, 3, 7, 2, 7) if S == 5 else tuple(int(n) for n in rng.integers(1, 6, S))
    N = sum(lengths)
    p = synthetic.make_poses_x(N, seed=4)
    pose = np.concatenate([getattr(p, k) for k, _ in POSE_FIELDS], axis=1)
    shape = np.concatenate([p.betas, p.expression], axis=1)
    j, _ = m.lbs(H.cuda(p.global_orient), H.cuda(pose), H.cuda(shape), H.cuda(p.transl), want_vertices=False)
    j3d = j[:, :55].contiguous()
    conf = H.cuda(rng.uniform(0.5, 1.5, (N, 55)).astype(np.float32))
    off = np.concatenate(([0], np.cumsum(lengths[:-1]))).astype(int)
    z = lambda c: torch.zeros(S, c, device="cuda")
    go, bp, be = z(3), z(162), 0.1 * torch.ones(S, 20, device="cuda")
    tr = j3d[torch.as_tensor(off, device="cuda"), 0].contiguous()
    cfg = native.default_fit_config()
    cfg.num_iters, cfg.pose_preserve_weight, cfg.conf_per_frame = 9, 5.0, 1
    cfg.prior_pose_dims, cfg.num_betas_prior = 63, 10
    got = native.fit_sequences(m, pr, cfg, 4, list(range(55)), lengths, j3d, conf, go, bp, be, tr)
    for s, (o, n) in enumerate(zip(off, lengths)):
        one = native.fit_sequence(m, pr, cfg, 4, list(range(55)), j3d[o:o + n][None].contiguous(), conf[o:o + n][None].contiguous(),
                                  go[s:s + 1], bp[s:s + 1], be[s:s + 1], tr[s:s + 1])
        for k in one:
            assert torch.equal(got[k][o:o + n], one[k][0]), (s, k)


def test_default_config_with_the_shape_pass(assets):
    """L-BFGS + the shape pre-pass (the reference's default): every sequence equals the single call started from the betas of
    the batched pass (``optimize_params_sequence(seq, init_params=<default start from those betas>, shape pass off)``), bit for
    bit; frame 0 fits its targets within the bound of test_gpu_api.py::test_shape_pre_pass_and_default_config_sequence."""
    from keypoints2body_amd.core.config import SequenceOptimizeConfig
    from keypoints2body_amd.core.engine import default_init_params, optimize_shape_pass_batched
    model, prior, mean = assets
    d = dict(np.load(H.GOLDEN / "shape_pass.npz"))
    seqs = [d["j3d"][:4], d["j3d"][:2], d["j3d"][1:6]]
    mean = (torch.tensor(d["mean_pose"]).cuda(), torch.tensor(d["init_betas"]).cuda())
    kw = dict(model=model, pose_prior=prior, mean_params=mean)
    batch = k2b.optimize_params_sequences(seqs, **kw)
    cfg = SequenceOptimizeConfig()
    cfg.frame.joints_category = "AMASS"
    xs = [torch.tensor(q).cuda() for q in seqs]
    conf = [torch.ones(22, device="cuda") for _ in seqs]
    betas = optimize_shape_pass_batched(model, cfg, mean[1], mean[0], xs, conf, "cuda", pose_prior=prior)
    for s, seq in enumerate(seqs):
        start = default_init_params(mean[0], betas[s:s + 1], xs[s][0:1], model, joints_category="AMASS", coordinate_mode="world")
        single = k2b.optimize_params_sequence(seq, init_params=start, config={"use_shape_optimization": False}, **kw)
        assert_same(batch, s, single)
        err_cm = float((single[0].joints[:, :22].cpu() - torch.tensor(seq[:1])).norm(dim=-1).mean()) * 100
        assert err_cm < 5.0


def _shape_inputs():
    from keypoints2body_amd.core.config import SequenceOptimizeConfig
    d = dict(np.load(H.GOLDEN / "shape_pass.npz"))
    cfg = SequenceOptimizeConfig(num_shape_frames=int(d["num_shape_frames"]), num_shape_iters=int(d["num_shape_iters"]))
    cfg.frame.joints_category = "AMASS"
    return d, cfg


def test_batched_shape_pass_matches_golden_and_the_single_pass(assets):
    """Against the reference-produced golden (1e-4) and against ``optimize_shape_pass`` on the same sequence (1e-5)."""
    from keypoints2body_amd.core.engine import optimize_shape_pass, optimize_shape_pass_batched
    model, prior, _ = assets
    d, cfg = _shape_inputs()
    got = optimize_shape_pass_batched(model, cfg, torch.tensor(d["init_betas"]), torch.tensor(d["mean_pose"]),
                                      [torch.tensor(d["j3d"])], [torch.tensor(d["conf"])], "cuda", pose_prior=prior)
    assert tuple(got.shape) == (1, 10)
    assert np.abs(got.cpu().numpy() - d["out_betas"]).max() < 1e-4
    one = optimize_shape_pass(model, cfg, torch.tensor(d["init_betas"]), torch.tensor(d["mean_pose"]), torch.tensor(d["j3d"]),
                              torch.tensor(d["conf"]), model.device, pose_prior=prior)
    assert float((got - one.reshape(1, -1)).abs().max()) < 1e-5


def test_batched_shape_pass_result_does_not_depend_on_the_batch(assets):
    """A sequence alone and inside a batch of 50 (other lengths, other confidences, other motion): the same bits."""
    from keypoints2body_amd.core.engine import optimize_shape_pass_batched
    model, prior, _ = assets
    d, cfg = _shape_inputs()
    rng = np.random.default_rng(17)
    xs = [torch.tensor(d["j3d"][: int(rng.integers(1, 7))] + rng.normal(0, 0.02, (1, 22, 3)).astype(np.float32)) for _ in range(50)]
    cs = [torch.tensor(rng.uniform(0.5, 1.5, 22).astype(np.float32)) for _ in range(50)]
    xs[23], cs[23] = torch.tensor(d["j3d"]), torch.tensor(d["conf"])
    args = (torch.tensor(d["init_betas"]), torch.tensor(d["mean_pose"]))
    many = optimize_shape_pass_batched(model, cfg, *args, xs, cs, "cuda", pose_prior=prior)
    alone = optimize_shape_pass_batched(model, cfg, *args, [xs[23]], [cs[23]], "cuda", pose_prior=prior)
    assert torch.equal(many[23:24], alone)
    for s in (0, 7, 49):
        assert torch.equal(many[s:s + 1], optimize_shape_pass_batched(model, cfg, *args, [xs[s]], [cs[s]], "cuda", pose_prior=prior))


def test_empty_sequence_and_errors(assets):
    model, prior, mean = assets
    seqs = make_sequences((3, 0, 2), seed=2)
    kw = dict(model=model, pose_prior=prior, mean_params=mean, joint_layout="AMASS")
    batch = k2b.optimize_params_sequences(seqs, config=cfg_of(True, False), **kw)
    assert batch.lengths.tolist() == [3, 0, 2] and batch.results(1) == [] and tuple(batch.pose(1).shape)[0] == 0
    assert_same(batch, 2, k2b.optimize_params_sequence(seqs[2], config=cfg_of(True, False), **kw))
    with pytest.raises(ValueError):
        k2b.optimize_params_sequences([], **kw)
    with pytest.raises(ValueError):
        k2b.optimize_params_sequences(seqs, init_params=[k2b.MANOData(betas=torch.zeros(1, 10), global_orient=torch.zeros(1, 3),
                                                                      body_pose=torch.zeros(1, 0))] * 3, **kw)
    with pytest.raises(NotImplementedError):
        k2b.optimize_params_sequences(seqs, body_model="mano", **kw)
    with pytest.raises(NotImplementedError):
        k2b.optimize_params_sequences(seqs, config={"frame": {"input_type": "joints2d"}}, **kw)
    with pytest.raises(RuntimeError):
        k2b.optimize_params_sequences(seqs, config={"frame": {"use_lbfgs": False}, "use_shape_optimization": True}, **kw)


def test_ragged_abi_checks(assets):
    from keypoints2body_amd import native
    m, pr = H.native_model(), H.native_prior()
    cfg = native.default_fit_config()
    z = lambda *s: torch.zeros(*s, device="cuda")
    args = (list(range(22)), [2, 1], z(3, 22, 3), None, z(2, 3), z(2, 69), z(2, 10), z(2, 3))
    with pytest.raises(ValueError):
        native.fit_sequences(m, pr, cfg, 4, *args, offsets=[0, 1])
    cfg.transl_prior_weight = 1.0
    with pytest.raises(ValueError):
        native.fit_sequences(m, pr, cfg, 4, *args)
    with pytest.raises(ValueError):
        native.fit_sequences_lbfgs(m, pr, cfg, 5, 3, *args, lr=1.0)


def write_eval_assets(tmp_path):
    """A synthetic smpl_neutral.npz, gmm_08.pkl, mean parameters and six AMASS-style sequences (one broken)."""
    from keypoints2body_amd import synthetic
    c = H.body_consts(0)
    np.savez(tmp_path / "smpl_neutral.npz", v_template=c.v_template, shapedirs=c.shapedirs, posedirs=c.posedirs,
             J_regressor=c.J_regressor, lbs_weights=c.lbs_weights, parents=c.parents, extra_vertex_ids=c.extra_vertex_ids)
    g = synthetic.make_gmm(0)
    with open(tmp_path / "gmm_08.pkl", "wb") as f:
        pickle.dump({"means": np.asarray(g.means), "covars": np.asarray(g.covars), "weights": np.asarray(g.weights)}, f, protocol=2)
    d = H.load_case("amass_noisy_conf")
    np.savez(tmp_path / "mean.npz", pose=np.concatenate([d["init_global_orient"][0], d["init_body_pose"][0]]),
             shape=d["init_betas"][0])
    root = tmp_path / "amass"
    (root / "sub").mkdir(parents=True)
    poses = synthetic.make_poses(40, seed=21)
    model = H.oracle_model()
    o = 0
    for i, n in enumerate((6, 3, 8, 5, 4)):
        sl = slice(o, o + n)
        o += n
        t = lambda a: torch.tensor(np.asarray(a[sl], np.float32))
        with torch.no_grad():
            j = model(global_orient=t(poses.global_orient), body_pose=t(poses.body_pose), betas=t(poses.betas),
                      transl=t(poses.transl)).joints[:, :24].numpy()
        np.savez((root / "sub" if i % 2 else root) / f"seq{i}.npz", joints=j, global_orient=poses.global_orient[sl],
                 body_pose=poses.body_pose[sl])
    np.savez(root / "broken.npz", joints=np.zeros((3, 24, 3), np.float32))          # no poses: fails to load
    return root


def _per_sequence_mpjae(tmp_path, root, args):
    """The dataset MPJAE from one ``optimize_params_sequence`` call per sequence (the reference's loop), and the count."""
    from keypoints2body_amd import evaluation
    from keypoints2body_amd.cli.eval import parse_args, sequence_config
    from keypoints2body_amd.core.engine import load_mean_pose_shape
    model = BodyModel.from_npz(str(tmp_path / "smpl_neutral.npz"))
    prior = MaxMixturePrior(prior_folder=str(tmp_path), num_gaussians=8)
    mean = load_mean_pose_shape(str(tmp_path / "mean.npz"), "cuda")
    cfg = sequence_config(parse_args(args))
    total, count, ok, shapes = 0.0, 0, 0, {}
    for path in evaluation.discover_amass_npz_files(root):
        try:
            joints, gt = evaluation.load_amass_sequence(path)
        except KeyError:
            continue
        res = k2b.optimize_params_sequence(joints, body_model="smpl", joint_layout="AMASS", model=model, config=cfg,
                                           pose_prior=prior, mean_params=mean)
        pred = torch.cat([torch.cat([r.params.global_orient, r.params.body_pose], 1) for r in res]).cpu().numpy()
        _, s, c = evaluation.evaluate_pose_pair(pred, gt)
        total, count, ok = total + s, count + c, ok + 1
        shapes[path] = (joints.shape[0], 72)
    return total / count, ok, shapes


def test_eval_cli_end_to_end(tmp_path, capsys, caplog):
    """The CLI against the reference's loop of per-sequence calls.  With ``--fix-shape`` (no shape pre-pass) the dataset MPJAE is
    the same number; in the default configuration the batched shape pass agrees with the per-sequence pass within 1e-5 (not bit
    for bit), which the warm-start chains amplify, so the two numbers agree within 0.05 deg."""
    import logging
    from keypoints2body_amd.cli.eval import main
    root = write_eval_assets(tmp_path)
    common = ["--amass-root", str(root), "--model-dir", str(tmp_path), "--prior-dir", str(tmp_path),
              "--mean-file", str(tmp_path / "mean.npz"), "--num-body-iters-first", "12", "--num-body-iters", "5",
              "--num-shape-iters", "8", "--num-shape-frames", "4", "--batch-sequences", "3"]
    with caplog.at_level(logging.INFO, logger="keypoints2body_amd.cli.eval"):
        value = main(common + ["--save-pred-dir", str(tmp_path / "pred")])
    out = capsys.readouterr().out
    assert "Dataset MPJAE(global_orient + body_pose):" in out and f"{value:.6f} deg" in out
    assert "success=5 failed=1" in caplog.text and "broken.npz" in caplog.text
    want, ok, shapes = _per_sequence_mpjae(tmp_path, root, common)
    assert ok == 5 and abs(value - want) < 0.05, (value, want)
    for path, shape in shapes.items():
        assert np.load(tmp_path / "pred" / path.relative_to(root))["pose"].shape == shape
    fixed = common + ["--fix-shape"]
    value_fixed = main(fixed)
    assert value_fixed == _per_sequence_mpjae(tmp_path, root, fixed)[0]
    with pytest.raises(KeyError):
        main(common + ["--fail-fast"])
