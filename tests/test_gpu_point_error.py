"""GPU: ``k2b_point_error`` (MPJPE / PA-MPJPE / PVE) against the float64 oracle of tests/point_error_common.py, its invariances,
its bit-reproducibility, its corner cases, the ``evaluation`` functions on top of it and the eval CLI's ``--position-metrics``.

Tolerances are derived, not tuned.  The kernel works in float64 on inputs that convert exactly and rounds once to float32 on store:
half an ulp, 2^-24 relative, taken with a factor 4 of slack as 2^-22; the float64 work adds about 1e-15 L times the conditioning
that tests/test_point_error_host.py bounds, covered by 1e-9 L.  Transforms: R to 2^-21, s to 2^-22 relative, t to
2^-21 max(L, |t|).  Where the covariance has rank one (two weighted points, or collinear ones) the error, the distances and the
scale are determined but the rotation is not - any turn about the line serves - so there R is held to being a proper rotation and
the transform to reproducing the kernel's distances (those of points without weight are not determined either), within the
float32 rounding of its 13 numbers (2^-20 max(L, |t|) max(1, s)).  No frame of four or more points that all carry weight is
treated so (asserted).
"""
import functools
import pickle

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import point_error_common as P

pytestmark = pytest.mark.gpu

REL, ABS_L = 2.0 ** -22, 1e-9
CASES = {name: (pred, gt, w) for name, pred, gt, w in P.parity_cases()}
assert len(CASES) == len(P.parity_cases())


@functools.lru_cache(maxsize=None)
def _oracle(name, mode):
    return P.oracle(*CASES[name], mode)


def _dev(a):
    return None if a is None else torch.as_tensor(a, device="cuda").contiguous()


def run(pred, gt, w=None, mode=0):
    """The kernel's ``(err [B], per_point [B][N], transform [B][13])`` as float64 numpy arrays."""
    from keypoints2body_amd import native
    err, pp, tf = native.point_error(_dev(pred), _dev(gt), weights=_dev(w), align=P.MODES[mode], per_point=True, transform=True)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy().astype(np.float64) for t in (err, pp, tf))


def check_against_oracle(pred, gt, w, mode, want, label=""):
    err, pp, tf = run(pred, gt, w, mode)
    L = P.frame_scale(pred, gt)
    d_err = np.abs(err - want["err"])
    d_pp = np.abs(pp - want["per_point"])
    print(f"{label} mode {mode}: err max|diff| / L {np.max(d_err / L):.3e}, distances {np.max(d_pp / L[:, None]):.3e}")
    assert np.all(d_err <= REL * np.abs(want["err"]) + ABS_L * L), (label, mode, d_err.max())
    loose = np.nan_to_num(want["gap"], nan=1.0) < 1e-8                # rank one: the rotation is any turn about a line,
    held = ~loose[:, None] | (P._frame_weights(w, *pp.shape) > 0)     # so a point WITHOUT weight may land anywhere on a circle
    if pp.shape[1] >= 4 and (w is None or w.ndim == 1):               # the relaxation is for two live points only: four or more
        assert not loose.any(), (label, mode, want["gap"])            # points that all carry weight never take it
    assert np.all((d_pp <= REL * np.abs(want["per_point"]) + ABS_L * L[:, None])[held]), (label, mode, d_pp[held].max())
    wt = want["transform"]
    s, R, t = tf[:, 0], tf[:, 1:10], tf[:, 10:]
    assert np.all(np.abs(s - wt[:, 0]) <= REL * np.abs(wt[:, 0])), (label, mode, s, wt[:, 0])
    tnorm = np.maximum(L, np.linalg.norm(wt[:, 10:], axis=1))
    ok = ~loose
    assert np.all(np.abs(R - wt[:, 1:10])[ok] <= 2.0 ** -21), (label, mode, np.abs(R - wt[:, 1:10])[ok].max())
    assert np.all(np.abs(t - wt[:, 10:])[ok] <= 2.0 ** -21 * tnorm[ok, None]), (label, mode)
    for b in np.nonzero(loose)[0]:
        Rb = R[b].reshape(3, 3)
        assert np.all(np.abs(Rb @ Rb.T - np.eye(3)) <= 2.0 ** -21) and abs(np.linalg.det(Rb) - 1.0) <= 2.0 ** -21, (label, mode, b)
        res = s[b] * pred[b].astype(np.float64) @ Rb.T + t[b] - gt[b].astype(np.float64)
        bound = 2.0 ** -20 * max(L[b], np.linalg.norm(t[b])) * max(1.0, s[b])
        assert np.all(np.abs(np.sqrt((res * res).sum(1)) - pp[b]) <= bound), (label, mode, b)      # the kernel's own distances


@pytest.mark.parametrize("name", list(CASES))
def test_parity_with_the_oracle(name):
    pred, gt, w = CASES[name]
    for mode in range(4):
        check_against_oracle(pred, gt, w, mode, _oracle(name, mode), name)


def test_known_transform_is_recovered():
    for scale in (True, False):
        pred, gt, s, R, t = P.known_transform_case(scale=scale)
        L = P.frame_scale(pred, gt)
        err3, _, tf3 = run(pred, gt, None, 3)
        assert np.all(err3 <= 1e-6 * L), err3
        assert np.all(np.abs(tf3[:, 0] - s) <= 1e-6) and np.all(np.abs(tf3[:, 1:10].reshape(-1, 3, 3) - R) <= 1e-6)
        if not scale:
            err2, _, _ = run(pred, gt, None, 2)
            assert np.all(err2 <= 1e-6 * L), err2
        else:                                                        # a rigid fit cannot absorb the scale
            assert np.all(run(pred, gt, None, 2)[0] > 1e-3)


def test_mirrored_copy_is_not_aligned_by_a_reflection():
    pred, gt = P.mirrored_case()
    for mode in (2, 3):
        want = P.oracle(pred, gt, None, mode)
        assert np.all(want["err"] > 0.05)
        check_against_oracle(pred, gt, None, mode, want, "mirrored")
        R = run(pred, gt, None, mode)[2][:, 1:10].reshape(-1, 3, 3)
        assert np.all(np.abs(np.linalg.det(R) - 1.0) <= 2.0 ** -21)


def test_invariances():
    """A common rigid motion of both sets leaves the rigid and similarity errors where they were, and so does scaling ``pred`` for
    the similarity.  The motions are exact in float32 - coordinates on a 2^-12 grid, a quarter turn about an axis with the axes
    swapped, a shift on the grid, a factor of four - so the moved inputs ARE the inputs moved, and the parity tolerance applies
    between the two results as it stands."""
    pred, gt, w = CASES["N63-B3-frame"]
    grid = lambda a: (np.round(a.astype(np.float64) * 4096.0) / 4096.0).astype(np.float32)
    pred, gt = grid(pred), grid(gt)
    Q = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, 1.0], [-1.0, 0.0, 0.0]], np.float32)      # a signed permutation, det +1
    assert np.linalg.det(Q) == 1.0
    shift = np.array([0.75, -1.5, 0.3125], np.float32)
    move = lambda a: a @ Q.T + shift
    pm, gm = move(pred), move(gt)
    assert np.array_equal(pm.astype(np.float64), pred.astype(np.float64) @ Q.astype(np.float64).T + shift)   # exact
    L = np.maximum(P.frame_scale(pred, gt), P.frame_scale(pm, gm))
    for mode in (2, 3):
        base, moved = run(pred, gt, w, mode), run(pm, gm, w, mode)
        check_against_oracle(pm, gm, w, mode, P.oracle(pm, gm, w, mode), "moved")
        assert np.all(np.abs(base[0] - moved[0]) <= REL * base[0] + ABS_L * L), (mode, np.abs(base[0] - moved[0]).max())
        assert np.all(np.abs(base[1] - moved[1]) <= REL * base[1] + ABS_L * L[:, None])
    base, scaled = run(pred, gt, w, 3), run(pred * np.float32(4.0), gt, w, 3)
    L = np.maximum(L, 4.0 * P.frame_scale(pred, pred))
    assert np.all(np.abs(base[0] - scaled[0]) <= REL * base[0] + ABS_L * L)
    assert np.all(np.abs(base[1] - scaled[1]) <= REL * base[1] + ABS_L * L[:, None])
    assert np.all(np.abs(base[2][:, 0] - 4.0 * scaled[2][:, 0]) <= REL * base[2][:, 0])


def test_root_alignment_is_mode_none_on_root_subtracted_inputs_bit_for_bit():
    from keypoints2body_amd import evaluation, native
    pred, gt, w = CASES["frames-N22-B5-frame"]
    p, g, wd = _dev(pred), _dev(gt), _dev(w)
    for root in (0, 7):
        a = evaluation.compute_position_error(p, g, align="root", root=root, weights=wd)
        b = native.point_error((p - p[:, root:root + 1]).contiguous(), (g - g[:, root:root + 1]).contiguous(), weights=wd, align="none")
        assert torch.equal(a, b)
        x, y = pred.astype(np.float32) - pred[:, root:root + 1], gt - gt[:, root:root + 1]          # float32, as torch subtracts
        want = P.oracle(x, y, w, 0)["err"]
        assert np.all(np.abs(a.cpu().numpy() - want) <= REL * want + ABS_L * P.frame_scale(x, y))


@pytest.mark.parametrize("N", [22, 1000])
def test_a_frames_outputs_do_not_depend_on_the_batch_or_its_position(N):
    from keypoints2body_amd import native
    B = 257
    pred, gt, w = P.make_case(31, B, N, "frame")
    one_p, one_g, one_w = P.make_case(32, 1, N, "frame")
    for mode in range(4):
        alone = native.point_error(_dev(one_p), _dev(one_g), weights=_dev(one_w), align=P.MODES[mode], per_point=True, transform=True)
        for pos in (0, 128, B - 1):
            p, g, ww = pred.copy(), gt.copy(), w.copy()
            p[pos], g[pos], ww[pos] = one_p[0], one_g[0], one_w[0]
            args = (_dev(p), _dev(g))
            kw = dict(weights=_dev(ww), align=P.MODES[mode], per_point=True, transform=True)
            first, again = native.point_error(*args, **kw), native.point_error(*args, **kw)
            for x, y, z in zip(first, again, alone):
                assert torch.equal(x, y)                             # two runs of the same call
                assert torch.equal(x[pos], z[0]), (mode, pos)        # the frame alone, B = 1


def test_corner_cases():
    from keypoints2body_amd import native
    rng = np.random.default_rng(41)
    # all pred points equal (and N == 1): R = I, s = 1, t = ybar - xbar
    for N, w in ((1, None), (9, None), (9, rng.uniform(0.3, 2.0, 9).astype(np.float32))):
        gt = rng.uniform(-1, 1, (3, N, 3)).astype(np.float32)
        pred = np.repeat(rng.uniform(-1, 1, (3, 1, 3)).astype(np.float32), N, axis=1)
        for mode in range(4):
            want = P.oracle(pred, gt, w, mode)
            check_against_oracle(pred, gt, w, mode, want, f"equal-N{N}")
            if mode >= 2:
                tf = run(pred, gt, w, mode)[2]
                assert np.array_equal(tf[:, :10], np.tile(np.concatenate([[1.0], np.eye(3).ravel()]), (3, 1)))
    # a frame without weight among others: error 0, distances 0, identity transform
    pred, gt, w = P.make_case(42, 5, 22, "frame")
    w[2] = 0.0
    for mode in range(4):
        err, pp, tf = run(pred, gt, w, mode)
        assert err[2] == 0.0 and np.all(pp[2] == 0.0)
        assert np.array_equal(tf[2], np.concatenate([[1.0], np.eye(3).ravel(), np.zeros(3)]))
        check_against_oracle(pred, gt, w, mode, P.oracle(pred, gt, w, mode), "zero-weight-frame")
    # one frame with a NaN among finite frames, in both regimes: that frame's error is not finite, every other frame is untouched
    for N in (22, 300):
        pred, gt, w = P.make_case(43, 6, N, "shared")
        clean = [run(pred, gt, w, mode) for mode in range(4)]
        bad = pred.copy()
        bad[3, N // 2, 1] = np.nan
        for mode in range(4):
            err, pp, tf = run(bad, gt, w, mode)
            assert not np.isfinite(err[3])
            if mode >= 1:
                assert not np.any(np.isfinite(pp[3])) and not np.any(np.isfinite(tf[3, 10:]))
            keep = [0, 1, 2, 4, 5]
            for got, ref in zip((err, pp, tf), clean[mode]):
                assert np.array_equal(got[keep], ref[keep])
    # no frames at all
    empty = torch.zeros((0, 22, 3), device="cuda")
    err, pp, tf = native.point_error(empty, empty, align="similarity", per_point=True, transform=True)
    assert err.shape == (0,) and pp.shape == (0, 22) and tf.shape == (0, 13)
    with pytest.raises(ValueError, match="equal shape"):
        native.point_error(torch.zeros((2, 22, 3), device="cuda"), torch.zeros((2, 21, 3), device="cuda"))
    with pytest.raises(ValueError, match="weights has shape"):
        native.point_error(torch.zeros((2, 22, 3), device="cuda"), torch.zeros((2, 22, 3), device="cuda"),
                           weights=torch.ones(21, device="cuda"))


def test_evaluation_functions():
    from keypoints2body_amd import evaluation
    pred, gt, w = P.make_case(51, 40, 22, "frame")
    w[7] = 0.0                                                        # left out of the mean
    L = P.frame_scale(pred, gt).max()
    names = {"none": 0, "translation": 1, "rigid": 2, "procrustes": 3}
    for align, mode in names.items():
        for weights in (None, w):
            want = P.oracle(pred, gt, weights, mode)["err"]
            live = np.ones(40, bool) if weights is None else weights.sum(1) > 0
            mean, total, count = evaluation.evaluate_position_pair(pred, gt, align=align, weights=weights)
            assert count == int(live.sum()) and abs(total - mean * count) <= 1e-12 * abs(total)
            assert abs(mean - want[live].mean()) <= REL * want[live].mean() + ABS_L * L, (align, mean, want[live].mean())
            per_frame = evaluation.compute_position_error(pred.reshape(8, 5, 22, 3), gt.reshape(8, 5, 22, 3), align=align,
                                                          weights=None if weights is None else weights.reshape(8, 5, 22))
            assert per_frame.shape == (8, 5) and per_frame.is_cuda
            assert np.all(np.abs(per_frame.cpu().numpy().reshape(-1) - want) <= REL * want + ABS_L * L)
    # fewer frames / points on one side: the common ones
    mean, _, count = evaluation.evaluate_position_pair(pred[:30, :20], gt, align="procrustes")
    assert count == 30 and abs(mean - P.oracle(pred[:30, :20], gt[:30, :20], None, 3)["err"].mean()) <= REL * mean + ABS_L * L
    for scale, mode in ((True, 3), (False, 2)):
        aligned, s, R, t = evaluation.procrustes_align(_dev(pred), _dev(gt), scale=scale, weights=_dev(w[:, :]) if scale else None)
        want = P.oracle(pred, gt, w if scale else None, mode)["transform"]
        ref = want[:, :1, None] * np.einsum("bij,bnj->bni", want[:, 1:10].reshape(-1, 3, 3), pred.astype(np.float64)) + want[:, None, 10:]
        live = np.ones(40, bool) if not scale else w.sum(1) > 0
        assert aligned.shape == (40, 22, 3) and s.shape == (40,) and R.shape == (40, 3, 3) and t.shape == (40, 3)
        assert np.all(np.abs(aligned.cpu().numpy().astype(np.float64) - ref)[live] <= 2.0 ** -20 * L)
    with pytest.raises(ValueError, match="align must be one of"):
        evaluation.compute_position_error(pred, gt, align="affine")


def _write_dataset(tmp_path):
    """A synthetic smpl_neutral.npz, gmm_08.pkl, mean parameters and two short AMASS-style sequences."""
    from keypoints2body_amd import synthetic
    c = H.body_consts(0)
    np.savez(tmp_path / "smpl_neutral.npz", v_template=c.v_template, shapedirs=c.shapedirs, posedirs=c.posedirs,
             J_regressor=c.J_regressor, lbs_weights=c.lbs_weights, parents=c.parents, extra_vertex_ids=c.extra_vertex_ids)
    g = synthetic.make_gmm(0)
    with open(tmp_path / "gmm_08.pkl", "wb") as f:
        pickle.dump({"means": np.asarray(g.means), "covars": np.asarray(g.covars), "weights": np.asarray(g.weights)}, f, protocol=2)
    d = H.load_case("amass_noisy_conf")
    np.savez(tmp_path / "mean.npz", pose=np.concatenate([d["init_global_orient"][0], d["init_body_pose"][0]]), shape=d["init_betas"][0])
    root = tmp_path / "amass"
    root.mkdir()
    poses = synthetic.make_poses(9, seed=23)
    model = H.oracle_model()
    for i, sl in enumerate((slice(0, 5), slice(5, 9))):
        t = lambda a: torch.tensor(np.asarray(a[sl], np.float32))
        with torch.no_grad():
            j = model(global_orient=t(poses.global_orient), body_pose=t(poses.body_pose), betas=t(poses.betas),
                      transl=t(poses.transl)).joints[:, :24].numpy()
        np.savez(root / f"seq{i}.npz", joints=j, global_orient=poses.global_orient[sl], body_pose=poses.body_pose[sl])
    return root


def test_eval_cli_position_metrics(tmp_path, capsys):
    from keypoints2body_amd import evaluation
    from keypoints2body_amd.api.sequence import optimize_params_sequences
    from keypoints2body_amd.cli.eval import main, parse_args, sequence_config
    from keypoints2body_amd.core.engine import load_mean_pose_shape
    from keypoints2body_amd.models.body_model import BodyModel
    from keypoints2body_amd.prior import MaxMixturePrior
    root = _write_dataset(tmp_path)
    args = ["--amass-root", str(root), "--model-dir", str(tmp_path), "--prior-dir", str(tmp_path), "--mean-file",
            str(tmp_path / "mean.npz"), "--num-body-iters-first", "12", "--num-body-iters", "5", "--fix-shape",
            "--skip-start-frames", "1", "--log-level", "WARNING"]
    capsys.readouterr()
    plain = main(args)
    out = capsys.readouterr().out.splitlines()
    mpjae_line = f"Dataset MPJAE(global_orient + body_pose): {plain:.6f} deg"
    assert out == [mpjae_line]
    value = main(args + ["--position-metrics"])
    out = capsys.readouterr().out.splitlines()
    assert value == plain and len(out) == 3 and out[2] == mpjae_line
    # the same fit through the API, scored with evaluate_position_pair over the frames after the skipped one
    model = BodyModel.from_npz(str(tmp_path / "smpl_neutral.npz"))
    prior = MaxMixturePrior(prior_folder=str(tmp_path), num_gaussians=8)
    mean = load_mean_pose_shape(str(tmp_path / "mean.npz"), "cuda")
    seqs = [evaluation.load_amass_sequence(p)[0] for p in evaluation.discover_amass_npz_files(root)]
    batch = optimize_params_sequences(seqs, body_model="smpl", joint_layout="AMASS", model=model, config=sequence_config(parse_args(args)),
                                      pose_prior=prior, mean_params=mean)
    want = {}
    for align in ("none", "procrustes"):
        parts = [evaluation.evaluate_position_pair(batch.joints_of(i)[1:, :22], seqs[i][1:], align=align) for i in range(2)]
        total, count = sum(p[1] for p in parts), sum(p[2] for p in parts)
        assert count == 3 + 4
        want[align] = 1000.0 * total / count
    assert out[0] == f"Dataset MPJPE(fit residual, 22 joints): {want['none']:.6f} mm"
    assert out[1] == f"Dataset PA-MPJPE(fit residual, 22 joints): {want['procrustes']:.6f} mm"
    assert want["procrustes"] > 0.0 and want["none"] > 0.0
