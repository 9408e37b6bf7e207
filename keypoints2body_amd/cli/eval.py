"""AMASS evaluation CLI (reference ``keypoints2body/cli/eval.py:160-288``) on the HIP engine.

    python -m keypoints2body_amd.cli.eval --amass-root DIR [--batch-sequences N] [...]

Fits every ``*.npz`` sequence under ``--amass-root`` in world mode with the AMASS joint layout and reports the dataset MPJAE
over ``global_orient + body_pose``, with the reference's flags, per-sequence failure accounting and final line.  With
``--position-metrics`` it also reports MPJPE and PA-MPJPE of the fitted joints against the input joints.  Where the
reference fits one sequence per call, this front end hands ``--batch-sequences`` sequences at a time to
``optimize_params_sequences`` (one launch for all their chains in the default warm-start world mode); the results equal the
per-sequence calls bit for bit.  Loading, the MPJAE kernel and saving are ``keypoints2body_amd.evaluation``.  There is no
``--cpu``: the engine has no CPU path.  Progress goes to ``logging`` (no progress bar).
"""
from __future__ import annotations

import argparse
import logging
from pathlib import Path
from typing import Optional, Sequence

import numpy as np

logger = logging.getLogger(__name__)


def configure_logging(level: str) -> None:
    logging.basicConfig(level=getattr(logging, level.upper()), format="%(asctime)s | %(levelname)s | %(message)s")


def _positive(text: str) -> int:
    v = int(text)
    if v < 1:
        raise argparse.ArgumentTypeError(f"must be >= 1, got {v}")
    return v


def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    p = argparse.ArgumentParser(
        description="Evaluate keypoints2body_amd on AMASS by fitting each sequence and computing MPJAE.")
    p.add_argument("--amass-root", type=Path, required=True)
    p.add_argument("--limit-seqs", type=int, default=-1)
    p.add_argument("--limit-frames", type=int, default=-1)
    p.add_argument("--skip-start-frames", type=int, default=0)
    p.add_argument("--num-shape-iters", type=int, default=40)
    p.add_argument("--num-shape-frames", type=int, default=50)
    p.add_argument("--num-body-iters-first", type=int, default=100)
    p.add_argument("--num-body-iters", type=int, default=50)
    p.add_argument("--fix-shape", action="store_true")
    p.add_argument("--fix-foot", action="store_true")
    p.add_argument("--use-adam", action="store_true")
    p.add_argument("--save-pred-dir", type=Path, default=None)
    p.add_argument("--fail-fast", action="store_true")
    p.add_argument("--gpu-id", type=int, default=0)
    p.add_argument("--log-level", default="INFO", choices=["DEBUG", "INFO", "WARNING", "ERROR"])
    # this engine's additions
    p.add_argument("--batch-sequences", type=_positive, default=64,
                   help="sequences per optimize_params_sequences call (their chains run side by side)")
    p.add_argument("--model-dir", type=Path, default=None, help="directory of smpl_neutral.npz (default ./data/models/)")
    p.add_argument("--prior-dir", type=Path, default=None, help="directory of gmm_08.pkl (default ./data/models/)")
    p.add_argument("--mean-file", type=Path, default=None,
                   help="mean pose / shape (.h5 or .npz; default ./data/models/neutral_smpl_mean_params.h5)")
    p.add_argument("--position-metrics", action="store_true",
                   help="also report MPJPE and PA-MPJPE (mm) of the fitted joints against the input joints")
    return p.parse_args(argv)


def sequence_config(args: argparse.Namespace):
    """The reference's configuration of one evaluation fit (``cli/eval.py:163-179``)."""
    from ..core.config import FrameOptimizeConfig, SequenceOptimizeConfig
    frame = FrameOptimizeConfig(coordinate_mode="world", use_lbfgs=not args.use_adam,
                                num_iters_first=args.num_body_iters_first, num_iters_followup=args.num_body_iters,
                                joints_category="AMASS", freeze_betas=args.fix_shape)
    return SequenceOptimizeConfig(frame=frame, num_shape_iters=args.num_shape_iters, num_shape_frames=args.num_shape_frames,
                                  use_shape_optimization=not args.fix_shape, fix_foot=args.fix_foot,
                                  limit_frames=args.limit_frames if args.limit_frames > 0 else None)


def _assets(args, device):
    """Body model, pose prior and mean parameters, loaded once for the whole run."""
    from ..api.common import DEFAULT_MEAN_FILE
    from ..api.model_factory import load_body_model
    from ..core.config import BodyModelConfig
    from ..core.engine import load_mean_pose_shape
    from ..prior import MaxMixturePrior
    mcfg = BodyModelConfig(model_type="smpl") if args.model_dir is None else BodyModelConfig(model_type="smpl",
                                                                                            model_dir=args.model_dir)
    model = load_body_model(mcfg, device)
    prior = MaxMixturePrior(prior_folder=str(args.prior_dir) if args.prior_dir is not None else "./data/models/",
                            num_gaussians=8, device=device)
    mean = load_mean_pose_shape(str(args.mean_file) if args.mean_file is not None else DEFAULT_MEAN_FILE, device)
    return model, prior, mean


def main(argv: Optional[Sequence[str]] = None) -> float:
    """Run the evaluation; prints the dataset MPJAE line (after the two positional lines of ``--position-metrics``) and returns
    the MPJAE."""
    import torch
    from .. import evaluation
    from ..api.sequence import optimize_params_sequences
    from ..core.constants import category_indices
    args = parse_args(argv)
    configure_logging(args.log_level)
    if args.skip_start_frames < 0:
        raise ValueError("--skip-start-frames must be >= 0.")
    device = torch.device(f"cuda:{args.gpu_id}")
    files = evaluation.discover_amass_npz_files(args.amass_root)
    if args.limit_seqs > 0:
        files = files[: args.limit_seqs]
    if not files:
        raise FileNotFoundError(f"No .npz files found under {args.amass_root}")
    model, prior, mean = _assets(args, device)

    totals = {"sum": 0.0, "count": 0, "ok": 0, "failed": 0}
    # --position-metrics: the fit residual in positional terms, over the joints the fit matched (the AMASS correspondence)
    position = {"none": [0.0, 0], "procrustes": [0.0, 0]}
    model_rows, target_rows = category_indices("AMASS")

    def failed(path, exc):
        totals["failed"] += 1
        logger.warning("Failed on %s: %s", path, exc)
        if args.fail_fast:
            raise exc

    def score_positions(fit_joints, joints):
        """Sequence MPJPE / PA-MPJPE in mm over the frames after --skip-start-frames; adds them to the dataset sums."""
        fit = fit_joints[args.skip_start_frames:, model_rows]
        tgt = torch.as_tensor(joints[args.skip_start_frames:, target_rows])
        seq = {align: evaluation.evaluate_position_pair(fit, tgt, align=align, device=device) for align in position}
        for align, (_, err_sum, frames) in seq.items():       # both values exist before either joins the dataset sums
            position[align][0] += err_sum
            position[align][1] += frames
        return 1000.0 * seq["none"][0], 1000.0 * seq["procrustes"][0]

    def score(path, gt_pose, pred_pose, fit_joints=None, joints=None):
        if args.skip_start_frames > 0:
            if pred_pose.shape[0] <= args.skip_start_frames:
                raise ValueError(f"Sequence too short after skipping {args.skip_start_frames} frame(s): "
                                 f"{pred_pose.shape[0]} available.")
            pred_eval, gt_eval = pred_pose[args.skip_start_frames:], gt_pose[args.skip_start_frames:]
        else:
            pred_eval, gt_eval = pred_pose, gt_pose
        seq_mpjae, angle_sum, angle_count = evaluation.evaluate_pose_pair(pred_eval, gt_eval, device=device)
        seq_mpjpe, seq_pa = score_positions(fit_joints, joints) if args.position_metrics else (None, None)
        totals["sum"] += angle_sum
        totals["count"] += angle_count
        totals["ok"] += 1
        if args.save_pred_dir is not None:
            evaluation.save_prediction_pose(pred_pose, path, args.amass_root, args.save_pred_dir)
        if not args.position_metrics:
            logger.info("%s: MPJAE %.3f deg (dataset %.3f deg, %d ok, %d failed)", path.name, seq_mpjae,
                        totals["sum"] / totals["count"], totals["ok"], totals["failed"])
            return
        logger.info("%s: MPJAE %.3f deg, MPJPE %.3f mm, PA-MPJPE %.3f mm (dataset %.3f deg, %d ok, %d failed)", path.name,
                    seq_mpjae, seq_mpjpe, seq_pa, totals["sum"] / totals["count"], totals["ok"], totals["failed"])

    cfg = sequence_config(args)
    for start in range(0, len(files), args.batch_sequences):
        chunk = files[start: start + args.batch_sequences]
        loaded = []
        for path in chunk:
            try:
                joints, gt_pose = evaluation.load_amass_sequence(path)
                if args.limit_frames > 0:
                    joints, gt_pose = joints[: args.limit_frames], gt_pose[: args.limit_frames]
                loaded.append((path, joints, gt_pose))
            except Exception as exc:          # (the reference counts a file that does not load as failed)
                failed(path, exc)
        if not loaded:
            continue
        try:
            batch = optimize_params_sequences([j for _, j, _ in loaded], body_model="smpl", joint_layout="AMASS",
                                              model=model, config=cfg, device=device, pose_prior=prior, mean_params=mean)
        except Exception as exc:              # one bad sequence must not sink its neighbours: fit them one by one
            if args.fail_fast:
                raise
            logger.warning("batch of %d sequences failed (%s): fitting them one by one", len(loaded), exc)
            batch = None
        for i, (path, joints, gt_pose) in enumerate(loaded):
            try:
                if batch is None:
                    one = optimize_params_sequences([joints], body_model="smpl", joint_layout="AMASS", model=model,
                                                    config=cfg, device=device, pose_prior=prior, mean_params=mean)
                    pred, fit_joints = one.pose(0), one.joints_of(0)
                else:
                    pred, fit_joints = batch.pose(i), batch.joints_of(i)
                score(path, gt_pose, np.asarray(pred.detach().cpu().numpy(), dtype=np.float32), fit_joints, joints)
            except Exception as exc:
                failed(path, exc)
        logger.info("%d / %d sequences done", min(start + args.batch_sequences, len(files)), len(files))

    if totals["count"] == 0:
        raise RuntimeError("No valid sequence was evaluated.")
    dataset_mpjae = totals["sum"] / totals["count"]
    logger.info("Finished evaluation: success=%d failed=%d dataset_MPJAE=%.6f deg", totals["ok"], totals["failed"],
                dataset_mpjae)
    if args.position_metrics:
        mpjpe, pa_mpjpe = (1000.0 * acc[0] / acc[1] for acc in position.values())
        logger.info("dataset_MPJPE=%.6f mm dataset_PA-MPJPE=%.6f mm over %d frames", mpjpe, pa_mpjpe, position["none"][1])
        print(f"Dataset MPJPE(fit residual, {len(model_rows)} joints): {mpjpe:.6f} mm")
        print(f"Dataset PA-MPJPE(fit residual, {len(model_rows)} joints): {pa_mpjpe:.6f} mm")
    print(f"Dataset MPJAE(global_orient + body_pose): {dataset_mpjae:.6f} deg")
    return dataset_mpjae


if __name__ == "__main__":
    main()
