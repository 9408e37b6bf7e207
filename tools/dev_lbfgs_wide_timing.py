"""Development: wall time (call + synchronise) of ``fit_world_lbfgs`` at ``max_iter = 30``.

    --case wide      the 55-joint model with 26 shape coefficients (P = 194: the step kernel's wide form), B = 1, 256, 1024, the
                     device driver and beside it the host driver (``lbfgs_driver = "host"``: the lock-step numpy twin over
                     evaluate-only launches - the only way a build without the wide form runs this fit)
    --case existing  the SMPL-X model with 20 shape coefficients and the SMPL model, B = 256 each (the narrow form); with
                     ``--lib PATH/libk2b.so`` on another build of the library, for parent-against-branch rounds
    --case trace     a few wide fits at B = 256 and nothing else: the program to put under ``rocprofv3 --kernel-trace``
    --summarise DIR  kernel durations of a ``rocprofv3 --kernel-trace --output-format csv -d DIR`` run (no GPU needed)

One line per measurement: median, minimum and maximum over ``--repeats`` calls after three warm-up calls."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np


def summarise(d):
    import csv, glob
    dur = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            n = r["Kernel_Name"].split("(")[0][-48:]
            dur.setdefault(n, []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    for n, v in sorted(dur.items()):
        print(f"{n:50s} calls {len(v):6d}  median {statistics.median(v) / 1e3:8.2f} us  mean {statistics.mean(v) / 1e3:8.2f} us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("wide", "existing", "trace"), default="wide")
    ap.add_argument("--lib")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--label", default="")
    ap.add_argument("--summarise")
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise)
    import torch
    from pathlib import Path
    from keypoints2body_amd import native, synthetic
    if args.lib:
        native._LIB_PATH = Path(args.lib).resolve()
    from tests import helpers as H
    pr = H.native_prior()

    def timed(name, run, repeats=args.repeats):
        for _ in range(3):
            run()
        torch.cuda.synchronize()
        ts = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0))
        print(f"{args.label}{name}: median {statistics.median(ts):9.3f} ms  min {min(ts):9.3f}  max {max(ts):9.3f}  ({repeats} calls)", flush=True)

    def tree_problem(m, NB, B):
        rng = np.random.default_rng(4)
        go, pose, shape, tr = (0.2 * rng.standard_normal((B, 3)), 0.15 * rng.standard_normal((B, 162)), 0.3 * rng.standard_normal((B, NB)),
                               rng.standard_normal((B, 3)))
        j3d = m.lbs(H.cuda(go), H.cuda(pose), H.cuda(shape), H.cuda(tr), want_vertices=False)[0][:, :55].contiguous()
        z = lambda c: torch.zeros(B, c, device="cuda")
        tr0 = (j3d[:, 0] - m.lbs(z(3), z(162), z(NB), None, want_vertices=False)[0][:, 0]).contiguous()
        return j3d, (z(3), z(162), z(NB), tr0)

    if args.case == "existing":
        m = H.native_model_x()
        j3d, init = tree_problem(m, 20, 256)
        cfg = native.default_fit_config()
        cfg.prior_pose_dims, cfg.num_betas_prior = 63, 10
        timed("SMPL-X NB 20 (P 188), B 256", lambda: native.fit_world_lbfgs(m, pr, cfg, list(range(55)), j3d, None, *init, max_iter=30, lr=1e-2))
        ms = H.native_model()
        p = synthetic.make_poses(256, seed=3)
        go, bp, be, tr = map(H.cuda, (p.global_orient, p.body_pose, p.betas, p.transl))
        j22 = ms.lbs(go, bp, be, tr, want_vertices=False)[0][:, :22].contiguous()
        cs = native.default_fit_config()
        timed("SMPL (P 85), B 256", lambda: native.fit_world_lbfgs(ms, pr, cs, list(range(22)), j22, None, go * 0.8, bp * 0.8, be * 0.5, tr + 0.02,
                                                                    max_iter=30, lr=1e-2))
        return

    # the wide model: its targets come from the oracle's CPU forward, as in tests/test_gpu_lbfgs_wide.py (written when k2b_lbs
    # did not skin a 55-joint model with more than 24 shape coefficients; kept so that the figures stay comparable)
    from keypoints2body_amd.core.fitters.world_space import WorldSpaceFitter
    from keypoints2body_amd.models.smpl_data import SMPLXData
    from tests import test_gpu_lbfgs_wide as W
    model, prior, _ = W._public()
    cfg = W._cfg(26)
    if args.case == "trace":
        j3d, init = W._problem(26, 256)
        for _ in range(5):
            native.fit_world_lbfgs(model.native, pr, cfg, list(range(55)), j3d, None, *init, max_iter=30, lr=1e-2)
        torch.cuda.synchronize()
        return
    for B in (1, 256, 1024):
        j3d, init = W._problem(26, B)
        timed(f"wide NB 26 (P 194), B {B}, device driver",
              lambda: native.fit_world_lbfgs(model.native, pr, cfg, list(range(55)), j3d, None, *init, max_iter=30, lr=1e-2))
        z = lambda n: torch.zeros(B, n)
        start = SMPLXData(betas=z(16), global_orient=z(3), body_pose=z(63), transl=init[3].cpu(), left_hand_pose=z(45), right_hand_pose=z(45),
                          expression=z(10), jaw_pose=z(3), leye_pose=z(3), reye_pose=z(3))
        fitter = WorldSpaceFitter(model, step_size=1e-2, num_iters_first=30, use_lbfgs=True, joints_category="GENERIC", pose_prior=prior)
        fitter.lbfgs_driver = "host"
        idx = torch.arange(55)
        timed(f"wide NB 26 (P 194), B {B}, host driver",
              lambda: fitter.fit_batch(start, j3d, None, seq_ind=0, target_model_indices=idx, run_forward=False), repeats=3)


if __name__ == "__main__":
    main()
