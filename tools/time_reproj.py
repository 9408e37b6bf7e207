"""What does the projected joint term (``k2b_fit_config.projection = 1``) cost?  The fused fit launch with the perspective
reprojection residual against the same launch with the 3D residual, same commit, same batch, same launch shape: 1024 and 4096
frames of SMPL and 1024 frames of SMPL-X, 100 Adam iterations (bench.py's problems; the projected targets are those joints
seen by a 500 px pinhole camera 3 m away).  Per configuration the two forms alternate in chunks of launches timed with
device events after a warm-up of both; the figure is the median chunk, the spread the range over the chunks.
Usage: python tools/time_reproj.py [--chunks 9] [--launches 40]      (prints a table and one JSON line)"""
import argparse
import dataclasses
import json
import statistics
import sys

import torch

sys.path.insert(0, ".")
import bench
from keypoints2body_amd.core.fitters.world_space import WorldSpaceFitter

FOCAL, DEPTH, ITERS = 500.0, 3.0, 100
CONFIGS = (("smpl", 1024), ("smpl", 4096), ("smplx", 1024))


def problem(kind, frames, dev):
    model, prior, j3d, init = bench.build_problem(frames, 0, frames, 1000, dev, kind)
    fitter = WorldSpaceFitter(model, step_size=1e-2, num_iters_first=ITERS, num_iters_followup=ITERS, use_lbfgs=False,
                              joints_category="AMASS" if kind == "smpl" else "GENERIC", device=dev, pose_prior=prior)
    start = fitter.packed_init(init) if model.packed else init
    idx = list(range(j3d.shape[1]))
    cfg3 = fitter._packed_config(fitter._config(0, 600.0, 5.0, False, False))
    # the same scene DEPTH metres down the optical axis, as centred pixels (third column unused)
    cam = j3d + torch.tensor([0.0, 0.0, DEPTH], device=dev)
    uv = torch.zeros_like(cam)
    uv[..., :2] = FOCAL * cam[..., :2] / cam[..., 2:3]
    start_p = dataclasses.replace(start, transl=(start.transl + torch.tensor([0.0, 0.0, DEPTH], device=dev)).contiguous())
    cfgp = fitter._packed_config(fitter._config(0, 1.0, 5.0, False, False))
    cfgp.projection, cfgp.focal[0], cfgp.focal[1] = 1, FOCAL, FOCAL
    return fitter, idx, (cfg3, j3d.contiguous(), start), (cfgp, uv.contiguous(), start_p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=9)
    ap.add_argument("--launches", type=int, default=40)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_reproj.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    rows = []
    for kind, frames in CONFIGS:
        fitter, idx, form3, formp = problem(kind, frames, dev)
        run = lambda f: fitter.fit_params(f[0], f[1], f[2], idx)
        for f in (form3, formp):                                  # warm-up: code objects, Adam tables
            for _ in range(3):
                out = run(f)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out["loss"]).all())
        ms = {"3d": [], "projected": []}
        for _ in range(a.chunks):
            for name, f in (("3d", form3), ("projected", formp)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.launches):
                    run(f)
                e1.record()
                torch.cuda.synchronize()
                ms[name].append(e0.elapsed_time(e1) / a.launches)
        med = {k: statistics.median(v) for k, v in ms.items()}
        rows.append(dict(model=kind, frames=frames, iters=ITERS, ms_3d=med["3d"], ms_projected=med["projected"],
                         ratio=med["projected"] / med["3d"], range_3d=[min(ms["3d"]), max(ms["3d"])],
                         range_projected=[min(ms["projected"]), max(ms["projected"])], chunks=a.chunks, launches=a.launches))
        r = rows[-1]
        print(f"{kind:5s} {frames:5d} frames: 3D {r['ms_3d']:.4f} ms [{r['range_3d'][0]:.4f} .. {r['range_3d'][1]:.4f}]   projected "
              f"{r['ms_projected']:.4f} ms [{r['range_projected'][0]:.4f} .. {r['range_projected'][1]:.4f}]   ratio {r['ratio']:.3f}")
    print(json.dumps({"tool": "time_reproj", "focal": FOCAL, "depth": DEPTH, "rows": rows}))


if __name__ == "__main__":
    main()
