"""What does a multi-view warm-start chain (``k2b_fit_multiview_sequences``) cost?  The same videos fitted, same commit, same run:
  single view   ``k2b_fit_image_sequences``: the chain under the projected joint term of ONE pinhole camera (the yardstick);
  C = 1, 2, 4, 8  the new entry: the chain under the joint term summed over a rig of C calibrated cameras, ONE launch.
Workloads: 24 joints, one video of 195 frames and 1024 videos of 64 frames; SMPL-X, 256 videos of 64 frames; Adam 30 / 10
(bench.py's problems; camera c of a rig looks at the centre of the bodies from 3 m away or more (outside every frame's joints), turned by 2 pi c / C about the vertical axis,
500 px focals; the single view is camera 0).  The configurations alternate in chunks timed with device events after a warm-up of
all; the figure is the median chunk, the spread the range over the chunks.  Every workload runs in a child process of its own
under a time limit; the first that fails or runs out of time ends the run.
Usage: python tools/time_multiview_chain.py [--chunks 7] [--calls 5] [--limit 240] [--out FILE]     (prints a table and one JSON line)"""
import argparse
import json
import math
import statistics
import subprocess
import sys

FOCAL, DEPTH, FIRST, FOLLOW, PRESERVE = 500.0, 3.0, 30, 10, 5.0
VIEWS = (1, 2, 4, 8)
WORKLOADS = (("smpl", 1, 195), ("smpl", 1024, 64), ("smplx", 256, 64))


def rig(C, centre=(0.0, 0.0, 0.0), depth=DEPTH):
    """C rows (rotation (3,3), translation, focal): camera c = Ry(2 pi c / C), looking at `centre` from `depth` metres away."""
    cams = []
    for c in range(C):
        a = 2.0 * math.pi * c / C
        rot = [[math.cos(a), 0.0, math.sin(a)], [0.0, 1.0, 0.0], [-math.sin(a), 0.0, math.cos(a)]]
        t = [(depth if i == 2 else 0.0) - sum(rot[i][j] * centre[j] for j in range(3)) for i in range(3)]
        cams.append((rot, t, [FOCAL, FOCAL]))
    return cams


def measure(kind, S, T, chunks, calls):
    import torch

    sys.path.insert(0, ".")
    import bench
    from keypoints2body_amd import native
    from keypoints2body_amd.core.fitters.world_space import WorldSpaceFitter
    if not torch.cuda.is_available():
        raise SystemExit("time_multiview_chain.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    n = S * T
    model, prior, j3d, init = bench.build_problem(n, 0, n, 1000, dev, kind)
    fitter = WorldSpaceFitter(model, step_size=1e-2, num_iters_first=FIRST, num_iters_followup=FOLLOW, use_lbfgs=False,
                              joints_category="AMASS" if kind == "smpl" else "GENERIC", device=dev, pose_prior=prior)
    start = fitter.packed_init(init) if model.packed else init
    idx = list(range(j3d.shape[1]))
    lengths = [T] * S
    first = lambda a: a[::T].contiguous()                             # sequence s owns rows s T .. s T + T - 1
    world = [first(a) for a in (start.global_orient, start.body_pose, start.betas, start.transl)]
    centre = [float(x) for x in j3d.mean(dim=(0, 1)).cpu()]         # the rig looks at the centre of all bodies
    # (a motion walks: every camera stands at least a metre outside the circle that holds all joints of all frames)
    depth = max(DEPTH, float((j3d - torch.tensor(centre, device=dev))[..., [0, 2]].norm(dim=-1).max()) + 1.0)
    shift = torch.tensor(rig(1, centre, depth)[0][1], device=dev)
    single = world[:3] + [(world[3] + shift).contiguous()]           # the single view's translation is the camera's

    def project(cams):                                                # (n, C, K, 3) rows (u', v', 0)
        views = []
        for rot, t, f in cams:
            q = j3d @ torch.tensor(rot, device=dev).T + torch.tensor(t, device=dev)
            uv = torch.zeros_like(q)
            uv[..., 0], uv[..., 1] = f[0] * q[..., 0] / q[..., 2], f[1] * q[..., 1] / q[..., 2]
            assert bool((q[..., 2] > 0.2).all()), float(q[..., 2].min())
            views.append(uv)
        return torch.stack(views, dim=1).contiguous()

    cfg = fitter._chain_config(1.0, PRESERVE, False, False)
    cfg.projection, cfg.focal[0], cfg.focal[1] = 1, FOCAL, FOCAL
    m, p = model.native, prior.native
    uv1 = project(rig(1, centre, depth))[:, 0].contiguous()
    ways = {"single": lambda: native.fit_image_sequences(m, p, cfg, FOLLOW, False, idx, lengths, uv1, None, *single)}
    for C in VIEWS:
        table, uv = native.camera_table(rig(C, centre, depth)), project(rig(C, centre, depth))
        ways[f"C{C}"] = (lambda table=table, uv=uv: native.fit_multiview_sequences(m, p, cfg, FOLLOW, False, table, idx, lengths, uv, None, *world))
    for run in ways.values():                                         # warm-up: code objects, Adam tables
        for _ in range(2):
            out = run()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out["loss"]).all())
    ms = {k: [] for k in ways}
    for _ in range(chunks):
        for name, run in ways.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                run()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / calls)
    med = {k: statistics.median(v) for k, v in ms.items()}
    row = dict(model=kind, sequences=S, frames=T, first=FIRST, follow=FOLLOW, chunks=chunks, calls=calls,
               depth=depth, ms=med, range={k: [min(v), max(v)] for k, v in ms.items()},
               spread={k: (max(v) - min(v)) / med[k] for k, v in ms.items()},
               us_per_frame={k: 1e3 * med[k] / n for k in ways},
               ratio_to_single={k: med[k] / med["single"] for k in ways if k != "single"})
    print(json.dumps(row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds a workload's process may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", nargs=3, metavar=("MODEL", "S", "T"), default=None, help="measure this workload in this process")
    a = ap.parse_args()
    if a.one:
        return measure(a.one[0], int(a.one[1]), int(a.one[2]), a.chunks, a.calls)
    rows, not_timed = [], []
    for i, (kind, S, T) in enumerate(WORKLOADS):
        cmd = [sys.executable, __file__, "--one", kind, str(S), str(T), "--chunks", str(a.chunks), "--calls", str(a.calls)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            r = None
        if r is None or r.returncode != 0:                            # nothing more is started on the GPU behind a failure
            not_timed = [f"{k} {s} x {t}" for k, s, t in WORKLOADS[i:]]
            print(f"{kind} {S} x {T}: {'time limit' if r is None else 'exit status %d' % r.returncode}; not timed: {not_timed}")
            if r is not None:
                print(r.stderr[-2000:])
            break
        row = json.loads(r.stdout.strip().splitlines()[-1])
        rows.append(row)
        cols = "   ".join(f"{k} {row['ms'][k]:.3f} ms ({row['ratio_to_single'][k]:.3f}, spread {100 * row['spread'][k]:.1f} %)" for k in row["ratio_to_single"])
        print(f"{kind:5s} {S:4d} x {T:3d} frames: single view {row['ms']['single']:.3f} ms ({row['us_per_frame']['single']:.2f} us/frame, spread "
              f"{100 * row['spread']['single']:.1f} %)   {cols}")
    line = json.dumps({"tool": "time_multiview_chain", "focal": FOCAL, "depth": DEPTH, "rows": rows, "not_timed": not_timed})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 1 if not_timed else 0


if __name__ == "__main__":
    sys.exit(main())
