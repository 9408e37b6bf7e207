"""What does a projected warm-start chain (``k2b_fit_image_sequences``) cost?  Three ways to fit the same videos, same commit:
  chain      the new entry: every sequence's chain in ONE launch;
  chain 3D   ``k2b_fit_sequences`` on the same shapes with the 3D joint term (what the projected form adds to the chain);
  host loop  one ``k2b_fit_world`` launch per time step with ``projection = 1``, each frame started from its predecessor's result:
             the only way to fit a video without the new entry.
Workloads: one sequence of 195 frames and 1024 sequences of 64 frames, Adam 30 / 10, SMPL and SMPL-X (bench.py's problems; the
projected targets are those joints seen by a 500 px pinhole camera 3 m away).  The three alternate in chunks timed with device
events after a warm-up of all; the figure is the median chunk, the spread the range over the chunks.  Every workload runs in a
child process of its own under a time limit; the first that fails or runs out of time ends the run.
Usage: python tools/time_reproj_chain.py [--chunks 7] [--calls 5] [--limit 240] [--out FILE]     (prints a table and one JSON line)"""
import argparse
import json
import statistics
import subprocess
import sys

FOCAL, DEPTH, FIRST, FOLLOW, PRESERVE = 500.0, 3.0, 30, 10, 5.0
WORKLOADS = (("smpl", 1, 195), ("smpl", 1024, 64), ("smplx", 1, 195), ("smplx", 1024, 64))


def measure(kind, S, T, chunks, calls):
    import copy

    import torch

    sys.path.insert(0, ".")
    import bench
    from keypoints2body_amd import native
    from keypoints2body_amd.core.fitters.world_space import WorldSpaceFitter
    if not torch.cuda.is_available():
        raise SystemExit("time_reproj_chain.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    n = S * T
    model, prior, j3d, init = bench.build_problem(n, 0, n, 1000, dev, kind)
    fitter = WorldSpaceFitter(model, step_size=1e-2, num_iters_first=FIRST, num_iters_followup=FOLLOW, use_lbfgs=False,
                              joints_category="AMASS" if kind == "smpl" else "GENERIC", device=dev, pose_prior=prior)
    start = fitter.packed_init(init) if model.packed else init
    idx = list(range(j3d.shape[1]))
    lengths = [T] * S
    shift = torch.tensor([0.0, 0.0, DEPTH], device=dev)
    first = lambda a: a[::T].contiguous()                             # sequence s owns rows s T .. s T + T - 1
    rows3 = [first(a) for a in (start.global_orient, start.body_pose, start.betas, start.transl)]
    rowsp = rows3[:3] + [(rows3[3] + shift).contiguous()]
    cam = j3d + shift
    uv = torch.zeros_like(cam)
    uv[..., :2] = FOCAL * cam[..., :2] / cam[..., 2:3]
    j3d, uv = j3d.contiguous(), uv.contiguous()
    cfg3 = fitter._chain_config(600.0, PRESERVE, False, False)
    cfgp = fitter._chain_config(1.0, PRESERVE, False, False)
    cfgp.projection, cfgp.focal[0], cfgp.focal[1] = 1, FOCAL, FOCAL
    step_cfg = []
    for t in range(2):                                                # the host loop's two configurations: first frame, follow-up
        c = copy.copy(cfgp)
        c.num_iters, c.pose_preserve_weight = (FIRST, 0.0) if t == 0 else (FOLLOW, PRESERVE)
        step_cfg.append(c)
    per_step = [uv[t::T].contiguous() for t in range(T)]
    m, p = model.native, prior.native

    def host_loop():
        cur, out = rowsp, None
        for t in range(T):
            out = native.fit_world(m, p, step_cfg[min(t, 1)], idx, per_step[t], None, *cur)
            cur = [out[k] for k in native.PARAM_KEYS]
        return out

    ways = {"chain": lambda: native.fit_image_sequences(m, p, cfgp, FOLLOW, False, idx, lengths, uv, None, *rowsp),
            "chain_3d": lambda: native.fit_sequences(m, p, cfg3, FOLLOW, idx, lengths, j3d, None, *rows3),
            "host_loop": host_loop}
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
               ms={k: med[k] for k in ways}, range={k: [min(v), max(v)] for k, v in ms.items()},
               us_per_frame={k: 1e3 * med[k] / n for k in ways},
               ratio_to_3d=med["chain"] / med["chain_3d"], host_loop_over_chain=med["host_loop"] / med["chain"])
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
        g = row["range"]
        step = {k: 1e3 * v / T for k, v in row["ms"].items()}          # us per time step of the chains (S frames side by side)
        print(f"{kind:5s} {S:4d} x {T:3d} frames: chain {row['ms']['chain']:.3f} ms ({step['chain']:.2f} us/step) [{g['chain'][0]:.3f} .. {g['chain'][1]:.3f}]   "
              f"3D chain {row['ms']['chain_3d']:.3f} ms ({step['chain_3d']:.2f} us/step)   host loop {row['ms']['host_loop']:.3f} ms "
              f"({step['host_loop']:.2f} us/step)   projected / 3D {row['ratio_to_3d']:.3f}   host loop / chain {row['host_loop_over_chain']:.2f}")
    line = json.dumps({"tool": "time_reproj_chain", "focal": FOCAL, "depth": DEPTH, "rows": rows, "not_timed": not_timed})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 1 if not_timed else 0


if __name__ == "__main__":
    sys.exit(main())
