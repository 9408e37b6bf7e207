#!/usr/bin/env python3
"""Throw-away timing of ``k2b_fit_multiview`` against the single-view and the 3D launches: 100 Adam iterations
in one launch, synthetic models of tests/fit_gradient_common.py, frames tiled from the seeded cases of tests/multiview_common.py.

    python tools/time_multiview.py --out multiview_timing.json                                 # device events, profiler off
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_multiview.py --calls DIR/calls.json --repeats 5
    python tools/time_multiview.py --parse DIR                                                  # kernel times of that trace per call

Configurations per (model, frames): ``3d`` (k2b_fit_world), ``proj`` (k2b_fit_world under projection = 1: the baseline) and
``views1/2/4/8``.  They alternate inside every repeat, after a warm-up of every one; the table gives the median and the
spread (min .. max) of a configuration and its ratio to ``proj``.  With a package that has no ``fit_multiview`` (an older
commit on ``PYTHONPATH``) only ``3d`` and ``proj`` run: that is how the parent commit is timed in the same session."""
import argparse
import csv
import glob
import json
import os
import sys

import numpy as np

sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))     # (behind PYTHONPATH: an older package there wins)

SIZES = (("smpl10", 1024), ("smpl10", 4096), ("smplx20", 1024))
VIEWS = (1, 2, 4, 8)
ITERS = 100
FIT_KERNELS = ("k2b_fit_world_kernel", "k2b_fit_tree_kernel")


def tile(a, B):
    return None if a is None else np.ascontiguousarray(np.resize(a, (B,) + a.shape[1:]))


def configurations(kind, B):
    """{label: closure that queues one fit launch}; every input is uploaded here, before any timing."""
    import torch
    from keypoints2body_amd import native
    from tests import fit_gradient_common as G
    from tests import helpers as H
    from tests import reproj_common as R
    model, prior = G.native_model(kind), H.native_prior()

    def inputs(case):
        return [H.cuda(tile(a, B)) for a in (case.go, case.pose, case.shape, case.tr)], H.cuda(tile(case.j3d, B))

    def adam(cfg):
        cfg.num_iters, cfg.step_size, cfg.transl_prior_weight = ITERS, 1e-2, 0.0
        return cfg

    out = {}
    c3 = G.base(kind, B=17)
    ins3, j3 = inputs(c3)
    cfg3 = adam(G.fit_config(c3))
    out["3d"] = lambda: native.fit_world(model, prior, cfg3, list(c3.idx), j3, None, *ins3)
    cp = R.base(kind, B=17)
    insp, jp = inputs(cp)
    cfgp = adam(R.fit_config(cp))
    out["proj"] = lambda: native.fit_world(model, prior, cfgp, list(cp.idx), jp, None, *insp)
    if hasattr(native, "fit_multiview"):
        from tests import multiview_common as MV
        for C in VIEWS:
            cv = MV.base(kind, C, B=17, seed=13)
            insv, jv = inputs(cv)
            cfgv = adam(MV.fit_config(cv))
            table = native.camera_table(list(cv.cams))
            out[f"views{C}"] = (lambda cv=cv, insv=insv, jv=jv, cfgv=cfgv, table=table:
                                native.fit_multiview(model, prior, cfgv, table, list(cv.idx), jv, None, *insv))
    torch.cuda.synchronize()
    return out


def measure(repeats, warmup, calls_path):
    import torch
    results, calls = {}, []
    for kind, B in SIZES:
        runs = configurations(kind, B)
        for _ in range(warmup):
            for run in runs.values():
                run()
        torch.cuda.synchronize()
        times = {k: [] for k in runs}
        for _ in range(repeats):
            for label, run in runs.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                run()
                b.record()
                b.synchronize()
                times[label].append(1e3 * a.elapsed_time(b))                 # microseconds
                calls.append(f"{kind}/{B}/{label}")
        results[f"{kind}/{B}"] = times
    if calls_path:
        json.dump({"warmup_calls_per_size": warmup, "sizes": [f"{k}/{b}" for k, b in SIZES], "timed_calls": calls}, open(calls_path, "w"))
    return results


def report(results, unit="us per launch of 100 iterations (device events around the call)"):
    print(f"# {unit}: median [min .. max], ratio of medians to proj")
    for size, times in results.items():
        base = float(np.median(times["proj"]))
        for label, t in times.items():
            print(f"{size:14s} {label:7s} {np.median(t):9.1f} [{min(t):9.1f} .. {max(t):9.1f}]  x{np.median(t) / base:5.3f}  n={len(t)}")


def parse(directory):
    """Kernel times of a ``rocprofv3 --kernel-trace`` run of this script: the fit kernels in start order against calls.json."""
    meta = json.load(open(os.path.join(directory, "calls.json")))
    (trace,) = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    rows = [r for r in csv.DictReader(open(trace)) if any(k in r["Kernel_Name"] for k in FIT_KERNELS)]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    dur = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows]
    calls = meta["timed_calls"]
    per_size = {s: [c for c in calls if c.startswith(s + "/")] for s in meta["sizes"]}
    labels_per_size = {s: list(dict.fromkeys(c.rsplit("/", 1)[1] for c in v)) for s, v in per_size.items()}
    expected = sum(len(v) + meta["warmup_calls_per_size"] * len(labels_per_size[s]) for s, v in per_size.items())
    if len(dur) != expected:
        raise SystemExit(f"{len(dur)} fit-kernel dispatches in the trace for {expected} calls: a call is more than one launch; read the stats file instead")
    results, at = {}, 0
    for s in meta["sizes"]:
        at += meta["warmup_calls_per_size"] * len(labels_per_size[s])
        times = {k: [] for k in labels_per_size[s]}
        for c in per_size[s]:
            times[c.rsplit("/", 1)[1]].append(dur[at])
            at += 1
        results[s] = times
    report(results, "us of kernel time per launch of 100 iterations (rocprofv3 --kernel-trace)")
    return results


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out")
    ap.add_argument("--calls")
    ap.add_argument("--parse")
    args = ap.parse_args()
    res = parse(args.parse) if args.parse else measure(args.repeats, args.warmup, args.calls)
    if not args.parse:
        report(res)
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)
