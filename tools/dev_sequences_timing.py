"""Timing of the ragged warm-start chains (``k2b_fit_sequences_lbfgs``: the reference's default sequence mode, L-BFGS 30 / 10)
for S = 1, 64, 256, 512, 1024 synthetic sequences of 195 frames, on the synthetic SMPL model and mixture.

    python tools/dev_sequences_timing.py [--sizes 1,64,256,512,1024] [--frames 195] [--reps 3] [--adam] [--shape-pass]
                                         [--single] [--out FILE]

Prints one JSON line per S: median device time of the one chain launch (CUDA events around the call), frames/s, and the
ratio to S = 1.  ``--shape-pass`` also times the batched shape pre-pass of the default configuration
(``optimize_shape_pass_batched``: 40 iterations over the first 50 frames of every sequence) and the two together.
``--single`` times the existing one-sequence entry ``k2b_fit_sequence_lbfgs`` (S = 1 only) for comparison.  Under
``rocprofv3 --kernel-trace --stats`` the kernel statistics show the launch count (one ``k2b_fit_world_kernel`` per chain call)."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,64,256,512,1024")
    ap.add_argument("--frames", type=int, default=195)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--adam", action="store_true")
    ap.add_argument("--shape-pass", action="store_true")
    ap.add_argument("--single", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from keypoints2body_amd import native, synthetic
    dev = torch.device("cuda:0")
    c = synthetic.make_body_model(0)
    g = synthetic.make_gmm(0)
    from keypoints2body_amd.prior import MixtureBuffers
    mb = MixtureBuffers.from_mixture(g.means, g.covars, g.weights)
    model = native.NativeModel(c.v_template, c.shapedirs, c.posedirs, c.J_regressor, c.lbs_weights, c.parents,
                               c.extra_vertex_ids, device=dev)
    prior = native.NativePrior(mb.means, mb.precisions, mb.nll_weights, device=dev)
    sizes = [int(s) for s in a.sizes.split(",")] if not a.single else [1]
    from keypoints2body_amd.models.body_model import BodyModel
    from keypoints2body_amd.prior import MaxMixturePrior
    body = BodyModel.synthetic(0, device=dev) if a.shape_pass else None
    gmm = MaxMixturePrior(mb, device=dev) if a.shape_pass else None
    T = a.frames
    rows = []
    base = None
    for S in sizes:
        N = S * T
        p = synthetic.make_poses(N, seed=S)
        t = lambda x: torch.as_tensor(np.asarray(x, np.float32), device=dev).contiguous()
        j, _ = model.lbs(t(p.global_orient), t(p.body_pose), t(p.betas), t(p.transl), want_vertices=False)
        j3d = j[:, :22].contiguous()
        lengths = np.full(S, T, np.int32)
        z = lambda k: torch.zeros(S, k, device=dev)
        tr = j3d[torch.arange(S, device=dev) * T, 0].contiguous()
        cfg = native.default_fit_config()
        cfg.pose_preserve_weight = 5.0
        cfg.num_iters = 30

        def timed(fn):
            fn()
            torch.cuda.synchronize()
            ms = []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                res = fn()
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1))
            return float(np.median(ms)), ms, res

        def shape_pass():
            from keypoints2body_amd.core.config import SequenceOptimizeConfig
            from keypoints2body_amd.core.engine import optimize_shape_pass_batched
            cfg_s = SequenceOptimizeConfig()
            cfg_s.frame.joints_category = "AMASS"
            seqs = [j3d[s * T:(s + 1) * T] for s in range(S)]
            return optimize_shape_pass_batched(body, cfg_s, torch.zeros(1, 10, device=dev), torch.zeros(1, 72, device=dev), seqs,
                                               [torch.ones(22, device=dev)] * S, dev, pose_prior=gmm)

        def run():
            if a.single:
                return native.fit_sequence_lbfgs(model, prior, cfg, 30, 10, list(range(22)), j3d, None, z(3), z(69), z(10), tr,
                                                 lr=1.0)
            if a.adam:
                return native.fit_sequences(model, prior, cfg, 10, list(range(22)), lengths, j3d, None, z(3), z(69), z(10), tr)
            return native.fit_sequences_lbfgs(model, prior, cfg, 30, 10, list(range(22)), lengths, j3d, None, z(3), z(69), z(10),
                                              tr, lr=1.0)
        run()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = run()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        assert bool(torch.isfinite(out["loss"]).all())
        med = float(np.median(ms))
        base = med if base is None else base
        r = {"S": S, "frames_per_sequence": T, "branch": "single" if a.single else ("adam" if a.adam else "lbfgs"),
             "call_ms_median": round(med, 3),
             "call_ms_all": [round(x, 3) for x in ms], "frames_per_s": round(N / (med / 1e3), 1),
             "ms_ratio_to_first_size": round(med / base, 3)}
        if a.shape_pass:
            sp, sp_all, betas = timed(shape_pass)
            assert bool(torch.isfinite(betas).all())
            r.update({"shape_pass_ms_median": round(sp, 3), "shape_pass_ms_all": [round(x, 3) for x in sp_all],
                      "default_config_ms": round(sp + med, 3), "default_config_frames_per_s": round(N / ((sp + med) / 1e3), 1)})
        rows.append(r)
        print(json.dumps(r), flush=True)
    if a.out:
        Path(a.out).write_text(json.dumps(rows, indent=1) + "\n")


if __name__ == "__main__":
    main()
