"""Development: IK-GAT inference timing (k2b_ikgat_kernel) at the default network shape (22 joints, H 128, 3 layers,
4 heads, pos-rot6: 9 inputs, seeded weights).  Each figure is the median of repeats of a call that ends in a device
synchronise, after a warm-up of the same shape:

* a 4096-frame batch (one launch), with its fp32 share of the 157.3 TF peak from the FLOPs counted below;
* the 96- and 195-frame chain (one launch, one workgroup walking the frames);
* ``optimize_params_frame`` with a warm network cache (host work, one launch, one device-to-host copy).

Kernel times come from a separate ``rocprofv3 --kernel-trace --stats`` run of this script.
Usage: python tools/dev_ikgat_timing.py [--repeats N] [--out FILE.json]"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from keypoints2body_amd import optimize_params_frame, synthetic  # noqa: E402
from keypoints2body_amd.core.config import FrameOptimizeConfig  # noqa: E402
from keypoints2body_amd.core.estimators.ikgat import IKGATEstimator  # noqa: E402
from keypoints2body_amd.models.smpl_data import SMPLData  # noqa: E402

J, IN, H, L, NH = 22, 9, 128, 3, 4
PEAK_FP32 = 157.3e12


def flops_per_frame(J=J, IN=IN, H=H, L=L, NH=NH, edges=3 * J - 2):
    """Multiply-adds x 2 of the network (shapes only): projections, attention logits, aggregation, head."""
    H2 = H // 2
    f = 2 * J * IN * H * 2                       # input_proj + residual_proj
    f += L * (2 * J * H * H + 2 * 2 * J * H + 2 * edges * H)     # GAT projection, a_src / a_dst, weighted sum
    f += 2 * J * H * H2 + 2 * J * H2 * 6         # head
    return f


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    root = Path(tempfile.mkdtemp(prefix="k2b_ikgat_timing_"))
    d = root / "ikgat" / "pos-rot6_to_rot6"
    d.mkdir(parents=True)
    torch.save({k: torch.from_numpy(v) for k, v in synthetic.make_ikgat_state(J, IN, H, L, NH, seed=0).items()}, d / "smplx.pth")
    parents = [int(p) for p in synthetic.SMPL_PARENTS[:J]]
    fcfg = dict(estimator_type="ikgat", coordinate_mode="camera", ikgat_model_dir=str(root), ikgat_model_format="smplx",
                ikgat_model_type="pos-rot6_to_rot6", ikgat_parent_ids=parents)
    est = IKGATEstimator(FrameOptimizeConfig(**fcfg))
    dev = est.device
    with np.load(Path(__file__).resolve().parents[1] / "tests" / "golden" / "ikgat_chain.npz") as z:
        motion, q0 = z["positions"], z["init_quaternions"]
    rec = {"shape": dict(J=J, input_dim=IN, hidden=H, layers=L, heads=NH), "repeats": args.repeats}

    B = 4096
    pos = torch.as_tensor(motion[np.arange(B) % motion.shape[0]], device=dev).contiguous()
    q = torch.as_tensor(np.broadcast_to(q0, (B, J, 4)).copy(), device=dev)
    t = timed(lambda: est.predict_frames(pos, q), args.repeats)
    fl = flops_per_frame() * B
    rec["batch_4096_ms"] = 1e3 * t
    rec["batch_4096_gflop"] = fl / 1e9
    rec["batch_4096_fp32_share_of_peak_wall"] = fl / t / PEAK_FP32
    print(f"[ikgat] batch 4096 frames: {1e3 * t:.3f} ms (wall, synchronised), {fl / 1e9:.2f} GFLOP, "
          f"{100 * fl / t / PEAK_FP32:.1f} % of the fp32 peak", flush=True)

    long = np.concatenate([motion, motion[::-1], motion[:3]])       # 195 frames
    for T in (96, 195):
        p = torch.as_tensor(long[:T], device=dev).contiguous()
        qi = torch.as_tensor(q0[None], device=dev).contiguous()
        t = timed(lambda: est.predict_frames(p, qi, chain=True), args.repeats)
        rec[f"chain_{T}_ms"] = 1e3 * t
        rec[f"chain_{T}_us_per_frame"] = 1e6 * t / T
        print(f"[ikgat] chain {T} frames: {1e3 * t:.3f} ms, {1e6 * t / T:.1f} us per frame", flush=True)

    z = lambda c: torch.zeros((1, c))
    init = SMPLData(betas=z(10), global_orient=z(3), body_pose=z(69), metadata={"ikgat_quaternions": q0})
    t = timed(lambda: optimize_params_frame(motion[5], prev_params=init, body_model="smpl", config=dict(fcfg)), args.repeats)
    rec["frame_call_warm_ms"] = 1e3 * t
    print(f"[ikgat] optimize_params_frame, warm cache: {1e3 * t:.3f} ms", flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
