#!/usr/bin/env python
"""Development timing of ``k2b_lbs_backward`` (not part of bench.py).

Per size - SMPL (V = 6890) at 1024 and 4096 frames, SMPL-X (V = 10 475, 20 shape coefficients) at 1024 frames - five rounds of
200 calls after a warm-up, three partners alternating inside every round, in one process:

  new   ``NativeModel.lbs_backward`` with both cotangents
  (a)   ``NativeModel.lbs`` (``k2b_lbs``) on the same batch
  (b)   the backward through the CPU-oracle module (``oracle/smpl_torch.py``) moved to the same GPU: ``torch.autograd.grad``
        of the same loss on retained graphs - what a user has to do without the entry.  The batch goes through the oracle in
        blocks of frames whose largest intermediate (the skinning weights expanded over the block, frames x V x J floats) stays
        under 1 GiB: 1024 frames for SMPL, 256 for SMPL-X.  (The one-piece graph of 4096 SMPL frames - 2.7 GB for that tensor -
        ended in an illegal memory access inside torch's own kernels, before any call into libk2b.so.)  A call of (b) is the
        backward of every block; at >= 100 ms per call it is timed over 20 calls per round, not 200.

and the joints-only route (``grad_vertices`` = None) of ``new``.  Times are device events around the calls of a round.  Every
round goes to ``profiles/lbs_backward.txt`` (``--out``)."""
import argparse
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

from keypoints2body_amd import native, synthetic  # noqa: E402

ROUNDS, CALLS, CALLS_TORCH = 5, 200, 20


def timed(fn, calls=CALLS):
    """Milliseconds per call: device events around `calls` calls."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / calls


def case(kind, B, log):
    from oracle.smpl_torch import TorchSMPL, TorchSMPLX
    if kind == "smpl":
        c = synthetic.make_body_model(0)
        p = synthetic.make_poses(B, 1)
        pose, shape = p.body_pose, p.betas
        ref = TorchSMPL(c).cuda()
    else:
        c = synthetic.make_body_model_x(0)
        p = synthetic.make_poses_x(B, 1)
        pose = np.concatenate([p.body_pose, p.jaw_pose, p.leye_pose, p.reye_pose, p.left_hand_pose, p.right_hand_pose], axis=1)
        shape = np.concatenate([p.betas, p.expression], axis=1)
        ref = TorchSMPLX(c).cuda()
    model = native.NativeModel(c.v_template, c.shapedirs, c.posedirs, c.J_regressor, c.lbs_weights, c.parents, c.extra_vertex_ids)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).cuda()
    go, pose, shape, tr = dev(p.global_orient), dev(pose), dev(shape), dev(p.transl)
    gen = torch.Generator(device="cuda").manual_seed(0)
    gj = torch.randn((B, model.num_output_joints, 3), device="cuda", generator=gen)
    gv = torch.randn((B, model.num_vertices, 3), device="cuda", generator=gen)
    model.reserve(B)

    block = 1
    while 2 * block <= B and 2 * block * model.num_vertices * model.num_joints * 4 <= 2 ** 30:
        block *= 2
    graphs = []
    for o in range(0, B, block):
        leaves = [t[o:o + block].clone().requires_grad_(True) for t in (go, pose, shape, tr)]
        joints, verts = ref._lbs(torch.cat(leaves[:2], dim=1), leaves[2], leaves[3])
        graphs.append(((gj[o:o + block] * joints).sum() + (gv[o:o + block] * verts).sum(), leaves))
    torch.cuda.synchronize()

    partners = {
        "new": lambda: model.lbs_backward(go, pose, shape, tr, gj, gv),
        "a_lbs": lambda: model.lbs(go, pose, shape, tr),
        "b_torch": lambda: [torch.autograd.grad(loss, leaves, retain_graph=True) for loss, leaves in graphs],
        "new_joints_only": lambda: model.lbs_backward(go, pose, shape, tr, gj, None),
    }
    calls = {k: CALLS_TORCH if k == "b_torch" else CALLS for k in partners}
    got = partners["new"]()
    want = [torch.cat(parts) for parts in zip(*partners["b_torch"]())]
    agree = max(float((g - w).abs().max() / w.abs().max()) for g, w in zip(got, want))
    log(f"{kind} V={model.num_vertices} B={B}: (b) in blocks of {block} frames, {CALLS_TORCH} calls per round; the others {CALLS}")
    for fn in partners.values():                          # warm-up of every shape the timed window uses
        timed(fn, 3)
    rounds = {k: [] for k in partners}
    for r in range(ROUNDS):
        for k, fn in partners.items():
            rounds[k].append(timed(fn, calls[k]))
        log(f"{kind} V={model.num_vertices} B={B} round {r}: " + " ".join(f"{k}={v[-1]:.4f}ms" for k, v in rounds.items()))
    new, a, b = rounds["new"], rounds["a_lbs"], rounds["b_torch"]
    log(f"{kind} V={model.num_vertices} B={B} summary: new slowest {max(new):.4f} ms, (b) fastest {min(b):.4f} ms -> "
        f"{'new under (b)' if max(new) < min(b) else '(b) wins'}; new / (a) = {np.median(new) / np.median(a):.1f} x (medians "
        f"{np.median(new):.4f} / {np.median(a):.4f} ms); joints-only {np.median(rounds['new_joints_only']):.4f} ms; "
        f"max relative difference to (b) {agree:.2e}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=str(REPO / "profiles" / "lbs_backward.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dev_lbs_backward_timing: no HIP device visible (a timing needs the GPU)")
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    with open(out, "w") as f:
        def log(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        log(f"# k2b_lbs_backward timing: {ROUNDS} rounds per partner, ms per call; device {torch.cuda.get_device_name()}")
        for kind, B in (("smpl", 1024), ("smpl", 4096), ("smplx", 1024)):
            case(kind, B, log)


if __name__ == "__main__":
    main()
