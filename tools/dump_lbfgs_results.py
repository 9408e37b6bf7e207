"""Development: save what the device L-BFGS returns (parameters, loss, gradient of ``fit_world_lbfgs`` at ``max_iter = 30``) for
a fixed set of cases as ``.npy`` files, to compare two builds of ``libk2b.so`` byte for byte - a change that is meant to leave
the existing sizes alone (another instantiation of the optimiser's header, say) must not move one bit of them.

    python tools/dump_lbfgs_results.py --out DIR [--lib PATH/libk2b.so]     # run once per build
    python tools/dump_lbfgs_results.py --compare DIR_A DIR_B                # no GPU needed

Cases: SMPL at B = 1, 300 (persistent launch), 700 (fused rounds), 1500 (two launches per round); the synthetic SMPL-H model,
B = 6; the synthetic SMPL-X model with 20 shape coefficients, B = 6 (both: the tree kernel's closure, the narrow step kernel)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np

KEYS = ("global_orient", "body_pose", "betas", "transl", "loss", "grad")


def compare(a, b):
    names = sorted(f for f in os.listdir(a) if f.endswith(".npy"))
    other = sorted(f for f in os.listdir(b) if f.endswith(".npy"))
    if names != other or not names:
        print(f"different file sets: {len(names)} in {a}, {len(other)} in {b}")
        return 1
    bad = 0
    for n in names:
        same = open(os.path.join(a, n), "rb").read() == open(os.path.join(b, n), "rb").read()
        bad += not same
        if not same:
            x, y = np.load(os.path.join(a, n)), np.load(os.path.join(b, n))
            print(f"{n}: DIFFERENT, max |a - b| = {np.abs(x - y).max():.3e}" if x.shape == y.shape else f"{n}: DIFFERENT shapes")
    print(f"{len(names)} files compared byte for byte: {len(names) - bad} equal, {bad} different")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--lib", help="another build of libk2b.so to load instead of the tree's")
    ap.add_argument("--compare", nargs=2, metavar=("DIR_A", "DIR_B"))
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    import torch
    from pathlib import Path
    from keypoints2body_amd import native, synthetic
    if args.lib:
        native._LIB_PATH = Path(args.lib).resolve()
    from tests import helpers as H
    os.makedirs(args.out, exist_ok=True)
    pr = H.native_prior()

    def save(name, out):
        for k in KEYS:
            np.save(os.path.join(args.out, f"{name}_{k}.npy"), out[k].cpu().numpy())
        print(f"{name}: loss mean {float(out['loss'].mean()):.6f}", flush=True)

    m = H.native_model()
    for B in (1, 300, 700, 1500):
        p = synthetic.make_poses(B, seed=21)
        go, bp, be, tr = map(H.cuda, (p.global_orient, p.body_pose, p.betas, p.transl))
        j3d = m.lbs(go, bp, be, tr, want_vertices=False)[0][:, :22].contiguous()
        save(f"smpl_B{B}", native.fit_world_lbfgs(m, pr, native.default_fit_config(), list(range(22)), j3d, None, go * 0.8, bp * 0.8,
                                                  be * 0.5, tr + 0.02, max_iter=30, lr=1e-2, want_grad=True))
    for name, m, J, NB in (("smplh", H.native_model_h(), 52, 10), ("smplx20", H.native_model_x(), 55, 20)):
        B, D = 6, 3 * (J - 1)
        rng = np.random.default_rng(4)
        go, pose, shape, tr = (0.2 * rng.standard_normal((B, 3)), 0.15 * rng.standard_normal((B, D)), 0.3 * rng.standard_normal((B, NB)),
                               rng.standard_normal((B, 3)))
        j3d = m.lbs(H.cuda(go), H.cuda(pose), H.cuda(shape), H.cuda(tr), want_vertices=False)[0][:, :J].contiguous()
        z = lambda c: torch.zeros(B, c, device="cuda")
        tr0 = (j3d[:, 0] - m.lbs(z(3), z(D), z(NB), None, want_vertices=False)[0][:, 0]).contiguous()
        cfg = native.default_fit_config()
        cfg.prior_pose_dims, cfg.num_betas_prior = 63, 10
        save(f"{name}_B{B}", native.fit_world_lbfgs(m, pr, cfg, list(range(J)), j3d, None, z(3), z(D), z(NB), tr0, max_iter=30, lr=1e-2,
                                                    want_grad=True))
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
