"""Development: Adam fit with the full SMPL-X block set (body 22 + two hands of 21 + a 51-point face: 52 kinematic and 63
surface targets, 42 of them landmarks) - per iteration the tree kernel in evaluate-only mode and k2b_surface_term_kernel with
its Adam tail - against the same fit on the 52 kinematic targets alone.  Usage: python tools/dev_surface_timing.py [B ...]"""
import sys, time
from pathlib import Path
import numpy as np, torch
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from tests import helpers as H
from keypoints2body_amd import native, synthetic
J, E, L = 55, 21, 51
c = synthetic.make_body_model_x(0, num_extra=E)
model = native.NativeModel(c.v_template, c.shapedirs, c.posedirs, c.J_regressor, c.lbs_weights, c.parents, c.extra_vertex_ids,
                           landmarks=synthetic.make_landmarks(10475, J, L, seed=0))
full = list(range(22)) + list(range(25, 118))
kin = [k for k, i in enumerate(full) if i < J]
iters = 100
for B in [int(a) for a in sys.argv[1:]] or [1024, 4096]:
    p = synthetic.make_poses_x(B, seed=3)
    pose = np.concatenate([p.body_pose, p.jaw_pose, p.leye_pose, p.reye_pose, p.left_hand_pose, p.right_hand_pose], axis=1)
    shape = np.concatenate([p.betas, p.expression], axis=1)
    j, _ = model.lbs(H.cuda(p.global_orient), H.cuda(pose), H.cuda(shape), H.cuda(p.transl), want_vertices=False)
    tgt = j[:, full].contiguous()
    cfg = native.default_fit_config(); cfg.num_iters = iters; cfg.prior_pose_dims, cfg.num_betas_prior = 63, 10
    z = lambda n: torch.zeros(B, n, device="cuda")
    tr = tgt[:, 0].contiguous()
    for name, fn in (("full block set (63 surface)", lambda: native.fit_world(model, H.native_prior(), cfg, full, tgt, None, z(3), z(162), z(20), tr)),
                     ("kinematic targets only    ", lambda: native.fit_world(model, H.native_prior(), cfg, [full[k] for k in kin],
                                                                             tgt[:, kin].contiguous(), None, z(3), z(162), z(20), tr))):
        fn(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3): fn()
        torch.cuda.synchronize()
        print(f"{name}: B={B}  {(time.perf_counter() - t0) / 3 * 1e3:8.3f} ms per {iters}-iteration Adam fit", flush=True)
