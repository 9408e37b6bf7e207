"""Development: the PROJECTED form of the surface term against its 3D form, on the pattern of tools/dev_surface_timing.py - a
100-iteration Adam fit with the full SMPL-X block set (52 kinematic and 63 surface targets), the same selection once through
k2b_fit_image (2D targets: the body's projection from 3 m at f = 500 px) and once through k2b_fit_world (3D targets), interleaved
on one build and one device.  Kernel times: run this under ``rocprofv3 --kernel-trace --stats`` in a run of its own.
Usage: python tools/dev_surface_image_timing.py [B ...]"""
import sys, time
from pathlib import Path
import numpy as np, torch
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from tests import helpers as H
from keypoints2body_amd import native, synthetic
J, E, L = 55, 21, 51
FOCAL, DEPTH = 500.0, 3.0
c = synthetic.make_body_model_x(0, num_extra=E)
model = native.NativeModel(c.v_template, c.shapedirs, c.posedirs, c.J_regressor, c.lbs_weights, c.parents, c.extra_vertex_ids,
                           landmarks=synthetic.make_landmarks(10475, J, L, seed=0))
full = list(range(22)) + list(range(25, 118))
iters, rounds = 100, 4
for B in [int(a) for a in sys.argv[1:]] or [1024]:
    p = synthetic.make_poses_x(B, seed=3)
    pose = np.concatenate([p.body_pose, p.jaw_pose, p.leye_pose, p.reye_pose, p.left_hand_pose, p.right_hand_pose], axis=1)
    shape = np.concatenate([p.betas, p.expression], axis=1)
    transl = p.transl.copy()
    transl[:, 2] += DEPTH
    j, _ = model.lbs(H.cuda(p.global_orient), H.cuda(pose), H.cuda(shape), H.cuda(transl), want_vertices=False)
    tgt3 = j[:, full].contiguous()
    tgt2 = torch.cat([FOCAL * tgt3[..., :2] / tgt3[..., 2:3], torch.zeros_like(tgt3[..., :1])], dim=-1).contiguous()
    cfg3 = native.default_fit_config(); cfg3.num_iters = iters; cfg3.prior_pose_dims, cfg3.num_betas_prior = 63, 10
    cfg2 = native.default_fit_config(); cfg2.num_iters = iters; cfg2.prior_pose_dims, cfg2.num_betas_prior = 63, 10
    cfg2.projection, cfg2.focal[0], cfg2.focal[1], cfg2.sigma, cfg2.joint_loss_weight = 1, FOCAL, FOCAL, 100.0, 1.0
    z = lambda n: torch.zeros(B, n, device="cuda")
    tr = tgt3[:, 0].contiguous()
    forms = (("projected (k2b_fit_image)", lambda: native.fit_image(model, H.native_prior(), cfg2, full, tgt2, None, z(3), z(162), z(20), tr)),
             ("3D        (k2b_fit_world)", lambda: native.fit_world(model, H.native_prior(), cfg3, full, tgt3, None, z(3), z(162), z(20), tr)))
    for _, fn in forms:
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in forms}
    for _ in range(rounds):                                   # interleaved: a drift of the device's clocks hits both forms alike
        for name, fn in forms:
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    for name, t in times.items():
        print(f"{name}: B={B}  median {np.median(t):8.3f} ms  (min {min(t):.3f}, max {max(t):.3f}) per {iters}-iteration Adam fit, 63 surface targets", flush=True)
