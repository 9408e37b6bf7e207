"""ORACLE TOOLING: the SMPL-X face-block golden, made by the REAL reference fitter (build container only).

Dict input with all four blocks - body (22), left hand (21), right hand (21) and a 51-point face - goes through the reference's
own adapter (``core/joints/adapters.py::normalize_frame_observations``), which gives the targets, their confidences and the
model joint indices (face: ``67 .. 117``, the reference's indexing).  Each frame is then fitted by the reference's
``WorldSpaceFitter.fit_frame`` with Adam (30 iterations), the way ``oracle/gen_golden_smplx.py`` drives it: the reference's
public ``optimize_params_frame`` builds its model through smplx, which is not installed here.  The ``model=`` plugin is
``TorchSMPLXLandmarks`` below: the oracle's ``TorchSMPLX`` on the synthetic SMPL-X model with the first 21 extras, plus
51 landmarks from ``synthetic.make_landmarks`` appended by smplx's ``vertices2landmarks`` formula (sum_k b_k v[ids_k] on the
untranslated mesh, translation added after) - 127 output joints, smplx's default layout.  As for the other SMPL-X goldens
the prior is the reference's own, evaluated at ``[body_pose | 0 x 6]``.  PARITY UNPINNED at the smplx boundary: smplx is not
installed here, and the landmark formula is restated.

Output: ``tests/golden/smplx_fit_face_block.npz``.   Usage:  python tools/gen_golden_face_block.py
"""
from __future__ import annotations

import os
import pickle
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

from keypoints2body_amd import synthetic  # noqa: E402
from oracle.gen_golden import GOLDEN, import_reference, sample_vertex_ids  # noqa: E402
from oracle.gen_golden_smplx import FIELDS, PaddedPrior, RecorderX  # noqa: E402
from oracle.smpl_torch import TorchSMPLX  # noqa: E402

J, E, L = 55, 21, 51
NUM_ITERS = 30
TRACE_ITERS = (1, 2, 10, 30)


class TorchSMPLXLandmarks(TorchSMPLX):
    """TorchSMPLX with smplx's static facial landmarks appended to the joints."""

    def __init__(self, consts, lmk_ids, lmk_bary):
        super().__init__(consts)
        self.lmk_ids = torch.as_tensor(np.asarray(lmk_ids), dtype=torch.long)
        self.lmk_bary = torch.as_tensor(np.asarray(lmk_bary), dtype=self.dtype)

    def forward(self, transl=None, **kw):
        out = super().forward(transl=transl, **kw)
        v = out.vertices if transl is None else out.vertices - transl[:, None, :]
        tri = v[:, self.lmk_ids.reshape(-1)].reshape(v.shape[0], -1, 3, 3)
        lmk = (tri * self.lmk_bary[None, :, :, None]).sum(dim=2)
        if transl is not None:
            lmk = lmk + transl[:, None, :]
        out.joints = torch.cat([out.joints, lmk], dim=1)
        return out


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    consts = synthetic.make_body_model_x(seed=0, num_extra=E)
    lmk_ids, lmk_bary = synthetic.make_landmarks(consts.num_vertices, J, L, seed=0)
    model = TorchSMPLXLandmarks(consts, lmk_ids, lmk_bary)
    gmm = synthetic.make_gmm(seed=0)
    scratch = tempfile.mkdtemp(prefix="k2b_goldenface_")
    os.makedirs(os.path.join(scratch, "data", "models"))
    with open(os.path.join(scratch, "data", "models", "gmm_08.pkl"), "wb") as f:
        pickle.dump({"means": gmm.means, "covars": gmm.covars, "weights": gmm.weights}, f)
    os.chdir(scratch)
    WorldSpaceFitter, _, _, _ = import_reference()
    from keypoints2body.core.joints.adapters import normalize_frame_observations  # type: ignore
    from keypoints2body.models.smpl_data import SMPLXData  # type: ignore

    B = 2
    poses = synthetic.make_poses_x(B, seed=7)
    tt = lambda a: torch.tensor(np.asarray(a))
    truth = {k: tt(getattr(poses, k)) for k in FIELDS}
    with torch.no_grad():
        gt = model(**truth).joints
    assert gt.shape[1] == J + E + L
    noisy = gt + tt(synthetic.target_noise(B, J + E + L, seed=9, scale=0.003))
    face_conf = (0.5 + synthetic.uniform(42, 51, 0)).astype(np.float32)
    blocks = []
    for i in range(B):
        n = noisy[i].numpy()
        blocks.append({"body": n[0:22], "left_hand": n[25:46], "right_hand": n[46:67],
                       "face": np.concatenate([n[67:118], face_conf[:, None]], axis=1)})
    norm = [normalize_frame_observations(b, layout=None, body_model="smplx") for b in blocks]
    j3d = torch.cat([x[0] for x in norm], dim=0).float()
    conf = norm[0][1].float()
    idx = norm[0][2]
    assert idx.tolist() == list(range(22)) + list(range(25, 118)) and norm[0][3] == "GENERIC"

    zeros = lambda c: torch.zeros(B, c)
    with torch.no_grad():
        j0 = model(global_orient=zeros(3), body_pose=zeros(63)).joints
    init = dict(global_orient=zeros(3), body_pose=zeros(63), transl=(j3d[:, 0] - j0[:, 0]).detach() + 0.01,
                left_hand_pose=zeros(45), right_hand_pose=zeros(45), expression=zeros(10), jaw_pose=zeros(3),
                leye_pose=zeros(3), reye_pose=zeros(3), betas=zeros(10))

    rec = RecorderX(model)
    fitter = WorldSpaceFitter(rec, step_size=1e-2, num_iters_first=NUM_ITERS, num_iters_followup=7, use_lbfgs=False,
                              joints_category="GENERIC", device=torch.device("cpu"))
    fitter.pose_prior = PaddedPrior(fitter.pose_prior)
    out = {k: [] for k in FIELDS + ("joints", "verts_sampled", "loss")}
    trace = {k: [[] for _ in TRACE_ITERS] for k in FIELDS}
    iter_losses = []
    for i in range(B):
        sl = slice(i, i + 1)
        rec.snaps.clear()
        losses = []
        orig = torch.Tensor.backward

        def spy(self, *a, **k):
            losses.append(float(self.detach()))
            return orig(self, *a, **k)

        torch.Tensor.backward = spy
        try:
            res = fitter.fit_frame(SMPLXData(**{k: init[k][sl] for k in FIELDS}), j3d[sl], conf_3d=conf, seq_ind=0,
                                   target_model_indices=idx, joint_loss_weight=600.0, pose_preserve_weight=5.0)
        finally:
            torch.Tensor.backward = orig
        assert len(rec.snaps) == NUM_ITERS + 1 and len(losses) == NUM_ITERS
        iter_losses.append(losses)
        for ti, t in enumerate(TRACE_ITERS):
            for k in FIELDS:
                trace[k][ti].append(rec.snaps[t][k])
        for k in FIELDS:
            out[k].append(getattr(res.params, k))
        out["joints"].append(res.joints)
        out["verts_sampled"].append(res.vertices[:, sample_vertex_ids(res.vertices.shape[1])])
        out["loss"].append(res.loss.reshape(1))
    cat = lambda xs: torch.cat(xs, dim=0).detach().numpy()
    payload = dict(case="face_block", num_iters=NUM_ITERS, seq_ind=0, freeze_betas=0,
                   model_fingerprint=np.uint64(consts.fingerprint()), num_extra=E, lmk_vertex_ids=lmk_ids, lmk_bary_coords=lmk_bary,
                   blocks_body=np.stack([b["body"] for b in blocks]), blocks_left_hand=np.stack([b["left_hand"] for b in blocks]),
                   blocks_right_hand=np.stack([b["right_hand"] for b in blocks]), blocks_face=np.stack([b["face"] for b in blocks]),
                   j3d=j3d.numpy(), conf=conf.numpy(), target_model_indices=idx.numpy(),
                   trace_iters=np.array(TRACE_ITERS), iter_losses=np.array(iter_losses),
                   sampled_vertex_ids=sample_vertex_ids(consts.num_vertices),
                   out_joints=cat(out["joints"]), out_verts_sampled=cat(out["verts_sampled"]), out_loss=cat(out["loss"]))
    for k in FIELDS:
        payload["init_" + k] = init[k].numpy()
        payload["out_" + k] = cat(out[k])
        payload["trace_" + k] = np.stack([cat(trace[k][ti]) for ti in range(len(TRACE_ITERS))])
    np.savez_compressed(GOLDEN / "smplx_fit_face_block.npz", **payload)
    print(f"[golden] smplx face_block: B={B} iters={NUM_ITERS} losses={payload['out_loss']}")


if __name__ == "__main__":
    main()
