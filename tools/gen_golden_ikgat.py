"""ORACLE TOOLING: the IK-GAT goldens, made by the REAL reference estimator (build container only).

The reference's public ``optimize_params_frame`` / ``optimize_params_sequence`` run with ``estimator_type="ikgat"`` on its
demo motion (``data/demo/test_motion1.npy``), so its own config checks, checkpoint loading, network
(``GATRotationRegressor``), pre- and post-processing and result objects produce the numbers.  Three third-party modules are
not installed here and are put into ``sys.modules`` before the reference is imported:

* ``torch_geometric.nn`` provides ``GATConv``, RESTATED in ``oracle/ikgat_torch.py`` from PyG's published formulation (eval
  mode, concat, self loops re-added, negative slope 0.2, no edge features).  PARITY UNPINNED at that boundary;
* ``smplx`` and ``h5py`` are empty stubs: the IK-GAT path loads neither a body model nor the mean-parameter file.

No trained weights ship with the reference: ``synthetic.make_ikgat_state`` makes seeded ones, written to a temporary
``<dir>/ikgat/<model_type>/<format>.pth``; the goldens store the generator's arguments and ``synthetic.checksum`` of the
weights, never the checkpoint.  Cases (``tests/golden/ikgat_<name>.npz``):

* ``pos``         pos_to_rot6, 22 joints (SMPL body parents), H 128 / 3 layers / 4 heads;
* ``indep``       pos-rot6, use_previous_frame_init=False: every frame starts from the same input quaternions;
* ``chain``       pos-rot6, use_previous_frame_init=True: frame t's input is frame t-1's prediction; also records how far the
                  last frame moves when frame 0's input quaternions are perturbed by 1e-6 (the reference's own sensitivity);
* ``small``       pos-rot6 through optimize_params_frame frame by frame, H 64 / 2 layers / 2 heads, 24 joints (SMPL parents;
                  joints 22 and 23 extend the demo's wrists);
* ``chainedges``  pos_to_rot6 with every parent -1 (the chain-edge graph), H 32 / 1 layer / 2 heads.

Prints the reference's per-frame CPU time at B = 1.   Usage:  python tools/gen_golden_ikgat.py [--out DIR]
(``--out``: write there instead of ``tests/golden``, to compare a regeneration with the committed files).
"""
from __future__ import annotations

import argparse
import os
import sys
import tempfile
import time
import types
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

from keypoints2body_amd import synthetic  # noqa: E402
from oracle.gen_golden import GOLDEN, REF_ROOT, import_reference  # noqa: E402
from oracle.ikgat_torch import GATConv  # noqa: E402

LIMIT = 96
FMT = "smplx"


def install_stubs():
    pyg = types.ModuleType("torch_geometric")
    pyg_nn = types.ModuleType("torch_geometric.nn")
    pyg_nn.GATConv = GATConv
    pyg.nn = pyg_nn
    sys.modules["torch_geometric"], sys.modules["torch_geometric.nn"] = pyg, pyg_nn
    sys.modules["h5py"] = types.ModuleType("h5py")
    sys.modules["smplx"] = types.ModuleType("smplx")


def write_checkpoint(root: Path, model_type: str, state: dict) -> None:
    d = root / "ikgat" / model_type
    d.mkdir(parents=True, exist_ok=True)
    torch.save({k: torch.from_numpy(v) for k, v in state.items()}, d / f"{FMT}.pth")


def unit_quats(n: int, seed: int) -> np.ndarray:
    """Seeded unit quaternions xyzw with qw >= 0.5 (moderate input rotations)."""
    q = synthetic.normalish(990, (n, 4), seed) * np.array([0.4, 0.4, 0.4, 0.0]) + np.array([0, 0, 0, 1.0])
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=Path, default=GOLDEN)
    out_dir = ap.parse_args().out.resolve()
    out_dir.mkdir(parents=True, exist_ok=True)
    torch.manual_seed(0)
    torch.set_num_threads(8)
    install_stubs()
    import_reference()
    from keypoints2body.api.frame import optimize_params_frame  # type: ignore
    from keypoints2body.api.sequence import optimize_params_sequence  # type: ignore
    from keypoints2body.models.smpl_data import SMPLData  # type: ignore

    motion = np.load(REF_ROOT.parent / "data" / "demo" / "test_motion1.npy").astype(np.float32)[:LIMIT]
    parents22 = [int(p) for p in synthetic.SMPL_PARENTS[:22]]
    parents24 = [int(p) for p in synthetic.SMPL_PARENTS[:24]]
    scratch = Path(tempfile.mkdtemp(prefix="k2b_golden_ikgat_"))
    os.chdir(scratch)

    def init(q):
        z = lambda c: torch.zeros((1, c))
        return SMPLData(betas=z(10), global_orient=z(3), body_pose=z(69), transl=None,
                        metadata={"ikgat_quaternions": q, "tag": "init"})

    def frame_cfg(model_type, parents, H, L, NH):
        return dict(estimator_type="ikgat", coordinate_mode="camera", ikgat_model_dir=str(scratch / model_type / f"h{H}"),
                    ikgat_model_format=FMT, ikgat_model_type=model_type, ikgat_parent_ids=parents, ikgat_hidden_dim=H,
                    ikgat_num_layers=L, ikgat_num_heads=NH)

    def run_seq(positions, model_type, parents, H, L, NH, seed, use_prev, q0=None):
        state = synthetic.make_ikgat_state(len(parents), 9 if model_type != "pos_to_rot6" else 3, H, L, NH, seed=seed)
        write_checkpoint(scratch / model_type / f"h{H}", model_type, state)
        cfg = {"frame": frame_cfg(model_type, parents, H, L, NH), "use_previous_frame_init": use_prev}
        t0 = time.perf_counter()
        res = optimize_params_sequence(positions, init_params=init(q0) if q0 is not None else None, body_model="smpl",
                                       config=cfg)
        dt = (time.perf_counter() - t0) / len(res)
        out = np.stack([r.params.metadata["ikgat_quaternions"] for r in res])
        return state, out, dt

    def save(name, positions, out, state, model_type, parents, H, L, NH, seed, use_prev, q0=None, **extra):
        qw = out[..., 3]
        assert qw.min() >= 0.2, f"{name}: min qw {qw.min():.3f} < 0.2"
        arrays = dict(positions=positions.astype(np.float32), quaternions=out.astype(np.float32),
                      parents=np.asarray(parents, np.int32), dims=np.array([len(parents), 9 if model_type != "pos_to_rot6" else 3,
                                                                           H, L, NH, seed], np.int64),
                      model_type=np.array(model_type), use_previous_frame_init=np.array(bool(use_prev)),
                      weights_checksum=np.array(synthetic.checksum(*state.values()), dtype=np.uint64), **extra)
        if q0 is not None:
            arrays["init_quaternions"] = q0
        np.savez_compressed(out_dir / f"ikgat_{name}.npz", **arrays)
        print(f"[ikgat] {name}: {out.shape[0]} frames, min qw {qw.min():.3f}, file {(out_dir / f'ikgat_{name}.npz').stat().st_size} B")

    q22 = unit_quats(22, seed=1)
    st, out, dt = run_seq(motion, "pos_to_rot6", parents22, 128, 3, 4, 0, True)
    save("pos", motion, out, st, "pos_to_rot6", parents22, 128, 3, 4, 0, True, cpu_ms_per_frame=np.array(1e3 * dt))
    print(f"[ikgat] reference CPU time, pos_to_rot6 H128 L3, B = 1: {1e3 * dt:.3f} ms / frame")

    st, out, dt = run_seq(motion, "pos-rot6_to_rot6", parents22, 128, 3, 4, 0, False, q22)
    save("indep", motion, out, st, "pos-rot6_to_rot6", parents22, 128, 3, 4, 0, False, q22, cpu_ms_per_frame=np.array(1e3 * dt))

    st, out, dt = run_seq(motion, "pos-rot6_to_rot6", parents22, 128, 3, 4, 0, True, q22)
    qp = q22.copy()
    qp[:, 0] += 1e-6
    _, out_p, _ = run_seq(motion, "pos-rot6_to_rot6", parents22, 128, 3, 4, 0, True, qp)
    sens = float(np.abs(out_p[-1] - out[-1]).max())
    print(f"[ikgat] chain sensitivity: last frame moves {sens:.3e} for a 1e-6 change of frame 0's input")
    save("chain", motion, out, st, "pos-rot6_to_rot6", parents22, 128, 3, 4, 0, True, q22,
         sensitivity=np.array(sens), cpu_ms_per_frame=np.array(1e3 * dt))

    # 24 joints: the demo's 22 plus two hand joints 8 cm past the wrists along the forearm
    T24 = 48
    m = motion[:T24]
    fore_l, fore_r = m[:, 20] - m[:, 18], m[:, 21] - m[:, 19]
    hands = np.stack([m[:, 20] + 0.08 * fore_l / np.linalg.norm(fore_l, axis=1, keepdims=True),
                      m[:, 21] + 0.08 * fore_r / np.linalg.norm(fore_r, axis=1, keepdims=True)], axis=1)
    m24 = np.concatenate([m, hands], axis=1).astype(np.float32)
    q24 = unit_quats(24, seed=2)
    st = synthetic.make_ikgat_state(24, 9, 64, 2, 2, seed=3)
    write_checkpoint(scratch / "pos-rot6_to_rot6" / "h64", "pos-rot6_to_rot6", st)
    cfg = frame_cfg("pos-rot6_to_rot6", parents24, 64, 2, 2)
    prev, outs = init(q24), []
    for t in range(T24):                      # the demo's loop: one optimize_params_frame per frame, metadata threaded
        res = optimize_params_frame(m24[t], prev_params=prev, body_model="smpl", config=dict(cfg))
        outs.append(res.params.metadata["ikgat_quaternions"])
        prev = res.params
    save("small", m24, np.stack(outs), st, "pos-rot6_to_rot6", parents24, 64, 2, 2, 3, True, q24)

    parents_none = [-1] * 22
    st, out, _ = run_seq(motion, "pos_to_rot6", parents_none, 32, 1, 2, 4, False)
    save("chainedges", motion, out, st, "pos_to_rot6", parents_none, 32, 1, 2, 4, False)


if __name__ == "__main__":
    main()
