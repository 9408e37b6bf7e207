"""IK-GAT estimator on the GPU (k2b_ikgat_kernel through optimize_params_frame / optimize_params_sequence).

Goldens: ``tests/golden/ikgat_*.npz``, made by the reference's own public API with PyG's GATConv restated
(``tools/gen_golden_ikgat.py``); the weights are regenerated from the recorded seed and checked by checksum."""
from __future__ import annotations

import os
from pathlib import Path

import numpy as np
import pytest
import torch

from keypoints2body_amd import optimize_params_frame, optimize_params_sequence, synthetic
from keypoints2body_amd.core.estimators import ikgat
from keypoints2body_amd.models.smpl_data import SMPLData

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"
TOL = 1e-4


def _golden(name):
    with np.load(GOLDEN / f"ikgat_{name}.npz") as z:
        g = {k: z[k] for k in z.files}
    g["J"], g["IN"], g["H"], g["L"], g["NH"], g["seed"] = (int(v) for v in g["dims"])
    g["model_type"] = str(g["model_type"])
    return g


def _checkpoint(root: Path, g, fmt="smplx", legacy=False) -> Path:
    st = synthetic.make_ikgat_state(g["J"], g["IN"], g["H"], g["L"], g["NH"], seed=g["seed"])
    assert synthetic.checksum(*st.values()) == int(g["weights_checksum"])
    if legacy:
        st = synthetic.make_ikgat_state(g["J"], g["IN"], g["H"], g["L"], g["NH"], seed=g["seed"], legacy_pyg=True)
    d = root / "ikgat" / g["model_type"]
    d.mkdir(parents=True, exist_ok=True)
    torch.save({k: torch.from_numpy(v) for k, v in st.items()}, d / f"{fmt}.pth")
    return d / f"{fmt}.pth"


def _frame_cfg(root, g, **kw):
    c = dict(estimator_type="ikgat", coordinate_mode="camera", ikgat_model_dir=str(root), ikgat_model_format="smplx",
             ikgat_model_type=g["model_type"], ikgat_parent_ids=[int(p) for p in g["parents"]], ikgat_hidden_dim=g["H"],
             ikgat_num_layers=g["L"], ikgat_num_heads=g["NH"])
    c.update(kw)
    return c


def _init(q=None, transl=None):
    z = lambda c: torch.zeros((1, c))
    meta = {"tag": "init"}
    if q is not None:
        meta["ikgat_quaternions"] = q
    return SMPLData(betas=z(10), global_orient=z(3), body_pose=z(69), transl=transl, metadata=meta)


def _sequence(tmp_path, g, **seq):
    _checkpoint(tmp_path, g)
    cfg = {"frame": _frame_cfg(tmp_path, g), "use_previous_frame_init": bool(g["use_previous_frame_init"])}
    cfg.update(seq)
    q0 = g.get("init_quaternions")
    return optimize_params_sequence(g["positions"], init_params=_init(q0) if q0 is not None else None, body_model="smpl",
                                    config=cfg)


@pytest.fixture(autouse=True)
def _fresh_cache():
    ikgat.clear_cache()
    yield
    ikgat.clear_cache()


@pytest.mark.parametrize("name", ["pos", "indep", "chain", "chainedges"])
def test_sequence_matches_reference(tmp_path, name):
    g = _golden(name)
    res = _sequence(tmp_path, g)
    got = np.stack([r.params.metadata["ikgat_quaternions"] for r in res])
    assert got.shape == g["quaternions"].shape
    assert np.abs(got - g["quaternions"]).max() < TOL


def test_frame_loop_matches_reference_second_shape(tmp_path):
    g = _golden("small")
    _checkpoint(tmp_path, g)
    prev, outs = _init(g["init_quaternions"]), []
    for t in range(g["positions"].shape[0]):
        res = optimize_params_frame(g["positions"][t], prev_params=prev, body_model="smpl", config=_frame_cfg(tmp_path, g))
        outs.append(res.params.metadata["ikgat_quaternions"])
        prev = res.params
    assert np.abs(np.stack(outs) - g["quaternions"]).max() < TOL


def test_frame_matches_reference_and_older_pyg_spelling(tmp_path):
    g = _golden("pos")
    for legacy in (False, True):
        ikgat.clear_cache()
        _checkpoint(tmp_path, g, legacy=legacy)
        for t in (0, 17, 95):
            res = optimize_params_frame(g["positions"][t], body_model="smpl", config=_frame_cfg(tmp_path, g))
            assert np.abs(res.params.metadata["ikgat_quaternions"] - g["quaternions"][t]).max() < TOL


def test_chain_is_bitwise_the_frame_loop_and_tracks_reference(tmp_path):
    g = _golden("chain")
    chain = np.stack([r.params.metadata["ikgat_quaternions"] for r in _sequence(tmp_path, g)])
    prev, loop = _init(g["init_quaternions"]), []
    for t in range(g["positions"].shape[0]):
        res = optimize_params_frame(g["positions"][t], prev_params=prev, body_model="smpl", config=_frame_cfg(tmp_path, g))
        loop.append(res.params.metadata["ikgat_quaternions"])
        prev = res.params
    assert np.array_equal(chain, np.stack(loop))
    # teacher forcing: the reference's frame t-1 as frame t's input, all frames in one batched launch
    est = ikgat.IKGATEstimator(ikgat_cfg(tmp_path, g))
    gold = g["quaternions"]
    q_in = np.concatenate([g["init_quaternions"][None], gold[:-1]]).astype(np.float32)
    pos = torch.as_tensor(g["positions"], device=est.device)
    forced = est.predict_frames(pos, torch.as_tensor(q_in, device=est.device)).cpu().numpy()
    assert np.abs(forced - gold).max() < TOL
    # free running: the last frame within the reference's own sensitivity to last-bit input changes
    assert np.abs(chain[-1] - gold[-1]).max() < max(TOL, 10 * float(g["sensitivity"]))


def ikgat_cfg(root, g):
    from keypoints2body_amd.core.config import FrameOptimizeConfig
    return FrameOptimizeConfig(**_frame_cfg(root, g))


@pytest.mark.parametrize("name", ["pos", "chain"])
def test_batch_invariance(tmp_path, name):
    g = _golden(name)
    _checkpoint(tmp_path, g)
    est = ikgat.IKGATEstimator(ikgat_cfg(tmp_path, g))
    dev, J, T = est.device, g["J"], g["positions"].shape[0]
    B = 4096
    rng = np.random.default_rng(0)
    slots = np.sort(rng.choice(B, size=T, replace=False))
    pos = g["positions"][rng.integers(0, T, size=B)].astype(np.float32)
    pos += rng.normal(0, 0.02, size=pos.shape).astype(np.float32)
    pos[slots] = g["positions"]
    q_one = g.get("init_quaternions")
    q = None
    if q_one is not None:
        q = g["quaternions"][rng.integers(0, T, size=B)].astype(np.float32)
        q[slots] = np.concatenate([q_one[None], g["quaternions"][:-1]])
        q = torch.as_tensor(q, device=dev)
    big = est.predict_frames(torch.as_tensor(pos, device=dev), q).cpu().numpy()
    for i, s in enumerate(slots):
        one = est.predict_frames(torch.as_tensor(pos[s: s + 1], device=dev),
                                 q[s: s + 1].contiguous() if q is not None else None).cpu().numpy()
        assert np.array_equal(big[s], one[0]), (i, s)


def test_result_objects(tmp_path):
    g = _golden("indep")
    _checkpoint(tmp_path, g)
    init = _init(g["init_quaternions"], transl=torch.tensor([[0.1, 0.2, 0.3]]))
    init.betas = torch.full((1, 10), 0.5)
    res = optimize_params_frame(g["positions"][3], prev_params=init, body_model="smpl", config=_frame_cfg(tmp_path, g))
    p = res.params
    assert isinstance(p, SMPLData) and p is not init
    for k in ("betas", "global_orient", "body_pose", "transl"):
        assert torch.equal(getattr(p, k).cpu(), getattr(init, k))
    assert p.metadata is not init.metadata and init.metadata["ikgat_quaternions"] is g["init_quaternions"]
    assert set(p.metadata) == {"tag", "ikgat_quaternions"} and p.metadata["tag"] == "init"
    q = p.metadata["ikgat_quaternions"]
    assert isinstance(q, np.ndarray) and q.dtype == np.float32 and q.shape == (22, 4)
    frame = torch.as_tensor(g["positions"][3])[None]
    assert torch.equal(res.joints.cpu(), frame) and torch.equal(res.vertices.cpu(), frame) and res.loss is None

    # sequence: every result's params are the init, frame 0's transl included (world mode, no init given)
    res = optimize_params_sequence(g["positions"][:5], init_params=_init(g["init_quaternions"]), body_model="smpl",
                                   config={"frame": _frame_cfg(tmp_path, g, coordinate_mode="camera"),
                                           "use_previous_frame_init": True})
    assert len(res) == 5 and all(r.params.transl is None and r.loss is None for r in res)
    gp = _golden("pos")
    _checkpoint(tmp_path, gp)
    res = optimize_params_sequence(gp["positions"][:4], body_model="smpl",
                                   config={"frame": _frame_cfg(tmp_path, gp, coordinate_mode="world")})
    root0 = torch.as_tensor(gp["positions"][0, 0])
    assert all(torch.equal(r.params.transl.cpu()[0], root0) for r in res)
    assert all(torch.equal(r.joints.cpu()[0], torch.as_tensor(gp["positions"][t])) for t, r in enumerate(res))


def test_refusals(tmp_path):
    g = _golden("indep")
    _checkpoint(tmp_path, g)
    with pytest.raises(ValueError, match="ikgat_quaternions"):
        optimize_params_frame(g["positions"][0], body_model="smpl", config=_frame_cfg(tmp_path, g))
    with pytest.raises(ValueError, match="ikgat_quaternions"):
        optimize_params_sequence(g["positions"][:3], body_model="smpl", config={"frame": _frame_cfg(tmp_path, g)})
    # joint count != len(parent_ids): refused before any launch
    bad = np.concatenate([g["positions"][0], g["positions"][0, :2]])
    with pytest.raises(ValueError, match="joints"):
        optimize_params_frame(bad, prev_params=_init(g["init_quaternions"]), body_model="smpl",
                              config=_frame_cfg(tmp_path, g))
    # the reference's type check: an SMPLData start with body_model="smplx" (the demo's second call)
    with pytest.raises(ValueError, match="SMPLXData"):
        optimize_params_frame(g["positions"][0], prev_params=_init(g["init_quaternions"]), body_model="smplx",
                              config=_frame_cfg(tmp_path, g))
    # world mode, no transl and no model to derive it from
    with pytest.raises(ValueError, match="transl"):
        optimize_params_frame(g["positions"][0], prev_params=_init(g["init_quaternions"]), body_model="smpl",
                              config=_frame_cfg(tmp_path, g, coordinate_mode="world"))
    # MANO / FLAME stay refused with IK-GAT too
    with pytest.raises(NotImplementedError):
        optimize_params_frame(g["positions"][0], body_model="mano", config=_frame_cfg(tmp_path, g))
    # an unsupported hidden width: refused at create, no launch
    root = tmp_path / "h72"
    st = synthetic.make_ikgat_state(22, 9, 72, 1, 4, seed=0)
    (root / "ikgat" / g["model_type"]).mkdir(parents=True)
    torch.save({k: torch.from_numpy(v) for k, v in st.items()}, root / "ikgat" / g["model_type"] / "smplx.pth")
    with pytest.raises(NotImplementedError, match="k2b_ikgat_create.*hidden_dim=72"):
        optimize_params_frame(g["positions"][0], prev_params=_init(g["init_quaternions"]), body_model="smpl",
                              config=_frame_cfg(root, g, ikgat_hidden_dim=72, ikgat_num_layers=1))


def test_checkpoint_read_once_per_file_state(tmp_path, monkeypatch):
    g = _golden("pos")
    path = _checkpoint(tmp_path, g)
    reads = []
    real = ikgat.read_checkpoint
    monkeypatch.setattr(ikgat, "read_checkpoint", lambda p: (reads.append(p), real(p))[1])
    a = optimize_params_frame(g["positions"][0], body_model="smpl", config=_frame_cfg(tmp_path, g))
    b = optimize_params_frame(g["positions"][1], body_model="smpl", config=_frame_cfg(tmp_path, g))
    assert len(reads) == 1
    st = os.stat(path)
    os.utime(path, ns=(st.st_atime_ns, st.st_mtime_ns + 2_000_000_000))
    c = optimize_params_frame(g["positions"][0], body_model="smpl", config=_frame_cfg(tmp_path, g))
    assert len(reads) == 2
    assert np.array_equal(a.params.metadata["ikgat_quaternions"], c.params.metadata["ikgat_quaternions"])
    assert not np.array_equal(a.params.metadata["ikgat_quaternions"], b.params.metadata["ikgat_quaternions"])
