"""Host side of the landmark / surface-target feature (no GPU): smplx constant adoption, the npz loader, target index
validation, the reference's face-block indexing and the C ABI's new symbols."""
import re
import types
from pathlib import Path

import numpy as np
import pytest
import torch

from keypoints2body_amd import native, synthetic
from keypoints2body_amd.models import body_model as bm

REPO = Path(__file__).resolve().parents[1]


def _stub(with_landmarks):
    c = synthetic.make_body_model_x(0, num_extra=21)
    m = types.SimpleNamespace(v_template=torch.tensor(c.v_template), shapedirs=torch.tensor(c.shapedirs[:, :, :10]),
                              expr_dirs=torch.tensor(c.shapedirs[:, :, 10:]), num_betas=10, num_expression_coeffs=10,
                              posedirs=torch.tensor(c.posedirs), J_regressor=torch.tensor(c.J_regressor),
                              lbs_weights=torch.tensor(c.lbs_weights), parents=torch.tensor(c.parents),
                              vertex_joint_selector=types.SimpleNamespace(extra_joints_idxs=torch.tensor(c.extra_vertex_ids)))
    faces = (np.arange(3 * 200).reshape(200, 3) * 17) % c.v_template.shape[0]
    lmk_faces = (np.arange(51) * 3) % 200 if with_landmarks else None
    if with_landmarks:
        m.faces_tensor = torch.tensor(faces, dtype=torch.long)
        m.lmk_faces_idx = torch.tensor(lmk_faces, dtype=torch.long)
        m.lmk_bary_coords = torch.tensor(np.full((51, 3), 1.0 / 3.0), dtype=torch.float32)
    return m, faces, lmk_faces


def test_smplx_constants_adopts_landmarks():
    m, faces, lmk_faces = _stub(True)
    d = bm.smplx_constants(m)
    ids, bary = d["landmarks"]
    assert ids.shape == (51, 3) and ids.dtype == np.int32 and bary.shape == (51, 3) and bary.dtype == np.float32
    np.testing.assert_array_equal(ids, faces[lmk_faces])
    np.testing.assert_allclose(bary, 1.0 / 3.0)


def test_smplx_constants_without_landmarks_is_unchanged():
    m, _, _ = _stub(False)
    d = bm.smplx_constants(m)
    assert "landmarks" not in d
    assert set(d) == {"v_template", "shapedirs", "posedirs", "J_regressor", "lbs_weights", "parents", "extra_vertex_ids",
                      "model_type", "num_betas"}


def test_from_npz_reads_optional_landmark_arrays(tmp_path, monkeypatch):
    c = synthetic.make_body_model_x(0, num_extra=21)
    ids, bary = synthetic.make_landmarks(seed=3)
    path = tmp_path / "model.npz"
    np.savez(path, v_template=c.v_template, shapedirs=c.shapedirs, posedirs=c.posedirs, J_regressor=c.J_regressor,
             lbs_weights=c.lbs_weights, parents=c.parents, extra_vertex_ids=c.extra_vertex_ids, lmk_vertex_ids=ids,
             lmk_bary_coords=bary)
    seen = {}

    def fake_init(self, *args, **kw):
        seen["landmarks"] = kw.get("landmarks")

    monkeypatch.setattr(bm.BodyModel, "__init__", fake_init)
    bm.BodyModel.from_npz(str(path))
    np.testing.assert_array_equal(seen["landmarks"][0], ids)
    np.testing.assert_array_equal(seen["landmarks"][1], bary)
    np.savez(path, v_template=c.v_template, shapedirs=c.shapedirs, posedirs=c.posedirs, J_regressor=c.J_regressor,
             lbs_weights=c.lbs_weights, parents=c.parents)
    bm.BodyModel.from_npz(str(path))
    assert seen["landmarks"] is None


def test_make_landmarks_is_seeded_and_on_the_simplex():
    ids, bary = synthetic.make_landmarks(seed=0)
    ids2, bary2 = synthetic.make_landmarks(seed=0)
    assert np.array_equal(ids, ids2) and np.array_equal(bary, bary2)
    assert ids.shape == (51, 3) and ids.min() >= 0 and ids.max() < 10475
    assert (bary >= 0).all() and np.allclose(bary.sum(axis=1), 1.0, atol=1e-6)
    assert all(len(set(r)) == 3 for r in ids.tolist())


def test_out_of_range_targets_raise_value_error():
    model = types.SimpleNamespace(num_joints=55, num_landmarks=51, num_output_joints=127)
    bm.check_target_indices(model, list(range(127)))
    with pytest.raises(ValueError, match="contour"):
        bm.check_target_indices(model, [0, 127])
    with pytest.raises(ValueError):
        bm.check_target_indices(model, [-1])


def test_face_block_of_51_points_addresses_67_to_117():
    from keypoints2body_amd.core.joints.adapters import _block_indices
    idx = _block_indices("face", 51, "smplx")
    assert idx.tolist() == list(range(67, 118))


def test_header_declares_and_library_exports_the_landmark_entries():
    header = (REPO / "include" / "k2b.h").read_text()
    declared = set(re.findall(r"\b(k2b_[a-z_]+)\s*\(", header))
    new = {"k2b_model_set_landmarks", "k2b_model_num_landmarks", "k2b_surface_term"}
    assert new <= declared and new <= set(native.EXPORTED_SYMBOLS)
    lib = native.load_library()
    for name in new:
        assert hasattr(lib, name), name
    assert lib.k2b_version() >> 16 == 1 and (lib.k2b_version() & 0xffff) >= 1
