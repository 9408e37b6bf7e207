"""bench.py --dump-outputs, checked without a GPU: one float32 .npy per output array, the same frames in every array, and
beyond the size cap a seeded sample of frames that is the same from run to run."""
import numpy as np
import torch

import bench


def _outputs(frames, vertices):
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
    out = {"global_orient": r(frames, 3), "body_pose": r(frames, 69), "betas": r(frames, 10), "transl": r(frames, 3),
           "loss": r(frames)}
    return out, r(frames, 45, 3), r(frames, vertices, 3)


def test_small_output_is_written_whole(tmp_path):
    out, joints, verts = _outputs(8, 100)
    bench.dump_outputs(str(tmp_path), out, joints, verts)
    expect = dict(out, joints=joints, vertices=verts)
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted(f"{k}.npy" for k in expect)
    for k, v in expect.items():
        a = np.load(tmp_path / f"{k}.npy")
        assert a.dtype == np.float32
        np.testing.assert_array_equal(a, v.numpy())


def test_large_output_is_a_fixed_sample_under_the_cap(tmp_path):
    out, joints, verts = _outputs(4096, 6890)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), out, joints, verts)
    total = sum(p.stat().st_size for p in (tmp_path / "a").iterdir())
    assert total <= bench.DUMP_BYTES + 4096
    rows = None
    for k, v in dict(out, joints=joints, vertices=verts).items():
        a, b = np.load(tmp_path / "a" / f"{k}.npy"), np.load(tmp_path / "b" / f"{k}.npy")
        np.testing.assert_array_equal(a, b)
        assert 0 < a.shape[0] < 4096
        # every array holds the same frames, in frame order
        flat = v.reshape(4096, -1).numpy()
        idx = [int(np.flatnonzero((flat == row).all(axis=1))[0]) for row in a.reshape(a.shape[0], -1)[:16]]
        assert idx == sorted(idx)
        rows = idx if rows is None else rows
        assert idx == rows
