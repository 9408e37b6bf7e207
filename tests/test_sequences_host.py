"""Host (no GPU): the pieces of ``optimize_params_sequences`` and the eval CLI that need no device - packing of ragged
inputs, argument checks raised before anything is launched, the CLI's argument parsing - and the C ABI entries of the
ragged chains (declared, exported, their argument checks answered before any HIP call)."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

REPO = Path(__file__).resolve().parents[1]


def test_pack_ragged_concatenates_and_offsets_are_exclusive_prefix_sums():
    from keypoints2body_amd.api.sequence import pack_ragged
    seqs = [torch.full((n, 22, 3), float(i)) for i, n in enumerate((3, 0, 5, 1))]
    packed, lengths, offsets = pack_ragged(seqs)
    assert lengths.tolist() == [3, 0, 5, 1] and offsets.tolist() == [0, 3, 3, 8]
    assert lengths.dtype == np.int32 and offsets.dtype == np.int32
    assert tuple(packed.shape) == (9, 22, 3)
    for i, (o, n) in enumerate(zip(offsets, lengths)):
        assert torch.equal(packed[o:o + n], seqs[i])
    empty, l0, o0 = pack_ragged([torch.zeros((0, 22, 3))])
    assert tuple(empty.shape) == (0, 22, 3) and l0.tolist() == [0] and o0.tolist() == [0]


def test_sequence_batch_slices_by_offsets():
    from keypoints2body_amd.api.sequence import SequenceBatch
    lengths = np.array([2, 0, 3], np.int32)
    offsets = np.array([0, 2, 2], np.int32)
    n = 5
    params = {"global_orient": torch.arange(n * 3.0).reshape(n, 3), "body_pose": torch.arange(n * 69.0).reshape(n, 69),
              "betas": torch.zeros(n, 10), "transl": torch.zeros(n, 3)}
    b = SequenceBatch(params=params, joints=torch.zeros(n, 45, 3), loss=torch.arange(float(n)), lengths=lengths,
                      offsets=offsets, _result_fn=None)
    assert len(b) == 3 and b.num_frames == 5
    assert tuple(b.pose(0).shape) == (2, 72) and tuple(b.pose(1).shape) == (0, 72) and tuple(b.pose(2).shape) == (3, 72)
    assert torch.equal(b.pose(2)[:, :3], params["global_orient"][2:5])
    assert torch.equal(b.pose(2)[:, 3:], params["body_pose"][2:5])
    assert torch.equal(b.loss_of(2), torch.tensor([2.0, 3.0, 4.0]))
    with pytest.raises(IndexError):
        b.pose(3)


@pytest.mark.parametrize("bad, err", [
    ([], ValueError),                                                   # an empty list
    ("not a list", TypeError),
    ([np.zeros((2, 22, 3), np.float32)], "init"),                       # init_params of the wrong kind (see below)
])
def test_optimize_params_sequences_rejects_before_launch(bad, err):
    import keypoints2body_amd as k2b
    if err == "init":
        with pytest.raises((TypeError, ValueError)):
            k2b.optimize_params_sequences(bad, init_params=[object()], config={"use_shape_optimization": False})
        with pytest.raises(ValueError):                                 # one start per sequence
            k2b.optimize_params_sequences(bad + bad, init_params=[None], config={"use_shape_optimization": False})
        return
    with pytest.raises(err):
        k2b.optimize_params_sequences(bad)


def test_optimize_params_sequences_refuses_what_the_single_call_refuses():
    import keypoints2body_amd as k2b
    seqs = [np.zeros((2, 22, 3), np.float32)]
    with pytest.raises(NotImplementedError):
        k2b.optimize_params_sequences(seqs, config={"frame": {"input_type": "joints2d"}})
    with pytest.raises(NotImplementedError):
        k2b.optimize_params_sequences(seqs, body_model="mano")
    with pytest.raises(RuntimeError):                                   # Adam + the shape pre-pass (shape.py:10,110-113)
        k2b.optimize_params_sequences(seqs, config={"frame": {"use_lbfgs": False}, "use_shape_optimization": True})


def test_new_abi_entries_are_declared_and_exported():
    from keypoints2body_amd import native
    header = (REPO / "include" / "k2b.h").read_text()
    declared = set(re.findall(r"\b(k2b_[a-z_]+)\s*\(", header))
    for name in ("k2b_fit_sequences", "k2b_fit_sequences_lbfgs"):
        assert name in declared and name in native.EXPORTED_SYMBOLS
    lib = native.load_library()
    assert lib.k2b_version() >> 16 == 1 and (lib.k2b_version() & 0xffff) >= 3


def _abi_call(name, lengths, offsets):
    from keypoints2body_amd import native
    lib = native.load_library()
    cfg = native.default_fit_config()
    L = np.asarray(lengths, np.int32)
    O = np.asarray(offsets, np.int32)
    idx = np.arange(22, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    nul = [None] * 11                                                   # targets, conf, 4 starts, 4 outputs, loss
    if name == "k2b_fit_sequences":
        return getattr(lib, name)(None, None, C.byref(cfg), len(L), p(L), p(O), 10, 22, p(idx), *nul, None)
    return getattr(lib, name)(None, None, C.byref(cfg), len(L), p(L), p(O), 22, p(idx), *nul, 30, 10, 100, 1.0, 1e-7, 1e-9, None)


@pytest.mark.parametrize("name", ["k2b_fit_sequences", "k2b_fit_sequences_lbfgs"])
def test_abi_checks_lengths_and_offsets_before_any_hip_call(name):
    from keypoints2body_amd import native
    lib = native.load_library()
    assert _abi_call(name, [2, -1], [0, 2]) == native.K2B_ERR_INVALID_ARGUMENT
    assert b"lengths[1]" in lib.k2b_last_error()
    assert _abi_call(name, [2, 3], [0, 1]) == native.K2B_ERR_INVALID_ARGUMENT
    assert b"offsets[1]" in lib.k2b_last_error()
    assert _abi_call(name, [2, 3], [0, 2]) == native.K2B_ERR_INVALID_ARGUMENT   # consistent: now the NULL model is refused
    assert b"model" in lib.k2b_last_error()


def test_eval_cli_parses_the_reference_flags_and_the_new_ones(tmp_path):
    from keypoints2body_amd.cli.eval import parse_args
    a = parse_args(["--amass-root", str(tmp_path)])
    assert a.amass_root == tmp_path and a.limit_seqs == -1 and a.limit_frames == -1 and a.skip_start_frames == 0
    assert (a.num_shape_iters, a.num_shape_frames, a.num_body_iters_first, a.num_body_iters) == (40, 50, 100, 50)
    assert not a.fix_shape and not a.fix_foot and not a.use_adam and not a.fail_fast
    assert a.save_pred_dir is None and a.gpu_id == 0 and a.log_level == "INFO"
    assert a.batch_sequences >= 1 and a.model_dir is None and a.prior_dir is None and a.mean_file is None
    b = parse_args(["--amass-root", str(tmp_path), "--limit-seqs", "3", "--limit-frames", "20", "--skip-start-frames", "2",
                    "--num-shape-iters", "5", "--num-shape-frames", "7", "--num-body-iters-first", "9", "--num-body-iters", "4",
                    "--fix-shape", "--fix-foot", "--use-adam", "--save-pred-dir", str(tmp_path / "p"), "--fail-fast",
                    "--gpu-id", "1", "--log-level", "DEBUG", "--batch-sequences", "16", "--model-dir", str(tmp_path),
                    "--prior-dir", str(tmp_path), "--mean-file", str(tmp_path / "m.npz")])
    assert (b.limit_seqs, b.limit_frames, b.skip_start_frames, b.num_shape_iters, b.num_shape_frames) == (3, 20, 2, 5, 7)
    assert (b.num_body_iters_first, b.num_body_iters, b.gpu_id, b.log_level, b.batch_sequences) == (9, 4, 1, "DEBUG", 16)
    assert b.fix_shape and b.fix_foot and b.use_adam and b.fail_fast and b.save_pred_dir == tmp_path / "p"
    with pytest.raises(SystemExit):
        parse_args(["--amass-root", str(tmp_path), "--cpu"])            # no CPU path in this engine
    with pytest.raises(SystemExit):
        parse_args(["--amass-root", str(tmp_path), "--batch-sequences", "0"])


def test_eval_cli_configs_follow_the_reference():
    from keypoints2body_amd.cli.eval import parse_args, sequence_config
    c = sequence_config(parse_args(["--amass-root", ".", "--fix-shape", "--limit-frames", "12", "--use-adam"]))
    assert c.frame.coordinate_mode == "world" and c.frame.joints_category == "AMASS" and c.frame.use_lbfgs is False
    assert c.frame.freeze_betas is True and c.use_shape_optimization is False and c.limit_frames == 12
    assert (c.frame.num_iters_first, c.frame.num_iters_followup, c.num_shape_iters, c.num_shape_frames) == (100, 50, 40, 50)
    d = sequence_config(parse_args(["--amass-root", "."]))
    assert d.frame.use_lbfgs is True and d.use_shape_optimization is True and d.limit_frames is None and not d.fix_foot


def test_sequence_order_is_longest_first_stable_and_invertible():
    """The chain-slot order of the ragged entries (``k2b_sequence_order``, no device call): sequences with frames, longest
    first, ties in the caller's order; its inverse maps every slot back to the caller's sequence."""
    from keypoints2body_amd import native
    lengths = np.array([1, 2, 5, 17, 30, 30, 64, 0, 2], np.int32)
    order = native.sequence_order(lengths)
    live = np.flatnonzero(lengths > 0)
    want = live[np.argsort(-lengths[live], kind="stable")]
    assert order.tolist() == want.tolist() == [6, 4, 5, 3, 2, 1, 8, 0]
    inverse = np.full(len(lengths), -1)
    inverse[order] = np.arange(len(order))
    assert all(order[inverse[s]] == s for s in live) and inverse[7] == -1
    rng = np.random.default_rng(3)
    for _ in range(20):
        L = rng.integers(0, 6, int(rng.integers(1, 300))).astype(np.int32)
        live = np.flatnonzero(L > 0)
        assert native.sequence_order(L).tolist() == live[np.argsort(-L[live], kind="stable")].tolist()
    with pytest.raises(ValueError):
        native.sequence_order([2, 3], offsets=[0, 1])
    assert native.sequence_order([0, 0]).tolist() == []
