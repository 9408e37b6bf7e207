"""The calls that the ten fit entries of the C ABI refuse, as data: one row per bad call.  ``tools/record_fit_refusals.py`` ran this
table through the real entries at the commit before ``csrc/k2b_fit_rules.h`` existed and wrote every code and message to
``tests/golden/fit_refusals.json``; ``tests/test_gpu_fit_refusals.py`` holds the entries to that recording and
``tests/test_fit_rules_host.py`` holds the rules alone to it, with the facts of the handles written out as integers.

A row is ``(id, entry, model, cfg overrides, call fields)``.  ``model``: a key of MODELS, or None for a NULL model handle; the prior
is the 69-wide synthetic mixture unless the call says ``prior=False`` (NULL handle); ``cfg=None`` is a NULL configuration.  Call
fields not named take the defaults of DEFAULTS.  Rows wrong in two ways at once pin the order of the checks."""
import numpy as np

from keypoints2body_amd import synthetic

ENTRIES = ("fit_world", "fit_sequence", "fit_sequences", "fit_image", "fit_image_sequences", "fit_multiview", "fit_world_lbfgs",
           "fit_sequence_lbfgs", "fit_sequences_lbfgs", "shape_pass_lbfgs")

CHAIN24_PARENTS = np.arange(-1, 23, dtype=np.int32)          # one 24-joint chain: depth 23, beyond both fit kernels

# how to make every model, and the facts the rules read from its handle (csrc/k2b_fit_rules.h, Facts)
MODELS = {
    "smpl": dict(make=lambda: synthetic.make_body_model(0), parents=synthetic.SMPL_PARENTS, E=21, L=0, NB=10, fit_ok=1, scan64=0),
    "smpl_scan64": dict(make=lambda: synthetic.make_body_model(0), parents=synthetic.SMPL_PARENTS, E=21, L=0, NB=10, fit_ok=1, scan64=1,
                        env={"K2B_FIT_SCAN64": "1"}),
    "smplx": dict(make=lambda: synthetic.make_body_model_x(0), parents=synthetic.SMPLX_PARENTS, E=72, L=0, NB=20, fit_ok=0, scan64=1),
    "smplx_lmk": dict(make=lambda: synthetic.make_body_model_x(0), parents=synthetic.SMPLX_PARENTS, E=72, L=51, NB=20, fit_ok=0, scan64=1,
                      landmarks=lambda: synthetic.make_landmarks()),
    "chain24": dict(make=lambda: synthetic.make_body_model(0, parents=CHAIN24_PARENTS.copy()), parents=CHAIN24_PARENTS, E=21, L=0, NB=10,
                    fit_ok=0, scan64=1),
}
PRIOR = dict(D=69, M=8)


def depths(parents):
    d = [0] * len(parents)
    for j in range(1, len(parents)):
        d[j] = d[int(parents[j])] + 1
    return d


PARAM_BUFFERS = ("j3d", "go_in", "bp_in", "be_in", "tr_in", "go_out", "bp_out", "be_out", "tr_out")
SHAPE_BUFFERS = ("seq_offsets", "betas_in", "betas_out", "j3d", "global_orient", "body_pose", "root_targets")
IDENTITY = ((1, 0, 0, 0, 1, 0, 0, 0, 1), (0, 0, 3), (500, 430))

DEFAULTS = dict(
    prior=True,
    B=2, K=None, idx=(0, 1),                 # K: len(idx) unless given; idx None: NULL
    null=(),                                 # names of PARAM_BUFFERS (shape pass: SHAPE_BUFFERS) passed as NULL
    preserve=False, tr_prior=False, grad_out=False,
    S=1, T=2, followup=5,                    # k2b_fit_sequence: S sequences of T frames
    lengths=(2,), offsets="prefix",          # ragged entries; lengths None: both NULL; offsets "prefix": the exclusive prefix sums
    max_iter=30, history=100, lr=1.0,        # L-BFGS (max_iter is first_iters in the chain entries)
    views=1, cameras="identity",             # "identity": `views` good cameras; None: NULL; else a list of (rotation, translation, focal)
    N=2, root_joint=0, free_betas=10,        # shape pass: S sequences over N frames
)

X63 = dict(prior_pose_dims=63)               # SMPL-X (and SMPL on the tree kernel): the prior over the first 63 pose dimensions
P1 = dict(projection=1, focal=(500.0, 430.0))
NAN, INF = float("nan"), float("inf")
SURF129 = (0,) + tuple(55 + i % 123 for i in range(129))


def _cams(n, **bad):
    """n identity cameras with one field of the last replaced: rotation=(slot, value) ..."""
    rows = [[list(IDENTITY[0]), list(IDENTITY[1]), list(IDENTITY[2])] for _ in range(n)]
    for field, (slot, value) in bad.items():
        rows[-1][("rotation", "translation", "focal").index(field)][slot] = value
    return rows


def _c(id, entry, model, cfg=(), **call):
    return dict(id=id, entry=entry, model=model, cfg=None if cfg is None else dict(cfg), call=call)


def _join(*ds):
    out = {}
    for d in ds:
        out.update(d)
    return out


CASES = [
    # ---- k2b_fit_world: the shared path ---------------------------------------------------------------------------------------
    _c("w_null_model", "fit_world", None),
    _c("w_null_prior", "fit_world", "smpl", prior=False),
    _c("w_null_cfg", "fit_world", "smpl", None),
    _c("w_proj2", "fit_world", "smpl", dict(projection=2)),
    _c("w_focal_nan", "fit_world", "smpl", dict(projection=1, focal=(NAN, 500.0))),
    _c("w_focal_inf", "fit_world", "smpl", dict(projection=1, focal=(500.0, INF))),
    _c("w_focal_and_idx", "fit_world", "smpl", dict(projection=1, focal=(0.0, 500.0)), idx=(0, 99)),
    _c("w_B_neg", "fit_world", "smpl", B=-1),
    _c("w_K0", "fit_world", "smpl", idx=()),
    _c("w_B0_K0", "fit_world", "smpl", B=0, idx=()),
    _c("w_K_big", "fit_world", "smpl", idx=tuple(i % 24 for i in range(46))),
    _c("w_idx_null", "fit_world", "smpl", idx=None, K=2),
    _c("w_iters0", "fit_world", "smpl", dict(num_iters=0)),
    _c("w_iters_big", "fit_world", "smpl", dict(num_iters=(1 << 20) + 1)),
    _c("w_null_and_iters", "fit_world", "smpl", dict(num_iters=0), null=("j3d",)),
    _c("w_beta1", "fit_world", "smpl", dict(adam_beta1=1.0)),
    _c("w_beta2", "fit_world", "smpl", dict(adam_beta2=-0.5)),
    _c("w_step_nan", "fit_world", "smpl", dict(step_size=NAN)),
    _c("w_eps0", "fit_world", "smpl", dict(adam_eps=0.0)),
    _c("w_eps_denormal", "fit_world", "smpl", dict(adam_eps=1e-40)),
    _c("w_B0_eps0", "fit_world", "smpl", dict(adam_eps=0.0), B=0),
    _c("w_null_j3d", "fit_world", "smpl", null=("j3d",)),
    _c("w_null_out", "fit_world", "smpl", null=("tr_out",)),
    _c("w_idx_range", "fit_world", "smpl", idx=(0, 45)),
    _c("w_idx_neg", "fit_world", "smpl", idx=(-1, 0)),
    _c("w_dup", "fit_world", "smpl", idx=(3, 3)),
    _c("w_dup_and_angle", "fit_world", "smpl", dict(angle_prior_index=(64, 55, 9, 12)), idx=(3, 3)),
    _c("w_dup_then_range", "fit_world", "smpl", idx=(3, 3, 99)),
    _c("w_angle", "fit_world", "smpl", dict(angle_prior_index=(52, 55, 9, 64))),
    _c("w_angle_neg", "fit_world", "smpl", dict(angle_prior_index=(-1, 55, 9, 12))),
    _c("w_debug_shape", "fit_world", "smpl", dict(debug_launch_shape=5)),
    _c("w_angle_and_debug", "fit_world", "smpl", dict(angle_prior_index=(52, 55, 9, 64), debug_launch_shape=5)),
    _c("w_surface_only", "fit_world", "smpl", idx=(24, 25)),
    _c("w_proj_surface", "fit_world", "smpl", P1, idx=(0, 24)),
    _c("w_badproj_and_surface", "fit_world", "smpl", dict(projection=2), idx=(0, 24)),
    _c("w_scan64_proj", "fit_world", "smpl_scan64", P1),
    _c("w_scan64_proj_dup", "fit_world", "smpl_scan64", P1, idx=(3, 3)),
    _c("w_scan64_proj_angle", "fit_world", "smpl_scan64", _join(P1, dict(angle_prior_index=(64, 55, 9, 12)))),
    _c("w_nbp_tree_dims", "fit_world", "smpl", dict(num_betas_prior=5)),
    _c("w_tree_dims62", "fit_world", "smpl", dict(prior_pose_dims=62)),
    _c("w_tree_dims66", "fit_world", "smpl", dict(prior_pose_dims=66)),
    _c("w_tree_dims72", "fit_world", "smpl", dict(prior_pose_dims=72)),
    _c("w_tree_x_default_dims", "fit_world", "smplx"),
    _c("w_tree_transl_w", "fit_world", "smpl", _join(X63, dict(transl_prior_weight=1.0))),
    _c("w_tree_transl_ptr", "fit_world", "smplx", X63, tr_prior=True),
    _c("w_tree_transl_and_B_neg", "fit_world", "smplx", _join(X63, dict(transl_prior_weight=1.0)), B=-1),
    _c("w_tree_dims_and_transl", "fit_world", "smplx", dict(transl_prior_weight=1.0)),
    _c("w_tree_B_neg", "fit_world", "smplx", X63, B=-1),
    _c("w_tree_iters0", "fit_world", "smplx", _join(X63, dict(num_iters=0))),
    _c("w_tree_null", "fit_world", "smplx", X63, null=("be_in",)),
    _c("w_tree_angle", "fit_world", "smpl", _join(X63, dict(angle_prior_index=(63, 55, 9, 12)))),
    _c("w_tree_dup", "fit_world", "smplx", X63, idx=(40, 40)),
    _c("w_tree_dup_and_angle", "fit_world", "smplx", _join(X63, dict(angle_prior_index=(52, 63, 9, 12))), idx=(40, 40)),
    _c("w_tree_debug", "fit_world", "smplx", _join(X63, dict(debug_launch_shape=-1))),
    _c("w_tree_surface_only", "fit_world", "smplx", X63, idx=(55, 56)),
    _c("w_tree_proj_surface", "fit_world", "smplx", _join(X63, P1), idx=(0, 55)),
    _c("w_tree_proj_surface_and_angle", "fit_world", "smplx", _join(X63, P1, dict(angle_prior_index=(63, 55, 9, 12))), idx=(0, 55)),
    _c("w_tree_more128", "fit_world", "smplx_lmk", X63, idx=SURF129),
    _c("w_tree_idx_range", "fit_world", "smplx", X63, idx=(0, 127)),
    _c("w_tree_lmk_idx_range", "fit_world", "smplx_lmk", X63, idx=(0, 178)),
    _c("w_tree_depth", "fit_world", "chain24", X63, idx=(0, 23)),
    _c("w_tree_depth_and_debug", "fit_world", "chain24", _join(X63, dict(debug_launch_shape=9)), idx=(0, 16)),
    _c("w_tree_angle_and_depth", "fit_world", "chain24", _join(X63, dict(angle_prior_index=(63, 55, 9, 12))), idx=(0, 23)),
    # ---- k2b_fit_sequence -------------------------------------------------------------------------------------------------------
    _c("s_proj", "fit_sequence", "smpl", P1),
    _c("s_T0", "fit_sequence", "smpl", T=0),
    _c("s_proj_and_T0", "fit_sequence", "smpl", dict(projection=2), T=0),
    _c("s_frames", "fit_sequence", "smpl", S=65536, T=32768),
    _c("s_followup0", "fit_sequence", "smpl", followup=0),
    _c("s_followup_big", "fit_sequence", "smpl", followup=(1 << 20) + 1),
    _c("s_chain_and_transl", "fit_sequence", "smpl", dict(transl_prior_weight=1.0)),
    _c("s_followup_and_transl", "fit_sequence", "smpl", dict(transl_prior_weight=1.0), followup=0),
    _c("s_null_model", "fit_sequence", None),
    _c("s_null_cfg", "fit_sequence", "smpl", None),
    _c("s_S_neg", "fit_sequence", "smpl", S=-1),
    _c("s_surface_in_chain", "fit_sequence", "smpl", idx=(0, 24)),
    _c("s_T1_surface_only", "fit_sequence", "smpl", T=1, idx=(24,)),
    _c("s_surface_only_chain", "fit_sequence", "smpl", idx=(24, 25)),
    _c("s_tree_surface_in_chain", "fit_sequence", "smplx", X63, idx=(0, 55)),
    _c("s_dup", "fit_sequence", "smpl", idx=(3, 3)),
    _c("s_T1_transl_tree", "fit_sequence", "smplx", _join(X63, dict(transl_prior_weight=1.0)), T=1),
    _c("s_null", "fit_sequence", "smpl", null=("go_out",)),
    # ---- k2b_fit_sequences ------------------------------------------------------------------------------------------------------
    _c("q_S_neg", "fit_sequences", "smpl", lengths=(), S=-1),
    _c("q_null_lengths", "fit_sequences", "smpl", lengths=None, S=1),
    _c("q_len_neg", "fit_sequences", "smpl", lengths=(-1,)),
    _c("q_offsets", "fit_sequences", "smpl", lengths=(2, 2), offsets=(0, 3)),
    _c("q_2_30", "fit_sequences", "smpl", lengths=(1 << 30, 1), offsets=(0, 1 << 30)),
    _c("q_null_model", "fit_sequences", None),
    _c("q_ragged_and_null_model", "fit_sequences", None, lengths=(2, 2), offsets=(1, 3)),
    _c("q_null_cfg", "fit_sequences", "smpl", None),
    _c("q_proj", "fit_sequences", "smpl", P1),
    _c("q_proj_and_followup", "fit_sequences", "smpl", P1, followup=0),
    _c("q_followup", "fit_sequences", "smpl", followup=0),
    _c("q_iters", "fit_sequences", "smpl", dict(num_iters=0)),
    _c("q_followup_and_iters", "fit_sequences", "smpl", dict(num_iters=0), followup=-3),
    _c("q_transl", "fit_sequences", "smpl", dict(transl_prior_weight=1.0)),
    _c("q_K0", "fit_sequences", "smpl", idx=()),
    _c("q_idx_null", "fit_sequences", "smpl", idx=None, K=2),
    _c("q_idx_range", "fit_sequences", "smpl", idx=(0, 45)),
    _c("q_transl_and_idx", "fit_sequences", "smpl", dict(transl_prior_weight=1.0), idx=(0, 45)),
    _c("q_empty_idx_range", "fit_sequences", "smpl", lengths=(0,), idx=(0, 45)),
    _c("q_null_buf", "fit_sequences", "smpl", null=("go_in",)),
    _c("q_surface", "fit_sequences", "smpl", idx=(0, 24)),
    _c("q_null_and_surface", "fit_sequences", "smpl", idx=(0, 24), null=("j3d",)),
    _c("q_dup", "fit_sequences", "smpl", idx=(3, 3)),
    _c("q_adam", "fit_sequences", "smpl", dict(adam_beta2=1.5)),
    _c("q_angle", "fit_sequences", "smpl", dict(angle_prior_index=(52, 55, 9, 64))),
    _c("q_tree_default_dims", "fit_sequences", "smplx"),
    _c("q_tree_dup", "fit_sequences", "smplx", X63, idx=(30, 30), lengths=(1, 1)),
    # ---- k2b_fit_image_sequences ------------------------------------------------------------------------------------------------
    _c("iq_S_neg", "fit_image_sequences", "smpl", P1, lengths=(), S=-1),
    _c("iq_offsets", "fit_image_sequences", "smpl", P1, lengths=(1, 1), offsets=(0, 0)),
    _c("iq_null_model", "fit_image_sequences", None, P1),
    _c("iq_proj0", "fit_image_sequences", "smpl"),
    _c("iq_proj0_and_surface", "fit_image_sequences", "smpl", idx=(0, 24)),
    _c("iq_focal", "fit_image_sequences", "smpl", dict(projection=1, focal=(500.0, -1.0))),
    _c("iq_focal_and_idx", "fit_image_sequences", "smpl", dict(projection=1, focal=(500.0, NAN)), idx=(0, 45)),
    _c("iq_followup", "fit_image_sequences", "smpl", P1, followup=0),
    _c("iq_iters", "fit_image_sequences", "smpl", _join(P1, dict(num_iters=-1))),
    _c("iq_transl", "fit_image_sequences", "smpl", _join(P1, dict(transl_prior_weight=0.5))),
    _c("iq_K0", "fit_image_sequences", "smpl", P1, idx=()),
    _c("iq_idx_range", "fit_image_sequences", "smpl", P1, idx=(0, 45)),
    _c("iq_surface", "fit_image_sequences", "smpl", P1, idx=(0, 24)),
    _c("iq_surface_and_null", "fit_image_sequences", "smpl", P1, idx=(0, 24), null=("tr_in",)),
    _c("iq_scan64", "fit_image_sequences", "smpl_scan64", P1),
    _c("iq_empty_scan64", "fit_image_sequences", "smpl_scan64", P1, lengths=(0,)),
    _c("iq_scan64_and_null", "fit_image_sequences", "smpl_scan64", P1, null=("j3d",)),
    _c("iq_null_buf", "fit_image_sequences", "smpl", P1, null=("be_out",)),
    _c("iq_dup", "fit_image_sequences", "smpl", P1, idx=(3, 3)),
    _c("iq_tree_dup", "fit_image_sequences", "smplx", _join(P1, X63), idx=(3, 3)),
    _c("iq_debug", "fit_image_sequences", "smpl", _join(P1, dict(debug_launch_shape=7))),
    # ---- k2b_fit_image ----------------------------------------------------------------------------------------------------------
    _c("i_null_model", "fit_image", None, P1),
    _c("i_null_cfg", "fit_image", "smpl", None),
    _c("i_proj0", "fit_image", "smpl"),
    _c("i_proj2", "fit_image", "smpl", dict(projection=2)),
    _c("i_focal", "fit_image", "smpl", dict(projection=1, focal=(500.0, -1.0))),
    _c("i_focal_and_idx", "fit_image", "smpl", dict(projection=1, focal=(0.0, 0.0)), idx=(0, 45)),
    _c("i_K0", "fit_image", "smpl", P1, idx=()),
    _c("i_idx_null", "fit_image", "smpl", P1, idx=None, K=1),
    _c("i_idx_range", "fit_image", "smpl", P1, idx=(0, 45)),
    _c("i_surface_count", "fit_image", "smplx_lmk", _join(P1, X63), idx=SURF129),
    _c("i_surface_only", "fit_image", "smpl", P1, idx=(24, 25)),
    _c("i_proj0_and_surface_only", "fit_image", "smpl", idx=(24, 25)),
    _c("i_scan64", "fit_image", "smpl_scan64", P1),
    _c("i_scan64_and_surface_only", "fit_image", "smpl_scan64", P1, idx=(24,)),
    _c("i_B_neg", "fit_image", "smpl", P1, B=-1),
    _c("i_scan64_and_B_neg", "fit_image", "smpl_scan64", P1, B=-1),
    _c("i_dup", "fit_image", "smpl", P1, idx=(0, 24, 0)),
    _c("i_null_j3d", "fit_image", "smpl", P1, null=("j3d",)),
    _c("i_tree_transl", "fit_image", "smplx", _join(P1, X63, dict(transl_prior_weight=1.0))),
    _c("i_tree_surface_only", "fit_image", "smplx", _join(P1, X63), idx=(55,)),
    _c("i_iters", "fit_image", "smpl", _join(P1, dict(num_iters=0)), idx=(0, 24)),
    # ---- k2b_fit_multiview ------------------------------------------------------------------------------------------------------
    _c("m_null_cfg", "fit_multiview", "smpl", None),
    _c("m_views0", "fit_multiview", "smpl", P1, views=0),
    _c("m_views9_and_null_model", "fit_multiview", None, P1, views=9, cameras=_cams(1)),
    _c("m_cameras_null", "fit_multiview", "smpl", P1, cameras=None),
    _c("m_views_and_cameras", "fit_multiview", "smpl", P1, views=-1, cameras=None),
    _c("m_proj0", "fit_multiview", "smpl"),
    _c("m_proj0_and_camera", "fit_multiview", "smpl", views=2, cameras=_cams(2, rotation=(4, NAN))),
    _c("m_rot_nan", "fit_multiview", "smpl", P1, views=2, cameras=_cams(2, rotation=(4, NAN))),
    _c("m_trans_inf", "fit_multiview", "smpl", P1, views=2, cameras=_cams(2, translation=(2, -INF))),
    _c("m_focal", "fit_multiview", "smpl", P1, cameras=_cams(1, focal=(1, 0.0))),
    _c("m_focal_and_idx", "fit_multiview", "smpl", P1, cameras=_cams(1, focal=(0, NAN)), idx=(0, 45)),
    _c("m_camera_and_null_model", "fit_multiview", None, P1, cameras=_cams(1, translation=(0, NAN))),
    _c("m_null_model", "fit_multiview", None, P1),
    _c("m_null_prior", "fit_multiview", "smpl", P1, prior=False),
    _c("m_K0", "fit_multiview", "smpl", P1, idx=()),
    _c("m_idx_range", "fit_multiview", "smpl", P1, idx=(0, 45)),
    _c("m_surface", "fit_multiview", "smpl", P1, idx=(0, 24)),
    _c("m_tree_surface", "fit_multiview", "smplx_lmk", _join(P1, X63), idx=(0, 130)),
    _c("m_scan64", "fit_multiview", "smpl_scan64", P1),
    _c("m_surface_and_scan64", "fit_multiview", "smpl_scan64", P1, idx=(0, 24)),
    _c("m_rows", "fit_multiview", "smplx", _join(P1, X63), B=(1 << 31) - 1, views=8, idx=tuple(i % 55 for i in range(127))),
    _c("m_B_neg", "fit_multiview", "smpl", P1, B=-1),
    _c("m_dup", "fit_multiview", "smpl", P1, views=2, idx=(3, 3)),
    _c("m_null_buf", "fit_multiview", "smpl", P1, null=("bp_in",)),
    _c("m_eps0", "fit_multiview", "smpl", _join(P1, dict(adam_eps=0.0))),
    _c("m_tree_transl", "fit_multiview", "smplx", _join(P1, X63), tr_prior=True),
    _c("m_B0_K0", "fit_multiview", "smpl", P1, B=0, idx=()),
    # ---- k2b_fit_world_lbfgs ----------------------------------------------------------------------------------------------------
    _c("l_null_model", "fit_world_lbfgs", None),
    _c("l_null_cfg", "fit_world_lbfgs", "smpl", None),
    _c("l_proj", "fit_world_lbfgs", "smpl", P1),
    _c("l_proj_and_history", "fit_world_lbfgs", "smpl", P1, history=101),
    _c("l_max_iter0", "fit_world_lbfgs", "smpl", max_iter=0),
    _c("l_max_iter_big", "fit_world_lbfgs", "smpl", max_iter=10001),
    _c("l_history", "fit_world_lbfgs", "smpl", history=101),
    _c("l_lr0", "fit_world_lbfgs", "smpl", lr=0.0),
    _c("l_lr_nan", "fit_world_lbfgs", "smpl", lr=NAN),
    _c("l_B_neg", "fit_world_lbfgs", "smpl", B=-1),
    _c("l_null_param", "fit_world_lbfgs", "smpl", null=("bp_out",)),
    _c("l_null_and_max_iter", "fit_world_lbfgs", "smpl", null=("bp_out",), max_iter=0),
    _c("l_B_neg_and_K0", "fit_world_lbfgs", "smpl", B=-1, idx=()),
    _c("l_K0", "fit_world_lbfgs", "smpl", idx=()),
    _c("l_idx_range", "fit_world_lbfgs", "smpl", idx=(0, 45)),
    _c("l_dup", "fit_world_lbfgs", "smpl", idx=(3, 3)),
    _c("l_dup_and_angle", "fit_world_lbfgs", "smpl", dict(angle_prior_index=(64, 55, 9, 12)), idx=(3, 3)),
    _c("l_angle", "fit_world_lbfgs", "smpl", dict(angle_prior_index=(52, 55, 64, 12))),
    _c("l_null_j3d", "fit_world_lbfgs", "smpl", null=("j3d",)),
    _c("l_adam", "fit_world_lbfgs", "smpl", dict(adam_beta1=-0.1)),
    _c("l_eps", "fit_world_lbfgs", "smpl", dict(adam_eps=-1.0)),
    _c("l_debug", "fit_world_lbfgs", "smpl", dict(debug_launch_shape=5)),
    _c("l_surface_only", "fit_world_lbfgs", "smpl", idx=(24, 25)),
    _c("l_tree_transl_w", "fit_world_lbfgs", "smplx", _join(X63, dict(transl_prior_weight=1.0))),
    _c("l_tree_transl_ptr", "fit_world_lbfgs", "smplx", X63, tr_prior=True),
    _c("l_tree_default_dims", "fit_world_lbfgs", "smplx"),
    _c("l_tree_dup", "fit_world_lbfgs", "smplx", X63, idx=(40, 40)),
    _c("l_tree_depth", "fit_world_lbfgs", "chain24", X63, idx=(0, 23)),
    # ---- k2b_fit_sequence_lbfgs -------------------------------------------------------------------------------------------------
    _c("sl_null_model", "fit_sequence_lbfgs", None),
    _c("sl_proj", "fit_sequence_lbfgs", "smpl", P1),
    _c("sl_first0", "fit_sequence_lbfgs", "smpl", max_iter=0),
    _c("sl_followup0", "fit_sequence_lbfgs", "smpl", followup=0),
    _c("sl_followup_big", "fit_sequence_lbfgs", "smpl", followup=10001),
    _c("sl_history", "fit_sequence_lbfgs", "smpl", history=1000),
    _c("sl_lr", "fit_sequence_lbfgs", "smpl", lr=-1.0),
    _c("sl_lr_and_followup", "fit_sequence_lbfgs", "smpl", lr=-1.0, followup=0),
    _c("sl_T_neg", "fit_sequence_lbfgs", "smpl", B=-1),
    _c("sl_transl", "fit_sequence_lbfgs", "smpl", dict(transl_prior_weight=1.0)),
    _c("sl_T0_transl", "fit_sequence_lbfgs", "smpl", dict(transl_prior_weight=1.0), B=0),
    _c("sl_transl_and_null", "fit_sequence_lbfgs", "smpl", dict(transl_prior_weight=1.0), null=("j3d",)),
    _c("sl_null_j3d", "fit_sequence_lbfgs", "smpl", null=("j3d",)),
    _c("sl_null_param", "fit_sequence_lbfgs", "smpl", null=("tr_in",)),
    _c("sl_K0", "fit_sequence_lbfgs", "smpl", idx=()),
    _c("sl_idx_range", "fit_sequence_lbfgs", "smpl", idx=(0, 45)),
    _c("sl_dup", "fit_sequence_lbfgs", "smpl", idx=(3, 3)),
    _c("sl_dup_and_angle", "fit_sequence_lbfgs", "smpl", dict(angle_prior_index=(64, 55, 9, 12)), idx=(3, 3)),
    _c("sl_angle", "fit_sequence_lbfgs", "smpl", dict(angle_prior_index=(64, 55, 9, 12))),
    _c("sl_adam", "fit_sequence_lbfgs", "smpl", dict(adam_beta2=1.0)),
    _c("sl_surface_only", "fit_sequence_lbfgs", "smpl", idx=(24,)),
    _c("sl_tree_dup", "fit_sequence_lbfgs", "smplx", X63, idx=(40, 40)),
    _c("sl_tree_default_dims", "fit_sequence_lbfgs", "smplx"),
    _c("sl_T1_dup", "fit_sequence_lbfgs", "smpl", B=1, idx=(3, 3)),
    # ---- k2b_fit_sequences_lbfgs ------------------------------------------------------------------------------------------------
    _c("ql_S_neg", "fit_sequences_lbfgs", "smpl", lengths=(), S=-1),
    _c("ql_offsets", "fit_sequences_lbfgs", "smpl", lengths=(2, 2), offsets=(0, 1)),
    _c("ql_ragged_and_null_model", "fit_sequences_lbfgs", None, lengths=(-2,)),
    _c("ql_null_model", "fit_sequences_lbfgs", None),
    _c("ql_proj", "fit_sequences_lbfgs", "smpl", P1),
    _c("ql_first0", "fit_sequences_lbfgs", "smpl", max_iter=0),
    _c("ql_followup", "fit_sequences_lbfgs", "smpl", followup=0),
    _c("ql_history", "fit_sequences_lbfgs", "smpl", history=101),
    _c("ql_lr", "fit_sequences_lbfgs", "smpl", lr=0.0),
    _c("ql_transl", "fit_sequences_lbfgs", "smpl", dict(transl_prior_weight=1.0)),
    _c("ql_followup_and_transl", "fit_sequences_lbfgs", "smpl", dict(transl_prior_weight=1.0), followup=0),
    _c("ql_K0", "fit_sequences_lbfgs", "smpl", idx=()),
    _c("ql_idx_range", "fit_sequences_lbfgs", "smpl", idx=(0, 45)),
    _c("ql_empty_idx_range", "fit_sequences_lbfgs", "smpl", lengths=(0, 0), idx=(0, 45)),
    _c("ql_null", "fit_sequences_lbfgs", "smpl", null=("be_in",)),
    _c("ql_null_and_surface", "fit_sequences_lbfgs", "smpl", null=("be_in",), idx=(0, 24)),
    _c("ql_surface", "fit_sequences_lbfgs", "smpl", idx=(0, 24)),
    _c("ql_smplx", "fit_sequences_lbfgs", "smplx", X63),
    _c("ql_tree63", "fit_sequences_lbfgs", "smpl", X63),
    _c("ql_dup", "fit_sequences_lbfgs", "smpl", idx=(3, 3)),
    _c("ql_dup_and_angle", "fit_sequences_lbfgs", "smpl", dict(angle_prior_index=(52, 55, 9, 64)), idx=(3, 3)),
    _c("ql_angle", "fit_sequences_lbfgs", "smpl", dict(angle_prior_index=(52, 55, 9, 64))),
    _c("ql_adam", "fit_sequences_lbfgs", "smpl", dict(adam_beta1=1.0)),
    _c("ql_debug", "fit_sequences_lbfgs", "smpl", dict(debug_launch_shape=5)),
    # ---- k2b_shape_pass_lbfgs ---------------------------------------------------------------------------------------------------
    _c("sp_null_model", "shape_pass_lbfgs", None),
    _c("sp_proj", "shape_pass_lbfgs", "smpl", P1),
    _c("sp_max_iter", "shape_pass_lbfgs", "smpl", max_iter=0),
    _c("sp_history", "shape_pass_lbfgs", "smpl", history=101),
    _c("sp_lr", "shape_pass_lbfgs", "smpl", lr=0.0),
    _c("sp_S_neg", "shape_pass_lbfgs", "smpl", S=-1),
    _c("sp_N_neg", "shape_pass_lbfgs", "smpl", N=-1),
    _c("sp_root", "shape_pass_lbfgs", "smpl", root_joint=24),
    _c("sp_root_and_free", "shape_pass_lbfgs", "smpl", root_joint=-1, free_betas=0),
    _c("sp_free0", "shape_pass_lbfgs", "smpl", free_betas=0),
    _c("sp_free11", "shape_pass_lbfgs", "smpl", free_betas=11),
    _c("sp_K0", "shape_pass_lbfgs", "smpl", idx=()),
    _c("sp_idx_null", "shape_pass_lbfgs", "smpl", idx=None, K=2),
    _c("sp_idx_surface", "shape_pass_lbfgs", "smpl", idx=(0, 24)),
    _c("sp_S0_idx_surface", "shape_pass_lbfgs", "smpl", S=0, N=0, idx=(0, 24)),
    _c("sp_null", "shape_pass_lbfgs", "smpl", null=("betas_in",)),
    _c("sp_null_j3d", "shape_pass_lbfgs", "smpl", null=("j3d",)),
    _c("sp_dup", "shape_pass_lbfgs", "smpl", idx=(3, 3)),
    _c("sp_angle", "shape_pass_lbfgs", "smpl", dict(angle_prior_index=(52, 55, 9, 64))),
    _c("sp_adam", "shape_pass_lbfgs", "smpl", dict(adam_eps=0.0)),
    _c("sp_debug", "shape_pass_lbfgs", "smpl", dict(debug_launch_shape=5)),
    _c("sp_tree_transl", "shape_pass_lbfgs", "smplx", _join(X63, dict(transl_prior_weight=1.0))),
    _c("sp_tree_default_dims", "shape_pass_lbfgs", "smplx"),
]
assert len({c["id"] for c in CASES}) == len(CASES)


def call_of(case):
    """The call fields of a row with the defaults filled in and K, lengths / offsets and S made consistent."""
    unknown = set(case["call"]) - set(DEFAULTS)
    assert not unknown, (case["id"], unknown)
    f = dict(DEFAULTS, **case["call"])
    if f["K"] is None:
        f["K"] = len(f["idx"])
    if f["lengths"] is None:
        f["offsets"] = None
    else:
        if "S" not in case["call"]:
            f["S"] = len(f["lengths"])
        if f["offsets"] == "prefix":
            f["offsets"] = tuple(int(x) for x in np.concatenate([[0], np.cumsum(f["lengths"], dtype=np.int64)[:-1]]))
    if f["cameras"] == "identity":
        f["cameras"] = _cams(max(f["views"], 0)) if 0 < f["views"] <= 8 else _cams(1)
    return f


# ---- the real entries ---------------------------------------------------------------------------------------------------------
class Handles:
    """The models and the prior of MODELS / PRIOR on the device, and zeroed device buffers large enough for every row."""

    ROWS = 8

    def __init__(self, device="cuda:0"):
        import os

        import torch

        from keypoints2body_amd import native
        from oracle.fit_torch import GMMPrior

        self.native, self.torch, self.device = native, torch, torch.device(device)
        self.models = {}
        for name, spec in MODELS.items():
            for k, v in spec.get("env", {}).items():
                os.environ[k] = v
            try:
                c = spec["make"]()
                self.models[name] = native.NativeModel(c.v_template, c.shapedirs, c.posedirs, c.J_regressor, c.lbs_weights, c.parents,
                                                       c.extra_vertex_ids, device=device,
                                                       landmarks=spec["landmarks"]() if "landmarks" in spec else None)
            finally:
                for k in spec.get("env", {}):
                    del os.environ[k]
            m = self.models[name]
            assert (m.num_joints, m.num_extra, m.num_landmarks, m.num_betas) == (len(spec["parents"]), spec["E"], spec["L"], spec["NB"])
        gmm = synthetic.make_gmm(0)
        p = GMMPrior(gmm.means, gmm.covars, gmm.weights)
        self.prior = native.NativePrior(p.means.numpy(), p.precisions.numpy(), p.nll_weights.numpy().reshape(-1), device=device)
        assert (self.prior.dim, self.prior.num_gaussians) == (PRIOR["D"], PRIOR["M"])
        # one zeroed buffer per argument: ROWS frames x 8 views x 192 targets x 3 is the largest any row that reaches a launch reads
        n = self.ROWS * 8 * 192 * 3
        self.buf = {k: torch.zeros(n, dtype=torch.float32, device=self.device)
                    for k in PARAM_BUFFERS + ("conf", "preserve", "tr_prior", "loss", "grad", "global_orient", "body_pose", "root_targets",
                                              "betas_in", "betas_out")}

    def config(self, overrides):
        cfg = self.native.default_fit_config()
        for k, v in overrides.items():
            if isinstance(v, tuple):
                getattr(cfg, k)[:] = list(v)
            else:
                setattr(cfg, k, v)
        return cfg


def run_case(h, case, outputs=None):
    """Call the entry of `case` with the handles `h`; returns (code, message).  `outputs`: device tensors to pass as the four
    output parameter arrays instead of the shared zeroed ones."""
    import ctypes as C

    native, torch = h.native, h.torch
    lib = native.load_library()
    f = call_of(case)
    entry = case["entry"]
    model = h.models[case["model"]].handle if case["model"] is not None else None
    prior = h.prior.handle if f["prior"] else None
    cfg = C.byref(h.config(case["cfg"])) if case["cfg"] is not None else None
    keep = []

    def host_i32(values):
        if values is None:
            return None
        a = np.ascontiguousarray(np.asarray(values, dtype=np.int64).astype(np.int32).reshape(-1))
        if a.size == 0:
            a = np.zeros(1, np.int32)
        keep.append(a)
        return a.ctypes.data_as(C.c_void_p)

    def dev(name, present=True):
        if not present or name in f["null"]:
            return None
        if outputs is not None and name in outputs:
            return C.c_void_p(outputs[name].data_ptr())
        return C.c_void_p(h.buf[name].data_ptr())

    idx = host_i32(f["idx"])
    fit_in = (f["K"], idx, dev("j3d"), dev("conf"), dev("go_in"), dev("bp_in"), dev("be_in"), dev("tr_in"))
    fit_out = (dev("go_out"), dev("bp_out"), dev("be_out"), dev("tr_out"), dev("loss"))
    world = (dev("preserve", f["preserve"]), dev("tr_prior", f["tr_prior"]))
    grad = (dev("grad", f["grad_out"]),)
    lbfgs_tail = (int(f["history"]), float(f["lr"]), 1e-7, 1e-9)
    ragged = (f["S"], host_i32(f["lengths"]), host_i32(f["offsets"]))
    head = (model, prior, cfg)
    with torch.cuda.device(h.device):
        stream = (C.c_void_p(torch.cuda.current_stream(h.device).cuda_stream),)
        if entry == "fit_world":
            args = head + (f["B"],) + fit_in + world + fit_out + grad
        elif entry == "fit_sequence":
            args = head + (f["S"], f["T"], f["followup"]) + fit_in + fit_out
        elif entry == "fit_sequences":
            args = head + ragged + (f["followup"],) + fit_in + fit_out
        elif entry == "fit_image_sequences":
            args = head + ragged + (f["followup"], 0) + fit_in + fit_out
        elif entry == "fit_image":
            args = head + (f["B"],) + fit_in + world + fit_out + grad
        elif entry == "fit_multiview":
            table = native.camera_table([tuple(r) for r in f["cameras"]]) if f["cameras"] is not None else None
            keep.append(table)
            args = head + (f["B"], f["views"], table) + fit_in + world + fit_out + grad
        elif entry == "fit_world_lbfgs":
            args = head + (f["B"],) + fit_in + world + fit_out + grad + (f["max_iter"],) + lbfgs_tail
        elif entry == "fit_sequence_lbfgs":
            args = head + (f["B"],) + fit_in + fit_out + (f["max_iter"], f["followup"]) + lbfgs_tail
        elif entry == "fit_sequences_lbfgs":
            args = head + ragged + fit_in + fit_out + (f["max_iter"], f["followup"]) + lbfgs_tail
        elif entry == "shape_pass_lbfgs":
            seq = torch.tensor([0] + [max(f["N"], 0)] * max(f["S"], 1), dtype=torch.int32, device=h.device)
            keep.append(seq)
            args = head + (f["S"], None if "seq_offsets" in f["null"] else C.c_void_p(seq.data_ptr()), f["N"], f["K"], idx, dev("j3d"),
                           dev("conf"), dev("global_orient"), dev("body_pose"), dev("root_targets"), f["root_joint"], f["free_betas"],
                           dev("betas_in"), dev("betas_out"), f["max_iter"]) + lbfgs_tail
        else:
            raise KeyError(entry)
        code = getattr(lib, "k2b_" + entry)(*args, *stream)
        message = lib.k2b_last_error().decode("utf-8", "replace") if code != 0 else ""
    return int(code), message


# ---- the same rows for tests/host/fit_rules_check.cpp -------------------------------------------------------------------------
CFG_FIELDS = ("num_iters", "step_size", "adam_beta1", "adam_beta2", "adam_eps", "freeze_betas", "conf_per_frame", "angle_prior_index",
              "transl_prior_weight", "debug_launch_shape", "prior_pose_dims", "num_betas_prior", "projection", "focal")


def _num(x):
    return repr(float(x)) if isinstance(x, float) else str(int(x))


def _list(values):
    return "null" if values is None else "-" if len(values) == 0 else ",".join(_num(v) for v in values)


def host_line(case, default_cfg):
    """One row as ``key=value`` tokens: the facts of the handles as integers, the configuration, the call.  `default_cfg`: the
    library's defaults as a dict of CFG_FIELDS."""
    f = call_of(case)
    t = [f"id={case['id']}", f"entry={case['entry']}"]
    if case["model"] is not None and f["prior"]:
        m = MODELS[case["model"]]
        t += [f"facts=1", f"J={len(m['parents'])}", f"E={m['E']}", f"L={m['L']}", f"NB={m['NB']}", f"fit_ok={m['fit_ok']}",
              f"scan64={m['scan64']}", f"depth={_list(depths(m['parents']))}", f"D={PRIOR['D']}", f"M={PRIOR['M']}"]
    else:
        t.append("facts=0")
    if case["cfg"] is None:
        t.append("cfg=0")
    else:
        cfg = dict(default_cfg, **case["cfg"])
        t.append("cfg=1")
        for k in CFG_FIELDS:
            t.append(f"{k}={_list(cfg[k]) if isinstance(cfg[k], (tuple, list)) else _num(cfg[k])}")
    shape = case["entry"] == "shape_pass_lbfgs"
    names = SHAPE_BUFFERS if shape else PARAM_BUFFERS
    t += [f"B={f['B']}", f"K={f['K']}", f"idx={_list(f['idx'])}", "null=" + ("".join("1" if n in f["null"] else "0" for n in names)),
          f"preserve={int(f['preserve'])}", f"tr_prior={int(f['tr_prior'])}", f"grad_out={int(f['grad_out'])}",
          f"S={f['S']}", f"T={f['T']}", f"followup={f['followup']}", f"lengths={_list(f['lengths'])}", f"offsets={_list(f['offsets'])}",
          f"max_iter={f['max_iter']}", f"history={f['history']}", f"lr={_num(float(f['lr']))}", f"views={f['views']}",
          f"N={f['N']}", f"root_joint={f['root_joint']}", f"free_betas={f['free_betas']}"]
    if f["cameras"] is None:
        t.append("cameras=null")
    else:
        t.append("cameras=" + ";".join(_list([float(np.float32(x)) for part in cam for x in part]) for cam in f["cameras"]))
    return " ".join(t)
