/*
 * k2b.h — C ABI of the MI355X-native SMPLify-style fitting engine (libk2b.so).
 *
 * The reference (saifkhichi96/keypoints2body) is pure Python and has no FFI; these
 * entry points are what a binding for its hot path would call, one per Python-level
 * seam that SURVEY.md §8(b) names.  Each declaration cites the reference interface it
 * replaces (paths relative to /root/reference/keypoints2body).  INTEGRATION.md shows the
 * ctypes stub a maintainer of the reference would add.
 *
 * Conventions
 *   - every function returns K2B_OK (0) or a negative k2b_status; k2b_last_error()
 *     returns a thread-local, human-readable message for the last failure;
 *   - "dev" pointers are device (HBM) addresses, e.g. torch `tensor.data_ptr()` of a
 *     contiguous float32 tensor on the HIP device; "host" pointers are host memory;
 *   - all matrices are row-major (C order), float32 unless stated;
 *   - launches are stream-ordered on `stream` (a hipStream_t passed as void*; NULL =
 *     the default stream).  Calls that may block the host or synchronise the device:
 *     *_create / *_destroy always; k2b_lbs when its per-model workspace has to GROW (first
 *     call, or more frames than any earlier call: hipDeviceSynchronize + hipFree/hipMalloc;
 *     k2b_model_reserve() pre-sizes it so that later calls never do); k2b_fit_world on the
 *     FIRST use of an (iterations, lr, beta1, beta2) combination per model (blocking upload
 *     of the Adam bias table; at most 64 tables are kept, least recently used evicted after
 *     a stream sync).  k2b_vertex_term never synchronises: its joint selection travels by value in
 *     the kernel arguments; k2b_surface_term, k2b_surface_term_image, and k2b_fit_world / k2b_fit_image with surface
 *     targets synchronise the
 *     stream on the FIRST use of a selection per model (its vertex table is gathered and cached);
 *   - buffers are caller-owned; inputs are never written; handles may be shared by
 *     threads as long as concurrent calls use different streams AND different
 *     workspaces (one workspace per handle: serialise calls on one handle);
 *   - an entry writes every element of its outputs and no byte outside them, and never an input; outputs and inputs of one
 *     call do not overlap, with ONE exception, the aliasing rule of the four frame fitters k2b_fit_world, k2b_fit_image,
 *     k2b_fit_multiview and k2b_fit_world_lbfgs: each of global_orient_out, body_pose_out, betas_out, transl_out may be the
 *     very buffer of its own *_in (the same address: the fit is then in place); preserve_pose may be the body_pose buffer
 *     and transl_prior_target the transl buffer, in place or not (the call keeps what it needs of the INITIAL values
 *     before it overwrites them, as it does for their NULL defaults); the result is, bit for bit, that of the call with
 *     separate buffers.  Any other overlap between an output and another buffer of the same call - a partial overlap, an
 *     output on another parameter's input, on the targets or on loss_out / grad_out - is not supported.  k2b_adam_step
 *     updates params, m and v in place by definition.  (tests/test_gpu_caller_buffers.py)
 *   - frames are independent, non-finite inputs included: in every entry with a frame or
 *     sequence dimension (k2b_fit_world, k2b_fit_world_lbfgs, k2b_fit_sequence, k2b_fit_sequences,
 *     k2b_fit_image, k2b_fit_image_sequences, k2b_fit_multiview, k2b_fit_multiview_sequences, k2b_fit_sequence_lbfgs, k2b_fit_sequences_lbfgs, k2b_shape_pass_lbfgs, k2b_lbs,
 *     k2b_lbs_backward, k2b_vertex_term, k2b_surface_term, k2b_surface_term_image) each output of a frame (in the chain
 *     entries and the shape pass: of a sequence; inside a chain a frame also never depends on
 *     a LATER frame) depends only on that frame's own inputs, bit for bit, even when another
 *     frame's inputs are NaN or +-Inf (a missing keypoint written as NaN, say).  A frame whose
 *     loss depends on a non-finite input reports a non-finite loss_out; its fitted parameters
 *     are then unspecified (under L-BFGS the optimiser stops at its finite start), and so are
 *     the frames behind it in the same sequence of an L-BFGS chain, which start from them; in
 *     an Adam chain those frames report a non-finite loss too.  The stand-alone terms, k2b_lbs and k2b_lbs_backward return
 *     non-finite values wherever float64 arithmetic on the same frame does, and possibly in
 *     more elements of that same frame.  (tests/test_gpu_isolation.py)
 *   - a call does not depend on the calls before it: every output is, bit for bit, what the same call returns on freshly
 *     created handles, whatever batches (larger ones, non-finite ones, refused ones) its handles, its thread and its
 *     stream served before, and whatever the output buffers held; k2b_fit_multiview and k2b_fit_multiview_sequences included,
 *     whose camera table travels in the kernel arguments and leaves nothing on a handle.  (tests/test_gpu_call_history.py, tests/test_gpu_multiview_fit.py;
 *     DESIGN.md 4.4e.)
 */
#ifndef K2B_H
#define K2B_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum k2b_status {
    K2B_OK = 0,
    K2B_ERR_INVALID_ARGUMENT = -1, /* -> Python ValueError (world_space.py:118-119, adapters.py:104-117) */
    K2B_ERR_UNSUPPORTED = -2,      /* -> Python NotImplementedError (api/frame.py:71-75) */
    K2B_ERR_HIP = -3,              /* -> Python RuntimeError: a HIP runtime call failed */
    K2B_ERR_NO_DEVICE = -4         /* -> Python RuntimeError: no gfx950 device / kernels not loadable */
} k2b_status;

typedef struct k2b_model k2b_model; /* body-model constants resident in HBM */
typedef struct k2b_prior k2b_prior; /* max-mixture pose prior resident in HBM */
typedef struct k2b_ikgat k2b_ikgat; /* IK-GAT rotation regressor (weights + graph) resident in HBM */

/* Library / ABI version: (major << 16) | minor. */
uint32_t k2b_version(void);
/* Marks a declaration with the ABI version that introduced it (documentation only: expands to nothing). */
#define K2B_SINCE(major, minor)
/* Message of the last failing call on this thread ("" if none). */
const char *k2b_last_error(void);

/* ---------------------------------------------------------------------------------
 * Body model.  Replaces `load_body_model` / `smplx.create(...).to(device)`
 * (api/model_factory.py:19-40) for the constants the path reads, and precomputes
 * J_template = J_regressor . v_template and J_dirs = J_regressor . shapedirs (the
 * dense J x V contraction, an fp32 MFMA kernel) so that the per-iteration kernel never
 * touches vertices (SURVEY.md §8a note N1).
 *
 * All pointers are HOST pointers; the arrays are copied.
 *   v_template  [V][3]        shapedirs [V][3][NB]      posedirs [9*(J-1)][3*V]
 *   j_regressor [J][V]        lbs_weights [V][J]        parents [J] (parents[0] = -1,
 *   extra_vertex_ids [E]      (output joints J..J+E-1 are these vertices)   parents[i] < i)
 * Limits: 2 <= J <= 64, 1 <= NB <= 32, E >= 0.  (24 joints with NB <= 16 run the 24-lane fused fit kernel,
 * everything else the tree kernel; the vertex kernels are built for 17-24 and 49-56 joints, with every NB up to 32: a frame's
 * 9(J-1) + NB + 2 features are staged in at most 34 k-steps of 16, 544 features, and 56 joints with 32 coefficients are 529.)
 * Development switch: with K2B_LBS_TILE set to a non-zero number in the environment WHEN THIS FUNCTION RUNS, k2b_lbs skins the
 * model with the tile kernel instead of a stream kernel (the same results within the forward's tolerance; a test twin).
 * ------------------------------------------------------------------------------- */
int k2b_model_create(k2b_model **out, int32_t num_vertices, int32_t num_joints, int32_t num_betas,
                     int32_t num_extra_joints, const float *v_template, const float *shapedirs,
                     const float *posedirs, const float *j_regressor, const float *lbs_weights,
                     const int32_t *parents, const int32_t *extra_vertex_ids);
void k2b_model_destroy(k2b_model *model);
/* Sizes: V, J, NB, E. */
int k2b_model_dims(const k2b_model *model, int32_t *num_vertices, int32_t *num_joints,
                   int32_t *num_betas, int32_t *num_extra_joints);
/* Pre-sizes the per-model LBS workspace for batches of up to `max_frames` frames, so that no later k2b_lbs
 * call on this model allocates or synchronises (see Conventions).  Synchronises the device if it has to grow. */
int k2b_model_reserve(k2b_model *model, int32_t max_frames);
/* Facial landmarks (smplx `vertices2landmarks`): landmark l is the barycentric point sum_k bary[l][k] v[vertex_ids[l][k]] of
 * one mesh triangle (smplx: vertex_ids = faces_tensor[lmk_faces_idx], bary = lmk_bary_coords).  HOST pointers, copied.  Call
 * at most once per handle (a second successful call fails; a failed call leaves no table and may be repeated), before any
 * fit or LBS call on it.  0 <= L <= 1024, vertex ids in [0, V), finite weights summing to 1 within 1e-3 per landmark
 * (barycentric).  With L > 0 the output joints follow smplx's layout: J kinematic joints, E extra vertices, L landmarks;
 * model joint index J + E + l names landmark l in model_joint_index.  Synchronises the device. */
int k2b_model_set_landmarks(k2b_model *model, int32_t num_landmarks, const int32_t *vertex_ids /*[L][3]*/,
                            const float *bary /*[L][3]*/);
int k2b_model_num_landmarks(const k2b_model *model, int32_t *num_landmarks);
/* Copies the precomputed J_template [J][3] and J_dirs [J][3][NB] to HOST buffers (either may be NULL). */
int k2b_model_joint_basis(const k2b_model *model, float *j_template, float *j_dirs);

/* ---------------------------------------------------------------------------------
 * Pose prior.  Replaces the buffers `MaxMixturePrior.__init__` registers
 * (core/prior.py:133-163): `means [M][D]`, `precisions [M][D][D]`, `nll_weights [M]`
 * (HOST pointers, float32, exactly those buffers).  D must equal 3*(J-1) of the model
 * it is used with.  The library symmetrises each precision (0.5 (P + P^T), the exact
 * gradient of the quadratic form) and stores -log(nll_weights).
 * ------------------------------------------------------------------------------- */
int k2b_prior_create(k2b_prior **out, int32_t num_gaussians, int32_t dim, const float *means,
                     const float *precisions, const float *nll_weights);
void k2b_prior_destroy(k2b_prior *prior);

/* ---------------------------------------------------------------------------------
 * Fit configuration.  Field-for-field the knobs of
 *   WorldSpaceFitter.__init__/fit_frame   (core/fitters/world_space.py:56-66, 93-103, 214)
 *   body_fitting_loss_3d                  (core/losses.py:24-38)
 *   torch.optim.Adam(lr, betas=(0.9, 0.999), eps=1e-8)  (world_space.py:249)
 * k2b_fit_config_default() fills the values the reference's world fitter uses.
 * Adam numbers: step_size >= 0 and 0 <= beta < 1 as in torch.  adam_eps: its float32 rounding must be a normal positive
 * number (1.17549435e-38 .. 3.4e38); every Adam entry (k2b_fit_world, k2b_fit_sequence, k2b_fit_sequences,
 * k2b_adam_step) returns K2B_ERR_INVALID_ARGUMENT for a negative value, NaN, 0 or a float32 denormal.  torch accepts 0;
 * here the update of a parameter with gradient 0 - one outside the optimiser, say - would be 0 * rcp(0) = NaN.  The
 * L-BFGS entries pass the config through the same checks.  Known deviation from torch: the fit entries form the first
 * moment as m + (1 - beta1)(g - m) for every beta1; torch's lerp switches to g - (g - m) beta1 from 1 - beta1 = 0.5 on.
 * For adam_beta1 <= 0.5 the two differ by an ulp of max(|m|, |g|) per step, which can lose a gradient that collapses by
 * orders of magnitude within one iteration; k2b_adam_step follows torch in both forms.  (tests/test_gpu_adam.py;
 * DESIGN.md 1.1.)
 * ------------------------------------------------------------------------------- */
typedef struct k2b_fit_config {
    int32_t num_iters;          /* num_iters_first if seq_ind == 0 else num_iters_followup */
    double step_size;           /* Adam lr (config.py:30), 1e-2 (0 = evaluate only).  Adam numbers are doubles */
    double adam_beta1;          /* 0.9     because torch keeps them as Python floats and forms     */
    double adam_beta2;          /* 0.999   1-beta, beta**t and lr/(1-beta1**t) in double before    */
    double adam_eps;            /* 1e-8    rounding to float32 (torch/optim/adam.py)               */
    float sigma;                /* GMoF sigma (losses.py:33), 100 */
    float joint_loss_weight;    /* 600 (config.py:34) */
    float pose_prior_weight;    /* 4.78*1.5 (losses.py:34) */
    float angle_prior_weight;   /* 15.2 (losses.py:36) */
    float shape_prior_weight;   /* 5.0 (losses.py:35) */
    float pose_preserve_weight; /* 5.0 if seq_ind > 0 else 0 (world_space.py:211) */
    int32_t freeze_betas;       /* betas excluded from the optimiser (world_space.py:171,228-229) */
    int32_t conf_per_frame;     /* 0: conf is [K] shared by all frames (the reference's behaviour,
                                   world_space.py:161-164); 1: conf is [B][K] */
    int32_t angle_prior_index[4]; /* body-pose indices of the bending prior (losses.py:16): 52,55,9,12 */
    float angle_prior_sign[4];    /* (losses.py:17): +1,-1,-1,-1 */
    /* Parameter groups handed to the optimiser: bit 0 global_orient, 1 body_pose, 2 betas, 3 transl.
     * 15 = world fitter (world_space.py:215-229); 9 = stage 1 of the camera-space fitter
     * (camera_space.py:137-141: [global_orient, camera_translation]).  freeze_betas clears bit 2. */
    int32_t optimize_mask;
    /* w_t^2 * |transl - transl_prior_target|^2, the depth term of camera_fitting_loss_3d
     * (losses.py:70-93: depth_loss_weight 100; its broadcast over the 4 torso joints makes the
     * effective weight 200 in that path).  0 = off. */
    float transl_prior_weight;
    /* Debug / test knob: 0 = the launcher picks the launch shape from the batch size (the product setting);
     * 1, 2, 3, 4 force the split / split-paired / paired / wide (16-wave) shape of the fused kernel (and a single launch), so
     * that the parity tests can drive every shape with small cases.  Results do not depend on it.  The tree kernel of the larger
     * models has two shapes: 1 = plain (every wave a frame + its share of the mixture), 2 = four extra component waves. */
    int32_t debug_launch_shape;
    /* Larger models (SMPL-H / SMPL-X): `body_pose` holds ALL non-root joints (SMPL-X: body 63 | jaw, eyes 9 | hands
     * 90), `betas` all shape coefficients (betas | expression).  The mixture, the bending prior and the preserve term
     * see the first prior_pose_dims values of body_pose (0 = all of them; SMPL-X: 63, the mixture's remaining
     * dimensions fixed at 0); the shape prior and freeze_betas apply to the first num_betas_prior coefficients
     * (0 = all; SMPL-X: 10, the expression stays free as in world_space.py:137-151,215-229). */
    int32_t prior_pose_dims;
    int32_t num_betas_prior;
    /* K2B_SINCE(1, 7).  Joint term in image space: 0 = off (the 3D term above, the default); 1 = perspective reprojection
     * (k2b_fit_world, and the chains of k2b_fit_image_sequences; several cameras: k2b_fit_multiview, k2b_fit_multiview_sequences).  The target buffer keeps its [B][K][3] layout; row k holds
     * (u - cx, v - cy, ignored): pixel coordinates WITH THE PRINCIPAL POINT ALREADY SUBTRACTED by the caller (in float64, before the rounding to float32:
     * raw pixel coordinates of a few hundred lose more in that rounding than the gradient tests allow).  For
     * every targeted joint, with (X, Y, Z) = p_k + transl (transl = the camera translation, as in the camera-space fitter):
     *     e_x = fx X / Z - u',   e_y = fy Y / Z - v'
     *     loss term = w_j^2 sum_k c_k^2 (gmof(e_x, sigma) + gmof(e_y, sigma)),   sigma in pixels
     * and every other term, optimize_mask, freeze_betas, the confidences and the loss convention as for the 3D term.
     * Z is divided by as it stands (no clamp): a joint behind the camera (Z < 0) is legal and finite; a targeted joint of
     * non-zero confidence at Z = 0 makes THAT frame's loss and gradient non-finite and no other frame's (Conventions); a joint
     * without a target, or with confidence 0, contributes exactly nothing whatever its depth.
     * Kinematic targets only in k2b_fit_world and the chains (a surface target: K2B_ERR_UNSUPPORTED); surface targets
     * (vertex-selected joints, landmarks) under projection are taken by k2b_fit_image, their term alone by
     * k2b_surface_term_image.  Adam only; independent frames here, warm-start chains
     * through k2b_fit_image_sequences (every other fit entry refuses projection != 0 with K2B_ERR_UNSUPPORTED, as does a
     * model created under K2B_FIT_SCAN64=1).
     * The term has NO counterpart in the reference (api/frame.py:71-75 raises for joints2d): it is defined here and held to
     * a float64 oracle of this formula, not to reference outputs. */
    int32_t projection;
    float focal[2];             /* fx, fy in pixels: finite and > 0; read only when projection != 0 */
} k2b_fit_config;

void k2b_fit_config_default(k2b_fit_config *cfg);
/* sizeof(k2b_fit_config) as compiled into the library: lets a binding verify its struct mirror. */
uint32_t k2b_fit_config_size(void);

/* ---------------------------------------------------------------------------------
 * k2b_fit_world — the hot path.  Replaces the Adam branch of
 * `WorldSpaceFitter.fit_frame` (core/fitters/world_space.py:93-256) for a batch of B
 * independent frames: per iteration the SMPL joint forward (Rodrigues, kinematic chain,
 * J(beta)), `body_fitting_loss_3d` (core/losses.py:24-67) with `MaxMixturePrior`
 * (core/prior.py:182-195), the analytic backward and the Adam update, all iterations
 * fused in one launch (one or two wavefronts per frame, or two frames per wavefront, by batch size).
 *
 *   model_joint_index [K] HOST int32: model joint fitted to target k (the reference's
 *       smpl_index / target_model_indices, world_space.py:194-201); values must be
 *       distinct.  Indices >= J name SURFACE targets: smplx's vertex-selected "extra" joints
 *       (J .. J+E-1) and landmarks (J+E .. J+E+L-1, k2b_model_set_landmarks); at most 128 of them, at
 *       least one kinematic joint beside them; any supported tree.  The call then queues TWO
 *       launches per iteration on the stream - the fused kernel in evaluate-only mode and the
 *       surface-term kernel with its Adam tail - with no host work in between; conf may be per
 *       frame there too.  At most 32 extra joints and no landmark: k2b_vertex_term's kernel (the
 *       results of the first release, bit for bit); otherwise k2b_surface_term's.  The first use of
 *       a selection of surface targets on a model synchronises the stream (its vertex table is
 *       gathered and cached: at most 64 selections per model, least recently used evicted after a
 *       device sync).
 *   j3d  dev [B][K][3]   target joints (already gathered with corr_index)
 *   conf dev [K] or [B][K] (see conf_per_frame); NULL = ones
 *   *_in dev: initial global_orient [B][3], body_pose [B][3(J-1)], betas [B][NB], transl [B][3]
 *   preserve_pose dev [B][3(J-1)] or NULL (= body_pose_in, as world_space.py:159)
 *   transl_prior_target dev [B][3] or NULL (= transl_in): centre of the transl prior
 *   *_out dev: fitted parameters, same shapes; each may be the buffer of its own *_in (Conventions, the aliasing rule;
 *       tests/test_gpu_caller_buffers.py)
 *   loss_out dev [B]: per-frame loss of the LAST iteration evaluated BEFORE its step
 *       (world_space.py:256); the reference's scalar is the sum over the batch
 *   grad_out dev [B][P] or NULL: d loss / d params at the last iteration, P = 3J + NB + 3,
 *       order [global_orient | body_pose | betas | transl] (debug / tests)
 * ------------------------------------------------------------------------------- */
int k2b_fit_world(const k2b_model *model, const k2b_prior *prior, const k2b_fit_config *cfg,
                  int32_t num_frames, int32_t num_targets, const int32_t *model_joint_index,
                  const float *j3d, const float *conf,
                  const float *global_orient_in, const float *body_pose_in, const float *betas_in,
                  const float *transl_in, const float *preserve_pose, const float *transl_prior_target,
                  float *global_orient_out, float *body_pose_out, float *betas_out, float *transl_out,
                  float *loss_out, float *grad_out, void *stream);

/* ---------------------------------------------------------------------------------
 * k2b_fit_sequence — the reference's sequence mode as ONE launch.  Replaces the frame loop of
 * `optimize_params_sequence` with `use_previous_frame_init=True` (api/sequence.py:214-281): frame 0 of
 * a sequence is fitted from the given start with cfg->num_iters iterations and no preserve term
 * (seq_ind == 0: world_space.py:159,211); every later frame starts from the previous frame's
 * RESULT, preserves that result's body pose with cfg->pose_preserve_weight (world_space.py:159) and
 * runs `followup_iters` iterations (world_space.py:214) with a fresh Adam state.  The chain of one
 * sequence is serial (one cooperating wavefront pair walks it); num_sequences chains run side by side.
 *
 *   j3d  dev [S][T][K][3], conf dev [K] or [S][T][K] (conf_per_frame)
 *   *_in dev [S][...]: start of frame 0 of every sequence
 *   *_out dev [S][T][...], loss_out dev [S][T]: every frame's fitted parameters / last-iteration loss
 * Kinematic targets only (vertex-selected joints: K2B_ERR_UNSUPPORTED - fit frame by frame); cfg->transl_prior_weight
 * must be 0.  24-joint models run the split shape of the fused kernel, larger trees (SMPL-X) the tree kernel.
 * ------------------------------------------------------------------------------- */
int k2b_fit_sequence(const k2b_model *model, const k2b_prior *prior, const k2b_fit_config *cfg,
                     int32_t num_sequences, int32_t frames_per_sequence, int32_t followup_iters,
                     int32_t num_targets, const int32_t *model_joint_index,
                     const float *j3d, const float *conf,
                     const float *global_orient_in, const float *body_pose_in, const float *betas_in,
                     const float *transl_in,
                     float *global_orient_out, float *body_pose_out, float *betas_out, float *transl_out,
                     float *loss_out, void *stream);

/* ---------------------------------------------------------------------------------
 * k2b_fit_world_lbfgs — the L-BFGS branch of the fitters, which is the reference's DEFAULT (core/config.py:29
 * `use_lbfgs=True`; world_space.py:231-247, camera_space.py:144-182,229-267): per frame
 *     torch.optim.LBFGS(params, max_iter=num_iters, lr=step_size, line_search_fn="strong_wolfe").step(closure)
 * followed by one more evaluation of the loss at the result (world_space.py:245-246).  The closure (loss and gradient at
 * the current parameters) is k2b_fit_world's evaluate-only launch under `cfg` (its num_iters / step_size are ignored; weights,
 * sigma, optimize_mask, freeze_betas, prior_pose_dims ... apply: parameters outside the optimiser get a zero gradient and
 * never move); the optimiser itself - two-loop recursion over up to `history_size` pairs (<= 0: torch's 100), strong-Wolfe
 * bracket / zoom with torch's cubic interpolation, tolerance_grad / tolerance_change / max_iter / max_eval = max_iter * 5 / 4
 * exits - is a state machine on the device, one independent instance per frame (k2b_lbfgs.hip).  The call only queues
 * launches on `stream`: no host synchronisation, nothing is read back.  max_eval + 2 rounds of [closure, optimiser step] + the
 * final evaluation, as ONE launch for at most two frames per CU (the rounds are iterations of the fused kernel's loop, the
 * optimiser runs on an idle wave of the workgroup), one launch per round up to four frames per CU (the step as a prologue
 * of the closure's launch), two launches per round beyond that and for the larger models; the result does not depend on which.  Arguments as k2b_fit_world; preserve_pose / transl_prior_target NULL = the initial body pose /
 * translation; each *_out may be the buffer of its own *_in (Conventions, the aliasing rule; tests/test_gpu_caller_buffers.py);
 * loss_out dev [B] and grad_out dev [B][3 + 3(J-1) + NB + 3] (either may be NULL) receive
 * loss and gradient AT the result.  Frames never interact (torch couples the frames of a batch in one line search; the
 * reference only ever passes one frame).  At most 256 parameters per frame (3 + 3(J-1) + NB + 3): every model the fit
 * kernels take (63 joints and 32 shape coefficients are 224); beyond 192 the optimiser's step kernel runs in its wide form.
 * (k2b_lbs skins 17-24 and 49-56 joints with up to 32 shape coefficients: a model with another joint count gets fitted
 * parameters from this entry, but no vertices / joints from k2b_lbs.)
 * Line searches branch on rounding, so results agree with torch's statistically (and iterate by iterate with the float64
 * twin core/lbfgs_batched.py while rounding has not yet been amplified): see DESIGN.md.
 * ------------------------------------------------------------------------------- */
int k2b_fit_world_lbfgs(const k2b_model *model, const k2b_prior *prior, const k2b_fit_config *cfg,
                        int32_t num_frames, int32_t num_targets, const int32_t *model_joint_index,
                        const float *j3d, const float *conf,
                        const float *global_orient_in, const float *body_pose_in, const float *betas_in,
                        const float *transl_in, const float *preserve_pose, const float *transl_prior_target,
                        float *global_orient_out, float *body_pose_out, float *betas_out, float *transl_out,
                        float *loss_out, float *grad_out,
                        int32_t max_iter, int32_t history_size, double lr, double tolerance_grad,
                        double tolerance_change, void *stream);

/* ---------------------------------------------------------------------------------
 * k2b_fit_sequence_lbfgs — the reference's DEFAULT sequence mode in one call: the frame loop of
 * `optimize_params_sequence` with `use_previous_frame_init=True` (api/sequence.py:214-281, config.py:57) over the L-BFGS
 * branch (`use_lbfgs=True`, config.py:29; world_space.py:231-247).  ONE sequence of num_frames frames: frame 0 is fitted from
 * the given start (*_in: one row) with first_iters iterations and no preserve term (world_space.py:159,211); every later frame
 * starts from its predecessor's RESULT, preserves that result's body pose with cfg->pose_preserve_weight and runs
 * followup_iters iterations (world_space.py:214).  Every frame is one k2b_fit_world_lbfgs fit; the call only queues launches
 * (no host work between the frames) - ONE launch for the whole sequence where the fused kernel takes it (24-joint model,
 * kinematic targets: the frame loop runs inside the persistent launch), a launch or a few per frame otherwise; same bits.
 *   j3d dev [T][K][3]; conf dev [K], or [T][K] with cfg->conf_per_frame (each frame reads its own row, as the sequence API
 *   passes `conf[idx]`); *_out dev [T][...], loss_out dev [T] (may be NULL): every frame's result / loss at the result.
 * cfg->transl_prior_weight must be 0.
 * ------------------------------------------------------------------------------- */
int k2b_fit_sequence_lbfgs(const k2b_model *model, const k2b_prior *prior, const k2b_fit_config *cfg,
                           int32_t num_frames, int32_t num_targets, const int32_t *model_joint_index,
                           const float *j3d, const float *conf,
                           const float *global_orient_in, const float *body_pose_in, const float *betas_in,
                           const float *transl_in,
                           float *global_orient_out, float *body_pose_out, float *betas_out, float *transl_out,
                           float *loss_out, int32_t first_iters, int32_t followup_iters, int32_t history_size,
                           double lr, double tolerance_grad, double tolerance_change, void *stream);

/* ---------------------------------------------------------------------------------
 * k2b_fit_sequences / k2b_fit_sequences_lbfgs (ABI 1.3) — many warm-start sequences of DIFFERENT lengths side by side:
 * k2b_fit_sequence (Adam branch) and k2b_fit_sequence_lbfgs (L-BFGS branch, one optimiser per sequence) for
 * num_sequences = S sequences at once.  Frames are packed: sequence s owns rows offsets[s] .. offsets[s] + lengths[s] - 1.
 *   lengths, offsets  host int32 [S]: lengths[s] >= 0 (0: an empty sequence, nothing is written for it), offsets = the
 *                     exclusive prefix sums of lengths
 *   j3d dev [sum T][K][3]; conf dev [K], or [sum T][K] with cfg->conf_per_frame
 *   *_in dev [S][...]: start of every sequence's first frame
 *   *_out dev [sum T][...], loss_out dev [sum T] (may be NULL): every frame's result / loss, in the caller's order
 * Internally the sequences are sorted by length, longest first, so that similar lengths share a workgroup; a sequence's result
 * is bit-identical to the same sequence fitted alone (k2b_fit_sequence / k2b_fit_sequence_lbfgs with S = 1, or the
 * first-frame fit for a sequence of one frame), whatever its neighbours, S or the order.  ONE launch: the Adam branch for
 * every model with kinematic targets (24 joints: the fused kernel; SMPL-H / SMPL-X: the tree kernel), the L-BFGS branch for
 * the 24-joint model with the prior over the whole pose and kinematic targets.  Other configurations return
 * K2B_ERR_UNSUPPORTED (fit sequence by sequence).  Bad lengths / offsets and cfg->transl_prior_weight != 0 return
 * K2B_ERR_INVALID_ARGUMENT before anything is launched.  The slot table is uploaded stream-ordered from pinned staging; the
 * host waits at most for the same thread's previous upload.
 * ------------------------------------------------------------------------------- */
int k2b_fit_sequences(const k2b_model *model, const k2b_prior *prior, const k2b_fit_config *cfg,
                      int32_t num_sequences, const int32_t *lengths, const int32_t *offsets, int32_t followup_iters,
                      int32_t num_targets, const int32_t *model_joint_index,
                      const float *j3d, const float *conf,
                      const float *global_orient_in, const float *body_pose_in, const float *betas_in,
                      const float *transl_in,
                      float *global_orient_out, float *body_pose_out, float *betas_out, float *transl_out,
                      float *loss_out, void *stream);
/* k2b_sequence_order — the launch order of the two entries above, for inspection (host only, no device call): order_out[i] =
 * the sequence in chain slot i (sequences with frames, longest first, ties in the caller's order), *num_slots = their count.
 * The arguments are checked as the entries check them. */
int k2b_sequence_order(int32_t num_sequences, const int32_t *lengths, const int32_t *offsets, int32_t *order_out,
                       int32_t *num_slots);

/* ---------------------------------------------------------------------------------
 * k2b_fit_image_sequences (ABI 1.8) — warm-start chains over 2D keypoints: k2b_fit_sequences' chain under the projected
 * joint term of k2b_fit_config::projection, S ragged videos side by side in ONE launch (S = 1: the single video).
 * Argument conventions as k2b_fit_sequences (packed rows, host lengths / offsets, *_in one row per sequence, loss_out may
 * be NULL), plus followup_freeze_betas.
 *   keypoints dev [sum T][K][3]: rows (u - cx, v - cy, ignored), centred pixels as for k2b_fit_world under projection
 *   conf      dev [K], or [sum T][K] with cfg->conf_per_frame; NULL = ones
 *   transl_*  the camera translation
 * cfg->projection must be 1 and cfg->focal finite and positive (else K2B_ERR_INVALID_ARGUMENT: 3D targets have
 * k2b_fit_sequences).  Step 0 of a sequence is k2b_fit_world under `cfg`: cfg->num_iters iterations, no preserve term.  Step
 * t > 0 starts from step t - 1's RESULT, preserves that result's body pose with cfg->pose_preserve_weight, runs
 * followup_iters iterations with a fresh Adam state and, with followup_freeze_betas != 0, holds the shape as
 * cfg->freeze_betas = 1 would (a video's shape is estimated on its first frame: 24-joint models hold all betas, SMPL-H /
 * SMPL-X the first num_betas_prior coefficients - the expression stays free); cfg->freeze_betas itself applies to every
 * step, step 0 included.  A sequence of length 1 is the first-frame fit; a sequence of length 0 writes nothing.  loss_out is
 * every frame's last-iteration loss before its step, preserve term included.
 * A sequence's rows are bit-identical to the same sequence fitted alone, and to a host loop of k2b_fit_world calls that
 * hands each result on (tests/test_gpu_reproj_chain.py).  A non-finite keypoint stays in its own SEQUENCE: the frames before
 * it are untouched, the frame itself and the frames behind it in that sequence may be non-finite (a warm start inherits).
 * Refused before anything is launched, outputs untouched: surface targets and a 24-joint model without a scan plan or created
 * under K2B_FIT_SCAN64=1 (K2B_ERR_UNSUPPORTED); cfg->transl_prior_weight != 0, bad lengths / offsets, bad followup_iters
 * (K2B_ERR_INVALID_ARGUMENT).  Adam only.
 * ------------------------------------------------------------------------------- */
int k2b_fit_image_sequences(const k2b_model *model, const k2b_prior *prior, const k2b_fit_config *cfg,
                            int32_t num_sequences, const int32_t *lengths, const int32_t *offsets, int32_t followup_iters,
                            int32_t followup_freeze_betas, int32_t num_targets, const int32_t *model_joint_index,
                            const float *keypoints, const float *conf,
                            const float *global_orient_in, const float *body_pose_in, const float *betas_in,
                            const float *transl_in,
                            float *global_orient_out, float *body_pose_out, float *betas_out, float *transl_out,
                            float *loss_out, void *stream) K2B_SINCE(1, 8);

/* ---------------------------------------------------------------------------------
 * k2b_fit_image (ABI 1.9) — B independent frames of 2D keypoints under Adam, surface targets included.  The argument list is
 * k2b_fit_world's, the aliasing rule for *_out, preserve_pose and transl_prior_target included (Conventions;
 * tests/test_gpu_caller_buffers.py); the target buffer holds rows (u - cx, v - cy, ignored), centred pixels (k2b_fit_config::projection).
 * cfg->projection must be 1 and cfg->focal finite and positive (else K2B_ERR_INVALID_ARGUMENT: 3D targets have
 * k2b_fit_world).  With kinematic targets only the call IS k2b_fit_world under projection: the same launch, the same bits.
 * With surface targets among model_joint_index (indices >= J: extra joints and landmarks) it queues, per iteration, the fit
 * kernel in evaluate-only mode (projected kinematic term and every prior) and the projected surface kernel
 * (k2b_surface_term_image's) with its Adam tail; every surface selection takes that kernel, extras-only ones included.  For a
 * surface target t with weighted vertex pairs (u_tk, b_tk):
 *     (X, Y, Z) = sum_k b_tk x_u + (sum_k b_tk) transl,   e_x = fx X / Z - u',   e_y = fy Y / Z - v'
 *     loss_t = w_j^2 c_t^2 (gmof(e_x, sigma) + gmof(e_y, sigma))
 * under the conventions of the kinematic term: Z divided by as it stands (a point behind the camera is legal and finite), a
 * target of confidence 0 contributes exactly nothing whatever its depth.  The surface rules of k2b_fit_world hold: at least
 * one kinematic joint, at most 128 surface targets, conf per frame allowed, the first use of a selection on a model
 * synchronises the stream.  Refused before anything is launched, outputs untouched: projection != 1 or a bad focal
 * (K2B_ERR_INVALID_ARGUMENT); no kinematic joint, more than 128 surface targets, a 24-joint model without a scan plan or
 * created under K2B_FIT_SCAN64=1 (K2B_ERR_UNSUPPORTED).  No counterpart in the reference (tests/test_gpu_reproj_surface.py
 * holds it to a float64 oracle of the formula).
 * ------------------------------------------------------------------------------- */
int k2b_fit_image(const k2b_model *model, const k2b_prior *prior, const k2b_fit_config *cfg,
                  int32_t num_frames, int32_t num_targets, const int32_t *model_joint_index,
                  const float *keypoints, const float *conf,
                  const float *global_orient_in, const float *body_pose_in, const float *betas_in,
                  const float *transl_in, const float *preserve_pose, const float *transl_prior_target,
                  float *global_orient_out, float *body_pose_out, float *betas_out, float *transl_out,
                  float *loss_out, float *grad_out, void *stream) K2B_SINCE(1, 9);

/* ---------------------------------------------------------------------------------
 * k2b_fit_multiview (ABI 1.10) — B independent frames of 2D keypoints seen by C calibrated cameras at once, under Adam.  Camera c
 * has a row-major world-to-camera matrix R_c, a translation t_c and focals (fx_c, fy_c); with p the posed model joint of
 * target k and transl the body's WORLD translation:
 *     q   = R_c (p + transl) + t_c
 *     e_x = fx_c q_x / q_z - u'_ck,   e_y = fy_c q_y / q_z - v'_ck     (u', v': pixels minus THAT camera's principal point)
 *     joint loss = w_j^2 sum_c sum_k conf_ck^2 (gmof(e_x, sigma) + gmof(e_y, sigma))
 *     d loss / d p = sum_c R_c^T (g_x, g_y, g_z)_c                       ((g_x, g_y, g_z)_c: the single-view form's, on q)
 * Every other term, optimize_mask, freeze_betas, transl_prior_weight and the loss convention are k2b_fit_world's; so is the
 * argument list from global_orient_in on, with its aliasing rule (Conventions; tests/test_gpu_caller_buffers.py).  The conventions of projection = 1 hold per pair (c, k): q_z is divided by as it
 * stands (IEEE division; a point behind a camera is legal and finite), a pair of confidence 0 is selected out and contributes
 * exactly nothing whatever its depth, a pair of non-zero confidence at q_z = 0 makes that frame non-finite and no other.  The
 * views are summed in the order 0 .. C - 1 in every launch shape: a frame's result is bit-identical in any batch and at any
 * position.  R_c need only be finite: the gradient is the exact chain rule for any linear map, and orthonormality is the
 * caller's business (the Python layer checks it).
 *   cameras    HOST [C], read during the call (they travel by value in the kernel arguments: all iterations in ONE launch, no
 *              upload and no synchronisation beyond k2b_fit_world's Adam table)
 *   keypoints  dev [B][C][K][3]: rows (u', v', ignored)
 *   conf       dev [C][K], or [B][C][K] with cfg->conf_per_frame; NULL = ones
 * 1 <= num_views <= 8; cfg->projection must be 1; cfg->focal is not read.  Refused before anything is queued, outputs
 * untouched: num_views outside 1..8, a non-finite camera field, a focal that is not finite and positive, projection != 1
 * (K2B_ERR_INVALID_ARGUMENT); surface targets (a model index >= J), a 24-joint model without a scan plan or created under
 * K2B_FIT_SCAN64=1, a translation prior on the tree kernel (K2B_ERR_UNSUPPORTED).  No counterpart in the reference
 * (tests/test_gpu_multiview_term.py holds it to a float64 oracle of the formula).
 * ------------------------------------------------------------------------------- */
typedef struct k2b_camera { /* K2B_SINCE(1, 10) */
    float rotation[9];    /* R_c, row-major: camera = R_c world + t_c */
    float translation[3]; /* t_c */
    float focal[2];       /* fx_c, fy_c in pixels: finite and positive */
} k2b_camera;
/* sizeof(k2b_camera) as the library was built (bindings check their mirror against it). */
uint32_t k2b_camera_size(void) K2B_SINCE(1, 10);
int k2b_fit_multiview(const k2b_model *model, const k2b_prior *prior, const k2b_fit_config *cfg,
                      int32_t num_frames, int32_t num_views, const k2b_camera *cameras,
                      int32_t num_targets, const int32_t *model_joint_index,
                      const float *keypoints, const float *conf,
                      const float *global_orient_in, const float *body_pose_in, const float *betas_in,
                      const float *transl_in, const float *preserve_pose, const float *transl_prior_target,
                      float *global_orient_out, float *body_pose_out, float *betas_out, float *transl_out,
                      float *loss_out, float *grad_out, void *stream) K2B_SINCE(1, 10);

/* ---------------------------------------------------------------------------------
 * k2b_fit_multiview_sequences (ABI 1.11) — warm-start chains over videos of a calibrated rig: k2b_fit_image_sequences' chain
 * under the joint term of k2b_fit_multiview, S ragged videos side by side in ONE launch (S = 1: the single video).  Argument
 * conventions as k2b_fit_image_sequences (packed rows, host lengths / offsets, *_in one row per sequence, loss_out may be
 * NULL, followup_freeze_betas), plus the rig of k2b_fit_multiview.
 *   cameras    HOST [C], ONE rig shared by all sequences and all frames, read during the call (by value in the kernel
 *              arguments: nothing is uploaded for them and nothing synchronises; the slot table of the sequences goes up through
 *              the calling thread's pinned staging, as for the other ragged entries)
 *   keypoints  dev [sum T][C][K][3]: rows (u', v', ignored), pixels minus THAT camera's principal point
 *   conf       dev [C][K], or [sum T][C][K] with cfg->conf_per_frame; NULL = ones
 *   transl_*   the body's WORLD translation
 * 1 <= num_views <= 8; cfg->projection must be 1; cfg->focal is not read.  Step 0 of a sequence is k2b_fit_multiview under
 * `cfg`: cfg->num_iters iterations, no preserve term.  Step t > 0 starts from step t - 1's RESULT, preserves that result's
 * body pose with cfg->pose_preserve_weight, runs followup_iters iterations with a fresh Adam state and, with
 * followup_freeze_betas != 0, holds the shape as cfg->freeze_betas = 1 would (24-joint models hold all betas, SMPL-H / SMPL-X
 * the first num_betas_prior coefficients - the expression stays free); cfg->freeze_betas itself applies to every step.  A
 * sequence of length 1 is the first-frame fit; a sequence of length 0 writes nothing.  loss_out is every frame's
 * last-iteration loss before its step, preserve term included.
 * Guarantees (tests/test_gpu_multiview_chain.py):
 *   - a sequence's rows are bit-identical to that sequence fitted alone, in any order and among any neighbours;
 *   - they are bit-identical to a host loop of k2b_fit_multiview calls that hands each result on (frame t > 0: start and
 *     preserve_pose = frame t - 1's result, followup_iters iterations, freeze_betas for the follow-up freeze);
 *   - the views are summed in the order 0 .. C - 1;
 *   - a non-finite keypoint stays in its own SEQUENCE: the frames before it are untouched, the frame itself reports a
 *     non-finite loss, and the frames behind it in that sequence may be non-finite (a warm start inherits).
 * Refused before anything is queued, outputs untouched: num_views outside 1..8, a non-finite camera field, a focal that is not
 * finite and positive, projection != 1, cfg->transl_prior_weight != 0, bad lengths / offsets, bad followup_iters, 2^27 or more
 * target rows (sum T x C x K) on a 24-joint model (K2B_ERR_INVALID_ARGUMENT); surface targets (a model index >= J), a 24-joint
 * model without a scan plan or created under K2B_FIT_SCAN64=1 (K2B_ERR_UNSUPPORTED).  Adam only.
 * ------------------------------------------------------------------------------- */
int k2b_fit_multiview_sequences(const k2b_model *model, const k2b_prior *prior, const k2b_fit_config *cfg,
                                int32_t num_sequences, const int32_t *lengths, const int32_t *offsets,
                                int32_t followup_iters, int32_t followup_freeze_betas,
                                int32_t num_views, const k2b_camera *cameras,
                                int32_t num_targets, const int32_t *model_joint_index,
                                const float *keypoints, const float *conf,
                                const float *global_orient_in, const float *body_pose_in, const float *betas_in,
                                const float *transl_in,
                                float *global_orient_out, float *body_pose_out, float *betas_out, float *transl_out,
                                float *loss_out, void *stream) K2B_SINCE(1, 11);

/* ---------------------------------------------------------------------------------
 * k2b_shape_pass_lbfgs (ABI 1.3) — the shape pre-pass of many sequences together (reference core/shape.py:10-115,
 * optimize_shape_multi_frame: torch.optim.LBFGS([betas], max_iter, lr, strong_wolfe) per sequence).  Sequence s owns frames
 * seq_offsets[s] .. seq_offsets[s + 1] - 1 (dev int32 [S + 1]); per frame the kinematic targets j3d dev [N][K][3], conf dev
 * [N][K] (or NULL), the fixed pose global_orient dev [N][3] / body_pose dev [N][3(J-1)] and the target root root_targets dev
 * [N][3].  The loss of a sequence is the sum over its frames of the evaluate-only fit under `cfg` (the caller sets sigma, the
 * weights and the shape prior) at shape = [betas | 0] and the root-aligned translation root_target - (J_template[root_joint] +
 * J_dirs[root_joint] betas); the gradient takes the chain rule through that alignment.  betas_in / betas_out dev
 * [S][num_free_betas].  Per round one small prep launch, ONE evaluate-only fit launch over all N frames, one fixed-order
 * per-sequence reduction and the device L-BFGS step (one instance per sequence); only launches are queued.  A sequence's result
 * does not depend on the others; a sequence without frames (seq_offsets[s] == seq_offsets[s + 1]) has its own betas row and
 * returns betas_in (tests/test_gpu_call_history.py).  Kinematic targets only.
 * ------------------------------------------------------------------------------- */
int k2b_shape_pass_lbfgs(const k2b_model *model, const k2b_prior *prior, const k2b_fit_config *cfg,
                         int32_t num_sequences, const int32_t *seq_offsets, int32_t num_frames, int32_t num_targets,
                         const int32_t *model_joint_index, const float *j3d, const float *conf,
                         const float *global_orient, const float *body_pose, const float *root_targets, int32_t root_joint,
                         int32_t num_free_betas, const float *betas_in, float *betas_out, int32_t max_iter,
                         int32_t history_size, double lr, double tolerance_grad, double tolerance_change, void *stream);

int k2b_fit_sequences_lbfgs(const k2b_model *model, const k2b_prior *prior, const k2b_fit_config *cfg,
                            int32_t num_sequences, const int32_t *lengths, const int32_t *offsets,
                            int32_t num_targets, const int32_t *model_joint_index,
                            const float *j3d, const float *conf,
                            const float *global_orient_in, const float *body_pose_in, const float *betas_in,
                            const float *transl_in,
                            float *global_orient_out, float *body_pose_out, float *betas_out, float *transl_out,
                            float *loss_out, int32_t first_iters, int32_t followup_iters, int32_t history_size,
                            double lr, double tolerance_grad, double tolerance_change, void *stream);

/* ---------------------------------------------------------------------------------
 * k2b_lbs — full SMPL forward.  Replaces `self.smpl(**kwargs)` (smplx `SMPL.forward`,
 * call sites world_space.py:34,192,278; engine.py:114) for a batch:
 *   joints_out dev [B][J+E+L][3], vertices_out dev [B][V][3] (NULL: joints only; the E
 *   vertex-selected joints and the 3L landmark vertices are then skinned alone).  transl may be NULL
 *   (no translation).  Landmarks are combined from the translated vertices.
 * Models: 17-24 joints (SMPL) and 49-56 joints (SMPL-H / SMPL-X) with 1 <= NB <= 32 shape coefficients (betas | expression);
 * any other joint count: K2B_ERR_UNSUPPORTED.
 * ------------------------------------------------------------------------------- */
int k2b_lbs(const k2b_model *model, int32_t num_frames, const float *global_orient,
            const float *body_pose, const float *betas, const float *transl,
            float *joints_out, float *vertices_out, void *stream);

/* ---------------------------------------------------------------------------------
 * k2b_lbs_backward (ABI 1.4) — the vector-Jacobian product of k2b_lbs: what `loss.backward()` through `self.smpl(**kwargs)`
 * computes for a loss over the model's joints and / or vertices.  Parameters as k2b_lbs (transl may be NULL; it is not read:
 * the forward is affine in it).
 *   grad_joints   dev [B][J+E+L][3] or NULL: cotangent of joints_out.  The J kinematic rows feed the chain, an extra-vertex row
 *                 adds to its vertex, a landmark row adds b_k x itself to its three vertices; every row adds to grad_transl
 *                 (a landmark's with the sum of its weights, as the forward combines translated vertices)
 *   grad_vertices dev [B][V][3] or NULL: cotangent of vertices_out.  NULL: only the vertices that extra joints and landmarks name
 *                 are visited (none: no vertex pass at all)
 *   grad_global_orient [B][3], grad_body_pose [B][3(J-1)], grad_betas [B][NB], grad_transl [B][3]: dev, each may be NULL (not
 *                 wanted; the others are unchanged by that).  grad_transl is defined whether or not the forward had a transl.
 * Everything is recomputed from the parameters: the forward saves nothing.  Stream-ordered, launches only; scratch (feature rows,
 * transforms and B x G x (12 (J + 1) + padded features) floats of partial sums, G <= 16 a function of V) is stream-ordered too.
 * The FIRST call on a model uploads a small table of its surface rows (blocking).  Sums have one fixed order: a frame's
 * gradient is bit-identical from run to run, in any batch, at any position.  Models as k2b_lbs; other joint counts:
 * K2B_ERR_UNSUPPORTED.  NULL model / parameter buffer, or both cotangents NULL: K2B_ERR_INVALID_ARGUMENT before any launch.
 * num_frames == 0 is a no-op.
 * ------------------------------------------------------------------------------- */
int k2b_lbs_backward(const k2b_model *model, int32_t num_frames, const float *global_orient,
                     const float *body_pose, const float *betas, const float *transl,
                     const float *grad_joints, const float *grad_vertices,
                     float *grad_global_orient, float *grad_body_pose, float *grad_betas, float *grad_transl,
                     void *stream) K2B_SINCE(1, 4);

/* Development: copies the first nbytes (<= 64 KiB) of the model's scratch row (where diagnostic builds leave their
 * in-kernel time stamps) to HOST memory; synchronises the device. */
int k2b_debug_read_dump(const k2b_model *model, void *host, int64_t nbytes);

/* Development (ABI 1.5): the device L-BFGS state machine alone, fed a CALLER'S closure results - what k2b_fit_world_lbfgs runs
 * behind its own closure, one round per call, so that tests can drive every branch of the optimiser with chosen (loss, gradient)
 * sequences.  No model is involved; the sizes are arguments.
 * k2b_debug_lbfgs_state_layout: for num_frames optimisers of num_params = 3 + pose_dim + num_betas + 3 parameters and `history`
 *   pairs, the bytes of the state buffer, the byte offsets of its integer and vector blocks, and the row lengths of the two scalar
 *   blocks: doubles [num_frames][doubles_per_frame] at offset 0, int32 [num_frames][ints_per_frame] at offset_ints (column order:
 *   csrc/k2b_lbfgs_plan.h).  Host only.
 * k2b_debug_lbfgs_step: advances the num_frames optimisers by ONE closure result.
 *   global_orient [B][3], body_pose [B][pose_dim], betas [B][num_betas], transl [B][3] (dev, in / out): the parameter arrays the
 *     closure would read.  Before the first call they hold the start; after a call, the point whose loss and gradient the next
 *     call expects (a finished frame: its final point).
 *   loss dev [B], grad dev [B][num_params] (layout of grad_out above): the closure's result at the arrays' current point.
 *   state: dev, 16-byte aligned, state_bytes >= the layout's bytes, caller-owned, ZEROED before the first call (all frames in
 *     phase INIT) and otherwise only ever written by this entry.
 *   history: ring slots, used as given (k2b_fit_world_lbfgs passes min(history_size, max_iter)); max_eval = max_iter * 5 / 4.
 *   finalize != 0: no result is consumed (loss / grad may be NULL); every frame's ACCEPTED point goes into the parameter arrays
 *     (what the fit does behind its last round); the state is not written.
 *   max_staged_pairs: cap on the history pairs staged in LDS (< 0: none; results do not depend on it).
 * Everything is checked on the host before any launch: num_params outside [8, 256] or history outside [1, 100]:
 * K2B_ERR_UNSUPPORTED; pose_dim / num_betas < 1, max_iter outside [1, 10000] (as the fit entries), lr <= 0, a negative
 * tolerance, a NULL buffer, a state buffer too small or misaligned: K2B_ERR_INVALID_ARGUMENT.  num_frames == 0 is a no-op.  Stream-ordered, one launch. */
int k2b_debug_lbfgs_state_layout(int32_t num_frames, int32_t num_params, int32_t history, int64_t *state_bytes,
                                 int64_t *offset_ints, int64_t *offset_vectors, int32_t *doubles_per_frame,
                                 int32_t *ints_per_frame) K2B_SINCE(1, 5);
int k2b_debug_lbfgs_step(int32_t num_frames, int32_t pose_dim, int32_t num_betas, float *global_orient, float *body_pose,
                         float *betas, float *transl, const float *loss, const float *grad, int32_t max_iter,
                         int32_t history, double lr, double tolerance_grad, double tolerance_change, void *state,
                         int64_t state_bytes, int32_t finalize, int32_t max_staged_pairs, void *stream) K2B_SINCE(1, 5);

/* ---------------------------------------------------------------------------------
 * Vertex-selected joints in the loss, stand-alone pieces.  `target_model_indices` of the reference
 * (world_space.py:198-201) may name smplx's "extra" joints, which are single mesh vertices
 * (index J + e, e < E).  k2b_fit_world handles them itself (see model_joint_index above); these
 * two entry points expose the pieces it is made of, for optimisers that run on the host (the
 * L-BFGS branch may call k2b_fit_world in evaluate-only mode instead) and for the parity tests.
 *
 * k2b_vertex_term: loss [B] and gradient [B][3 + 3(J-1) + NB + 3] (layout of grad_out above)
 *   of  joint_loss_weight^2 conf_e^2 sum_xyz gmof(vertex_e + transl - target_e)  over the E_sel
 *   selected extra joints; extra_index HOST int32 [E_sel] in [0, E); targets dev [B][E_sel][3];
 *   conf dev [E_sel] or NULL.  At most 32 selected joints per call.
 * k2b_adam_step: torch.optim.Adam single-tensor update of n floats for step t = 1, 2, ...
 *   (bias corrections formed in double like the fused kernel's table); m, v are the caller's
 *   state buffers (zero before the first step).  eps as k2b_fit_config::adam_eps: a normal positive float32, else
 *   K2B_ERR_INVALID_ARGUMENT.  The first moment follows both forms of torch's lerp (from 1 - beta1 = 0.5 on:
 *   g - (g - m) beta1), so beta1 = 0 gives m = g exactly.
 * ------------------------------------------------------------------------------- */
int k2b_vertex_term(const k2b_model *model, int32_t num_frames, int32_t num_selected,
                    const int32_t *extra_index, const float *targets, const float *conf,
                    float sigma, float joint_loss_weight, const float *global_orient,
                    const float *body_pose, const float *betas, const float *transl,
                    float *loss_out, float *grad_out, void *stream);
/* k2b_surface_term: k2b_vertex_term generalised to surface targets (extra joints and landmarks):
 *   model_joint_index HOST int32 [T], each in [J, J+E+L); targets dev [B][T][3]; conf dev [T], or [B][T] with
 *   conf_per_frame != 0, or NULL.  At most 128 targets per call.  Loss [B] and gradient [B][3 + 3(J-1) + NB + 3]. */
int k2b_surface_term(const k2b_model *model, int32_t num_frames, int32_t num_selected,
                     const int32_t *model_joint_index, const float *targets, const float *conf,
                     int32_t conf_per_frame, float sigma, float joint_loss_weight, const float *global_orient,
                     const float *body_pose, const float *betas, const float *transl,
                     float *loss_out, float *grad_out, void *stream);
/* k2b_surface_term_image (ABI 1.9): k2b_surface_term under perspective projection (k2b_fit_image has the formula).  targets dev
 *   [B][T][3] rows (u - cx, v - cy, ignored); sigma in pixels; focal HOST [2] = (fx, fy), finite and > 0 (else
 *   K2B_ERR_INVALID_ARGUMENT).  Limits, outputs and stream behaviour as k2b_surface_term. */
int k2b_surface_term_image(const k2b_model *model, int32_t num_frames, int32_t num_selected,
                           const int32_t *model_joint_index, const float *targets, const float *conf,
                           int32_t conf_per_frame, float sigma, float joint_loss_weight, const float focal[2],
                           const float *global_orient, const float *body_pose, const float *betas, const float *transl,
                           float *loss_out, float *grad_out, void *stream) K2B_SINCE(1, 9);
int k2b_adam_step(int64_t n, float *params, const float *grad, float *m, float *v, int32_t step,
                  double step_size, double beta1, double beta2, double eps, void *stream);

/* ---------------------------------------------------------------------------------
 * k2b_angular_error_deg — the evaluation metric behind MPJAE.  Replaces
 * `compute_angular_error_deg` (reference cli/eval.py:131-140, with `rotvec_to_rotmat`
 * :88-128) for n pairs of axis-angle rotations:
 *   pred, gt dev [n][3]; err_deg_out dev [n] = geodesic angle in degrees, clipped like
 *   the reference (cos in [-1 + 1e-6, 1 - 1e-6]).  n == 0 is a no-op.
 * ------------------------------------------------------------------------------- */
int k2b_angular_error_deg(int64_t n, const float *pred_rotvec, const float *gt_rotvec,
                          float *err_deg_out, void *stream);

/* ---------------------------------------------------------------------------------
 * k2b_point_error (ABI 1.6) — the positional metrics of a fit: MPJPE (align_mode 0, or 1 after a translation), PA-MPJPE
 * (align_mode 3) and PVE (the same over vertices).  For each frame b of num_frames, two point sets x = pred[b], y = gt[b]:
 *     err[b] = sum_i w_i |a(x_i) - y_i| / sum_i w_i         (a weighted mean of Euclidean distances, not an RMS)
 *   pred, gt dev [B][N][3]; weights dev [N] shared by all frames, or [B][N] with weights_per_frame != 0, non-negative;
 *   NULL = ones.
 *   align_mode 0: a(x) = x.   1: a(x) = x + (ybar - xbar), the weighted centroids.
 *              2: a(x) = R x + t, the rotation R in SO(3) and t that minimise sum w |R x + t - y|^2 (Kabsch).
 *              3: a(x) = s R x + t (Umeyama); R is always a proper rotation, so a mirrored set is not aligned by a reflection.
 *   err_out dev [B];  per_point_out dev [B][N] or NULL: the unweighted distances |a(x_i) - y_i|;
 *   transform_out dev [B][13] or NULL: s, R row-major, t (modes 0 and 1: s = 1, R = I and the t that was used).
 * Corner cases: all weighted points of x coincide (or N == 1): R = I, s = 1, t = ybar - xbar.  A frame whose weights sum to 0:
 * err 0, distances 0, the identity transform.  A non-finite input makes that frame's outputs non-finite and no other frame's.
 * Centroids, covariance, decomposition (Horn's quaternion form, a fixed number of Jacobi sweeps) and residuals are float64, the
 * results rounded to float32 once.  Every sum has one fixed order: a frame's outputs are bit-identical from run to run and do
 * not depend on num_frames or on the frame's position.  1 <= N <= 2^20; up to 256 points four frames share a workgroup, beyond
 * that a frame has its own, and at most 2^24 - 1 workgroups fit the launch: otherwise K2B_ERR_UNSUPPORTED.  N < 1, B < 0, an
 * align_mode outside 0..3, a NULL pred / gt / err_out: K2B_ERR_INVALID_ARGUMENT before any HIP call.  num_frames == 0 is a
 * no-op.  Stream-ordered, one launch, no allocation, no synchronisation.
 * ------------------------------------------------------------------------------- */
int k2b_point_error(int32_t num_frames, int32_t num_points, const float *pred, const float *gt,
                    const float *weights, int32_t weights_per_frame, int32_t align_mode,
                    float *err_out, float *per_point_out, float *transform_out, void *stream) K2B_SINCE(1, 6);

/* ---------------------------------------------------------------------------------
 * IK-GAT rotation regressor — inference of the reference's learned estimator
 * (core/estimators/ikgat/: gan_regressor.py:39-126, inference.py:39-43 and 83-120,
 * utils.py:13-52) in eval mode.  Per frame: joint positions minus joint 0 (plus the 6-D form
 * of the input quaternions when input_dim == 9) -> J unit quaternions, xyzw, qw >= 0.
 *
 * k2b_ikgat_create: HOST pointers, copied.
 *   parents [J]: parent of each joint, negative = none; edges run both ways between a joint and its
 *     parent; with no parent >= 0 at all the graph is the chain i <-> i+1 (gan_regressor.py:16-36).
 *     Self loops are removed and one is added per joint (PyG GATConv), so a joint that is its own parent keeps one.
 *     J == 1 is accepted although the reference cannot run it (its edge tensor is malformed there): the graph
 *     is the self loop only, so every attention weight is 1 and the joint sees its own features.
 *   weights [num_weights] float32: the state dict's tensors, row-major, concatenated in this order
 *   (H = hidden_dim, H2 = H / 2, IN = input_dim; the table the library reads is ikgat_segment in csrc/k2b_ikgat_plan.h,
 *   and num_weights is its sum):
 *     input_proj.weight [H][IN], input_proj.bias [H], joint_pos_embed.weight [J][H],
 *     residual_proj.weight [H][IN], residual_proj.bias [H],
 *     for each layer l: gat_layers.l.lin.weight [H][H], gat_layers.l.att_src [H], gat_layers.l.att_dst [H],
 *       gat_layers.l.bias [H], layer_norms.l.weight [H], layer_norms.l.bias [H],
 *     output_head.0.weight [H2][H], output_head.0.bias [H2], output_head.2.weight [H2], output_head.2.bias [H2],
 *     output_head.4.weight [6][H2], output_head.4.bias [6].
 *   Supported: 1 <= J <= 64, H a multiple of 16 and <= 256, num_heads dividing H, 1 <= num_layers <= 8,
 *   input_dim 3 or 9, and one frame's working set within 160 KiB of LDS; anything else K2B_ERR_UNSUPPORTED.
 *   A parent >= J or a num_weights that does not match the dimensions: K2B_ERR_INVALID_ARGUMENT.
 * k2b_ikgat_predict: positions dev [num_frames][J][3]; quat_in dev [num_frames][J][4] xyzw (input_dim 9;
 *   ignored and may be NULL for input_dim 3); quat_out dev [num_frames][J][4].
 *   chain == 0: the frames are independent.  chain != 0 (input_dim 9): frame 0 reads quat_in[0], frame t > 0
 *   reads frame t-1's output (warm-started sequence, one workgroup, one launch; only quat_in[0] is read); the result
 *   is bit-identical to num_frames calls with chain == 0 and num_frames == 1 that pass each output on.
 *   A frame's outputs do not depend on num_frames or on its position in the batch.  num_frames == 0 is a no-op.
 * ------------------------------------------------------------------------------- */
int k2b_ikgat_create(k2b_ikgat **out, int32_t num_joints, int32_t input_dim, int32_t hidden_dim,
                     int32_t num_layers, int32_t num_heads, const int32_t *parents, const float *weights,
                     int64_t num_weights);
void k2b_ikgat_destroy(k2b_ikgat *net);
int k2b_ikgat_predict(const k2b_ikgat *net, int32_t num_frames, const float *positions, const float *quat_in,
                      int32_t chain, float *quat_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* K2B_H */
