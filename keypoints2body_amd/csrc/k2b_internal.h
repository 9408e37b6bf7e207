// Internal declarations shared by the HIP translation units of libk2b.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "k2b_device.h"
#include "k2b_launch_plan.h"   // (and k2b_layout.h: kFitJoints, kPrior*, the fit kernel's LDS layout)
#include "k2b_lbfgs_plan.h"    // kLbfgsMaxHistory, lbfgs_state_bytes / lbfgs_state_rows, the schedule and the workspace maps
#include "k2b_ikgat_plan.h"    // the IK-GAT set-up: weight image, LDS map, launch
#include "k2b_lbs_plan.h"      // LbsRoute, the stream kernels' k-step counts, lbs_frames_padded, the sizes and passes of the LBS pair

namespace k2b {

constexpr int kMaxJoints = 64;
// The fit kernels' joint term has two forms, the 3D residual and the perspective reprojection of k2b_fit_config::projection.  The
// projected instantiations carry this bit in their first template argument (the shape-coefficient capacity, <= 32).
constexpr int kProjForm = 256;
// A third form (k2b_fit_multiview): the reprojection residual summed over up to kMaxViews calibrated cameras, a run-time loop over
// FitArgs::view inside the joint term.  It rides in the first template argument as kProjForm does (never together with it).
constexpr int kViewsForm = 512;
// The multi-view form inside a warm-start chain (k2b_fit_multiview_sequences): a bit of the fused kernel's first template argument
// beside kViewsForm, split shape only - the instantiations for independent frames stay the code they were.  (The tree kernel has
// its CHAIN parameter.)
constexpr int kViewsChainForm = 1024;
constexpr int kFormMask = kProjForm - 1;      // the capacity under the form bits
// one camera of a multi-view call as the kernels read it (k2b.h, k2b_camera): q = r (p + transl) + t, pixels = (fx q_x, fy q_y) / q_z
struct FitView { float r[9], t[3], fx, fy; };
// the 64 x 64 core of every component as MFMA A fragments (f16 hi / lo, see k2b_api_prior.hip):
//   [m][tile 4][ks0 hi, ks1 hi, ks0 lo, ks1 lo][64 lanes][8 halfs]
constexpr int kPriorFrag32Halfs = kPriorMaxGauss * 4 * 4 * 64 * 8;

// Kernel arguments of the fused fit (passed by value).
// Arguments of the device L-BFGS (k2b_lbfgs.hip); defined here because the fused fit kernel carries a copy (FitArgs::lbv).
struct LbfgsArgs {
    int B, P, D, NB, H;                  // frames, parameters per frame (3 + D + NB + 3), pose / shape widths, history slots
    int max_iter, max_eval;
    double lr, tol_g, tol_c;             // lr, tolerance_grad, tolerance_change
    float *go, *bp, *be, *tr;            // the point to evaluate next, in the closure's own parameter arrays (in / out)
    const float *loss_in, *grad_in;      // closure result at that point: [B], [B][P]
    double* sd;                          // state: scalars, integers, vectors (lbfgs_state_bytes)
    int* si;
    float* sv;
    int finalize;                        // 1: no result consumed, every frame's accepted point -> parameter arrays
};

struct FitArgs {
    // model (device)
    // tree tables are indexed by LANE: lanes follow the model's scan plan (reversed DFS order with holes, k2b_scan_plan.h) or,
    // without one, the DFS pre-order of the kinematic tree
    const float* dt;            // [64][3]     J_template[j] - J_template[parent]  (root: J_template[0])
    const float* dd;            // [64][3][16] same for J_dirs, zero padded
    const int* lane_tab;        // [64][kLaneTabStride]
    int num_rounds;             // pointer-doubling rounds needed by the targeted joints of this call
    int num_betas;
    int scan64;                 // 0: the lane tables carry a scan plan (fp32 chain / end scans); 1: DFS order, fp64 prefix differences
    // prior (device)
    const float* pa_image;      // LDS image, kPriorImageFloats floats (see k2b_api_prior.hip)
    const void* pa_frag32;      // kPriorFrag32Halfs f16
    const float* row_const;     // [8][64] per-lane rim constants: P_BB row (5), (P mu)_B, (P_BA mu_A), mu_B
    const float* neg_log_nllw;  // [8]
    float inv_scale[kPriorMaxGauss];  // 1 / (power-of-two scale of component m's fragments)
    int num_gauss;
    int frames_per_wg;          // set by launch_fit_world
    // call (device unless noted)
    int num_frames, num_targets;
    int lane_target[kFitJoints];  // target index fitted by joint j, or -1
    const float* j3d;
    const float* conf;
    int conf_per_frame;
    const float *go_in, *bp_in, *be_in, *tr_in, *preserve, *tr_prior;
    float *go_out, *bp_out, *be_out, *tr_out, *loss_out, *grad_out;
    const float2* adam_coef;    // [num_iters] {lr / (1 - b1^t), sqrt(1 - b2^t)}
    int num_iters;
    float one_minus_beta1, beta2, one_minus_beta2, eps;
    float sigma, joint_w, pose_prior_w, angle_w, shape_w, preserve_w;
    int freeze_betas;
    int opt_mask;               // bit 0 global_orient, 1 body_pose, 2 betas, 3 transl
    float transl_prior_w;
    int angle_index[4];
    float angle_sign[4];
    int num_cus;
    int chain_len, chain_iters; // warm-start chain: num_frames SEQUENCES of chain_len frames each (1: independent frames)
    int force_shape;            // ForceShape (k2b_launch_plan.h): automatic = chosen by the batch size, or k2b_fit_config::debug_launch_shape
    // L-BFGS step as a prologue of the closure's own launch (k2b_lbfgs.hip), an LbMode: none; step = every frame's row wave first
    // consumes the PREVIOUS launch's loss / gradient (lb->loss_in / grad_in) and writes the next point into the parameter arrays, then
    // the launch evaluates it; finalize = the finalise step (accepted points into the parameter arrays), then the evaluation.  Split shape only.
    int lb_mode;
    LbfgsArgs lbv;              // the optimiser's arguments (by value: no device copy to keep in step)
    // LbMode::persistent: the whole fit in ONE launch (num_iters = rounds + 1 closures; at most two frames per workgroup); the row wave
    // writes each closure's result to lb_loss / lb_grad (= lb->loss_in / grad_in), lb_history = lb->H (host copies: no device read)
    const float *lb_loss, *lb_grad;
    int lb_history;
    int lb_chain_max_iter;      // LbMode::persistent with chain_len > 1 (the default sequence mode in ONE launch): max_iter of the follow-up frames (lbv: the first's)
    // ragged chains (chain_len > 1): NULL = every slot s is sequence s with chain_len frames at rows s * chain_len; else [slot][4] =
    // {row of the start parameters, first frame row, frame count >= 1, 0} (device).  A workgroup runs as many steps as its
    // longest slot; a slot whose sequence has ended takes the barriers and writes nothing.
    const int* chain_meta;
    // joint term (k2b_fit_config::projection, focal): 0 = 3D residual, 1 = perspective reprojection of centred pixel targets.  Behind
    // everything else: the 3D instantiations never read them, and their kernel-argument offsets stay what they were.
    int projection;
    float focal_x, focal_y;
    // projected chains (k2b_fit_image_sequences): 1 = the steps > 0 of a chain hold the shape group as freeze_betas does (a video's
    // shape is estimated on its first frame).  Last, and read by the projected instantiations only: every other argument keeps its offset.
    int chain_freeze_shape;
    // several views (k2b_fit_multiview; 0 = one of the forms above): targets [frame][view][target][3], conf [view][target] or
    // [frame][view][target], the cameras by value.  Behind everything else and read by the kViewsForm instantiations only.
    int num_views;
    FitView view[kMaxViews];
};

// chain_frames: the frames of all sequences of a chain (chain_len > 1) whose slots come from chain_meta, read with num_views > 0 only
hipError_t launch_fit_world(const FitArgs& a, hipStream_t stream, long long chain_frames = 0);

// Kernel arguments of the fused fit for large trees (k2b_fit_tree.hip: 25..64 joints, SMPL-H / SMPL-X).
struct FitTreeArgs {
    // model (device), indexed by LANE (DFS pre-order of the kinematic tree)
    const float* dt;            // [64][3]      rest offset from the parent at shape 0 (root: its rest joint)
    const float* dd;            // [64][3][32]  the same for the shape directions, zero padded
    const int* tab;             // [64][8]: joint, parent lane, subtree size, depth, prior source lane, prior source
                                //          component, first prior dimension of this joint (-1: none), unused
    const int* anc;             // [64][4]: lane of the ancestor 1, 2, 4, 8 levels up, or 63 (a non-joint lane: identity)
    int num_joints, num_shape, num_rounds;   // pointer-doubling rounds the targeted joints need: 2^rounds > their depth
    // prior (device): the mixture folded to its first prior_dims <= 64 dimensions (see k2b_fit_tree.hip)
    const k2b_half* pfrag;      // [8][4 tiles][ks0 hi, ks1 hi, ks0 lo, ks1 lo][64 lanes][8]: the 64 x 64 core of every (scaled) precision
                                // matrix as v_mfma_f32_16x16x32_f16 A fragments - the image k2b_fit.hip uses (k2b_prior::frag32)
    float inv_scale[8];         // per component: 1 / (power-of-two scale of its fragments)
    const float *ph, *pb, *pmu; // [M][64]          h = b - A mu, b, mu
    const float* pcl;           // [M]              0.5 c_m - log(nll weight)
    int num_gauss, prior_dims;
    // call
    int num_frames, num_targets;
    int lane_target[64];        // target index fitted by the joint of lane l, or -1
    const float* j3d;
    const float* conf;
    int conf_per_frame;
    const float *go_in, *bp_in, *be_in, *tr_in, *preserve;
    float *go_out, *bp_out, *be_out, *tr_out, *loss_out, *grad_out;
    const float2* adam_coef;    // [num_iters] {lr / (1 - b1^t), sqrt(1 - b2^t)}
    int num_iters;
    float one_minus_beta1, beta2, one_minus_beta2, eps;
    float sigma, joint_w, pose_prior_w, angle_w, shape_w, preserve_w;
    int freeze_betas, num_betas_prior;   // the shape prior and freeze_betas apply to the first num_betas_prior coefficients
    int opt_mask;               // bit 0 global_orient, 1 body_pose, 2 shape coefficients, 3 transl
    int angle_index[4];
    float angle_sign[4];
    int chain_len, chain_iters;  // warm-start chain: num_frames SEQUENCES of chain_len frames each (<= 1: independent frames)
    const int* chain_meta;       // ragged chains: as FitArgs::chain_meta
    int comp_waves;             // set by launch_fit_tree: 4 = the mixture runs on four dedicated component waves (<= 4 frames per CU)
    int debug_shape;             // TreeShape (k2b_launch_plan.h): automatic = chosen by the batch size; plain / comp_waves force one (tests)
    int projection;              // as FitArgs::projection, focal_x, focal_y
    float focal_x, focal_y;
    int chain_freeze_shape;      // as FitArgs::chain_freeze_shape: steps > 0 freeze the first num_betas_prior coefficients (the expression stays free)
    int num_views;               // as FitArgs::num_views, view
    FitView view[kMaxViews];
};
hipError_t launch_fit_tree(const FitTreeArgs& a, int num_cus, hipStream_t stream);

// Batched shape pre-pass (k2b_shape.hip, k2b_shape_pass_lbfgs): S sequences, sequence s owns frames seq_off[s] .. seq_off[s + 1].
struct ShapePassArgs {
    int S, D, NB, nb;              // sequences, body-pose width, shape coefficients of the model, betas optimised (the first nb)
    const int* seq_off;            // dev [S + 1]
    const float *jt0, *jd0;        // dev: J_template[root] [3], J_dirs[root] [3][NB]
    const float* root_y;           // dev [sum n][3]: target root of every frame
    const float* be_state;         // dev [S][NB]: the optimiser's points (betas in front)
    float *be_f, *tr_f;            // dev [sum n][NB], [sum n][3]: per-frame shape rows and root-aligned translations
    const float *grad_f, *loss_f;  // dev [sum n][3 + D + NB + 3], [sum n]: the evaluate-only launch's results
    float *grad_state, *loss_state; // dev [S][3 + D + NB + 3], [S]: what the L-BFGS step consumes
};
hipError_t launch_shape_prep(const ShapePassArgs& a, hipStream_t stream);
hipError_t launch_shape_reduce(const ShapePassArgs& a, hipStream_t stream);

// Pose set-up for LBS: per frame the relative transforms A_j (3x4) and the feature vector
// X = [vec(R_1..R_{J-1} - I) | beta | 1 | 1] as f16 hi/lo MFMA operands, plus the posed
// kinematic joints (+ transl).
struct PoseArgs {
    const float* j_basis_lane; // [3][1 + NB][64]: J_template (k' = 0) and J_dirs (k' = 1 + k) with the joint as the fastest index, zeros for lanes >= J
    const int* parents;        // [J]
    int num_joints, num_betas, num_out_joints;
    int num_frames, frames_padded;
    int k_steps_x;             // 16-deep k-steps of the vertex GEMM (features)
    const float *go, *bp, *be, *tr;  // tr may be null
    k2b_half *xh, *xl;         // pieces [k_steps_x][frames_padded / 32]
    k2b_half* a2;              // group layout of the tile kernel (see TileArgs)
    int a2_stream_order;       // 1: k-groups of an entry in the stream kernel's order hi.. | PAD | lo.. | ZERO (see StreamArgs)
    float* joints_out;         // [B][num_out_joints][3] (first J rows written) or null
    int xcd_frames;            // set by the launcher: 0 = workgroup b takes frame b; else XCD label b % 8 takes the frames [x, x + 1) * xcd_frames
    int x_fp8;                 // LbsRouteRecord::pose_fp8: the pieces of xl of the 32-deep k-steps 0..kF8PoseSteps - 1 hold the e4m3 strip
                               // [X_hi8 | X_lo8] of the k-step (k2b_lbs_fp8.h) instead of the f16 lo terms; 17-24 joints only
};
hipError_t launch_pose_setup(const PoseArgs& a, int pose_capacity, hipStream_t stream);   // (LbsRouteRecord::pose_capacity)

// ---- tile kernel (k2b_lbs_tile_kernel): 128 frames x 128 vertices per workgroup, persistent ------------------
// Operands of the transform GEMM T = A . W^T in k-GROUPS of 8 joints over 16-row tiles (256 B = [16 rows][8 halfs]):
//   A  [16-frame tile][entry 12][NGP][16][8]   groups: hi_0..hi_{GA-1}, lo_0..lo_{GA-1}, PAD (translation terms), ZERO
//   W  [16-vertex tile][NGP][16][8]            groups: hi_0..hi_{GA-1}, lo_0..lo_{GA-1}, ONES ([1,1,1,0,...] per row), ZERO
//      (the ZERO group only ever meets zeros of A, so its first half per row is free to carry a tag: 1 + output joint of the vertex)
// GA = ceil(J / 8), NGP = 2 GA + 2 (a multiple of 4: whole 1 KiB pieces).  The three f16-split products (hi.hi + hi.lo +
// lo.hi) are ONE contraction over the concatenated group sequences  A: hi | hi | lo | PAD,  W: hi | lo | hi | ONES
// (3 GA + 1 groups, padded to a multiple of four with ZERO): ceil((3 GA + 1) / 4) MFMAs of depth 32 per output tile, no
// padding of J to 16, and the PAD x ONES position adds the frame's translation (three f16 terms) to the entries 3, 7, 11
// inside the GEMM.  (tile_groups_a, tile_ngp: k2b_layout.h)
struct TileArgs {
    const k2b_half *xh, *xl;     // X fragments [k_steps_x][f_tiles]          (pose set-up)
    const k2b_half *a2;          // A groups    [2 f_tiles][12][NGP][16][8]   (pose set-up)
    const k2b_half *pdh, *pdl;   // Pd fragments [k_steps_x][3][v_tiles]      (model)
    const k2b_half *w2;          // W groups    [2 v_tiles][NGP][16][8]       (model)
    int groups_a;                // GA
    int k_steps_x, f_tiles, v_tiles;
    int num_frames, num_out;
    float* out;                  // [B][out_stride][3], rows out_row0 .. out_row0 + num_out - 1
    int out_stride, out_row0;
    float* dump;                 // >= 64 x 3 floats: where lanes without a valid (frame, vertex) put their store
    // vertex-selected output joints (smplx's extra joints) written by the same launch: a vertex whose W row carries "1 + e" in
    // its padding group is stored a second time, to joints_out[frame][joints_row0 + e]; null: no joint copies
    float* joints_out;
    int joints_stride, joints_row0;   // J + E, J
    int num_wgs;                 // grid size (a multiple of 8), set by the launcher
};
hipError_t launch_skin_tiles(const TileArgs& a, int num_cus, hipStream_t stream);

// ---- stream kernels (k2b_lbs_stream.hip): the same tile, Pd global -> registers -------------------------------------------------
// One kernel body (stream_body<S>) behind three entry points, one description S each; the descriptions hold what differs (pose
// k-steps, X resident or in a ring, fragment counts and products, the counted-wait tables) and live in k2b_lbs_stream.hip.
//   k2b_lbs_stream_kernel     17-24 joints, 7 pose k-steps (SMPL)                                      LbsRoute::stream
//   k2b_lbs_stream_f8_kernel  the same with the pose corrections of the k-steps 0..5 as e4m3 MFMAs: 23, 24 joints        LbsRoute::stream, pose_fp8
//   k2b_lbs_stream_x_kernel   49-56 joints, 16 pose k-steps (<= 512 features: SMPL-H, SMPL-X up to 24 shape coefficients) LbsRoute::stream_x
//   k2b_lbs_stream_xw_kernel  49-56 joints, 17 pose k-steps (513-544 features: SMPL-X with 25-32, 56 joints with 16-32)   LbsRoute::stream_xw
// Every other model with 17-24 or 49-56 joints, and any model created under K2B_LBS_TILE=1, runs the tile kernel (the rule and
// the k-step counts kStream*KSteps: k2b_lbs_plan.h, lbs_route).
// Operands (1 KiB pieces = 64 lanes x 8 halfs in v_mfma_f32_16x16x32_f16 operand order: lane = row + 16 k-group), SMPL:
//   X   as for the tile kernel
//   A   [16-frame tile][entry 12][fragment 2]: fragment 0 = k-groups hi_0 hi_1 hi_2 PAD, fragment 1 = lo_0 lo_1 lo_2 ZERO
//       (the pose set-up writes this group order with PoseArgs::a2_stream_order)
//   Pd  [k-step 7][16-vertex tile][coordinate 3][hi | lo]
//   W   [16-vertex tile][3]: [hi | ONES], [hi | tag], [lo | 0]   (tag: 1 + output joint of the vertex, first half of the group)
struct StreamArgs {
    const k2b_half *xh, *xl, *a2, *pd, *w;
    int f32_tiles;               // 32-frame tiles (frames padded / 32)
    int nv16;                    // 16-vertex tiles of the padded vertex set, a multiple of 8
    int num_frames, num_out;
    float* out;
    int out_stride, out_row0;
    float* dump;
    float* joints_out;           // see TileArgs
    int joints_stride, joints_row0;
    int num_wgs;
    // route stream with LbsRouteRecord::pose_fp8 (description SmplF8; k2b_lbs_fp8.h): the lo strips of the k-steps 0..5 of xl and pd are
    // e4m3, and these are the scale exponents of pd's two terms (the model's image: VertexSetImages::pd8_lo_exp, pd8_hi_exp)
    int pose_fp8, pd8_lo_exp, pd8_hi_exp;
};
hipError_t launch_skin_stream(LbsRoute route, const StreamArgs& a, int num_cus, hipStream_t stream);   // one of the three stream routes (stream: a.pose_fp8 picks SmplF8)
// SMPL-X: the same operands with
//   A   [16-frame tile][entry 12][fragment 4]: hi_0-3 | hi_4-6 PAD | lo_0-3 | lo_4-6 ZERO   (a2_stream_order with GA = 7)
//   Pd  [k-step 16][16-vertex tile][coordinate 3][hi | lo]
//   W   [16-vertex tile][5]: hi_0-3, [hi_4-6 | ONES], lo_0-3, [lo_4-6 | 0], [hi_4-6 | tag]
// 49-56 joints with 513-544 features (SMPL-X with 25-32 shape coefficients; 56 joints from 16 on): SMPL-X's operands, Pd [k-step 17]
hipError_t launch_gather_joints(const float* verts, const int* ids, float* joints, int num_frames, int V, int J, int E,
                                int out_stride, hipStream_t stream);   // out_stride: J + E (+ L: landmark rows behind)

// J x V contraction on the matrix cores: out[J][N] = j_regressor[J][V] . rhs[V][N].
hipError_t launch_jreg_contract(const float* j_regressor, const float* rhs, float* out, int J, int V, int N,
                                float* partial_ws, int num_splits, hipStream_t stream);

// Joint-loss term of vertex-selected joints and its gradient (slow path, k2b_vertex.hip).
struct VertexTermArgs {
    // model (device): smplx tensors as uploaded by k2b_model_create
    const float *v_template, *shapedirs, *posedirs, *lbs_weights, *j_template, *j_dirs;
    const int *parents, *extra_ids;
    int num_vertices, num_betas, num_joints;
    // call
    int num_frames, num_sel;
    int sel[32];                // index into extra_ids of every fitted vertex joint
    int sel_k[32];              // its column in targets / conf
    int num_targets;            // columns of targets / conf
    const float* targets;       // dev [B][num_targets][3]
    const float* conf;          // dev [num_targets] or [B][num_targets] (conf_per_frame) or null
    int conf_per_frame;
    float sigma, joint_w;
    const float *go, *bp, *be, *tr;
    float *loss_out, *grad_out; // dev [B], [B][3 + 69 + NB + 3] (grad_out may be null with the Adam tail)
    // Adam tail (grad_in != null): the launch adds its loss / gradient to those of the evaluate-only launch of the fused
    // kernel (loss_in, grad_in), applies the optimiser's membership mask and makes the frame's Adam step in place
    const float *loss_in, *grad_in;
    float *go_w, *bp_w, *be_w, *tr_w;   // the parameters again, writable (same buffers as go, bp, be, tr)
    float *adam_m, *adam_v;             // dev [B][P]
    const float2* adam_coef;            // this step's {lr / (1 - b1^t), sqrt(1 - b2^t)}
    float one_minus_beta1, beta2, one_minus_beta2, eps;
    int opt_mask;
    int frozen_shape;                   // the first `frozen_shape` shape coefficients take no step (frozen betas beside a free expression)
};
hipError_t launch_vertex_term(const VertexTermArgs& a, hipStream_t stream);

// Surface-point term (k2b_surface.hip): targets that are weighted vertex sets of up to 3 (vertex, weight) pairs (extra joints:
// one pair of weight 1; landmarks: the barycentric pairs of a triangle), over a compact table of the selection's U vertices.
constexpr int kSurfMaxVerts = 3 * kSurfMaxTargets;    // distinct vertices per call
constexpr int kMaxLandmarks = 1024;                   // landmarks per model (k2b_model_set_landmarks)
struct SurfaceTermArgs {
    // compact table of the U distinct vertices (device, k2b_surface_gather_kernel)
    const float *vt, *sd, *pd, *lw;     // [U][3], [U][3][NB], [9(J-1)][3U], [U][J]
    const float *j_template, *j_dirs;
    const int* parents;
    int num_u, num_betas, num_joints;
    // targets (device): pair slots / weights [T][3] (unused pairs: slot 0, weight 0), target column [T], and the pairs of
    // every vertex as CSR (offsets [U + 1], target [n], weight [n])
    const int *pair_u, *sel_k, *inv_off, *inv_t;
    const float *pair_w, *inv_w;
    // call: as VertexTermArgs
    int num_frames, num_sel, num_targets;
    const float* targets;
    const float* conf;
    int conf_per_frame;
    float sigma, joint_w;
    const float *go, *bp, *be, *tr;
    float *loss_out, *grad_out;
    const float *loss_in, *grad_in;
    float *go_w, *bp_w, *be_w, *tr_w;
    float *adam_m, *adam_v;
    const float2* adam_coef;
    float one_minus_beta1, beta2, one_minus_beta2, eps;
    int opt_mask;
    int frozen_shape;
    // perspective form of the target block (k2b.h, k2b_fit_config::projection): targets are rows (u', v', ignored)
    int projection;
    float focal_x, focal_y;
};
hipError_t launch_surface_term(const SurfaceTermArgs& a, hipStream_t stream);
hipError_t launch_surface_gather(const float* v_template, const float* shapedirs, const float* posedirs, const float* lbs_weights,
                                 const int* ids, int n, int V, int J, int NB, float* vt, float* sd, float* pd, float* lw,
                                 hipStream_t stream);
hipError_t launch_landmarks(const float* src, int src_stride, const int* ids, const float* w, float* joints, int out_stride, int row0,
                            int num_frames, int L, hipStream_t stream);

hipError_t launch_adam(float* x, const float* g, float* m, float* v, long long n, float lr_over_bc1, float sqrt_bc2,
                       float one_minus_beta1, float beta2, float one_minus_beta2, float eps, hipStream_t stream);

// Raises a kernel's dynamic-LDS limit once PER DEVICE (the attribute is per device; a process-wide flag left the second
// GPU of a process without it, and two threads raced on it): one atomic flag per device ordinal and kernel instantiation.
template <class Kernel>
inline hipError_t ensure_dynamic_lds(Kernel kernel, std::atomic<unsigned long long>& done_mask, size_t bytes) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const unsigned long long bit = 1ull << (dev & 63);
    if (done_mask.load(std::memory_order_acquire) & bit) return hipSuccess;
    e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);   // idempotent: a race repeats it
    if (e == hipSuccess) done_mask.fetch_or(bit, std::memory_order_release);
    return e;
}

// ---- device-resident L-BFGS (k2b_lbfgs.hip): one state machine per frame, one closure result consumed per step launch ----------
hipError_t launch_lbfgs_step(const LbfgsArgs& a, hipStream_t stream, int max_staged_pairs = -1);   // (plan_lbfgs_step; < 0: no cap on the staged pairs)
hipError_t launch_lbfgs_frame_prep(float* go, const float* sgo, float* bp, const float* sbp, float* be, const float* sbe, float* tr,
                                   const float* str, float* pres, int D, int NB, void* state, size_t state_bytes, hipStream_t stream);

// Geodesic angle (degrees) between n pairs of axis-angle rotations (evaluation metric, k2b_metrics.hip).
hipError_t launch_angular_error(const float* pred, const float* gt, float* out, long long n, hipStream_t stream);

// Positional error of B frames of N points after an alignment (MPJPE / PA-MPJPE / PVE, k2b_metrics.hip): one wave per frame
// up to kPointErrorWavePoints points (four frames per workgroup), one workgroup per frame beyond.
constexpr int kPointErrorWavePoints = 256;
constexpr int kPointErrorMaxPoints = 1 << 20;
struct PointErrorArgs {
    const float* pred;       // [B][N][3]
    const float* gt;         // [B][N][3]
    const float* weights;    // [N], [B][N] (weights_per_frame) or NULL (ones)
    int weights_per_frame;
    int align_mode;          // 0 none, 1 translation, 2 rigid, 3 similarity
    int num_frames, num_points;
    float* err;              // [B]
    float* per_point;        // [B][N] or NULL
    float* transform;        // [B][13] or NULL: s, R row-major, t
};
// workgroups of the launch (256 threads each); the HIP runtime takes at most 2^32 - 1 threads per grid dimension
inline long long point_error_workgroups(int num_frames, int num_points) {
    return num_points <= kPointErrorWavePoints ? ((long long)num_frames + 3) / 4 : (long long)num_frames;
}
constexpr long long kPointErrorMaxWorkgroups = 0xffffffffll / 256;
hipError_t launch_point_error(const PointErrorArgs& a, hipStream_t stream);

// ---- IK-GAT regressor inference (k2b_ikgat.hip): B frames of J joint positions (+ input quaternions when in == 9) -> J
// quaternions per frame.  Batched: ceil(B / F) workgroups of F frames; chain: one workgroup walks the B frames in order,
// frame t + 1 reading frame t's outputs as its input quaternions.
struct IkgatArgs {
    const float* w;          // the device weight image (IkgatImage, k2b_ikgat_plan.h)
    const int* csr;          // [J + 1] in-edge offsets, then the source node of every in-edge (self loops included)
    const float* pos;        // [B][J][3]
    const float* quat_in;    // [B][J][4] xyzw (in == 9), or NULL
    float* quat_out;         // [B][J][4] xyzw
    int B, J, H, heads, L, in, F, KC, ldx, nedges, chain;
};
hipError_t launch_ikgat(const IkgatArgs& a, const IkgatLaunch& launch, hipStream_t stream);   // a.F = launch.F

}  // namespace k2b
