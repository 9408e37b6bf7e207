// k2b_lbs_plan.h — the host decisions of the LBS pair (k2b_lbs, k2b_lbs_backward) as pure functions: which kernel skins a model
// and with how many k-steps, the sizes of a call (padded frames, workspace, grids, LDS), the ordered passes of a forward call, and
// every derived size of a backward call.  The ONE statement of those rules: the handle keeps the
// route record, the entries and launchers execute these plans, and tests/host/lbs_plan_check.cpp holds them to definitions
// written out independently, without a GPU.  No HIP runtime: a plain host C++ program may include this header alone.
#pragma once
#include "k2b_launch_plan.h"
#include "k2b_layout.h"
#include "k2b_lbs_fp8.h"

namespace k2b {

// ---- route: which kernel skins a model ---------------------------------------------------------------------------------------------
// 32-deep pose k-steps of the three stream kernels (k2b_lbs_stream.hip; operand layouts: k2b_internal.h, StreamArgs)
constexpr int kStreamKSteps = 7;
constexpr int kStreamXKSteps = 16;
constexpr int kStreamXWKSteps = 17;
constexpr int kMaxXSteps = 34;       // 16-deep k-steps of the feature vector the pose set-up can stage (SMPL: 14, SMPL-X: 32, or 34 with
                                     // 25-32 shape coefficients: 9 x 54 + 32 + 2 = 520 features)

enum class LbsRoute { unsupported, tile, stream, stream_x, stream_xw };
struct LbsRouteRecord {
    LbsRoute route = LbsRoute::unsupported;   // unsupported: neither 17-24 nor 49-56 joints (the fit kernels still take the model)
    int groups_a = 0;                         // GA = ceil(J / 8)
    int k_steps_x = 0;                        // 16-deep k-steps of the vertex GEMM (features), even: the kernels stage 32-deep slices
    int w_frags = 0;                          // W fragments per 16-vertex tile of the stream kernel's image (0: the tile kernel's images)
    int pose_capacity = 0;                    // shape-loop capacity of the pose set-up instantiation
    bool pose_fp8 = false;                    // route stream only: the correction products of the pose k-steps 0..5 as block-scaled
                                              // e4m3 MFMAs (k2b_lbs_fp8.h): e4m3 strips in the Pd images and in X, description SmplF8
    constexpr bool streams() const { return route == LbsRoute::stream || route == LbsRoute::stream_x || route == LbsRoute::stream_xw; }
};
// stream_kernels: the build routes to the stream kernels (K2B_LBS_STREAM); tile_forced: the model was created under K2B_LBS_TILE.
// 17-24 joints take the stream kernel only at its own k-step count.  49-56 joints with fewer features than SMPL-X (SMPL-H: 477 ->
// 15 k-steps) are padded up to the 16-k-step kernel - one all-zero k-step more buys the stream kernel - or take the 17-k-step one
// (513-544 features: 55 joints from 25 shape coefficients on, 56 from 16).  Everything else, and a forced model, runs the tile kernel.
// A model on the route `stream` gets the e4m3 form of the pose corrections (pose_fp8) when the k-steps 0..5 hold pose features
// only - 9 (J - 1) >= 192: 23 and 24 joints; shape coefficients and the template there would cost more than 5e-6 m - and the model
// was not created under K2B_LBS_POSE_F16 (pose_f16_forced): the three-f16-product twin, which is also the choice for a model whose
// pose correctives are large (measured on the synthetic model: X . Pd within 1.2e-6 m of float64 at +-pi per component; with 1 %
// of the posedirs x 20 or all of them x 10 the e4m3 form reads 5e-6 to 1.2e-5 m, the f16 form 1e-8).
constexpr LbsRouteRecord lbs_route(int J, int NB, bool stream_kernels, bool tile_forced, bool pose_f16_forced = false) {
    LbsRouteRecord r;
    const int GA = r.groups_a = tile_groups_a(J);
    int KX = (9 * (J - 1) + NB + 2 + 31) / 32 * 2;
    if (stream_kernels && GA == 7 && KX < 2 * kStreamXKSteps) KX = 2 * kStreamXKSteps;
    r.k_steps_x = KX;
    if ((GA != 3 && GA != 7) || KX > kMaxXSteps || NB < 1 || NB > kMaxShape) return r;
    const bool streams = stream_kernels && !tile_forced;
    r.route = streams && GA == 3 && KX == 2 * kStreamKSteps   ? LbsRoute::stream
            : streams && GA == 7 && KX == 2 * kStreamXKSteps  ? LbsRoute::stream_x
            : streams && GA == 7 && KX == 2 * kStreamXWKSteps ? LbsRoute::stream_xw
                                                              : LbsRoute::tile;
    r.w_frags = r.route == LbsRoute::stream ? 3 : r.streams() ? 5 : 0;
    r.pose_fp8 = r.route == LbsRoute::stream && !pose_f16_forced && 9 * (J - 1) >= 32 * kF8PoseSteps;
    r.pose_capacity = NB <= 10 ? 10 : GA == 3 ? (NB <= 16 ? 16 : 32) : (NB <= 20 ? 20 : 32);
    return r;
}

// ---- sizes of a forward call -------------------------------------------------------------------------------------------------------
constexpr int lbs_frames_padded(int num_frames) { return (num_frames + 31) / 32 * 32; }

// Element counts of the grow-only per-model workspace at `bpad` padded frames: X hi and X lo (each), the A operand, and the 3 L
// landmark vertices of a joints-only call.
struct LbsWorkspace { size_t x_halfs, a2_halfs, landmark_floats; };
constexpr LbsWorkspace lbs_workspace(const LbsRouteRecord& r, int bpad, int L) {
    return LbsWorkspace{(size_t)r.k_steps_x * bpad * 16, (size_t)(bpad / 16) * 12 * tile_ngp(r.groups_a) * 128, (size_t)bpad * 3 * L * 3};
}

// Pose set-up: one workgroup per frame.  With the XCD walk (K2B_POSE_XCD, batches above 256 frames) XCD label x = block % 8 takes
// the contiguous frames [x, x + 1) * xcd_frames, a multiple of 32 (k2b_lbs.hip); xcd_frames 0: workgroup b takes frame b.
struct LbsPoseGrid { int xcd_frames, grid; };
constexpr LbsPoseGrid lbs_pose_grid(int num_frames, bool xcd_walk) {
    const int per = xcd_walk && num_frames > 256 ? (num_frames + 255) / 256 * 32 : 0;
    return LbsPoseGrid{per, per ? 8 * per : num_frames};
}

// Persistent grids: the tile kernel walks (4 x 32-vertex tiles) x (4 x 32-frame tiles), a stream kernel (8 x 16-vertex tiles) x
// (4 x 32-frame tiles).
constexpr int lbs_tile_grid(int num_cus, int v_tiles, int f_tiles) {
    return persistent_grid(num_cus, (long long)((v_tiles + 3) / 4) * ((f_tiles + 3) / 4));
}
constexpr int lbs_stream_grid(int num_cus, int nv16, int f32_tiles) {
    return persistent_grid(num_cus, (long long)(nv16 >> 3) * ((f32_tiles + 3) >> 2));
}
// dynamic LDS of the tile kernel: two ring slots and the W image of eight 16-vertex tiles
constexpr int kTileSlotBytes = 64 * 1024;
constexpr size_t lbs_tile_lds_bytes(int GA) { return (size_t)2 * kTileSlotBytes + (size_t)8 * tile_ngp(GA) * 256; }

// ---- passes of a forward call ------------------------------------------------------------------------------------------------------
// Rows of joints_out: J kinematic (pose set-up), E vertex-selected, L landmarks; stride J + E + L.  With the mesh requested its
// launch also writes the vertex-selected joints whose vertices are tagged in the W image (joints_in_mesh), else a gather follows;
// landmarks are combined from the call's vertices.  Without it the E extra vertices are skinned straight into joints_out and the
// 3 L landmark vertices into the model's workspace, then combined.
struct LbsPass {
    enum Kind : int { pose_setup, skin, gather, landmarks } kind;
    enum Set : int { mesh, extra, landmark_verts } set;                  // skin: the vertex set
    enum Buf : int { vertices_out, joints_out, landmark_ws } buf;        // skin: the output; gather, landmarks: the source
    int stride, row0;                                                    // rows per frame of `buf` and the first row written / read
    bool joint_copies;                                                   // skin: tagged vertices are stored to joints_out as well
};
struct LbsForwardPlan {
    int num_passes;
    LbsPass pass[4];
};
constexpr LbsForwardPlan lbs_forward_plan(bool want_joints, bool want_vertices, int J, int V, int E, int L, bool joints_in_mesh) {
    LbsForwardPlan p{0, {}};
    if (!want_joints && !want_vertices) return p;
    const int ostride = J + E + L;
    p.pass[p.num_passes++] = LbsPass{LbsPass::pose_setup, LbsPass::mesh, LbsPass::joints_out, ostride, 0, false};
    if (want_vertices) {
        const bool copies = want_joints && E > 0 && joints_in_mesh;
        p.pass[p.num_passes++] = LbsPass{LbsPass::skin, LbsPass::mesh, LbsPass::vertices_out, V, 0, copies};
        if (want_joints && E > 0 && !copies) p.pass[p.num_passes++] = LbsPass{LbsPass::gather, LbsPass::mesh, LbsPass::vertices_out, V, 0, false};
        if (want_joints && L > 0) p.pass[p.num_passes++] = LbsPass{LbsPass::landmarks, LbsPass::mesh, LbsPass::vertices_out, V, 0, false};
        return p;
    }
    if (E > 0) p.pass[p.num_passes++] = LbsPass{LbsPass::skin, LbsPass::extra, LbsPass::joints_out, ostride, J, false};
    if (L > 0) {
        p.pass[p.num_passes++] = LbsPass{LbsPass::skin, LbsPass::landmark_verts, LbsPass::landmark_ws, 3 * L, 0, false};
        p.pass[p.num_passes++] = LbsPass{LbsPass::landmarks, LbsPass::landmark_verts, LbsPass::landmark_ws, 3 * L, 0, false};
    }
    return p;
}

// ---- backward (k2b_lbs_backward.hip) ----------------------------------------------------------------------------------------------
// the dense kernel's tile as the plan needs it; k2b_lbs_backward.hip names the same numbers kBwdFrames / kBwdChunk / kBwdRow next to
// the kernel and asserts that they agree
constexpr int kBwdPlanFrames = 16;                // frames of a tile: the M of every product
constexpr int kBwdPlanChunk = 64;                 // vertices per chunk
constexpr int kBwdPlanRow = 3 * kBwdPlanChunk + 4;   // LDS row stride of the [frame][3 vertex + c] tiles
constexpr int kBwdMaxGroups = 16;                 // slabs per frame at most
constexpr int kBwdMinChunksPerGroup = 4;
constexpr int kBwdMaxFrameTiles = 65535;          // grid.y of the dense launch

constexpr size_t lbs_backward_dense_lds_bytes(int J, int KP, int MT) {
    return ((size_t)kBwdPlanFrames * (KP + 4) + (size_t)kBwdPlanFrames * J * 12 + 3 * (size_t)kBwdPlanFrames * kBwdPlanRow +
            (size_t)kBwdPlanChunk * (16 * MT + 1) + 3 * kBwdPlanChunk) * sizeof(float);
}
constexpr int lbs_backward_frame_tiles(int B) { return ceil_div(B, kBwdPlanFrames); }

struct LbsBackwardPlan {
    bool exceeds_launch;         // more 16-frame tiles than one launch takes: the call is refused
    int PF, PF16, KP;            // pose features 9 (J - 1), padded to 16, and the padded row [pose PF16 | shape 16 or 32]
    int QN, SL;                  // (J + 1) * 12 floats of Q, slab size QN + KP
    int NV, nchunks, chunks_per_group, G;   // vertices of the dense launch, their chunks and groups (G 0: no dense launch)
    int frames_padded, frame_tiles;
    size_t x_floats, t_floats, slab_floats; // the workspace in this order: X [frames_padded][KP], T [frames_padded][J][12], slabs [B][G][SL]
    int dense_mt, dense_tpw;     // instantiation <MT, TPW> of the dense kernel: <2, 4> up to 24 joints, else <4, 9>
    size_t dense_lds_bytes;
    constexpr size_t workspace_floats() const { return x_floats + t_floats + slab_floats; }
};
// V: vertices of the mesh; U: distinct vertices the surface rows (extra joints, landmarks) name; dense: grad_vertices given
constexpr LbsBackwardPlan lbs_backward_plan(int J, int NB, int V, int U, int B, bool dense) {
    LbsBackwardPlan p{};
    p.frame_tiles = lbs_backward_frame_tiles(B);
    p.exceeds_launch = p.frame_tiles > kBwdMaxFrameTiles;
    p.frames_padded = p.frame_tiles * kBwdPlanFrames;
    p.PF = 9 * (J - 1); p.PF16 = (p.PF + 15) / 16 * 16; p.KP = p.PF16 + (NB <= 16 ? 16 : 32);
    p.QN = (J + 1) * 12; p.SL = p.QN + p.KP;
    p.NV = dense ? V : U;
    p.nchunks = ceil_div(p.NV, kBwdPlanChunk);
    const int spread = ceil_div(p.nchunks, kBwdMaxGroups);
    p.chunks_per_group = spread < kBwdMinChunksPerGroup ? kBwdMinChunksPerGroup : spread;
    p.G = ceil_div(p.nchunks, p.chunks_per_group);
    p.x_floats = p.G ? (size_t)p.frames_padded * p.KP : 0;
    p.t_floats = p.G ? (size_t)p.frames_padded * J * 12 : 0;
    p.slab_floats = (size_t)B * p.G * p.SL;
    p.dense_mt = J <= 24 ? 2 : 4;
    p.dense_tpw = J <= 24 ? 4 : 9;
    p.dense_lds_bytes = lbs_backward_dense_lds_bytes(J, p.KP, p.dense_mt);
    return p;
}

}  // namespace k2b
