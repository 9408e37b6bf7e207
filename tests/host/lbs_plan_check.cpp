// Host check of the LBS pair's plans (csrc/k2b_lbs_plan.h): the route of every layout, the sizes of a call, the passes of a forward
// call and the backward's derived sizes against the rules as k2b_internal.h and DESIGN.md 4.2 / 4.2b / 4.2b-2 word them, written
// out here on their own - joint ranges 17-24 and 49-56, the k-step counts 14 / 32 / 34, the operand shapes - and never by calling
// the header's helpers.  No HIP call, no device.
// Usage: lbs_plan_check   (tests/test_lbs_plan_host.py); prints one line "(J, NB, F, KX, route)" per supported layout, one line
// per section and "N failures" last.
#include <cstdio>
#include <string>
#include <vector>

#include "k2b_lbs_plan.h"

using namespace k2b;

static int g_failures = 0;
static char g_where[256];
#define WHERE(...) std::snprintf(g_where, sizeof g_where, __VA_ARGS__)
#define CHECK(cond, ...)                                                        \
    do {                                                                        \
        if (!(cond)) {                                                          \
            if (++g_failures <= 20) {                                           \
                std::printf("FAIL %s: %s  [", g_where, #cond);                  \
                std::printf(__VA_ARGS__);                                       \
                std::printf("]\n");                                             \
            }                                                                   \
        }                                                                       \
    } while (0)
static void section(const char* name, int failures_before) { std::printf("%s: %s\n", name, g_failures == failures_before ? "ok" : "FAILED"); }

static const int kFrames[] = {1, 31, 32, 33, 37, 255, 256, 257, 4096, 10000};
static const int kCus[] = {1, 8, 64, 256, 304};
static const int kVerts[] = {1, 15, 16, 333, 6890, 10475};
static const int kLandmarks[] = {0, 1, 51, 1024};
static const size_t kLdsLimit = 160 * 1024;

// ---- the rules, restated ---------------------------------------------------------------------------------------------------------
static long long cdiv(long long a, long long b) { return a / b + (a % b != 0); }
static bool small_family(int J) { return J >= 17 && J <= 24; }     // SMPL
static bool large_family(int J) { return J >= 49 && J <= 56; }     // SMPL-H / SMPL-X
static bool supported(int J) { return small_family(J) || large_family(J); }
static int features(int J, int NB) { return 9 * (J - 1) + NB + 2; }   // X = [vec(R_1.. - I) | shape | 1 | 1]
// 16-deep k-steps and the kernel's name: the stream kernel takes 17-24 joints at 7 pose k-steps of depth 32; 49-56 joints are padded
// up to the 16-k-step kernel or take the 17-k-step one; the rest of both families runs the tile kernel
static const char* route_rule(int J, int NB, bool stream_kernels, bool tile_forced, int* kx) {
    *kx = 2 * (int)cdiv(features(J, NB), 32);
    if (stream_kernels && large_family(J) && *kx < 32) *kx = 32;
    if (!supported(J)) return "unsupported";
    if (!stream_kernels || tile_forced) return "tile";
    if (small_family(J)) return *kx == 14 ? "stream" : "tile";
    return *kx == 32 ? "stream_x" : *kx == 34 ? "stream_xw" : "tile";
}
static const char* route_name(LbsRoute r) {
    switch (r) {
        case LbsRoute::tile: return "tile";
        case LbsRoute::stream: return "stream";
        case LbsRoute::stream_x: return "stream_x";
        case LbsRoute::stream_xw: return "stream_xw";
        default: return "unsupported";
    }
}
static int grid_rule(int cus, long long tiles) {      // one workgroup per CU, a multiple of the 8 XCD labels, no more than the tiles need
    const int per_cu = cus < 8 ? 8 : cus / 8 * 8;
    return tiles < per_cu ? (int)(cdiv(tiles, 8) * 8) : per_cu;
}

// ---- route, KX, W fragments, pose capacity ---------------------------------------------------------------------------------------
static void check_routes() {
    const int before = g_failures;
    for (int J = 2; J <= 64; ++J)
        for (int NB = 1; NB <= 32; ++NB)
            for (int mode = 0; mode < 3; ++mode) {      // the build's default; a model under K2B_LBS_TILE; a build without the stream kernels
                const bool stream_kernels = mode != 2, tile_forced = mode == 1;
                WHERE("route J=%d NB=%d mode=%d", J, NB, mode);
                const LbsRouteRecord r = lbs_route(J, NB, stream_kernels, tile_forced);
                int kx = 0;
                const std::string want = route_rule(J, NB, stream_kernels, tile_forced, &kx);
                const int F = features(J, NB);
                CHECK(want == route_name(r.route), "route %s, expected %s", route_name(r.route), want.c_str());
                CHECK(r.k_steps_x == kx && r.groups_a == (int)cdiv(J, 8), "KX %d GA %d, expected %d %d", r.k_steps_x, r.groups_a, kx, (int)cdiv(J, 8));
                CHECK(r.streams() == (want.rfind("stream", 0) == 0), "streams() %d", (int)r.streams());
                if (!supported(J)) { CHECK(r.w_frags == 0 && r.pose_capacity == 0, "unsupported: %d fragments, capacity %d", r.w_frags, r.pose_capacity); continue; }
                CHECK(r.k_steps_x % 2 == 0 && 16 * r.k_steps_x >= F && r.k_steps_x <= kMaxXSteps, "KX %d for %d features", r.k_steps_x, F);
                CHECK(16 * (r.k_steps_x - 2) < F || (stream_kernels && large_family(J) && r.k_steps_x == 32), "KX %d is more than %d features need", r.k_steps_x, F);
                CHECK(r.w_frags == (want == "stream" ? 3 : want == "tile" ? 0 : 5), "%d W fragments on %s", r.w_frags, want.c_str());
                CHECK(lbs_route(J, NB, stream_kernels, !tile_forced).k_steps_x == r.k_steps_x, "K2B_LBS_TILE moves KX");
                if (mode == 0) std::printf("(%d, %d, %d, %d, %s)\n", J, NB, F, r.k_steps_x, route_name(r.route));
            }
    section("route table and padding of KX", before);
}

// the shape loop of the pose set-up is instantiated for 10 / 16 / 32 coefficients (17-24 joints) and 10 / 20 / 32 (49-56)
static void check_pose_capacity() {
    const int before = g_failures;
    const int small[] = {10, 16, 32}, large[] = {10, 20, 32};
    for (int J = 2; J <= 64; ++J)
        for (int NB = 1; NB <= 32 && supported(J); ++NB)
            for (int forced = 0; forced < 2; ++forced) {
                WHERE("pose capacity J=%d NB=%d forced=%d", J, NB, forced);
                int cap = 0;                                   // the smallest instantiated one that holds NB
                for (int c : small_family(J) ? small : large)
                    if (cap == 0 && c >= NB) cap = c;
                const int got = lbs_route(J, NB, true, forced != 0).pose_capacity;
                CHECK(got == cap, "capacity %d, expected %d", got, cap);
            }
    section("pose capacity", before);
}

// ---- sizes of a forward call -------------------------------------------------------------------------------------------------------
static void check_forward_sizes() {
    int before = g_failures;
    for (int B : kFrames) {
        WHERE("padded frames B=%d", B);
        const int bpad = lbs_frames_padded(B);
        CHECK(bpad % 32 == 0 && bpad >= B && bpad < B + 32, "%d", bpad);
    }
    section("padded frames", before);

    before = g_failures;
    for (int J = 2; J <= 64; ++J) {
        if (!supported(J)) continue;
        for (int NB = 1; NB <= 32; ++NB)
            for (int B : kFrames)
                for (int L : kLandmarks)
                    for (int forced = 0; forced < 2; ++forced) {
                        WHERE("workspace J=%d NB=%d B=%d L=%d forced=%d", J, NB, B, L, forced);
                        const LbsRouteRecord r = lbs_route(J, NB, true, forced != 0);
                        const size_t bpad = (size_t)cdiv(B, 32) * 32;
                        const LbsWorkspace w = lbs_workspace(r, (int)bpad, L);
                        int kx = 0;
                        route_rule(J, NB, true, forced != 0, &kx);
                        // X: [KX][32-frame tile] pieces of 1 KiB; A: [16-frame tile][entry 12][NGP = 2 GA + 2 groups][16 rows][8 halfs];
                        // landmark vertices: [frame][3 L][3] floats
                        CHECK(w.x_halfs == (size_t)kx * (bpad / 32) * 512, "X %zu", w.x_halfs);
                        CHECK(w.a2_halfs == (bpad / 16) * 12 * (2 * (size_t)cdiv(J, 8) + 2) * 16 * 8, "A2 %zu", w.a2_halfs);
                        CHECK(w.landmark_floats == bpad * 3 * (size_t)L * 3, "landmarks %zu", w.landmark_floats);
                    }
    }
    section("workspace", before);

    before = g_failures;
    for (int B : kFrames)
        for (int walk = 0; walk < 2; ++walk) {
            WHERE("pose grid B=%d walk=%d", B, walk);
            const LbsPoseGrid g = lbs_pose_grid(B, walk != 0);
            CHECK((g.xcd_frames != 0) == (walk && B > 256), "xcd_frames %d", g.xcd_frames);
            CHECK(g.xcd_frames % 32 == 0 && g.grid >= B && g.grid < B + 256, "xcd_frames %d grid %d", g.xcd_frames, g.grid);
            // the kernel's walk: workgroup b takes frame (b % 8) xcd_frames + b / 8, or frame b; every frame of the batch exactly once
            std::vector<int> hits(B, 0);
            for (int b = 0; b < g.grid; ++b) {
                const int f = g.xcd_frames ? (b & 7) * g.xcd_frames + (b >> 3) : b;
                CHECK(f >= 0, "frame %d", f);
                if (f >= 0 && f < B) ++hits[f];
            }
            bool once = true;
            for (int h : hits) once = once && h == 1;
            CHECK(once, "a frame is taken by no workgroup or by two");
        }
    section("pose grid", before);

    before = g_failures;
    for (int C : kCus)
        for (int B : kFrames)
            for (int V : kVerts) {
                WHERE("grids C=%d B=%d V=%d", C, B, V);
                const int f32 = (int)cdiv(B, 32), v32 = (int)cdiv(V, 32), nv16 = (int)cdiv(V, 128) * 8;   // stream images: whole 128-vertex groups
                CHECK(lbs_tile_grid(C, v32, f32) == grid_rule(C, cdiv(V, 128) * cdiv(B, 128)), "tile grid %d", lbs_tile_grid(C, v32, f32));
                CHECK(lbs_stream_grid(C, nv16, f32) == grid_rule(C, cdiv(V, 128) * cdiv(B, 128)), "stream grid %d", lbs_stream_grid(C, nv16, f32));
            }
    for (int GA : {3, 7}) {
        WHERE("tile LDS GA=%d", GA);
        // two 64 KiB ring slots and the W groups of eight 16-vertex tiles: [8][NGP][16][8] halfs
        CHECK(lbs_tile_lds_bytes(GA) == 2 * 65536 + (size_t)8 * (2 * GA + 2) * 16 * 8 * 2 && lbs_tile_lds_bytes(GA) <= kLdsLimit, "%zu", lbs_tile_lds_bytes(GA));
    }
    section("persistent grids", before);
}

// ---- passes of a forward call ------------------------------------------------------------------------------------------------------
static void check_forward_passes() {
    const int before = g_failures;
    for (int J : {17, 24, 49, 56})
        for (int V : kVerts)
            for (int E : {0, 1, 5})
                for (int L : kLandmarks)
                    for (int wants = 0; wants < 4; ++wants)
                        for (int in_mesh = 0; in_mesh < 2; ++in_mesh) {
                            const bool want_j = wants & 1, want_v = wants & 2;
                            WHERE("passes J=%d V=%d E=%d L=%d joints=%d vertices=%d in_mesh=%d", J, V, E, L, (int)want_j, (int)want_v, in_mesh);
                            const LbsForwardPlan p = lbs_forward_plan(want_j, want_v, J, V, E, L, in_mesh != 0);
                            if (!want_j && !want_v) { CHECK(p.num_passes == 0, "%d passes for no output", p.num_passes); continue; }
                            CHECK(p.num_passes >= 1 && p.num_passes <= 4 && p.pass[0].kind == LbsPass::pose_setup, "%d passes", p.num_passes);
                            const int rows = J + E + L;
                            std::vector<int> row(rows, 0);       // writes per row of joints_out
                            int verts = 0, ws = 0, ws_reads = 0; // writes of vertices_out and of the landmark workspace
                            auto write_rows = [&](int first, int n) { for (int i = first; i < first + n; ++i) { CHECK(i >= 0 && i < rows, "row %d", i); if (i >= 0 && i < rows) ++row[i]; } };
                            for (int i = 0; i < p.num_passes && i < 4; ++i) {
                                const LbsPass& q = p.pass[i];
                                const int stride = q.buf == LbsPass::vertices_out ? V : q.buf == LbsPass::joints_out ? rows : 3 * L;
                                switch (q.kind) {
                                    case LbsPass::pose_setup:
                                        CHECK(i == 0, "pose set-up at %d", i);
                                        if (want_j) write_rows(0, J);   // (the kernel writes the kinematic rows where joints_out is given)
                                        break;
                                    case LbsPass::skin: {
                                        CHECK(q.stride == stride, "stride %d", q.stride);
                                        const int n = q.set == LbsPass::mesh ? V : q.set == LbsPass::extra ? E : 3 * L;
                                        CHECK(n > 0, "an empty vertex set is skinned");
                                        if (q.buf == LbsPass::vertices_out) { CHECK(q.set == LbsPass::mesh && q.row0 == 0, "set %d", q.set); ++verts; }
                                        else if (q.buf == LbsPass::landmark_ws) { CHECK(q.set == LbsPass::landmark_verts && q.row0 == 0, "set %d", q.set); ++ws; }
                                        else { CHECK(q.set == LbsPass::extra, "set %d into joints_out", q.set); write_rows(q.row0, n); }
                                        if (q.joint_copies) {           // tagged vertices of the mesh: rows J .. J + E - 1
                                            CHECK(want_j && in_mesh && q.set == LbsPass::mesh, "joint copies");
                                            write_rows(J, E);
                                        }
                                        break;
                                    }
                                    case LbsPass::gather:
                                        CHECK(q.buf == LbsPass::vertices_out && q.stride == V && verts == 1, "gather from %d", q.buf);
                                        write_rows(J, E);
                                        break;
                                    case LbsPass::landmarks:
                                        CHECK(q.stride == stride, "stride %d", q.stride);
                                        if (q.buf == LbsPass::vertices_out) CHECK(verts == 1 && q.set == LbsPass::mesh, "landmarks before the mesh");
                                        else { CHECK(q.buf == LbsPass::landmark_ws && ws == 1 && q.set == LbsPass::landmark_verts, "landmarks before their vertices"); ++ws_reads; }
                                        write_rows(J + E, L);
                                        break;
                                }
                            }
                            bool once = true;
                            for (int w : row) once = once && w == (want_j ? 1 : 0);
                            CHECK(once, "an output row is written by no pass or by two, or without being asked for");
                            CHECK(verts == (want_v ? 1 : 0), "vertices written %d times", verts);
                            CHECK(ws == ws_reads && ws == (want_j && !want_v && L > 0 ? 1 : 0), "landmark workspace written %d times, read %d", ws, ws_reads);
                        }
    section("forward passes", before);
}

// ---- backward ----------------------------------------------------------------------------------------------------------------------
static void check_backward() {
    const int before = g_failures;
    std::vector<int> frames(kFrames, kFrames + sizeof kFrames / sizeof *kFrames);
    frames.push_back(65535 * 16);          // the last batch of one launch and the first beyond it
    frames.push_back(65535 * 16 + 1);
    size_t worst_lds = 0;
    for (int J = 2; J <= 64; ++J)
        for (int NB = 1; NB <= 32; ++NB)
            for (int V : kVerts)
                for (int U : {0, 1, 5, 64, 65, 3 * 1024 + 32})
                    for (int B : frames)
                        for (int dense = 0; dense < 2; ++dense) {
                            if (U > V) continue;
                            WHERE("backward J=%d NB=%d V=%d U=%d B=%d dense=%d", J, NB, V, U, B, dense);
                            const LbsBackwardPlan p = lbs_backward_plan(J, NB, V, U, B, dense != 0);
                            // the feature row [pose, padded to 16 | shape 16 or 32], Q = (J + 1) x 12, a slab = Q | row
                            const int PF = 9 * (J - 1), PF16 = (int)cdiv(PF, 16) * 16, KP = PF16 + (NB <= 16 ? 16 : 32);
                            CHECK(p.PF == PF && p.PF16 == PF16 && p.KP == KP && p.QN == (J + 1) * 12 && p.SL == p.QN + KP, "PF %d PF16 %d KP %d QN %d SL %d", p.PF, p.PF16, p.KP, p.QN, p.SL);
                            // chunks of 64 vertices in at most 16 groups of at least 4 chunks
                            const int NV = dense ? V : U;
                            CHECK(p.NV == NV && p.nchunks == (int)cdiv(NV, 64), "NV %d nchunks %d", p.NV, p.nchunks);
                            CHECK((long long)p.G * p.chunks_per_group >= p.nchunks && p.G <= 16 && p.chunks_per_group >= 4, "G %d x %d chunks", p.G, p.chunks_per_group);
                            CHECK((long long)(p.G - 1) * p.chunks_per_group < p.nchunks || p.G == 0, "group %d is empty", p.G - 1);
                            CHECK((p.G == 0) == (NV == 0), "G %d for %d vertices", p.G, NV);
                            CHECK(p.chunks_per_group == 4 || (long long)16 * (p.chunks_per_group - 1) < p.nchunks, "%d chunks per group is more than 16 groups need", p.chunks_per_group);
                            CHECK(kBwdMaxGroups == 16 && kBwdMinChunksPerGroup == 4 && kBwdPlanChunk == 64 && kBwdPlanFrames == 16, "constants");
                            // frames in tiles of 16; grid.y of a launch holds 65535
                            CHECK(p.frame_tiles == (int)cdiv(B, 16) && p.frames_padded == 16 * p.frame_tiles, "tiles %d padded %d", p.frame_tiles, p.frames_padded);
                            CHECK(p.exceeds_launch == (p.frame_tiles > 65535), "exceeds_launch %d at %d tiles", (int)p.exceeds_launch, p.frame_tiles);
                            // workspace X [padded][KP] | T [padded][J][12] | slabs [B][G][SL]: three parts back to back; nothing without a dense launch
                            const size_t x = p.G ? (size_t)p.frames_padded * KP : 0, t = p.G ? (size_t)p.frames_padded * J * 12 : 0, s = (size_t)B * p.G * p.SL;
                            CHECK(p.x_floats == x && p.t_floats == t && p.slab_floats == s && p.workspace_floats() == x + t + s, "parts %zu %zu %zu of %zu", p.x_floats, p.t_floats,
                                  p.slab_floats, p.workspace_floats());
                            if (!supported(J)) continue;
                            // the dense kernel: MT 16-row tiles hold the joints and the row of ones, four waves of TPW 16-feature tiles the row;
                            // LDS = X tile [16][KP + 4] | T [16][J][12] | three [16][196] tiles | W [64][16 MT + 1] | 192 columns
                            CHECK((p.dense_mt == 2 && p.dense_tpw == 4) || (p.dense_mt == 4 && p.dense_tpw == 9), "<%d, %d> is not instantiated", p.dense_mt, p.dense_tpw);
                            CHECK(16 * p.dense_mt >= J + 1 && 4 * p.dense_tpw * 16 >= KP, "<%d, %d> for %d joints, row %d", p.dense_mt, p.dense_tpw, J, KP);
                            CHECK((p.dense_mt == 2) == small_family(J), "MT %d", p.dense_mt);
                            const size_t lds = ((size_t)16 * (KP + 4) + (size_t)16 * J * 12 + 3 * 16 * 196 + (size_t)64 * (16 * p.dense_mt + 1) + 192) * 4;
                            CHECK(p.dense_lds_bytes == lds && lds <= kLdsLimit, "LDS %zu", p.dense_lds_bytes);
                            if (lds > worst_lds) worst_lds = lds;
                        }
    std::printf("backward: largest dense LDS %zu B of %zu\n", worst_lds, kLdsLimit);
    section("backward", before);
}

int main() {
    check_routes();
    check_pose_capacity();
    check_forward_sizes();
    check_forward_passes();
    check_backward();
    std::printf("%d failures\n", g_failures);
    return g_failures ? 1 : 0;
}
