// k2b_lbs_backward.hip — k2b_lbs_backward: the vector-Jacobian product of k2b_lbs (include/k2b.h), dense over all V vertices.
//
// Notation of k2b_vertex.hip (whose header derives the per-vertex backward).  With g_v the cotangent of vertex v (the caller's
// grad_vertices row, plus the rows of grad_joints that are vertices: an extra joint adds its cotangent to its vertex, a
// landmark b_k x its cotangent to its three vertices, the rule of k2b_surface.hip), vp_v the blended vertex and Rg_j, p_j, Jr_j
// the world rotation, world position and rest position of joint j, a frame needs these sums over its vertices:
//   Q_j  = sum_v w_vj g_v [vp_v ; 1]^T   (3 x 4 per joint: N_j | F_j; one more row block with w = 1 holds sum_v g_v)
//   GX_f = sum_{v,c} posedirs[f][3v + c] gvp_v[c],   GS_k = sum_{v,c} shapedirs[v][c][k] gvp_v[c],   gvp_v = sum_j w_vj Rg_j^T g_v
// and from them M_j = axial(N_j Rg_j^T) + (p_j - Rg_j Jr_j) x F_j, the moment of the vertices attached to joint j.
//
// Three launches per call, no host work in between:
//   prep   one wave per frame: Rodrigues, chain; the feature row X = [vec(R_1.. - I) | 0 | shape | 0] and T_j = [Rg_j | p_j - Rg_j Jr_j]
//   dense  one workgroup per (16-frame tile, group of vertex chunks); per chunk of kBwdChunk vertices
//            A   vp = v_template + X . [posedirs ; shapedirs]      fp32 MFMA, K = features
//            Q   W^T . (g (x) [vp ; 1]) per frame                  fp32 MFMA, K = vertices of the chunk
//            gvp (sum_j w_vj Rg_j)^T g_v                           VALU, one (frame, vertex) per lane
//            C   GX | GS = gvp . [posedirs ; shapedirs]^T          fp32 MFMA, K = 3 x vertices of the chunk
//          with Q and GX | GS accumulated in registers over the chunks of the group and stored ONCE, to the group's slab.
//          The constants are read from the model's fp32 arrays as k2b_model_create uploaded them: no further image.
//   tail   one wave per frame: adds the slabs in group order, then the chain backward of k2b_vertex.hip (torque about each joint
//          through the left Jacobian, axial(G R^T) from GX, rest joints through J_dirs, the kinematic rows of grad_joints).
// v_mfma_f32_16x16x4_f32 is a k-ordered chain of fp32 fma: every sum above has ONE order, fixed by the vertex count alone (the
// chunks, their groups and the slab order are functions of V), so a frame's gradient has the same bits in every batch.
// With grad_vertices == NULL the dense launch walks the compact list of the vertices that extra joints and landmarks name
// (or is skipped when there are none).
#include <algorithm>

#include "k2b_host.h"

namespace k2b {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kBwdFrames = 16;                    // frames of a tile: the M of every product
constexpr int kBwdChunk = 64;                     // vertices per chunk
constexpr int kBwdCols = 3 * kBwdChunk;
constexpr int kBwdRow = kBwdCols + 4;             // LDS row stride of the [frame][3 vertex + c] tiles (4 x odd: conflict-free A reads)
constexpr int kBwdThreads = 256;
// groups, workspace and LDS bytes of a call are sized for this tile by lbs_backward_plan (k2b_lbs_plan.h)
static_assert(kBwdFrames == kBwdPlanFrames && kBwdChunk == kBwdPlanChunk && kBwdRow == kBwdPlanRow, "k2b_lbs_plan.h plans for another tile");

struct BwdArgs {
    // model (device): smplx tensors as uploaded by k2b_model_create
    const float *v_template, *shapedirs, *posedirs, *lbs_weights, *j_template, *j_dirs;
    const int* parents;
    int V, J, NB;
    int PF, PF16, KP;            // pose features 9 (J - 1), padded to 16, and the padded row [pose PF16 | shape 16 or 32]
    int QN, SL;                  // (J + 1) * 12 floats of Q, slab size QN + KP
    // vertex set of the dense launch: all V vertices, or the compact list (vlist) of the surface rows' vertices
    const int* vlist;
    int NV, nchunks, chunks_per_group, G;
    // rows of grad_joints that are vertices, sorted by vertex: position in the vertex set, row, weight; offsets per chunk
    const int *item_pos, *item_row, *chunk_off;
    const float* item_w;
    int ostride;                 // rows of grad_joints: J + E + L
    // call
    int B;
    const float *go, *bp, *be;
    const float *grad_joints, *grad_vertices;
    float *X, *T, *slab;         // workspace: [B16][KP], [B16][J][12], [B][G][SL]
    float *g_go, *g_bp, *g_be, *g_tr;
};

// Local rotation, rest joint and chain of joint `lane` of frame f (k2b_vertex_term_kernel's forward); all 64 lanes call it.
struct JointState {
    Rodrigues rod;
    Mat3 Rg;
    Vec3 pg, Jr;
    int par;
};
__device__ __forceinline__ JointState chain_forward(const BwdArgs& a, int f, int lane, float (*sR)[9], float (*sJr)[3], int* spar) {
    const int J = a.J, NB = a.NB, D = 3 * (J - 1);
    const bool isJ = lane < J;
    JointState s;
    Vec3 th = {0.f, 0.f, 0.f};
    s.par = -1;
    s.Jr = {0.f, 0.f, 0.f};
    if (isJ) {
        const float* src = lane == 0 ? a.go + (size_t)f * 3 : a.bp + (size_t)f * D + 3 * (lane - 1);
        th = {src[0], src[1], src[2]};
        s.par = a.parents[lane];
        float e[3];
        for (int c = 0; c < 3; ++c) {
            float v = a.j_template[lane * 3 + c];
            for (int k = 0; k < NB; ++k) v += a.j_dirs[(lane * 3 + c) * NB + k] * a.be[(size_t)f * NB + k];
            e[c] = v;
        }
        s.Jr = {e[0], e[1], e[2]};
    }
    s.rod = rodrigues_fwd(th);
    if (isJ) {
        for (int i = 0; i < 9; ++i) sR[lane][i] = s.rod.R.m[i];
        sJr[lane][0] = s.Jr.x; sJr[lane][1] = s.Jr.y; sJr[lane][2] = s.Jr.z;
        spar[lane] = s.par < 0 ? -1 : s.par;
    }
    __syncthreads();
    s.Rg = s.rod.R;
    s.pg = s.Jr;
    if (isJ) {
        // p_j = p_par + Rg_par (Jr_j - Jr_par): walk towards the root
        if (s.par >= 0) s.pg = s.Jr - Vec3{sJr[s.par][0], sJr[s.par][1], sJr[s.par][2]};
        for (int anc = s.par; anc >= 0; anc = spar[anc]) {
            Mat3 Ra;
            for (int i = 0; i < 9; ++i) Ra.m[i] = sR[anc][i];
            const int pa = spar[anc];
            const Vec3 da = pa >= 0 ? Vec3{sJr[anc][0] - sJr[pa][0], sJr[anc][1] - sJr[pa][1], sJr[anc][2] - sJr[pa][2]}
                                    : Vec3{sJr[anc][0], sJr[anc][1], sJr[anc][2]};
            s.pg = mul(Ra, s.pg) + da;
            s.Rg = mul(Ra, s.Rg);
        }
    }
    return s;
}

__device__ __forceinline__ Vec3 axial_of_GRt_b(const Mat3& G, const Mat3& R) {
    // axial(G R^T): M = G R^T, result (M32 - M23, M13 - M31, M21 - M12)
    float M[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) M[3 * r + c] = G.m[3 * r] * R.m[3 * c] + G.m[3 * r + 1] * R.m[3 * c + 1] + G.m[3 * r + 2] * R.m[3 * c + 2];
    return {M[7] - M[5], M[2] - M[6], M[3] - M[1]};
}

// ---- prep: one wave per frame of the padded batch (frames beyond B get zero rows) ---------------------------------------------
__global__ __launch_bounds__(64) void k2b_lbs_backward_prep_kernel(const BwdArgs a) {
    __shared__ float sR[kMaxJoints][9], sJr[kMaxJoints][3];
    __shared__ int spar[kMaxJoints];
    __shared__ float sXf[9 * (kMaxJoints - 1) + 1];
    const int f = blockIdx.x, lane = threadIdx.x, J = a.J;
    float* X = a.X + (size_t)f * a.KP;
    float* T = a.T + (size_t)f * J * 12;
    if (f >= a.B) {
        for (int k = lane; k < a.KP; k += 64) X[k] = 0.f;
        for (int k = lane; k < J * 12; k += 64) T[k] = 0.f;
        return;
    }
    const JointState s = chain_forward(a, f, lane, sR, sJr, spar);
    if (lane < J) {
        const Vec3 t = s.pg - mul(s.Rg, s.Jr);
        float* d = T + lane * 12;
        d[0] = s.Rg.m[0]; d[1] = s.Rg.m[1]; d[2] = s.Rg.m[2]; d[3] = t.x;
        d[4] = s.Rg.m[3]; d[5] = s.Rg.m[4]; d[6] = s.Rg.m[5]; d[7] = t.y;
        d[8] = s.Rg.m[6]; d[9] = s.Rg.m[7]; d[10] = s.Rg.m[8]; d[11] = t.z;
        if (lane > 0)
            for (int i = 0; i < 9; ++i) sXf[(lane - 1) * 9 + i] = s.rod.R.m[i] - ((i % 4 == 0) ? 1.f : 0.f);
    }
    __syncthreads();
    for (int k = lane; k < a.KP; k += 64) {
        float v = 0.f;
        if (k < a.PF) v = sXf[k];
        else if (k >= a.PF16 && k - a.PF16 < a.NB) v = a.be[(size_t)f * a.NB + (k - a.PF16)];
        X[k] = v;
    }
}

// ---- dense: (frame tile, chunk group) per workgroup -----------------------------------------------------------------------------
// MT: 16-row tiles of the joints (+ the row of ones) in Q; TPW: 16-feature tiles of GX | GS per wave.
// MFMA operand maps (v_mfma_f32_16x16x4_f32): A[row = lane & 15][k = lane >> 4], B[k = lane >> 4][col = lane & 15],
// C/D[row = 4 (lane >> 4) + reg][col = lane & 15].
template <int MT, int TPW>
__global__ __launch_bounds__(kBwdThreads) void k2b_lbs_backward_dense_kernel(const BwdArgs a) {
    extern __shared__ float lds[];
    constexpr int WJ = 16 * MT, WS = WJ + 1;
    const int J = a.J, KP = a.KP, XS = KP + 4, V = a.V, NB = a.NB, PF = a.PF, PF16 = a.PF16;
    float* sX = lds;                                  // [16][XS]      feature rows of the tile
    float* sT = sX + kBwdFrames * XS;                 // [16][J][12]   skinning transforms
    float* sg = sT + kBwdFrames * J * 12;             // [16][kBwdRow] vertex cotangents of the chunk
    float* svp = sg + kBwdFrames * kBwdRow;           // [16][kBwdRow] blended vertices
    float* sgvp = svp + kBwdFrames * kBwdRow;         // [16][kBwdRow] blend-shape cotangents
    float* sW = sgvp + kBwdFrames * kBwdRow;          // [64][WS]      skinning weights | 1 | 0..
    int* sCol = reinterpret_cast<int*>(sW + kBwdChunk * WS);   // [192]  column 3 vertex + c of every chunk column

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 15, lq = lane >> 4;
    const int grp = blockIdx.x, f0 = blockIdx.y * kBwdFrames;

    for (int i = tid; i < kBwdFrames * KP; i += kBwdThreads) {
        const int f = i / KP, k = i - f * KP;
        sX[f * XS + k] = a.X[(size_t)(f0 + f) * KP + k];
    }
    for (int i = tid; i < kBwdFrames * J * 12; i += kBwdThreads) sT[i] = a.T[(size_t)f0 * J * 12 + i];

    // feature tiles of this wave in product C: row pointer of its lane's feature and the stride between columns
    const int pose_tiles = PF16 / 16, ntiles = KP / 16;
    const float* crow[TPW];
    int cstride[TPW];
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
        const int tile = wave * TPW + t;
        if (tile < pose_tiles) {
            crow[t] = a.posedirs + (size_t)min(16 * tile + lr, PF - 1) * 3 * V;
            cstride[t] = 1;
        } else {
            crow[t] = a.shapedirs + min(16 * (tile - pose_tiles) + lr, NB - 1);
            cstride[t] = NB;
        }
    }
    f32x4 accQ[4][MT], accG[TPW];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int m = 0; m < MT; ++m) accQ[i][m] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < TPW; ++t) accG[t] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int ci = 0; ci < a.chunks_per_group; ++ci) {
        const int chunk = grp * a.chunks_per_group + ci;
        if (chunk >= a.nchunks) break;                // (the same for every lane of the workgroup)
        const int v0 = chunk * kBwdChunk;
        // ---- stage the chunk: columns, weights, cotangents -------------------------------------------------------------------
        for (int n = tid; n < kBwdCols; n += kBwdThreads) {
            const int v = n / 3, ic = min(v0 + v, a.NV - 1);
            sCol[n] = 3 * (a.vlist ? a.vlist[ic] : ic) + (n - 3 * v);
        }
        for (int i = tid; i < kBwdChunk * WJ; i += kBwdThreads) {
            const int v = i / WJ, j = i - v * WJ, ic = min(v0 + v, a.NV - 1);
            const int vid = a.vlist ? a.vlist[ic] : ic;
            sW[v * WS + j] = j < J ? a.lbs_weights[(size_t)vid * J + j] : (j == J ? 1.f : 0.f);
        }
        for (int i = tid; i < kBwdFrames * kBwdCols; i += kBwdThreads) {
            const int f = i / kBwdCols, n = i - f * kBwdCols, v = n / 3;
            float g = 0.f;
            if (a.grad_vertices && f0 + f < a.B && v0 + v < a.NV) {
                const int ic = v0 + v;
                const int vid = a.vlist ? a.vlist[ic] : ic;
                g = a.grad_vertices[((size_t)(f0 + f) * V + vid) * 3 + (n - 3 * v)];
            }
            sg[f * kBwdRow + n] = g;
        }
        __syncthreads();
        // rows of grad_joints that are vertices of this chunk, in table order (one lane per frame and coordinate)
        if (a.grad_joints && tid < 3 * kBwdFrames) {
            const int f = tid / 3, c = tid - 3 * f;
            if (f0 + f < a.B) {
                const float* gj = a.grad_joints + (size_t)(f0 + f) * a.ostride * 3 + c;
                float* dst = sg + f * kBwdRow + c;
                for (int it = a.chunk_off[chunk]; it < a.chunk_off[chunk + 1]; ++it)
                    dst[3 * (a.item_pos[it] - v0)] += a.item_w[it] * gj[3 * a.item_row[it]];
            }
        }
        // ---- A: vp = v_template + X . [posedirs ; shapedirs], three 16-column tiles per wave -------------------------------
        {
            int col[3];
            f32x4 acc[3];
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                col[t] = sCol[16 * (3 * wave + t) + lr];
                const float vt = a.v_template[col[t]];
                acc[t] = f32x4{vt, vt, vt, vt};
            }
            const float* xrow = sX + lr * XS;
            for (int k = lq; k < PF16; k += 4) {
                if (k - lq >= PF) break;              // whole k-steps of padding
                const float av = xrow[k];
                const float* prow = a.posedirs + (size_t)min(k, PF - 1) * 3 * V;
#pragma unroll
                for (int t = 0; t < 3; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, prow[col[t]], acc[t], 0, 0, 0);
            }
            for (int k = lq; k - lq < NB; k += 4) {
                const float av = xrow[PF16 + k];
                const int kc = min(k, NB - 1);
#pragma unroll
                for (int t = 0; t < 3; ++t)
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, a.shapedirs[(size_t)col[t] * NB + kc], acc[t], 0, 0, 0);
            }
#pragma unroll
            for (int t = 0; t < 3; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) svp[(4 * lq + r) * kBwdRow + 16 * (3 * wave + t) + lr] = acc[t][r];
        }
        __syncthreads();
        // ---- Q: per frame W^T . (g (x) [vp ; 1]); wave w owns the frames 4 w .. 4 w + 3 -----------------------------------------
        {
            const int qr = min(lr >> 2, 2), qc = lr & 3;
            const bool live = lr < 12;
            for (int v = lq; v < kBwdChunk; v += 4) {
                float aw[MT];
#pragma unroll
                for (int m = 0; m < MT; ++m) aw[m] = sW[v * WS + 16 * m + lr];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int f = 4 * wave + i;
                    const float gval = sg[f * kBwdRow + 3 * v + qr];
                    const float pv = qc < 3 ? svp[f * kBwdRow + 3 * v + qc] : 1.f;
                    const float b = live ? gval * pv : 0.f;
#pragma unroll
                    for (int m = 0; m < MT; ++m) accQ[i][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(aw[m], b, accQ[i][m], 0, 0, 0);
                }
            }
        }
        // ---- gvp = (sum_j w_vj Rg_j)^T g_v: lane = vertex, wave w the frames w, w + 4, w + 8, w + 12 --------------------------
        for (int i = 0; i < 4; ++i) {
            const int f = wave + 4 * i;
            const float* w = sW + lane * WS;
            const float* T = sT + f * J * 12;
            float R[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            for (int j = 0; j < J; ++j) {
                const float wj = w[j];
                const float* Tj = T + j * 12;
                R[0] += wj * Tj[0]; R[1] += wj * Tj[1]; R[2] += wj * Tj[2];
                R[3] += wj * Tj[4]; R[4] += wj * Tj[5]; R[5] += wj * Tj[6];
                R[6] += wj * Tj[8]; R[7] += wj * Tj[9]; R[8] += wj * Tj[10];
            }
            const float* g = sg + f * kBwdRow + 3 * lane;
            float* o = sgvp + f * kBwdRow + 3 * lane;
            o[0] = R[0] * g[0] + R[3] * g[1] + R[6] * g[2];
            o[1] = R[1] * g[0] + R[4] * g[1] + R[7] * g[2];
            o[2] = R[2] * g[0] + R[5] * g[1] + R[8] * g[2];
        }
        __syncthreads();
        // ---- C: GX | GS += gvp . [posedirs ; shapedirs]^T, K = the chunk's 192 columns ----------------------------------------
        {
            const float* grow = sgvp + lr * kBwdRow;
            for (int n = lq; n < kBwdCols; n += 4) {
                const float av = grow[n];
                const int c = sCol[n];
#pragma unroll
                for (int t = 0; t < TPW; ++t)
                    if (wave * TPW + t < ntiles)
                        accG[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, crow[t][(size_t)cstride[t] * c], accG[t], 0, 0, 0);
            }
        }
        __syncthreads();
    }

    // ---- the group's slab ----------------------------------------------------------------------------------------------------
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int f = f0 + 4 * wave + i;
        if (f >= a.B || lr >= 12) continue;
        float* q = a.slab + ((size_t)f * a.G + grp) * a.SL;
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = 16 * m + 4 * lq + r;
                if (j <= J) q[j * 12 + lr] = accQ[i][m][r];
            }
    }
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
        const int tile = wave * TPW + t;
        if (tile >= ntiles) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int f = f0 + 4 * lq + r;
            if (f < a.B) a.slab[((size_t)f * a.G + grp) * a.SL + a.QN + 16 * tile + lr] = accG[t][r];
        }
    }
}

// ---- tail: one wave per frame ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k2b_lbs_backward_tail_kernel(const BwdArgs a) {
    constexpr int QM = (kMaxJoints + 1) * 12, KM = 16 * ((9 * (kMaxJoints - 1) + 15) / 16) + kMaxShape;
    __shared__ float sR[kMaxJoints][9], sJr[kMaxJoints][3];
    __shared__ int spar[kMaxJoints];
    __shared__ float sS[QM + KM];                     // the frame's sums: Q | GX | GS
    __shared__ float sF[kMaxJoints][3], sM[kMaxJoints][3];
    const int f = blockIdx.x, lane = threadIdx.x;
    const int J = a.J, NB = a.NB, D = 3 * (J - 1);
    const bool isJ = lane < J;

    // the slabs in group order
    for (int e = lane; e < a.SL; e += 64) {
        float s = 0.f;
        for (int g = 0; g < a.G; ++g) s += a.slab[((size_t)f * a.G + g) * a.SL + e];
        sS[e] = s;
    }
    const JointState st = chain_forward(a, f, lane, sR, sJr, spar);   // (its barrier also publishes sS)
    const float* sGX = sS + a.QN;
    const float* sGS = sGX + a.PF16;

    // ---- joints: force and moment of the vertices attached to each joint, and the joint's own cotangent --------------------
    Vec3 Fv = {0.f, 0.f, 0.f}, gk = {0.f, 0.f, 0.f};
    if (isJ) {
        const float* q = sS + lane * 12;
        // H = N Rg^T, sum_v w (Rg vp) x g = (H21 - H12, H02 - H20, H10 - H01)
        float H[9];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c)
                H[3 * r + c] = q[4 * r] * st.Rg.m[3 * c] + q[4 * r + 1] * st.Rg.m[3 * c + 1] + q[4 * r + 2] * st.Rg.m[3 * c + 2];
        Fv = {q[3], q[7], q[11]};
        const Vec3 t = st.pg - mul(st.Rg, st.Jr);
        Vec3 M = Vec3{H[7] - H[5], H[2] - H[6], H[3] - H[1]} + cross(t, Fv);
        if (a.grad_joints) {
            const float* gj = a.grad_joints + ((size_t)f * a.ostride + lane) * 3;
            gk = {gj[0], gj[1], gj[2]};
        }
        const Vec3 F = Fv + gk;
        M = M + cross(st.pg, gk);
        sF[lane][0] = F.x; sF[lane][1] = F.y; sF[lane][2] = F.z;
        sM[lane][0] = M.x; sM[lane][1] = M.y; sM[lane][2] = M.z;
    }
    __syncthreads();

    // ---- subtree sums, torque, pull-back (k2b_vertex_term_kernel) -----------------------------------------------------------------
    Vec3 gth = {0.f, 0.f, 0.f}, gd = {0.f, 0.f, 0.f}, gJ = {0.f, 0.f, 0.f};
    if (isJ) {
        Vec3 aj = {0.f, 0.f, 0.f}, tj = {0.f, 0.f, 0.f};
        for (int k = 0; k < J; ++k) {               // k in subtree(lane)  <=>  lane is k or an ancestor of k
            bool below = false;
            for (int t = k; t >= 0; t = spar[t])
                if (t == lane) { below = true; break; }
            if (below) {
                aj.x += sF[k][0]; aj.y += sF[k][1]; aj.z += sF[k][2];
                tj.x += sM[k][0]; tj.y += sM[k][1]; tj.z += sM[k][2];
            }
        }
        const Vec3 torque = tj - cross(st.pg, aj);
        Vec3 w = mul(st.rod.R, mulT(st.Rg, torque));               // Rg = Rgp R  =>  Rgp^T v = R (Rg^T v)
        gd = mul(st.rod.R, mulT(st.Rg, aj));                       // dL/d(Jr_j - Jr_par)
        if (lane > 0) {
            Mat3 G;
            for (int i = 0; i < 9; ++i) G.m[i] = sGX[(lane - 1) * 9 + i];
            w = w + axial_of_GRt_b(G, st.rod.R);
        }
        const Rodrigues& rod = st.rod;
        const float a1 = rod.s * rod.inv_angle, a3 = (1.0f - rod.c) * rod.inv_angle;
        const float uw = rod.u.x * w.x + rod.u.y * w.y + rod.u.z * w.z;
        const float a2uw = (1.0f - a1) * uw;
        const Vec3 uxw = cross(rod.u, w);
        gth = {a1 * w.x + a2uw * rod.u.x - a3 * uxw.x, a1 * w.y + a2uw * rod.u.y - a3 * uxw.y, a1 * w.z + a2uw * rod.u.z - a3 * uxw.z};
        gJ = mulT(st.Rg, Fv);                                      // dL/dJr_j = -Rg_j^T F_j (the vertices' part)
    }

    // ---- outputs ------------------------------------------------------------------------------------------------------------------
    if (isJ) {
        float* dst = lane == 0 ? a.g_go : a.g_bp;
        if (dst) {
            dst += lane == 0 ? (size_t)f * 3 : (size_t)f * D + 3 * (lane - 1);
            dst[0] = gth.x; dst[1] = gth.y; dst[2] = gth.z;
        }
    }
    if (a.g_be) {
        // shape through the joint offsets (gd), through the rest joints inside the skinning transform (gJ), and through the vertices (GS)
        for (int k = 0; k < NB; ++k) {
            float s = 0.f;
            if (isJ)
                for (int c = 0; c < 3; ++c) {
                    const float dj = a.j_dirs[(lane * 3 + c) * NB + k];
                    const float dp = st.par >= 0 ? a.j_dirs[(st.par * 3 + c) * NB + k] : 0.f;
                    const float gdc = c == 0 ? gd.x : (c == 1 ? gd.y : gd.z);
                    const float gjc = c == 0 ? gJ.x : (c == 1 ? gJ.y : gJ.z);
                    s += gdc * (dj - dp) - gjc * dj;
                }
            s = wave_sum(s);
            if (lane == 0) a.g_be[(size_t)f * NB + k] = s + sGS[k];
        }
    }
    if (a.g_tr) {
        // every output row moves with the translation: sum_v g_v (the Q row of ones) and the kinematic rows
        const float tx = wave_sum(gk.x), ty = wave_sum(gk.y), tz = wave_sum(gk.z);
        if (lane == 0) {
            const float* q1 = sS + J * 12;
            a.g_tr[(size_t)f * 3] = tx + q1[3];
            a.g_tr[(size_t)f * 3 + 1] = ty + q1[7];
            a.g_tr[(size_t)f * 3 + 2] = tz + q1[11];
        }
    }
}

// the instantiation and its LDS bytes come with the plan (k2b_lbs_plan.h)
template <int MT, int TPW>
hipError_t launch_dense_as(const BwdArgs& a, const LbsBackwardPlan& p, hipStream_t stream) {
    static std::atomic<unsigned long long> done{0};
    if (const hipError_t e = ensure_dynamic_lds(k2b_lbs_backward_dense_kernel<MT, TPW>, done, p.dense_lds_bytes); e != hipSuccess) return e;
    hipLaunchKernelGGL((k2b_lbs_backward_dense_kernel<MT, TPW>), dim3(p.G, p.frame_tiles), dim3(kBwdThreads), p.dense_lds_bytes, stream, a);
    return hipGetLastError();
}
hipError_t launch_dense(const BwdArgs& a, const LbsBackwardPlan& p, hipStream_t stream) {
    return p.dense_mt == 2 ? launch_dense_as<2, 4>(a, p, stream) : launch_dense_as<4, 9>(a, p, stream);
}

}  // namespace

namespace host {

// The rows of grad_joints that are vertices (extra joints, landmark corners) as k2b_model_tables.h (lbs_backward_image) lays them
// out; built on the first backward call of a model (blocking upload).  Caller holds m->mu.
int lbs_backward_tables(k2b_model* m) {
    k2b_model::LbsBackward& t = m->bwd;
    if (t.built && t.L == m->lmk.L) return K2B_OK;
    if (t.built) HIP_TRY(hipDeviceSynchronize());               // landmarks arrived after a backward call: nothing may still read the old table
    std::vector<tables::BackwardItem> items;
    for (int e = 0; e < m->E; ++e) items.push_back({m->h_extra_ids[e], m->J + e, 1.f});
    for (int l = 0; l < m->lmk.L; ++l)
        for (int k = 0; k < 3; ++k) items.push_back({m->lmk.h_ids[3 * l + k], m->J + m->E + l, m->lmk.h_w[3 * l + k]});
    const tables::BackwardImage img = tables::lbs_backward_image(std::move(items), m->V, kBwdChunk);
    HIP_TRY(t.ints.upload(img.ints.data(), img.ints.size()));
    HIP_TRY(t.w.upload(img.w.data(), img.w.size()));
    static_cast<tables::BackwardOffsets&>(t) = img;
    t.L = m->lmk.L; t.built = true;
    return K2B_OK;
}

}  // namespace host
}  // namespace k2b

using namespace k2b::host;

extern "C" int k2b_lbs_backward(const k2b_model* model_c, int32_t B, const float* go, const float* bp, const float* be, const float* tr,
                                const float* grad_joints, const float* grad_vertices, float* g_go, float* g_bp, float* g_be,
                                float* g_tr, void* stream_v) {
    (void)tr;                                         // the forward is affine in transl: its cotangent needs no value of it
    k2b_model* m = const_cast<k2b_model*>(model_c);
    if (!m) return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_lbs_backward: model is NULL");
    if (B < 0) return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_lbs_backward: num_frames=%d", B);
    if (B == 0) return K2B_OK;
    if (!go || !bp || !be) return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_lbs_backward: NULL parameter buffer");
    if (!grad_joints && !grad_vertices) return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_lbs_backward: no cotangent given");
    if (m->lbs.route == k2b::LbsRoute::unsupported)
        return fail(K2B_ERR_UNSUPPORTED, "k2b_lbs_backward: %d joints; k2b_lbs and its backward are built for 17-24 (SMPL) and 49-56 (SMPL-H / SMPL-X) joints", m->J);
    if (m->NB < 1 || m->NB > k2b::kMaxShape) return fail(K2B_ERR_UNSUPPORTED, "k2b_lbs_backward: %d shape coefficients, at most %d", m->NB, k2b::kMaxShape);
    if (k2b::lbs_backward_frame_tiles(B) > k2b::kBwdMaxFrameTiles) return fail(K2B_ERR_UNSUPPORTED, "k2b_lbs_backward: %d frames exceed one launch", B);
    if (!g_go && !g_bp && !g_be && !g_tr) return K2B_OK;
    hipStream_t stream = (hipStream_t)stream_v;
    {
        std::lock_guard<std::mutex> lk(m->mu);
        if (const int rc = lbs_backward_tables(m); rc != K2B_OK) return rc;
    }
    const k2b_model::LbsBackward& t = m->bwd;
    // the vertex set: every vertex, or (no vertex cotangent) the vertices the surface rows name
    const bool dense = grad_vertices != nullptr;
    const k2b::LbsBackwardPlan p = k2b::lbs_backward_plan(m->J, m->NB, m->V, t.U, B, dense);
    k2b::BwdArgs a{};
    a.v_template = m->v_template.get(); a.shapedirs = m->shapedirs.get(); a.posedirs = m->posedirs.get(); a.lbs_weights = m->lbs_weights.get();
    a.j_template = m->j_template.get(); a.j_dirs = m->j_dirs.get(); a.parents = m->parents.get();
    a.V = m->V; a.J = m->J; a.NB = m->NB;
    a.PF = p.PF; a.PF16 = p.PF16; a.KP = p.KP; a.QN = p.QN; a.SL = p.SL;
    a.ostride = m->J + m->E + m->lmk.L;
    a.NV = p.NV; a.nchunks = p.nchunks; a.chunks_per_group = p.chunks_per_group; a.G = p.G;   // G 0: a joints-only call on a model without surface rows
    a.vlist = dense ? nullptr : t.ints.get();
    a.item_row = t.ints.get() + t.o_rows;
    a.item_pos = t.ints.get() + (dense ? t.o_pos_dense : t.o_pos_compact);
    a.chunk_off = t.ints.get() + (dense ? t.o_off_dense : t.o_off_compact);
    a.item_w = t.w.get();
    a.B = B; a.go = go; a.bp = bp; a.be = be; a.grad_joints = grad_joints; a.grad_vertices = grad_vertices;
    a.g_go = g_go; a.g_bp = g_bp; a.g_be = g_be; a.g_tr = g_tr;
    StreamWorkspace ws(stream);
    if (p.G) {
        HIP_TRY(ws.alloc(p.workspace_floats() * sizeof(float)));
        a.X = reinterpret_cast<float*>(ws.get()); a.T = a.X + p.x_floats; a.slab = a.T + p.t_floats;
        hipLaunchKernelGGL(k2b::k2b_lbs_backward_prep_kernel, dim3(p.frames_padded), dim3(64), 0, stream, a);
        HIP_TRY_MSG(hipGetLastError(), "k2b_lbs_backward: prep launch failed");
        HIP_TRY_MSG(k2b::launch_dense(a, p, stream), "k2b_lbs_backward: dense launch failed");
    }
    hipLaunchKernelGGL(k2b::k2b_lbs_backward_tail_kernel, dim3(B), dim3(64), 0, stream, a);
    HIP_TRY_MSG(hipGetLastError(), "k2b_lbs_backward: tail launch failed");
    return K2B_OK;
}
