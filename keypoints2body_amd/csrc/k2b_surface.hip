// k2b_surface.hip — joint-loss term of SURFACE POINTS (model joint index >= J beyond what k2b_vertex.hip takes), the
// gather of their vertex rows, and the landmark pass of the forward.
//
// A surface target is a weighted vertex set of up to three (vertex, weight) pairs: smplx's vertex-selected "extra" joints
// are one pair of weight 1, its facial landmarks the three barycentric pairs of one mesh triangle (smplx
// `vertices2landmarks`: sum_k b_k v[faces[lmk_faces_idx, k]]).  The term, its backward and the Adam tail are those of
// k2b_vertex_term_kernel (k2b_vertex.hip, whose header comment derives them); what generalises:
//   x_t = sum_k b_tk (x_{u_tk} + transl)           (x_u: the skinned vertex u without translation; the forward's
//                                                    formula: k2b_lbs combines translated vertices)
//   g_u = sum over the pairs (t, k) of vertex u of b_tk dL/dx_t,   dL/dtransl = sum_t (sum_k b_tk) dL/dx_t
// and from g_u on the vertex kernel's backward applies unchanged, vertex by vertex.  (k2b_model_set_landmarks requires
// every landmark's weights to sum to 1 within 1e-3, so this is smplx's sum_k b_k x_u + transl to that accuracy.)
//
// Per call the host collects the selection's U distinct vertices (at most 3 x kSurfMaxTargets) and gathers their rows of
// v_template, shapedirs, posedirs ([PF][3U]: one row of pose features reads 3U contiguous floats) and lbs_weights into a
// compact table (k2b_surface_gather_kernel), cached per model and selection (k2b_api_model.hip).  Per iteration one 256-lane
// workgroup handles one frame: joints on the first wave, vertices / targets / pose features spread over all four waves,
// every reduction a fixed-order loop (a frame's result does not depend on the batch it rides in).
//
// The term has a second, PROJECTED form (k2b_surface_term_kernel<true>: k2b_surface_term_image, k2b_fit_image) for 2D keypoints:
// the same point x_t seen by a pinhole camera, e = (fx X / Z - u', fy Y / Z - v'), loss_t = w^2 c_t^2 (gmof(e_x) + gmof(e_y)),
// dL/dx_t = (g_x, g_y, -(X g_x + Y g_y) / Z) with g_x = fx gmof'(e_x) / Z.  Only the target block differs; the 3D instantiation
// keeps its code.
#include "k2b_internal.h"

namespace k2b {

namespace {

constexpr int kSurfThreads = 256;

__device__ __forceinline__ Vec3 axial_of_GRt_s(const Mat3& G, const Mat3& R) {
    // axial(G R^T): M = G R^T, result (M32 - M23, M13 - M31, M21 - M12)
    float M[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) M[3 * r + c] = G.m[3 * r] * R.m[3 * c] + G.m[3 * r + 1] * R.m[3 * c + 1] + G.m[3 * r + 2] * R.m[3 * c + 2];
    return {M[7] - M[5], M[2] - M[6], M[3] - M[1]};
}

// PROJ: the perspective form of the target block (k2b.h, k2b_fit_config::projection, as k2b_fit_tree.hip's joint term); everything
// before the point and after dL/dx_t is the 3D form's.
template <bool PROJ>
__global__ __launch_bounds__(kSurfThreads) void k2b_surface_term_kernel(const SurfaceTermArgs a) {
    constexpr int VJM = kMaxJoints, PFM = 9 * (kMaxJoints - 1), UM = kSurfMaxVerts, TM = kSurfMaxTargets;
    const int VJ = a.num_joints;
    __shared__ float sR[VJM][9], sRg[VJM][9], sp[VJM][3], sJr[VJM][3];
    __shared__ float sX[PFM + 1], sGX[PFM + 1];
    __shared__ float svp[UM][3], sx[UM][3], sgu[UM][3], sgvp[UM][3];
    __shared__ float sgt[TM][3], slt[TM], swt[TM];
    __shared__ float sF[VJM][3], sM[VJM][3], sgd[VJM][3], sgJ[VJM][3];
    __shared__ float sGrad[3 + 3 * (VJM - 1) + kMaxShape + 3];
    __shared__ int spar[VJM];

    const int f = blockIdx.x;
    const int tid = threadIdx.x;
    const int NB = a.num_betas, U = a.num_u, T = a.num_sel;
    const int PF = 9 * (VJ - 1);
    const int D = 3 * (VJ - 1);
    const int U3 = 3 * U;
    const bool isJ = tid < VJ;
    const float* be = a.be + (size_t)f * NB;

    // ---- joints: local rotation, rest joint, chain (as k2b_vertex_term_kernel) --------------------------------------
    Vec3 th = {0.f, 0.f, 0.f};
    int par = -1;
    Vec3 Jr = {0.f, 0.f, 0.f};
    if (isJ) {
        const float* src = tid == 0 ? a.go + (size_t)f * 3 : a.bp + (size_t)f * D + 3 * (tid - 1);
        th = {src[0], src[1], src[2]};
        par = a.parents[tid];
        float e[3];
        for (int c = 0; c < 3; ++c) {
            float s = a.j_template[tid * 3 + c];
            for (int k = 0; k < NB; ++k) s += a.j_dirs[(tid * 3 + c) * NB + k] * be[k];
            e[c] = s;
        }
        Jr = {e[0], e[1], e[2]};
    }
    const Rodrigues rod = rodrigues_fwd(th);
    if (isJ) {
        for (int i = 0; i < 9; ++i) sR[tid][i] = rod.R.m[i];
        sJr[tid][0] = Jr.x; sJr[tid][1] = Jr.y; sJr[tid][2] = Jr.z;
        spar[tid] = par < 0 ? -1 : par;
        if (tid > 0)
            for (int i = 0; i < 9; ++i) sX[(tid - 1) * 9 + i] = rod.R.m[i] - ((i % 4 == 0) ? 1.f : 0.f);
    }
    __syncthreads();
    Mat3 Rg = rod.R;
    Vec3 pg = Jr;
    if (isJ) {
        if (par >= 0) pg = Jr - Vec3{sJr[par][0], sJr[par][1], sJr[par][2]};
        for (int anc = par; anc >= 0; anc = spar[anc]) {
            Mat3 Ra;
            for (int i = 0; i < 9; ++i) Ra.m[i] = sR[anc][i];
            const int pa = spar[anc];
            const Vec3 da = pa >= 0 ? Vec3{sJr[anc][0] - sJr[pa][0], sJr[anc][1] - sJr[pa][1], sJr[anc][2] - sJr[pa][2]}
                                    : Vec3{sJr[anc][0], sJr[anc][1], sJr[anc][2]};
            pg = mul(Ra, pg) + da;
            Rg = mul(Ra, Rg);
        }
        for (int i = 0; i < 9; ++i) sRg[tid][i] = Rg.m[i];
        sp[tid][0] = pg.x; sp[tid][1] = pg.y; sp[tid][2] = pg.z;
    }
    __syncthreads();

    // ---- distinct vertices: blend shapes and skinning (no translation) ------------------------------------------------
    for (int u = tid; u < U; u += kSurfThreads) {
        float vp[3];
        for (int c = 0; c < 3; ++c) {
            float s = a.vt[u * 3 + c];
            for (int k = 0; k < NB; ++k) s += a.sd[(u * 3 + c) * NB + k] * be[k];
            for (int k = 0; k < PF; ++k) s += a.pd[(size_t)k * U3 + u * 3 + c] * sX[k];
            vp[c] = s;
        }
        Vec3 x = {0.f, 0.f, 0.f};
        for (int j = 0; j < VJ; ++j) {
            const float w = a.lw[u * VJ + j];
            Mat3 R;
            for (int i = 0; i < 9; ++i) R.m[i] = sRg[j][i];
            const Vec3 q = mul(R, Vec3{vp[0] - sJr[j][0], vp[1] - sJr[j][1], vp[2] - sJr[j][2]}) + Vec3{sp[j][0], sp[j][1], sp[j][2]};
            x.x += w * q.x; x.y += w * q.y; x.z += w * q.z;
        }
        svp[u][0] = vp[0]; svp[u][1] = vp[1]; svp[u][2] = vp[2];
        sx[u][0] = x.x; sx[u][1] = x.y; sx[u][2] = x.z;
    }
    __syncthreads();

    // ---- targets: weighted point, GMoF loss, dL/dx --------------------------------------------------------------------
    const float tx = a.tr[(size_t)f * 3], ty = a.tr[(size_t)f * 3 + 1], tz = a.tr[(size_t)f * 3 + 2];
    for (int t = tid; t < T; t += kSurfThreads) {
        Vec3 x = {0.f, 0.f, 0.f};
        float sw = 0.f;
        for (int k = 0; k < 3; ++k) {
            const float w = a.pair_w[t * 3 + k];
            const int u = a.pair_u[t * 3 + k];
            x.x += w * sx[u][0]; x.y += w * sx[u][1]; x.z += w * sx[u][2];
            sw += w;
        }
        const int kcol = a.sel_k[t];
        const float* y = a.targets + ((size_t)f * a.num_targets + kcol) * 3;
        swt[t] = sw;
        const float cf = a.conf ? a.conf[(a.conf_per_frame ? (size_t)f * a.num_targets : 0) + kcol] : 1.0f;
        const float wc = (a.joint_w * a.joint_w) * (cf * cf);
        const float s2 = a.sigma * a.sigma;
        if constexpr (PROJ) {
            // e = (fx X / Z - u', fy Y / Z - v'), the target row (u', v', ignored) in centred pixels, sigma in pixels.  Z is divided
            // by as it stands (IEEE division, no clamp: a point behind the camera is legal), so a target of confidence 0 is left
            // out by the branch, not by its weight (0 . inf at Z = 0).
            float l = 0.f;
            Vec3 g = {0.f, 0.f, 0.f};
            if (cf != 0.f) {
                const float X = x.x + sw * tx, Y = x.y + sw * ty, iz = 1.0f / (x.z + sw * tz);
                const float ex = a.focal_x * X * iz - y[0], ey = a.focal_y * Y * iz - y[1];
                const float x2 = ex * ex, y2 = ey * ey;
                const float dx = s2 + x2, dy = s2 + y2;
                l = wc * ((s2 * x2) / dx + (s2 * y2) / dy);
                const float k2 = 2.f * wc * (s2 * s2);
                const float gx = a.focal_x * (k2 * ex / (dx * dx)) * iz, gy = a.focal_y * (k2 * ey / (dy * dy)) * iz;
                g = {gx, gy, -(X * gx + Y * gy) * iz};
            }
            slt[t] = l;
            sgt[t][0] = g.x; sgt[t][1] = g.y; sgt[t][2] = g.z;
            continue;
        }
        const float ex = x.x + sw * tx - y[0], ey = x.y + sw * ty - y[1], ez = x.z + sw * tz - y[2];
        const float x2 = ex * ex, y2 = ey * ey, z2 = ez * ez;
        const float dx = s2 + x2, dy = s2 + y2, dz = s2 + z2;
        slt[t] = wc * ((s2 * x2) / dx + (s2 * y2) / dy + (s2 * z2) / dz);
        const float k2 = 2.f * wc * (s2 * s2);
        sgt[t][0] = k2 * ex / (dx * dx); sgt[t][1] = k2 * ey / (dy * dy); sgt[t][2] = k2 * ez / (dz * dz);
    }
    __syncthreads();

    // ---- vertices: dL/dx_u (CSR of the pairs, fixed order), dL/dvp = sum_j w_j Rg_j^T g -------------------------------
    for (int u = tid; u < U; u += kSurfThreads) {
        Vec3 g = {0.f, 0.f, 0.f};
        for (int i = a.inv_off[u]; i < a.inv_off[u + 1]; ++i) {
            const int t = a.inv_t[i];
            const float w = a.inv_w[i];
            g.x += w * sgt[t][0]; g.y += w * sgt[t][1]; g.z += w * sgt[t][2];
        }
        Vec3 gvp = {0.f, 0.f, 0.f};
        for (int j = 0; j < VJ; ++j) {
            const float w = a.lw[u * VJ + j];
            Mat3 R;
            for (int i = 0; i < 9; ++i) R.m[i] = sRg[j][i];
            const Vec3 t = mulT(R, g);
            gvp.x += w * t.x; gvp.y += w * t.y; gvp.z += w * t.z;
        }
        sgu[u][0] = g.x; sgu[u][1] = g.y; sgu[u][2] = g.z;
        sgvp[u][0] = gvp.x; sgvp[u][1] = gvp.y; sgvp[u][2] = gvp.z;
    }
    __syncthreads();

    // ---- joints: force and moment of the vertices attached to each joint; pose-blend gradient G_X = Pd^T g_vp ----------
    if (isJ) {
        Vec3 F = {0.f, 0.f, 0.f}, M = {0.f, 0.f, 0.f};
        for (int u = 0; u < U; ++u) {
            const float w = a.lw[u * VJ + tid];
            const Vec3 ge = {sgu[u][0], sgu[u][1], sgu[u][2]};
            const Vec3 q = mul(Rg, Vec3{svp[u][0] - Jr.x, svp[u][1] - Jr.y, svp[u][2] - Jr.z}) + pg;
            const Vec3 m = cross(q, ge);
            F.x += w * ge.x; F.y += w * ge.y; F.z += w * ge.z;
            M.x += w * m.x; M.y += w * m.y; M.z += w * m.z;
        }
        sF[tid][0] = F.x; sF[tid][1] = F.y; sF[tid][2] = F.z;
        sM[tid][0] = M.x; sM[tid][1] = M.y; sM[tid][2] = M.z;
    }
    for (int k = tid; k < PF; k += kSurfThreads) {
        const float* row = a.pd + (size_t)k * U3;
        float s = 0.f;
        for (int u = 0; u < U; ++u) s += row[u * 3] * sgvp[u][0] + row[u * 3 + 1] * sgvp[u][1] + row[u * 3 + 2] * sgvp[u][2];
        sGX[k] = s;
    }
    __syncthreads();

    // ---- joints: subtree sums, torque, pull-back ---------------------------------------------------------------------
    if (isJ) {
        Vec3 aj = {0.f, 0.f, 0.f}, tj = {0.f, 0.f, 0.f};
        for (int k = 0; k < VJ; ++k) {          // k in subtree(tid)  <=>  tid is k or an ancestor of k
            bool below = false;
            for (int t = k; t >= 0; t = spar[t])
                if (t == tid) { below = true; break; }
            if (below) {
                aj.x += sF[k][0]; aj.y += sF[k][1]; aj.z += sF[k][2];
                tj.x += sM[k][0]; tj.y += sM[k][1]; tj.z += sM[k][2];
            }
        }
        const Vec3 torque = tj - cross(pg, aj);
        Vec3 w = mul(rod.R, mulT(Rg, torque));
        const Vec3 gd = mul(rod.R, mulT(Rg, aj));                   // dL/d(Jr_j - Jr_par)
        if (tid > 0) {
            Mat3 G;
            for (int i = 0; i < 9; ++i) G.m[i] = sGX[(tid - 1) * 9 + i];
            w = w + axial_of_GRt_s(G, rod.R);
        }
        const float a1 = rod.s * rod.inv_angle, a3 = (1.0f - rod.c) * rod.inv_angle;
        const float uw = rod.u.x * w.x + rod.u.y * w.y + rod.u.z * w.z;
        const float a2uw = (1.0f - a1) * uw;
        const Vec3 uxw = cross(rod.u, w);
        float* dst = tid == 0 ? sGrad : sGrad + 3 + 3 * (tid - 1);
        dst[0] = a1 * w.x + a2uw * rod.u.x - a3 * uxw.x;
        dst[1] = a1 * w.y + a2uw * rod.u.y - a3 * uxw.y;
        dst[2] = a1 * w.z + a2uw * rod.u.z - a3 * uxw.z;
        const Vec3 gJ = mulT(Rg, Vec3{sF[tid][0], sF[tid][1], sF[tid][2]});   // dL/dJr_j = -Rg_j^T F_j
        sgd[tid][0] = gd.x; sgd[tid][1] = gd.y; sgd[tid][2] = gd.z;
        sgJ[tid][0] = gJ.x; sgJ[tid][1] = gJ.y; sgJ[tid][2] = gJ.z;
    }
    __syncthreads();

    // ---- shape coefficients (joint offsets, rest joints, vertex shape blend), loss and translation ---------------------
    if (tid < NB) {
        const int k = tid;
        float s = 0.f;
        for (int j = 0; j < VJ; ++j) {
            const int pj = spar[j];
            for (int c = 0; c < 3; ++c) {
                const float dj = a.j_dirs[(j * 3 + c) * NB + k];
                const float dp = pj >= 0 ? a.j_dirs[(pj * 3 + c) * NB + k] : 0.f;
                s += sgd[j][c] * (dj - dp) - sgJ[j][c] * dj;
            }
        }
        for (int u = 0; u < U; ++u)
            for (int c = 0; c < 3; ++c) s += a.sd[(u * 3 + c) * NB + k] * sgvp[u][c];
        sGrad[3 + D + k] = s;
    } else if (tid >= 128 && tid < 132) {
        const int c = tid - 128;                 // 0..2: translation component, 3: loss
        float s = 0.f;
        for (int t = 0; t < T; ++t) s += c < 3 ? swt[t] * sgt[t][c] : slt[t];
        if (c < 3) sGrad[3 + D + NB + c] = s;
        else a.loss_out[f] = s + (a.loss_in ? a.loss_in[f] : 0.f);
    }
    __syncthreads();

    // ---- outputs -----------------------------------------------------------------------------------------------------
    const int P = 3 + D + NB + 3;
    if (!a.grad_in) {
        for (int p = tid; p < P; p += kSurfThreads) a.grad_out[(size_t)f * P + p] = sGrad[p];
        return;
    }
    // Adam tail, as k2b_vertex_term_kernel's
    const float2 co = *a.adam_coef;
    const float inv_bc2 = fast_rcp(co.y);
    for (int p = tid; p < P; p += kSurfThreads) {
        const int group = p < 3 ? 0 : (p < 3 + D ? 1 : (p < 3 + D + NB ? 2 : 3));
        const bool opt = ((a.opt_mask >> group) & 1) && !(group == 2 && p - 3 - D < a.frozen_shape);
        const float g = opt ? a.grad_in[(size_t)f * P + p] + sGrad[p] : 0.f;
        if (a.grad_out) a.grad_out[(size_t)f * P + p] = g;
        float* x = group == 0 ? a.go_w + (size_t)f * 3 + p
                 : (group == 1 ? a.bp_w + (size_t)f * D + (p - 3)
                 : (group == 2 ? a.be_w + (size_t)f * NB + (p - 3 - D) : a.tr_w + (size_t)f * 3 + (p - 3 - D - NB)));
        const size_t i = (size_t)f * P + p;
        const float mi = a.adam_m[i] + a.one_minus_beta1 * (g - a.adam_m[i]);
        const float vi = a.adam_v[i] * a.beta2 + a.one_minus_beta2 * g * g;
        const float denom = fast_sqrt(vi) * inv_bc2 + a.eps;
        a.adam_m[i] = mi;
        a.adam_v[i] = vi;
        *x = *x - co.x * (mi * fast_rcp(denom));
    }
}

// Compact rows of n vertices: vt [n][3], sd [n][3][NB], pd [PF][3n], lw [n][J]
__global__ __launch_bounds__(256) void k2b_surface_gather_kernel(const float* __restrict__ v_template, const float* __restrict__ shapedirs,
                                                                 const float* __restrict__ posedirs, const float* __restrict__ lbs_weights,
                                                                 const int* __restrict__ ids, int n, int V, int J, int NB,
                                                                 float* vt, float* sd, float* pd, float* lw) {
    const int PF = 9 * (J - 1);
    const long long n_vt = 3LL * n, n_sd = 3LL * n * NB, n_pd = (long long)PF * 3 * n, n_lw = (long long)n * J;
    const long long total = n_vt + n_sd + n_pd + n_lw;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        long long r = i;
        if (r < n_vt) { const int u = (int)(r / 3), c = (int)(r % 3); vt[r] = v_template[(size_t)ids[u] * 3 + c]; continue; }
        r -= n_vt;
        if (r < n_sd) { const int u = (int)(r / (3 * NB)); const int rest = (int)(r % (3 * NB)); sd[r] = shapedirs[(size_t)ids[u] * 3 * NB + rest]; continue; }
        r -= n_sd;
        if (r < n_pd) {
            const long long k = r / (3LL * n);
            const int col = (int)(r % (3LL * n)), u = col / 3, c = col % 3;
            pd[r] = posedirs[(size_t)k * 3 * V + (size_t)ids[u] * 3 + c];
            continue;
        }
        r -= n_pd;
        { const int u = (int)(r / J), j = (int)(r % J); lw[r] = lbs_weights[(size_t)ids[u] * J + j]; }
    }
}

// joints[f][row0 + l] = sum_k w[l][k] src[f][ids[l][k]]
__global__ __launch_bounds__(256) void k2b_landmarks_kernel(const float* __restrict__ src, int src_stride, const int* __restrict__ ids,
                                                            const float* __restrict__ w, float* joints, int out_stride, int row0,
                                                            int num_frames, int L) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)num_frames * L) return;
    const int f = (int)(i / L), l = (int)(i % L);
    float x = 0.f, y = 0.f, z = 0.f;
    for (int k = 0; k < 3; ++k) {
        const float* s = src + ((size_t)f * src_stride + ids[l * 3 + k]) * 3;
        const float b = w[l * 3 + k];
        x += b * s[0]; y += b * s[1]; z += b * s[2];
    }
    float* d = joints + ((size_t)f * out_stride + row0 + l) * 3;
    d[0] = x; d[1] = y; d[2] = z;
}

}  // namespace

hipError_t launch_surface_term(const SurfaceTermArgs& a, hipStream_t stream) {
    if (a.num_frames <= 0 || a.num_sel <= 0) return hipSuccess;
    if (a.num_sel > kSurfMaxTargets || a.num_u < 1 || a.num_u > kSurfMaxVerts || a.num_joints < 1 || a.num_joints > kMaxJoints ||
        a.num_betas > kMaxShape)
        return hipErrorInvalidValue;
    if (a.projection)
        hipLaunchKernelGGL(k2b_surface_term_kernel<true>, dim3(a.num_frames), dim3(kSurfThreads), 0, stream, a);
    else
        hipLaunchKernelGGL(k2b_surface_term_kernel<false>, dim3(a.num_frames), dim3(kSurfThreads), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_surface_gather(const float* v_template, const float* shapedirs, const float* posedirs, const float* lbs_weights,
                                 const int* ids, int n, int V, int J, int NB, float* vt, float* sd, float* pd, float* lw,
                                 hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k2b_surface_gather_kernel, dim3(256), dim3(256), 0, stream, v_template, shapedirs, posedirs, lbs_weights, ids, n,
                       V, J, NB, vt, sd, pd, lw);
    return hipGetLastError();
}

hipError_t launch_landmarks(const float* src, int src_stride, const int* ids, const float* w, float* joints, int out_stride, int row0,
                            int num_frames, int L, hipStream_t stream) {
    if (num_frames <= 0 || L <= 0) return hipSuccess;
    const long long n = (long long)num_frames * L;
    hipLaunchKernelGGL(k2b_landmarks_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, src, src_stride, ids, w, joints,
                       out_stride, row0, num_frames, L);
    return hipGetLastError();
}

}  // namespace k2b
