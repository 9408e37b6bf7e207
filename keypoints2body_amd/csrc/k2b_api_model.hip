// k2b_api_model.hip — the model handle of the C ABI (include/k2b.h): constants and their kernel-side images, the tree
// tables of the two fit kernels, landmarks, and the per-model tables and workspaces that calls build on first use.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <numeric>

#include "k2b_host.h"

#ifndef K2B_LBS_STREAM
#define K2B_LBS_STREAM 1      // 0: development builds that keep the tile kernel for 17-24 joint models (A/B timing)
#endif

using namespace k2b::host;

namespace {
// LBS B operands of a vertex set from HOST constants in which vertex v's rows are those of `ids`: the images of the model's
// route (k2b_model_tables.h, vertex_set_images) go up; a stream model has none of the tile kernel's (SMPL-X: 64 MB less per GPU)
int build_vertex_set(k2b_model* m, VertexSet& vs, const std::vector<int>& ids, const std::vector<int>& tag,
                     const float* v_template, const float* shapedirs, const float* posedirs, const float* lbs_weights, int V) {
    // (the e4m3 strips of a subset of the mesh take the mesh's scales: a vertex has the same codes in every set)
    const bool subset = &vs != &m->mesh;
    const k2b::tables::VertexSetShape shape{m->J, m->NB, m->P, m->lbs.k_steps_x, m->lbs.w_frags, m->lbs.pose_fp8, subset, m->mesh.pd8_lo_exp, m->mesh.pd8_hi_exp};
    const k2b::tables::VertexSetImages im = k2b::tables::vertex_set_images(shape, ids, tag, v_template, shapedirs, posedirs, lbs_weights, V);
    vs.num = (int)ids.size();
    vs.v_tiles = im.v_tiles;
    vs.nv16 = im.nv16;
    vs.pd8_lo_exp = im.pd8_lo_exp;
    vs.pd8_hi_exp = im.pd8_hi_exp;
    const std::pair<DevBuf<k2b::k2b_half>*, const std::vector<k2b::k2b_half>*> images[] = {
        {&vs.spd, &im.spd}, {&vs.sw, &im.sw}, {&vs.w2, &im.w2}, {&vs.pdh, &im.pdh}, {&vs.pdl, &im.pdl}};
    for (const auto& [dev, host] : images)
        if (!host->empty())
            if (const hipError_t e = dev->upload(host->data(), host->size()); e != hipSuccess) return (int)e;
    return 0;
}

// k2b_model_set_landmarks after validation, caller holds m->mu
int set_landmarks_locked(k2b_model* m, int32_t L, const int32_t* vertex_ids, const float* bary) {
    k2b_model::Landmarks& lm = m->lmk;
    lm.h_ids.assign(vertex_ids, vertex_ids + 3 * L);
    lm.h_w.assign(bary, bary + 3 * L);
    std::vector<int> seq(3 * L);
    for (int i = 0; i < 3 * L; ++i) seq[i] = i;
    HIP_TRY(lm.ids.upload(vertex_ids, (size_t)3 * L));
    HIP_TRY(lm.w.upload(bary, (size_t)3 * L));
    HIP_TRY(lm.seq.upload(seq.data(), seq.size()));
    // LBS operands of the 3L vertices: their rows gathered on the device, then laid out on the host like the extra joints'
    const int n = 3 * L, J = m->J, NB = m->NB, PF = m->P;
    const size_t nf = (size_t)n * 3 + (size_t)n * 3 * NB + (size_t)PF * 3 * n + (size_t)n * J;
    DevBuf<float> g;
    HIP_TRY(g.alloc(nf));
    float *gvt = g.get(), *gsd = gvt + (size_t)n * 3, *gpd = gsd + (size_t)n * 3 * NB, *glw = gpd + (size_t)PF * 3 * n;
    hipError_t e = k2b::launch_surface_gather(m->v_template.get(), m->shapedirs.get(), m->posedirs.get(), m->lbs_weights.get(), lm.ids.get(), n, m->V, J, NB,
                                              gvt, gsd, gpd, glw, nullptr);
    std::vector<float> h(nf);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(h.data(), g.get(), nf * sizeof(float), hipMemcpyDeviceToHost);
    (void)g.reset();
    if (e != hipSuccess) return fail(K2B_ERR_HIP, "k2b_model_set_landmarks: gathering the landmark vertices failed: %s", hipGetErrorString(e));
    const float* hvt = h.data();
    const float *hsd = hvt + (size_t)n * 3, *hpd = hsd + (size_t)n * 3 * NB, *hlw = hpd + (size_t)PF * 3 * n;
    if (build_vertex_set(m, lm.verts, seq, std::vector<int>(), hvt, hsd, hpd, hlw, n) != 0)
        return fail(K2B_ERR_HIP, "k2b_model_set_landmarks: uploading LBS operands failed");
    lm.L = L;
    // a workspace reserved before this call covers the landmark vertices too
    if (m->ws_bpad > 0) return reserve_lbs_workspace(m, m->ws_bpad);
    return K2B_OK;
}

// ---- the steps of k2b_model_create, in its order -------------------------------------------------------------------------------
// LBS operands: the route (stream kernels or the tile kernel), then the B side of the two GEMMs for the mesh and the extra joints
int create_lbs_operands(k2b_model* m, const float* v_template, const float* shapedirs, const float* posedirs, const float* lbs_weights) {
    const int V = m->V, E = m->E;
    // development switch K2B_LBS_TILE (non-zero): this model is skinned by the tile kernel whatever the stream kernels would
    // take - their run-time twin.  Per model, fixed here; nothing else reads it.
    const char* tile_env = getenv("K2B_LBS_TILE");
    // development switch K2B_LBS_POSE_F16 (non-zero): a model of the route `stream` keeps the three f16 products of the pose phase
    // (images, pose set-up and kernel) - the run-time twin of the e4m3 form, and the choice for a model with large pose
    // correctives (k2b_lbs_plan.h, lbs_route).  Per model, fixed here; nothing else reads it.
    const char* f16_env = getenv("K2B_LBS_POSE_F16");
    m->lbs = k2b::lbs_route(m->J, m->NB, K2B_LBS_STREAM != 0, tile_env && atoi(tile_env) != 0, f16_env && atoi(f16_env) != 0);
    HIP_TRY(m->dump.alloc(64 * 1024 / sizeof(float)));     // 64 x 3 floats used; the rest is room for diagnostic builds
    std::vector<int> all(V), tag(V, 0);
    std::iota(all.begin(), all.end(), 0);
    // an output joint rides in the W image of its vertex (k2b_lbs.hip) - unless two joints share a vertex or the index
    // does not fit an f16 integer, in which case the gather launch stays
    m->joints_in_mesh = E > 0 && E <= 1024;
    for (int e = 0; e < E && m->joints_in_mesh; ++e) {
        if (tag[m->h_extra_ids[e]]) m->joints_in_mesh = false;
        tag[m->h_extra_ids[e]] = e + 1;
    }
    if (!m->joints_in_mesh) std::fill(tag.begin(), tag.end(), 0);
    if (build_vertex_set(m, m->mesh, all, tag, v_template, shapedirs, posedirs, lbs_weights, V) != 0 ||
        (E > 0 && build_vertex_set(m, m->extra, m->h_extra_ids, std::vector<int>(), v_template, shapedirs, posedirs, lbs_weights, V) != 0))
        return fail(K2B_ERR_HIP, "k2b_model_create: uploading LBS operands failed");
    return K2B_OK;
}

// joint basis: the J x V contraction on the matrix cores, its host copy, and the lane-major image of the pose set-up kernel
int create_joint_basis(k2b_model* m) {
    const int V = m->V, J = m->J, NB = m->NB, splits = 32;
    const int Jp = (J + 15) / 16 * 16, Np = (3 * NB + 15) / 16 * 16;
    DevBuf<float> ws;
    HIP_TRY(ws.alloc((size_t)splits * Jp * Np));
    HIP_TRY(m->j_template.alloc((size_t)J * 3));
    HIP_TRY(m->j_dirs.alloc((size_t)J * 3 * NB));
    HIP_TRY(k2b::launch_jreg_contract(m->j_regressor.get(), m->v_template.get(), m->j_template.get(), J, V, 3, ws.get(), splits, nullptr));
    HIP_TRY(k2b::launch_jreg_contract(m->j_regressor.get(), m->shapedirs.get(), m->j_dirs.get(), J, V, 3 * NB, ws.get(), splits, nullptr));
    HIP_TRY(hipDeviceSynchronize());
    m->h_j_template.resize((size_t)J * 3);
    m->h_j_dirs.resize((size_t)J * 3 * NB);
    HIP_TRY(hipMemcpy(m->h_j_template.data(), m->j_template.get(), m->h_j_template.size() * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(m->h_j_dirs.data(), m->j_dirs.get(), m->h_j_dirs.size() * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(ws.reset());
    // the same numbers lane-major for the pose set-up kernel (lane = joint): one of its loads touches 1-2 cache lines instead
    // of one per joint
    std::vector<float> lane((size_t)3 * (1 + NB) * 64, 0.f);
    for (int j = 0; j < J; ++j)
        for (int c = 0; c < 3; ++c) {
            lane[((size_t)c * (1 + NB)) * 64 + j] = m->h_j_template[j * 3 + c];
            for (int k = 0; k < NB; ++k) lane[((size_t)c * (1 + NB) + 1 + k) * 64 + j] = m->h_j_dirs[((size_t)j * 3 + c) * NB + k];
        }
    HIP_TRY(m->j_basis_lane.upload(lane.data(), lane.size()));
    return K2B_OK;
}

// tables of the fused fit kernel, by lane (k2b_model_tables.h, fused_tables); empty for a model the kernel does not take
int create_fused_tables(k2b_model* m) {
    const k2b::Tree& t = m->kin;
    bool ok = (m->J == k2b::kFitJoints) && m->NB <= k2b::kMaxBetas;
    if (!ok) m->fit_why = "the 24-lane fused fit kernel is built for the 24-joint SMPL tree with <= 16 betas";
    if (ok && (k2b::rounds_for_depth(t.max_depth) > k2b::kMaxRounds || m->J > 32)) { ok = false; m->fit_why = "tree too deep / large for the fused fit kernel"; }
    // Development switch K2B_FIT_SCAN64 (non-zero): this model gets the DFS placement and the fp64 scans whatever its tree allows -
    // the run-time twin of the fp32 form.  Per model, fixed here; nothing else reads it.
    const char* scan_env = getenv("K2B_FIT_SCAN64");
    k2b::ScanPlan plan;
    if (ok && !(scan_env && atoi(scan_env) != 0)) plan = k2b::fit_scan_plan(t);
    m->fit_scan64 = !plan.valid;
    const k2b::tables::LaneTables f = ok ? k2b::tables::fused_tables(t, plan, m->NB, m->h_j_template.data(), m->h_j_dirs.data()) : k2b::tables::fused_tables_empty();
    HIP_TRY(m->dt.upload(f.dt.data(), f.dt.size()));
    HIP_TRY(m->dd.upload(f.dd.data(), f.dd.size()));
    HIP_TRY(m->tree.upload(f.tab.data(), f.tab.size()));
    m->fit_ok = ok;
    return K2B_OK;
}

// tables of the tree fit kernel (k2b_model_tables.h, tree_tables); the lane table goes up per prior width (tree_lane_table)
int create_tree_tables(k2b_model* m) {
    k2b::tables::LaneTables t = k2b::tables::tree_tables(m->kin, m->NB, m->h_j_template.data(), m->h_j_dirs.data());
    HIP_TRY(m->tt_anc.upload(t.anc.data(), t.anc.size()));
    HIP_TRY(m->tt_dt.upload(t.dt.data(), t.dt.size()));
    HIP_TRY(m->tt_dd.upload(t.dd.data(), t.dd.size()));
    m->h_tt_tab = std::move(t.tab);
    return K2B_OK;
}
}  // namespace

namespace k2b {
namespace host {

// Adam bias terms in double, exactly as torch/optim/adam.py computes them in Python floats; cached per model
int adam_table(k2b_model* model, const k2b_fit_config* cfg, hipStream_t stream, float2** out) {
    std::lock_guard<std::mutex> lk(model->mu);
    const auto key = std::make_tuple((int)cfg->num_iters, cfg->step_size, cfg->adam_beta1, cfg->adam_beta2);
    auto it = model->adam_tables.find(key);
    if (it != model->adam_tables.end()) {
        it->second.last_use = ++model->adam_clock;
        *out = it->second.dev.get();
        return K2B_OK;
    }
    std::vector<float2> h(cfg->num_iters);
    const double lr = cfg->step_size, b1 = cfg->adam_beta1, b2 = cfg->adam_beta2;
    for (int t = 1; t <= cfg->num_iters; ++t) {
        const double bc1 = 1.0 - std::pow(b1, (double)t), bc2 = 1.0 - std::pow(b2, (double)t);
        h[t - 1] = make_float2((float)(lr / bc1), (float)std::sqrt(bc2));
    }
    constexpr size_t kMaxAdamTables = 64;
    if (model->adam_tables.size() >= kMaxAdamTables) {
        HIP_TRY(hipStreamSynchronize(stream));               // a launch in flight may still read the table that leaves
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(evict_lru(model->adam_tables));
    }
    DevBuf<float2> coef;
    HIP_TRY(coef.upload(h.data(), h.size()));
    *out = coef.get();
    model->adam_tables.emplace(key, k2b_model::AdamTable{std::move(coef), ++model->adam_clock});
    return K2B_OK;
}

// The tree kernel's lane table for a prior over the first prior_dims pose dimensions (checked by the caller): one immutable
// [64][8] table per width, built and uploaded on the first use of that width (at most 21 widths of 2 KB: nothing is evicted).
int tree_lane_table(k2b_model* m, int prior_dims, const int** out) {
    std::lock_guard<std::mutex> lk(m->mu);
    auto it = m->tt_tabs.find(prior_dims);
    if (it == m->tt_tabs.end()) {
        const std::vector<int> tab = k2b::tables::tree_tab_with_prior(m->h_tt_tab, m->kin, prior_dims);
        DevBuf<int> dev;
        HIP_TRY(dev.upload(tab.data(), tab.size()));
        it = m->tt_tabs.emplace(prior_dims, std::move(dev)).first;
    }
    *out = it->second.get();
    return K2B_OK;
}

// Compact table of the surface-point term for targets sel[t] (model joint indices >= J) in target columns col[t]: the U distinct
// vertices in order of first appearance, their rows gathered on the device, the (slot, weight) pairs of every target and the
// pairs of every vertex (CSR).  Cached per model and selection; the first use of a selection synchronises `stream`.
int surface_table(k2b_model* m, const std::vector<int>& sel, const std::vector<int>& col, hipStream_t stream, k2b::SurfaceTermArgs* out) {
    const int J = m->J, E = m->E, NB = m->NB, PF = m->P, T = (int)sel.size();
    if (T < 1 || T > k2b::kSurfMaxTargets)
        return fail(K2B_ERR_UNSUPPORTED, "k2b_fit_world: %d surface targets (vertex-selected joints and landmarks), at most %d per call", T,
                    k2b::kSurfMaxTargets);
    std::vector<int> key;
    for (int t = 0; t < T; ++t) { key.push_back(sel[t]); key.push_back(col[t]); }
    std::lock_guard<std::mutex> lk(m->mu);
    auto it = m->surface_tables.find(key);
    if (it != m->surface_tables.end()) {
        it->second.last_use = ++m->surface_clock;
        *out = it->second.a;
        return K2B_OK;
    }
    std::vector<int> pair_v(3 * T, -1);                      // the pairs of every target: one vertex of weight 1, or a landmark's triangle
    std::vector<float> pair_w(3 * T, 0.f);
    for (int t = 0; t < T; ++t) {
        const int j = sel[t];
        if (j < J + E) { pair_v[t * 3] = m->h_extra_ids[j - J]; pair_w[t * 3] = 1.f; continue; }
        for (int k = 0; k < 3; ++k) { pair_v[t * 3 + k] = m->lmk.h_ids[(j - J - E) * 3 + k]; pair_w[t * 3 + k] = m->lmk.h_w[(j - J - E) * 3 + k]; }
    }
    const k2b::tables::SurfaceIndex ix = k2b::tables::surface_index(T, pair_v, pair_w);
    const int U = (int)ix.ids.size(), n = (int)ix.inv_t.size();
    // one allocation: floats (vt, sd, pd, lw, pair_w, inv_w), then ints (pair_u, sel_k, inv_off, inv_t, ids)
    const size_t n_tab = (size_t)U * 3 + (size_t)U * 3 * NB + (size_t)PF * 3 * U + (size_t)U * J;
    const size_t n_f = n_tab + 3 * (size_t)T + (size_t)n;
    const size_t n_i = 3 * (size_t)T + T + (U + 1) + (size_t)n + U;
    std::vector<float> hf(ix.pair_w);
    hf.insert(hf.end(), ix.inv_w.begin(), ix.inv_w.end());
    std::vector<int> hi(ix.pair_u);
    for (const std::vector<int>* part : {&col, &ix.inv_off, &ix.inv_t, &ix.ids}) hi.insert(hi.end(), part->begin(), part->end());
    constexpr size_t kMaxSurfaceTables = 64;
    if (m->surface_tables.size() >= kMaxSurfaceTables) {
        HIP_TRY(hipDeviceSynchronize());                     // a launch in flight may still read the table that leaves
        HIP_TRY(evict_lru(m->surface_tables));
    }
    k2b_model::SurfaceTable st;                              // released on the failure returns below
    HIP_TRY(st.dev.alloc(n_f * sizeof(float) + n_i * sizeof(int)));
    float* f = reinterpret_cast<float*>(st.dev.get());
    int* ip = reinterpret_cast<int*>(f + n_f);
    if (hipMemcpy(f + n_tab, hf.data(), hf.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(ip, hi.data(), hi.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess)
        return fail(K2B_ERR_HIP, "k2b_fit_world: uploading the surface-term table failed");
    k2b::SurfaceTermArgs& a = st.a;
    a.vt = f; a.sd = f + (size_t)U * 3; a.pd = a.sd + (size_t)U * 3 * NB; a.lw = a.pd + (size_t)PF * 3 * U;
    a.pair_w = f + n_tab; a.inv_w = a.pair_w + 3 * T;
    a.pair_u = ip; a.sel_k = ip + 3 * T; a.inv_off = a.sel_k + T; a.inv_t = a.inv_off + U + 1;
    const int* dids = a.inv_t + n;
    a.j_template = m->j_template.get(); a.j_dirs = m->j_dirs.get(); a.parents = m->parents.get();
    a.num_u = U; a.num_betas = NB; a.num_joints = J; a.num_sel = T;
    if (k2b::launch_surface_gather(m->v_template.get(), m->shapedirs.get(), m->posedirs.get(), m->lbs_weights.get(), dids, U, m->V, J, NB, f, const_cast<float*>(a.sd),
                                   const_cast<float*>(a.pd), const_cast<float*>(a.lw), stream) != hipSuccess ||
        hipStreamSynchronize(stream) != hipSuccess)
        return fail(K2B_ERR_HIP, "k2b_fit_world: gathering the surface-term table failed");
    st.last_use = ++m->surface_clock;
    *out = a;
    m->surface_tables.emplace(key, std::move(st));
    return K2B_OK;
}

// grow-only per-model workspace of the per-frame LBS operands (caller holds m->mu)
int reserve_lbs_workspace(k2b_model* m, int bpad) {
    const k2b::LbsWorkspace n = k2b::lbs_workspace(m->lbs, bpad, m->lmk.L);
    if (m->lmk.L > 0 && bpad > m->lmk.ws_bpad) {             // the landmark vertices of joints-only calls
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(m->lmk.ws.reset());
        m->lmk.ws_bpad = 0;
        HIP_TRY(m->lmk.ws.alloc(n.landmark_floats));
        m->lmk.ws_bpad = bpad;
    }
    if (bpad <= m->ws_bpad) return K2B_OK;
    HIP_TRY(hipDeviceSynchronize());
    for (auto* w : {&m->wsXh, &m->wsXl, &m->wsA2}) HIP_TRY(w->reset());
    m->ws_bpad = 0;
    const size_t nx = n.x_halfs, na2 = n.a2_halfs;
    HIP_TRY(m->wsA2.alloc(na2));
    HIP_TRY(hipMemset(m->wsA2.get(), 0, na2 * sizeof(k2b::k2b_half)));    // PAD / ZERO groups and padding frames stay zero
    HIP_TRY(m->wsXh.alloc(nx));
    HIP_TRY(m->wsXl.alloc(nx));
    // rows of padding frames are never written by the set-up kernel: keep them finite
    HIP_TRY(hipMemset(m->wsXh.get(), 0, nx * sizeof(k2b::k2b_half)));
    HIP_TRY(hipMemset(m->wsXl.get(), 0, nx * sizeof(k2b::k2b_half)));
    m->ws_bpad = bpad;
    return K2B_OK;
}

}  // namespace host
}  // namespace k2b

extern "C" {

int k2b_model_create(k2b_model** out, int32_t V, int32_t J, int32_t NB, int32_t E, const float* v_template,
                     const float* shapedirs, const float* posedirs, const float* j_regressor,
                     const float* lbs_weights, const int32_t* parents, const int32_t* extra_vertex_ids) {
    if (!out) return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_model_create: out is NULL");
    *out = nullptr;
    if (V <= 0 || J < 2 || J > k2b::kMaxJoints || NB < 1 || NB > k2b::kMaxShape || E < 0)
        return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_model_create: bad sizes V=%d J=%d NB=%d E=%d (need 2<=J<=64, 1<=NB<=32)", V, J, NB, E);
    if (!v_template || !shapedirs || !posedirs || !j_regressor || !lbs_weights || !parents || (E > 0 && !extra_vertex_ids))
        return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_model_create: NULL constant array");
    if (parents[0] >= 0) return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_model_create: parents[0] must be -1 (root)");
    for (int j = 1; j < J; ++j)
        if (parents[j] < 0 || parents[j] >= j)
            return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_model_create: parents[%d]=%d must be in [0,%d)", j, parents[j], j);
    for (int e = 0; e < E; ++e)
        if (extra_vertex_ids[e] < 0 || extra_vertex_ids[e] >= V)
            return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_model_create: extra_vertex_ids[%d]=%d out of range", e, extra_vertex_ids[e]);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(K2B_ERR_NO_DEVICE, "k2b_model_create: no HIP device visible (this engine has no CPU path)");

    // released (device buffers included) on every early return below; handed to the caller at the end
    std::unique_ptr<k2b_model> owner(new k2b_model);
    k2b_model* m = owner.get();
    m->V = V; m->J = J; m->NB = NB; m->E = E; m->P = 9 * (J - 1);
    m->kin = k2b::Tree(J, parents);
    HIP_TRY(m->v_template.upload(v_template, (size_t)V * 3));
    HIP_TRY(m->shapedirs.upload(shapedirs, (size_t)V * 3 * NB));
    HIP_TRY(m->posedirs.upload(posedirs, (size_t)m->P * 3 * V));
    HIP_TRY(m->j_regressor.upload(j_regressor, (size_t)J * V));
    HIP_TRY(m->lbs_weights.upload(lbs_weights, (size_t)V * J));
    HIP_TRY(m->parents.upload(parents, (size_t)J));
    HIP_TRY(m->extra_ids.upload(extra_vertex_ids, (size_t)E));
    m->h_extra_ids.assign(extra_vertex_ids, extra_vertex_ids + E);
    if (const int rc = create_lbs_operands(m, v_template, shapedirs, posedirs, lbs_weights); rc != K2B_OK) return rc;
    if (const int rc = create_joint_basis(m); rc != K2B_OK) return rc;
    if (const int rc = create_fused_tables(m); rc != K2B_OK) return rc;
    if (const int rc = create_tree_tables(m); rc != K2B_OK) return rc;
    *out = owner.release();
    return K2B_OK;
}

// Development entry, outside include/k2b.h: the scan plan of a parent table (k2b_scan_plan.h) without a device, for the host
// tests.  lane_of[J], lane_flags[32] (kScan* bits; 0: hole).  Returns 1 for a valid plan, 0 where the tree gets the DFS
// placement and the fp64 scans (nothing is written), -1 for bad arguments.
int k2b_dev_fit_scan_plan(int32_t J, const int32_t* parents, int32_t* lane_of, int32_t* lane_flags) {
    if (J < 1 || J > k2b::kMaxJoints || !parents || !lane_of || !lane_flags || parents[0] >= 0) return -1;
    for (int j = 1; j < J; ++j)
        if (parents[j] < 0 || parents[j] >= j) return -1;
    const k2b::ScanPlan plan = k2b::fit_scan_plan(k2b::Tree(J, parents));
    if (!plan.valid) return 0;
    for (int j = 0; j < J; ++j) lane_of[j] = plan.lane_of[j];
    for (int l = 0; l < k2b::kScanLanes; ++l) lane_flags[l] = plan.flags[l];
    return 1;
}

// Development entries, outside include/k2b.h: the e4m3 operands of the SMPL stream kernel's pose phase (k2b_lbs_fp8.h) without a
// device, for the host tests.
// out[i] = e4m3fn code of x[i] / 2^exp (round to nearest even, saturating)
int k2b_dev_e4m3_encode(int64_t n, const float* x, int32_t exp, uint8_t* out) {
    if (n < 0 || !x || !out || exp < -60 || exp > 60) return -1;
    for (int64_t i = 0; i < n; ++i) out[i] = k2b::e4m3_encode_scaled(x[i], exp);
    return 0;
}
// the smallest power-of-two scale exponent at which max_abs does not saturate
int k2b_dev_e4m3_scale_exp(float max_abs) { return k2b::e4m3_scale_exp(max_abs); }
// X side: the f16 terms of x[i] (as floats) and their two codes, as the pose set-up stores them
int k2b_dev_lbs_x_fp8(int64_t n, const float* x, float* hi, float* lo, uint8_t* hi8, uint8_t* lo8) {
    if (n < 0 || !x || !hi || !lo || !hi8 || !lo8) return -1;
    for (int64_t i = 0; i < n; ++i) {
        const k2b::k2b_half h = (k2b::k2b_half)x[i], l = (k2b::k2b_half)(x[i] - (float)h);
        const k2b::XCodes q = k2b::x_fp8_codes(h, l);
        hi[i] = (float)h; lo[i] = (float)l; hi8[i] = q.hi8; lo8[i] = q.lo8;
    }
    return 0;
}
// The stream image Pd of the vertex set `ids` (n rows of a V-vertex model) as k2b_model_create would build it with or without
// K2B_LBS_POSE_F16.  info[4]: pose_fp8 of the route, 16-vertex tiles, the two scale exponents (lo, hi).  spd = NULL: only
// *spd_halfs and info are written.  Returns 0, -1 for bad arguments, -2 where the model is not on the route `stream`.
// given_exps != NULL: the two scales (lo, hi) of the model's mesh, as a subset of it takes them.
int k2b_dev_lbs_pose_fp8_image(int32_t J, int32_t NB, int32_t V, int32_t n, const int32_t* ids, const float* v_template, const float* shapedirs,
                               const float* posedirs, const float* lbs_weights, int32_t pose_f16, const int32_t* given_exps, uint16_t* spd,
                               int64_t* spd_halfs, int32_t* info) {
    if (J < 2 || NB < 1 || V < 1 || n < 1 || !ids || !v_template || !shapedirs || !posedirs || !lbs_weights || !spd_halfs || !info) return -1;
    for (int i = 0; i < n; ++i)
        if (ids[i] < 0 || ids[i] >= V) return -1;
    const k2b::LbsRouteRecord r = k2b::lbs_route(J, NB, true, false, pose_f16 != 0);
    if (r.route != k2b::LbsRoute::stream) return -2;
    const k2b::tables::VertexSetShape shape{J, NB, 9 * (J - 1), r.k_steps_x, r.w_frags, r.pose_fp8, given_exps != nullptr, given_exps ? given_exps[0] : 0,
                                            given_exps ? given_exps[1] : 0};
    const k2b::tables::VertexSetImages im = k2b::tables::vertex_set_images(shape, std::vector<int>(ids, ids + n), std::vector<int>(), v_template, shapedirs, posedirs, lbs_weights, V);
    info[0] = r.pose_fp8; info[1] = im.nv16; info[2] = im.pd8_lo_exp; info[3] = im.pd8_hi_exp;
    if (spd && *spd_halfs >= (int64_t)im.spd.size()) memcpy(spd, im.spd.data(), im.spd.size() * sizeof(uint16_t));
    else if (spd) return -1;
    *spd_halfs = (int64_t)im.spd.size();
    return 0;
}

// Development entry, outside include/k2b.h: the first `halfs` halfs of the model's X workspace (hi and lo pieces, frag_elem order
// with the padded frame count of the call that wrote them) as it stands after the last k2b_lbs call, for the GPU tests that hold
// the e4m3 form to its own operands.  Synchronises the device first.  Returns 0, -1 for a NULL argument or a size above the workspace.
int k2b_dev_lbs_read_x(const k2b_model* model_c, uint16_t* xh, uint16_t* xl, int64_t halfs) {
    k2b_model* m = const_cast<k2b_model*>(model_c);
    if (!m || !xh || !xl || halfs < 0) return -1;
    std::lock_guard<std::mutex> lk(m->mu);
    if ((uint64_t)halfs > (uint64_t)k2b::lbs_workspace(m->lbs, m->ws_bpad, 0).x_halfs) return -1;
    if (halfs == 0) return 0;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(xh, m->wsXh.get(), (size_t)halfs * sizeof(uint16_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(xl, m->wsXl.get(), (size_t)halfs * sizeof(uint16_t), hipMemcpyDeviceToHost));
    return 0;
}

void k2b_model_destroy(k2b_model* m) {
    if (!m) return;
    (void)hipDeviceSynchronize();
    delete m;
}

int k2b_debug_read_dump(const k2b_model* m, void* host, int64_t nbytes) {
    if (!m || !host || nbytes < 0 || nbytes > 64 * 1024) return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_debug_read_dump: bad arguments");
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(host, m->dump.get(), (size_t)nbytes, hipMemcpyDeviceToHost));
    return K2B_OK;
}

int k2b_model_dims(const k2b_model* m, int32_t* V, int32_t* J, int32_t* NB, int32_t* E) {
    if (!m) return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_model_dims: model is NULL");
    if (V) *V = m->V;
    if (J) *J = m->J;
    if (NB) *NB = m->NB;
    if (E) *E = m->E;
    return K2B_OK;
}

int k2b_model_set_landmarks(k2b_model* m, int32_t L, const int32_t* vertex_ids, const float* bary) {
    if (!m) return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_model_set_landmarks: model is NULL");
    if (m->lmk_set) return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_model_set_landmarks: the model already has a landmark table");
    if (L < 0 || L > k2b::kMaxLandmarks)
        return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_model_set_landmarks: num_landmarks=%d (0..%d)", L, k2b::kMaxLandmarks);
    if (L > 0 && (!vertex_ids || !bary)) return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_model_set_landmarks: NULL table");
    for (int i = 0; i < 3 * L; ++i) {
        if (vertex_ids[i] < 0 || vertex_ids[i] >= m->V)
            return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_model_set_landmarks: vertex_ids[%d][%d]=%d outside [0,%d)", i / 3, i % 3, vertex_ids[i], m->V);
        if (!std::isfinite(bary[i]))
            return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_model_set_landmarks: bary[%d][%d] is not finite", i / 3, i % 3);
    }
    for (int l = 0; l < L; ++l) {
        const double sum = (double)bary[3 * l] + bary[3 * l + 1] + bary[3 * l + 2];
        if (std::fabs(sum - 1.0) > 1e-3)
            return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_model_set_landmarks: the weights of landmark %d sum to %g, not 1 (barycentric)", l, sum);
    }
    std::lock_guard<std::mutex> lk(m->mu);
    if (L == 0) { m->lmk_set = true; return K2B_OK; }
    const int rc = set_landmarks_locked(m, L, vertex_ids, bary);
    if (rc != K2B_OK) {                                       // nothing of a failed call stays on the handle: it may be retried
        m->lmk = k2b_model::Landmarks{};
        return rc;
    }
    m->lmk_set = true;
    return K2B_OK;
}

int k2b_model_num_landmarks(const k2b_model* m, int32_t* L) {
    if (!m || !L) return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_model_num_landmarks: NULL argument");
    *L = m->lmk.L;
    return K2B_OK;
}

int k2b_model_joint_basis(const k2b_model* m, float* j_template, float* j_dirs) {
    if (!m) return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_model_joint_basis: model is NULL");
    if (j_template) memcpy(j_template, m->h_j_template.data(), m->h_j_template.size() * sizeof(float));
    if (j_dirs) memcpy(j_dirs, m->h_j_dirs.data(), m->h_j_dirs.size() * sizeof(float));
    return K2B_OK;
}

int k2b_model_reserve(k2b_model* m, int32_t max_frames) {
    if (!m) return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_model_reserve: model is NULL");
    if (max_frames < 0) return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_model_reserve: max_frames=%d", max_frames);
    std::lock_guard<std::mutex> lk(m->mu);
    return reserve_lbs_workspace(m, k2b::lbs_frames_padded(max_frames));
}

}  // extern "C"
