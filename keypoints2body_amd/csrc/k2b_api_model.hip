// k2b_api_model.hip — the model handle of the C ABI (include/k2b.h): constants and their kernel-side images, the tree
// tables of the two fit kernels, landmarks, and the per-model tables and workspaces that calls build on first use.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "k2b_host.h"
#include "k2b_scan_plan.h"

#ifndef K2B_LBS_STREAM
#define K2B_LBS_STREAM 1      // 0: development builds that keep the tile kernel for 17-24 joint models (A/B timing)
#endif

using namespace k2b::host;

namespace {
// LBS B operands of a vertex set (f16 hi/lo, MFMA fragment order; k2b_lbs.hip, k2b_lbs_stream.hip) from HOST constants in which
// vertex v's rows are those of `ids` (posedirs row stride 3 * V).  tag[i] = 1 + e when vertex i of the set is the vertex of
// output joint J + e (mesh set only), else 0.
int build_vertex_set(k2b_model* m, VertexSet& vs, const std::vector<int>& ids, const std::vector<int>& tag,
                     const float* v_template, const float* shapedirs, const float* posedirs, const float* lbs_weights, int V) {
    const int KX = m->k_steps_x, P = m->P, NB = m->NB, J = m->J;
    const int n = (int)ids.size();
    vs.num = n;
    vs.v_tiles = (n + 31) / 32;
    const int vp = vs.v_tiles * 32;
    std::vector<k2b::k2b_half> pdh((size_t)KX * 3 * vp * 16, (k2b::k2b_half)0.f), pdl(pdh.size(), (k2b::k2b_half)0.f);
    for (int i = 0; i < n; ++i) {
        const int v = ids[i];
        for (int c = 0; c < 3; ++c) {
            auto put = [&](int k, k2b::k2b_half hi, k2b::k2b_half lo) {
                const size_t o = k2b::frag_elem(((size_t)(k >> 4) * 3 + c) * vs.v_tiles + (i >> 5), k, i);
                pdh[o] = hi;
                pdl[o] = lo;
            };
            auto split = [&](int k, float x) -> float {   // returns what two f16 terms leave over
                const float xs = x * k2b::kPdScale;
                const k2b::k2b_half hi = (k2b::k2b_half)xs;
                const k2b::k2b_half lo = (k2b::k2b_half)(xs - (float)hi);
                put(k, hi, lo);
                return xs - (float)hi - (float)lo;
            };
            for (int k = 0; k < P; ++k) split(k, posedirs[(size_t)k * 3 * V + 3 * v + c]);
            for (int k = 0; k < NB; ++k) split(P + k, shapedirs[((size_t)v * 3 + c) * NB + k]);
            const float rest = split(P + NB, v_template[(size_t)v * 3 + c]);
            // the template is metre-scale: keep its third term as an extra K row (feature = 1)
            const k2b::k2b_half rh = (k2b::k2b_half)rest;
            put(P + NB + 1, rh, (k2b::k2b_half)(rest - (float)rh));
        }
    }
    // tile-kernel layout of W: [16-vertex tile][hi groups | lo groups | ONES | ZERO][16 rows][8 joints]
    const int GA = k2b::tile_groups_a(J), NGP = k2b::tile_ngp(GA), v16 = vs.v_tiles * 2;
    std::vector<k2b::k2b_half> w2((size_t)v16 * NGP * 128, (k2b::k2b_half)0.f);
    for (int t = 0; t < v16; ++t)
        for (int r = 0; r < 16; ++r) {
            const int i = t * 16 + r;
            k2b::k2b_half* rowp = w2.data() + ((size_t)t * NGP * 16 + r) * 8;
            if (i < n)
                for (int j = 0; j < J; ++j) {
                    const float w = lbs_weights[(size_t)ids[i] * J + j];
                    const k2b::k2b_half hi = (k2b::k2b_half)w;
                    rowp[(size_t)(j >> 3) * 128 + (j & 7)] = hi;
                    rowp[(size_t)(GA + (j >> 3)) * 128 + (j & 7)] = (k2b::k2b_half)(w - (float)hi);
                }
            for (int k = 0; k < 3; ++k) rowp[(size_t)(2 * GA) * 128 + k] = (k2b::k2b_half)1.f;   // ONES: picks up the PAD terms
            if (i < n && !tag.empty() && tag[i]) rowp[(size_t)(2 * GA + 1) * 128] = (k2b::k2b_half)(float)tag[i];   // ZERO group: joint tag
        }
    hipError_t e;
    if (m->streams()) {
        // stream kernels: Pd [k-step][16-vertex tile][coord][hi | lo] and W [16-vertex tile][3 or 5 fragments], 1 KiB pieces in
        // MFMA operand order (lane = row + 16 k-group, 8 halfs); vertex tiles padded to whole 128-vertex groups
        const int nv16 = (n + 127) / 128 * 8, SK = KX / 2, NWF = m->stream ? 3 : 5;
        vs.nv16 = nv16;
        std::vector<k2b::k2b_half> spd((size_t)SK * nv16 * 6 * 512, (k2b::k2b_half)0.f), sw((size_t)nv16 * NWF * 512, (k2b::k2b_half)0.f);
        for (int i = 0; i < n; ++i) {
            const int v16 = i >> 4, r = i & 15;
            for (int c = 0; c < 3; ++c)
                for (int k = 0; k < KX * 16; ++k) {      // the split values already sit in pdh / pdl: same k, same scale
                    const size_t src = k2b::frag_elem(((size_t)(k >> 4) * 3 + c) * vs.v_tiles + (i >> 5), k, i);
                    const size_t dst = ((((size_t)(k >> 5) * nv16 + v16) * 3 + c) * 2) * 512 + (size_t)((((k >> 3) & 3) * 16 + r) * 8 + (k & 7));
                    spd[dst] = pdh[src];
                    spd[dst + 512] = pdl[src];
                }
            k2b::k2b_half* wt = sw.data() + (size_t)v16 * NWF * 512;
            auto at = [&](int frag, int group, int k) -> k2b::k2b_half& { return wt[(size_t)frag * 512 + (size_t)((group * 16 + r) * 8 + k)]; };
            for (int j = 0; j < J; ++j) {
                const float w = lbs_weights[(size_t)ids[i] * J + j];
                const k2b::k2b_half hi = (k2b::k2b_half)w, lo = (k2b::k2b_half)(w - (float)hi);
                const int gj = j >> 3, kj = j & 7;
                if (m->stream) { at(0, gj, kj) = hi; at(1, gj, kj) = hi; at(2, gj, kj) = lo; }
                else if (gj < 4) { at(0, gj, kj) = hi; at(2, gj, kj) = lo; }
                else { at(1, gj - 4, kj) = hi; at(4, gj - 4, kj) = hi; at(3, gj - 4, kj) = lo; }
            }
            // last group of the fragment that meets the PAD group of A: ONES; of the one that meets ZERO: the joint tag
            for (int k = 0; k < 3; ++k) at(m->stream ? 0 : 1, 3, k) = (k2b::k2b_half)1.f;
            if (!tag.empty() && tag[i]) at(m->stream ? 1 : 4, 3, 0) = (k2b::k2b_half)(float)tag[i];
        }
        if ((e = vs.spd.upload(spd.data(), spd.size())) != hipSuccess) return (int)e;
        if ((e = vs.sw.upload(sw.data(), sw.size())) != hipSuccess) return (int)e;
    }
    if (m->streams()) return 0;                      // the tile kernel's images stay on the host (SMPL-X: 64 MB less per GPU)
    if ((e = vs.w2.upload(w2.data(), w2.size())) != hipSuccess) return (int)e;
    if ((e = vs.pdh.upload(pdh.data(), pdh.size())) != hipSuccess) return (int)e;
    if ((e = vs.pdl.upload(pdl.data(), pdl.size())) != hipSuccess) return (int)e;
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
    std::vector<int> ids, pair_u(3 * T, 0);
    std::vector<float> pair_w(3 * T, 0.f);
    std::map<int, int> slot;
    for (int t = 0; t < T; ++t) {
        const int j = sel[t];
        for (int k = 0; k < 3; ++k) {
            int v;
            float w;
            if (j < J + E) {
                if (k > 0) break;
                v = m->h_extra_ids[j - J]; w = 1.f;
            } else {
                v = m->lmk.h_ids[(j - J - E) * 3 + k]; w = m->lmk.h_w[(j - J - E) * 3 + k];
            }
            auto ins = slot.emplace(v, (int)ids.size());
            if (ins.second) ids.push_back(v);
            pair_u[t * 3 + k] = ins.first->second;
            pair_w[t * 3 + k] = w;
        }
    }
    const int U = (int)ids.size();
    std::vector<int> inv_off(U + 1, 0), inv_t;
    std::vector<float> inv_w;
    {
        std::vector<std::vector<std::pair<int, float>>> lists(U);
        for (int t = 0; t < T; ++t)
            for (int k = 0; k < 3; ++k)
                if (pair_w[t * 3 + k] != 0.f) lists[pair_u[t * 3 + k]].push_back({t, pair_w[t * 3 + k]});
        for (int u = 0; u < U; ++u) {
            for (const auto& p : lists[u]) { inv_t.push_back(p.first); inv_w.push_back(p.second); }
            inv_off[u + 1] = (int)inv_t.size();
        }
    }
    const int n = (int)inv_t.size();
    // one allocation: floats (vt, sd, pd, lw, pair_w, inv_w), then ints (pair_u, sel_k, inv_off, inv_t, ids)
    const size_t n_tab = (size_t)U * 3 + (size_t)U * 3 * NB + (size_t)PF * 3 * U + (size_t)U * J;
    const size_t n_f = n_tab + 3 * (size_t)T + (size_t)n;
    const size_t n_i = 3 * (size_t)T + T + (U + 1) + (size_t)n + U;
    std::vector<float> hf(3 * (size_t)T + n);
    std::copy(pair_w.begin(), pair_w.end(), hf.begin());
    std::copy(inv_w.begin(), inv_w.end(), hf.begin() + 3 * T);
    std::vector<int> hi;
    hi.insert(hi.end(), pair_u.begin(), pair_u.end());
    hi.insert(hi.end(), col.begin(), col.end());
    hi.insert(hi.end(), inv_off.begin(), inv_off.end());
    hi.insert(hi.end(), inv_t.begin(), inv_t.end());
    hi.insert(hi.end(), ids.begin(), ids.end());
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
    if (m->lmk.L > 0 && bpad > m->lmk.ws_bpad) {             // the landmark vertices of joints-only calls
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(m->lmk.ws.reset());
        m->lmk.ws_bpad = 0;
        HIP_TRY(m->lmk.ws.alloc((size_t)bpad * 3 * m->lmk.L * 3));
        m->lmk.ws_bpad = bpad;
    }
    if (bpad <= m->ws_bpad) return K2B_OK;
    HIP_TRY(hipDeviceSynchronize());
    for (auto* w : {&m->wsXh, &m->wsXl, &m->wsA2}) HIP_TRY(w->reset());
    m->ws_bpad = 0;
    const size_t nx = (size_t)m->k_steps_x * bpad * 16;
    const size_t na2 = (size_t)(bpad / 16) * 12 * k2b::tile_ngp(m->groups_a) * 128;
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
    HIP_TRY(m->v_template.upload(v_template, (size_t)V * 3));
    HIP_TRY(m->shapedirs.upload(shapedirs, (size_t)V * 3 * NB));
    HIP_TRY(m->posedirs.upload(posedirs, (size_t)m->P * 3 * V));
    HIP_TRY(m->j_regressor.upload(j_regressor, (size_t)J * V));
    HIP_TRY(m->lbs_weights.upload(lbs_weights, (size_t)V * J));
    HIP_TRY(m->parents.upload(parents, (size_t)J));
    HIP_TRY(m->extra_ids.upload(extra_vertex_ids, (size_t)E));
    m->h_extra_ids.assign(extra_vertex_ids, extra_vertex_ids + E);

    // LBS operands: B side of the two GEMMs, f16 hi/lo in fragment order (k2b_lbs.hip)
    {
        const int P = m->P;
        int KX = ((P + NB + 2 + 31) / 32) * 2;         // even: the kernels stage 32-deep slices
        m->groups_a = k2b::tile_groups_a(J);
        // 49-56 joints with fewer features than SMPL-X (SMPL-H: 477 -> 15 k-steps): one all-zero k-step more buys the stream kernel
        if (K2B_LBS_STREAM && m->groups_a == 7 && KX < 2 * k2b::kStreamXKSteps) KX = 2 * k2b::kStreamXKSteps;
        m->k_steps_x = KX;
        // development switch K2B_LBS_TILE (non-zero): this model is skinned by the tile kernel whatever the stream kernels would
        // take - their run-time twin.  Per model, fixed here; nothing else reads it.
        const char* tile_env = getenv("K2B_LBS_TILE");
        const bool streams = K2B_LBS_STREAM && !(tile_env && atoi(tile_env) != 0);
        m->stream = streams && m->groups_a == 3 && KX == 2 * k2b::kStreamKSteps;
        m->stream_x = streams && m->groups_a == 7 && KX == 2 * k2b::kStreamXKSteps;
        m->stream_xw = streams && m->groups_a == 7 && KX == 2 * k2b::kStreamXWKSteps;      // 513-544 features: 55 joints from 25 shape coefficients on, 56 from 16
        HIP_TRY(m->dump.alloc(64 * 1024 / sizeof(float)));     // 64 x 3 floats used; the rest is room for diagnostic builds
        std::vector<int> all(V), ex(extra_vertex_ids, extra_vertex_ids + E), tag(V, 0);
        for (int v = 0; v < V; ++v) all[v] = v;
        // an output joint rides in the W image of its vertex (k2b_lbs.hip) - unless two joints share a vertex or the index
        // does not fit an f16 integer, in which case the gather launch stays
        m->joints_in_mesh = E > 0 && E <= 1024;
        for (int e = 0; e < E && m->joints_in_mesh; ++e) {
            if (tag[extra_vertex_ids[e]]) m->joints_in_mesh = false;
            tag[extra_vertex_ids[e]] = e + 1;
        }
        if (!m->joints_in_mesh) std::fill(tag.begin(), tag.end(), 0);
        if (build_vertex_set(m, m->mesh, all, tag, v_template, shapedirs, posedirs, lbs_weights, V) != 0 ||
            (E > 0 && build_vertex_set(m, m->extra, ex, std::vector<int>(), v_template, shapedirs, posedirs, lbs_weights, V) != 0))
            return fail(K2B_ERR_HIP, "k2b_model_create: uploading LBS operands failed");
    }

    // J x V contraction on the matrix cores
    {
        const int splits = 32;
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
    }

    // tables of the fused fit kernel, by lane (the placement is chosen below)
    bool ok = (J == k2b::kFitJoints) && NB <= k2b::kMaxBetas;
    if (!ok) m->fit_why = "the 24-lane fused fit kernel is built for the 24-joint SMPL tree with <= 16 betas";
    std::vector<std::vector<int>> children(J);
    std::vector<int> depth(J, 0);
    int maxd = 0;
    for (int j = 1; j < J; ++j) {
        children[parents[j]].push_back(j);
        depth[j] = depth[parents[j]] + 1;
        maxd = depth[j] > maxd ? depth[j] : maxd;
    }
    std::vector<int> order, lane_of(J, -1), size(J, 1);
    {
        std::vector<int> stack{0};
        while (!stack.empty()) {
            const int j = stack.back();
            stack.pop_back();
            lane_of[j] = (int)order.size();
            order.push_back(j);
            for (auto it = children[j].rbegin(); it != children[j].rend(); ++it) stack.push_back(*it);
        }
        for (int j = J - 1; j >= 1; --j) size[parents[j]] += size[j];
    }
    int rounds = 0;
    while ((1 << rounds) < maxd + 1) ++rounds;
    if (ok && (rounds > k2b::kMaxRounds || J > 32)) { ok = false; m->fit_why = "tree too deep / large for the fused fit kernel"; }
    m->depth = depth;
    // Lane placement of the fused kernel.  With a scan plan (k2b_scan_plan.h): reversed DFS order with holes, the subtree sums are
    // fp32 chain / end scans.  Without one (a junction inside a limb, a chain of more than 8 joints, ...): DFS order, where every
    // subtree is the lane range that starts at its joint, and the fp64 prefix differences.
    // Development switch K2B_FIT_SCAN64 (non-zero): this model gets the DFS placement and the fp64 scans whatever its tree allows -
    // the run-time twin of the fp32 form.  Per model, fixed here; nothing else reads it.
    const char* scan_env = getenv("K2B_FIT_SCAN64");
    k2b::ScanPlan plan;
    if (ok && !(scan_env && atoi(scan_env) != 0)) plan = k2b::fit_scan_plan(J, parents);
    m->fit_scan64 = !plan.valid;
    std::vector<int> f_lane_of = lane_of, f_joint_at(k2b::kScanLanes, -1);
    if (plan.valid) {
        f_lane_of = plan.lane_of;
        f_joint_at.assign(plan.joint_at, plan.joint_at + k2b::kScanLanes);
    } else if (ok) {
        for (int l = 0; l < J; ++l) f_joint_at[l] = order[l];
    }
    std::vector<int> tab((size_t)64 * k2b::kLaneTabStride, -1);
    for (int l = 0; l < 64; ++l) tab[(size_t)l * k2b::kLaneTabStride + k2b::kLaneTabScan] = 0;
    std::vector<float> dt((size_t)64 * 3, 0.f), dd((size_t)64 * 3 * k2b::kMaxBetas, 0.f);
    if (ok) {
        for (int l = 0; l < k2b::kScanLanes; ++l) {
            const int j = f_joint_at[l];
            if (j < 0) continue;                     // a hole or a lane beyond the tree: no joint, zero offset, identity transform
            const int p = parents[j];
            int* t = tab.data() + (size_t)l * k2b::kLaneTabStride;
            t[0] = j;
            t[1] = p >= 0 ? f_lane_of[p] : -1;
            // ancestor lane 2^r levels up (pointer doubling), -1 once past the root
            int anc = t[1];
            for (int r = 0; r < k2b::kMaxRounds; ++r) {
                t[2 + r] = anc;
                for (int s = 0; s < (1 << r) && anc >= 0; ++s) {   // advance 2^r more levels
                    const int aj = f_joint_at[anc];
                    anc = parents[aj] >= 0 ? f_lane_of[parents[aj]] : -1;
                }
            }
            t[2 + k2b::kMaxRounds] = size[j];        // DFS placement: subtree = lanes [l, l + size)
            t[3 + k2b::kMaxRounds] = depth[j];
            t[k2b::kLaneTabScan] = plan.valid ? plan.flags[l] : 0;
            for (int c = 0; c < 3; ++c) {
                dt[l * 3 + c] = m->h_j_template[j * 3 + c] - (p >= 0 ? m->h_j_template[p * 3 + c] : 0.f);
                for (int k = 0; k < NB; ++k)
                    dd[(l * 3 + c) * k2b::kMaxBetas + k] =
                        m->h_j_dirs[(j * 3 + c) * NB + k] - (p >= 0 ? m->h_j_dirs[(p * 3 + c) * NB + k] : 0.f);
            }
        }
    }
    HIP_TRY(m->dt.upload(dt.data(), dt.size()));
    HIP_TRY(m->dd.upload(dd.data(), dd.size()));
    HIP_TRY(m->tree.upload(tab.data(), tab.size()));
    m->fit_ok = ok;
    {   // tree fit kernel: [64][8] lane table (prior columns filled per call), rest offsets and their shape directions
        std::vector<int> tt((size_t)64 * 8, -1);
        std::vector<float> tdt((size_t)64 * 3, 0.f), tdd((size_t)64 * 3 * k2b::kMaxShape, 0.f);
        for (int l = 0; l < 64; ++l) { tt[l * 8 + 1] = 0; tt[l * 8 + 2] = 1; tt[l * 8 + 3] = 1000; }
        for (int l = 0; l < J; ++l) {
            const int j = order[l], p = parents[j];
            tt[l * 8 + 0] = j; tt[l * 8 + 1] = p >= 0 ? lane_of[p] : 0; tt[l * 8 + 2] = size[j]; tt[l * 8 + 3] = depth[j];
            for (int c = 0; c < 3; ++c) {
                tdt[l * 3 + c] = m->h_j_template[j * 3 + c] - (p >= 0 ? m->h_j_template[p * 3 + c] : 0.f);
                for (int k = 0; k < NB; ++k)
                    tdd[(l * 3 + c) * k2b::kMaxShape + k] =
                        m->h_j_dirs[(j * 3 + c) * NB + k] - (p >= 0 ? m->h_j_dirs[(p * 3 + c) * NB + k] : 0.f);
            }
        }
        // ancestors 1, 2, 4, 8 levels up (pointer doubling); 63 = "none": a lane that is no joint and holds the identity
        std::vector<int> tanc((size_t)64 * 4, 63);
        if (J <= 63)
            for (int l = 0; l < J; ++l) {
                int aj = order[l];
                for (int r = 0, dist = 0; r < 4; ++r) {
                    for (; dist < (1 << r) && aj >= 0; ++dist) aj = parents[aj];
                    tanc[l * 4 + r] = aj >= 0 ? lane_of[aj] : 63;
                }
            }
        m->tt_lane_of = lane_of;
        HIP_TRY(m->tt_anc.upload(tanc.data(), tanc.size()));
        HIP_TRY(m->tt_dt.upload(tdt.data(), tdt.size()));
        HIP_TRY(m->tt_dd.upload(tdd.data(), tdd.size()));
        HIP_TRY(m->tt_tab.upload(tt.data(), tt.size()));
    }
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
    const k2b::ScanPlan plan = k2b::fit_scan_plan(J, parents);
    if (!plan.valid) return 0;
    for (int j = 0; j < J; ++j) lane_of[j] = plan.lane_of[j];
    for (int l = 0; l < k2b::kScanLanes; ++l) lane_flags[l] = plan.flags[l];
    return 1;
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
