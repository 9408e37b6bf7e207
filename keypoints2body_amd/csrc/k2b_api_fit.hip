// k2b_api_fit.hip — the fit calls of the C ABI (include/k2b.h): one description of a call (FitCall, k2b_host.h), one set-up
// path for the two fit kernels (the fused 24-lane kernel, k2b_fit.hip; the tree kernel, k2b_fit_tree.hip), the Adam path with
// surface targets, and the Adam entries for frames, sequences and ragged sequences.  What an entry refuses is k2b_fit_rules.h:
// every entry asks it once, first; nothing here forms an argument refusal of its own.
#include <algorithm>
#include <cstring>
#include <type_traits>

#include "k2b_host.h"

using namespace k2b::host;

namespace {

// ---- set-up shared by the two fit kernels ----------------------------------------------------------------------------------
// (What a call is refused for is k2b_fit_rules.h, asked by the entries: nothing below checks an argument again.)
// The targets of a call by kind: kinematic joints (model index < J) are fitted by a lane of the fit kernel, surface targets
// (extra joints, landmarks) by k2b_vertex_term_kernel / k2b_surface_term_kernel.
struct Targets {
    int lane_target[64];                     // target column fitted by lane l, or -1
    std::vector<int> vsel, vcol;             // surface targets: model index, target column
    int max_depth = 0;                       // (depth of the deepest targeted joint)
};
// lane_of: the lane of every joint (tree kernel), or null where lane = joint (24-lane kernel)
Targets classify_targets(const k2b_model* model, const FitCall& c, const int* lane_of) {
    Targets t;
    for (int& l : t.lane_target) l = -1;
    for (int k = 0; k < c.K; ++k) {
        const int j = c.model_joint_index[k];
        if (j >= model->J) {
            t.vsel.push_back(j);
            t.vcol.push_back(k);
            continue;
        }
        t.lane_target[lane_of ? lane_of[j] : j] = k;
        t.max_depth = std::max(t.max_depth, model->kin.depth[j]);
    }
    return t;
}
// a chain's follow-up frames restart the optimiser: one table long enough for both counts, each reads its prefix
int chain_adam_table(k2b_model* model, const k2b_fit_config* cfg, const FitCall& c, float2** coef) {
    k2b_fit_config tc = *cfg;
    if (c.chain.len > 1 && c.chain.iters > tc.num_iters) tc.num_iters = c.chain.iters;
    return adam_table(model, &tc, c.stream, coef);
}
// the fields that FitArgs and FitTreeArgs name alike
template <class Args>
void fill_call_fields(Args& a, const k2b_fit_config* cfg, const FitCall& c, const float2* coef) {
    a.num_frames = c.B; a.num_targets = c.K;
    a.j3d = c.j3d; a.conf = c.conf; a.conf_per_frame = cfg->conf_per_frame ? 1 : 0;
    a.go_in = c.in.go; a.bp_in = c.in.bp; a.be_in = c.in.be; a.tr_in = c.in.tr; a.preserve = c.preserve;
    a.go_out = c.out.go; a.bp_out = c.out.bp; a.be_out = c.out.be; a.tr_out = c.out.tr;
    a.loss_out = c.loss_out; a.grad_out = c.grad_out;
    a.adam_coef = coef; a.num_iters = cfg->num_iters;
    // 1 - beta is formed in double (Python float) and only then rounded to the tensor dtype
    a.one_minus_beta1 = (float)(1.0 - cfg->adam_beta1);
    a.beta2 = (float)cfg->adam_beta2; a.one_minus_beta2 = (float)(1.0 - cfg->adam_beta2);
    a.eps = (float)cfg->adam_eps;
    a.sigma = cfg->sigma; a.joint_w = cfg->joint_loss_weight; a.pose_prior_w = cfg->pose_prior_weight;
    a.angle_w = cfg->angle_prior_weight; a.shape_w = cfg->shape_prior_weight; a.preserve_w = cfg->pose_preserve_weight;
    a.freeze_betas = cfg->freeze_betas ? 1 : 0;
    a.chain_len = c.chain.len > 1 ? c.chain.len : 1;
    a.chain_iters = c.chain.iters;
    a.chain_meta = c.chain.len > 1 ? c.chain.meta : nullptr;
    a.projection = cfg->projection; a.focal_x = cfg->focal[0]; a.focal_y = cfg->focal[1];
    a.chain_freeze_shape = c.chain.len > 1 && c.chain.freeze_shape ? 1 : 0;
    a.num_views = c.num_views;
    for (int v = 0; v < c.num_views; ++v) {
        const k2b_camera& cam = c.cameras[v];
        k2b::FitView& w = a.view[v];
        memcpy(w.r, cam.rotation, sizeof w.r);
        memcpy(w.t, cam.translation, sizeof w.t);
        w.fx = cam.focal[0]; w.fy = cam.focal[1];
    }
}

// ---- surface targets: the Adam loop as pairs of launches ---------------------------------------------------------------------
// Targets with model index >= J go to the vertex-term kernel when they are at most 32 extra joints (the path of the first
// release, bit for bit), to the surface-point kernel otherwise (landmarks among them, or more than 32).  Under projection every
// selection takes the surface-point kernel: the vertex-term kernel is 3D only.
bool needs_surface_kernel(const k2b_model* m, const k2b_fit_config* cfg, const std::vector<int>& sel) {
    if (cfg->projection != 0 || sel.size() > 32) return true;
    for (int j : sel)
        if (j >= m->J + m->E) return true;
    return false;
}

// Adam fit with vertex-selected joints among the targets (world_space.py:198-201 with indices >= J).  The fused kernel
// fits kinematic joints only, so every iteration is two launches queued back to back: the fused kernel in evaluate-only
// mode (kinematic targets + every prior -> loss, gradient) and the vertex-term kernel with its Adam tail (vertex targets,
// sum of the gradients, the optimiser step in place).  `a` is the fused launch fully set up for the caller's buffers.
template <class Args, class Launch>
int fit_world_vertex_joints(k2b_model* model, const k2b_fit_config* cfg, Args a, const float* tr_prior_src, int frozen_shape,
                            const Targets& targets, hipStream_t stream, Launch launch_eval) {
    const std::vector<int>& ssel = targets.vsel;
    const std::vector<int>& vcol = targets.vcol;
    const int B = a.num_frames, NB = model->NB, D = 3 * (model->J - 1), P = 3 + D + NB + 3;
    const bool surface = needs_surface_kernel(model, cfg, ssel);
    k2b::SurfaceTermArgs s{};
    if (surface)
        if (const int rc = surface_table(model, ssel, vcol, stream, &s); rc != K2B_OK) return rc;
    const int iters = cfg->num_iters;
    float2 *coef = nullptr, *coef_eval = nullptr;
    if (const int rc = adam_table(model, cfg, stream, &coef); rc != K2B_OK) return rc;
    {
        k2b_fit_config ec = *cfg;
        ec.num_iters = 1;
        ec.step_size = 0.0;
        if (const int rc = adam_table(model, &ec, stream, &coef_eval); rc != K2B_OK) return rc;
    }
    // stream-ordered scratch: gradient and loss of the evaluate launch, Adam state, copies of the preserve pose and the
    // translation prior's centre (their defaults are the INITIAL parameters, which the in-place steps overwrite)
    const k2b::VertexJointsMap m = k2b::vertex_joints_map(B, P, D);
    StreamWorkspace scratch(stream);
    HIP_TRY(scratch.alloc(m.total));
    auto f = [&](size_t off) { return reinterpret_cast<float*>(scratch.get() + off); };
    float *gbuf = f(m.grad), *mbuf = f(m.adam_m), *vbuf = f(m.adam_v), *lbuf = f(m.loss), *pres = f(m.preserve), *trp = f(m.tr_prior);
#define TRY_VJ(expr) HIP_TRY_MSG(expr, "k2b_fit_world: HIP call failed in the vertex-joint path")
    TRY_VJ(hipMemsetAsync(mbuf, 0, m.moments_bytes, stream));
    TRY_VJ(start_in_place(B, D, NB, {a.go_in, a.bp_in, a.be_in, a.tr_in}, {a.go_out, a.bp_out, a.be_out, a.tr_out}, a.preserve, tr_prior_src,
                          pres, trp, stream));
    float* user_grad = a.grad_out;
    float* user_loss = a.loss_out;
    a.go_in = a.go_out; a.bp_in = a.bp_out; a.be_in = a.be_out; a.tr_in = a.tr_out;
    a.preserve = pres;
    if constexpr (std::is_same<Args, k2b::FitArgs>::value) a.tr_prior = trp;
    a.adam_coef = coef_eval; a.num_iters = 1;
    a.loss_out = lbuf; a.grad_out = gbuf;

    k2b::VertexTermArgs v{};
    v.v_template = model->v_template.get(); v.shapedirs = model->shapedirs.get(); v.posedirs = model->posedirs.get();
    v.lbs_weights = model->lbs_weights.get(); v.j_template = model->j_template.get(); v.j_dirs = model->j_dirs.get();
    v.parents = model->parents.get(); v.extra_ids = model->extra_ids.get();
    v.num_vertices = model->V; v.num_betas = NB; v.num_joints = model->J;
    v.frozen_shape = frozen_shape;
    v.num_frames = B; v.num_sel = surface ? 0 : (int)ssel.size();
    for (int e = 0; e < v.num_sel; ++e) { v.sel[e] = ssel[e] - model->J; v.sel_k[e] = vcol[e]; }
    v.num_targets = a.num_targets; v.targets = a.j3d; v.conf = a.conf; v.conf_per_frame = a.conf_per_frame;
    v.sigma = a.sigma; v.joint_w = a.joint_w;
    v.go = a.go_out; v.bp = a.bp_out; v.be = a.be_out; v.tr = a.tr_out;
    v.go_w = a.go_out; v.bp_w = a.bp_out; v.be_w = a.be_out; v.tr_w = a.tr_out;
    float* loss_sink = user_loss ? user_loss : lbuf;
    v.loss_in = lbuf; v.grad_in = gbuf;
    v.adam_m = mbuf; v.adam_v = vbuf;
    v.one_minus_beta1 = a.one_minus_beta1; v.beta2 = a.beta2; v.one_minus_beta2 = a.one_minus_beta2; v.eps = a.eps;
    v.opt_mask = a.opt_mask;
    // the surface kernel: the same call fields
    s.num_frames = B; s.num_targets = v.num_targets; s.targets = v.targets; s.conf = v.conf; s.conf_per_frame = v.conf_per_frame;
    s.sigma = v.sigma; s.joint_w = v.joint_w;
    s.go = v.go; s.bp = v.bp; s.be = v.be; s.tr = v.tr;
    s.go_w = v.go_w; s.bp_w = v.bp_w; s.be_w = v.be_w; s.tr_w = v.tr_w;
    s.loss_in = v.loss_in; s.grad_in = v.grad_in; s.adam_m = v.adam_m; s.adam_v = v.adam_v;
    s.one_minus_beta1 = v.one_minus_beta1; s.beta2 = v.beta2; s.one_minus_beta2 = v.one_minus_beta2; s.eps = v.eps;
    s.opt_mask = v.opt_mask; s.frozen_shape = v.frozen_shape;
    s.projection = a.projection; s.focal_x = a.focal_x; s.focal_y = a.focal_y;
    for (int it = 0; it < iters; ++it) {
        TRY_VJ(launch_eval(a));
        v.adam_coef = coef + it;
        const bool last = it == iters - 1;
        v.loss_out = last ? loss_sink : lbuf;        // (lbuf: read and written by the same lane)
        v.grad_out = last ? user_grad : nullptr;
        if (surface) {
            s.adam_coef = v.adam_coef; s.loss_out = v.loss_out; s.grad_out = v.grad_out;
            TRY_VJ(k2b::launch_surface_term(s, stream));
        } else {
            TRY_VJ(k2b::launch_vertex_term(v, stream));
        }
    }
#undef TRY_VJ
    return K2B_OK;
}

// ---- the two kernels -------------------------------------------------------------------------------------------------------
// large trees (SMPL-H / SMPL-X), or a prior over a prefix of the body pose: k2b_fit_tree.hip
int fit_tree(k2b_model* model, k2b_prior* prior, const k2b_fit_config* cfg, int prior_dims, const FitCall& c) {
    const int J = model->J, NB = model->NB;
    k2b::FitTreeArgs a{};
    const Targets t = classify_targets(model, c, model->kin.pos.data());
    memcpy(a.lane_target, t.lane_target, sizeof a.lane_target);
    for (int i = 0; i < 4; ++i) {
        a.angle_index[i] = cfg->angle_prior_index[i];
        a.angle_sign[i] = cfg->angle_prior_sign[i];
    }
    const k2b_prior::Folded* f = nullptr;
    if (const int rc = folded_prior(prior, prior_dims, &f); rc != K2B_OK) return rc;
    float2* coef = nullptr;
    if (const int rc = chain_adam_table(model, cfg, c, &coef); rc != K2B_OK) return rc;
    if (const int rc = tree_lane_table(model, prior_dims, &a.tab); rc != K2B_OK) return rc;
    a.dt = model->tt_dt.get(); a.dd = model->tt_dd.get(); a.anc = model->tt_anc.get();
    a.num_joints = J; a.num_shape = NB;
    a.num_rounds = k2b::rounds_for_depth(t.max_depth);      // global transforms are only needed down to the deepest targeted joint
    a.pfrag = prior->frag32.get(); a.ph = f->ph.get(); a.pb = f->pb.get(); a.pmu = f->pmu.get(); a.pcl = f->pcl.get();
    for (int m = 0; m < k2b::kPriorMaxGauss; ++m) a.inv_scale[m] = prior->inv_scale[m];
    a.num_gauss = prior->M; a.prior_dims = prior_dims;
    fill_call_fields(a, cfg, c, coef);
    a.num_betas_prior = cfg->num_betas_prior > 0 ? (cfg->num_betas_prior < NB ? cfg->num_betas_prior : NB) : NB;
    a.opt_mask = cfg->optimize_mask & 15;
    a.debug_shape = cfg->debug_launch_shape <= k2b::TreeShape::comp_waves ? cfg->debug_launch_shape : k2b::TreeShape::automatic;
    const int cus = device_cus();
    if (!t.vsel.empty())
        return fit_world_vertex_joints(model, cfg, a, nullptr, cfg->freeze_betas ? a.num_betas_prior : 0, t, c.stream,
                                       [&](const k2b::FitTreeArgs& e) { return k2b::launch_fit_tree(e, cus, c.stream); });
    HIP_TRY(k2b::launch_fit_tree(a, cus, c.stream));
    return K2B_OK;
}

// the 24-joint SMPL tree with the prior over the whole pose: k2b_fit.hip
int fit_fused(k2b_model* model, const k2b_prior* prior, const k2b_fit_config* cfg, const FitCall& c) {
    k2b::FitArgs a{};
    const Targets t = classify_targets(model, c, nullptr);
    for (int i = 0; i < 4; ++i) {
        a.angle_index[i] = cfg->angle_prior_index[i];
        a.angle_sign[i] = cfg->angle_prior_sign[i];
    }
    float2* coef = nullptr;
    if (const int rc = chain_adam_table(model, cfg, c, &coef); rc != K2B_OK) return rc;

    a.dt = model->dt.get(); a.dd = model->dd.get(); a.lane_tab = model->tree.get();
    a.scan64 = model->fit_scan64 ? 1 : 0;
    a.num_rounds = k2b::rounds_for_depth(t.max_depth);
    a.num_betas = model->NB;
    a.pa_image = prior->pa_image.get(); a.row_const = prior->row_const.get(); a.neg_log_nllw = prior->nlw.get();
    a.pa_frag32 = prior->frag32.get();
    for (int m = 0; m < k2b::kPriorMaxGauss; ++m) a.inv_scale[m] = prior->inv_scale[m];
    a.frames_per_wg = 0;
    a.num_gauss = prior->M;
    memcpy(a.lane_target, t.lane_target, sizeof a.lane_target);
    fill_call_fields(a, cfg, c, coef);
    a.tr_prior = c.tr_prior ? c.tr_prior : c.in.tr;
    a.opt_mask = (cfg->optimize_mask & 15) & (cfg->freeze_betas ? ~4 : ~0);
    a.transl_prior_w = cfg->transl_prior_weight;
    a.force_shape = cfg->debug_launch_shape;
    a.num_cus = device_cus();
    a.lb_mode = c.lbfgs.mode;
    if (const k2b::LbfgsArgs* lb = c.lbfgs.args) { a.lbv = *lb; a.lb_loss = lb->loss_in; a.lb_grad = lb->grad_in; a.lb_history = lb->H; }
    a.lb_chain_max_iter = c.lbfgs.chain_max_iter;
    if (!t.vsel.empty())
        return fit_world_vertex_joints(model, cfg, a, a.tr_prior, 0, t, c.stream,
                                       [&](const k2b::FitArgs& e) { return k2b::launch_fit_world(e, c.stream); });
    HIP_TRY(k2b::launch_fit_world(a, c.stream, c.chain.frames));
    return K2B_OK;
}

// The call of a k2b_fit_world-shaped entry (frames, optional arrays, gradient output) goes through the rules, then the set-up.
struct FrameArgs {
    int32_t B, K;
    const int32_t* model_joint_index;
    const float *targets, *conf;
    ConstParams in;
    const float *preserve, *tr_prior;
    Params out;
    float *loss_out, *grad_out;
    void* stream;
};
int fit_frames(k2b::rules::Entry entry, const k2b_model* model, const k2b_prior* prior, const k2b_fit_config* cfg, const FrameArgs& f,
               int num_views = 0, const k2b_camera* cameras = nullptr) {
    FitCall c = fit_call(f.B, f.K, f.model_joint_index, f.targets, f.conf, f.in, f.out, f.loss_out, f.stream);
    c.preserve = f.preserve; c.tr_prior = f.tr_prior; c.grad_out = f.grad_out;
    c.num_views = num_views; c.cameras = cameras;
    k2b::rules::Facts facts;
    bool go;
    if (const int rc = judge(rule_call(entry, model, prior, cfg, c, &facts), &go); rc != K2B_OK || !go) return rc;
    return fit_world_impl(model, prior, cfg, c);
}

// Many warm-start sequences of different lengths side by side (the Adam branch): every sequence is k2b_fit_sequence's chain,
// packed frames [sum T][...], ONE launch (the fused kernel for 24-joint models, the tree kernel for SMPL-H / SMPL-X).  A
// sequence's result does not depend on the others, on their number or on their order.  k2b_fit_sequences fits 3D targets;
// k2b_fit_image_sequences (ABI 1.8) is the same chain under the projected joint term, whose follow-up frames may hold the shape;
// k2b_fit_multiview_sequences (ABI 1.11) that chain under the multi-view term (FitCall::num_views, cameras set by the entry).
int fit_ragged_chain(k2b::rules::Entry entry, const k2b_model* model, const k2b_prior* prior, const k2b_fit_config* cfg, int32_t num_sequences,
                     const int32_t* lengths, const int32_t* offsets, int32_t followup_iters, bool freeze_shape, FitCall c) {
    k2b::rules::Facts facts;
    k2b::rules::Call r = rule_call(entry, model, prior, cfg, c, &facts);
    r.num_sequences = num_sequences; r.lengths = lengths; r.offsets = offsets; r.followup_iters = followup_iters;
    bool go;
    if (const int rc = judge(r, &go); rc != K2B_OK || !go) return rc;
    const k2b::rules::RaggedSlots slots = k2b::rules::ragged_order(num_sequences, lengths, offsets);
    StreamWorkspace ws(c.stream);
    HIP_TRY(ws.alloc(slots.meta.size() * sizeof(int)));
    int* meta = reinterpret_cast<int*>(ws.get());
    if (const int rc = upload_slots(slots.meta, meta, c.stream); rc != K2B_OK) return rc;
    // chain.len > 1 selects the chain; the steps come from the table (a workgroup walks its longest sequence)
    c.B = slots.slots;
    c.chain.len = slots.max_len > 1 ? slots.max_len : 2; c.chain.iters = followup_iters; c.chain.meta = meta;
    c.chain.freeze_shape = freeze_shape;
    c.chain.frames = (long long)offsets[num_sequences - 1] + lengths[num_sequences - 1];
    return fit_world_impl(model, prior, cfg, c);
}

}  // namespace

namespace k2b {
namespace host {

hipError_t start_in_place(int B, int D, int NB, const ConstParams& in, const Params& out, const float* preserve, const float* tr_prior,
                          float* pres, float* trp, hipStream_t stream) {
    const struct { const float* src; float* dst; size_t n; } cp[] = {
        {preserve ? preserve : in.bp, pres, (size_t)B * D}, {tr_prior ? tr_prior : in.tr, trp, (size_t)B * 3},
        {in.go, out.go, (size_t)B * 3}, {in.bp, out.bp, (size_t)B * D}, {in.be, out.be, (size_t)B * NB}, {in.tr, out.tr, (size_t)B * 3}};
    for (const auto& c : cp)
        if (c.src != c.dst)
            if (const hipError_t e = hipMemcpyAsync(c.dst, c.src, c.n * sizeof(float), hipMemcpyDeviceToDevice, stream); e != hipSuccess) return e;
    return hipSuccess;
}

int fit_world_impl(const k2b_model* model_c, const k2b_prior* prior, const k2b_fit_config* cfg, const FitCall& c) {
    k2b_model* model = const_cast<k2b_model*>(model_c);
    const rules::FusedEligibility el = rules::fused_eligibility(fit_facts(model, prior), *cfg);
    if (!el.fused) return fit_tree(model, const_cast<k2b_prior*>(prior), cfg, el.prior_dims, c);
    return fit_fused(model, prior, cfg, c);
}

// The slot table goes up through pinned staging owned by the calling thread: the copy is stream-ordered and the host never
// waits for the stream - only, before the staging is reused, for the previous call's copy out of it (normally long done).
// (One grow-only pinned buffer and one event per thread that calls the entries; they live as long as the thread's runtime.)
int upload_slots(const std::vector<int>& meta, int* dev, hipStream_t stream) {
    struct Stage { int* host = nullptr; size_t cap = 0; hipEvent_t copied = nullptr; };
    thread_local Stage st;
    const size_t n = meta.size();
    if (st.copied) HIP_TRY(hipEventSynchronize(st.copied));
    if (n > st.cap) {
        if (st.host) HIP_TRY(hipHostFree(st.host));
        st.host = nullptr;
        st.cap = 0;
        HIP_TRY(hipHostMalloc((void**)&st.host, n * sizeof(int), hipHostMallocDefault));
        st.cap = n;
    }
    if (!st.copied) HIP_TRY(hipEventCreateWithFlags(&st.copied, hipEventDisableTiming));
    memcpy(st.host, meta.data(), n * sizeof(int));
    HIP_TRY(hipMemcpyAsync(dev, st.host, n * sizeof(int), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipEventRecord(st.copied, stream));
    return K2B_OK;
}

}  // namespace host
}  // namespace k2b

extern "C" {

using k2b::rules::Entry;

int k2b_fit_world(const k2b_model* model, const k2b_prior* prior, const k2b_fit_config* cfg, int32_t B, int32_t K,
                  const int32_t* model_joint_index, const float* j3d, const float* conf, const float* go_in,
                  const float* bp_in, const float* be_in, const float* tr_in, const float* preserve,
                  const float* tr_prior, float* go_out,
                  float* bp_out, float* be_out, float* tr_out, float* loss_out, float* grad_out, void* stream) {
    return fit_frames(Entry::fit_world, model, prior, cfg, {B, K, model_joint_index, j3d, conf, {go_in, bp_in, be_in, tr_in}, preserve, tr_prior,
                                                            {go_out, bp_out, be_out, tr_out}, loss_out, grad_out, stream});
}

int k2b_fit_sequence(const k2b_model* model, const k2b_prior* prior, const k2b_fit_config* cfg, int32_t num_sequences,
                     int32_t frames_per_sequence, int32_t followup_iters, int32_t K, const int32_t* model_joint_index,
                     const float* j3d, const float* conf, const float* go_in, const float* bp_in, const float* be_in,
                     const float* tr_in, float* go_out, float* bp_out, float* be_out, float* tr_out, float* loss_out,
                     void* stream) {
    FitCall c = fit_call(num_sequences, K, model_joint_index, j3d, conf, {go_in, bp_in, be_in, tr_in}, {go_out, bp_out, be_out, tr_out}, loss_out,
                         stream);
    k2b::rules::Facts facts;
    k2b::rules::Call r = rule_call(Entry::fit_sequence, model, prior, cfg, c, &facts);
    r.frames_per_sequence = frames_per_sequence; r.followup_iters = followup_iters;
    bool go;
    if (const int rc = judge(r, &go); rc != K2B_OK || !go) return rc;
    if (frames_per_sequence == 1) {           // a chain of one: the first-frame fit (no preserve term)
        k2b_fit_config c1 = *cfg;
        c1.pose_preserve_weight = 0.0f;
        return fit_world_impl(model, prior, &c1, c);
    }
    c.chain.len = frames_per_sequence; c.chain.iters = followup_iters;
    return fit_world_impl(model, prior, cfg, c);
}

int k2b_fit_sequences(const k2b_model* model, const k2b_prior* prior, const k2b_fit_config* cfg, int32_t num_sequences,
                      const int32_t* lengths, const int32_t* offsets, int32_t followup_iters, int32_t K,
                      const int32_t* model_joint_index, const float* j3d, const float* conf, const float* go_in,
                      const float* bp_in, const float* be_in, const float* tr_in, float* go_out, float* bp_out, float* be_out,
                      float* tr_out, float* loss_out, void* stream) {
    return fit_ragged_chain(Entry::fit_sequences, model, prior, cfg, num_sequences, lengths, offsets, followup_iters, false,
                            fit_call(0, K, model_joint_index, j3d, conf, {go_in, bp_in, be_in, tr_in}, {go_out, bp_out, be_out, tr_out}, loss_out, stream));
}

int k2b_fit_image_sequences(const k2b_model* model, const k2b_prior* prior, const k2b_fit_config* cfg, int32_t num_sequences,
                            const int32_t* lengths, const int32_t* offsets, int32_t followup_iters, int32_t followup_freeze_betas,
                            int32_t K, const int32_t* model_joint_index, const float* keypoints, const float* conf,
                            const float* go_in, const float* bp_in, const float* be_in, const float* tr_in, float* go_out,
                            float* bp_out, float* be_out, float* tr_out, float* loss_out, void* stream) {
    return fit_ragged_chain(Entry::fit_image_sequences, model, prior, cfg, num_sequences, lengths, offsets, followup_iters, followup_freeze_betas != 0,
                            fit_call(0, K, model_joint_index, keypoints, conf, {go_in, bp_in, be_in, tr_in}, {go_out, bp_out, be_out, tr_out}, loss_out,
                                     stream));
}

// Independent frames of 2D keypoints, surface targets included (ABI 1.9): k2b_fit_world under projection, the one entry whose
// surface targets take the projected form of k2b_surface.hip.
int k2b_fit_image(const k2b_model* model, const k2b_prior* prior, const k2b_fit_config* cfg, int32_t B, int32_t K,
                  const int32_t* model_joint_index, const float* keypoints, const float* conf, const float* go_in,
                  const float* bp_in, const float* be_in, const float* tr_in, const float* preserve, const float* tr_prior,
                  float* go_out, float* bp_out, float* be_out, float* tr_out, float* loss_out, float* grad_out, void* stream) {
    return fit_frames(Entry::fit_image, model, prior, cfg, {B, K, model_joint_index, keypoints, conf, {go_in, bp_in, be_in, tr_in}, preserve, tr_prior,
                                                            {go_out, bp_out, be_out, tr_out}, loss_out, grad_out, stream});
}

// Independent frames of 2D keypoints seen by several calibrated cameras (ABI 1.10): the shared path with FitCall::num_views set.
int k2b_fit_multiview(const k2b_model* model, const k2b_prior* prior, const k2b_fit_config* cfg, int32_t B, int32_t num_views,
                      const k2b_camera* cameras, int32_t K, const int32_t* model_joint_index, const float* keypoints,
                      const float* conf, const float* go_in, const float* bp_in, const float* be_in, const float* tr_in,
                      const float* preserve, const float* tr_prior, float* go_out, float* bp_out, float* be_out, float* tr_out,
                      float* loss_out, float* grad_out, void* stream) {
    return fit_frames(Entry::fit_multiview, model, prior, cfg, {B, K, model_joint_index, keypoints, conf, {go_in, bp_in, be_in, tr_in}, preserve,
                                                                tr_prior, {go_out, bp_out, be_out, tr_out}, loss_out, grad_out, stream},
                      num_views, cameras);
}

// Warm-start chains over videos of a calibrated rig (ABI 1.11): k2b_fit_image_sequences' chain with FitCall::num_views set.
int k2b_fit_multiview_sequences(const k2b_model* model, const k2b_prior* prior, const k2b_fit_config* cfg, int32_t num_sequences,
                                const int32_t* lengths, const int32_t* offsets, int32_t followup_iters, int32_t followup_freeze_betas,
                                int32_t num_views, const k2b_camera* cameras, int32_t K, const int32_t* model_joint_index,
                                const float* keypoints, const float* conf, const float* go_in, const float* bp_in, const float* be_in,
                                const float* tr_in, float* go_out, float* bp_out, float* be_out, float* tr_out, float* loss_out,
                                void* stream) {
    FitCall c = fit_call(0, K, model_joint_index, keypoints, conf, {go_in, bp_in, be_in, tr_in}, {go_out, bp_out, be_out, tr_out}, loss_out, stream);
    c.num_views = num_views; c.cameras = cameras;
    return fit_ragged_chain(Entry::fit_multiview_sequences, model, prior, cfg, num_sequences, lengths, offsets, followup_iters,
                            followup_freeze_betas != 0, c);
}

int k2b_sequence_order(int32_t num_sequences, const int32_t* lengths, const int32_t* offsets, int32_t* order_out, int32_t* num_slots) {
    k2b::rules::Verdict v;
    if (k2b::rules::check_ragged("k2b_sequence_order", num_sequences, lengths, offsets, v) != K2B_OK) return fail(v.code, "%s", v.message);
    const k2b::rules::RaggedSlots r = k2b::rules::ragged_order(num_sequences, lengths, offsets);
    if (!num_slots || (r.slots > 0 && !order_out)) return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_sequence_order: NULL output");
    for (int i = 0; i < r.slots; ++i) order_out[i] = r.meta[(size_t)i * 4];
    *num_slots = r.slots;
    return K2B_OK;
}

}  // extern "C"
