// k2b_api_fit.hip — the fit calls of the C ABI (include/k2b.h): one description of a call (FitCall, k2b_host.h), one set-up
// path for the two fit kernels (the fused 24-lane kernel, k2b_fit.hip; the tree kernel, k2b_fit_tree.hip), the Adam path with
// surface targets, and the Adam entries for frames, sequences and ragged sequences.
#include <algorithm>
#include <cstring>
#include <type_traits>

#include "k2b_host.h"

using namespace k2b::host;

namespace {

// ---- set-up shared by the two fit kernels ----------------------------------------------------------------------------------
// the argument checks of a call, in the order the entries have always made them
int validate_call(const k2b_model* model, const k2b_fit_config* cfg, const FitCall& c) {
    if (c.B < 0) return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_fit_world: num_frames=%d", c.B);
    if (c.K < 1 || c.K > model->J + model->E + model->lmk.L) return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_fit_world: num_targets=%d out of range", c.K);
    if (!c.model_joint_index) return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_fit_world: model_joint_index is NULL");
    if (cfg->num_iters < 1 || cfg->num_iters > (1 << 20)) return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_fit_world: num_iters=%d", cfg->num_iters);
    if (!(cfg->step_size >= 0.0) || !(cfg->adam_beta1 >= 0.0 && cfg->adam_beta1 < 1.0) || !(cfg->adam_beta2 >= 0.0 && cfg->adam_beta2 < 1.0))
        return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_fit_world: bad Adam hyper-parameters");
    if (!adam_eps_ok(cfg->adam_eps))
        return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_fit_world: adam_eps=%g must round to a normal positive float32", cfg->adam_eps);
    if (c.B == 0) return K2B_OK;             // (nothing to fit: the callers return here)
    if (!c.j3d || !c.in.go || !c.in.bp || !c.in.be || !c.in.tr || !c.out.go || !c.out.bp || !c.out.be || !c.out.tr)
        return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_fit_world: NULL parameter / target buffer (init transl is required, world_space.py:118-119)");
    return K2B_OK;
}

// The targets of a call by kind: kinematic joints (model index < J) are fitted by a lane of the fit kernel, surface targets
// (extra joints, landmarks) by k2b_vertex_term_kernel / k2b_surface_term_kernel.
struct Targets {
    int lane_target[64];                     // target column fitted by lane l, or -1
    std::vector<int> vsel, vcol;             // surface targets: model index, target column
    int num_kinematic = 0, max_depth = 0;    // (depth of the deepest targeted joint)
};
// lane_of: the lane of every joint (tree kernel), or null where lane = joint (24-lane kernel)
int classify_targets(const k2b_model* model, const FitCall& c, const int* lane_of, Targets* t) {
    const int J = model->J;
    for (int& l : t->lane_target) l = -1;
    for (int k = 0; k < c.K; ++k) {
        const int j = c.model_joint_index[k];
        if (j < 0 || j >= J + model->E + model->lmk.L)
            return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_fit_world: model_joint_index[%d]=%d out of range", k, j);
        if (j >= J) {
            if ((int)t->vsel.size() >= k2b::kSurfMaxTargets)
                return fail(K2B_ERR_UNSUPPORTED, "k2b_fit_world: more than %d surface targets (vertex-selected joints and landmarks)", k2b::kSurfMaxTargets);
            t->vsel.push_back(j);
            t->vcol.push_back(k);
            continue;
        }
        const int l = lane_of ? lane_of[j] : j;
        if (t->lane_target[l] >= 0) return fail(K2B_ERR_UNSUPPORTED, "k2b_fit_world: joint %d is targeted twice", j);
        t->lane_target[l] = k;
        ++t->num_kinematic;
        t->max_depth = std::max(t->max_depth, model->kin.depth[j]);
    }
    return K2B_OK;
}
int check_surface_targets(const Targets& t, const FitCall& c, int J) {
    if (t.vsel.empty()) return K2B_OK;
    if (t.num_kinematic == 0)
        return fail(K2B_ERR_UNSUPPORTED, "k2b_fit_world: at least one kinematic joint (model index < %d) must be among the targets", J);
    if (c.chain.len > 1)
        return fail(K2B_ERR_UNSUPPORTED, "k2b_fit_sequence: vertex-selected joints are not built into the chain (fit frame by frame)");
    return K2B_OK;
}
// k2b_fit_config::projection: its values, and what the projected joint term is not built into
int check_projection(const k2b_fit_config* cfg, const FitCall& c) {
    if (cfg->projection == 0) return K2B_OK;
    if (cfg->projection != 1) return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_fit_world: projection=%d must be 0 or 1", cfg->projection);
    if (const int rc = check_focal("k2b_fit_world", cfg->focal); rc != K2B_OK) return rc;
    // (a chain under projection is k2b_fit_image_sequences' alone: FitCall::Chain::image)
    if ((c.chain.len > 1 && !c.chain.image) || c.lbfgs.mode != k2b::LbMode::none)
        return fail(K2B_ERR_UNSUPPORTED, "k2b_fit_world: the projected joint term is built for independent frames under Adam only");
    return K2B_OK;
}
// (k2b_fit_image alone lets them through: FitCall::projected_surface)
int check_projected_targets(const k2b_fit_config* cfg, const FitCall& c, const Targets& t) {
    if (cfg->projection != 0 && !t.vsel.empty() && !c.projected_surface)
        return fail(K2B_ERR_UNSUPPORTED, "k2b_fit_world: surface targets (vertex-selected joints, landmarks) keep the 3D term: "
                    "no projection for model indices beyond the kinematic joints");
    return K2B_OK;
}
int check_debug_shape(const k2b_fit_config* cfg) {
    if (cfg->debug_launch_shape < k2b::ForceShape::automatic || cfg->debug_launch_shape > k2b::ForceShape::wide)
        return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_fit_world: debug_launch_shape=%d must be 0..4", cfg->debug_launch_shape);
    return K2B_OK;
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
    a.chain_freeze_shape = c.chain.len > 1 && c.chain.image && c.chain.freeze_shape ? 1 : 0;
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
    if (prior_dims < 3 || prior_dims > 64 || prior_dims % 3 != 0 || prior_dims > prior->D || prior_dims > 3 * (J - 1))
        return fail(K2B_ERR_UNSUPPORTED, "k2b_fit_world: the tree kernel takes a prior over the first 3..63 body-pose dimensions "
                    "(a multiple of 3, at most the mixture's %d), got %d", prior->D, prior_dims);
    if (cfg->transl_prior_weight != 0.0f || c.tr_prior)
        return fail(K2B_ERR_UNSUPPORTED, "k2b_fit_world: the translation prior (camera-space fitter) is not built for %d-joint models", J);
    if (const int rc = validate_call(model, cfg, c); rc != K2B_OK || c.B == 0) return rc;
    k2b::FitTreeArgs a{};
    Targets t;
    if (const int rc = classify_targets(model, c, model->kin.pos.data(), &t); rc != K2B_OK) return rc;
    if (const int rc = check_projected_targets(cfg, c, t); rc != K2B_OK) return rc;
    memcpy(a.lane_target, t.lane_target, sizeof a.lane_target);
    for (int i = 0; i < 4; ++i) {
        const int ai = cfg->angle_prior_index[i];
        if (ai < 0 || ai >= prior_dims) return fail(K2B_ERR_UNSUPPORTED, "k2b_fit_world: angle_prior_index[%d]=%d must be in [0,%d)", i, ai, prior_dims);
        a.angle_index[i] = ai;
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
    if (J > 63 || a.num_rounds > 4) return fail(K2B_ERR_UNSUPPORTED, "k2b_fit_world: the tree kernel takes up to 63 joints and depth 15");
    a.pfrag = prior->frag32.get(); a.ph = f->ph.get(); a.pb = f->pb.get(); a.pmu = f->pmu.get(); a.pcl = f->pcl.get();
    for (int m = 0; m < k2b::kPriorMaxGauss; ++m) a.inv_scale[m] = prior->inv_scale[m];
    a.num_gauss = prior->M; a.prior_dims = prior_dims;
    fill_call_fields(a, cfg, c, coef);
    a.num_betas_prior = cfg->num_betas_prior > 0 ? (cfg->num_betas_prior < NB ? cfg->num_betas_prior : NB) : NB;
    a.opt_mask = cfg->optimize_mask & 15;
    if (const int rc = check_debug_shape(cfg); rc != K2B_OK) return rc;
    a.debug_shape = cfg->debug_launch_shape <= k2b::TreeShape::comp_waves ? cfg->debug_launch_shape : k2b::TreeShape::automatic;
    const int cus = device_cus();
    if (!t.vsel.empty()) {
        if (const int rc = check_surface_targets(t, c, J); rc != K2B_OK) return rc;
        return fit_world_vertex_joints(model, cfg, a, nullptr, cfg->freeze_betas ? a.num_betas_prior : 0, t, c.stream,
                                       [&](const k2b::FitTreeArgs& e) { return k2b::launch_fit_tree(e, cus, c.stream); });
    }
    HIP_TRY(k2b::launch_fit_tree(a, cus, c.stream));
    return K2B_OK;
}

// the 24-joint SMPL tree with the prior over the whole pose: k2b_fit.hip
int fit_fused(k2b_model* model, const k2b_prior* prior, const k2b_fit_config* cfg, const FitCall& c) {
    if (const int rc = validate_call(model, cfg, c); rc != K2B_OK || c.B == 0) return rc;
    k2b::FitArgs a{};
    Targets t;
    if (const int rc = classify_targets(model, c, nullptr, &t); rc != K2B_OK) return rc;
    if (const int rc = check_projected_targets(cfg, c, t); rc != K2B_OK) return rc;
    if (cfg->projection != 0 && model->fit_scan64)
        return fail(K2B_ERR_UNSUPPORTED, "k2b_fit_world: the projected joint term is built for the fp32 scans only (this model has no scan "
                    "plan, or was created under K2B_FIT_SCAN64)");
    if (const int rc = check_surface_targets(t, c, model->J); rc != K2B_OK) return rc;
    for (int i = 0; i < 4; ++i) {
        const int ai = cfg->angle_prior_index[i];
        if (ai < 0 || ai >= 64) return fail(K2B_ERR_UNSUPPORTED, "k2b_fit_world: angle_prior_index[%d]=%d must be in [0,64)", i, ai);
        a.angle_index[i] = ai;
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
    if (const int rc = check_debug_shape(cfg); rc != K2B_OK) return rc;
    a.force_shape = cfg->debug_launch_shape;
    a.num_cus = device_cus();
    a.lb_mode = c.lbfgs.mode;
    if (const k2b::LbfgsArgs* lb = c.lbfgs.args) { a.lbv = *lb; a.lb_loss = lb->loss_in; a.lb_grad = lb->grad_in; a.lb_history = lb->H; }
    a.lb_chain_max_iter = c.lbfgs.chain_max_iter;
    if (c.lbfgs.mode != k2b::LbMode::none && (!t.vsel.empty() || (c.chain.len > 1 && c.lbfgs.mode != k2b::LbMode::persistent) || !c.lbfgs.args))
        return fail(K2B_ERR_UNSUPPORTED, "k2b_fit_world: the fused L-BFGS step needs kinematic targets and independent frames");
    if (!t.vsel.empty())
        return fit_world_vertex_joints(model, cfg, a, a.tr_prior, 0, t, c.stream,
                                       [&](const k2b::FitArgs& e) { return k2b::launch_fit_world(e, c.stream); });
    HIP_TRY(k2b::launch_fit_world(a, c.stream));
    return K2B_OK;
}

}  // namespace

namespace k2b {
namespace host {

FusedEligibility fused_eligibility(const k2b_model* model, const k2b_prior* prior, const k2b_fit_config* cfg) {
    const int pose_dims_all = 3 * (model->J - 1);
    const int prior_dims = cfg->prior_pose_dims > 0 ? cfg->prior_pose_dims : (prior->D < pose_dims_all ? prior->D : pose_dims_all);
    const bool fused = model->fit_ok && prior->D == pose_dims_all && prior_dims == pose_dims_all &&
                       (cfg->num_betas_prior == 0 || cfg->num_betas_prior == model->NB);
    return {prior_dims, fused};
}

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
    if (!model || !prior || !cfg) return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_fit_world: model, prior and cfg are required");
    if (c.chain.len > 1 && (c.chain.iters < 1 || c.chain.iters > (1 << 20)))
        return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_fit_sequence: followup_iters=%d", c.chain.iters);
    if (c.chain.len > 1 && (c.preserve || c.tr_prior || c.grad_out || cfg->transl_prior_weight != 0.0f))
        return fail(K2B_ERR_UNSUPPORTED, "k2b_fit_sequence: no explicit preserve pose, translation prior or gradient output in a chain");
    // (several views: the entry has checked its own form of the projection - cfg->focal is not read there)
    if (const int rc = c.num_views > 0 ? K2B_OK : check_projection(cfg, c); rc != K2B_OK) return rc;
    const FusedEligibility el = fused_eligibility(model, prior, cfg);
    if (!el.fused) return fit_tree(model, const_cast<k2b_prior*>(prior), cfg, el.prior_dims, c);
    return fit_fused(model, prior, cfg, c);
}

int ragged_slots(const char* who, int32_t S, const int32_t* lengths, const int32_t* offsets, RaggedSlots* r) {
    if (S < 0) return fail(K2B_ERR_INVALID_ARGUMENT, "%s: num_sequences=%d", who, S);
    if (S > 0 && (!lengths || !offsets)) return fail(K2B_ERR_INVALID_ARGUMENT, "%s: lengths and offsets are required", who);
    int64_t next = 0;
    for (int s = 0; s < S; ++s) {
        if (lengths[s] < 0) return fail(K2B_ERR_INVALID_ARGUMENT, "%s: lengths[%d]=%d", who, s, lengths[s]);
        if (offsets[s] != next)
            return fail(K2B_ERR_INVALID_ARGUMENT, "%s: offsets[%d]=%d, expected %lld (the exclusive prefix sum of lengths)", who, s,
                        offsets[s], (long long)next);
        next += lengths[s];
        if (next > ((int64_t)1 << 30)) return fail(K2B_ERR_INVALID_ARGUMENT, "%s: more than 2^30 frames", who);
    }
    std::vector<int> order;
    for (int s = 0; s < S; ++s)
        if (lengths[s] > 0) order.push_back(s);
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return lengths[x] > lengths[y]; });
    r->slots = (int)order.size();
    r->max_len = r->slots ? lengths[order[0]] : 0;
    r->meta.assign((size_t)r->slots * 4, 0);
    for (int i = 0; i < r->slots; ++i) {
        r->meta[(size_t)i * 4 + 0] = order[i];
        r->meta[(size_t)i * 4 + 1] = offsets[order[i]];
        r->meta[(size_t)i * 4 + 2] = lengths[order[i]];
    }
    return K2B_OK;
}
int check_focal(const char* who, const float* focal) {
    for (int i = 0; i < 2; ++i)
        if (!(focal[i] > 0.0f) || !(focal[i] <= 3.402823466e38f))      // (NaN fails the first comparison)
            return fail(K2B_ERR_INVALID_ARGUMENT, "%s: focal[%d]=%g must be finite and positive", who, i, (double)focal[i]);
    return K2B_OK;
}
bool kinematic_only(const k2b_model* m, int32_t K, const int32_t* idx) {
    for (int k = 0; k < K; ++k)
        if (idx[k] < 0 || idx[k] >= m->J) return false;
    return true;
}
// every model joint index inside the model's outputs (joints, extra joints, landmarks)
int check_targets(const char* who, const k2b_model* m, int32_t K, const int32_t* idx) {
    if (K < 1 || !idx) return fail(K2B_ERR_INVALID_ARGUMENT, "%s: num_targets=%d / model_joint_index", who, K);
    for (int k = 0; k < K; ++k)
        if (idx[k] < 0 || idx[k] >= m->J + m->E + m->lmk.L)
            return fail(K2B_ERR_INVALID_ARGUMENT, "%s: model_joint_index[%d]=%d out of range", who, k, idx[k]);
    return K2B_OK;
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

int k2b_fit_world(const k2b_model* model, const k2b_prior* prior, const k2b_fit_config* cfg, int32_t B, int32_t K,
                  const int32_t* model_joint_index, const float* j3d, const float* conf, const float* go_in,
                  const float* bp_in, const float* be_in, const float* tr_in, const float* preserve,
                  const float* tr_prior, float* go_out,
                  float* bp_out, float* be_out, float* tr_out, float* loss_out, float* grad_out, void* stream) {
    FitCall c = fit_call(B, K, model_joint_index, j3d, conf, stream);
    c.in = {go_in, bp_in, be_in, tr_in};
    c.out = {go_out, bp_out, be_out, tr_out};
    c.preserve = preserve; c.tr_prior = tr_prior; c.loss_out = loss_out; c.grad_out = grad_out;
    return fit_world_impl(model, prior, cfg, c);
}

int k2b_fit_sequence(const k2b_model* model, const k2b_prior* prior, const k2b_fit_config* cfg, int32_t num_sequences,
                     int32_t frames_per_sequence, int32_t followup_iters, int32_t K, const int32_t* model_joint_index,
                     const float* j3d, const float* conf, const float* go_in, const float* bp_in, const float* be_in,
                     const float* tr_in, float* go_out, float* bp_out, float* be_out, float* tr_out, float* loss_out,
                     void* stream) {
    if (const int rc = refuse_projection("k2b_fit_sequence", cfg); rc != K2B_OK) return rc;
    if (frames_per_sequence < 1) return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_fit_sequence: frames_per_sequence=%d", frames_per_sequence);
    if ((int64_t)num_sequences * frames_per_sequence > (int64_t)1 << 30)
        return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_fit_sequence: %d x %d frames", num_sequences, frames_per_sequence);
    FitCall c = fit_call(num_sequences, K, model_joint_index, j3d, conf, stream);
    c.in = {go_in, bp_in, be_in, tr_in};
    c.out = {go_out, bp_out, be_out, tr_out};
    c.loss_out = loss_out;
    if (frames_per_sequence == 1) {           // a chain of one: the first-frame fit (no preserve term)
        k2b_fit_config c1 = *cfg;
        c1.pose_preserve_weight = 0.0f;
        return fit_world_impl(model, prior, &c1, c);
    }
    c.chain.len = frames_per_sequence; c.chain.iters = followup_iters;
    return fit_world_impl(model, prior, cfg, c);
}

// Many warm-start sequences of different lengths side by side (the Adam branch): every sequence is k2b_fit_sequence's chain,
// packed frames [sum T][...], ONE launch (the fused kernel for 24-joint models, the tree kernel for SMPL-H / SMPL-X).  A
// sequence's result does not depend on the others, on their number or on their order.
int k2b_fit_sequences(const k2b_model* model, const k2b_prior* prior, const k2b_fit_config* cfg, int32_t num_sequences,
                      const int32_t* lengths, const int32_t* offsets, int32_t followup_iters, int32_t K,
                      const int32_t* model_joint_index, const float* j3d, const float* conf, const float* go_in,
                      const float* bp_in, const float* be_in, const float* tr_in, float* go_out, float* bp_out, float* be_out,
                      float* tr_out, float* loss_out, void* stream_v) {
    const char* who = "k2b_fit_sequences";
    RaggedSlots r;
    if (const int rc = ragged_slots(who, num_sequences, lengths, offsets, &r); rc != K2B_OK) return rc;
    if (!model || !prior || !cfg) return fail(K2B_ERR_INVALID_ARGUMENT, "%s: model, prior and cfg are required", who);
    if (const int rc = refuse_projection(who, cfg); rc != K2B_OK) return rc;
    if (followup_iters < 1 || followup_iters > (1 << 20)) return fail(K2B_ERR_INVALID_ARGUMENT, "%s: followup_iters=%d", who, followup_iters);
    if (cfg->num_iters < 1 || cfg->num_iters > (1 << 20)) return fail(K2B_ERR_INVALID_ARGUMENT, "%s: num_iters=%d", who, cfg->num_iters);
    if (cfg->transl_prior_weight != 0.0f) return fail(K2B_ERR_INVALID_ARGUMENT, "%s: transl_prior_weight must be 0 in a chain", who);
    if (const int rc = check_targets(who, model, K, model_joint_index); rc != K2B_OK) return rc;
    if (r.slots == 0) return K2B_OK;
    if (!j3d || !go_in || !bp_in || !be_in || !tr_in || !go_out || !bp_out || !be_out || !tr_out)
        return fail(K2B_ERR_INVALID_ARGUMENT, "%s: NULL parameter / target buffer", who);
    if (!kinematic_only(model, K, model_joint_index))
        return fail(K2B_ERR_UNSUPPORTED, "%s: surface targets (vertex-selected joints, landmarks) are not built into the chain", who);
    hipStream_t stream = (hipStream_t)stream_v;
    StreamWorkspace ws(stream);
    HIP_TRY(ws.alloc(r.meta.size() * sizeof(int)));
    int* meta = reinterpret_cast<int*>(ws.get());
    if (const int rc = upload_slots(r.meta, meta, stream); rc != K2B_OK) return rc;
    // chain.len > 1 selects the chain; the steps come from the table (a workgroup walks its longest sequence)
    FitCall c = fit_call(r.slots, K, model_joint_index, j3d, conf, stream_v);
    c.in = {go_in, bp_in, be_in, tr_in};
    c.out = {go_out, bp_out, be_out, tr_out};
    c.loss_out = loss_out;
    c.chain.len = r.max_len > 1 ? r.max_len : 2; c.chain.iters = followup_iters; c.chain.meta = meta;
    return fit_world_impl(model, prior, cfg, c);
}

// Warm-start chains over 2D keypoints (ABI 1.8): k2b_fit_sequences' chain with the projected joint term, the one entry that
// lets a chain through check_projection (FitCall::Chain::image).  Every refusal comes before anything is queued.
int k2b_fit_image_sequences(const k2b_model* model, const k2b_prior* prior, const k2b_fit_config* cfg, int32_t num_sequences,
                            const int32_t* lengths, const int32_t* offsets, int32_t followup_iters, int32_t followup_freeze_betas,
                            int32_t K, const int32_t* model_joint_index, const float* keypoints, const float* conf,
                            const float* go_in, const float* bp_in, const float* be_in, const float* tr_in, float* go_out,
                            float* bp_out, float* be_out, float* tr_out, float* loss_out, void* stream_v) {
    const char* who = "k2b_fit_image_sequences";
    RaggedSlots r;
    if (const int rc = ragged_slots(who, num_sequences, lengths, offsets, &r); rc != K2B_OK) return rc;
    if (!model || !prior || !cfg) return fail(K2B_ERR_INVALID_ARGUMENT, "%s: model, prior and cfg are required", who);
    if (cfg->projection != 1)
        return fail(K2B_ERR_INVALID_ARGUMENT, "%s: projection=%d must be 1 (3D targets: k2b_fit_sequences)", who, cfg->projection);
    if (const int rc = check_focal(who, cfg->focal); rc != K2B_OK) return rc;
    if (followup_iters < 1 || followup_iters > (1 << 20)) return fail(K2B_ERR_INVALID_ARGUMENT, "%s: followup_iters=%d", who, followup_iters);
    if (cfg->num_iters < 1 || cfg->num_iters > (1 << 20)) return fail(K2B_ERR_INVALID_ARGUMENT, "%s: num_iters=%d", who, cfg->num_iters);
    if (cfg->transl_prior_weight != 0.0f) return fail(K2B_ERR_INVALID_ARGUMENT, "%s: transl_prior_weight must be 0 in a chain", who);
    if (const int rc = check_targets(who, model, K, model_joint_index); rc != K2B_OK) return rc;
    if (!kinematic_only(model, K, model_joint_index))
        return fail(K2B_ERR_UNSUPPORTED, "%s: surface targets (vertex-selected joints, landmarks) keep the 3D term and are not built "
                    "into the chain", who);
    if (fused_eligibility(model, prior, cfg).fused && model->fit_scan64)
        return fail(K2B_ERR_UNSUPPORTED, "%s: the projected joint term is built for the fp32 scans only (this model has no scan plan, or "
                    "was created under K2B_FIT_SCAN64)", who);
    if (r.slots == 0) return K2B_OK;
    if (!keypoints || !go_in || !bp_in || !be_in || !tr_in || !go_out || !bp_out || !be_out || !tr_out)
        return fail(K2B_ERR_INVALID_ARGUMENT, "%s: NULL parameter / target buffer", who);
    hipStream_t stream = (hipStream_t)stream_v;
    StreamWorkspace ws(stream);
    HIP_TRY(ws.alloc(r.meta.size() * sizeof(int)));
    int* meta = reinterpret_cast<int*>(ws.get());
    if (const int rc = upload_slots(r.meta, meta, stream); rc != K2B_OK) return rc;
    FitCall c = fit_call(r.slots, K, model_joint_index, keypoints, conf, stream_v);
    c.in = {go_in, bp_in, be_in, tr_in};
    c.out = {go_out, bp_out, be_out, tr_out};
    c.loss_out = loss_out;
    c.chain.len = r.max_len > 1 ? r.max_len : 2; c.chain.iters = followup_iters; c.chain.meta = meta;
    c.chain.image = true; c.chain.freeze_shape = followup_freeze_betas != 0;
    return fit_world_impl(model, prior, cfg, c);
}

// Independent frames of 2D keypoints, surface targets included (ABI 1.9): k2b_fit_world under projection with the one flag that
// lets surface targets through check_projected_targets (FitCall::projected_surface).  What the shared path would refuse about
// the surface targets is refused here first, by this entry's name; every refusal comes before anything is queued.
int k2b_fit_image(const k2b_model* model, const k2b_prior* prior, const k2b_fit_config* cfg, int32_t B, int32_t K,
                  const int32_t* model_joint_index, const float* keypoints, const float* conf, const float* go_in,
                  const float* bp_in, const float* be_in, const float* tr_in, const float* preserve, const float* tr_prior,
                  float* go_out, float* bp_out, float* be_out, float* tr_out, float* loss_out, float* grad_out, void* stream) {
    const char* who = "k2b_fit_image";
    if (!model || !prior || !cfg) return fail(K2B_ERR_INVALID_ARGUMENT, "%s: model, prior and cfg are required", who);
    if (cfg->projection != 1)
        return fail(K2B_ERR_INVALID_ARGUMENT, "%s: projection=%d must be 1 (3D targets: k2b_fit_world)", who, cfg->projection);
    if (const int rc = check_focal(who, cfg->focal); rc != K2B_OK) return rc;
    if (const int rc = check_targets(who, model, K, model_joint_index); rc != K2B_OK) return rc;
    int surface = 0;
    for (int k = 0; k < K; ++k) surface += model_joint_index[k] >= model->J ? 1 : 0;
    if (surface > k2b::kSurfMaxTargets)
        return fail(K2B_ERR_UNSUPPORTED, "%s: %d surface targets (vertex-selected joints and landmarks), at most %d per call", who, surface,
                    k2b::kSurfMaxTargets);
    if (surface > 0 && surface == K)
        return fail(K2B_ERR_UNSUPPORTED, "%s: at least one kinematic joint (model index < %d) must be among the targets", who, model->J);
    if (fused_eligibility(model, prior, cfg).fused && model->fit_scan64)
        return fail(K2B_ERR_UNSUPPORTED, "%s: the projected joint term is built for the fp32 scans only (this model has no scan plan, or "
                    "was created under K2B_FIT_SCAN64)", who);
    FitCall c = fit_call(B, K, model_joint_index, keypoints, conf, stream);
    c.in = {go_in, bp_in, be_in, tr_in};
    c.out = {go_out, bp_out, be_out, tr_out};
    c.preserve = preserve; c.tr_prior = tr_prior; c.loss_out = loss_out; c.grad_out = grad_out;
    c.projected_surface = true;
    return fit_world_impl(model, prior, cfg, c);
}

// Independent frames of 2D keypoints seen by several calibrated cameras (ABI 1.10): the shared path with FitCall::num_views set.
// Every refusal comes before anything is queued; what the shared path would refuse about the form is refused here, by name.
int k2b_fit_multiview(const k2b_model* model, const k2b_prior* prior, const k2b_fit_config* cfg, int32_t B, int32_t num_views,
                      const k2b_camera* cameras, int32_t K, const int32_t* model_joint_index, const float* keypoints,
                      const float* conf, const float* go_in, const float* bp_in, const float* be_in, const float* tr_in,
                      const float* preserve, const float* tr_prior, float* go_out, float* bp_out, float* be_out, float* tr_out,
                      float* loss_out, float* grad_out, void* stream) {
    const char* who = "k2b_fit_multiview";
    // (what concerns the views alone comes first and follows no handle)
    if (!cfg) return fail(K2B_ERR_INVALID_ARGUMENT, "%s: model, prior and cfg are required", who);
    if (num_views < 1 || num_views > k2b::kMaxViews)
        return fail(K2B_ERR_INVALID_ARGUMENT, "%s: num_views=%d must be 1..%d", who, num_views, k2b::kMaxViews);
    if (!cameras) return fail(K2B_ERR_INVALID_ARGUMENT, "%s: cameras is NULL", who);
    if (cfg->projection != 1)
        return fail(K2B_ERR_INVALID_ARGUMENT, "%s: projection=%d must be 1 (3D targets: k2b_fit_world)", who, cfg->projection);
    for (int v = 0; v < num_views; ++v) {
        const k2b_camera& cam = cameras[v];
        for (int i = 0; i < 12; ++i) {
            const float x = i < 9 ? cam.rotation[i] : cam.translation[i - 9];
            if (!(x >= -3.402823466e38f && x <= 3.402823466e38f))      // (NaN fails the first comparison)
                return fail(K2B_ERR_INVALID_ARGUMENT, "%s: cameras[%d].%s[%d] is not finite", who, v, i < 9 ? "rotation" : "translation",
                            i < 9 ? i : i - 9);
        }
        if (const int rc = check_focal(who, cam.focal); rc != K2B_OK) return rc;
    }
    if (!model || !prior) return fail(K2B_ERR_INVALID_ARGUMENT, "%s: model, prior and cfg are required", who);
    if (const int rc = check_targets(who, model, K, model_joint_index); rc != K2B_OK) return rc;
    if (!kinematic_only(model, K, model_joint_index))
        return fail(K2B_ERR_UNSUPPORTED, "%s: surface targets (vertex-selected joints, landmarks) are not built into the multi-view "
                    "term: model indices below %d only", who, model->J);
    if (fused_eligibility(model, prior, cfg).fused && model->fit_scan64)
        return fail(K2B_ERR_UNSUPPORTED, "%s: the projected joint term is built for the fp32 scans only (this model has no scan plan, or "
                    "was created under K2B_FIT_SCAN64)", who);
    if (B > 0 && (int64_t)B * num_views * K > ((int64_t)1 << 40)) return fail(K2B_ERR_INVALID_ARGUMENT, "%s: %d x %d x %d target rows", who, B, num_views, K);
    FitCall c = fit_call(B, K, model_joint_index, keypoints, conf, stream);
    c.in = {go_in, bp_in, be_in, tr_in};
    c.out = {go_out, bp_out, be_out, tr_out};
    c.preserve = preserve; c.tr_prior = tr_prior; c.loss_out = loss_out; c.grad_out = grad_out;
    c.num_views = num_views; c.cameras = cameras;
    return fit_world_impl(model, prior, cfg, c);
}

int k2b_sequence_order(int32_t num_sequences, const int32_t* lengths, const int32_t* offsets, int32_t* order_out, int32_t* num_slots) {
    RaggedSlots r;
    if (const int rc = ragged_slots("k2b_sequence_order", num_sequences, lengths, offsets, &r); rc != K2B_OK) return rc;
    if (!num_slots || (r.slots > 0 && !order_out)) return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_sequence_order: NULL output");
    for (int i = 0; i < r.slots; ++i) order_out[i] = r.meta[(size_t)i * 4];
    *num_slots = r.slots;
    return K2B_OK;
}

}  // extern "C"
