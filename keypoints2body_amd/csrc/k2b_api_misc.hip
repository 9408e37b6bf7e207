// k2b_api_misc.hip — the entries of the C ABI (include/k2b.h) that are one launch or none: version, the calling thread's
// error message, config defaults, the LBS forward, the vertex / surface terms, the Adam step, the angular and
// positional errors and the IK-GAT regressor.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <memory>

#include "k2b_host.h"

using namespace k2b::host;

namespace {

thread_local std::string g_err;

// One skin pass of k2b_lbs (k2b_lbs_plan.h, LbsPass): the fields StreamArgs and TileArgs share, then each one's own, launched by
// the model's route.
template <class Args>
Args skin_args(const k2b::PoseArgs& pa, const VertexSet& vs, const k2b::LbsPass& p, float* out, float* dump) {
    Args a{};
    a.xh = pa.xh; a.xl = pa.xl; a.a2 = pa.a2;
    a.num_frames = pa.num_frames; a.num_out = vs.num; a.out = out; a.out_stride = p.stride; a.out_row0 = p.row0;
    a.dump = dump;
    a.joints_out = p.joint_copies ? pa.joints_out : nullptr; a.joints_stride = pa.num_out_joints; a.joints_row0 = pa.num_joints;
    return a;
}
hipError_t launch_skin(const k2b_model* m, const k2b::PoseArgs& pa, const VertexSet& vs, const k2b::LbsPass& p, float* out, hipStream_t stream) {
    if (m->lbs.streams()) {
        k2b::StreamArgs sa = skin_args<k2b::StreamArgs>(pa, vs, p, out, m->dump.get());
        sa.pd = vs.spd.get(); sa.w = vs.sw.get(); sa.f32_tiles = pa.frames_padded / 32; sa.nv16 = vs.nv16;
        sa.pose_fp8 = m->lbs.pose_fp8; sa.pd8_lo_exp = vs.pd8_lo_exp; sa.pd8_hi_exp = vs.pd8_hi_exp;
        return k2b::launch_skin_stream(m->lbs.route, sa, device_cus(), stream);
    }
    k2b::TileArgs ta = skin_args<k2b::TileArgs>(pa, vs, p, out, m->dump.get());
    ta.pdh = vs.pdh.get(); ta.pdl = vs.pdl.get(); ta.w2 = vs.w2.get();
    ta.groups_a = m->lbs.groups_a; ta.k_steps_x = m->lbs.k_steps_x; ta.f_tiles = pa.frames_padded / 32; ta.v_tiles = vs.v_tiles;
    return k2b::launch_skin_tiles(ta, device_cus(), stream);
}

}  // namespace

namespace k2b {
namespace host {

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

// one cached count per device ordinal (a race repeats the query and stores the same value)
int device_cus() {
    constexpr int kMaxDevices = 64;
    static std::atomic<int> cached[kMaxDevices];
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) dev = 0;
    if ((cus = cached[dev].load(std::memory_order_relaxed)) > 0) return cus;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    cached[dev].store(cus, std::memory_order_relaxed);
    return cus;
}

}  // namespace host
}  // namespace k2b

extern "C" {

uint32_t k2b_version(void) { return (1u << 16) | 11u; }
const char* k2b_last_error(void) { return g_err.c_str(); }

uint32_t k2b_fit_config_size(void) { return (uint32_t)sizeof(k2b_fit_config); }
uint32_t k2b_camera_size(void) { return (uint32_t)sizeof(k2b_camera); }

void k2b_fit_config_default(k2b_fit_config* c) {
    if (!c) return;
    c->num_iters = 30;           // FrameOptimizeConfig.num_iters_first (core/config.py:32)
    c->step_size = 1e-2;
    c->adam_beta1 = 0.9;
    c->adam_beta2 = 0.999;
    c->adam_eps = 1e-8;
    c->sigma = 100.0f;
    c->joint_loss_weight = 600.0f;
    c->pose_prior_weight = (float)(4.78 * 1.5);
    c->angle_prior_weight = 15.2f;
    c->shape_prior_weight = 5.0f;
    c->pose_preserve_weight = 0.0f;
    c->freeze_betas = 0;
    c->conf_per_frame = 0;
    const int idx[4] = {52, 55, 9, 12};
    const float sg[4] = {1.f, -1.f, -1.f, -1.f};
    for (int i = 0; i < 4; ++i) { c->angle_prior_index[i] = idx[i]; c->angle_prior_sign[i] = sg[i]; }
    c->optimize_mask = 15;
    c->transl_prior_weight = 0.0f;
    c->debug_launch_shape = 0;
    c->prior_pose_dims = 0;
    c->num_betas_prior = 0;
    c->projection = 0;
    c->focal[0] = c->focal[1] = 0.0f;
}

int k2b_lbs(const k2b_model* model_c, int32_t B, const float* go, const float* bp, const float* be, const float* tr,
            float* joints_out, float* vertices_out, void* stream_v) {
    k2b_model* m = const_cast<k2b_model*>(model_c);
    if (!m) return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_lbs: model is NULL");
    if (B < 0) return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_lbs: num_frames=%d", B);
    if (B == 0) return K2B_OK;
    if (!go || !bp || !be) return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_lbs: NULL parameter buffer");
    if (!joints_out && !vertices_out) return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_lbs: no output requested");
    if (m->lbs.route == k2b::LbsRoute::unsupported)
        return fail(K2B_ERR_UNSUPPORTED, "k2b_lbs: %d joints; the vertex kernel is built for 17-24 (SMPL) and 49-56 (SMPL-H / SMPL-X) joints", m->J);
    hipStream_t stream = (hipStream_t)stream_v;
    const int L = m->lmk.L, bpad = k2b::lbs_frames_padded(B);
    const k2b::LbsForwardPlan plan = k2b::lbs_forward_plan(joints_out != nullptr, vertices_out != nullptr, m->J, m->V, m->E, L, m->joints_in_mesh);
    {
        std::lock_guard<std::mutex> lk(m->mu);
        if (const int rc = reserve_lbs_workspace(m, bpad); rc != K2B_OK) return rc;
    }
    k2b::PoseArgs pa{};
    pa.j_basis_lane = m->j_basis_lane.get(); pa.parents = m->parents.get();
    pa.num_joints = m->J; pa.num_betas = m->NB; pa.num_out_joints = m->J + m->E + L;   // rows of joints_out: J kinematic, E extra vertices, L landmarks
    pa.num_frames = B; pa.frames_padded = bpad; pa.k_steps_x = m->lbs.k_steps_x;
    pa.go = go; pa.bp = bp; pa.be = be; pa.tr = tr;
    pa.xh = m->wsXh.get(); pa.xl = m->wsXl.get(); pa.a2 = m->wsA2.get(); pa.joints_out = joints_out;
    pa.a2_stream_order = m->lbs.streams() ? 1 : 0;
    pa.x_fp8 = m->lbs.pose_fp8 ? 1 : 0;
    const VertexSet* const sets[] = {&m->mesh, &m->extra, &m->lmk.verts};                 // by LbsPass::Set
    float* const bufs[] = {vertices_out, joints_out, m->lmk.ws.get()};                    // by LbsPass::Buf
    for (int i = 0; i < plan.num_passes; ++i) {
        const k2b::LbsPass& p = plan.pass[i];
        float* const buf = bufs[p.buf];
        switch (p.kind) {
            case k2b::LbsPass::pose_setup: HIP_TRY(k2b::launch_pose_setup(pa, m->lbs.pose_capacity, stream)); break;
            case k2b::LbsPass::skin: HIP_TRY(launch_skin(m, pa, *sets[p.set], p, buf, stream)); break;
            case k2b::LbsPass::gather:       // only when an output joint's vertex cannot ride in the W image
                HIP_TRY(k2b::launch_gather_joints(buf, m->extra_ids.get(), joints_out, B, p.stride, m->J, m->E, pa.num_out_joints, stream));
                break;
            case k2b::LbsPass::landmarks:    // a stream-ordered pass over this call's vertices, or over the 3L skinned alone (ids: their sequence)
                HIP_TRY(k2b::launch_landmarks(buf, p.stride, (p.set == k2b::LbsPass::mesh ? m->lmk.ids : m->lmk.seq).get(), m->lmk.w.get(), joints_out,
                                              pa.num_out_joints, m->J + m->E, B, L, stream));
                break;
        }
    }
    return K2B_OK;
}

int k2b_vertex_term(const k2b_model* model_c, int32_t B, int32_t E_sel, const int32_t* extra_index, const float* targets,
                    const float* conf, float sigma, float joint_loss_weight, const float* go, const float* bp, const float* be,
                    const float* tr, float* loss_out, float* grad_out, void* stream_v) {
    k2b_model* m = const_cast<k2b_model*>(model_c);
    if (!m) return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_vertex_term: model is NULL");
    if (B < 0 || E_sel < 0) return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_vertex_term: negative size");
    if (B == 0 || E_sel == 0) return K2B_OK;
    if (m->J > 64 || m->NB > 32) return fail(K2B_ERR_UNSUPPORTED, "k2b_vertex_term: %d joints / %d shape coefficients, at most 64 / 32", m->J, m->NB);
    if (E_sel > 32) return fail(K2B_ERR_UNSUPPORTED, "k2b_vertex_term: %d vertex-selected joints, at most 32 per call", E_sel);
    if (!extra_index || !targets || !go || !bp || !be || !tr || !loss_out || !grad_out)
        return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_vertex_term: NULL buffer");
    for (int e = 0; e < E_sel; ++e)
        if (extra_index[e] < 0 || extra_index[e] >= m->E)
            return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_vertex_term: extra_index[%d]=%d outside [0,%d)", e, extra_index[e], m->E);
    hipStream_t stream = (hipStream_t)stream_v;
    k2b::VertexTermArgs a{};
    a.v_template = m->v_template.get(); a.shapedirs = m->shapedirs.get(); a.posedirs = m->posedirs.get(); a.lbs_weights = m->lbs_weights.get();
    a.j_template = m->j_template.get(); a.j_dirs = m->j_dirs.get(); a.parents = m->parents.get(); a.extra_ids = m->extra_ids.get();
    a.num_vertices = m->V; a.num_betas = m->NB; a.num_joints = m->J;
    a.num_frames = B; a.num_sel = E_sel; a.targets = targets; a.conf = conf;
    for (int e = 0; e < E_sel; ++e) { a.sel[e] = extra_index[e]; a.sel_k[e] = e; }
    a.num_targets = E_sel;
    a.sigma = sigma; a.joint_w = joint_loss_weight;
    a.go = go; a.bp = bp; a.be = be; a.tr = tr; a.loss_out = loss_out; a.grad_out = grad_out;
    HIP_TRY(k2b::launch_vertex_term(a, stream));
    return K2B_OK;
}

// k2b_surface_term (focal = null) and k2b_surface_term_image
static int surface_term(const char* who, const k2b_model* model_c, int32_t B, int32_t T, const int32_t* model_joint_index,
                        const float* targets, const float* conf, int32_t conf_per_frame, float sigma, float joint_loss_weight,
                        const float* focal, const float* go, const float* bp, const float* be, const float* tr, float* loss_out,
                        float* grad_out, void* stream_v) {
    k2b_model* m = const_cast<k2b_model*>(model_c);
    if (!m) return fail(K2B_ERR_INVALID_ARGUMENT, "%s: model is NULL", who);
    if (B < 0 || T < 0) return fail(K2B_ERR_INVALID_ARGUMENT, "%s: negative size", who);
    if (focal)
        if (const int rc = k2b::host::check_focal(who, focal); rc != K2B_OK) return rc;
    if (B == 0 || T == 0) return K2B_OK;
    if (T > k2b::kSurfMaxTargets) return fail(K2B_ERR_UNSUPPORTED, "%s: %d targets, at most %d per call", who, T, k2b::kSurfMaxTargets);
    if (!model_joint_index || !targets || !go || !bp || !be || !tr || !loss_out || !grad_out)
        return fail(K2B_ERR_INVALID_ARGUMENT, "%s: NULL buffer", who);
    std::vector<int> sel(T), col(T);
    for (int t = 0; t < T; ++t) {
        const int j = model_joint_index[t];
        if (j < m->J || j >= m->J + m->E + m->lmk.L)
            return fail(K2B_ERR_INVALID_ARGUMENT, "%s: model_joint_index[%d]=%d outside [%d,%d)", who, t, j, m->J, m->J + m->E + m->lmk.L);
        sel[t] = j;
        col[t] = t;
    }
    hipStream_t stream = (hipStream_t)stream_v;
    k2b::SurfaceTermArgs a{};
    if (const int rc = surface_table(m, sel, col, stream, &a); rc != K2B_OK) return rc;
    a.num_frames = B; a.num_targets = T; a.targets = targets; a.conf = conf; a.conf_per_frame = conf_per_frame ? 1 : 0;
    a.sigma = sigma; a.joint_w = joint_loss_weight;
    if (focal) { a.projection = 1; a.focal_x = focal[0]; a.focal_y = focal[1]; }
    a.go = go; a.bp = bp; a.be = be; a.tr = tr; a.loss_out = loss_out; a.grad_out = grad_out;
    HIP_TRY(k2b::launch_surface_term(a, stream));
    return K2B_OK;
}

int k2b_surface_term(const k2b_model* model, int32_t B, int32_t T, const int32_t* model_joint_index, const float* targets,
                     const float* conf, int32_t conf_per_frame, float sigma, float joint_loss_weight, const float* go, const float* bp,
                     const float* be, const float* tr, float* loss_out, float* grad_out, void* stream) {
    return surface_term("k2b_surface_term", model, B, T, model_joint_index, targets, conf, conf_per_frame, sigma, joint_loss_weight, nullptr,
                        go, bp, be, tr, loss_out, grad_out, stream);
}

int k2b_surface_term_image(const k2b_model* model, int32_t B, int32_t T, const int32_t* model_joint_index, const float* targets,
                           const float* conf, int32_t conf_per_frame, float sigma, float joint_loss_weight, const float focal[2],
                           const float* go, const float* bp, const float* be, const float* tr, float* loss_out, float* grad_out,
                           void* stream) {
    if (!focal) return k2b::host::fail(K2B_ERR_INVALID_ARGUMENT, "k2b_surface_term_image: focal is NULL");
    return surface_term("k2b_surface_term_image", model, B, T, model_joint_index, targets, conf, conf_per_frame, sigma, joint_loss_weight,
                        focal, go, bp, be, tr, loss_out, grad_out, stream);
}

int k2b_adam_step(int64_t n, float* params, const float* grad, float* mbuf, float* vbuf, int32_t step, double step_size,
                  double beta1, double beta2, double eps, void* stream_v) {
    if (n < 0 || step < 1) return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_adam_step: n=%lld step=%d", (long long)n, step);
    if (!k2b::host::adam_eps_ok(eps)) return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_adam_step: eps=%g must round to a normal positive float32", eps);
    if (n == 0) return K2B_OK;
    if (!params || !grad || !mbuf || !vbuf) return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_adam_step: NULL buffer");
    const double bc1 = 1.0 - std::pow(beta1, (double)step), bc2 = 1.0 - std::pow(beta2, (double)step);
    HIP_TRY(k2b::launch_adam(params, grad, mbuf, vbuf, (long long)n, (float)(step_size / bc1), (float)std::sqrt(bc2),
                             (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps, (hipStream_t)stream_v));
    return K2B_OK;
}

int k2b_angular_error_deg(int64_t n, const float* pred_rotvec, const float* gt_rotvec, float* err_deg_out, void* stream_v) {
    if (n < 0) return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_angular_error_deg: n=%lld must be >= 0", (long long)n);
    if (n == 0) return K2B_OK;
    if (!pred_rotvec || !gt_rotvec || !err_deg_out) return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_angular_error_deg: NULL buffer");
    if (n > (int64_t)0x7fffffff * 256) return fail(K2B_ERR_UNSUPPORTED, "k2b_angular_error_deg: n=%lld exceeds one launch", (long long)n);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(K2B_ERR_NO_DEVICE, "k2b_angular_error_deg: no HIP device visible (this engine has no CPU path)");
    HIP_TRY(k2b::launch_angular_error(pred_rotvec, gt_rotvec, err_deg_out, (long long)n, (hipStream_t)stream_v));
    return K2B_OK;
}

int k2b_point_error(int32_t B, int32_t N, const float* pred, const float* gt, const float* weights, int32_t weights_per_frame,
                    int32_t align_mode, float* err_out, float* per_point_out, float* transform_out, void* stream_v) {
    if (N < 1) return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_point_error: num_points=%d must be >= 1", N);
    if (B < 0) return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_point_error: num_frames=%d must be >= 0", B);
    if (align_mode < 0 || align_mode > 3)
        return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_point_error: align_mode=%d, expected 0 (none), 1 (translation), 2 (rigid) or 3 (similarity)", align_mode);
    if (B == 0) return K2B_OK;
    if (!pred || !gt || !err_out) return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_point_error: NULL buffer (pred, gt and err_out are required)");
    if (N > k2b::kPointErrorMaxPoints)
        return fail(K2B_ERR_UNSUPPORTED, "k2b_point_error: num_points=%d, at most %d", N, k2b::kPointErrorMaxPoints);
    if (k2b::point_error_workgroups(B, N) > k2b::kPointErrorMaxWorkgroups)
        return fail(K2B_ERR_UNSUPPORTED, "k2b_point_error: num_frames=%d with num_points=%d exceeds one launch (%lld workgroups, at most %lld)", B, N,
                    k2b::point_error_workgroups(B, N), k2b::kPointErrorMaxWorkgroups);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(K2B_ERR_NO_DEVICE, "k2b_point_error: no HIP device visible (this engine has no CPU path)");
    k2b::PointErrorArgs a{};
    a.pred = pred; a.gt = gt; a.weights = weights; a.weights_per_frame = weights_per_frame ? 1 : 0; a.align_mode = align_mode;
    a.num_frames = B; a.num_points = N; a.err = err_out; a.per_point = per_point_out; a.transform = transform_out;
    HIP_TRY(k2b::launch_point_error(a, (hipStream_t)stream_v));
    return K2B_OK;
}

// ---- IK-GAT regressor (k2b_ikgat.hip; the set-up is k2b_ikgat_plan.h) ----
int k2b_ikgat_create(k2b_ikgat** out, int32_t J, int32_t IN, int32_t H, int32_t L, int32_t NH, const int32_t* parents,
                     const float* weights, int64_t num_weights) {
    if (out) *out = nullptr;
    const k2b::IkgatDims dims{J, IN, H, L, NH};
    k2b::IkgatVerdict v;
    if (k2b::ikgat_create_rules(out != nullptr, dims, parents, weights != nullptr, num_weights, v) != K2B_OK) return fail(v.code, "%s", v.message);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(K2B_ERR_NO_DEVICE, "k2b_ikgat_create: no HIP device visible (this engine has no CPU path)");
    const std::vector<int> csr = k2b::ikgat_csr(J, parents);
    std::unique_ptr<k2b_ikgat> n(new k2b_ikgat);              // released with its buffers if an upload fails
    n->plan = k2b::ikgat_plan(dims, csr[J]);
    const std::vector<float> image = k2b::ikgat_pack(n->plan, weights);
    hipError_t e = n->w.upload(image.data(), image.size());
    if (e == hipSuccess) e = n->csr.upload(csr.data(), csr.size());
    if (e != hipSuccess) return fail(K2B_ERR_HIP, "k2b_ikgat_create: upload failed: %s", hipGetErrorString(e));
    *out = n.release();
    return K2B_OK;
}

void k2b_ikgat_destroy(k2b_ikgat* n) {
    if (!n) return;
    (void)hipDeviceSynchronize();
    delete n;
}

int k2b_ikgat_predict(const k2b_ikgat* n, int32_t num_frames, const float* positions, const float* quat_in, int32_t chain,
                      float* quat_out, void* stream_v) {
    k2b::IkgatVerdict v;
    if (k2b::ikgat_predict_rules(n ? &n->plan : nullptr, num_frames, positions != nullptr, quat_in != nullptr, quat_out != nullptr, v) != K2B_OK)
        return fail(v.code, "%s", v.message);
    if (v.nothing) return K2B_OK;
    const k2b::IkgatPlan& p = n->plan;
    const k2b::IkgatLaunch launch = k2b::ikgat_launch(p, num_frames, chain != 0);
    k2b::IkgatArgs a{};
    a.w = n->w.get(); a.csr = n->csr.get(); a.pos = positions; a.quat_in = p.IN == 9 ? quat_in : nullptr; a.quat_out = quat_out;
    a.B = num_frames; a.J = p.J; a.H = p.H; a.heads = p.NH; a.L = p.L; a.in = p.IN; a.KC = p.KC; a.ldx = p.LDX; a.nedges = p.nedges;
    a.chain = chain ? 1 : 0;
    a.F = launch.F;
    HIP_TRY(k2b::launch_ikgat(a, launch, (hipStream_t)stream_v));
    return K2B_OK;
}

}  // extern "C"
