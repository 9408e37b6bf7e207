// k2b_host.h — private to the host units of the C ABI (k2b_api_*.hip): the handle types behind include/k2b.h, error
// reporting, owning device buffers and what the units call in one another.  Nothing here reaches a kernel: kernel argument
// structs (k2b_internal.h) keep raw pointers, filled with .get().
#pragma once
#include <cstdint>
#include <map>
#include <mutex>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "../../include/k2b.h"
#include "k2b_fit_rules.h"
#include "k2b_internal.h"
#include "k2b_model_tables.h"

namespace k2b {
namespace host __attribute__((visibility("hidden"))) {

// records the calling thread's message for k2b_last_error() and returns `code` (k2b_api_misc.hip)
int fail(int code, const char* fmt, ...);
int device_cus();                        // CUs of the calling thread's current device (cached per device ordinal)

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e__ = (expr);                                                               \
        if (e__ != hipSuccess)                                                                 \
            return ::k2b::host::fail(K2B_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
    } while (0)
// for calls queued between other launches: clears the sticky error and reports a fixed message ("who: text")
#define HIP_TRY_MSG(expr, ...)                                                                 \
    do {                                                                                       \
        if ((expr) != hipSuccess) {                                                            \
            (void)hipGetLastError();                                                           \
            return ::k2b::host::fail(K2B_ERR_HIP, __VA_ARGS__);                                \
        }                                                                                      \
    } while (0)

// Owning device pointer: hipFree in the destructor, move-only.
template <class T>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p_, o.p_); return *this; }   // (o releases what this held)
    ~DevBuf() { (void)reset(); }
    T* get() const { return p_; }
    hipError_t reset() {
        const hipError_t e = p_ ? hipFree(p_) : hipSuccess;
        p_ = nullptr;
        return e;
    }
    // n elements (at least one is allocated); what the buffer held is released first
    hipError_t alloc(size_t n) {
        (void)reset();
        return hipMalloc(reinterpret_cast<void**>(&p_), (n ? n : 1) * sizeof(T));
    }
    hipError_t upload(const T* src, size_t n) {
        hipError_t e = alloc(n);
        if (e == hipSuccess && n) e = hipMemcpy(p_, src, n * sizeof(T), hipMemcpyHostToDevice);
        return e;
    }

private:
    T* p_ = nullptr;
};

// Stream-ordered scratch of one call: hipMallocAsync on the stream, hipFreeAsync behind whatever the call queued.
class StreamWorkspace {
public:
    explicit StreamWorkspace(hipStream_t stream) : stream_(stream) {}
    StreamWorkspace(const StreamWorkspace&) = delete;
    ~StreamWorkspace() { if (p_) (void)hipFreeAsync(p_, stream_); }
    hipError_t alloc(size_t bytes) { return hipMallocAsync(reinterpret_cast<void**>(&p_), bytes, stream_); }
    unsigned char* get() const { return p_; }

private:
    hipStream_t stream_;
    unsigned char* p_ = nullptr;
};

// The least recently used entry of a cache (values with `dev` and `last_use`) leaves.  The caller has waited for every launch
// that may still read it.
template <class Map>
hipError_t evict_lru(Map& cache) {
    auto victim = cache.begin();
    for (auto it = cache.begin(); it != cache.end(); ++it)
        if (it->second.last_use < victim->second.last_use) victim = it;
    const hipError_t e = victim->second.dev.reset();
    cache.erase(victim);
    return e;
}

// LBS B operands of a vertex set (f16 hi/lo, MFMA fragment order)
struct VertexSet {
    DevBuf<k2b_half> pdh, pdl;
    DevBuf<k2b_half> w2;                     // W in the tile kernel's group layout (k2b_internal.h, TileArgs)
    DevBuf<k2b_half> spd, sw;                // stream kernel's Pd / W (k2b_internal.h, StreamArgs), or null
    int v_tiles = 0, num = 0, nv16 = 0;
    int pd8_lo_exp = 0, pd8_hi_exp = 0;      // scales of spd's e4m3 strips (LbsRouteRecord::pose_fp8; k2b_model_tables.h, pose_fp8_strips)
};

}  // namespace host
}  // namespace k2b

struct __attribute__((visibility("hidden"))) k2b_model {
    template <class T> using DevBuf = k2b::host::DevBuf<T>;
    using VertexSet = k2b::host::VertexSet;
    int V = 0, J = 0, NB = 0, E = 0, P = 0;
    DevBuf<float> v_template, shapedirs, posedirs, j_regressor, lbs_weights;
    DevBuf<int> parents, extra_ids;
    DevBuf<float> j_template, j_dirs;                        // device
    DevBuf<float> j_basis_lane;                              // device: [3][1 + NB][64 lanes] = template | directions, lane = joint (pose set-up)
    std::vector<float> h_j_template, h_j_dirs;               // host copies
    // fused-fit tables (J == 24 only)
    bool fit_ok = false;
    bool fit_scan64 = false;                                 // lanes in DFS order and fp64 subtree scans (no scan plan, or K2B_FIT_SCAN64)
    std::string fit_why;
    DevBuf<float> dt, dd;
    DevBuf<int> tree;
    k2b::Tree kin;                                           // the kinematic tree (k2b_tree.h): DFS order, depth of every joint
    VertexSet mesh, extra;                                   // the whole mesh and the E extra-joint vertices
    bool joints_in_mesh = false;                             // every extra joint's vertex is tagged in mesh.w2 (no gather launch)
    k2b::LbsRouteRecord lbs;                                 // which kernel skins this model, GA, k-steps, W fragments, pose capacity (k2b_lbs_plan.h, lbs_route)
    // tables of the tree fit kernel (any J <= 64), lane order = DFS pre-order (lane of joint j: kin.pos[j])
    DevBuf<float> tt_dt, tt_dd;
    DevBuf<int> tt_anc;
    std::vector<int> h_tt_tab;                               // host: the [64][8] lane table with empty prior columns
    std::map<int, DevBuf<int>> tt_tabs;                      // the lane table per prior width, built on first use, never written after its upload (guarded by mu)
    DevBuf<k2b::k2b_half> wsA2;                              // per-frame A operand of the tile kernel
    DevBuf<float> dump;                                      // 64 x 3 floats: store target of lanes outside the batch
    // LBS per-frame operand workspace (grow-only)
    DevBuf<k2b::k2b_half> wsXh, wsXl;
    int ws_bpad = 0;
    // Adam coefficient tables, one per (iters, lr, b1, b2); at most kMaxAdamTables, least recently used evicted
    struct AdamTable { DevBuf<float2> dev; uint64_t last_use; };
    std::map<std::tuple<int, double, double, double>, AdamTable> adam_tables;
    uint64_t adam_clock = 0;
    std::vector<int> h_extra_ids;                            // host copy of extra_vertex_ids
    // landmarks (k2b_model_set_landmarks): output joint J + E + l = sum_k w[l][k] v[ids[l][k]]
    struct Landmarks {
        int L = 0;
        std::vector<int> h_ids;
        std::vector<float> h_w;
        DevBuf<int> ids, seq;                                // device [L][3]; seq[l][k] = 3 l + k (rows of the set below)
        DevBuf<float> w;                                     // device [L][3]
        VertexSet verts;                                     // LBS operands of the 3L landmark vertices (joints-only forward)
        DevBuf<float> ws;                                    // LBS workspace (grow-only, with wsXh ...): the 3L vertices of a
        int ws_bpad = 0;                                     // joints-only call, [ws_bpad][3L][3]
    } lmk;
    bool lmk_set = false;
    // compact tables of the surface-point term (k2b_surface.hip), one per selection of (model index, target column) pairs;
    // at most kMaxSurfaceTables, least recently used evicted
    struct SurfaceTable {
        DevBuf<unsigned char> dev;
        k2b::SurfaceTermArgs a{};                            // table pointers and sizes filled, call fields not
        uint64_t last_use = 0;
    };
    std::map<std::vector<int>, SurfaceTable> surface_tables;
    uint64_t surface_clock = 0;
    // k2b_lbs_backward (k2b_lbs_backward.hip): the rows of grad_joints that are vertices, sorted by vertex, built on first use.
    // One int image (offsets o_*): vertex list [U] | rows [n] | positions in the mesh [n] | positions in the list [n] | item
    // offsets per chunk of the mesh | per chunk of the list
    struct LbsBackward : k2b::tables::BackwardOffsets {
        bool built = false;
        int L = 0;                                           // landmarks the table was built with
        DevBuf<int> ints;
        DevBuf<float> w;                                     // [n] weight of every item
    } bwd;
    std::mutex mu;
};

struct __attribute__((visibility("hidden"))) k2b_prior {
    template <class T> using DevBuf = k2b::host::DevBuf<T>;
    int M = 0, D = 0;
    DevBuf<float> pa_image, row_const, nlw;
    DevBuf<k2b::k2b_half> frag32;
    float inv_scale[k2b::kPriorMaxGauss] = {};
    // host copies (symmetrised precisions in double, means, nll weights) and the mixture folded to its first Dv
    // dimensions for the tree fit kernel, built on first use per Dv
    std::vector<double> Ps, mu;
    std::vector<float> nllw;
    struct Folded { DevBuf<float> pA, ph, pb, pmu, pcl; };
    std::map<int, Folded> folded;
    std::mutex mu_lock;
};

struct __attribute__((visibility("hidden"))) k2b_ikgat {
    k2b::IkgatPlan plan{};                   // (k2b_ikgat_plan.h)
    k2b::host::DevBuf<float> w;
    k2b::host::DevBuf<int> csr;
};

namespace k2b {
namespace host __attribute__((visibility("hidden"))) {

// ---- k2b_api_model.hip, k2b_api_prior.hip: per-handle tables built on first use ----------------------------------------------
int adam_table(k2b_model* model, const k2b_fit_config* cfg, hipStream_t stream, float2** out);
int folded_prior(k2b_prior* p, int Dv, const k2b_prior::Folded** out);
int surface_table(k2b_model* m, const std::vector<int>& sel, const std::vector<int>& col, hipStream_t stream, SurfaceTermArgs* out);
int tree_lane_table(k2b_model* m, int prior_dims, const int** out);
int reserve_lbs_workspace(k2b_model* m, int bpad);           // caller holds m->mu
int lbs_backward_tables(k2b_model* m);                       // caller holds m->mu (k2b_lbs_backward.hip)

// ---- k2b_api_fit.hip: one description of a fit call --------------------------------------------------------------------------
struct ConstParams { const float *go = nullptr, *bp = nullptr, *be = nullptr, *tr = nullptr; };
struct Params {
    float *go = nullptr, *bp = nullptr, *be = nullptr, *tr = nullptr;
    ConstParams as_const() const { return {go, bp, be, tr}; }
};
struct FitCall {
    int32_t B = 0, K = 0;                    // frames (in a chain: sequences or slots), targets
    const int32_t* model_joint_index = nullptr;
    const float *j3d = nullptr, *conf = nullptr;
    ConstParams in;
    Params out;
    const float *preserve = nullptr, *tr_prior = nullptr;
    float *loss_out = nullptr, *grad_out = nullptr;
    hipStream_t stream = nullptr;
    // warm-start chain (len > 1): frames per sequence, follow-up iterations, ragged slot table (FitArgs::chain_meta);
    // freeze_shape (k2b_fit_image_sequences, k2b_fit_multiview_sequences): the steps > 0 hold the shape (FitArgs::chain_freeze_shape);
    // frames: the frames of all sequences of a ragged chain (launch_fit_world's bound on the views' target rows)
    struct Chain { int len = 1, iters = 0; const int* meta = nullptr; bool freeze_shape = false; long long frames = 0; } chain;
    // the L-BFGS step inside the fused launch (FitArgs::lb_mode, lbv, lb_chain_max_iter)
    struct Lbfgs { int mode = LbMode::none; const LbfgsArgs* args = nullptr; int chain_max_iter = 0; } lbfgs;
    // k2b_fit_multiview, k2b_fit_multiview_sequences: the joint term summed over num_views calibrated cameras (HOST table; targets
    // [B][views][K][3], conf [views][K] or [B][views][K], B the frames of all sequences in a chain); cfg->focal is not read then
    int num_views = 0;
    const k2b_camera* cameras = nullptr;
};
// what every entry knows of its call; the optional arrays, the chain and the views are set by name
inline FitCall fit_call(int32_t B, int32_t K, const int32_t* model_joint_index, const float* j3d, const float* conf, const ConstParams& in,
                        const Params& out, float* loss_out, void* stream) {
    FitCall c;
    c.B = B; c.K = K; c.model_joint_index = model_joint_index; c.j3d = j3d; c.conf = conf; c.in = in; c.out = out; c.loss_out = loss_out;
    c.stream = (hipStream_t)stream;
    return c;
}

// ---- what a call is refused for: k2b_fit_rules.h, asked once by every fit entry before anything is allocated, built or queued -----
using rules::adam_eps_ok;
inline rules::Facts fit_facts(const k2b_model* m, const k2b_prior* p) {
    return {m->J, m->E, m->lmk.L, m->NB, m->fit_ok, m->fit_scan64, m->kin.depth.data(), p->D, p->M};
}
// the call of `entry` as the rules see it: the handles' facts go to *facts (absent handles: no facts), what the entry alone
// knows (chain, ragged table, L-BFGS numbers) is set by name
inline rules::Call rule_call(rules::Entry entry, const k2b_model* m, const k2b_prior* p, const k2b_fit_config* cfg, const FitCall& c,
                             rules::Facts* facts) {
    rules::Call r;
    r.entry = entry; r.cfg = cfg;
    if (m && p) { *facts = fit_facts(m, p); r.facts = facts; }
    r.B = c.B; r.K = c.K; r.index = c.model_joint_index;
    r.targets_null = !c.j3d;
    r.params_null = !c.in.go || !c.in.bp || !c.in.be || !c.in.tr || !c.out.go || !c.out.bp || !c.out.be || !c.out.tr;
    r.preserve = c.preserve != nullptr; r.tr_prior = c.tr_prior != nullptr; r.grad_out = c.grad_out != nullptr;
    r.num_views = c.num_views; r.cameras = c.cameras;
    return r;
}
// K2B_OK with *go saying whether there is anything to fit, or the refusal recorded for k2b_last_error()
inline int judge(const rules::Call& r, bool* go) {
    rules::Verdict v;
    if (rules::judge(r, v) != K2B_OK) return fail(v.code, "%s", v.message);
    *go = !v.nothing;
    return K2B_OK;
}
inline int check_focal(const char* who, const float* focal) {      // (the term entries of k2b_api_misc.hip)
    rules::Verdict v;
    return rules::check_focal(who, focal, v) != K2B_OK ? fail(v.code, "%s", v.message) : K2B_OK;
}

// The shared set-up of a call that the rules have accepted: the fused kernel or the tree kernel, surface targets, the launches.
int fit_world_impl(const k2b_model* model, const k2b_prior* prior, const k2b_fit_config* cfg, const FitCall& call);
// The in-place start of a fit that steps in the output arrays: the defaults of the preserve pose and of the translation prior's
// centre are the INITIAL parameters, so they go to scratch (`pres` [B][D], `trp` [B][3]) first; then the start goes into the
// outputs where the two differ.
hipError_t start_in_place(int B, int D, int NB, const ConstParams& in, const Params& out, const float* preserve, const float* tr_prior,
                          float* pres, float* trp, hipStream_t stream);
// Ragged sequences of the k2b_fit_sequences* entries: the chain slots (rules::ragged_order) go up to the device.
int upload_slots(const std::vector<int>& meta, int* dev, hipStream_t stream);

}  // namespace host
}  // namespace k2b
