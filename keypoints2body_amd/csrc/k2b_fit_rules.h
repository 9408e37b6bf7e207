// k2b_fit_rules.h — what each of the eleven fit entries of the C ABI (include/k2b.h) refuses, as pure functions: given who is calling
// and what they pass, is the call accepted, and if not, with which code and which message.  The ONE statement of those rules
// (DESIGN.md 4.9): every entry fills the facts of its handles and the description of its call, asks judge() once, before anything
// is allocated, built or queued, and hands a refusal to fail(); the set-up behind it (k2b_api_fit.hip, k2b_api_lbfgs.hip) checks
// nothing again.  tests/host/fit_rules_check.cpp holds the rules to the refusals recorded from the entries before this header
// existed (tests/golden/fit_refusals.json) and to a table of what is built written out independently, without a GPU.
//
// The order of the checks of an entry is part of its contract: callers and tests match the text of the refusal that wins when a
// call is wrong in several ways.  Each entry's function below reads top to bottom in that order.  The entry's identity decides
// which refusals a call can get: the shared path (shared_path, the checks k2b_fit_world has always made, under its name) asks
// `entry` where it once was told by flags what its caller had already let through.
// No HIP runtime: a plain host C++17 program may include this header alone.
#pragma once
#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/k2b.h"
#include "k2b_lbfgs_plan.h"   // kLbfgsMaxHistory, lbfgs_followup_closures (and k2b_launch_plan.h: ForceShape; k2b_layout.h: kSurfMaxTargets, kMaxViews)
#include "k2b_tree.h"         // rounds_for_depth

namespace k2b {
namespace rules {

enum class Entry {
    fit_world, fit_sequence, fit_sequences, fit_image, fit_image_sequences, fit_multiview,
    fit_world_lbfgs, fit_sequence_lbfgs, fit_sequences_lbfgs, shape_pass_lbfgs,
    fit_multiview_sequences      // (appended: the values of the first ten are recorded in tests and golden files)
};
constexpr int kNumEntries = 11;
constexpr const char* entry_name(Entry e) {
    constexpr const char* names[kNumEntries] = {"k2b_fit_world", "k2b_fit_sequence", "k2b_fit_sequences", "k2b_fit_image", "k2b_fit_image_sequences",
                                                "k2b_fit_multiview", "k2b_fit_world_lbfgs", "k2b_fit_sequence_lbfgs", "k2b_fit_sequences_lbfgs",
                                                "k2b_shape_pass_lbfgs", "k2b_fit_multiview_sequences"};
    return names[(int)e];
}
constexpr bool is_lbfgs(Entry e) {
    return e == Entry::fit_world_lbfgs || e == Entry::fit_sequence_lbfgs || e == Entry::fit_sequences_lbfgs || e == Entry::shape_pass_lbfgs;
}
constexpr bool is_multiview(Entry e) { return e == Entry::fit_multiview || e == Entry::fit_multiview_sequences; }

// What the rules read from the two handles.  (k2b_host.h fills it from k2b_model and k2b_prior.)
struct Facts {
    int J, E, L, NB;               // kinematic joints, vertex-selected joints, landmarks, shape coefficients
    bool fit_ok, fit_scan64;       // the fused 24-lane kernel takes the model; its lanes are in DFS order with fp64 scans
    const int* depth;              // [J] levels below the root
    int D, M;                      // the prior: dimensions, components
};

// Whether the fused 24-lane kernel takes calls of (model, prior, cfg), and the prior width the call means.  k2b_fit.hip relies on
// `fused` having been checked here.
struct FusedEligibility { int prior_dims; bool fused; };
inline FusedEligibility fused_eligibility(const Facts& f, const k2b_fit_config& cfg) {
    const int pose_dims_all = 3 * (f.J - 1);
    const int prior_dims = cfg.prior_pose_dims > 0 ? cfg.prior_pose_dims : (f.D < pose_dims_all ? f.D : pose_dims_all);
    const bool fused = f.fit_ok && f.D == pose_dims_all && prior_dims == pose_dims_all && (cfg.num_betas_prior == 0 || cfg.num_betas_prior == f.NB);
    return {prior_dims, fused};
}

// The call as the rules see it.  Fields an entry does not have keep their defaults.
struct Call {
    Entry entry = Entry::fit_world;
    const Facts* facts = nullptr;             // null: the model or the prior handle is absent
    const k2b_fit_config* cfg = nullptr;
    int B = 0, K = 0;                         // frames (k2b_fit_sequence: sequences; k2b_fit_sequence_lbfgs: frames of the one sequence), targets
    const int32_t* index = nullptr;           // model_joint_index [K]
    bool targets_null = false;                // the target array is NULL (shape pass: one of the per-frame arrays, with frames to read)
    bool params_null = false;                 // one of the eight parameter arrays is NULL (shape pass: seq_offsets or a betas array)
    bool preserve = false, tr_prior = false, grad_out = false;      // the optional arrays that were given
    int frames_per_sequence = 1;              // k2b_fit_sequence
    int followup_iters = 0;                   // the chain entries
    int num_sequences = 0;                    // the ragged entries and the shape pass
    const int32_t *lengths = nullptr, *offsets = nullptr;
    int max_iter = 0, history_size = 0;       // the L-BFGS entries (max_iter: first_iters in a chain)
    double lr = 0.0;
    int num_views = 0;                        // k2b_fit_multiview, k2b_fit_multiview_sequences
    const k2b_camera* cameras = nullptr;
    int num_frames = 0, root_joint = 0, num_free_betas = 0;         // the shape pass
};

struct Verdict {
    int code = K2B_OK;
    bool nothing = false;                     // accepted, and there is nothing to fit: the entry returns K2B_OK at once
    char message[512] = "";
    int refuse(int c, const char* fmt, ...) __attribute__((format(printf, 3, 4))) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(message, sizeof message, fmt, ap);
        va_end(ap);
        return code = c;
    }
    int accept_nothing() { nothing = true; return code = K2B_OK; }
};

// ---- ragged sequences: the chain slots in launch order (the sequences with frames, longest first, ties in the caller's order) -----
struct RaggedSlots {
    std::vector<int> meta;                    // [slot][4] = {sequence (row of its start parameters), first frame row, frames, 0}
    int slots = 0, max_len = 0;
};
inline RaggedSlots ragged_order(int32_t S, const int32_t* lengths, const int32_t* offsets) {      // (of a table check_ragged accepts)
    std::vector<int> order;
    for (int s = 0; s < S; ++s)
        if (lengths[s] > 0) order.push_back(s);
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return lengths[x] > lengths[y]; });
    RaggedSlots r;
    r.slots = (int)order.size();
    r.max_len = r.slots ? lengths[order[0]] : 0;
    r.meta.assign((size_t)r.slots * 4, 0);
    for (int i = 0; i < r.slots; ++i) {
        r.meta[(size_t)i * 4 + 0] = order[i];
        r.meta[(size_t)i * 4 + 1] = offsets[order[i]];
        r.meta[(size_t)i * 4 + 2] = lengths[order[i]];
    }
    return r;
}
// (also k2b_sequence_order's check, under its name)
inline int check_ragged(const char* who, int32_t S, const int32_t* lengths, const int32_t* offsets, Verdict& v) {
    if (S < 0) return v.refuse(K2B_ERR_INVALID_ARGUMENT, "%s: num_sequences=%d", who, S);
    if (S > 0 && (!lengths || !offsets)) return v.refuse(K2B_ERR_INVALID_ARGUMENT, "%s: lengths and offsets are required", who);
    int64_t next = 0;
    for (int s = 0; s < S; ++s) {
        if (lengths[s] < 0) return v.refuse(K2B_ERR_INVALID_ARGUMENT, "%s: lengths[%d]=%d", who, s, lengths[s]);
        if (offsets[s] != next)
            return v.refuse(K2B_ERR_INVALID_ARGUMENT, "%s: offsets[%d]=%d, expected %lld (the exclusive prefix sum of lengths)", who, s, offsets[s],
                            (long long)next);
        next += lengths[s];
        if (next > ((int64_t)1 << 30)) return v.refuse(K2B_ERR_INVALID_ARGUMENT, "%s: more than 2^30 frames", who);
    }
    return K2B_OK;
}

// ---- the checks several entries make, each under the name of the entry that makes it --------------------------------------------
inline bool iters_ok(int n, int most) { return n >= 1 && n <= most; }
constexpr int kMaxAdamIters = 1 << 20, kMaxLbfgsIters = 10000;

// Adam's eps as the kernels see it: its float32 rounding must be a normal positive number (k2b.h, k2b_fit_config).  With 0, a
// negative value, NaN or a float32 denormal (flushed to 0) the update of a parameter with gradient 0 - one outside the
// optimiser, say - is 0 * rcp(0) = NaN.  (NaN fails the first comparison.)
inline bool adam_eps_ok(double eps) {
    const float e = (float)eps;
    return e >= 1.17549435e-38f && e <= 3.402823466e38f;
}
inline bool is_finite(float x) { return x >= -3.402823466e38f && x <= 3.402823466e38f; }      // (NaN fails the first comparison)

inline int check_handles(const char* who, const Call& c, Verdict& v) {
    if (!c.facts || !c.cfg) return v.refuse(K2B_ERR_INVALID_ARGUMENT, "%s: model, prior and cfg are required", who);
    return K2B_OK;
}
// k2b_fit_config::projection is built into k2b_fit_world's Adam loop, k2b_fit_image, k2b_fit_image_sequences' chain,
// k2b_fit_multiview and k2b_fit_multiview_sequences' chain: the other chain entries and the L-BFGS entries refuse it by name
inline int refuse_projection(const char* who, const Call& c, Verdict& v) {
    if (c.cfg && c.cfg->projection != 0)
        return v.refuse(K2B_ERR_UNSUPPORTED, "%s: the projected joint term (projection=%d) is built into k2b_fit_world only", who, c.cfg->projection);
    return K2B_OK;
}
inline int check_focal(const char* who, const float* focal, Verdict& v) {                     // fx, fy: finite and positive
    for (int i = 0; i < 2; ++i)
        if (!(focal[i] > 0.0f) || !(focal[i] <= 3.402823466e38f))                            // (NaN fails the first comparison)
            return v.refuse(K2B_ERR_INVALID_ARGUMENT, "%s: focal[%d]=%g must be finite and positive", who, i, (double)focal[i]);
    return K2B_OK;
}
// the entries of 2D keypoints: projection must be 1, with usable focals (`other`: where 3D targets go)
inline int require_projection(const char* who, const char* other, const Call& c, Verdict& v) {
    if (c.cfg->projection != 1)
        return v.refuse(K2B_ERR_INVALID_ARGUMENT, "%s: projection=%d must be 1 (3D targets: %s)", who, c.cfg->projection, other);
    return K2B_OK;
}
// every model joint index inside the model's outputs (joints, extra joints, landmarks)
inline int check_targets(const char* who, const Call& c, Verdict& v) {
    const Facts& f = *c.facts;
    if (c.K < 1 || !c.index) return v.refuse(K2B_ERR_INVALID_ARGUMENT, "%s: num_targets=%d / model_joint_index", who, c.K);
    for (int k = 0; k < c.K; ++k)
        if (c.index[k] < 0 || c.index[k] >= f.J + f.E + f.L)
            return v.refuse(K2B_ERR_INVALID_ARGUMENT, "%s: model_joint_index[%d]=%d out of range", who, k, c.index[k]);
    return K2B_OK;
}
inline bool kinematic_only(int J, int32_t K, const int32_t* index) {
    for (int k = 0; k < K; ++k)
        if (index[k] < 0 || index[k] >= J) return false;
    return true;
}
// the projected joint term of the fused kernel rides on the fp32 scans
inline int check_scan_plan(const char* who, const Call& c, Verdict& v) {
    if (fused_eligibility(*c.facts, *c.cfg).fused && c.facts->fit_scan64)
        return v.refuse(K2B_ERR_UNSUPPORTED, "%s: the projected joint term is built for the fp32 scans only (this model has no scan plan, or was "
                        "created under K2B_FIT_SCAN64)", who);
    return K2B_OK;
}
// What the L-BFGS entries check alike: the handles, the projection, the iteration count, the history, the step length, the
// model's width, and in a chain the follow-up count.
inline int check_lbfgs(const char* who, const Call& c, bool chain, Verdict& v) {
    if (check_handles(who, c, v)) return v.code;
    if (refuse_projection(who, c, v)) return v.code;
    if (!iters_ok(c.max_iter, kMaxLbfgsIters)) return v.refuse(K2B_ERR_INVALID_ARGUMENT, "%s: max_iter=%d", who, c.max_iter);
    if (c.history_size > kLbfgsMaxHistory)
        return v.refuse(K2B_ERR_UNSUPPORTED, "%s: history_size=%d (at most %d)", who, c.history_size, kLbfgsMaxHistory);
    if (!(c.lr > 0.0)) return v.refuse(K2B_ERR_INVALID_ARGUMENT, "%s: lr must be positive", who);
    const int P = 3 + 3 * (c.facts->J - 1) + c.facts->NB + 3;
    if (P > 256) return v.refuse(K2B_ERR_UNSUPPORTED, "%s: %d parameters per frame (at most 256)", who, P);
    if (chain && !iters_ok(c.followup_iters, kMaxLbfgsIters)) return v.refuse(K2B_ERR_INVALID_ARGUMENT, "%s: followup_iters=%d", who, c.followup_iters);
    return K2B_OK;
}

// ---- the shared path: what k2b_fit_world checks, and every other entry behind its own checks, under k2b_fit_world's name ----------
// The launch as the shared path meets it.  closure: an L-BFGS entry's evaluate-only launches, whose iteration count and step
// length are the entry's own (valid) values, not the configuration's.
struct Shared {
    int B = 0;                                // frames, or chain slots
    int chain_len = 1, chain_iters = 0;       // chain_len > 1: a warm-start chain
    bool closure = false;
    bool preserve = false, tr_prior = false, grad_out = false, buffers_null = false;
};
inline int shared_path(const Call& c, const Shared& s, Verdict& v) {
    if (!c.facts || !c.cfg) return v.refuse(K2B_ERR_INVALID_ARGUMENT, "k2b_fit_world: model, prior and cfg are required");
    const Facts& f = *c.facts;
    const k2b_fit_config& cfg = *c.cfg;
    const bool chain = s.chain_len > 1;
    if (chain && !iters_ok(s.chain_iters, kMaxAdamIters)) return v.refuse(K2B_ERR_INVALID_ARGUMENT, "k2b_fit_sequence: followup_iters=%d", s.chain_iters);
    if (chain && (s.preserve || s.tr_prior || s.grad_out || cfg.transl_prior_weight != 0.0f))
        return v.refuse(K2B_ERR_UNSUPPORTED, "k2b_fit_sequence: no explicit preserve pose, translation prior or gradient output in a chain");
    // k2b_fit_config::projection: its values, and what the projected joint term is not built into.  (The multi-view entries have
    // checked their own form of it - cfg->focal is not read there; the L-BFGS entries have refused it by name.)
    if (!is_multiview(c.entry) && cfg.projection != 0) {
        if (cfg.projection != 1) return v.refuse(K2B_ERR_INVALID_ARGUMENT, "k2b_fit_world: projection=%d must be 0 or 1", cfg.projection);
        if (check_focal("k2b_fit_world", cfg.focal, v)) return v.code;
        if ((chain && c.entry != Entry::fit_image_sequences) || is_lbfgs(c.entry))
            return v.refuse(K2B_ERR_UNSUPPORTED, "k2b_fit_world: the projected joint term is built for independent frames under Adam only");
    }
    // large trees (SMPL-H / SMPL-X), or a prior over a prefix of the body pose: the tree kernel
    const FusedEligibility el = fused_eligibility(f, cfg);
    if (!el.fused) {
        if (el.prior_dims < 3 || el.prior_dims > 64 || el.prior_dims % 3 != 0 || el.prior_dims > f.D || el.prior_dims > 3 * (f.J - 1))
            return v.refuse(K2B_ERR_UNSUPPORTED, "k2b_fit_world: the tree kernel takes a prior over the first 3..63 body-pose dimensions "
                            "(a multiple of 3, at most the mixture's %d), got %d", f.D, el.prior_dims);
        if (cfg.transl_prior_weight != 0.0f || s.tr_prior)
            return v.refuse(K2B_ERR_UNSUPPORTED, "k2b_fit_world: the translation prior (camera-space fitter) is not built for %d-joint models", f.J);
    }
    // the arguments of the call
    if (s.B < 0) return v.refuse(K2B_ERR_INVALID_ARGUMENT, "k2b_fit_world: num_frames=%d", s.B);
    if (c.K < 1 || c.K > f.J + f.E + f.L) return v.refuse(K2B_ERR_INVALID_ARGUMENT, "k2b_fit_world: num_targets=%d out of range", c.K);
    if (!c.index) return v.refuse(K2B_ERR_INVALID_ARGUMENT, "k2b_fit_world: model_joint_index is NULL");
    if (!s.closure && !iters_ok(cfg.num_iters, kMaxAdamIters)) return v.refuse(K2B_ERR_INVALID_ARGUMENT, "k2b_fit_world: num_iters=%d", cfg.num_iters);
    if ((!s.closure && !(cfg.step_size >= 0.0)) || !(cfg.adam_beta1 >= 0.0 && cfg.adam_beta1 < 1.0) || !(cfg.adam_beta2 >= 0.0 && cfg.adam_beta2 < 1.0))
        return v.refuse(K2B_ERR_INVALID_ARGUMENT, "k2b_fit_world: bad Adam hyper-parameters");
    if (!adam_eps_ok(cfg.adam_eps))
        return v.refuse(K2B_ERR_INVALID_ARGUMENT, "k2b_fit_world: adam_eps=%g must round to a normal positive float32", cfg.adam_eps);
    if (s.B == 0) return v.accept_nothing();
    if (s.buffers_null)
        return v.refuse(K2B_ERR_INVALID_ARGUMENT, "k2b_fit_world: NULL parameter / target buffer (init transl is required, world_space.py:118-119)");
    // the targets by kind: kinematic joints (model index < J) are fitted by a lane of the fit kernel, each by one target; surface
    // targets (extra joints, landmarks) by the vertex-term / surface-term kernels
    bool targeted[64] = {};
    int surface = 0, kinematic = 0, max_depth = 0;
    for (int k = 0; k < c.K; ++k) {
        const int j = c.index[k];
        if (j < 0 || j >= f.J + f.E + f.L) return v.refuse(K2B_ERR_INVALID_ARGUMENT, "k2b_fit_world: model_joint_index[%d]=%d out of range", k, j);
        if (j >= f.J) {
            if (surface >= kSurfMaxTargets)
                return v.refuse(K2B_ERR_UNSUPPORTED, "k2b_fit_world: more than %d surface targets (vertex-selected joints and landmarks)", kSurfMaxTargets);
            ++surface;
            continue;
        }
        if (targeted[j]) return v.refuse(K2B_ERR_UNSUPPORTED, "k2b_fit_world: joint %d is targeted twice", j);
        targeted[j] = true;
        ++kinematic;
        max_depth = std::max(max_depth, f.depth[j]);
    }
    // (k2b_fit_image alone fits surface targets under projection: the projected form of k2b_surface.hip)
    if (cfg.projection != 0 && surface > 0 && c.entry != Entry::fit_image)
        return v.refuse(K2B_ERR_UNSUPPORTED, "k2b_fit_world: surface targets (vertex-selected joints, landmarks) keep the 3D term: "
                        "no projection for model indices beyond the kinematic joints");
    const auto check_surface_targets = [&]() -> int {
        if (surface == 0) return K2B_OK;
        if (kinematic == 0)
            return v.refuse(K2B_ERR_UNSUPPORTED, "k2b_fit_world: at least one kinematic joint (model index < %d) must be among the targets", f.J);
        if (chain) return v.refuse(K2B_ERR_UNSUPPORTED, "k2b_fit_sequence: vertex-selected joints are not built into the chain (fit frame by frame)");
        return K2B_OK;
    };
    const auto check_debug_shape = [&]() -> int {
        if (cfg.debug_launch_shape < ForceShape::automatic || cfg.debug_launch_shape > ForceShape::wide)
            return v.refuse(K2B_ERR_INVALID_ARGUMENT, "k2b_fit_world: debug_launch_shape=%d must be 0..4", cfg.debug_launch_shape);
        return K2B_OK;
    };
    const int angle_dims = el.fused ? 64 : el.prior_dims;
    if (el.fused) {
        if (cfg.projection != 0 && f.fit_scan64)
            return v.refuse(K2B_ERR_UNSUPPORTED, "k2b_fit_world: the projected joint term is built for the fp32 scans only (this model has no scan "
                            "plan, or was created under K2B_FIT_SCAN64)");
        if (check_surface_targets()) return v.code;
    }
    for (int i = 0; i < 4; ++i)
        if (cfg.angle_prior_index[i] < 0 || cfg.angle_prior_index[i] >= angle_dims)
            return v.refuse(K2B_ERR_UNSUPPORTED, "k2b_fit_world: angle_prior_index[%d]=%d must be in [0,%d)", i, cfg.angle_prior_index[i], angle_dims);
    if (!el.fused && (f.J > 63 || rounds_for_depth(max_depth) > 4))      // (transforms are needed down to the deepest targeted joint)
        return v.refuse(K2B_ERR_UNSUPPORTED, "k2b_fit_world: the tree kernel takes up to 63 joints and depth 15");
    if (check_debug_shape()) return v.code;
    if (!el.fused && check_surface_targets()) return v.code;
    // (The L-BFGS step inside the fused launch needs kinematic targets and, outside the persistent launch, independent frames: the
    // L-BFGS entries choose such a launch only where that holds - lbfgs_scheme_for's fused_ok - so there is nothing to refuse.)
    return K2B_OK;
}

inline Shared frames_of(const Call& c) {
    Shared s;
    s.B = c.B;
    s.preserve = c.preserve; s.tr_prior = c.tr_prior; s.grad_out = c.grad_out;
    s.buffers_null = c.targets_null || c.params_null;
    return s;
}

// ---- the entries, each in the order it has always checked ---------------------------------------------------------------------------
inline int judge_fit_sequence(const Call& c, Verdict& v) {
    const char* who = entry_name(c.entry);
    if (refuse_projection(who, c, v)) return v.code;
    if (c.frames_per_sequence < 1) return v.refuse(K2B_ERR_INVALID_ARGUMENT, "%s: frames_per_sequence=%d", who, c.frames_per_sequence);
    if ((int64_t)c.B * c.frames_per_sequence > (int64_t)1 << 30)
        return v.refuse(K2B_ERR_INVALID_ARGUMENT, "%s: %d x %d frames", who, c.B, c.frames_per_sequence);
    Shared s = frames_of(c);
    s.chain_len = c.frames_per_sequence; s.chain_iters = c.followup_iters;
    return shared_path(c, s, v);
}

// k2b_fit_sequences and, over 2D keypoints, k2b_fit_image_sequences: the one entry whose chain runs under the projected joint term
inline int judge_ragged_chain(const Call& c, Verdict& v) {
    const char* who = entry_name(c.entry);
    const bool image = c.entry == Entry::fit_image_sequences;
    if (check_ragged(who, c.num_sequences, c.lengths, c.offsets, v)) return v.code;
    if (check_handles(who, c, v)) return v.code;
    if (image) {
        if (require_projection(who, "k2b_fit_sequences", c, v)) return v.code;
        if (check_focal(who, c.cfg->focal, v)) return v.code;
    } else if (refuse_projection(who, c, v)) {
        return v.code;
    }
    if (!iters_ok(c.followup_iters, kMaxAdamIters)) return v.refuse(K2B_ERR_INVALID_ARGUMENT, "%s: followup_iters=%d", who, c.followup_iters);
    if (!iters_ok(c.cfg->num_iters, kMaxAdamIters)) return v.refuse(K2B_ERR_INVALID_ARGUMENT, "%s: num_iters=%d", who, c.cfg->num_iters);
    if (c.cfg->transl_prior_weight != 0.0f) return v.refuse(K2B_ERR_INVALID_ARGUMENT, "%s: transl_prior_weight must be 0 in a chain", who);
    if (check_targets(who, c, v)) return v.code;
    const bool kinematic = kinematic_only(c.facts->J, c.K, c.index);
    if (image) {
        if (!kinematic)
            return v.refuse(K2B_ERR_UNSUPPORTED, "%s: surface targets (vertex-selected joints, landmarks) keep the 3D term and are not built "
                            "into the chain", who);
        if (check_scan_plan(who, c, v)) return v.code;
    }
    const RaggedSlots r = ragged_order(c.num_sequences, c.lengths, c.offsets);
    if (r.slots == 0) return v.accept_nothing();
    if (c.targets_null || c.params_null) return v.refuse(K2B_ERR_INVALID_ARGUMENT, "%s: NULL parameter / target buffer", who);
    if (!kinematic) return v.refuse(K2B_ERR_UNSUPPORTED, "%s: surface targets (vertex-selected joints, landmarks) are not built into the chain", who);
    Shared s = frames_of(c);
    s.B = r.slots; s.chain_len = r.max_len > 1 ? r.max_len : 2; s.chain_iters = c.followup_iters;
    return shared_path(c, s, v);
}

inline int judge_fit_image(const Call& c, Verdict& v) {
    const char* who = entry_name(c.entry);
    if (check_handles(who, c, v)) return v.code;
    if (require_projection(who, "k2b_fit_world", c, v)) return v.code;
    if (check_focal(who, c.cfg->focal, v)) return v.code;
    if (check_targets(who, c, v)) return v.code;
    int surface = 0;
    for (int k = 0; k < c.K; ++k) surface += c.index[k] >= c.facts->J ? 1 : 0;
    if (surface > kSurfMaxTargets)
        return v.refuse(K2B_ERR_UNSUPPORTED, "%s: %d surface targets (vertex-selected joints and landmarks), at most %d per call", who, surface,
                        kSurfMaxTargets);
    if (surface > 0 && surface == c.K)
        return v.refuse(K2B_ERR_UNSUPPORTED, "%s: at least one kinematic joint (model index < %d) must be among the targets", who, c.facts->J);
    if (check_scan_plan(who, c, v)) return v.code;
    return shared_path(c, frames_of(c), v);
}

// what concerns the views alone: it comes first and follows no handle (`other`: where 3D targets go)
inline int check_views(const char* who, const char* other, const Call& c, Verdict& v) {
    if (!c.cfg) return v.refuse(K2B_ERR_INVALID_ARGUMENT, "%s: model, prior and cfg are required", who);
    if (c.num_views < 1 || c.num_views > kMaxViews)
        return v.refuse(K2B_ERR_INVALID_ARGUMENT, "%s: num_views=%d must be 1..%d", who, c.num_views, kMaxViews);
    if (!c.cameras) return v.refuse(K2B_ERR_INVALID_ARGUMENT, "%s: cameras is NULL", who);
    if (require_projection(who, other, c, v)) return v.code;
    for (int i = 0; i < c.num_views; ++i) {
        const k2b_camera& cam = c.cameras[i];
        for (int e = 0; e < 12; ++e)
            if (!is_finite(e < 9 ? cam.rotation[e] : cam.translation[e - 9]))
                return v.refuse(K2B_ERR_INVALID_ARGUMENT, "%s: cameras[%d].%s[%d] is not finite", who, i, e < 9 ? "rotation" : "translation",
                                e < 9 ? e : e - 9);
        if (check_focal(who, cam.focal, v)) return v.code;
    }
    return K2B_OK;
}
// the multi-view term fits kinematic joints, on the tree kernel or on the fused kernel's fp32 scans
inline int check_view_targets(const char* who, const Call& c, Verdict& v) {
    if (check_targets(who, c, v)) return v.code;
    if (!kinematic_only(c.facts->J, c.K, c.index))
        return v.refuse(K2B_ERR_UNSUPPORTED, "%s: surface targets (vertex-selected joints, landmarks) are not built into the multi-view "
                        "term: model indices below %d only", who, c.facts->J);
    return check_scan_plan(who, c, v);
}

inline int judge_fit_multiview(const Call& c, Verdict& v) {
    const char* who = entry_name(c.entry);
    if (check_views(who, "k2b_fit_world", c, v)) return v.code;
    if (check_handles(who, c, v)) return v.code;
    if (check_view_targets(who, c, v)) return v.code;
    if (c.B > 0 && (int64_t)c.B * c.num_views * c.K > ((int64_t)1 << 40))
        return v.refuse(K2B_ERR_INVALID_ARGUMENT, "%s: %d x %d x %d target rows", who, c.B, c.num_views, c.K);
    return shared_path(c, frames_of(c), v);
}

// k2b_fit_multiview_sequences: k2b_fit_image_sequences' chain under k2b_fit_multiview's joint term - the table of sequences, the
// views, then what the chain entries check, in their order
inline int judge_fit_multiview_sequences(const Call& c, Verdict& v) {
    const char* who = entry_name(c.entry);
    if (check_ragged(who, c.num_sequences, c.lengths, c.offsets, v)) return v.code;
    if (check_views(who, "k2b_fit_sequences", c, v)) return v.code;
    if (check_handles(who, c, v)) return v.code;
    if (!iters_ok(c.followup_iters, kMaxAdamIters)) return v.refuse(K2B_ERR_INVALID_ARGUMENT, "%s: followup_iters=%d", who, c.followup_iters);
    if (!iters_ok(c.cfg->num_iters, kMaxAdamIters)) return v.refuse(K2B_ERR_INVALID_ARGUMENT, "%s: num_iters=%d", who, c.cfg->num_iters);
    if (c.cfg->transl_prior_weight != 0.0f) return v.refuse(K2B_ERR_INVALID_ARGUMENT, "%s: transl_prior_weight must be 0 in a chain", who);
    if (check_view_targets(who, c, v)) return v.code;
    const RaggedSlots r = ragged_order(c.num_sequences, c.lengths, c.offsets);
    if (r.slots == 0) return v.accept_nothing();
    if (c.targets_null || c.params_null) return v.refuse(K2B_ERR_INVALID_ARGUMENT, "%s: NULL parameter / target buffer", who);
    // (the fused kernel's lanes address the target rows of the one launch by a 32-bit index: k2b_fit.hip)
    const int64_t frames = (int64_t)c.offsets[c.num_sequences - 1] + c.lengths[c.num_sequences - 1];
    if (fused_eligibility(*c.facts, *c.cfg).fused && frames * c.num_views * c.K >= ((int64_t)1 << 27))
        return v.refuse(K2B_ERR_INVALID_ARGUMENT, "%s: %lld x %d x %d target rows (fewer than 2^27 in one call)", who, (long long)frames, c.num_views,
                        c.K);
    Shared s = frames_of(c);
    s.B = r.slots; s.chain_len = r.max_len > 1 ? r.max_len : 2; s.chain_iters = c.followup_iters;
    return shared_path(c, s, v);
}

// The closure of the L-BFGS entries is the shared path's evaluate-only launch on frames that are already in the output arrays,
// with the preserve pose in scratch.
inline Shared closure_of(const Call& c, int B) {
    Shared s;
    s.B = B;
    s.closure = true;
    s.buffers_null = c.targets_null;
    return s;
}
inline int judge_fit_world_lbfgs(const Call& c, Verdict& v) {
    const char* who = entry_name(c.entry);
    if (check_lbfgs(who, c, false, v)) return v.code;
    if (c.B < 0) return v.refuse(K2B_ERR_INVALID_ARGUMENT, "%s: num_frames=%d", who, c.B);
    if (c.B == 0) return v.accept_nothing();
    if (c.params_null) return v.refuse(K2B_ERR_INVALID_ARGUMENT, "%s: NULL parameter buffer", who);
    Shared s = closure_of(c, c.B);
    s.preserve = true;
    s.tr_prior = c.tr_prior || c.cfg->transl_prior_weight != 0.0f;     // (the centre's default, the start, is an explicit array by then)
    s.grad_out = c.grad_out;
    return shared_path(c, s, v);
}
inline int judge_fit_sequence_lbfgs(const Call& c, Verdict& v) {
    const char* who = entry_name(c.entry);
    if (check_lbfgs(who, c, true, v)) return v.code;
    if (c.B < 0) return v.refuse(K2B_ERR_INVALID_ARGUMENT, "%s: frames=%d", who, c.B);
    if (c.cfg->transl_prior_weight != 0.0f) return v.refuse(K2B_ERR_UNSUPPORTED, "%s: no translation prior in a chain", who);
    if (c.B == 0) return v.accept_nothing();
    if (c.targets_null || c.params_null) return v.refuse(K2B_ERR_INVALID_ARGUMENT, "%s: NULL parameter / target buffer", who);
    // frame by frame, or the whole sequence as one chain slot of the persistent launch: the shared path refuses the same of both
    return shared_path(c, closure_of(c, 1), v);
}
inline int judge_fit_sequences_lbfgs(const Call& c, Verdict& v) {
    const char* who = entry_name(c.entry);
    if (check_ragged(who, c.num_sequences, c.lengths, c.offsets, v)) return v.code;
    if (check_lbfgs(who, c, true, v)) return v.code;
    if (c.cfg->transl_prior_weight != 0.0f) return v.refuse(K2B_ERR_INVALID_ARGUMENT, "%s: transl_prior_weight must be 0 in a chain", who);
    if (check_targets(who, c, v)) return v.code;
    const RaggedSlots r = ragged_order(c.num_sequences, c.lengths, c.offsets);
    if (r.slots == 0) return v.accept_nothing();
    if (c.targets_null || c.params_null) return v.refuse(K2B_ERR_INVALID_ARGUMENT, "%s: NULL parameter / target buffer", who);
    if (!(fused_eligibility(*c.facts, *c.cfg).fused && kinematic_only(c.facts->J, c.K, c.index)))
        return v.refuse(K2B_ERR_UNSUPPORTED, "%s: one launch needs the 24-joint model, the prior over the whole pose and kinematic targets", who);
    Shared s = closure_of(c, r.slots);
    s.chain_len = r.max_len > 1 ? r.max_len : 2; s.chain_iters = lbfgs_followup_closures(c.followup_iters);
    return shared_path(c, s, v);
}
// the shape pre-pass: its closure is one evaluate-only launch over all frames (none: nothing reaches the shared path)
inline int judge_shape_pass_lbfgs(const Call& c, Verdict& v) {
    const char* who = entry_name(c.entry);
    if (check_lbfgs(who, c, false, v)) return v.code;
    const Facts& f = *c.facts;
    if (c.num_sequences < 0 || c.num_frames < 0)
        return v.refuse(K2B_ERR_INVALID_ARGUMENT, "%s: %d sequences, %d frames", who, c.num_sequences, c.num_frames);
    if (c.root_joint < 0 || c.root_joint >= f.J) return v.refuse(K2B_ERR_INVALID_ARGUMENT, "%s: root_joint=%d", who, c.root_joint);
    if (c.num_free_betas < 1 || c.num_free_betas > f.NB || c.num_free_betas > 32)
        return v.refuse(K2B_ERR_INVALID_ARGUMENT, "%s: num_free_betas=%d (1..min(%d, 32))", who, c.num_free_betas, f.NB);
    if (c.K < 1 || !c.index) return v.refuse(K2B_ERR_INVALID_ARGUMENT, "%s: num_targets=%d / model_joint_index", who, c.K);
    for (int k = 0; k < c.K; ++k)
        if (c.index[k] < 0 || c.index[k] >= f.J)
            return v.refuse(K2B_ERR_INVALID_ARGUMENT, "%s: model_joint_index[%d]=%d (kinematic joints only)", who, k, c.index[k]);
    if (c.num_sequences == 0) return v.accept_nothing();
    if (c.params_null || c.targets_null) return v.refuse(K2B_ERR_INVALID_ARGUMENT, "%s: NULL buffer", who);
    if (c.num_frames == 0) return K2B_OK;
    return shared_path(c, closure_of(c, c.num_frames), v);
}

// Is the call accepted?  v.code is the answer (K2B_OK, or the refusal with v.message), v.nothing says that an accepted call has
// nothing to fit.
inline int judge(const Call& c, Verdict& v) {
    switch (c.entry) {
    case Entry::fit_world: return shared_path(c, frames_of(c), v);
    case Entry::fit_sequence: return judge_fit_sequence(c, v);
    case Entry::fit_sequences:
    case Entry::fit_image_sequences: return judge_ragged_chain(c, v);
    case Entry::fit_image: return judge_fit_image(c, v);
    case Entry::fit_multiview: return judge_fit_multiview(c, v);
    case Entry::fit_world_lbfgs: return judge_fit_world_lbfgs(c, v);
    case Entry::fit_sequence_lbfgs: return judge_fit_sequence_lbfgs(c, v);
    case Entry::fit_sequences_lbfgs: return judge_fit_sequences_lbfgs(c, v);
    case Entry::shape_pass_lbfgs: return judge_shape_pass_lbfgs(c, v);
    case Entry::fit_multiview_sequences: return judge_fit_multiview_sequences(c, v);
    }
    return v.refuse(K2B_ERR_INVALID_ARGUMENT, "unknown fit entry");
}

}  // namespace rules
}  // namespace k2b
