// k2b_api_lbfgs.hip — the L-BFGS entries of the C ABI (include/k2b.h): one device-driven fit (lbfgs_run), the entries for frames, a
// warm-start sequence and ragged sequences, and the shape pre-pass.  The closure is the evaluate-only fit launch of k2b_api_fit.hip,
// the optimiser k2b_lbfgs.hip's state machine; only launches are queued.  Which launches, in which order, on which result buffer,
// and where every array of a workspace lies is k2b_lbfgs_plan.h: this unit executes those plans.
#include <cstdlib>

#include "k2b_host.h"

using namespace k2b::host;

namespace {

// development switch K2B_LBFGS_SCHEME: 1 forces two launches per round, 2 the fused rounds wherever they apply, any other
// value but 0 keeps a sequence out of the one-launch chain (tools/dev_lbfgs_schemes.py)
int lbfgs_scheme() {
    static const int scheme = [] { const char* e = getenv("K2B_LBFGS_SCHEME"); return e ? atoi(e) : 0; }();
    return scheme;
}

// development switch K2B_LBFGS_STAGE_PAIRS: at most that many history pairs of a frame are staged in LDS by the step kernel (0:
// none; every pair of the two-loop recursion then comes from global memory), and the fit takes the step kernel - two launches per
// round, no persistent chain.  Read on EVERY call (a test changes it in-process).  Staging only changes where the same floats
// are read from: the results do not change by a bit (tests/test_gpu_lbfgs_wide.py).  Unset or empty: no cap (-1).
int lbfgs_stage_cap() {
    const char* e = getenv("K2B_LBFGS_STAGE_PAIRS");
    if (!e || !*e) return -1;
    const int v = atoi(e);
    return v < 0 ? -1 : v;
}

template <class T>
T* ws_at(unsigned char* ws, size_t off) { return reinterpret_cast<T*>(ws + off); }

// The optimiser's part of a workspace (k2b_lbfgs_plan.h, LbfgsOptMap) as pointers: its state, closure-result buffers A and B.
struct LbfgsWs {
    unsigned char* ws;
    k2b::LbfgsOptMap m;
    bool state_cleared;                      // (the caller did)
    float* grad(k2b::LbfgsBuf b) const { return b == k2b::LbfgsBuf::A ? ws_at<float>(ws, m.grad_a) : b == k2b::LbfgsBuf::B ? ws_at<float>(ws, m.grad_b) : nullptr; }
    float* loss(k2b::LbfgsBuf b) const { return b == k2b::LbfgsBuf::A ? ws_at<float>(ws, m.loss_a) : b == k2b::LbfgsBuf::B ? ws_at<float>(ws, m.loss_b) : nullptr; }
    // scalars and integers: phase INIT (vectors are written before they are read)
    hipError_t clear(hipStream_t stream) const { return hipMemsetAsync(ws + m.state, 0, k2b::lbfgs_clear_bytes(m), stream); }
};

struct LbfgsOpts {
    int max_iter, history;                   // (history: already cut to what a fit of max_iter iterations can fill)
    double lr, tol_g, tol_c;
};
// B optimiser instances over the points `p`, reading closure result buffer A of `w`
k2b::LbfgsArgs make_lbfgs_args(int B, int D, int NB, const LbfgsOpts& o, const Params& p, const LbfgsWs& w) {
    k2b::LbfgsArgs la{};
    la.B = B; la.P = 3 + D + NB + 3; la.D = D; la.NB = NB; la.H = o.history;
    la.max_iter = o.max_iter; la.max_eval = k2b::lbfgs_max_eval(o.max_iter);
    la.lr = o.lr; la.tol_g = o.tol_g; la.tol_c = o.tol_c;
    la.go = p.go; la.bp = p.bp; la.be = p.be; la.tr = p.tr;
    la.loss_in = w.loss(k2b::LbfgsBuf::A); la.grad_in = w.grad(k2b::LbfgsBuf::A);
    la.sd = ws_at<double>(w.ws, w.m.state); la.si = ws_at<int>(w.ws, w.m.ints); la.sv = ws_at<float>(w.ws, w.m.vectors);
    return la;
}
k2b::LbfgsArgs make_lbfgs_args(int B, const k2b_model* model, const LbfgsOpts& o, const Params& p, const LbfgsWs& w) {
    return make_lbfgs_args(B, 3 * (model->J - 1), model->NB, o, p, w);
}
k2b::LbfgsArgs step_args(const k2b::LbfgsArgs& la, const k2b::LbfgsLaunch& l) {
    k2b::LbfgsArgs s = la;
    s.finalize = l.finalize ? 1 : 0;
    return s;
}

// launches [0, launches) of a fit's schedule (k2b_lbfgs_plan.h), each handed to `launch`
template <class Launch>
int lbfgs_drive(k2b::LbfgsScheme scheme, int rounds, int launches, Launch&& launch) {
    for (int i = 0; i < launches; ++i)
        if (const int rc = launch(k2b::lbfgs_launch_at(scheme, rounds, i)); rc != K2B_OK) return rc;
    return K2B_OK;
}

// whether the fused kernel takes the frames of a call with the L-BFGS step inside: 24-joint model, the prior over the whole pose,
// kinematic targets only
bool fused_takes(const k2b_model* model, const k2b_prior* prior, const k2b_fit_config* cfg, const FitCall& c) {
    return k2b::rules::fused_eligibility(fit_facts(model, prior), *cfg).fused && k2b::rules::kinematic_only(model->J, c.K, c.model_joint_index);
}

// One device-driven L-BFGS fit of the frames of `at`, whose start is ALREADY in the parameter arrays at.out (in place): state
// cleared, then the schedule of its scheme.  `w` = the optimiser's part of stream-ordered scratch, at.preserve / at.tr_prior =
// preserve pose / translation prior centre (device, outside the arrays).
int lbfgs_run(const k2b_model* model, const k2b_prior* prior, const k2b_fit_config* cfg, const FitCall& at, const LbfgsOpts& o,
              LbfgsWs& w) {
    using Kind = k2b::LbfgsLaunchKind;
    hipStream_t stream = at.stream;
    const int B = at.B;
    if (!w.state_cleared) HIP_TRY(w.clear(stream));
    w.state_cleared = false;
    k2b_fit_config ec = *cfg;
    ec.num_iters = 1;
    ec.step_size = 0.0;                                                  // evaluate-only: the closure
    k2b_fit_config pc = ec;
    pc.num_iters = k2b::lbfgs_persistent_closures(o.max_iter);           // at most two frames per CU: the whole fit is ONE launch (k2b_fit.hip, LbMode::persistent)
    FitCall ev = at;
    ev.in = at.out.as_const();
    // One launch per round where the fused kernel takes the frames (24-joint model, the prior over the whole pose, kinematic
    // targets only, at most four frames per CU - lbfgs_scheme_for, k2b_launch_plan.h), otherwise two launches per round.
    const int stage_cap = lbfgs_stage_cap();
    const k2b::LbfgsScheme scheme = k2b::lbfgs_scheme_for(B, device_cus(), fused_takes(model, prior, cfg, at), stage_cap, lbfgs_scheme());
    // the optimiser's arguments travel in the launch's own arguments: [0] reads result buffer A, [1] reads B
    const k2b::LbfgsArgs la = make_lbfgs_args(B, model, o, at.out, w);
    k2b::LbfgsArgs both[2] = {la, la};
    both[1].loss_in = w.loss(k2b::LbfgsBuf::B); both[1].grad_in = w.grad(k2b::LbfgsBuf::B);
    const int rounds = k2b::lbfgs_rounds(o.max_iter);
    return lbfgs_drive(scheme, rounds, k2b::lbfgs_launch_count(scheme, rounds), [&](const k2b::LbfgsLaunch& l) -> int {
        const k2b::LbfgsArgs& args = both[l.reads == k2b::LbfgsBuf::B];
        if (l.kind == Kind::step) {
            HIP_TRY(k2b::launch_lbfgs_step(step_args(args, l), stream, stage_cap));
            return K2B_OK;
        }
        ev.lbfgs.mode = l.kind == Kind::closure ? k2b::LbMode::none : l.kind == Kind::step_closure ? k2b::LbMode::step
                      : l.kind == Kind::finalize_closure ? k2b::LbMode::finalize : k2b::LbMode::persistent;
        ev.lbfgs.args = l.kind == Kind::closure ? nullptr : &args;
        // the closure at the result leaves the loss (+ gradient) with the caller (world_space.py:245-246 evaluates the loss once
        // more behind the optimiser)
        const bool last = l.writes == k2b::LbfgsBuf::out;
        ev.loss_out = last ? (at.loss_out ? at.loss_out : w.loss(l.loss_spare)) : w.loss(l.writes);
        ev.grad_out = last ? at.grad_out : w.grad(l.writes);
        return fit_world_impl(model, prior, l.kind == Kind::persistent ? &pc : &ec, ev);
    });
}

// The widths and the history cut of an accepted call.
struct LbfgsDims { int D, NB, P, history, H; };      // history: the caller's (0: the default), H: what the longest fit can fill of it
LbfgsDims lbfgs_dims(const k2b_model* model, int max_iter, int followup_iters, int history_size) {
    LbfgsDims d;
    d.D = 3 * (model->J - 1); d.NB = model->NB; d.P = 3 + d.D + d.NB + 3;
    d.history = history_size > 0 ? history_size : k2b::kLbfgsMaxHistory;
    d.H = k2b::lbfgs_history_cut(d.history, followup_iters > max_iter ? followup_iters : max_iter);
    return d;
}
// the entry's call as the rules see it (k2b_fit_rules.h), with the L-BFGS numbers
k2b::rules::Call lbfgs_rule_call(k2b::rules::Entry entry, const k2b_model* model, const k2b_prior* prior, const k2b_fit_config* cfg, const FitCall& c,
                                 k2b::rules::Facts* facts, int max_iter, int followup_iters, int history_size, double lr) {
    k2b::rules::Call r = rule_call(entry, model, prior, cfg, c, facts);
    r.max_iter = max_iter; r.followup_iters = followup_iters; r.history_size = history_size; r.lr = lr;
    return r;
}

// The default sequence mode in ONE launch (k2b_fit.hip: chain + LbMode::persistent): the frame loop runs inside the persistent launch -
// per frame a fresh optimiser on the workgroup's idle wave, the start and the preserve pose from the predecessor's result in
// registers.  `c` = the chain's call (slots, targets, parameters, chain.len / chain.meta), `la` = the first frame's optimiser.
int lbfgs_chain_launch(const k2b_model* model, const k2b_prior* prior, const k2b_fit_config* cfg, FitCall c, const k2b::LbfgsArgs& la,
                       int followup_iters) {
    k2b_fit_config pc = *cfg;
    pc.num_iters = k2b::lbfgs_persistent_closures(la.max_iter);
    pc.step_size = 0.0;
    c.chain.iters = k2b::lbfgs_followup_closures(followup_iters);
    c.lbfgs.mode = k2b::LbMode::persistent; c.lbfgs.args = &la; c.lbfgs.chain_max_iter = followup_iters;
    return fit_world_impl(model, prior, &pc, c);
}

}  // namespace

extern "C" {

// L-BFGS branch of the fitters on the device (world_space.py:231-247, camera_space.py:144-182,229-267): per frame
// torch.optim.LBFGS(max_iter, lr, line_search_fn="strong_wolfe").step(closure), the closure = this library's evaluate-only fit
// launch, the optimiser = k2b_lbfgs.hip's state machine.  Only launches are queued: max_eval + 2 rounds of [closure, step], then
// the accepted points go back into the parameter arrays and one more closure launch leaves the final loss (+ gradient).
int k2b_fit_world_lbfgs(const k2b_model* model_c, const k2b_prior* prior, const k2b_fit_config* cfg, int32_t B, int32_t K,
                        const int32_t* model_joint_index, const float* j3d, const float* conf, const float* go_in,
                        const float* bp_in, const float* be_in, const float* tr_in, const float* preserve, const float* tr_prior,
                        float* go_out, float* bp_out, float* be_out, float* tr_out, float* loss_out, float* grad_out,
                        int32_t max_iter, int32_t history_size, double lr, double tolerance_grad, double tolerance_change,
                        void* stream_v) {
    const char* who = "k2b_fit_world_lbfgs";
    const ConstParams in{go_in, bp_in, be_in, tr_in};
    const Params out{go_out, bp_out, be_out, tr_out};
    FitCall at = fit_call(B, K, model_joint_index, j3d, conf, in, out, loss_out, stream_v);
    at.preserve = preserve; at.tr_prior = tr_prior; at.grad_out = grad_out;
    k2b::rules::Facts facts;
    bool go;
    if (const int rc = judge(lbfgs_rule_call(k2b::rules::Entry::fit_world_lbfgs, model_c, prior, cfg, at, &facts, max_iter, 0, history_size, lr), &go);
        rc != K2B_OK || !go)
        return rc;
    const LbfgsDims d = lbfgs_dims(model_c, max_iter, 0, history_size);
    hipStream_t stream = (hipStream_t)stream_v;
    // stream-ordered workspace: optimiser state, closure results, the preserve pose and the translation prior's centre (their
    // defaults are the INITIAL parameters, which the parameter arrays stop holding after the first step)
    const k2b::LbfgsWorldMap m = k2b::lbfgs_world_map(B, d.P, d.D, d.H);
    StreamWorkspace ws(stream);
    HIP_TRY(ws.alloc(m.total));
    LbfgsWs w{ws.get(), m.opt, false};
    float *pres = ws_at<float>(ws.get(), m.preserve), *trp = ws_at<float>(ws.get(), m.tr_prior);
    HIP_TRY_MSG(start_in_place(B, d.D, d.NB, in, out, preserve, tr_prior, pres, trp, stream), "%s: HIP call failed", who);
    at.preserve = pres;
    at.tr_prior = (tr_prior || cfg->transl_prior_weight != 0.0f) ? trp : nullptr;   // (the tree kernel has no translation prior)
    return lbfgs_run(model_c, prior, cfg, at, {max_iter, d.H, lr, tolerance_grad, tolerance_change}, w);
}

// The reference's DEFAULT sequence mode in one call: the frame loop of optimize_params_sequence with use_previous_frame_init=True
// (api/sequence.py:214-281) over the L-BFGS branch (world_space.py:231-247).  Frame 0 is fitted from the given start with
// first_iters iterations and no preserve term; every later frame starts from its predecessor's RESULT, preserves that result's
// body pose with cfg->pose_preserve_weight (world_space.py:159,211) and runs followup_iters iterations; each frame is one
// device-driven L-BFGS fit (k2b_fit_world_lbfgs) and only launches are queued - no host work between the frames.
int k2b_fit_sequence_lbfgs(const k2b_model* model_c, const k2b_prior* prior, const k2b_fit_config* cfg, int32_t T, int32_t K,
                           const int32_t* model_joint_index, const float* j3d, const float* conf, const float* go_in,
                           const float* bp_in, const float* be_in, const float* tr_in, float* go_out, float* bp_out, float* be_out,
                           float* tr_out, float* loss_out, int32_t first_iters, int32_t followup_iters, int32_t history_size, double lr,
                           double tolerance_grad, double tolerance_change, void* stream_v) {
    const ConstParams in{go_in, bp_in, be_in, tr_in};
    const Params out{go_out, bp_out, be_out, tr_out};
    k2b::rules::Facts facts;
    bool go;
    if (const int rc = judge(lbfgs_rule_call(k2b::rules::Entry::fit_sequence_lbfgs, model_c, prior, cfg,
                                             fit_call(T, K, model_joint_index, j3d, conf, in, out, loss_out, stream_v), &facts, first_iters,
                                             followup_iters, history_size, lr), &go);
        rc != K2B_OK || !go)
        return rc;
    const LbfgsDims d = lbfgs_dims(model_c, first_iters, followup_iters, history_size);
    hipStream_t stream = (hipStream_t)stream_v;
    const int D = d.D, NB = d.NB;
    const k2b::LbfgsSequenceMap m = k2b::lbfgs_sequence_map(d.P, D, d.H);
    StreamWorkspace ws(stream);
    HIP_TRY(ws.alloc(m.total));
#define TRY_Q(expr) HIP_TRY_MSG(expr, "k2b_fit_sequence_lbfgs: HIP call failed")
    LbfgsWs w{ws.get(), m.opt, false};
    float* pres = ws_at<float>(ws.get(), m.preserve);
    // the whole sequence in ONE launch where the fused kernel takes it (24-joint model, the prior over the whole pose, kinematic targets)
    // (one sequence = one chain slot; any K2B_LBFGS_SCHEME but 0 keeps it out of the chain)
    FitCall c = fit_call(1, K, model_joint_index, j3d, conf, in, out, loss_out, stream_v);       // rows t of the outputs: frame t's point
    if (lbfgs_scheme() == 0 && T > 1 &&
        k2b::lbfgs_scheme_for(1, device_cus(), fused_takes(model_c, prior, cfg, c), lbfgs_stage_cap(), 0) == k2b::LbfgsScheme::persistent) {
        c.chain.len = T;
        const k2b::LbfgsArgs la = make_lbfgs_args(1, model_c, {first_iters, d.H, lr, tolerance_grad, tolerance_change}, c.out, w);
        TRY_Q(w.clear(stream));
        return lbfgs_chain_launch(model_c, prior, cfg, c, la, followup_iters);
    }
    k2b_fit_config fc = *cfg;
    fc.conf_per_frame = 0;                                        // (one frame per fit: its row of a per-frame array is a shared row)
    for (int t = 0; t < T; ++t) {
        float *go = go_out + (size_t)t * 3, *bp = bp_out + (size_t)t * D, *be = be_out + (size_t)t * NB, *tr = tr_out + (size_t)t * 3;
        const float *sgo = t ? go - 3 : go_in, *sbp = t ? bp - D : bp_in, *sbe = t ? be - NB : be_in, *str = t ? tr - 3 : tr_in;
        // start of this frame = the start given (frame 0) or the previous frame's result; its body pose is also what is preserved
        // (one small launch: the four parameter rows, the preserve pose and the cleared optimiser state)
        TRY_Q(k2b::launch_lbfgs_frame_prep(go, sgo, bp, sbp, be, sbe, tr, str, pres, D, NB, ws_at<void>(ws.get(), m.opt.state),
                                           k2b::lbfgs_clear_bytes(m.opt), stream));
        w.state_cleared = true;
        fc.pose_preserve_weight = t ? cfg->pose_preserve_weight : 0.0f;
        const int iters = t ? followup_iters : first_iters;
        FitCall at = fit_call(1, K, model_joint_index, j3d + (size_t)t * K * 3,
                              conf ? conf + (cfg->conf_per_frame ? (size_t)t * K : 0) : nullptr, {}, {go, bp, be, tr},
                              loss_out ? loss_out + t : nullptr, stream_v);
        at.preserve = pres;
        const LbfgsOpts o{iters, k2b::lbfgs_history_cut(d.history, iters), lr, tolerance_grad, tolerance_change};
        if (const int rc = lbfgs_run(model_c, prior, &fc, at, o, w); rc != K2B_OK) return rc;
    }
#undef TRY_Q
    return K2B_OK;
}

// The default sequence mode (L-BFGS, warm start) for many sequences of different lengths: k2b_fit_sequence_lbfgs's persistent
// chain with one optimiser per sequence, ONE launch (24-joint model, the prior over the whole pose, kinematic targets; other
// configurations: K2B_ERR_UNSUPPORTED, the caller fits sequence by sequence).
int k2b_fit_sequences_lbfgs(const k2b_model* model_c, const k2b_prior* prior, const k2b_fit_config* cfg, int32_t num_sequences,
                            const int32_t* lengths, const int32_t* offsets, int32_t K, const int32_t* model_joint_index,
                            const float* j3d, const float* conf, const float* go_in, const float* bp_in, const float* be_in,
                            const float* tr_in, float* go_out, float* bp_out, float* be_out, float* tr_out, float* loss_out,
                            int32_t first_iters, int32_t followup_iters, int32_t history_size, double lr, double tolerance_grad,
                            double tolerance_change, void* stream_v) {
    const char* who = "k2b_fit_sequences_lbfgs";
    // (rows of the outputs: each frame's point)
    FitCall c = fit_call(0, K, model_joint_index, j3d, conf, {go_in, bp_in, be_in, tr_in}, {go_out, bp_out, be_out, tr_out}, loss_out, stream_v);
    k2b::rules::Facts facts;
    k2b::rules::Call call = lbfgs_rule_call(k2b::rules::Entry::fit_sequences_lbfgs, model_c, prior, cfg, c, &facts, first_iters, followup_iters,
                                            history_size, lr);
    call.num_sequences = num_sequences; call.lengths = lengths; call.offsets = offsets;
    bool go;
    if (const int rc = judge(call, &go); rc != K2B_OK || !go) return rc;
    const k2b::rules::RaggedSlots r = k2b::rules::ragged_order(num_sequences, lengths, offsets);
    const LbfgsDims d = lbfgs_dims(model_c, first_iters, followup_iters, history_size);
    hipStream_t stream = (hipStream_t)stream_v;
    const k2b::LbfgsSequencesMap m = k2b::lbfgs_sequences_map(r.slots, d.P, d.H);
    StreamWorkspace ws(stream);
    HIP_TRY(ws.alloc(m.total));
    int* meta = ws_at<int>(ws.get(), m.meta);
    if (const int rc = upload_slots(r.meta, meta, stream); rc != K2B_OK) return rc;
    const LbfgsWs w{ws.get(), m.opt, false};
    HIP_TRY_MSG(w.clear(stream), "%s: HIP call failed", who);
    // as k2b_fit_sequence_lbfgs's one-launch chain, with one optimiser instance per chain slot (k2b_fit.hip: LbMode::persistent)
    c.B = r.slots; c.chain.len = r.max_len > 1 ? r.max_len : 2; c.chain.meta = meta;
    const k2b::LbfgsArgs la = make_lbfgs_args(r.slots, model_c, {first_iters, d.H, lr, tolerance_grad, tolerance_change}, c.out, w);
    return lbfgs_chain_launch(model_c, prior, cfg, c, la, followup_iters);
}

// The shape pre-pass of S sequences together (reference core/shape.py:10-115, one torch.optim.LBFGS over betas per sequence):
// per round [prep (k2b_shape.hip: shape rows, root-aligned translations) -> ONE evaluate-only fused launch over all frames ->
// reduce (per-sequence loss and gradient in frame order) -> the L-BFGS state machine, one instance per sequence]; max_eval + 2
// rounds and the finalise step are queued on `stream`, nothing comes back to the host.
int k2b_shape_pass_lbfgs(const k2b_model* model_c, const k2b_prior* prior, const k2b_fit_config* cfg, int32_t num_sequences,
                         const int32_t* seq_offsets, int32_t num_frames, int32_t K, const int32_t* model_joint_index,
                         const float* j3d, const float* conf, const float* global_orient, const float* body_pose,
                         const float* root_targets, int32_t root_joint, int32_t num_free_betas, const float* betas_in,
                         float* betas_out, int32_t max_iter, int32_t history_size, double lr, double tolerance_grad,
                         double tolerance_change, void* stream_v) {
    k2b::rules::Facts facts;
    k2b::rules::Call r = lbfgs_rule_call(k2b::rules::Entry::shape_pass_lbfgs, model_c, prior, cfg,
                                         fit_call(num_frames, K, model_joint_index, j3d, conf, {}, {}, nullptr, stream_v), &facts, max_iter, 0,
                                         history_size, lr);
    r.num_sequences = num_sequences; r.num_frames = num_frames; r.root_joint = root_joint; r.num_free_betas = num_free_betas;
    r.params_null = !seq_offsets || !betas_in || !betas_out;
    r.targets_null = num_frames > 0 && (!j3d || !global_orient || !body_pose || !root_targets);
    bool go;
    if (const int rc = judge(r, &go); rc != K2B_OK || !go) return rc;
    const LbfgsDims d = lbfgs_dims(model_c, max_iter, 0, history_size);
    const int NB = d.NB, D = d.D;
    hipStream_t stream = (hipStream_t)stream_v;
    const int S = num_sequences, N = num_frames, nb = num_free_betas;
    // behind the optimiser's workspace: its parameter arrays [S][...], then the per-frame closure buffers [N][...]
    const k2b::ShapePassMap m = k2b::shape_pass_map(S, N, d.P, D, NB, d.H);
    StreamWorkspace ws(stream);
    HIP_TRY(ws.alloc(m.total));
#define TRY_Q(expr) HIP_TRY_MSG(expr, "k2b_shape_pass_lbfgs: HIP call failed")
    const LbfgsWs w{ws.get(), m.opt, false};
    auto f = [&](size_t off) { return ws_at<float>(ws.get(), off); };
    const Params pts{f(m.go_s), f(m.bp_s), f(m.be_s), f(m.tr_s)};
    TRY_Q(w.clear(stream));                                                               // every instance in phase INIT
    TRY_Q(hipMemsetAsync(pts.go, 0, m.points_bytes, stream));                             // pose / transl of the points: 0, never move
    TRY_Q(hipMemcpy2DAsync(pts.be, (size_t)NB * sizeof(float), betas_in, (size_t)nb * sizeof(float), (size_t)nb * sizeof(float), S,
                           hipMemcpyDeviceToDevice, stream));
    k2b::ShapePassArgs sa{};
    sa.S = S; sa.D = D; sa.NB = NB; sa.nb = nb; sa.seq_off = seq_offsets;
    sa.jt0 = model_c->j_template.get() + (size_t)root_joint * 3; sa.jd0 = model_c->j_dirs.get() + (size_t)root_joint * 3 * NB;
    sa.root_y = root_targets; sa.be_state = pts.be; sa.be_f = f(m.be_f); sa.tr_f = f(m.tr_f); sa.grad_f = f(m.grad_f); sa.loss_f = f(m.loss_f);
    sa.grad_state = w.grad(k2b::LbfgsBuf::A); sa.loss_state = w.loss(k2b::LbfgsBuf::A);
    k2b_fit_config ec = *cfg;
    ec.num_iters = 1;
    ec.step_size = 0.0;                                                                  // evaluate-only: the closure
    ec.conf_per_frame = conf ? 1 : 0;
    FitCall ev = fit_call(N, K, model_joint_index, j3d, conf, {global_orient, body_pose, sa.be_f, sa.tr_f},
                          {f(m.go_o), f(m.bp_o), f(m.be_o), f(m.tr_o)}, f(m.loss_f), stream_v);
    ev.grad_out = f(m.grad_f);
    const k2b::LbfgsArgs la = make_lbfgs_args(S, model_c, {max_iter, d.H, lr, tolerance_grad, tolerance_change}, pts, w);
    // two launches per round with [prep, fit, reduce] as the closure; nothing asks for the loss at the result: the schedule
    // ends with its finalise step (the accepted points)
    const k2b::LbfgsScheme scheme = k2b::LbfgsScheme::two_launches;
    const int rounds = k2b::lbfgs_rounds(max_iter), stage_cap = lbfgs_stage_cap();
    const int rc = lbfgs_drive(scheme, rounds, k2b::lbfgs_launch_count(scheme, rounds) - 1, [&](const k2b::LbfgsLaunch& l) -> int {
        if (l.kind == k2b::LbfgsLaunchKind::step) {
            TRY_Q(k2b::launch_lbfgs_step(step_args(la, l), stream, stage_cap));
            return K2B_OK;
        }
        TRY_Q(k2b::launch_shape_prep(sa, stream));
        if (N > 0)
            if (const int frc = fit_world_impl(model_c, prior, &ec, ev); frc != K2B_OK) return frc;
        TRY_Q(k2b::launch_shape_reduce(sa, stream));
        return K2B_OK;
    });
    if (rc != K2B_OK) return rc;
    TRY_Q(hipMemcpy2DAsync(betas_out, (size_t)nb * sizeof(float), pts.be, (size_t)NB * sizeof(float), (size_t)nb * sizeof(float), S,
                           hipMemcpyDeviceToDevice, stream));
#undef TRY_Q
    return K2B_OK;
}

// Development: the optimiser alone, fed a caller's closure results (include/k2b.h).  The state buffer's layout ...
int k2b_debug_lbfgs_state_layout(int32_t B, int32_t P, int32_t H, int64_t* state_bytes, int64_t* offset_ints, int64_t* offset_vectors,
                                 int32_t* doubles_per_frame, int32_t* ints_per_frame) {
    const char* who = "k2b_debug_lbfgs_state_layout";
    if (B < 0) return fail(K2B_ERR_INVALID_ARGUMENT, "%s: num_frames=%d", who, B);
    if (P < 8 || P > 256) return fail(K2B_ERR_UNSUPPORTED, "%s: %d parameters per frame (8 to 256)", who, P);
    if (H < 1 || H > k2b::kLbfgsMaxHistory)
        return fail(K2B_ERR_UNSUPPORTED, "%s: history=%d (1 to %d)", who, H, k2b::kLbfgsMaxHistory);
    if (!state_bytes || !offset_ints || !offset_vectors || !doubles_per_frame || !ints_per_frame)
        return fail(K2B_ERR_INVALID_ARGUMENT, "%s: NULL output", who);
    size_t off_si = 0, off_sv = 0;
    *state_bytes = (int64_t)k2b::lbfgs_state_bytes(B, P, H, &off_si, &off_sv);
    *offset_ints = (int64_t)off_si;
    *offset_vectors = (int64_t)off_sv;
    int nd = 0, ni = 0;
    k2b::lbfgs_state_rows(H, &nd, &ni);
    *doubles_per_frame = nd;
    *ints_per_frame = ni;
    return K2B_OK;
}

// ... and one step: make_lbfgs_args + launch_lbfgs_step on the caller's buffers, everything checked before the launch.
int k2b_debug_lbfgs_step(int32_t B, int32_t D, int32_t NB, float* go, float* bp, float* be, float* tr, const float* loss,
                         const float* grad, int32_t max_iter, int32_t H, double lr, double tolerance_grad, double tolerance_change,
                         void* state, int64_t state_bytes, int32_t finalize, int32_t max_staged_pairs, void* stream_v) {
    const char* who = "k2b_debug_lbfgs_step";
    if (B < 0) return fail(K2B_ERR_INVALID_ARGUMENT, "%s: num_frames=%d", who, B);
    if (D < 1 || NB < 1) return fail(K2B_ERR_INVALID_ARGUMENT, "%s: pose_dim=%d, num_betas=%d (at least 1 each)", who, D, NB);
    const long long P64 = 3ll + D + NB + 3;
    if (P64 < 8 || P64 > 256) return fail(K2B_ERR_UNSUPPORTED, "%s: %lld parameters per frame (8 to 256)", who, P64);
    const int P = (int)P64;
    if (H < 1 || H > k2b::kLbfgsMaxHistory)
        return fail(K2B_ERR_UNSUPPORTED, "%s: history=%d (1 to %d)", who, H, k2b::kLbfgsMaxHistory);
    if (max_iter < 1 || max_iter > 10000) return fail(K2B_ERR_INVALID_ARGUMENT, "%s: max_iter=%d", who, max_iter);
    if (!(lr > 0.0)) return fail(K2B_ERR_INVALID_ARGUMENT, "%s: lr must be positive", who);
    if (!(tolerance_grad >= 0.0) || !(tolerance_change >= 0.0)) return fail(K2B_ERR_INVALID_ARGUMENT, "%s: negative tolerance", who);
    if (B == 0) return K2B_OK;
    if (!go || !bp || !be || !tr || !state) return fail(K2B_ERR_INVALID_ARGUMENT, "%s: NULL parameter / state buffer", who);
    if (!finalize && (!loss || !grad)) return fail(K2B_ERR_INVALID_ARGUMENT, "%s: NULL closure result", who);
    LbfgsWs w{static_cast<unsigned char*>(state), {}, false};
    const size_t need = k2b::lbfgs_state_bytes(B, P, H, &w.m.ints, &w.m.vectors);
    if (state_bytes < 0 || (size_t)state_bytes < need)
        return fail(K2B_ERR_INVALID_ARGUMENT, "%s: state buffer of %lld bytes, %zu needed", who, (long long)state_bytes, need);
    if (reinterpret_cast<uintptr_t>(state) % 16) return fail(K2B_ERR_INVALID_ARGUMENT, "%s: state buffer not 16-byte aligned", who);
    k2b::LbfgsArgs la = make_lbfgs_args(B, D, NB, {max_iter, H, lr, tolerance_grad, tolerance_change}, {go, bp, be, tr}, w);
    // (a finalize call consumes no result, but the kernel requests the gradient row with the state vectors: any readable rows do)
    la.loss_in = loss;
    la.grad_in = grad ? grad : la.sv;
    la.finalize = finalize ? 1 : 0;
    HIP_TRY_MSG(k2b::launch_lbfgs_step(la, (hipStream_t)stream_v, max_staged_pairs < 0 ? -1 : max_staged_pairs), "%s: launch failed", who);
    return K2B_OK;
}

}  // extern "C"
