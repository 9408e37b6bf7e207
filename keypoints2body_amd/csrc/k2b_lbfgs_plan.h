// k2b_lbfgs_plan.h — what the host decides about a device L-BFGS fit, as pure functions: the layout of the optimiser's state, the
// iteration counts, the schedule of launches with the closure-result buffer each reads and writes, the step kernel's launch, and
// the map of every workspace the entries carve.  The ONE statement of these: k2b_api_lbfgs.hip and k2b_lbfgs.hip
// execute the plans, k2b_lbfgs_device.h reads the state layout, and tests/host/lbfgs_plan_check.cpp holds all of it to rules written
// out independently, without a GPU.  No HIP runtime: a plain host C++ program may include this header alone.
#pragma once
#include "k2b_launch_plan.h"

namespace k2b {

constexpr int kLbfgsMaxHistory = 100;    // torch.optim.LBFGS's default history_size

// ---- state layout ----------------------------------------------------------------------------------------------------------------
namespace lbfgs_dev {

enum { PH_INIT = 0, PH_BRACKET = 1, PH_ZOOM = 2, PH_DONE = 3 };
// per-frame scalars (double) and integers.  THE order of a frame's two state rows: the development entry k2b_debug_lbfgs_step
// (include/k2b.h) hands the rows back as they are, and the binding names their columns after these enumerators, lower case,
// without the prefix (native.LBFGS_STATE_DOUBLES / LBFGS_STATE_INTS; tests/test_host_logic.py holds the two together):
//   doubles [SD_RO + H]: loss, prev_loss, hdiag, t, t_prev, f_prev, gtd_prev, f0, gtd0, dnorm, bt0, bt1, bf0, bf1, bg0, bg1, ro[H]
//   integers [SI_COUNT]: phase, nold, niter, evals, ls_iter, max_ls, ls_evals, first, low, insuf, head
// State: the doubles of all frames, then the integers of all frames, then (16-byte aligned) the vectors (lbfgs_state_bytes).
enum { SD_LOSS, SD_PREV_LOSS, SD_HDIAG, SD_T, SD_T_PREV, SD_F_PREV, SD_GTD_PREV, SD_F0, SD_GTD0, SD_DNORM, SD_BT0, SD_BT1, SD_BF0, SD_BF1,
       SD_BG0, SD_BG1, SD_RO };                      // SD_RO .. SD_RO + H - 1: 1 / (y . s) of the history pairs
enum { SI_PHASE, SI_NOLD, SI_NITER, SI_EVALS, SI_LS_ITER, SI_MAX_LS, SI_LS_EVALS, SI_FIRST, SI_LOW, SI_INSUF, SI_HEAD, SI_COUNT };
// per-frame vectors (float [P] each), then Y [H][P] and S [H][P]
enum { SV_X, SV_G, SV_PREV_G, SV_D, SV_G_PREV, SV_G0, SV_BG0, SV_BG1, SV_HIST };

// Vector elements per lane, a compile-time parameter of the state machine: element e = lane + 64 k, k < EPL, so P <= 64 EPL.
// Three cover the 24- and 52-joint models and the 55-joint one up to 24 shape coefficients (P <= 192): the fit kernel's three
// inlined copies and the step kernel's narrow form.  Four (P <= 256) cover every model the library fits (the tree kernel:
// 63 joints, 32 shape coefficients, P = 224): the step kernel's wide form only.
constexpr int kEpl = 3, kEplWide = 4;

}  // namespace lbfgs_dev

// bytes of the state of B frames; *off_si, *off_sv: where the integers and the vectors begin
inline size_t lbfgs_state_bytes(int B, int P, int H, size_t* off_si, size_t* off_sv) {
    size_t n = (size_t)B * (lbfgs_dev::SD_RO + H) * sizeof(double);
    *off_si = n;
    n += (size_t)B * lbfgs_dev::SI_COUNT * sizeof(int);
    n = (n + 15) / 16 * 16;
    *off_sv = n;
    n += (size_t)B * (lbfgs_dev::SV_HIST + 2 * (size_t)H) * P * sizeof(float);
    return n;
}
// row lengths of the two scalar blocks
inline void lbfgs_state_rows(int H, int* doubles_per_frame, int* ints_per_frame) {
    *doubles_per_frame = lbfgs_dev::SD_RO + H;
    *ints_per_frame = lbfgs_dev::SI_COUNT;
}

// ---- counts ----------------------------------------------------------------------------------------------------------------------
K2B_HD constexpr int lbfgs_max_eval(int max_iter) { return max_iter * 5 / 4; }                  // torch's default max_eval
// [closure, step] rounds the host queues: the most any frame can need (every evaluation, the first one, one to see the exit)
K2B_HD constexpr int lbfgs_rounds(int max_iter) { return lbfgs_max_eval(max_iter) + 2; }
// closures of a persistent launch (FitArgs::num_iters): the rounds and the closure at the result
K2B_HD constexpr int lbfgs_persistent_closures(int max_iter) { return lbfgs_rounds(max_iter) + 1; }
// the same for a chain's follow-up frames (FitArgs::chain_iters)
K2B_HD constexpr int lbfgs_followup_closures(int followup_iters) { return lbfgs_persistent_closures(followup_iters); }
// history slots a fit can fill: it makes at most max_iter - 1 pairs
K2B_HD constexpr int lbfgs_history_cut(int history_size, int max_iter) { return history_size < max_iter ? history_size : max_iter; }

// ---- round schedule --------------------------------------------------------------------------------------------------------------
// The launches of one fit, in order.  A closure writes a result (loss, gradient) into buffer A or B of the workspace, or - the
// closure at the result - into the caller's outputs; a step consumes the result its predecessor wrote.
//   two launches per round:  [closure -> A, step <- A] x rounds, finalise step, closure -> outputs
//   fused rounds:            closure -> A, then launch i = [step <- buffer (i - 1) & 1 | closure -> buffer i & 1] for i = 1 .. rounds,
//                            then [finalise | closure -> outputs]
//   persistent:              one launch
enum class LbfgsLaunchKind { closure, step, step_closure, finalize_closure, persistent };
enum class LbfgsBuf { none, A, B, out };
struct LbfgsLaunch {
    LbfgsLaunchKind kind;
    bool finalize;         // a step that consumes no result: every frame's accepted point goes into the parameter arrays
    LbfgsBuf reads;        // the buffer the optimiser's arguments name (a finalise consumes nothing: its loads only need readable rows)
    LbfgsBuf writes;
    LbfgsBuf loss_spare;   // writes == out and the caller wants no loss: the scratch buffer that takes it
};
K2B_HD constexpr int lbfgs_launch_count(LbfgsScheme scheme, int rounds) {
    return scheme == LbfgsScheme::two_launches ? 2 * rounds + 2 : scheme == LbfgsScheme::fused_rounds ? rounds + 2 : 1;
}
K2B_HD constexpr LbfgsLaunch lbfgs_launch_at(LbfgsScheme scheme, int rounds, int i) {
    using K = LbfgsLaunchKind;
    using B = LbfgsBuf;
    if (scheme == LbfgsScheme::persistent) return {K::persistent, false, B::A, B::out, B::B};
    if (scheme == LbfgsScheme::two_launches) {
        if (i < 2 * rounds) return i % 2 == 0 ? LbfgsLaunch{K::closure, false, B::none, B::A, B::none} : LbfgsLaunch{K::step, false, B::A, B::none, B::none};
        if (i == 2 * rounds) return {K::step, true, B::A, B::none, B::none};
        return {K::closure, false, B::none, B::out, B::A};
    }
    const B rd = ((i - 1) & 1) ? B::B : B::A, wr = (i & 1) ? B::B : B::A;
    if (i == 0) return {K::closure, false, B::none, B::A, B::none};
    if (i <= rounds) return {K::step_closure, false, rd, wr, B::none};
    // the last step has consumed result `rounds - 1`: the arguments stay on the buffer it wrote, the spare is the other one
    return {K::finalize_closure, true, rd, B::out, wr};
}

// ---- step kernel (k2b_lbfgs.hip) ---------------------------------------------------------------------------------------------------
// LDS: the 2 H alphas and rho, then as many staged history pairs as a fit can collect (one per outer iteration) - within 48 KiB, so
// that several frames share a CU; pairs beyond that are read from global memory.  (P > 192: a pair is 2 KiB and H = 30 leaves room
// for 23 of the 30, so the reference's default max_iter = 30 reads pairs 23.. from global memory - tests/test_gpu_lbfgs_wide.py.)
// cap >= 0 caps the number further (development switch: the results do not depend on it).
struct LbfgsStepPlan { bool ok; int pairs, lds_bytes; bool wide; };       // wide: four vector elements per lane (P > 192)
K2B_HD constexpr LbfgsStepPlan plan_lbfgs_step(int P, int H, int max_iter, int cap) {
    if (P > 64 * lbfgs_dev::kEplWide || H < 1 || H > kLbfgsMaxHistory) return {false, 0, 0, false};
    const int PL = (P + 63) / 64 * 64, room = lbfgs_staged_pairs(lbfgs_step_lds_bytes(), P, H);
    int pairs = lbfgs_history_cut(H, max_iter);
    if (pairs > room) pairs = room;
    if (cap >= 0 && pairs > cap) pairs = cap;
    return {true, pairs, 2 * H * (int)sizeof(double) + pairs * 2 * PL * (int)sizeof(float), P > 64 * lbfgs_dev::kEpl};
}

// ---- workspace maps --------------------------------------------------------------------------------------------------------------
// Regions of one allocation, laid out in the order they are asked for: each begins at the next multiple of its alignment.
struct WsLayout {
    size_t at = 0;
    constexpr size_t region(size_t bytes, size_t align) {
        at = (at + align - 1) / align * align;
        const size_t off = at;
        at += bytes;
        return off;
    }
    constexpr size_t floats(size_t n) { return region(n * sizeof(float), sizeof(float)); }
};

// The optimiser's part: its state, then the two closure-result buffers (gradients [B][P], losses [B]), padded to 16 bytes.
struct LbfgsOptMap { size_t state, ints, vectors, grad_a, loss_a, grad_b, loss_b, end; };
constexpr size_t lbfgs_clear_bytes(const LbfgsOptMap& m) { return m.vectors - m.state; }   // scalars and integers: zero = phase INIT
inline LbfgsOptMap lbfgs_opt_map(WsLayout& l, int B, int P, int H) {
    LbfgsOptMap m{};
    size_t si = 0, sv = 0;
    const size_t n = lbfgs_state_bytes(B, P, H, &si, &sv);
    m.state = l.region(n, 16); m.ints = m.state + si; m.vectors = m.state + sv;
    m.grad_a = l.region((size_t)B * P * sizeof(float), 16); m.loss_a = l.floats(B);
    m.grad_b = l.floats((size_t)B * P); m.loss_b = l.floats(B);
    m.end = l.region(0, 16);
    return m;
}
// k2b_fit_world_lbfgs: behind it the preserve pose [B][D] and the translation prior's centre [B][3]
struct LbfgsWorldMap { LbfgsOptMap opt; size_t preserve, tr_prior, total; };
inline LbfgsWorldMap lbfgs_world_map(int B, int P, int D, int H) {
    WsLayout l;
    LbfgsWorldMap m{};
    m.opt = lbfgs_opt_map(l, B, P, H);
    m.preserve = l.floats((size_t)B * D); m.tr_prior = l.floats((size_t)B * 3);
    m.total = l.at;
    return m;
}
// k2b_fit_sequence_lbfgs: one optimiser, the preserve pose [D]
struct LbfgsSequenceMap { LbfgsOptMap opt; size_t preserve, total; };
inline LbfgsSequenceMap lbfgs_sequence_map(int P, int D, int H) {
    WsLayout l;
    LbfgsSequenceMap m{};
    m.opt = lbfgs_opt_map(l, 1, P, H);
    m.preserve = l.floats(D);
    m.total = l.at;
    return m;
}
// k2b_fit_sequences_lbfgs: the slot table [slots][4] in front, one optimiser per slot
struct LbfgsSequencesMap { size_t meta; LbfgsOptMap opt; size_t total; };
inline LbfgsSequencesMap lbfgs_sequences_map(int slots, int P, int H) {
    WsLayout l;
    LbfgsSequencesMap m{};
    m.meta = l.region((size_t)slots * 4 * sizeof(int), 16);
    m.opt = lbfgs_opt_map(l, slots, P, H);
    m.total = l.at;
    return m;
}
// k2b_shape_pass_lbfgs: one optimiser per sequence, its points [S][...] (one block: cleared together), then per frame the shape
// rows and translations the closure reads, the parameters it writes, its loss and its gradient
struct ShapePassMap {
    LbfgsOptMap opt;
    size_t go_s, bp_s, be_s, tr_s, points_bytes;
    size_t be_f, tr_f, go_o, bp_o, be_o, tr_o, loss_f, grad_f, total;
};
inline ShapePassMap shape_pass_map(int S, int N, int P, int D, int NB, int H) {
    WsLayout l;
    ShapePassMap m{};
    m.opt = lbfgs_opt_map(l, S, P, H);
    m.go_s = l.floats((size_t)S * 3); m.bp_s = l.floats((size_t)S * D); m.be_s = l.floats((size_t)S * NB); m.tr_s = l.floats((size_t)S * 3);
    m.points_bytes = l.at - m.go_s;
    m.be_f = l.floats((size_t)N * NB); m.tr_f = l.floats((size_t)N * 3);
    m.go_o = l.floats((size_t)N * 3); m.bp_o = l.floats((size_t)N * D); m.be_o = l.floats((size_t)N * NB); m.tr_o = l.floats((size_t)N * 3);
    m.loss_f = l.floats(N); m.grad_f = l.floats((size_t)N * P);
    m.total = l.at;
    return m;
}
// fit_world_vertex_joints (k2b_api_fit.hip): the evaluate launch's gradient, Adam's two moments (one block: cleared together), the
// loss, the preserve pose and the translation prior's centre
struct VertexJointsMap { size_t grad, adam_m, adam_v, moments_bytes, loss, preserve, tr_prior, total; };
inline VertexJointsMap vertex_joints_map(int B, int P, int D) {
    WsLayout l;
    VertexJointsMap m{};
    m.grad = l.floats((size_t)B * P); m.adam_m = l.floats((size_t)B * P); m.adam_v = l.floats((size_t)B * P);
    m.moments_bytes = l.at - m.adam_m;
    m.loss = l.floats(B); m.preserve = l.floats((size_t)B * D); m.tr_prior = l.floats((size_t)B * 3);
    m.total = l.at;
    return m;
}

}  // namespace k2b
