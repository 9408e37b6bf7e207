// Host check of the device L-BFGS host driver's plans (csrc/k2b_lbfgs_plan.h): the schedule of launches replayed for every scheme,
// the iteration counts against torch's rule, the state layout against a sum made frame by frame, every workspace map against the
// pointer arithmetic the entries used to do by hand (transcribed below), the step kernel's plan against a count of the pairs that
// fit.  The rules are written out here on their own and never taken from the header's helpers.  No HIP call, no device.
// Usage: lbfgs_plan_check   (tests/test_lbfgs_plan_host.py); prints one line per section and "N failures" last.
#include <cstddef>
#include <cstdio>
#include <string>
#include <vector>

#include "k2b_lbfgs_plan.h"

using namespace k2b;

static int g_failures = 0;
static std::string g_where;
#define CHECK(cond, ...)                                                        \
    do {                                                                        \
        if (!(cond)) {                                                          \
            if (++g_failures <= 20) {                                           \
                std::printf("FAIL %s: %s  [", g_where.c_str(), #cond);          \
                std::printf(__VA_ARGS__);                                       \
                std::printf("]\n");                                             \
            }                                                                   \
        }                                                                       \
    } while (0)
#define WHERE(...)                                        \
    do {                                                  \
        char where__[160];                                \
        std::snprintf(where__, sizeof where__, __VA_ARGS__); \
        g_where = where__;                                \
    } while (0)

static size_t up16(size_t n) { return (n + 15) / 16 * 16; }
// torch.optim.LBFGS: max_eval = max_iter * 5 // 4
static int torch_max_eval(int max_iter) { const int x = max_iter * 5; return (x - x % 4) / 4; }

// ---- schedule ---------------------------------------------------------------------------------------------------------------------
static void check_schedule() {
    using K = LbfgsLaunchKind;
    using B = LbfgsBuf;
    const LbfgsScheme schemes[3] = {LbfgsScheme::two_launches, LbfgsScheme::fused_rounds, LbfgsScheme::persistent};
    std::vector<int> iters;
    for (int i = 1; i <= 40; ++i) iters.push_back(i);
    iters.push_back(10000);
    for (int si = 0; si < 3; ++si)
        for (int max_iter : iters) {
            const int r = torch_max_eval(max_iter) + 2;
            const LbfgsScheme s = schemes[si];
            WHERE("schedule scheme=%d max_iter=%d", si, max_iter);
            const int n = lbfgs_launch_count(s, r);
            CHECK(n == (si == 0 ? 2 * r + 2 : si == 1 ? r + 2 : 1), "%d launches", n);
            B pending = B::none;               // the buffer that holds a result no step has consumed
            LbfgsLaunch prev{K::closure, false, B::none, B::none, B::none};
            int consumed = 0, finalised = 0;
            for (int i = 0; i < n; ++i) {
                WHERE("schedule scheme=%d max_iter=%d launch=%d", si, max_iter, i);
                const LbfgsLaunch l = lbfgs_launch_at(s, r, i);
                const bool last = i == n - 1;
                if (si == 0) CHECK(l.kind == K::closure || l.kind == K::step, "kind %d", (int)l.kind);
                if (si == 1) CHECK(l.kind == (i == 0 ? K::closure : last ? K::finalize_closure : K::step_closure), "kind %d", (int)l.kind);
                if (si == 2) CHECK(l.kind == K::persistent, "kind %d", (int)l.kind);
                CHECK(l.reads == B::none || l.reads == B::A || l.reads == B::B, "reads %d", (int)l.reads);
                CHECK(l.reads == B::none || l.reads != l.writes, "reads and writes buffer %d", (int)l.reads);
                CHECK(l.finalize == (l.kind == K::finalize_closure || (l.kind == K::step && l.finalize)), "finalize flag");
                const bool consumes = (l.kind == K::step && !l.finalize) || l.kind == K::step_closure;
                if (consumes) {
                    CHECK(finalised == 0, "a step behind the finalise");
                    CHECK(l.reads != B::none && pending == l.reads && prev.writes == l.reads, "reads %d, pending %d, predecessor wrote %d",
                          (int)l.reads, (int)pending, (int)prev.writes);
                    ++consumed;
                    pending = B::none;
                }
                if (l.finalize) {
                    CHECK(consumed == r && finalised == 0, "%d results consumed before the finalise, %d rounds", consumed, r);
                    ++finalised;
                }
                const bool writes = l.kind != K::step;
                CHECK(writes == (l.writes != B::none), "writes %d", (int)l.writes);
                if (writes) {
                    // the closure at the result is the last launch and the only one that writes the caller's outputs
                    CHECK((l.writes == B::out) == last, "writes %d", (int)l.writes);
                    if (!last) pending = l.writes;
                }
                if (last) {
                    // without a loss output the final loss goes to scratch: A with two launches per round, buffer (rounds - 1) & 1 with
                    // fused rounds, B with the persistent launch
                    const B want = si == 0 ? B::A : si == 1 ? (((r - 1) & 1) ? B::B : B::A) : B::B;
                    CHECK(l.writes == B::out && l.loss_spare == want, "spare %d, expected %d", (int)l.loss_spare, (int)want);
                    CHECK(l.loss_spare != l.reads, "the spare is the buffer the launch reads");
                } else {
                    CHECK(l.loss_spare == B::none, "spare %d", (int)l.loss_spare);
                }
                prev = l;
            }
            WHERE("schedule scheme=%d max_iter=%d", si, max_iter);
            if (si != 2) CHECK(consumed == r && finalised == 1, "%d consumed, %d finalised, %d rounds", consumed, finalised, r);
        }
}

// ---- counts -----------------------------------------------------------------------------------------------------------------------
static void check_counts() {
    for (int it = 1; it <= 10000; ++it) {
        WHERE("counts max_iter=%d", it);
        const int ev = torch_max_eval(it);
        CHECK(lbfgs_max_eval(it) == ev, "%d evaluations, expected %d", lbfgs_max_eval(it), ev);
        CHECK(lbfgs_rounds(it) == ev + 2, "%d rounds", lbfgs_rounds(it));
        CHECK(lbfgs_persistent_closures(it) == ev + 3, "%d closures", lbfgs_persistent_closures(it));
        CHECK(lbfgs_followup_closures(it) == ev + 3, "%d follow-up closures", lbfgs_followup_closures(it));
        for (int h = 1; h <= 100; h += (h < 5 ? 1 : 19)) {
            const int want = h < it ? h : it;
            CHECK(lbfgs_history_cut(h, it) == want, "history %d cut to %d", h, lbfgs_history_cut(h, it));
        }
    }
}

// ---- state layout and workspace maps -------------------------------------------------------------------------------------------
static const int kBatches[] = {0, 1, 2, 3, 17}, kWidths[] = {8, 85, 88, 192, 193, 224, 256}, kHistories[] = {1, 30, 100}, kFrames[] = {0, 1, 5};

struct StateSum { size_t ints, vectors, bytes; };
static StateSum state_by_frames(int B, int P, int H) {
    size_t doubles = 0, ints = 0, floats = 0;
    for (int f = 0; f < B; ++f) {
        doubles += 16 + H;                     // sixteen scalars and one rho per history pair
        ints += 11;
        for (int v = 0; v < 8 + 2 * H; ++v) floats += P;   // eight vectors, then Y [H] and S [H]
    }
    StateSum s{};
    s.ints = doubles * sizeof(double);
    s.vectors = up16(s.ints + ints * sizeof(int));
    s.bytes = s.vectors + floats * sizeof(float);
    return s;
}

static void check_state_layout() {
    using namespace lbfgs_dev;
    WHERE("state layout enumerators");
    CHECK(SD_RO == 16 && SI_COUNT == 11 && SV_HIST == 8, "SD_RO %d SI_COUNT %d SV_HIST %d", (int)SD_RO, (int)SI_COUNT, (int)SV_HIST);
    CHECK(PH_INIT == 0, "a cleared state is not phase INIT");
    for (int B : kBatches)
        for (int P : kWidths)
            for (int H : kHistories) {
                WHERE("state layout B=%d P=%d H=%d", B, P, H);
                size_t si = 1, sv = 1;
                const size_t n = lbfgs_state_bytes(B, P, H, &si, &sv);
                const StateSum want = state_by_frames(B, P, H);
                CHECK(si == want.ints && sv == want.vectors && n == want.bytes, "%zu %zu %zu, expected %zu %zu %zu", si, sv, n, want.ints,
                      want.vectors, want.bytes);
                CHECK(sv % 16 == 0 && si % sizeof(int) == 0, "alignment of %zu / %zu", si, sv);
                int nd = 0, ni = 0;
                lbfgs_state_rows(H, &nd, &ni);
                CHECK(nd == 16 + H && ni == 11, "rows of %d doubles, %d ints", nd, ni);
            }
}

// one region of a map as the check sees it: where it is, how long, the alignment it must have
struct Region { const char* name; size_t off, bytes, align; };
static void check_regions(const std::vector<Region>& rs, size_t total, size_t want_total) {
    size_t end = 0;
    for (const Region& r : rs) {
        CHECK(r.off >= end, "%s at %zu begins before %zu", r.name, r.off, end);
        CHECK(r.off % r.align == 0, "%s at %zu, alignment %zu", r.name, r.off, r.align);
        end = r.off + r.bytes;
    }
    CHECK(total >= end && total == want_total, "total %zu, expected %zu, regions end at %zu", total, want_total, end);
}
// the optimiser's part at `base`, as lbfgs_ws_layout / lbfgs_ws_assign carved it; returns the first byte behind it
static size_t check_opt(const LbfgsOptMap& m, size_t base, int B, int P, int H, std::vector<Region>* rs) {
    const StateSum st = state_by_frames(B, P, H);
    const size_t n_state = up16(st.bytes), n_res = up16(2 * ((size_t)B * P + B) * sizeof(float));
    const size_t gbuf = base + n_state, lbuf = gbuf + (size_t)B * P * 4, gbuf2 = lbuf + (size_t)B * 4, lbuf2 = gbuf2 + (size_t)B * P * 4;
    CHECK(m.state == base && m.ints == base + st.ints && m.vectors == base + st.vectors, "state %zu %zu %zu", m.state, m.ints, m.vectors);
    CHECK(m.grad_a == gbuf && m.loss_a == lbuf && m.grad_b == gbuf2 && m.loss_b == lbuf2, "results %zu %zu %zu %zu, expected %zu %zu %zu %zu",
          m.grad_a, m.loss_a, m.grad_b, m.loss_b, gbuf, lbuf, gbuf2, lbuf2);
    CHECK(m.end == base + n_state + n_res, "end %zu", m.end);
    CHECK(lbfgs_clear_bytes(m) == st.vectors, "%zu bytes cleared", lbfgs_clear_bytes(m));
    rs->push_back({"state doubles", m.state, st.ints, 16});
    rs->push_back({"state ints", m.ints, (size_t)B * 11 * 4, sizeof(int)});
    rs->push_back({"state vectors", m.vectors, st.bytes - st.vectors, 16});
    rs->push_back({"gradients A", m.grad_a, (size_t)B * P * 4, 16});
    rs->push_back({"losses A", m.loss_a, (size_t)B * 4, sizeof(float)});
    rs->push_back({"gradients B", m.grad_b, (size_t)B * P * 4, sizeof(float)});
    rs->push_back({"losses B", m.loss_b, (size_t)B * 4, sizeof(float)});
    rs->push_back({"end of the optimiser's part", m.end, 0, 16});
    return base + n_state + n_res;
}

static void check_maps() {
    const size_t F = sizeof(float);
    for (int B : kBatches)
        for (int P : kWidths)
            for (int NB : {1, 10, 32}) {
                const int D = P - 6 - NB;
                if (D < 1) continue;
                for (int H : kHistories) {
                    std::vector<Region> rs;
                    {   // k2b_fit_world_lbfgs: pres = behind the optimiser, trp = pres + B D; n_opt + (B D + 3 B) floats
                        WHERE("world map B=%d P=%d NB=%d H=%d", B, P, NB, H);
                        const LbfgsWorldMap m = lbfgs_world_map(B, P, D, H);
                        const size_t n_opt = check_opt(m.opt, 0, B, P, H, &rs);
                        CHECK(m.preserve == n_opt && m.tr_prior == n_opt + (size_t)B * D * F, "preserve %zu, tr_prior %zu", m.preserve, m.tr_prior);
                        rs.push_back({"preserve", m.preserve, (size_t)B * D * F, 16});
                        rs.push_back({"tr_prior", m.tr_prior, (size_t)B * 3 * F, F});
                        check_regions(rs, m.total, n_opt + ((size_t)B * D + (size_t)B * 3) * F);
                    }
                    if (B == 1) {   // k2b_fit_sequence_lbfgs: one optimiser, pres behind it; n_opt + D floats
                        WHERE("sequence map P=%d NB=%d H=%d", P, NB, H);
                        rs.clear();
                        const LbfgsSequenceMap m = lbfgs_sequence_map(P, D, H);
                        const size_t n_opt = check_opt(m.opt, 0, 1, P, H, &rs);
                        CHECK(m.preserve == n_opt, "preserve %zu", m.preserve);
                        rs.push_back({"preserve", m.preserve, (size_t)D * F, 16});
                        check_regions(rs, m.total, n_opt + (size_t)D * F);
                    }
                    {   // k2b_fit_sequences_lbfgs: n_meta = the [slots][4] table padded to 16 bytes, the optimiser at n_meta
                        WHERE("sequences map slots=%d P=%d H=%d", B, P, H);
                        rs.clear();
                        const LbfgsSequencesMap m = lbfgs_sequences_map(B, P, H);
                        const size_t n_meta = up16((size_t)B * 4 * sizeof(int));
                        CHECK(m.meta == 0, "meta %zu", m.meta);
                        rs.push_back({"slot table", m.meta, (size_t)B * 4 * sizeof(int), 16});
                        const size_t end = check_opt(m.opt, n_meta, B, P, H, &rs);
                        check_regions(rs, m.total, end);
                    }
                    for (int N : kFrames) {
                        // k2b_shape_pass_lbfgs: go_s behind the optimiser, bp_s = go_s + S*3 ... grad_f = loss_f + N;
                        // n_opt + (S P + N (NB + 3 + 3 + D + NB + 3 + 1 + P)) floats
                        WHERE("shape pass map S=%d N=%d P=%d NB=%d H=%d", B, N, P, NB, H);
                        rs.clear();
                        const int S = B;
                        const ShapePassMap m = shape_pass_map(S, N, P, D, NB, H);
                        const size_t go_s = check_opt(m.opt, 0, S, P, H, &rs);
                        const size_t bp_s = go_s + (size_t)S * 3 * F, be_s = bp_s + (size_t)S * D * F, tr_s = be_s + (size_t)S * NB * F;
                        const size_t be_f = tr_s + (size_t)S * 3 * F, tr_f = be_f + (size_t)N * NB * F;
                        const size_t go_o = tr_f + (size_t)N * 3 * F, bp_o = go_o + (size_t)N * 3 * F, be_o = bp_o + (size_t)N * D * F;
                        const size_t tr_o = be_o + (size_t)N * NB * F, loss_f = tr_o + (size_t)N * 3 * F, grad_f = loss_f + (size_t)N * F;
                        CHECK(m.go_s == go_s && m.bp_s == bp_s && m.be_s == be_s && m.tr_s == tr_s, "points %zu %zu %zu %zu", m.go_s, m.bp_s, m.be_s, m.tr_s);
                        CHECK(m.points_bytes == (size_t)S * P * F, "%zu bytes of points", m.points_bytes);
                        CHECK(m.be_f == be_f && m.tr_f == tr_f && m.go_o == go_o && m.bp_o == bp_o && m.be_o == be_o && m.tr_o == tr_o &&
                              m.loss_f == loss_f && m.grad_f == grad_f, "frame buffers %zu %zu %zu %zu %zu %zu %zu %zu", m.be_f, m.tr_f, m.go_o, m.bp_o,
                              m.be_o, m.tr_o, m.loss_f, m.grad_f);
                        const size_t off[12] = {m.go_s, m.bp_s, m.be_s, m.tr_s, m.be_f, m.tr_f, m.go_o, m.bp_o, m.be_o, m.tr_o, m.loss_f, m.grad_f};
                        const size_t len[12] = {(size_t)S * 3, (size_t)S * D, (size_t)S * NB, (size_t)S * 3, (size_t)N * NB, (size_t)N * 3,
                                                (size_t)N * 3, (size_t)N * D, (size_t)N * NB, (size_t)N * 3, (size_t)N, (size_t)N * P};
                        for (int i = 0; i < 12; ++i) rs.push_back({"shape pass array", off[i], len[i] * F, i == 0 ? (size_t)16 : F});
                        check_regions(rs, m.total, go_s + ((size_t)S * P + (size_t)N * (NB + 3 + 3 + D + NB + 3 + 1 + P)) * F);
                    }
                    if (H == kHistories[0]) {   // fit_world_vertex_joints: gbuf, mbuf = + B P, vbuf = + 2 B P, lbuf = + 3 B P, pres = lbuf + B, trp = pres + B D
                        WHERE("vertex-joints map B=%d P=%d NB=%d", B, P, NB);
                        rs.clear();
                        const VertexJointsMap m = vertex_joints_map(B, P, D);
                        const size_t n_g = (size_t)B * P;
                        CHECK(m.grad == 0 && m.adam_m == n_g * F && m.adam_v == 2 * n_g * F && m.loss == 3 * n_g * F &&
                              m.preserve == (3 * n_g + B) * F && m.tr_prior == (3 * n_g + B + (size_t)B * D) * F, "%zu %zu %zu %zu %zu %zu", m.grad, m.adam_m,
                              m.adam_v, m.loss, m.preserve, m.tr_prior);
                        CHECK(m.moments_bytes == 2 * n_g * F, "%zu bytes of moments", m.moments_bytes);
                        rs = {{"gradient", m.grad, n_g * F, F}, {"adam m", m.adam_m, n_g * F, F}, {"adam v", m.adam_v, n_g * F, F},
                              {"loss", m.loss, (size_t)B * F, F}, {"preserve", m.preserve, (size_t)B * D * F, F}, {"tr_prior", m.tr_prior, (size_t)B * 3 * F, F}};
                        check_regions(rs, m.total, (3 * n_g + B + (size_t)B * D + (size_t)B * 3) * F);
                    }
                }
            }
}

// ---- step plan --------------------------------------------------------------------------------------------------------------------
static void check_step_plan() {
    for (int P = 1; P <= 300; ++P)
        for (int H = -1; H <= 102; ++H)
            for (int max_iter : {1, 5, 30, 10000})
                for (int cap : {-1, 0, 3, 1000}) {
                    WHERE("step plan P=%d H=%d max_iter=%d cap=%d", P, H, max_iter, cap);
                    const LbfgsStepPlan p = plan_lbfgs_step(P, H, max_iter, cap);
                    const bool refused = P > 256 || H < 1 || H > 100;
                    CHECK(p.ok == !refused, "ok %d", (int)p.ok);
                    if (refused || !p.ok) continue;
                    // a pair: two vectors of P floats in whole rows of 64 lanes; the pairs stand behind 2 H doubles, all within 48 KiB
                    int rows = 0;
                    while (rows * 64 < P) ++rows;
                    const int pair_bytes = 2 * rows * 64 * 4, head = 2 * H * 8;
                    int room = 0;
                    while (head + (room + 1) * pair_bytes <= 48 * 1024) ++room;
                    int want = H < max_iter ? H : max_iter;
                    if (want > room) want = room;
                    if (cap >= 0 && want > cap) want = cap;
                    CHECK(p.pairs == want, "%d pairs, expected %d (room for %d)", p.pairs, want, room);
                    CHECK(p.lds_bytes == head + want * pair_bytes && p.lds_bytes <= 48 * 1024, "%d bytes of LDS", p.lds_bytes);
                    CHECK(p.wide == (P > 192), "wide %d", (int)p.wide);
                }
}

int main() {
    struct { const char* name; void (*run)(); } sections[] = {{"schedule", check_schedule}, {"counts", check_counts},
        {"state layout", check_state_layout}, {"workspace maps", check_maps}, {"step plan", check_step_plan}};
    for (const auto& s : sections) {
        const int before = g_failures;
        s.run();
        std::printf("%s: %s\n", s.name, g_failures == before ? "ok" : "FAILED");
    }
    std::printf("%d failures\n", g_failures);
    return g_failures ? 1 : 0;
}
