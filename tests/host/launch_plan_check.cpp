// Host check of the launch policy (csrc/k2b_launch_plan.h): every plan against the rules as DESIGN.md 4.1, 4.6 and 4.7 word them,
// written out here on their own - tables of capacities and waves, the thresholds 4 / 8 / 16, the split into whole rounds plus a
// remainder - and never by calling the header's helpers.  No HIP call, no device.
// Usage: launch_plan_check   (tests/test_launch_plan_host.py); prints one line per section and "N failures" last.
#include <cstdio>
#include <string>

#include "k2b_launch_plan.h"

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

// ---- the rules, restated ---------------------------------------------------------------------------------------------------------
enum { SPLIT = 0, SPLIT_PAIRED = 1, PAIRED = 2, WIDE = 3, SPLIT_LBFGS = 4 };
static const int kCap[5] = {4, 8, 16, 16, 4};        // frame slots of a workgroup, by shape
static const int kWaves[5] = {8, 8, 8, 16, 8};
static const int kForced[5] = {-1, SPLIT, SPLIT_PAIRED, PAIRED, WIDE};   // debug_launch_shape 1..4
static int cdiv(int a, int b) { return a / b + (a % b != 0); }
static int imin(int a, int b) { return a < b ? a : b; }
static int imax(int a, int b) { return a > b ? a : b; }
static int shape_for(int frames_per_cu) { return frames_per_cu <= 4 ? SPLIT : (frames_per_cu <= 8 ? SPLIT_PAIRED : WIDE); }

struct Want { int first, n, shape, fpw; };

static void check_launch(const FitLaunch& l, const Want& w, int num_betas, bool scan64) {
    CHECK(l.first_frame == w.first && l.num_frames == w.n, "frames [%d, +%d), expected [%d, +%d)", l.first_frame, l.num_frames, w.first, w.n);
    CHECK(l.shape == w.shape, "shape %d, expected %d", l.shape, w.shape);
    CHECK(l.frames_per_wg == w.fpw, "frames_per_wg %d, expected %d", l.frames_per_wg, w.fpw);
    CHECK(l.shape >= 0 && l.shape < 5, "shape %d", l.shape);
    if (l.shape < 0 || l.shape >= 5) return;
    CHECK(l.frames_per_wg >= 1 && l.frames_per_wg <= kCap[l.shape], "frames_per_wg %d, capacity %d", l.frames_per_wg, kCap[l.shape]);
    CHECK(l.frames_per_wg >= 1 && l.grid == cdiv(l.num_frames, imax(l.frames_per_wg, 1)), "grid %d", l.grid);
    CHECK(l.block_threads == kWaves[l.shape] * 64, "block %d", l.block_threads);
    CHECK(l.NBT == (num_betas <= 10 ? 10 : 16) && l.scan64 == scan64, "NBT %d scan64 %d", l.NBT, (int)l.scan64);
}

static void check_fit_world(int C) {
    for (int n = 0; n <= 3 * 16 * C + 17; ++n)
        for (int force = 0; force <= 4; ++force)
            for (int lb = 0; lb <= 3; ++lb)
                for (int chain = 0; chain <= 1; ++chain)
                    for (int nb = 10; nb <= 16; nb += 6)
                        for (int s64 = 0; s64 <= 1; ++s64) {
                            char where[128];
                            std::snprintf(where, sizeof where, "fit C=%d n=%d force=%d lb=%d chain=%d nb=%d scan64=%d", C, n, force, lb, chain, nb, s64);
                            g_where = where;
                            const FitPlan p = plan_fit_world(n, C, nb, s64 != 0, force, lb, chain ? 7 : 1);
                            const int per_cu = n > 0 ? cdiv(n, C) : 0;
                            bool ok = true;
                            if (n > 0 && chain) ok = lb == 0 || lb == 3;
                            else if (n > 0 && lb != 0) ok = per_cu <= (lb == 3 ? 2 : 4);
                            CHECK(p.ok == ok, "ok %d, expected %d", (int)p.ok, (int)ok);
                            if (!ok || n == 0) { CHECK(p.num_launches == 0, "%d launches", p.num_launches); continue; }
                            Want w[2];
                            int nw = 1;
                            if (chain) {
                                w[0] = {0, n, lb == 3 ? SPLIT_LBFGS : SPLIT, imin(imax(per_cu, 1), lb == 3 ? 2 : 4)};
                            } else if (lb != 0) {
                                w[0] = {0, n, SPLIT_LBFGS, imin(imax(per_cu, 1), 4)};
                            } else if (force != 0) {
                                const int sh = kForced[force];
                                w[0] = {0, n, sh, n < C ? imin(kCap[sh], n) : imin(kCap[sh], per_cu)};
                            } else if (n > 16 * C && n % (16 * C) != 0) {
                                const int head = n / (16 * C) * (16 * C), rem = n - head, sh = shape_for(cdiv(rem, C));
                                w[0] = {0, head, WIDE, 16};
                                w[1] = {head, rem, sh, imin(kCap[sh], cdiv(rem, C))};
                                nw = 2;
                            } else {
                                const int sh = shape_for(per_cu);
                                w[0] = {0, n, sh, imin(kCap[sh], per_cu)};
                            }
                            CHECK(p.num_launches == nw, "%d launches, expected %d", p.num_launches, nw);
                            if (p.num_launches != nw) continue;
                            // in order, disjoint, covering [0, n)
                            int next = 0;
                            for (int i = 0; i < nw; ++i) {
                                CHECK(p.launch[i].first_frame == next && p.launch[i].num_frames > 0, "launch %d starts at %d, expected %d", i, p.launch[i].first_frame, next);
                                next = p.launch[i].first_frame + p.launch[i].num_frames;
                                check_launch(p.launch[i], w[i], nb, s64 != 0);
                                if (!chain && lb == 0 && force == 0) CHECK(p.launch[i].shape != PAIRED, "automatic shape is paired");
                            }
                            CHECK(next == n, "covered %d of %d", next, n);
                        }
    std::printf("fit_world C=%d: %s\n", C, g_failures ? "FAILED" : "ok");
}

// rows worked out by hand at 256 CUs
static void check_pinned() {
    struct Row { int n, launches; Want a, b; };
    const Row rows[] = {
        {1024, 1, {0, 1024, SPLIT, 4}, {}},
        {1025, 1, {0, 1025, SPLIT_PAIRED, 5}, {}},
        {2048, 1, {0, 2048, SPLIT_PAIRED, 8}, {}},
        {2049, 1, {0, 2049, WIDE, 9}, {}},
        {4096, 1, {0, 4096, WIDE, 16}, {}},
        {4097, 2, {0, 4096, WIDE, 16}, {4096, 1, SPLIT, 1}},
        {8999, 2, {0, 8192, WIDE, 16}, {8192, 807, SPLIT, 4}},
        {10000, 2, {0, 8192, WIDE, 16}, {8192, 1808, SPLIT_PAIRED, 8}},
    };
    for (const Row& r : rows) {
        g_where = "pinned n=" + std::to_string(r.n);
        const FitPlan p = plan_fit_world(r.n, 256, 10, false, 0, 0, 1);
        CHECK(p.ok && p.num_launches == r.launches, "%d launches", p.num_launches);
        if (p.num_launches != r.launches) continue;
        check_launch(p.launch[0], r.a, 10, false);
        if (r.launches == 2) check_launch(p.launch[1], r.b, 10, false);
    }
    g_where = "pinned grids";
    CHECK(plan_fit_world(1024, 256, 10, false, 0, 0, 1).launch[0].grid == 256, "1024 frames");
    CHECK(plan_fit_world(4096, 256, 10, false, 0, 0, 1).launch[0].grid == 256, "4096 frames");
    std::printf("pinned rows: %s\n", g_failures ? "FAILED" : "ok");
}

// the scheme lbfgs_run takes and the plan its launches get agree
static void check_schemes(int C) {
    const int caps[] = {-1, 0, 5}, devs[] = {0, 1, 2, 3};
    for (int n = 1; n <= 3 * 16 * C + 17; ++n) {
        const int per_cu = cdiv(n, C);
        for (int fused_ok = 0; fused_ok <= 1; ++fused_ok)
            for (int cap : caps)
                for (int dev : devs) {
                    char where[128];
                    std::snprintf(where, sizeof where, "scheme C=%d n=%d fused_ok=%d cap=%d dev=%d", C, n, fused_ok, cap, dev);
                    g_where = where;
                    const LbfgsScheme s = lbfgs_scheme_for(n, C, fused_ok != 0, cap, dev);
                    LbfgsScheme want = LbfgsScheme::two_launches;
                    if (fused_ok && cap < 0 && dev != 1 && per_cu <= 4) want = (dev != 2 && per_cu <= 2) ? LbfgsScheme::persistent : LbfgsScheme::fused_rounds;
                    CHECK(s == want, "scheme %d, expected %d", (int)s, (int)want);
                    const bool ok_step = plan_fit_world(n, C, 10, false, 0, LbMode::step, 1).ok;
                    const bool ok_fin = plan_fit_world(n, C, 10, false, 0, LbMode::finalize, 1).ok;
                    const bool ok_pers = plan_fit_world(n, C, 10, false, 0, LbMode::persistent, 1).ok;
                    if (s == LbfgsScheme::fused_rounds) CHECK(ok_step && ok_fin, "fused rounds without a plan");
                    if (s == LbfgsScheme::persistent) CHECK(ok_pers, "persistent without a plan");
                    if (!ok_step || !ok_fin) CHECK(s == LbfgsScheme::two_launches, "no fused plan, scheme %d", (int)s);
                    if (!ok_pers) CHECK(s != LbfgsScheme::persistent, "no persistent plan");
                }
    }
    std::printf("schemes C=%d: %s\n", C, g_failures ? "FAILED" : "ok");
}

static void check_fit_tree(int C) {
    const int shapes[] = {1, 10, 16, 17, 20, 21, 32};
    for (int n = 1; n <= 3 * 16 * C + 17; ++n)
        for (int ns : shapes)
            for (int chain = 0; chain <= 1; ++chain)
                for (int dbg = 0; dbg <= 2; ++dbg) {
                    char where[128];
                    std::snprintf(where, sizeof where, "tree C=%d n=%d num_shape=%d chain=%d debug=%d", C, n, ns, chain, dbg);
                    g_where = where;
                    const FitTreePlan p = plan_fit_tree(n, C, ns, chain != 0, dbg);
                    const int per_cu = imin(cdiv(n, C), 8);          // at most 8 frames per workgroup
                    const bool four = dbg != 1 && (per_cu <= 4 || dbg == 2);
                    const int tw = dbg == 2 ? imin(per_cu, 4) : per_cu;
                    CHECK(p.frames_per_wg == tw && tw >= 1 && tw <= 8, "frames_per_wg %d, expected %d", p.frames_per_wg, tw);
                    CHECK(p.comp_waves == (four ? 4 : 0), "comp_waves %d", p.comp_waves);
                    CHECK(p.grid == cdiv(n, tw), "grid %d", p.grid);
                    CHECK(p.block_threads == 64 * (tw + (four ? 4 : 0)) && p.block_threads <= 64 * 12, "block %d", p.block_threads);
                    CHECK(p.NS == (ns <= 16 ? 16 : (ns <= 20 ? 20 : 32)), "NS %d", p.NS);
                    CHECK(p.chain == (chain != 0), "chain");
                }
    std::printf("fit_tree C=%d: %s\n", C, g_failures ? "FAILED" : "ok");
}

// the LDS areas of the fused fit kernel, from their documented extents (floats)
static const int kPriorImage = 2 * 5 * 64 * 4 + 8 * 2 * 64 + 8 * (4 * 21) * 4;   // rim rows | mu, c | rim fragments
static const int kSlots = 16 * (2 * 96 + 64 + 4), kQ = 16 * 8, kY = 16 * (8 * 64 + 4), kDd = 64 * 52, kPlo = 8 * 4 * 2 * 64 * 4, kWx = 16 * 64, kRc = 8 * 64;

static void check_lds_and_pairs() {
    g_where = "LDS layout";
    CHECK(fit_lds::LDS_FLOATS == kPriorImage + kSlots + kQ + kY + kDd + kPlo + kWx + kRc, "LDS_FLOATS %d", fit_lds::LDS_FLOATS);
    CHECK(fit_lds::LDS_FLOATS * 4 <= 160 * 1024 && fit_lds::kLdsBudgetBytes == 160 * 1024, "%d bytes", fit_lds::LDS_FLOATS * 4);
    CHECK(kPriorImageFloats == kPriorImage, "prior image %d", kPriorImageFloats);
    const int Ps[] = {8, 64, 65, 85, 91, 192, 193, 256}, Hs[] = {1, 2, 30, 100};
    for (int F = 1; F <= 4; ++F) {
        // step kernel: 48 KiB; fused prologue: y exchange + J_dirs table + lo fragments + rim products over the workgroup's frames,
        // in 16-byte units; persistent loop: half of the lo fragments, likewise
        const int budgets[3] = {48 * 1024, (kY + kDd + kPlo + kWx) * 4 / F / 16 * 16, kPlo * 4 / 2 / F / 16 * 16};
        const int got[3] = {lbfgs_step_lds_bytes(), lbfgs_prologue_lds_bytes(F), lbfgs_persistent_lds_bytes(F)};
        for (int b = 0; b < 3; ++b) {
            g_where = "budget " + std::to_string(b) + " F=" + std::to_string(F);
            CHECK(got[b] == budgets[b], "%d bytes, expected %d", got[b], budgets[b]);
            for (int P : Ps)
                for (int H : Hs) {
                    int k = 0;
                    while (2 * H * 8 + (k + 1) * 2 * (64 * ((P + 63) / 64)) * 4 <= budgets[b]) ++k;
                    g_where = "pairs budget " + std::to_string(b) + " F=" + std::to_string(F) + " P=" + std::to_string(P) + " H=" + std::to_string(H);
                    CHECK(lbfgs_staged_pairs(budgets[b], P, H) == k, "%d pairs, expected %d", lbfgs_staged_pairs(budgets[b], P, H), k);
                }
        }
    }
    g_where = "pairs, no room";
    CHECK(lbfgs_staged_pairs(100, 85, 100) == 0 && lbfgs_staged_pairs(0, 8, 1) == 0, "negative room");
    std::printf("LDS layout and staged pairs: %s\n", g_failures ? "FAILED" : "ok");
}

static void check_persistent_grid() {
    g_where = "persistent_grid";
    for (int C : {1, 8, 64, 250, 256, 304})
        for (long long tiles : {1ll, 7ll, 8ll, 9ll, 255ll, 256ll, 300ll, 100000ll, 5000000000ll}) {
            const int g = persistent_grid(C, tiles);
            const int per_cu = C < 8 ? 8 : C / 8 * 8;
            long long want = tiles < per_cu ? (tiles + 7) / 8 * 8 : per_cu;
            CHECK(g == want && g % 8 == 0 && g >= 8, "C=%d tiles=%lld grid=%d", C, tiles, g);
        }
    std::printf("persistent_grid: %s\n", g_failures ? "FAILED" : "ok");
}

int main() {
    for (int C : {1, 8, 64, 256, 304}) {
        check_fit_world(C);
        check_schemes(C);
        check_fit_tree(C);
    }
    check_pinned();
    check_lds_and_pairs();
    check_persistent_grid();
    std::printf("%d failures\n", g_failures);
    return g_failures ? 1 : 0;
}
