// Host check of what k2b_fit_multiview_sequences refuses (csrc/k2b_fit_rules.h, which this program includes alone: no HIP runtime,
// no library).  Built with the address and undefined-behaviour sanitizers by tests/test_multiview_chain_host.py.
//
//   multiview_chain_rules_check    a table of bad and good calls of the new entry, each held to its code and to a piece of its
//                                  message (which always starts with the entry's name); then the other ten entries, which
//                                  take no views: a call that carries a rig is judged exactly as the same call without one, and
//                                  the entries that refuse the projected joint term still refuse it by name.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "k2b_fit_rules.h"

namespace R = k2b::rules;

static const char* const kName = "k2b_fit_multiview_sequences";
static int failures = 0;

#define CHECK(cond, ...)                                 \
    do {                                                 \
        if (!(cond)) {                                   \
            ++failures;                                  \
            printf("FAIL %s:%d: ", __FILE__, __LINE__);  \
            printf(__VA_ARGS__);                         \
            printf("\n");                                \
        }                                                \
    } while (0)

static const int kSmplParents[24] = {-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21};
static const int kSmplxParents[55] = {-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 15, 15, 15,
                                      20, 25, 26, 20, 28, 29, 20, 31, 32, 20, 34, 35, 20, 37, 38,
                                      21, 40, 41, 21, 43, 44, 21, 46, 47, 21, 49, 50, 21, 52, 53};

// one call of the new entry with everything it points to; `good()` is accepted on both models
struct Owned {
    R::Facts facts{};
    k2b_fit_config cfg{};
    std::vector<int> depth;
    std::vector<int32_t> index, lengths, offsets;
    std::vector<k2b_camera> cameras;
    R::Call call;
};

static k2b_camera camera() {
    k2b_camera cam{};
    cam.rotation[0] = cam.rotation[4] = cam.rotation[8] = 1.0f;
    cam.translation[2] = 3.0f;
    cam.focal[0] = 500.0f; cam.focal[1] = 430.0f;
    return cam;
}

// model: 0 = the 24-joint SMPL on the fused kernel's fp32 scans, 1 = the same without a scan plan (fp64 scans), 2 = the 55-joint
// SMPL-X on the tree kernel (extra joints and landmarks behind its joints)
static void good(Owned& o, int model, int views = 2, R::Entry entry = R::Entry::fit_multiview_sequences) {
    const int J = model == 2 ? 55 : 24;
    const int* parents = model == 2 ? kSmplxParents : kSmplParents;
    o.depth.assign(J, 0);
    for (int j = 1; j < J; ++j) o.depth[j] = o.depth[parents[j]] + 1;
    o.facts = model == 2 ? R::Facts{55, 72, 51, 20, false, true, o.depth.data(), 69, 8} : R::Facts{24, 21, 0, 10, true, model == 1, o.depth.data(), 69, 8};
    k2b_fit_config& g = o.cfg;
    g = k2b_fit_config{};
    g.num_iters = 30; g.step_size = 1e-2; g.adam_beta1 = 0.9; g.adam_beta2 = 0.999; g.adam_eps = 1e-8;
    const int angle[4] = {52, 55, 9, 12};
    for (int i = 0; i < 4; ++i) g.angle_prior_index[i] = angle[i];
    g.optimize_mask = 15;
    if (model == 2) g.prior_pose_dims = 63;
    g.projection = 1;
    g.focal[0] = g.focal[1] = NAN;                // (not read: every camera carries its own)
    o.index = {0, 1, 2, 16, 17, 0};               // (the last entry is never read: K counts those before it)
    o.lengths = {3, 0, 1, 2};
    o.offsets = {0, 3, 3, 4};
    o.cameras.assign(views > 0 ? views : 1, camera());
    R::Call& c = o.call;
    c = R::Call{};
    c.entry = entry; c.facts = &o.facts; c.cfg = &o.cfg;
    c.K = 5; c.index = o.index.data();
    c.followup_iters = 10;
    c.num_sequences = 4; c.lengths = o.lengths.data(); c.offsets = o.offsets.data();
    c.num_views = views; c.cameras = o.cameras.data();
}

struct Row {
    const char* what;
    int models;                                   // bit m: run on model m
    int code;                                     // expected
    const char* message;                          // a piece of the expected message ("" where the call is accepted)
    bool nothing;                                 // accepted with nothing to fit
    std::function<void(Owned&)> spoil;
};

static void run_table() {
    const int INV = K2B_ERR_INVALID_ARGUMENT, UNS = K2B_ERR_UNSUPPORTED, ALL = 7, TAKEN = 5 /* models 0 and 2 */;
    const std::vector<Row> rows = {
        {"the good call", TAKEN, K2B_OK, "", false, [](Owned&) {}},
        {"one view", TAKEN, K2B_OK, "", false, [](Owned& o) { o.call.num_views = 1; }},
        {"eight views", TAKEN, K2B_OK, "", false, [](Owned& o) { o.cameras.assign(8, camera()); o.call.cameras = o.cameras.data(); o.call.num_views = 8; }},
        {"a single frame", TAKEN, K2B_OK, "", false, [](Owned& o) { o.lengths = {1}; o.offsets = {0}; o.call.num_sequences = 1; o.call.lengths = o.lengths.data(); o.call.offsets = o.offsets.data(); }},
        {"no sequences", TAKEN, K2B_OK, "", true, [](Owned& o) { o.call.num_sequences = 0; }},
        {"empty sequences only", TAKEN, K2B_OK, "", true, [](Owned& o) { o.lengths = {0, 0}; o.offsets = {0, 0}; o.call.num_sequences = 2; o.call.lengths = o.lengths.data(); o.call.offsets = o.offsets.data(); }},
        {"empty sequences, NULL buffers", TAKEN, K2B_OK, "", true, [](Owned& o) { o.lengths = {0}; o.offsets = {0}; o.call.num_sequences = 1; o.call.lengths = o.lengths.data(); o.call.offsets = o.offsets.data(); o.call.targets_null = o.call.params_null = true; }},
        {"a focal in the configuration is not read", TAKEN, K2B_OK, "", false, [](Owned& o) { o.cfg.focal[0] = -1.0f; }},
        {"no views", ALL, INV, "num_views=0 must be 1..8", false, [](Owned& o) { o.call.num_views = 0; }},
        {"nine views", ALL, INV, "num_views=9 must be 1..8", false, [](Owned& o) { o.call.num_views = 9; }},
        {"negative views", ALL, INV, "num_views=-1 must be 1..8", false, [](Owned& o) { o.call.num_views = -1; }},
        {"no cameras", ALL, INV, "cameras is NULL", false, [](Owned& o) { o.call.cameras = nullptr; }},
        {"projection 0", ALL, INV, "projection=0 must be 1 (3D targets: k2b_fit_sequences)", false, [](Owned& o) { o.cfg.projection = 0; }},
        {"projection 2", ALL, INV, "projection=2 must be 1", false, [](Owned& o) { o.cfg.projection = 2; }},
        {"a NaN rotation", ALL, INV, "cameras[1].rotation[4] is not finite", false, [](Owned& o) { o.cameras[1].rotation[4] = NAN; }},
        {"an infinite translation", ALL, INV, "cameras[0].translation[2] is not finite", false, [](Owned& o) { o.cameras[0].translation[2] = -INFINITY; }},
        {"a zero focal", ALL, INV, "focal[0]=0 must be finite and positive", false, [](Owned& o) { o.cameras[1].focal[0] = 0.0f; }},
        {"a negative focal", ALL, INV, "focal[1]=-430 must be finite and positive", false, [](Owned& o) { o.cameras[0].focal[1] = -430.0f; }},
        {"a NaN focal", ALL, INV, "focal[1]=nan must be finite and positive", false, [](Owned& o) { o.cameras[0].focal[1] = NAN; }},
        {"an infinite focal", ALL, INV, "focal[0]=inf must be finite and positive", false, [](Owned& o) { o.cameras[0].focal[0] = INFINITY; }},
        {"no configuration", ALL, INV, "model, prior and cfg are required", false, [](Owned& o) { o.call.cfg = nullptr; }},
        {"no handles", ALL, INV, "model, prior and cfg are required", false, [](Owned& o) { o.call.facts = nullptr; }},
        {"a translation prior", ALL, INV, "transl_prior_weight must be 0 in a chain", false, [](Owned& o) { o.cfg.transl_prior_weight = 1.0f; }},
        {"negative sequences", ALL, INV, "num_sequences=-1", false, [](Owned& o) { o.call.num_sequences = -1; }},
        {"no lengths", ALL, INV, "lengths and offsets are required", false, [](Owned& o) { o.call.lengths = nullptr; }},
        {"no offsets", ALL, INV, "lengths and offsets are required", false, [](Owned& o) { o.call.offsets = nullptr; }},
        {"a negative length", ALL, INV, "lengths[2]=-1", false, [](Owned& o) { o.lengths[2] = -1; }},
        {"offsets that are no prefix sums", ALL, INV, "offsets[2]=4, expected 3 (the exclusive prefix sum of lengths)", false, [](Owned& o) { o.offsets[2] = 4; }},
        {"offsets that do not start at 0", ALL, INV, "offsets[0]=1, expected 0", false, [](Owned& o) { o.offsets[0] = 1; }},
        {"no follow-up iterations", ALL, INV, "followup_iters=0", false, [](Owned& o) { o.call.followup_iters = 0; }},
        {"too many follow-up iterations", ALL, INV, "followup_iters=1048577", false, [](Owned& o) { o.call.followup_iters = (1 << 20) + 1; }},
        {"no first iterations", ALL, INV, "num_iters=0", false, [](Owned& o) { o.cfg.num_iters = 0; }},
        {"no targets", ALL, INV, "num_targets=0 / model_joint_index", false, [](Owned& o) { o.call.K = 0; }},
        {"no joint index", ALL, INV, "num_targets=5 / model_joint_index", false, [](Owned& o) { o.call.index = nullptr; }},
        {"a joint index outside the model", ALL, INV, "model_joint_index[3]=-1 out of range", false, [](Owned& o) { o.index[3] = -1; }},
        {"a surface target (an extra joint)", ALL, UNS, "surface targets (vertex-selected joints, landmarks) are not built into the multi-view term", false,
         [](Owned& o) { o.index[4] = o.facts.J; }},
        {"a 24-joint model without a scan plan", 2, UNS, "built for the fp32 scans only", false, [](Owned&) {}},
        {"NULL targets", ALL & ~2, INV, "NULL parameter / target buffer", false, [](Owned& o) { o.call.targets_null = true; }},
        {"a NULL parameter array", ALL & ~2, INV, "NULL parameter / target buffer", false, [](Owned& o) { o.call.params_null = true; }},
        {"a joint targeted twice", TAKEN, UNS, "k2b_fit_world: joint 1 is targeted twice", false, [](Owned& o) { o.index[2] = 1; }},
        {"bad Adam hyper-parameters", TAKEN, INV, "k2b_fit_world: bad Adam hyper-parameters", false, [](Owned& o) { o.cfg.adam_beta1 = 1.0; }},
    };
    for (const Row& row : rows)
        for (int m = 0; m < 3; ++m) {
            if (!(row.models >> m & 1)) continue;
            Owned o;
            good(o, m);
            row.spoil(o);
            R::Verdict v;
            const int code = R::judge(o.call, v);
            CHECK(code == v.code, "%s (model %d): judge() returned %d, the verdict holds %d", row.what, m, code, v.code);
            CHECK(code == row.code, "%s (model %d): code %d, expected %d (%s)", row.what, m, code, row.code, v.message);
            if (row.code == K2B_OK) {
                CHECK(v.nothing == row.nothing, "%s (model %d): nothing to fit = %d", row.what, m, (int)v.nothing);
                continue;
            }
            CHECK(strstr(v.message, row.message) != nullptr, "%s (model %d): message '%s' lacks '%s'", row.what, m, v.message, row.message);
            // a refusal of the entry's own carries its name in front; the shared path speaks under k2b_fit_world's, as for every entry
            const bool shared = !strncmp(row.message, "k2b_fit_world:", 14);
            CHECK(!strncmp(v.message, shared ? "k2b_fit_world: " : "k2b_fit_multiview_sequences: ", shared ? 15 : 29), "%s (model %d): '%s' does not start with the name", row.what,
                  m, v.message);
        }
    // the first refusal wins in the documented order: the table of sequences, the views, the handles, the chain's numbers, the targets
    {
        Owned o;
        good(o, 0);
        o.offsets[1] = 7; o.call.num_views = 0; o.call.followup_iters = 0;
        R::Verdict v;
        R::judge(o.call, v);
        CHECK(strstr(v.message, "offsets[1]=7") != nullptr, "order: '%s'", v.message);
        o.offsets[1] = 3;
        R::judge(o.call, v);
        CHECK(strstr(v.message, "num_views=0") != nullptr, "order: '%s'", v.message);
        o.call.num_views = 2; o.index[4] = 24;
        R::judge(o.call, v);
        CHECK(strstr(v.message, "followup_iters=0") != nullptr, "order: '%s'", v.message);
    }
    // the fused kernel's 32-bit row index: 2^27 target rows or more in one call are refused, the tree kernel takes them
    for (int m = 0; m < 3; m += 2) {
        Owned o;
        good(o, m, 8);
        o.lengths = {1 << 22, 1}; o.offsets = {0, 1 << 22};            // (2^22 + 1) frames x 8 views x 5 targets > 2^27
        o.call.num_sequences = 2; o.call.lengths = o.lengths.data(); o.call.offsets = o.offsets.data();
        R::Verdict v;
        const int code = R::judge(o.call, v);
        if (m == 0) CHECK(code == K2B_ERR_INVALID_ARGUMENT && strstr(v.message, "4194305 x 8 x 5 target rows") != nullptr, "rows: %d '%s'", code, v.message);
        else CHECK(code == K2B_OK && !v.nothing, "rows on the tree kernel: %d '%s'", code, v.message);
    }
}

// ---- the other ten entries -----------------------------------------------------------------------------------------------------------
static void run_others() {
    CHECK(R::kNumEntries == 11 && (int)R::Entry::fit_multiview_sequences == 10, "the new enumerator is the eleventh");
    CHECK(!strcmp(R::entry_name(R::Entry::fit_multiview_sequences), kName), "entry_name");
    const R::Entry lbfgs[4] = {R::Entry::fit_world_lbfgs, R::Entry::fit_sequence_lbfgs, R::Entry::fit_sequences_lbfgs, R::Entry::shape_pass_lbfgs};
    for (int e = 0; e < R::kNumEntries; ++e) {
        bool want = false;
        for (R::Entry l : lbfgs) want = want || l == (R::Entry)e;
        CHECK(R::is_lbfgs((R::Entry)e) == want, "is_lbfgs(%s)", R::entry_name((R::Entry)e));
    }
    CHECK(R::is_multiview(R::Entry::fit_multiview) && R::is_multiview(R::Entry::fit_multiview_sequences) && !R::is_multiview(R::Entry::fit_image_sequences),
          "is_multiview");
    // Every other entry, on the fused and on the tree model, under projection 0 and 1: the verdict of a call that carries a rig
    // of two cameras is that of the same call without one - they take no views -, and k2b_fit_multiview itself still wants them.
    for (int e = 0; e < 10; ++e)
        for (int m = 0; m < 3; m += 2)
            for (int projection = 0; projection < 2; ++projection) {
                const R::Entry entry = (R::Entry)e;
                R::Verdict with, without;
                for (int rig = 0; rig < 2; ++rig) {
                    Owned o;
                    good(o, m, rig ? 2 : 0, entry);
                    o.cfg.projection = projection;
                    o.cfg.focal[0] = o.cfg.focal[1] = 500.0f;
                    if (!rig) o.call.cameras = nullptr;
                    R::Call& c = o.call;
                    c.B = 2; c.frames_per_sequence = 2;
                    c.max_iter = 30; c.history_size = 100; c.lr = 1.0;
                    c.num_frames = 6; c.num_free_betas = 10;
                    if (entry == R::Entry::shape_pass_lbfgs) { o.offsets = {0, 3, 3, 4, 6}; c.offsets = o.offsets.data(); }
                    R::judge(c, rig ? with : without);
                }
                const char* name = R::entry_name(entry);
                if (entry == R::Entry::fit_multiview) {
                    CHECK(without.code == K2B_ERR_INVALID_ARGUMENT && strstr(without.message, "k2b_fit_multiview: num_views=0") != nullptr, "%s without a rig: '%s'",
                          name, without.message);
                    CHECK(projection == 1 ? with.code == K2B_OK : (with.code == K2B_ERR_INVALID_ARGUMENT && strstr(with.message, "projection=0") != nullptr),
                          "%s with a rig, projection %d: %d '%s'", name, projection, with.code, with.message);
                    continue;
                }
                CHECK(with.code == without.code && with.nothing == without.nothing && !strcmp(with.message, without.message),
                      "%s (model %d, projection %d): a rig changes the verdict: %d '%s' against %d '%s'", name, m, projection, with.code, with.message,
                      without.code, without.message);
                // the projected joint term: built into k2b_fit_world, k2b_fit_image and k2b_fit_image_sequences, refused by name elsewhere
                const bool takes = entry == R::Entry::fit_world || entry == R::Entry::fit_image || entry == R::Entry::fit_image_sequences;
                if (projection == 1 && !takes)
                    CHECK(with.code == K2B_ERR_UNSUPPORTED && strstr(with.message, "the projected joint term") != nullptr && !strncmp(with.message, name, strlen(name)),
                          "%s under projection: %d '%s'", name, with.code, with.message);
                if (projection == 1 && takes) CHECK(with.code == K2B_OK, "%s under projection: %d '%s'", name, with.code, with.message);
                if (projection == 0 && (entry == R::Entry::fit_image || entry == R::Entry::fit_image_sequences))
                    CHECK(with.code == K2B_ERR_INVALID_ARGUMENT && strstr(with.message, "projection=0 must be 1") != nullptr, "%s: '%s'", name, with.message);
                if (projection == 0 && !(entry == R::Entry::fit_image || entry == R::Entry::fit_image_sequences))
                    CHECK(with.code == K2B_OK || (entry == R::Entry::fit_sequences_lbfgs && m == 2 && with.code == K2B_ERR_UNSUPPORTED), "%s on 3D targets: %d '%s'",
                          name, with.code, with.message);
            }
}

int main() {
    run_table();
    run_others();
    printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
