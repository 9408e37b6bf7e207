// Host check of csrc/k2b_fit_rules.h, which it includes alone (no HIP runtime, no library): built with the address and
// undefined-behaviour sanitizers by tests/test_fit_rules_host.py.
//
//   fit_rules_check cases FILE   every line of FILE is one call (tests/fit_refusal_cases.py, host_line: the facts of the handles as
//                                integers, the configuration, the call); prints "id<TAB>code<TAB>message" per line.  The test
//                                compares that with the refusals recorded from the entries (tests/golden/fit_refusals.json).
//   fit_rules_check sweep        the accepting side: for every entry and every combination of model x form of the joint term x
//                                frames x targets that the entry can express, whether the rules accept, printed as one table and
//                                held to the table BUILT below, which is written out from the wording of DESIGN.md and
//                                include/k2b.h, not derived from the header.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "k2b_fit_rules.h"

namespace R = k2b::rules;

static const char* const kEntryKeys[R::kNumEntries] = {"fit_world", "fit_sequence", "fit_sequences", "fit_image", "fit_image_sequences", "fit_multiview",
                                                       "fit_world_lbfgs", "fit_sequence_lbfgs", "fit_sequences_lbfgs", "shape_pass_lbfgs"};

// ---- one call with everything it points to ---------------------------------------------------------------------------------------
struct Owned {
    R::Facts facts{};
    k2b_fit_config cfg{};
    std::vector<int> depth;
    std::vector<int32_t> index, lengths, offsets;
    std::vector<k2b_camera> cameras;
    R::Call call;
};

static std::vector<double> numbers(const std::string& s) {
    std::vector<double> out;
    if (s == "-" || s == "null") return out;
    std::stringstream ss(s);
    std::string item;
    while (std::getline(ss, item, ',')) out.push_back(strtod(item.c_str(), nullptr));      // (strtod reads nan and inf)
    return out;
}
template <class T>
static std::vector<T> as(const std::vector<double>& v) {
    std::vector<T> out;
    for (double x : v) out.push_back((T)x);
    return out;
}

static bool parse(const std::string& line, std::string* id, Owned* o) {
    std::map<std::string, std::string> kv;
    std::stringstream ss(line);
    std::string tok;
    while (ss >> tok) {
        const size_t eq = tok.find('=');
        if (eq == std::string::npos) return false;
        kv[tok.substr(0, eq)] = tok.substr(eq + 1);
    }
    auto I = [&](const char* k) { return (int)strtol(kv.at(k).c_str(), nullptr, 10); };
    auto F = [&](const char* k) { return strtod(kv.at(k).c_str(), nullptr); };
    *id = kv.at("id");
    R::Call& c = o->call;
    int e = 0;
    while (e < R::kNumEntries && kv.at("entry") != kEntryKeys[e]) ++e;
    if (e == R::kNumEntries) return false;
    c.entry = (R::Entry)e;
    if (I("facts")) {
        o->depth = as<int>(numbers(kv.at("depth")));
        o->facts = {I("J"), I("E"), I("L"), I("NB"), I("fit_ok") != 0, I("scan64") != 0, o->depth.data(), I("D"), I("M")};
        if ((int)o->depth.size() != o->facts.J) return false;
        c.facts = &o->facts;
    }
    if (I("cfg")) {
        k2b_fit_config& g = o->cfg;
        g.num_iters = I("num_iters"); g.step_size = F("step_size"); g.adam_beta1 = F("adam_beta1"); g.adam_beta2 = F("adam_beta2");
        g.adam_eps = F("adam_eps"); g.freeze_betas = I("freeze_betas"); g.conf_per_frame = I("conf_per_frame");
        const std::vector<double> ai = numbers(kv.at("angle_prior_index")), fo = numbers(kv.at("focal"));
        if (ai.size() != 4 || fo.size() != 2) return false;
        for (int i = 0; i < 4; ++i) g.angle_prior_index[i] = (int)ai[i];
        g.transl_prior_weight = (float)F("transl_prior_weight"); g.debug_launch_shape = I("debug_launch_shape");
        g.prior_pose_dims = I("prior_pose_dims"); g.num_betas_prior = I("num_betas_prior"); g.projection = I("projection");
        g.focal[0] = (float)fo[0]; g.focal[1] = (float)fo[1];
        c.cfg = &o->cfg;
    }
    c.B = I("B"); c.K = I("K");
    if (kv.at("idx") != "null") {
        o->index = as<int32_t>(numbers(kv.at("idx")));
        o->index.push_back(0);                                   // (never read: K counts the entries before it)
        c.index = o->index.data();
    }
    const std::string& nulls = kv.at("null");
    if (c.entry == R::Entry::shape_pass_lbfgs) {                 // seq_offsets, betas_in, betas_out | j3d, global_orient, body_pose, root_targets
        c.params_null = nulls.substr(0, 3).find('1') != std::string::npos;
        c.targets_null = I("N") > 0 && nulls.substr(3).find('1') != std::string::npos;
    } else {                                                     // j3d | the eight parameter arrays
        c.targets_null = nulls[0] == '1';
        c.params_null = nulls.substr(1).find('1') != std::string::npos;
    }
    c.preserve = I("preserve") != 0; c.tr_prior = I("tr_prior") != 0; c.grad_out = I("grad_out") != 0;
    c.followup_iters = I("followup");
    if (c.entry == R::Entry::fit_sequence) { c.B = I("S"); c.frames_per_sequence = I("T"); }
    c.num_sequences = I("S");
    if (kv.at("lengths") != "null") {
        o->lengths = as<int32_t>(numbers(kv.at("lengths")));
        o->offsets = as<int32_t>(numbers(kv.at("offsets")));
        o->lengths.push_back(0); o->offsets.push_back(0);
        c.lengths = o->lengths.data(); c.offsets = o->offsets.data();
    }
    c.max_iter = I("max_iter"); c.history_size = I("history"); c.lr = F("lr");
    c.num_views = I("views");
    if (kv.at("cameras") != "null") {
        std::stringstream cs(kv.at("cameras"));
        std::string one;
        while (std::getline(cs, one, ';')) {
            const std::vector<double> x = numbers(one);
            if (x.size() != 14) return false;
            k2b_camera cam{};
            for (int i = 0; i < 9; ++i) cam.rotation[i] = (float)x[i];
            for (int i = 0; i < 3; ++i) cam.translation[i] = (float)x[9 + i];
            cam.focal[0] = (float)x[12]; cam.focal[1] = (float)x[13];
            o->cameras.push_back(cam);
        }
        c.cameras = o->cameras.data();
    }
    c.num_frames = I("N"); c.root_joint = I("root_joint"); c.num_free_betas = I("free_betas");
    return true;
}

static int run_cases(const char* path) {
    std::ifstream in(path);
    if (!in) { fprintf(stderr, "cannot read %s\n", path); return 2; }
    std::string line;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        Owned o;
        std::string id;
        try {
            if (!parse(line, &id, &o)) { fprintf(stderr, "bad line: %s\n", line.c_str()); return 2; }
        } catch (const std::out_of_range&) {
            fprintf(stderr, "missing field: %s\n", line.c_str());
            return 2;
        }
        R::Verdict v;
        const int code = R::judge(o.call, v);
        if (code != v.code) { fprintf(stderr, "%s: judge() returned %d, the verdict holds %d\n", id.c_str(), code, v.code); return 2; }
        printf("%s\t%d\t%s\n", id.c_str(), v.code, v.code == K2B_OK ? (v.nothing ? "(nothing to fit)" : "(accepted)") : v.message);
    }
    return 0;
}

// ---- what is built ------------------------------------------------------------------------------------------------------------------
// Models: the 24-joint SMPL the fused kernel takes with its fp32 scan plan (F), the same model without a scan plan (K2B_FIT_SCAN64:
// fp64 scans, S), the 55-joint SMPL-X with landmarks on the tree kernel, the prior over the first 63 pose dimensions (X).
// Forms of the joint term: 3D targets, one projected view (cfg.projection = 1), 1 and 8 calibrated views.  Frames: independent, or
// warm-start chains of 2.  Targets: kinematic joints only, or one kinematic joint and one surface target.
enum Form { F3D, PROJ, VIEWS1, VIEWS8 };
static const char* const kFormNames[] = {"3D", "projected", "1 view", "8 views"};
struct Built { R::Entry entry; Form form; bool chain, surface; const char* fsx; };      // fsx: 'Y' / 'N' for models F, S, X
// Every combination an entry can express; what is not listed cannot be asked of that entry at all.  From include/k2b.h and
// the projected term is built into k2b_fit_world (kinematic targets), k2b_fit_image (surface targets too),
// k2b_fit_image_sequences (chains, kinematic) and k2b_fit_multiview (views, kinematic, independent frames), on the tree kernel and
// on the fused kernel's fp32 scans; every other entry is 3D only.  Chains take kinematic targets only; independent frames take
// surface targets under Adam and under L-BFGS (two launches per round).  k2b_fit_sequence_lbfgs falls back to frame-by-frame
// fits, which take what k2b_fit_world_lbfgs takes; k2b_fit_sequences_lbfgs is the one launch of the fused kernel or nothing.  The
// shape pre-pass fits kinematic joints of 3D targets.
static const Built kBuilt[] = {
    {R::Entry::fit_world, F3D, false, false, "YYY"},          {R::Entry::fit_world, F3D, false, true, "YYY"},
    {R::Entry::fit_world, PROJ, false, false, "YNY"},         {R::Entry::fit_world, PROJ, false, true, "NNN"},
    {R::Entry::fit_sequence, F3D, false, false, "YYY"},       {R::Entry::fit_sequence, F3D, false, true, "YYY"},
    {R::Entry::fit_sequence, F3D, true, false, "YYY"},        {R::Entry::fit_sequence, F3D, true, true, "NNN"},
    {R::Entry::fit_sequence, PROJ, false, false, "NNN"},      {R::Entry::fit_sequence, PROJ, false, true, "NNN"},
    {R::Entry::fit_sequence, PROJ, true, false, "NNN"},       {R::Entry::fit_sequence, PROJ, true, true, "NNN"},
    {R::Entry::fit_sequences, F3D, true, false, "YYY"},       {R::Entry::fit_sequences, F3D, true, true, "NNN"},
    {R::Entry::fit_sequences, PROJ, true, false, "NNN"},      {R::Entry::fit_sequences, PROJ, true, true, "NNN"},
    {R::Entry::fit_image, F3D, false, false, "NNN"},          {R::Entry::fit_image, F3D, false, true, "NNN"},
    {R::Entry::fit_image, PROJ, false, false, "YNY"},         {R::Entry::fit_image, PROJ, false, true, "YNY"},
    {R::Entry::fit_image_sequences, F3D, true, false, "NNN"}, {R::Entry::fit_image_sequences, F3D, true, true, "NNN"},
    {R::Entry::fit_image_sequences, PROJ, true, false, "YNY"}, {R::Entry::fit_image_sequences, PROJ, true, true, "NNN"},
    {R::Entry::fit_multiview, VIEWS1, false, false, "YNY"},   {R::Entry::fit_multiview, VIEWS1, false, true, "NNN"},
    {R::Entry::fit_multiview, VIEWS8, false, false, "YNY"},   {R::Entry::fit_multiview, VIEWS8, false, true, "NNN"},
    {R::Entry::fit_world_lbfgs, F3D, false, false, "YYY"},    {R::Entry::fit_world_lbfgs, F3D, false, true, "YYY"},
    {R::Entry::fit_world_lbfgs, PROJ, false, false, "NNN"},   {R::Entry::fit_world_lbfgs, PROJ, false, true, "NNN"},
    {R::Entry::fit_sequence_lbfgs, F3D, true, false, "YYY"},  {R::Entry::fit_sequence_lbfgs, F3D, true, true, "YYY"},
    {R::Entry::fit_sequence_lbfgs, PROJ, true, false, "NNN"}, {R::Entry::fit_sequence_lbfgs, PROJ, true, true, "NNN"},
    {R::Entry::fit_sequences_lbfgs, F3D, true, false, "YYN"}, {R::Entry::fit_sequences_lbfgs, F3D, true, true, "NNN"},
    {R::Entry::fit_sequences_lbfgs, PROJ, true, false, "NNN"}, {R::Entry::fit_sequences_lbfgs, PROJ, true, true, "NNN"},
    {R::Entry::shape_pass_lbfgs, F3D, false, false, "YYY"},   {R::Entry::shape_pass_lbfgs, F3D, false, true, "NNN"},
    {R::Entry::shape_pass_lbfgs, PROJ, false, false, "NNN"},  {R::Entry::shape_pass_lbfgs, PROJ, false, true, "NNN"},
};

static const int kSmplParents[24] = {-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21};
static const int kSmplxParents[55] = {-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 15, 15, 15,
                                      20, 25, 26, 20, 28, 29, 20, 31, 32, 20, 34, 35, 20, 37, 38,
                                      21, 40, 41, 21, 43, 44, 21, 46, 47, 21, 49, 50, 21, 52, 53};

static int run_sweep() {
    int failures = 0;
    std::vector<int> d24(24, 0), d55(55, 0);
    for (int j = 1; j < 24; ++j) d24[j] = d24[kSmplParents[j]] + 1;
    for (int j = 1; j < 55; ++j) d55[j] = d55[kSmplxParents[j]] + 1;
    const R::Facts models[3] = {{24, 21, 0, 10, true, false, d24.data(), 69, 8}, {24, 21, 0, 10, true, true, d24.data(), 69, 8},
                                {55, 72, 51, 20, false, true, d55.data(), 69, 8}};
    const char* const model_names[3] = {"SMPL fused", "SMPL fp64 scans", "SMPL-X tree"};
    std::vector<k2b_camera> cams(8);
    for (k2b_camera& cam : cams) {
        cam = k2b_camera{};
        cam.rotation[0] = cam.rotation[4] = cam.rotation[8] = 1.0f;
        cam.translation[2] = 3.0f;
        cam.focal[0] = 500.0f; cam.focal[1] = 430.0f;
    }
    const int32_t lengths[1] = {2}, offsets[1] = {0};
    printf("%-28s %-10s %-12s %-10s %-16s %s\n", "entry", "form", "frames", "targets", "model", "accepted");
    for (const Built& b : kBuilt)
        for (int m = 0; m < 3; ++m) {
            k2b_fit_config cfg{};                                   // k2b_fit_config_default, restated
            cfg.num_iters = 30; cfg.step_size = 1e-2; cfg.adam_beta1 = 0.9; cfg.adam_beta2 = 0.999; cfg.adam_eps = 1e-8;
            const int angle[4] = {52, 55, 9, 12};
            for (int i = 0; i < 4; ++i) cfg.angle_prior_index[i] = angle[i];
            cfg.optimize_mask = 15;
            if (m == 2) cfg.prior_pose_dims = 63;
            if (b.form != F3D) { cfg.projection = 1; cfg.focal[0] = 500.0f; cfg.focal[1] = 430.0f; }
            const int32_t index[2] = {0, b.surface ? models[m].J : 1};
            R::Call c;
            c.entry = b.entry; c.facts = &models[m]; c.cfg = &cfg;
            c.B = 2; c.K = 2; c.index = index;
            c.frames_per_sequence = b.chain ? 2 : 1; c.followup_iters = 5;
            c.num_sequences = 1; c.lengths = lengths; c.offsets = offsets;
            c.max_iter = 30; c.history_size = 100; c.lr = 1.0;
            if (b.form >= VIEWS1) { c.num_views = b.form == VIEWS1 ? 1 : 8; c.cameras = cams.data(); }
            c.num_frames = 2; c.num_free_betas = 10;
            R::Verdict v;
            const bool accepted = R::judge(c, v) == K2B_OK && !v.nothing;
            printf("%-28s %-10s %-12s %-10s %-16s %s%s%s\n", R::entry_name(b.entry), kFormNames[b.form], b.chain ? "chain" : "independent",
                   b.surface ? "surface" : "kinematic", model_names[m], accepted ? "yes" : "no", accepted ? "" : ": ", accepted ? "" : v.message);
            if (accepted != (b.fsx[m] == 'Y')) {
                ++failures;
                printf("FAIL: the table of what is built says %c\n", b.fsx[m]);
            }
        }
    printf("%d failures\n", failures);
    return failures ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc == 3 && !strcmp(argv[1], "cases")) return run_cases(argv[2]);
    if (argc == 2 && !strcmp(argv[1], "sweep")) return run_sweep();
    fprintf(stderr, "usage: fit_rules_check cases FILE | fit_rules_check sweep\n");
    return 2;
}
