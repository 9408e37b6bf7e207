// Host check of the IK-GAT set-up (csrc/k2b_ikgat_plan.h): the packed weight image, the graph, the LDS map, the launch, the caller's
// layout and the refusals, against expectations written out here on their own - where the caller's tensors lie, what a transposed
// matrix and a folded attention column are, the byte counts of DESIGN.md 4.8 - and against the recordings under tests/golden.
// The image is read back through the accessors the kernel uses.  No HIP call, no device.
// Usage (tests/test_ikgat_plan_host.py):
//   ikgat_plan_check sweep              one line "case <name> J IN H L heads nedges LDX KC F <image hash> <csr hash>" per net, one line
//                                       per section, "N failures" last
//   ikgat_plan_check layout J IN H L    the caller's segments "name layer rows cols", then "total N"
//   ikgat_plan_check refusals FILE      rows "id out J IN H L heads num_weights parents" -> "id<TAB>code<TAB>message"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "k2b_ikgat_plan.h"

using namespace k2b;

static int g_failures = 0;
static char g_where[256];
#define WHERE(...) std::snprintf(g_where, sizeof g_where, __VA_ARGS__)
#define CHECK(cond, ...)                                                        \
    do {                                                                        \
        if (!(cond)) {                                                          \
            if (++g_failures <= 20) {                                           \
                std::printf("FAIL %s: %s  [", g_where, #cond);                  \
                std::printf(__VA_ARGS__);                                       \
                std::printf("]\n");                                             \
            }                                                                   \
        }                                                                       \
    } while (0)
static void section(const char* name, int failures_before) { std::printf("%s: %s\n", name, g_failures == failures_before ? "ok" : "FAILED"); }

// ---- the nets: the shape sweep of DESIGN.md 4.8 -------------------------------------------------------------------------------
enum Graph { tree, star, no_parents, smpl };
struct Case { const char* name; int J, IN, H, L, NH; Graph graph; };
static const Case kCases[] = {
    {"J2_H16_h16", 2, 9, 16, 1, 16, tree},      {"J64_H256_L8", 64, 9, 256, 8, 8, tree},   {"J22_H256", 22, 9, 256, 3, 4, tree},
    {"J55_H208_h13", 55, 3, 208, 2, 13, tree},  {"J24_H48_h3", 24, 9, 48, 3, 3, smpl},     {"J33_H80_h5", 33, 3, 80, 8, 5, tree},
    {"J64_H16_h2", 64, 9, 16, 1, 2, tree},      {"J22_H192_h192", 22, 9, 192, 3, 192, tree}, {"J22_in3", 22, 3, 128, 3, 4, tree},
    {"J1_in3", 1, 3, 16, 1, 1, no_parents},     {"star64", 64, 9, 128, 2, 4, star},        {"chain64", 64, 3, 64, 2, 4, no_parents},
    {"default", 22, 9, 128, 3, 4, smpl},        {"J64_H256_L2", 64, 9, 256, 2, 8, tree},   {"J22_H144_h2", 22, 9, 144, 4, 2, tree},
};
static const int kSmplParents[24] = {-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21};

static std::vector<int32_t> parents_of(const Case& c) {
    std::vector<int32_t> p(c.J, -1);
    for (int i = 1; i < c.J; ++i) p[i] = c.graph == tree ? (i * 7 + 3) % i : c.graph == star ? 0 : c.graph == smpl ? kSmplParents[i] : -1 - i % 3;
    return p;
}
// weights: multiples of 1/1024 in (-1, 1) from a 32-bit linear congruential generator; a product of two has 22 significant bits, so
// a double sum of up to 256 of them is exact and "rounded once" has one meaning
static std::vector<float> weights_of(int64_t n, uint32_t seed) {
    std::vector<float> w((size_t)n);
    uint32_t s = seed * 2654435761u + 12345u;
    for (auto& x : w) { s = s * 1664525u + 1013904223u; x = (float)((int)(s >> 21) - 1024) / 1024.f; }
    return w;
}
static uint64_t fnv1a(const void* data, size_t bytes) {
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < bytes; ++i) h = (h ^ ((const unsigned char*)data)[i]) * 1099511628211ull;
    return h;
}
// the float count of the caller's array, restated from include/k2b.h
static int64_t caller_floats(int J, int IN, int H, int L) {
    const int64_t h = H, h2 = H / 2;
    return (h * IN + h) + J * h + (h * IN + h) + L * (h * h + 5 * h) + (h2 * h + h2) + 2 * h2 + (6 * h2 + 6);
}

#ifndef IKGAT_PLAN_CHECK_CASES_ONLY
static size_t bytes_by_hand(int J, int IN, int H, int LDX, int nedges, int F, int KC) {
    const size_t R = (size_t)F * J;
    return 4 * (R * H + R * LDX + (size_t)KC * LDX + R * IN + R * 4) + 4 * (size_t)(J + 1 + nedges);
}

static void check_image(const Case& c, const IkgatPlan& p, const std::vector<float>& w, const std::vector<float>& dw) {
    const int J = c.J, IN = c.IN, H = c.H, L = c.L, NH = c.NH, C = H / NH, H2 = H / 2, LDX = p.LDX;
    const IkgatImageT<size_t> img = ikgat_image((size_t)0, J, IN, H, L, LDX);   // offsets, as the kernel takes pointers
    CHECK(dw.size() == img.end, "%zu %zu", dw.size(), img.end);
    std::vector<int> seen(dw.size(), 0);
    // piece: `rows` rows of `cols` floats at `at`, `stride` apart, holding expect(row, col)
    const auto piece = [&](const char* what, size_t at, int rows, int cols, int stride, auto expect) {
        for (int r = 0; r < rows; ++r)
            for (int k = 0; k < stride; ++k) {
                const size_t i = at + (size_t)r * stride + k;
                if (i >= dw.size()) { CHECK(false, "%s row %d col %d past the image", what, r, k); return; }
                ++seen[i];
                const float want = k < cols ? expect(r, k) : 0.f;
                if (std::memcmp(&dw[i], &want, 4) != 0) { CHECK(false, "%s row %d col %d: %a, expected %a", what, r, k, dw[i], want); return; }
            }
    };
    const auto as_given = [&](const float* src, int cols) { return [=](int r, int k) { return src[(size_t)r * cols + k]; }; };
    // the caller's tensors (include/k2b.h), walked by hand
    const float* in_w = w.data();
    const float* in_b = in_w + H * IN;
    const float* emb = in_b + H;
    const float* res_w = emb + J * H;
    const float* res_b = res_w + H * IN;
    const float* layers = res_b + H;
    piece("input_proj.weight", img.w_in, H, IN, IN, as_given(in_w, IN));
    piece("input_proj.bias", img.b_in, 1, H, H, as_given(in_b, H));
    piece("joint_pos_embed", img.emb, J, H, H, as_given(emb, H));
    piece("residual_proj.weight", img.w_res, H, IN, IN, as_given(res_w, IN));
    piece("residual_proj.bias", img.b_res, 1, H, H, as_given(res_b, H));
    for (int l = 0; l < L; ++l) {
        const float* W = layers + (size_t)l * (H * H + 5 * H);
        const float *att_src = W + H * H, *att_dst = att_src + H, *bias = att_dst + H;
        const IkgatLayerT<size_t> layer = img.layer(l);
        CHECK(layer.w % 4 == 0, "layer %d at %zu", l, layer.w);
        // [W^T | W^T att_src | W^T att_dst | 0]: column H + hd is head hd's a_src, column H + heads + hd its a_dst
        piece("extended projection", layer.w, H, H + 2 * NH, LDX, [&](int k, int col) {
            if (col < H) return W[(size_t)col * H + k];
            const int hd = (col - H) % NH;
            const float* att = col - H < NH ? att_src : att_dst;
            double s = 0.0;
            for (int ch = hd * C; ch < (hd + 1) * C; ++ch) s += (double)W[(size_t)ch * H + k] * (double)att[ch];
            return (float)s;
        });
        CHECK(ikgat_col_src(H, NH) == H && ikgat_col_dst(H, NH) == H + NH, "%d %d", ikgat_col_src(H, NH), ikgat_col_dst(H, NH));
        piece("gat bias", layer.bias, 1, H, H, as_given(bias, H));
        piece("layer norm weight", layer.lng, 1, H, H, as_given(bias + H, H));
        piece("layer norm bias", layer.lnb, 1, H, H, as_given(bias + 2 * H, H));
    }
    const float* w1 = layers + (size_t)L * (H * H + 5 * H);
    const float *b1 = w1 + H2 * H, *w2 = b1 + 3 * H2, *b2 = w2 + 6 * H2;
    CHECK(img.w1t % 4 == 0 && img.w2t % 4 == 0, "%zu %zu", img.w1t, img.w2t);
    piece("head matrix 1, transposed", img.w1t, H, H2, H2, [&](int k, int col) { return w1[(size_t)col * H + k]; });
    piece("head bias 1", img.b1, 1, H2, H2, as_given(b1, H2));
    piece("head layer norm weight", img.g1, 1, H2, H2, as_given(b1 + H2, H2));
    piece("head layer norm bias", img.be1, 1, H2, H2, as_given(b1 + 2 * H2, H2));
    piece("head matrix 2, transposed, columns 6 and 7 zero", img.w2t, H2, 6, 8, [&](int k, int col) { return w2[(size_t)col * H2 + k]; });
    piece("head bias 2", img.b2, 1, 6, 6, as_given(b2, 6));
    CHECK(b2 + 6 == w.data() + w.size(), "the hand walk ends %td floats from the end", w.data() + w.size() - (b2 + 6));
    size_t once = 0;
    for (int s : seen) once += s == 1;
    CHECK(once == seen.size(), "%zu of %zu floats are covered exactly once", once, seen.size());
}

static void check_csr(const Case& c, const std::vector<int32_t>& par, const std::vector<int>& csr) {
    const int J = c.J;
    // in-neighbours by definition: both ways between a joint and its parent, the chain without any parent, one self loop each
    bool any = false;
    for (int i = 0; i < J; ++i) any = any || par[i] >= 0;
    std::vector<std::vector<char>> edge(J, std::vector<char>(J, 0));       // edge[target][source]
    for (int i = 0; i < J; ++i) {
        if (any && par[i] >= 0) edge[i][par[i]] = edge[par[i]][i] = 1;
        if (!any && i + 1 < J) edge[i][i + 1] = edge[i + 1][i] = 1;
    }
    for (int i = 0; i < J; ++i) edge[i][i] = 1;
    CHECK((int)csr.size() == J + 1 + csr[J] && csr[0] == 0, "%zu", csr.size());
    for (int i = 0; i < J; ++i) {
        int want = 0;
        for (int s = 0; s < J; ++s) want += edge[i][s];
        CHECK(csr[i + 1] - csr[i] == want, "joint %d: %d in-edges, expected %d", i, csr[i + 1] - csr[i], want);
        for (int e = csr[i]; e < csr[i + 1]; ++e) {
            const int s = csr[J + 1 + e];
            CHECK(s >= 0 && s < J && edge[i][s] == 1, "joint %d <- %d", i, s);
            if (s >= 0 && s < J) edge[i][s] = 2;      // (a repeated source fails the line above)
        }
        CHECK(csr[J + 1 + csr[i + 1] - 1] == i, "joint %d: the self loop comes last", i);
    }
}

static void check_lds(const Case& c, const IkgatPlan& p) {
    const int J = c.J, H = c.H, H2 = H / 2;
    WHERE("%s", c.name);
    CHECK(p.KC % 4 == 0 && p.KC >= 4 && p.KC <= H2 && p.KC * p.LDX <= 4096 && (p.KC == H2 || (p.KC + 4) * p.LDX > 4096), "KC %d LDX %d", p.KC, p.LDX);
    CHECK(p.LDX % 4 == 0 && p.LDX >= H + 2 * c.NH && p.LDX < H + 2 * c.NH + 4, "LDX %d", p.LDX);
    for (int F = 1; F <= p.F; ++F) {
        WHERE("%s F %d", c.name, F);
        const IkgatLds m = p.lds(F);
        const size_t R = (size_t)F * J;
        CHECK(m.hb == 0 && m.hb < m.xb && m.xb < m.wb && m.wb < m.xin && m.xin < m.qv && m.qv < m.csr && m.csr < m.end, "order");
        CHECK(m.xb - m.hb == R * H && m.wb - m.xb == R * p.LDX && m.qv - m.xin == R * c.IN && m.csr - m.qv == R * 4 &&
              m.end - m.csr == (size_t)(J + 1 + p.nedges), "region sizes");
        CHECK((4 * m.wb) % 16 == 0, "wb at byte %zu", 4 * m.wb);
        const size_t chunk = m.xin - m.wb;      // the largest k-chunk any of the three block_mm calls stages
        CHECK(chunk >= (size_t)p.KC * p.LDX && chunk >= (size_t)p.KC * H2 && chunk >= (size_t)(p.KC < H2 ? p.KC : H2) * 8, "wb holds %zu floats", chunk);
        CHECK(R * 8 <= m.xb - m.hb, "the head's output rows");
        CHECK(H2 <= p.LDX, "the head's hidden rows");
        CHECK(4 * m.end == bytes_by_hand(J, c.IN, H, p.LDX, p.nedges, F, p.KC), "%zu", 4 * m.end);
        CHECK(4 * m.end <= 160 * 1024 && (F == 1 || 4 * m.end <= 80 * 1024), "%zu B", 4 * m.end);
    }
    WHERE("%s", c.name);
    CHECK(p.F >= 1 && p.F <= 16 && (p.F == 16 || p.lds_bytes(p.F + 1) > 80 * 1024), "F %d", p.F);
}

static void check_launch(const Case& c, const IkgatPlan& p) {
    for (int B = 1; B <= 257; B = B == 35 ? 255 : B == 255 ? 257 : B + 1) {
        WHERE("%s B %d", c.name, B);
        const IkgatLaunch b = ikgat_launch(p, B, false), ch = ikgat_launch(p, B, true);
        CHECK(b.F >= 1 && b.F <= (p.F < B ? p.F : B), "F %d", b.F);
        CHECK(b.grid * b.F >= B && B > (b.grid - 1) * b.F, "grid %d F %d", b.grid, b.F);
        CHECK(b.lds_bytes == p.lds_bytes(b.F) && b.lds_bytes <= 160 * 1024, "%zu", b.lds_bytes);
        CHECK(ch.F == 1 && ch.grid == 1 && ch.lds_bytes == p.lds_bytes(1), "chain F %d grid %d", ch.F, ch.grid);
    }
}

static IkgatPlan plan_of(int J, int IN, int H, int L, int NH, int nedges) { return ikgat_plan(IkgatDims{J, IN, H, L, NH}, nedges); }

// from the formulas as DESIGN.md 4.8 and include/k2b.h state them, worked by hand
static void check_by_hand() {
    WHERE("default net");
    const std::vector<int32_t> par(kSmplParents, kSmplParents + 22);
    const IkgatPlan p = plan_of(22, 9, 128, 3, 4, ikgat_csr(22, par.data())[22]);
    CHECK(p.nedges == 64 && p.LDX == 136 && p.KC == 28 && p.F == 2, "%d %d %d %d", p.nedges, p.LDX, p.KC, p.F);
    CHECK(p.lds_bytes(1) == 39956 && p.lds_bytes(2) == 64332 && p.lds_bytes(3) == 88708, "%zu %zu %zu", p.lds_bytes(1), p.lds_bytes(2), p.lds_bytes(3));
    CHECK(ikgat_segment_offsets(IkgatDims{22, 9, 128, 3, 4}).back() == 65222, "num_weights");
    WHERE("(64,9,256,.,8)");
    const IkgatPlan q = plan_of(64, 9, 256, 2, 8, 190);
    CHECK(q.LDX == 272 && q.KC == 12 && q.F == 1, "%d %d %d", q.LDX, q.KC, q.F);
    WHERE("(64,9,256,.,256)");
    std::vector<int32_t> chain(64);
    for (int i = 0; i < 64; ++i) chain[i] = i - 1;
    IkgatVerdict v;
    const IkgatDims d{64, 9, 256, 1, 256};
    CHECK(ikgat_create_rules(true, d, chain.data(), true, caller_floats(64, 9, 256, 1), v) == K2B_ERR_UNSUPPORTED, "%d", v.code);
    CHECK(std::strstr(v.message, "278780 B") && std::strstr(v.message, "163840"), "%s", v.message);
}

static int sweep() {
    int before = g_failures, n = 0;
    std::vector<IkgatPlan> plans;
    for (const Case& c : kCases) {
        WHERE("%s", c.name);
        const IkgatDims d{c.J, c.IN, c.H, c.L, c.NH};
        const std::vector<int32_t> par = parents_of(c);
        const int64_t nw = ikgat_segment_offsets(d).back();
        CHECK(nw == caller_floats(c.J, c.IN, c.H, c.L), "%lld", (long long)nw);
        const std::vector<float> w = weights_of(nw, (uint32_t)++n);
        IkgatVerdict v;
        CHECK(ikgat_create_rules(true, d, par.data(), true, nw, v) == K2B_OK, "%s", v.message);
        const std::vector<int> csr = ikgat_csr(c.J, par.data());
        const IkgatPlan p = ikgat_plan(d, csr[c.J]);
        const std::vector<float> dw = ikgat_pack(p, w.data());
        std::printf("case %s %d %d %d %d %d %d %d %d %d %016" PRIx64 " %016" PRIx64 "\n", c.name, c.J, c.IN, c.H, c.L, c.NH, p.nedges, p.LDX, p.KC, p.F,
                    fnv1a(dw.data(), 4 * dw.size()), fnv1a(csr.data(), 4 * csr.size()));
        check_image(c, p, w, dw);
        check_csr(c, par, csr);
        plans.push_back(p);
    }
    section("image and graph", before);
    before = g_failures;
    check_by_hand();
    section("values worked by hand", before);
    before = g_failures;
    for (size_t i = 0; i < plans.size(); ++i) check_lds(kCases[i], plans[i]);
    section("LDS map", before);
    before = g_failures;
    for (size_t i = 0; i < plans.size(); ++i) check_launch(kCases[i], plans[i]);
    section("launch", before);
    std::printf("%d failures\n", g_failures);
    return g_failures != 0;
}

static int layout(int J, int IN, int H, int L) {
    const IkgatDims d{J, IN, H, L, 1};
    for (int i = 0; i < ikgat_num_segments(d); ++i) {
        const IkgatSegment s = ikgat_segment(d, i);
        std::printf("%s %d %d %d\n", s.name, s.layer, s.rows, s.cols);
    }
    std::printf("total %lld\n", (long long)ikgat_segment_offsets(d).back());
    return 0;
}

static int refusals(const char* path) {
    std::ifstream in(path);
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream row(line);
        std::string id, par;
        int out = 0;
        IkgatDims d{};
        long long nw = 0;
        row >> id >> out >> d.J >> d.IN >> d.H >> d.L >> d.NH >> nw >> par;
        std::vector<int32_t> parents;
        if (par != "-") {
            std::istringstream list(par);
            for (std::string item; std::getline(list, item, ',');) parents.push_back(std::atoi(item.c_str()));
        }
        IkgatVerdict v;
        ikgat_create_rules(out != 0, d, par == "-" ? nullptr : parents.data(), nw >= 0, nw < 0 ? 0 : nw, v);
        std::printf("%s\t%d\t%s\n", id.c_str(), v.code, v.message);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "sweep")) return sweep();
    if (argc == 6 && !std::strcmp(argv[1], "layout")) return layout(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]));
    if (argc == 3 && !std::strcmp(argv[1], "refusals")) return refusals(argv[2]);
    std::fprintf(stderr, "usage: ikgat_plan_check sweep | layout J IN H L | refusals FILE\n");
    return 2;
}
#endif
