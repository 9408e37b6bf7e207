// Host check of the model handle's table builders (csrc/k2b_tree.h, k2b_scan_plan.h, k2b_model_tables.h): every table against a
// brute-force definition taken from the parent table (or the toy constants) alone.  No HIP call, no device.
// Usage: model_tables_check NAME=p0,p1,... [NAME=...]   one parent table per argument (tests/test_model_tables_host.py).
// Images are checked from the READING side: every element's coordinates are decoded from its index, as a kernel addresses it, and
// its value is computed from the constants - the builders scatter the other way round.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <vector>

#include "k2b_model_tables.h"

using namespace k2b;
using k2b::tables::BackwardImage;
using k2b::tables::BackwardItem;

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

// seeded values in (-1, 1) with a few exact zeros
static float noise(unsigned& s) {
    s = s * 1664525u + 1013904223u;
    return (s >> 28) == 0 ? 0.f : ((int)((s >> 8) & 0xffff) - 32768) / 32768.f;
}
static std::vector<float> noise_vec(size_t n, unsigned seed, float scale = 1.f) {
    std::vector<float> v(n);
    for (float& x : v) x = scale * noise(seed);
    return v;
}

// ---- brute force over the parent table ----------------------------------------------------------------------------------------
static int walk_up(const std::vector<int>& par, int j, int levels) {       // -1 past the root
    for (int s = 0; s < levels && j >= 0; ++s) j = par[j];
    return j;
}
static bool in_subtree(const std::vector<int>& par, int root, int j) {
    for (; j >= 0; j = par[j])
        if (j == root) return true;
    return false;
}

static void check_tree(const std::vector<int>& par, const Tree& t) {
    const int J = (int)par.size();
    CHECK(t.J == J && (int)t.order.size() == J && (int)t.pos.size() == J, "J=%d", J);
    int maxd = 0;
    for (int j = 0; j < J; ++j) {
        int size = 0, depth = 0;
        for (int k = 0; k < J; ++k) size += in_subtree(par, j, k);
        for (int a = par[j]; a >= 0; a = par[a]) ++depth;
        maxd = depth > maxd ? depth : maxd;
        CHECK(t.size[j] == size, "joint %d: size %d, walks say %d", j, t.size[j], size);
        CHECK(t.depth[j] == depth, "joint %d: depth %d, walks say %d", j, t.depth[j], depth);
        CHECK(t.order[t.pos[j]] == j, "joint %d: order[pos] = %d", j, t.order[t.pos[j]]);
        for (size_t c = 0; c < t.children[j].size(); ++c) {
            CHECK(par[t.children[j][c]] == j, "joint %d: child %d", j, t.children[j][c]);
            CHECK(c == 0 || t.children[j][c - 1] < t.children[j][c], "joint %d: children not ascending", j);
        }
        int nchildren = 0;
        for (int k = 0; k < J; ++k) nchildren += par[k] == j;
        CHECK((int)t.children[j].size() == nchildren, "joint %d: %zu children, %d in the table", j, t.children[j].size(), nchildren);
        // DFS window: [pos, pos + size) holds exactly the subtree, the joint first
        CHECK(t.pos[j] + t.size[j] <= J, "joint %d: window past the tree", j);
        for (int l = 0; l < J; ++l)
            CHECK((l >= t.pos[j] && l < t.pos[j] + t.size[j]) == in_subtree(par, j, t.order[l]), "joint %d: position %d", j, l);
        // pre-order with ascending children: a joint's first child follows it, a later child follows the previous one's window
        for (size_t c = 0; c < t.children[j].size(); ++c) {
            const int want = c == 0 ? t.pos[j] + 1 : t.pos[t.children[j][c - 1]] + t.size[t.children[j][c - 1]];
            CHECK(t.pos[t.children[j][c]] == want, "joint %d: child %zu at %d, not %d", j, c, t.pos[t.children[j][c]], want);
        }
        for (int levels = 0; levels <= 17; ++levels)
            CHECK(t.ancestor(j, levels) == walk_up(par, j, levels), "joint %d, %d levels", j, levels);
    }
    CHECK(t.max_depth == maxd, "max depth %d, walks say %d", t.max_depth, maxd);
    for (int d = 0; d < 40; ++d) {
        const int r = rounds_for_depth(d);
        CHECK((1 << r) > d && (r == 0 || (1 << (r - 1)) <= d), "rounds_for_depth(%d) = %d", d, r);
    }
}

static void check_offsets(const std::vector<int>& par, int l, int j, int NB, int stride, const std::vector<float>& jt, const std::vector<float>& jd,
                          const std::vector<float>& dt, const std::vector<float>& dd) {
    for (int c = 0; c < 3; ++c) {
        const int p = j >= 0 ? par[j] : -1;
        const float want = j < 0 ? 0.f : jt[j * 3 + c] - (p >= 0 ? jt[p * 3 + c] : 0.f);
        CHECK(dt[l * 3 + c] == want, "lane %d: dt[%d]", l, c);
        for (int k = 0; k < stride; ++k) {
            const float wd = (j < 0 || k >= NB) ? 0.f : jd[(j * 3 + c) * NB + k] - (p >= 0 ? jd[(p * 3 + c) * NB + k] : 0.f);
            CHECK(dd[(l * 3 + c) * stride + k] == wd, "lane %d: dd[%d][%d]", l, c, k);
        }
    }
}

static void check_tree_tables(const std::vector<int>& par, const Tree& t) {
    const int J = (int)par.size(), NB = 10;
    const std::vector<float> jt = noise_vec((size_t)J * 3, 11), jd = noise_vec((size_t)J * 3 * NB, 12);
    const tables::LaneTables tt = tables::tree_tables(t, NB, jt.data(), jd.data());
    CHECK(tt.tab.size() == 64 * 8 && tt.anc.size() == 64 * 4 && tt.dt.size() == 64 * 3 && tt.dd.size() == 64 * 3 * kMaxShape, "sizes");
    const int before = g_failures;               // the lane map must be sound before rows are read through it
    std::vector<int> lane_of(J, -1);
    for (int l = 0; l < 64; ++l) {
        const int* row = tt.tab.data() + l * 8;
        const int j = row[0];
        CHECK((j >= 0) == (l < J), "lane %d holds joint %d", l, j);
        if (l < J && j >= 0 && j < J) {
            CHECK(lane_of[j] < 0, "joint %d sits in two lanes", j);
            lane_of[j] = l;
        }
    }
    for (int j = 0; j < J; ++j) CHECK(lane_of[j] >= 0, "joint %d has no lane", j);     // with the loop above: lane_of and joint_at are inverse
    if (g_failures != before) return;
    for (int l = 0; l < 64; ++l) {
        const int* row = tt.tab.data() + l * 8;
        const int j = row[0];
        if (j >= 0) {
            CHECK(row[1] == (par[j] >= 0 ? lane_of[par[j]] : 0), "lane %d: parent lane %d", l, row[1]);
            CHECK(row[2] == t.size[j] && row[3] == t.depth[j], "lane %d: size %d depth %d", l, row[2], row[3]);
            for (int k = 0; k < J; ++k)
                CHECK((lane_of[k] >= l && lane_of[k] < l + row[2]) == in_subtree(par, j, k), "lane %d: window and joint %d", l, k);
        } else {
            CHECK(row[1] == 0 && row[2] == 1 && row[3] == 1000, "lane %d: no joint, but %d %d %d", l, row[1], row[2], row[3]);
        }
        for (int c = 4; c < 8; ++c) CHECK(row[c] == -1, "lane %d: column %d of the base table is %d", l, c, row[c]);
        for (int r = 0; r < 4; ++r) {
            // 63 = "none"; a 64-joint tree, whose lane 63 is a joint, keeps "none" everywhere (the kernel's entry refuses it)
            const int a = (j >= 0 && J <= 63) ? walk_up(par, j, 1 << r) : -1;
            CHECK(tt.anc[l * 4 + r] == (a >= 0 ? lane_of[a] : 63), "lane %d: ancestor %d levels up is lane %d", l, 1 << r, tt.anc[l * 4 + r]);
        }
        check_offsets(par, l, j, NB, kMaxShape, jt, jd, tt.dt, tt.dd);
    }
    for (int width : {57, 60, 63}) {
        if (width > 3 * (J - 1)) continue;
        const std::vector<int> tab = tables::tree_tab_with_prior(tt.tab, t, width);
        CHECK(tab.size() == tt.tab.size(), "width %d: size", width);
        for (int l = 0; l < 64; ++l) {
            const int* row = tab.data() + l * 8;
            for (int c = 0; c < 4; ++c) CHECK(row[c] == tt.tab[l * 8 + c], "width %d lane %d: column %d changed", width, l, c);
            CHECK(row[4] == (l < width ? lane_of[1 + l / 3] : -1) && row[5] == (l < width ? l % 3 : -1), "width %d: dimension %d maps to (%d, %d)",
                  width, l, row[4], row[5]);
            const int j = row[0];
            const bool set = j >= 1 && 3 * (j - 1) + 2 < width;
            CHECK(row[6] == (set ? 3 * (j - 1) : -1), "width %d lane %d (joint %d): third column %d", width, l, j, row[6]);
            CHECK(row[7] == -1, "width %d lane %d: last column %d", width, l, row[7]);
        }
    }
}

static void check_fused_tables(const std::vector<int>& par, const Tree& t, const ScanPlan& plan) {
    const int J = (int)par.size(), NB = 10;
    const std::vector<float> jt = noise_vec((size_t)J * 3, 13), jd = noise_vec((size_t)J * 3 * NB, 14);
    const tables::LaneTables f = tables::fused_tables(t, plan, NB, jt.data(), jd.data());
    CHECK(f.tab.size() == 64 * (size_t)kLaneTabStride && f.anc.empty() && f.dt.size() == 64 * 3 && f.dd.size() == 64 * 3 * (size_t)kMaxBetas, "sizes");
    const int before = g_failures;               // the lane map must be sound before rows are read through it
    std::vector<int> lane_of(J, -1);
    for (int l = 0; l < 64; ++l) {
        const int j = f.tab[l * kLaneTabStride];
        CHECK(j < J && (j < 0 || l < kScanLanes), "lane %d holds joint %d", l, j);
        if (j >= 0 && j < J) {
            CHECK(lane_of[j] < 0, "joint %d sits in two lanes", j);
            lane_of[j] = l;
        }
    }
    for (int j = 0; j < J; ++j) CHECK(lane_of[j] >= 0, "joint %d has no lane", j);
    if (g_failures != before) return;
    for (int l = 0; l < 64; ++l) {
        const int* row = f.tab.data() + l * kLaneTabStride;
        const int j = row[0];
        if (j < 0) {
            for (int c = 0; c < kLaneTabStride; ++c) CHECK(row[c] == (c == kLaneTabScan ? 0 : -1), "hole %d: entry %d is %d", l, c, row[c]);
        } else {
            CHECK(row[1] == (par[j] >= 0 ? lane_of[par[j]] : -1), "lane %d: parent lane %d", l, row[1]);
            for (int r = 0; r < kMaxRounds; ++r) {
                const int a = walk_up(par, j, 1 << r);
                CHECK(row[2 + r] == (a >= 0 ? lane_of[a] : -1), "lane %d: ancestor %d levels up is lane %d", l, 1 << r, row[2 + r]);
            }
            CHECK(row[2 + kMaxRounds] == t.size[j] && row[3 + kMaxRounds] == t.depth[j], "lane %d: size / depth", l);
            CHECK(row[kLaneTabScan] == (plan.valid ? plan.flags[l] : 0), "lane %d: scan flags %d", l, row[kLaneTabScan]);
            if (plan.valid) CHECK(plan.lane_of[j] == l && plan.joint_at[l] == j, "lane %d: the plan puts joint %d elsewhere", l, j);
            else CHECK(l == t.pos[j], "lane %d: joint %d is not at its DFS position", l, j);
            // the subtree is the lane window that starts (DFS) or ends (reversed DFS with holes) at the joint
            int first = l, last = l + t.size[j] - 1;
            if (plan.valid) {
                last = l;
                for (int k = 0; k < J; ++k)
                    if (in_subtree(par, j, k) && lane_of[k] < first) first = lane_of[k];
            }
            for (int k = 0; k < J; ++k)
                CHECK((lane_of[k] >= first && lane_of[k] <= last) == in_subtree(par, j, k), "lane %d: window [%d, %d] and joint %d", l, first, last, k);
        }
        check_offsets(par, l, j, NB, kMaxBetas, jt, jd, f.dt, f.dd);
    }
}

// ---- vertex-set images of a toy model -----------------------------------------------------------------------------------------
struct Toy {
    int V, J, NB, P;
    std::vector<float> vt, sd, pd, lw;
    Toy(int V_, int J_, int NB_) : V(V_), J(J_), NB(NB_), P(9 * (J_ - 1)) {
        vt = noise_vec((size_t)V * 3, 21);
        sd = noise_vec((size_t)V * 3 * NB, 22, 0.05f);
        pd = noise_vec((size_t)P * 3 * V, 23, 0.01f);
        lw = noise_vec((size_t)V * J, 24);
        for (float& w : lw) w = std::fabs(w);
    }
};
static k2b_half hi_of(float x) { return (k2b_half)x; }
static k2b_half lo_of(float x) { return (k2b_half)(x - (float)(k2b_half)x); }

static void check_vertex_set(const Toy& m, int wfrags, const std::vector<int>& ids, const std::vector<int>& tag) {
    const int KX = ((m.P + m.NB + 2 + 31) / 32) * 2, n = (int)ids.size(), J = m.J, P = m.P, NB = m.NB;
    const tables::VertexSetShape shape{J, NB, P, KX, wfrags};
    const tables::VertexSetImages im = tables::vertex_set_images(shape, ids, tag, m.vt.data(), m.sd.data(), m.pd.data(), m.lw.data(), m.V);
    // a stream route returns no pdh / pdl: its Pd is checked against the tile route's of the same set
    const tables::VertexSetImages tile = wfrags == 0 ? im : tables::vertex_set_images({J, NB, P, KX, 0}, ids, tag, m.vt.data(), m.sd.data(), m.pd.data(), m.lw.data(), m.V);
    const int vt = (n + 31) / 32;
    CHECK(im.v_tiles == vt, "v_tiles %d", im.v_tiles);
    CHECK(tile.pdh.size() == (size_t)KX * 3 * vt * 512 && tile.pdl.size() == tile.pdh.size(), "Pd size %zu", tile.pdh.size());
    auto tag_of = [&](int i) { return (i < n && !tag.empty()) ? tag[i] : 0; };
    auto weight = [&](int i, int j) { return (i < n && j < J) ? m.lw[(size_t)ids[i] * J + j] : 0.f; };
    // Pd: piece [k-step][coordinate][32-vertex tile], inside it [h][row][8]
    for (size_t e = 0; wfrags == 0 && e < im.pdh.size(); ++e) {
        const size_t frag = e / 512;
        const int h = (int)(e / 256) % 2, row = (int)(e / 8) % 32, kk = (int)e % 8;
        const int ks = (int)(frag / (3 * vt)), c = (int)(frag / vt) % 3, tile = (int)(frag % vt);
        const int k = ks * 16 + h * 8 + kk, i = tile * 32 + row;
        k2b_half wh = (k2b_half)0.f, wl = (k2b_half)0.f;
        if (i < n && k < P + NB + 2) {
            const int v = ids[i];
            const float x = k < P ? m.pd[(size_t)k * 3 * m.V + 3 * v + c] : k < P + NB ? m.sd[((size_t)v * 3 + c) * NB + (k - P)] : m.vt[(size_t)v * 3 + c];
            const float xs = x * kPdScale;
            wh = hi_of(xs); wl = lo_of(xs);
            if (k == P + NB + 1) {                   // what the template's two terms leave over, split again
                const float rest = xs - (float)wh - (float)wl;
                wh = hi_of(rest); wl = lo_of(rest);
            }
        }
        CHECK(im.pdh[e] == wh && im.pdl[e] == wl, "Pd element %zu (k %d, coordinate %d, vertex %d)", e, k, c, i);
        CHECK(e == frag_elem(frag, k, i), "frag_elem(%zu, %d, %d)", frag, k, i);
    }
    if (wfrags == 0) {
        // W2 [16-vertex tile][hi groups | lo groups | ONES | ZERO][16 rows][8 joints]
        const int GA = (J + 7) / 8, NGP = 2 * GA + 2;
        CHECK(im.w2.size() == (size_t)vt * 2 * NGP * 128 && im.spd.empty() && im.sw.empty() && im.nv16 == 0, "tile route: image sizes");
        for (size_t e = 0; e < im.w2.size(); ++e) {
            const int t = (int)(e / ((size_t)NGP * 128)), g = (int)(e / 128) % NGP, r = (int)(e / 8) % 16, k = (int)e % 8, i = t * 16 + r;
            k2b_half want = (k2b_half)0.f;
            if (g < GA) want = hi_of(weight(i, 8 * g + k));
            else if (g < 2 * GA) want = lo_of(weight(i, 8 * (g - GA) + k));
            else if (g == 2 * GA) want = (k2b_half)(k < 3 ? 1.f : 0.f);           // ONES: every row, padding rows too
            else if (k == 0) want = (k2b_half)(float)tag_of(i);                    // ZERO group: the joint tag
            CHECK(im.w2[e] == want, "W2 element %zu (tile %d group %d row %d k %d)", e, t, g, r, k);
        }
        return;
    }
    const int nv16 = (n + 127) / 128 * 8;
    CHECK(im.w2.empty() && im.pdh.empty() && im.pdl.empty() && im.nv16 == nv16, "stream route: a tile image built, or nv16 %d", im.nv16);
    CHECK(im.spd.size() == (size_t)(KX / 2) * nv16 * 6 * 512 && im.sw.size() == (size_t)nv16 * wfrags * 512, "stream route: image sizes");
    // Pd [32-deep k-step][16-vertex tile][coordinate][hi | lo], a piece = [k-group 4][row 16][8]: pdh / pdl re-indexed
    for (size_t e = 0; e < im.spd.size(); ++e) {
        const int kk = (int)e % 8, r = (int)(e / 8) % 16, q = (int)(e / 128) % 4, hl = (int)(e / 512) % 2, c = (int)(e / 1024) % 3;
        const int v16 = (int)(e / 3072) % nv16, ks = (int)(e / ((size_t)3072 * nv16));
        const int k = ks * 32 + q * 8 + kk, i = v16 * 16 + r;
        k2b_half want = (k2b_half)0.f;
        if (i < vt * 32) want = (hl ? tile.pdl : tile.pdh)[frag_elem(((size_t)(k >> 4) * 3 + c) * vt + (i >> 5), k, i)];
        CHECK(im.spd[e] == want, "stream Pd element %zu (k %d, coordinate %d, vertex %d, %s)", e, k, c, i, hl ? "lo" : "hi");
    }
    // W [16-vertex tile][fragment], a piece = [k-group 4][row 16][8].  3 fragments: [hi | ONES], [hi | tag], [lo | 0];
    // 5 fragments: hi_0-3, [hi_4-6 | ONES], lo_0-3, [lo_4-6 | 0], [hi_4-6 | tag]
    for (size_t e = 0; e < im.sw.size(); ++e) {
        const int k = (int)e % 8, r = (int)(e / 8) % 16, g = (int)(e / 128) % 4, frag = (int)(e / 512) % wfrags, v16 = (int)(e / ((size_t)512 * wfrags));
        const int i = v16 * 16 + r;
        const float ones = (i < n && k < 3) ? 1.f : 0.f, tg = k == 0 ? (float)tag_of(i) : 0.f;
        k2b_half want;
        if (wfrags == 3) {
            const float w = weight(i, 8 * g + k);
            want = g == 3 ? (k2b_half)(frag == 0 ? ones : frag == 1 ? tg : 0.f) : (frag == 2 ? lo_of(w) : hi_of(w));
        } else {
            const bool upper = frag == 1 || frag == 3 || frag == 4;
            const float w = weight(i, 8 * (g + (upper ? 4 : 0)) + k);
            if (upper && g == 3) want = (k2b_half)(frag == 1 ? ones : frag == 4 ? tg : 0.f);
            else want = (frag == 2 || frag == 3) ? lo_of(w) : hi_of(w);
        }
        CHECK(im.sw[e] == want, "stream W element %zu (tile %d fragment %d group %d row %d k %d)", e, v16, frag, g, r, k);
        // and the weight decodes back from its two terms
        if (wfrags == 3 && frag == 0 && g < 3 && i < n && 8 * g + k < J) {
            const float w = weight(i, 8 * g + k);
            CHECK((float)im.sw[e] + (float)im.sw[e + 1024] == (float)(k2b_half)w + (float)(k2b_half)(w - (float)(k2b_half)w), "weight (%d, %d) from hi + lo", i, 8 * g + k);
        }
    }
}

static void check_vertex_sets() {
    const Toy toy(40, 20, 5);
    std::vector<int> all(toy.V), tag(toy.V, 0);
    for (int v = 0; v < toy.V; ++v) all[v] = v;
    tag[3] = 1; tag[17] = 2; tag[39] = 3;
    const std::vector<int> some{31, 2, 17, 9, 38, 0, 21};
    for (int wfrags : {0, 3}) {
        g_where = "vertex set, 20 joints, " + std::string(wfrags ? "stream" : "tile") + " route, mesh";
        check_vertex_set(toy, wfrags, all, tag);
        g_where = "vertex set, 20 joints, " + std::string(wfrags ? "stream" : "tile") + " route, subset";
        check_vertex_set(toy, wfrags, some, std::vector<int>());
    }
    const Toy wide(40, 52, 5);                       // joints in the upper k-groups: the five-fragment W
    g_where = "vertex set, 52 joints, stream route, mesh";
    check_vertex_set(wide, 5, all, tag);
    g_where = "vertex set, 52 joints, tile route, subset";
    check_vertex_set(wide, 0, some, std::vector<int>());
}

// ---- surface index ---------------------------------------------------------------------------------------------------------------
static void check_surface_index() {
    g_where = "surface index";
    // extra joints (one pair of weight 1), landmarks (three pairs; zero weights, shared vertices, a vertex twice in one triangle)
    const std::vector<int> pv{7, -1, -1, 12, 5, 7, 5, -1, -1, 30, 31, 12, 7, 7, 2, 40, 41, 42};
    const std::vector<float> pw{1.f, 0.f, 0.f, 0.25f, 0.f, 0.75f, 1.f, 0.f, 0.f, 0.2f, 0.3f, 0.5f, 0.5f, 0.25f, 0.25f, 0.f, 1.f, 0.f};
    const int T = (int)pv.size() / 3;
    const tables::SurfaceIndex ix = tables::surface_index(T, pv, pw);
    std::vector<int> first;
    for (int v : pv)
        if (v >= 0 && std::find(first.begin(), first.end(), v) == first.end()) first.push_back(v);
    CHECK(ix.ids == first, "ids are not the distinct vertices in order of first appearance");
    const int U = (int)ix.ids.size();
    CHECK((int)ix.pair_u.size() == 3 * T && (int)ix.pair_w.size() == 3 * T && (int)ix.inv_off.size() == U + 1, "sizes");
    int nonzero = 0;
    for (int i = 0; i < 3 * T; ++i) {
        if (pv[i] < 0) { CHECK(ix.pair_u[i] == 0 && ix.pair_w[i] == 0.f, "pair %d: unused, but (%d, %g)", i, ix.pair_u[i], ix.pair_w[i]); continue; }
        CHECK(ix.pair_u[i] >= 0 && ix.pair_u[i] < U && ix.ids[ix.pair_u[i]] == pv[i] && ix.pair_w[i] == pw[i], "pair %d", i);
        nonzero += pw[i] != 0.f;
    }
    CHECK(ix.inv_off[0] == 0 && ix.inv_off[U] == nonzero && (int)ix.inv_t.size() == nonzero && (int)ix.inv_w.size() == nonzero, "CSR holds %d pairs, %d have weight",
          ix.inv_off[U], nonzero);
    for (int u = 0; u < U; ++u) {
        CHECK(ix.inv_off[u] <= ix.inv_off[u + 1], "offsets fall at vertex %d", u);
        // the list of vertex u = its pairs of non-zero weight in (target, pair) order: each exactly once, targets ascending
        int at = ix.inv_off[u];
        for (int i = 0; i < 3 * T; ++i)
            if (pv[i] == ix.ids[u] && pw[i] != 0.f) {
                CHECK(at < ix.inv_off[u + 1] && ix.inv_t[at] == i / 3 && ix.inv_w[at] == pw[i], "vertex %d: entry %d is not pair %d", u, at, i);
                ++at;
            }
        CHECK(at == ix.inv_off[u + 1], "vertex %d: %d entries too many", u, ix.inv_off[u + 1] - at);
    }
}

// ---- LBS backward image --------------------------------------------------------------------------------------------------------
static void check_backward_image() {
    g_where = "backward image";
    const int V = 200, chunk = 64;
    // extra joints, then landmark corners: vertices shared between rows, out of order, in every chunk but one
    const std::vector<BackwardItem> items{{150, 24, 1.f}, {3, 25, 1.f}, {64, 26, 1.f}, {199, 27, 1.f}, {3, 28, 0.5f}, {150, 28, 0.25f}, {63, 28, 0.25f},
                                          {64, 29, 0.f}, {3, 29, 0.6f}, {0, 29, 0.4f}};
    const BackwardImage t = tables::lbs_backward_image(items, V, chunk);
    const int n = (int)items.size();
    std::set<int> distinct;
    for (const BackwardItem& it : items) distinct.insert(it.vid);
    const int U = (int)distinct.size(), ncd = (V + chunk - 1) / chunk, ncc = (U + chunk - 1) / chunk;
    const int before = g_failures;
    CHECK(t.n == n && t.U == U, "n %d U %d", t.n, t.U);
    CHECK(t.o_rows == U && t.o_pos_dense == U + n && t.o_pos_compact == U + 2 * n && t.o_off_dense == U + 3 * n && t.o_off_compact == U + 3 * n + ncd + 1 &&
          (int)t.ints.size() == t.o_off_compact + ncc + 1 && (int)t.w.size() == n, "offsets of the image");
    if (g_failures != before) return;
    CHECK(std::vector<int>(t.ints.begin(), t.ints.begin() + U) == std::vector<int>(distinct.begin(), distinct.end()), "vertex list");
    // sorted by vertex, stable: item i of the image is the i-th of the input in (vertex, input position) order
    std::vector<int> used(n, 0);
    for (int i = 0; i < n; ++i) {
        const int vid = t.ints[t.o_pos_dense + i];
        CHECK(i == 0 || t.ints[t.o_pos_dense + i - 1] <= vid, "item %d: not sorted by vertex", i);
        int src = -1;
        for (int k = 0; k < n && src < 0; ++k)
            if (!used[k] && items[k].vid == vid) src = k;            // the first input item of that vertex not yet placed
        CHECK(src >= 0, "item %d: vertex %d has no input item left", i, vid);
        if (src < 0) continue;
        used[src] = 1;
        CHECK(t.ints[t.o_rows + i] == items[src].row && t.w[i] == items[src].w, "item %d: not input item %d (stable order)", i, src);
        CHECK(t.ints[t.ints[t.o_pos_compact + i]] == vid, "item %d: position %d in the list", i, t.ints[t.o_pos_compact + i]);
    }
    for (int set = 0; set < 2; ++set) {
        const int off = set ? t.o_off_compact : t.o_off_dense, pos = set ? t.o_pos_compact : t.o_pos_dense, nc = set ? ncc : ncd;
        for (int c = 0; c <= nc; ++c) {
            int below = 0;
            for (int i = 0; i < n; ++i) below += t.ints[pos + i] < c * chunk;
            CHECK(t.ints[off + c] == below, "%s offsets: chunk %d starts at %d, %d items lie below it", set ? "compact" : "dense", c, t.ints[off + c], below);
            CHECK(c == 0 || t.ints[off + c - 1] <= t.ints[off + c], "%s offsets fall at chunk %d", set ? "compact" : "dense", c);
        }
        CHECK(t.ints[off + nc] == n, "%s offsets end at %d, not %d", set ? "compact" : "dense", t.ints[off + nc], n);
    }
    const BackwardImage none = tables::lbs_backward_image({}, V, chunk);
    CHECK(none.n == 0 && none.U == 0 && (int)none.ints.size() == ncd + 1 + 1 && none.ints[none.o_off_compact] == 0, "a model without surface rows");
}

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: %s NAME=p0,p1,... [...]\n", argv[0]); return 2; }
    for (int a = 1; a < argc; ++a) {
        const std::string arg = argv[a];
        const size_t eq = arg.find('=');
        if (eq == std::string::npos) { std::printf("bad argument %s\n", argv[a]); return 2; }
        const std::string name = arg.substr(0, eq);
        std::vector<int> par;
        for (size_t at = eq + 1; at < arg.size();) {
            size_t used = 0;
            par.push_back(std::stoi(arg.substr(at), &used));
            at += used + 1;
        }
        bool valid = !par.empty() && par[0] < 0 && (int)par.size() <= 64;
        for (size_t j = 1; j < par.size(); ++j) valid = valid && par[j] >= 0 && par[j] < (int)j;
        if (!valid) { std::printf("%s: not a parent table\n", name.c_str()); return 2; }
        const int before = g_failures;
        const Tree t((int)par.size(), par.data());
        g_where = name + ", tree";
        check_tree(par, t);
        g_where = name + ", tree kernel's tables";
        check_tree_tables(par, t);
        bool planned = false;
        if (t.J <= kScanLanes) {
            g_where = name + ", fused kernel's tables, DFS placement";
            check_fused_tables(par, t, ScanPlan());
            const ScanPlan plan = fit_scan_plan(t);
            planned = plan.valid;
            g_where = name + ", fused kernel's tables, scan plan";
            if (plan.valid) check_fused_tables(par, t, plan);
        }
        std::printf("%-8s %2d joints, depth %2d, scan plan %s: %s\n", name.c_str(), t.J, t.max_depth, planned ? "yes" : "no ", g_failures == before ? "ok" : "FAILED");
    }
    check_vertex_sets();
    check_surface_index();
    check_backward_image();
    std::printf("%d failure%s\n", g_failures, g_failures == 1 ? "" : "s");
    return g_failures ? 1 : 0;
}
