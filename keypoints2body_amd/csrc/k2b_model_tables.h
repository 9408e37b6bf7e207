// Host images of every table a model handle uploads: the lane and ancestor tables of the two fit kernels, the LBS operands of a
// vertex set, the surface term's index and the LBS backward's item image.  Functions from host vectors to host vectors, no
// device call: k2b_api_model.hip and k2b_lbs_backward.hip only allocate and upload what these return, and
// tests/host/model_tables_check.cpp checks every table against its definition without a GPU.
#pragma once
#include <algorithm>
#include <map>
#include <vector>

#include "k2b_layout.h"
#include "k2b_lbs_fp8.h"
#include "k2b_scan_plan.h"

namespace k2b {
namespace tables {

// ---- fit kernels: tables indexed by lane ---------------------------------------------------------------------------------------
// Lane l's rows of an offset table pair, dt [64][3] and dd [64][3][stride]: the rest position of joint j minus its parent's
// (p < 0, the root: its own), and the same for the NB shape directions.  jt [J][3], jd [J][3][NB].
inline void offset_to_parent(int l, int j, int p, int NB, int stride, const float* jt, const float* jd, float* dt, float* dd) {
    for (int c = 0; c < 3; ++c) {
        dt[l * 3 + c] = jt[j * 3 + c] - (p >= 0 ? jt[p * 3 + c] : 0.f);
        for (int k = 0; k < NB; ++k) dd[(l * 3 + c) * stride + k] = jd[(j * 3 + c) * NB + k] - (p >= 0 ? jd[(p * 3 + c) * NB + k] : 0.f);
    }
}
// out[r]: lane of the ancestor 2^r levels above joint j (pointer doubling), `none` once past the root
inline void ancestor_lanes(const Tree& t, int j, const std::vector<int>& lane_of, int rounds, int none, int* out) {
    for (int r = 0; r < rounds; ++r) {
        const int a = t.ancestor(j, 1 << r);
        out[r] = a >= 0 ? lane_of[a] : none;
    }
}

// The tables of a fit kernel over 64 lanes, no lane holding a joint yet: tab [64][tab_stride] (-1), anc [64][anc_stride] (`none`),
// dt [64][3] and dd [64][3][dd_stride] (zero)
struct LaneTables {
    std::vector<int> tab, anc;
    std::vector<float> dt, dd;
    LaneTables(int tab_stride, int anc_stride, int none, int dd_stride)
        : tab((size_t)64 * tab_stride, -1), anc((size_t)64 * anc_stride, none), dt((size_t)64 * 3, 0.f), dd((size_t)64 * 3 * dd_stride, 0.f) {}
};
// Fused kernel (FitArgs: lane_tab = tab, dt, dd; its ancestors are columns of tab).  As they come from here: the tables of a model
// the kernel does not take.
inline LaneTables fused_tables_empty() {
    LaneTables f(kLaneTabStride, 0, 0, kMaxBetas);
    for (int l = 0; l < 64; ++l) f.tab[(size_t)l * kLaneTabStride + kLaneTabScan] = 0;
    return f;
}
// Lane placement.  With a valid scan plan (k2b_scan_plan.h): reversed DFS order with holes, the subtree sums are fp32 chain / end
// scans.  Without one (a junction inside a limb, a chain of more than 8 joints, ...): DFS order, where every subtree is the lane
// range that starts at its joint, and the fp64 prefix differences.  At most 32 joints, NB <= kMaxBetas.
inline LaneTables fused_tables(const Tree& t, const ScanPlan& plan, int NB, const float* jt, const float* jd) {
    LaneTables f = fused_tables_empty();
    const std::vector<int>& lane_of = plan.valid ? plan.lane_of : t.pos;
    for (int l = 0; l < kScanLanes; ++l) {
        const int j = plan.valid ? plan.joint_at[l] : (l < t.J ? t.order[l] : -1);
        if (j < 0) continue;                         // a hole or a lane beyond the tree: no joint, zero offset, identity transform
        const int p = t.parents[j];
        int* row = f.tab.data() + (size_t)l * kLaneTabStride;
        row[0] = j;
        row[1] = p >= 0 ? lane_of[p] : -1;
        ancestor_lanes(t, j, lane_of, kMaxRounds, -1, row + 2);
        row[2 + kMaxRounds] = t.size[j];             // DFS placement: subtree = lanes [l, l + size)
        row[3 + kMaxRounds] = t.depth[j];
        row[kLaneTabScan] = plan.valid ? plan.flags[l] : 0;
        offset_to_parent(l, j, p, NB, kMaxBetas, jt, jd, f.dt.data(), f.dd.data());
    }
    return f;
}

// Tree kernel (FitTreeArgs: tab, anc, dt, dd), lanes in DFS pre-order, up to 64 joints.  tab [64][8] with empty prior columns
// (tree_tab_with_prior fills them per width); anc [64][4]: ancestors 1, 2, 4, 8 levels up, 63 = "none": a lane that is no joint
// and holds the identity (left at 63 throughout for a 64-joint tree, which the kernel's entry refuses).
inline LaneTables tree_tables(const Tree& t, int NB, const float* jt, const float* jd) {
    LaneTables o(8, 4, 63, kMaxShape);
    for (int l = 0; l < 64; ++l) { o.tab[l * 8 + 1] = 0; o.tab[l * 8 + 2] = 1; o.tab[l * 8 + 3] = 1000; }
    for (int l = 0; l < t.J; ++l) {
        const int j = t.order[l], p = t.parents[j];
        o.tab[l * 8 + 0] = j; o.tab[l * 8 + 1] = p >= 0 ? t.pos[p] : 0; o.tab[l * 8 + 2] = t.size[j]; o.tab[l * 8 + 3] = t.depth[j];
        offset_to_parent(l, j, p, NB, kMaxShape, jt, jd, o.dt.data(), o.dd.data());
        if (t.J <= 63) ancestor_lanes(t, j, t.pos, 4, 63, o.anc.data() + l * 4);
    }
    return o;
}
// The lane table for a prior over the first `width` pose dimensions (a multiple of 3 in 3..63, at most 3 (J - 1)).  Row i,
// columns 4 and 5: prior dimension i is component i % 3 of joint 1 + i / 3, read from that joint's lane; column 6 of a joint's
// lane: its first prior dimension when all three of them are inside the width, else -1.
inline std::vector<int> tree_tab_with_prior(std::vector<int> tab, const Tree& t, int width) {
    for (int i = 0; i < width; ++i) {
        tab[i * 8 + 4] = t.pos[1 + i / 3];
        tab[i * 8 + 5] = i % 3;
    }
    for (int j = 1; j < t.J; ++j)
        if (3 * (j - 1) + 2 < width) tab[t.pos[j] * 8 + 6] = 3 * (j - 1);
    return tab;
}

// ---- LBS operands of a vertex set ----------------------------------------------------------------------------------------------
struct VertexSetShape {
    int J, NB, P, KX;                        // joints, shape coefficients, pose features 9 (J - 1), 16-deep k-steps of the features
    int wfrags;                              // W fragments per 16-vertex tile of the model's stream kernel (3: 17-24 joints, 5: 49-56); 0: tile kernel
    bool pose_fp8 = false;                   // wfrags 3 only (LbsRouteRecord::pose_fp8): the lo strips of the k-steps 0..5 of spd as e4m3
    bool pd8_given = false;                  // pose_fp8: take the two scales below instead of choosing them from this set - a subset of the
    int pd8_lo_exp = 0, pd8_hi_exp = 0;      // mesh (extra joints, landmark vertices) gets the mesh's codes, bit for bit
};
// B operands (f16 hi/lo, MFMA fragment order; k2b_lbs.hip, k2b_lbs_stream.hip), the images of the model's route alone: the tile
// kernel reads pdh / pdl (Pd fragments [KX][3][v_tiles]) and w2; a stream kernel reads spd (pdh / pdl re-indexed) and sw.
struct VertexSetImages {
    int v_tiles = 0, nv16 = 0;               // 32-vertex tiles; 16-vertex tiles of the stream images (whole 128-vertex groups)
    std::vector<k2b_half> pdh, pdl, w2, spd, sw;
    int pd8_lo_exp = 0, pd8_hi_exp = 0;      // pose_fp8: the power-of-two scales of the e4m3 strips, Pd_lo8 = e4m3(Pd_lo / 2^lo_exp)
};

// The e4m3 strips of a stream image (k2b_lbs_fp8.h): for the k-steps 0..kF8PoseSteps - 1 the 1 KiB f16 lo piece of every
// (k-step, 16-vertex tile, coordinate) is replaced by [lane group g][vertex row 16][16 bytes] with g 0, 1 = Pd_lo8 of the
// features 0..15 and 16..31 of the k-step and g 2, 3 = Pd_hi8 of the same - the codes of the f16 terms the piece pair held, one
// scale per term for the whole image, chosen from the term's largest magnitude unless given.  spd [k-step][nv16][3][hi | lo][512 halfs].
inline void pose_fp8_strips(VertexSetImages& o, bool given, int lo_exp, int hi_exp) {
    const size_t pairs = (size_t)kF8PoseSteps * o.nv16 * 3;
    float max_lo = 0.f, max_hi = 0.f;
    for (size_t p = 0; p < pairs; ++p)
        for (int e = 0; e < 512; ++e) {
            const float hi = (float)o.spd[p * 1024 + e], lo = (float)o.spd[p * 1024 + 512 + e];
            max_hi = std::max(max_hi, hi < 0 ? -hi : hi);
            max_lo = std::max(max_lo, lo < 0 ? -lo : lo);
        }
    o.pd8_lo_exp = given ? lo_exp : e4m3_scale_exp(max_lo);
    o.pd8_hi_exp = given ? hi_exp : e4m3_scale_exp(max_hi);
    for (size_t p = 0; p < pairs; ++p) {
        k2b_half* hi = o.spd.data() + p * 1024;
        uint8_t strip[1024];
        for (int r = 0; r < 16; ++r)
            for (int k = 0; k < 32; ++k) {
                const int src = (((k >> 3) & 3) * 16 + r) * 8 + (k & 7);          // f16 operand order: lane = row + 16 k-group, 8 halfs
                strip[((k >> 4) * 16 + r) * 16 + (k & 15)] = e4m3_encode_scaled((float)hi[512 + src], o.pd8_lo_exp);
                strip[((2 + (k >> 4)) * 16 + r) * 16 + (k & 15)] = e4m3_encode_scaled((float)hi[src], o.pd8_hi_exp);
            }
        unsigned char* dst = reinterpret_cast<unsigned char*>(hi + 512);
        for (int i = 0; i < 1024; ++i) dst[i] = strip[i];
    }
}
// Vertex i of the set is row ids[i] of the constants (posedirs row stride 3 * V).  tag[i] = 1 + e when vertex i is the vertex of
// output joint J + e (mesh set only), else 0; an empty tag: none.
inline VertexSetImages vertex_set_images(const VertexSetShape& s, const std::vector<int>& ids, const std::vector<int>& tag, const float* v_template,
                                         const float* shapedirs, const float* posedirs, const float* lbs_weights, int V) {
    const int KX = s.KX, P = s.P, NB = s.NB, J = s.J, n = (int)ids.size();
    VertexSetImages o;
    o.v_tiles = (n + 31) / 32;
    const int vp = o.v_tiles * 32;
    auto &pdh = o.pdh, &pdl = o.pdl;
    pdh.assign((size_t)KX * 3 * vp * 16, (k2b_half)0.f);
    pdl.assign(pdh.size(), (k2b_half)0.f);
    for (int i = 0; i < n; ++i) {
        const int v = ids[i];
        for (int c = 0; c < 3; ++c) {
            auto put = [&](int k, k2b_half hi, k2b_half lo) {
                const size_t e = frag_elem(((size_t)(k >> 4) * 3 + c) * o.v_tiles + (i >> 5), k, i);
                pdh[e] = hi;
                pdl[e] = lo;
            };
            auto split = [&](int k, float x) -> float {   // returns what two f16 terms leave over
                const float xs = x * kPdScale;
                const k2b_half hi = (k2b_half)xs;
                const k2b_half lo = (k2b_half)(xs - (float)hi);
                put(k, hi, lo);
                return xs - (float)hi - (float)lo;
            };
            for (int k = 0; k < P; ++k) split(k, posedirs[(size_t)k * 3 * V + 3 * v + c]);
            for (int k = 0; k < NB; ++k) split(P + k, shapedirs[((size_t)v * 3 + c) * NB + k]);
            const float rest = split(P + NB, v_template[(size_t)v * 3 + c]);
            // the template is metre-scale: keep its third term as an extra K row (feature = 1)
            const k2b_half rh = (k2b_half)rest;
            put(P + NB + 1, rh, (k2b_half)(rest - (float)rh));
        }
    }
    if (s.wfrags == 0) {
        // tile-kernel layout of W: [16-vertex tile][hi groups | lo groups | ONES | ZERO][16 rows][8 joints]
        const int GA = tile_groups_a(J), NGP = tile_ngp(GA), v16 = o.v_tiles * 2;
        o.w2.assign((size_t)v16 * NGP * 128, (k2b_half)0.f);
        for (int t = 0; t < v16; ++t)
            for (int r = 0; r < 16; ++r) {
                const int i = t * 16 + r;
                k2b_half* rowp = o.w2.data() + ((size_t)t * NGP * 16 + r) * 8;
                if (i < n)
                    for (int j = 0; j < J; ++j) {
                        const float w = lbs_weights[(size_t)ids[i] * J + j];
                        const k2b_half hi = (k2b_half)w;
                        rowp[(size_t)(j >> 3) * 128 + (j & 7)] = hi;
                        rowp[(size_t)(GA + (j >> 3)) * 128 + (j & 7)] = (k2b_half)(w - (float)hi);
                    }
                for (int k = 0; k < 3; ++k) rowp[(size_t)(2 * GA) * 128 + k] = (k2b_half)1.f;   // ONES: picks up the PAD terms
                if (i < n && !tag.empty() && tag[i]) rowp[(size_t)(2 * GA + 1) * 128] = (k2b_half)(float)tag[i];   // ZERO group: joint tag
            }
        return o;
    }
    // stream kernels: Pd [k-step][16-vertex tile][coord][hi | lo] and W [16-vertex tile][3 or 5 fragments], 1 KiB pieces in
    // MFMA operand order (lane = row + 16 k-group, 8 halfs); vertex tiles padded to whole 128-vertex groups
    const bool three = s.wfrags == 3;
    const int nv16 = (n + 127) / 128 * 8, SK = KX / 2, NWF = s.wfrags;
    o.nv16 = nv16;
    o.spd.assign((size_t)SK * nv16 * 6 * 512, (k2b_half)0.f);
    o.sw.assign((size_t)nv16 * NWF * 512, (k2b_half)0.f);
    for (int i = 0; i < n; ++i) {
        const int v16 = i >> 4, r = i & 15;
        for (int c = 0; c < 3; ++c)
            for (int k = 0; k < KX * 16; ++k) {      // the split values already sit in pdh / pdl: same k, same scale
                const size_t src = frag_elem(((size_t)(k >> 4) * 3 + c) * o.v_tiles + (i >> 5), k, i);
                const size_t dst = ((((size_t)(k >> 5) * nv16 + v16) * 3 + c) * 2) * 512 + (size_t)((((k >> 3) & 3) * 16 + r) * 8 + (k & 7));
                o.spd[dst] = pdh[src];
                o.spd[dst + 512] = pdl[src];
            }
        k2b_half* wt = o.sw.data() + (size_t)v16 * NWF * 512;
        auto at = [&](int frag, int group, int k) -> k2b_half& { return wt[(size_t)frag * 512 + (size_t)((group * 16 + r) * 8 + k)]; };
        for (int j = 0; j < J; ++j) {
            const float w = lbs_weights[(size_t)ids[i] * J + j];
            const k2b_half hi = (k2b_half)w, lo = (k2b_half)(w - (float)hi);
            const int gj = j >> 3, kj = j & 7;
            if (three) { at(0, gj, kj) = hi; at(1, gj, kj) = hi; at(2, gj, kj) = lo; }
            else if (gj < 4) { at(0, gj, kj) = hi; at(2, gj, kj) = lo; }
            else { at(1, gj - 4, kj) = hi; at(4, gj - 4, kj) = hi; at(3, gj - 4, kj) = lo; }
        }
        // last group of the fragment that meets the PAD group of A: ONES; of the one that meets ZERO: the joint tag
        for (int k = 0; k < 3; ++k) at(three ? 0 : 1, 3, k) = (k2b_half)1.f;
        if (!tag.empty() && tag[i]) at(three ? 1 : 4, 3, 0) = (k2b_half)(float)tag[i];
    }
    pdh.clear();
    pdl.clear();
    if (three && s.pose_fp8) pose_fp8_strips(o, s.pd8_given, s.pd8_lo_exp, s.pd8_hi_exp);
    return o;
}

// ---- surface term (k2b_surface.hip) ----------------------------------------------------------------------------------------
// Index of T targets that are weighted sets of up to 3 vertices.  pair_v / pair_w [T][3]: vertex and weight of target t's pair k
// (vertex < 0: no pair).  ids: the U distinct vertices in order of first appearance; pair_u [T][3]: slot of every pair in ids
// (no pair: slot 0, weight 0); inv_*: the pairs of non-zero weight by vertex, as CSR over the slots, in target order.
struct SurfaceIndex {
    std::vector<int> ids, pair_u, inv_off, inv_t;
    std::vector<float> pair_w, inv_w;
};
inline SurfaceIndex surface_index(int T, const std::vector<int>& pair_v, const std::vector<float>& pair_w) {
    SurfaceIndex o;
    o.pair_u.assign(3 * T, 0);
    o.pair_w.assign(3 * T, 0.f);
    std::map<int, int> slot;
    for (int i = 0; i < 3 * T; ++i) {
        if (pair_v[i] < 0) continue;
        auto ins = slot.emplace(pair_v[i], (int)o.ids.size());
        if (ins.second) o.ids.push_back(pair_v[i]);
        o.pair_u[i] = ins.first->second;
        o.pair_w[i] = pair_w[i];
    }
    const int U = (int)o.ids.size();
    o.inv_off.assign(U + 1, 0);
    for (int i = 0; i < 3 * T; ++i)
        if (o.pair_w[i] != 0.f) ++o.inv_off[o.pair_u[i] + 1];
    for (int u = 0; u < U; ++u) o.inv_off[u + 1] += o.inv_off[u];
    o.inv_t.resize(o.inv_off[U]);
    o.inv_w.resize(o.inv_off[U]);
    std::vector<int> fill(o.inv_off.begin(), o.inv_off.end() - 1);
    for (int i = 0; i < 3 * T; ++i)
        if (o.pair_w[i] != 0.f) {
            const int at = fill[o.pair_u[i]]++;
            o.inv_t[at] = i / 3;
            o.inv_w[at] = o.pair_w[i];
        }
    return o;
}

// ---- LBS backward (k2b_lbs_backward.hip) -------------------------------------------------------------------------------------
// The rows of grad_joints that are vertices (extra joints, landmark corners), sorted by vertex (stable), for both vertex sets of
// the dense launch: the whole mesh of V vertices and the compact list of the U distinct vertices, each cut into chunks.
struct BackwardItem { int vid, row; float w; };
struct BackwardOffsets {
    int U = 0, n = 0;                        // distinct vertices, items
    int o_rows = 0, o_pos_dense = 0, o_pos_compact = 0, o_off_dense = 0, o_off_compact = 0;
};
// ints: vertex list [U] | rows [n] | positions in the mesh [n] | positions in the list [n] | item offsets per chunk of the mesh
// | per chunk of the list (one entry more than chunks each, the last one n); w [n]: weight of every item
struct BackwardImage : BackwardOffsets {
    std::vector<int> ints;
    std::vector<float> w;
};
inline BackwardImage lbs_backward_image(std::vector<BackwardItem> items, int V, int chunk) {
    std::stable_sort(items.begin(), items.end(), [](const BackwardItem& x, const BackwardItem& y) { return x.vid < y.vid; });
    BackwardImage t;
    const int n = (int)items.size();
    std::vector<int> vlist;
    for (const BackwardItem& it : items)
        if (vlist.empty() || vlist.back() != it.vid) vlist.push_back(it.vid);
    const int U = (int)vlist.size();
    const int nc_dense = (V + chunk - 1) / chunk, nc_compact = (U + chunk - 1) / chunk;
    t.U = U; t.n = n;
    t.o_rows = U; t.o_pos_dense = U + n; t.o_pos_compact = U + 2 * n; t.o_off_dense = U + 3 * n; t.o_off_compact = t.o_off_dense + nc_dense + 1;
    t.ints.resize((size_t)t.o_off_compact + nc_compact + 1);
    t.w.resize(n);
    std::copy(vlist.begin(), vlist.end(), t.ints.begin());
    for (int i = 0, u = 0; i < n; ++i) {
        while (vlist[u] != items[i].vid) ++u;
        t.ints[t.o_rows + i] = items[i].row;
        t.ints[t.o_pos_dense + i] = items[i].vid;
        t.ints[t.o_pos_compact + i] = u;
        t.w[i] = items[i].w;
    }
    auto chunk_offsets = [&](int pos, int off, int chunks) {     // off[c]: the first item at or behind position c * chunk of its vertex set
        for (int c = 0, i = 0; c <= chunks; ++c) {
            while (i < n && t.ints[pos + i] < c * chunk) ++i;
            t.ints[off + c] = i;
        }
    };
    chunk_offsets(t.o_pos_dense, t.o_off_dense, nc_dense);
    chunk_offsets(t.o_pos_compact, t.o_off_compact, nc_compact);
    return t;
}

}  // namespace tables
}  // namespace k2b
