// k2b_ikgat_plan.h — the set-up of the IK-GAT regressor (k2b_ikgat_create / k2b_ikgat_predict, k2b_ikgat.hip) as pure functions:
// what the two entries refuse, the order of the caller's weights, where each piece of the packed device image lies, the packer,
// the graph, the LDS map of a workgroup and the choice of LDX, KC, F and the launch.  The ONE statement of each:
// the entries execute these functions, the kernel takes its weight pointers and its LDS regions from the same descriptions, and
// tests/host/ikgat_plan_check.cpp holds them to expectations written out independently, without a GPU.
// No HIP runtime: a plain host C++17 program may include this header alone.
#pragma once
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/k2b.h"
#include "k2b_launch_plan.h"   // K2B_HD, ceil_div

namespace k2b {

constexpr size_t kIkgatMaxLds = 160 * 1024;       // one workgroup's LDS: a net whose single frame needs more is refused
constexpr size_t kIkgatBatchLds = 80 * 1024;      // two workgroups per CU for batched launches: F grows while F frames fit in this
constexpr int kIkgatMaxFrames = 16;               // ... and up to this
constexpr int kIkgatChunkFloats = 4096;           // weights staged per k-chunk: KC * (columns) <= this
constexpr int kIkgatOutCols = 8;                  // the head's last matrix: 6 outputs padded to a multiple of 4 columns

struct IkgatDims { int J, IN, H, L, NH; };        // joints, input width (3 or 9), hidden width, GAT layers, heads

// ---- the caller's layout: the state dict's tensors, row-major, concatenated in this order (include/k2b.h) ---------------------------
enum IkgatInputSeg { kSegInW, kSegInB, kSegEmb, kSegResW, kSegResB, kIkgatInputSegs };
enum IkgatLayerSeg { kSegLin, kSegAttSrc, kSegAttDst, kSegBias, kSegLnW, kSegLnB, kIkgatLayerSegs };
enum IkgatHeadSeg { kSegH0W, kSegH0B, kSegH2W, kSegH2B, kSegH4W, kSegH4B, kIkgatHeadSegs };
struct IkgatSegment { const char* name; int layer; int rows, cols; };      // layer: -1 outside the GAT layers ("l" in the name)
inline int ikgat_num_segments(const IkgatDims& d) { return kIkgatInputSegs + d.L * kIkgatLayerSegs + kIkgatHeadSegs; }
inline IkgatSegment ikgat_segment(const IkgatDims& d, int i) {
    const int J = d.J, IN = d.IN, H = d.H, H2 = H / 2;
    const IkgatSegment input[kIkgatInputSegs] = {{"input_proj.weight", -1, H, IN}, {"input_proj.bias", -1, 1, H}, {"joint_pos_embed.weight", -1, J, H},
                                                 {"residual_proj.weight", -1, H, IN}, {"residual_proj.bias", -1, 1, H}};
    const IkgatSegment layer[kIkgatLayerSegs] = {{"gat_layers.l.lin.weight", 0, H, H}, {"gat_layers.l.att_src", 0, 1, H}, {"gat_layers.l.att_dst", 0, 1, H},
                                                 {"gat_layers.l.bias", 0, 1, H}, {"layer_norms.l.weight", 0, 1, H}, {"layer_norms.l.bias", 0, 1, H}};
    const IkgatSegment head[kIkgatHeadSegs] = {{"output_head.0.weight", -1, H2, H}, {"output_head.0.bias", -1, 1, H2}, {"output_head.2.weight", -1, 1, H2},
                                               {"output_head.2.bias", -1, 1, H2}, {"output_head.4.weight", -1, 6, H2}, {"output_head.4.bias", -1, 1, 6}};
    if (i < kIkgatInputSegs) return input[i];
    i -= kIkgatInputSegs;
    if (i >= d.L * kIkgatLayerSegs) return head[i - d.L * kIkgatLayerSegs];
    IkgatSegment s = layer[i % kIkgatLayerSegs];
    s.layer = i / kIkgatLayerSegs;
    return s;
}
// start of every segment in the caller's array, and the array's length last
inline std::vector<int64_t> ikgat_segment_offsets(const IkgatDims& d) {
    std::vector<int64_t> off(1, 0);
    for (int i = 0; i < ikgat_num_segments(d); ++i) off.push_back(off.back() + (int64_t)ikgat_segment(d, i).rows * ikgat_segment(d, i).cols);
    return off;
}

// ---- the choices -----------------------------------------------------------------------------------------------------------------
// columns of a GAT layer's extended projection: H of x', heads of a_src, heads of a_dst, padded to a multiple of 4
K2B_HD constexpr int ikgat_ldx(int H, int heads) { return (H + 2 * heads + 3) & ~3; }
K2B_HD constexpr int ikgat_col_src(int H, int /*heads*/) { return H; }
K2B_HD constexpr int ikgat_col_dst(int H, int heads) { return H + heads; }
// rows of a staged k-chunk: a multiple of 4 (block_mm reads k in fours), >= 4 since LDX <= 3 H + 3 <= 771
K2B_HD constexpr int ikgat_kc(int H, int ldx) {
    const int fit = (kIkgatChunkFloats / ldx) & ~3;
    return H / 2 < fit ? H / 2 : fit;
}

// ---- the LDS map of one workgroup of F frames (R = F J node rows) -----------------------------------------------------------------
// P: float* from the start of dynamic LDS (the kernel carves its regions from it, as the pointer chain it has always walked: its
// registers do not move), or size_t from 0 for offsets in 4-byte words
template <class P>
struct IkgatLdsT {
    P hb;       // [R][H]    node features h; the head's 6 outputs (stride kIkgatOutCols) at the end
    P xb;       // [R][LDX]  x' | a_src | a_dst of a GAT layer, then the head's hidden layer
    P wb;       // [KC][LDX] staged weight chunk (16-byte loads)
    P xin;      // [R][IN]   network input
    P qv;       // [R][4]    input quaternions (chain: the previous frame's outputs)
    P csr;      // int [J + 1] offsets, then the in-neighbours
    P end;
};
template <class P>
K2B_HD constexpr IkgatLdsT<P> ikgat_lds_map(P base, int J, int IN, int H, int ldx, int nedges, int F, int KC) {
    const int R = F * J;
    IkgatLdsT<P> m{};
    m.hb = base;
    m.xb = m.hb + (size_t)R * H;
    m.wb = m.xb + (size_t)R * ldx;
    m.xin = m.wb + (size_t)KC * ldx;
    m.qv = m.xin + (size_t)R * IN;
    m.csr = m.qv + (size_t)R * 4;
    m.end = m.csr + (size_t)(J + 1 + nedges);
    return m;
}
using IkgatLds = IkgatLdsT<size_t>;

// ---- the plan of a handle, and the launch of one call ------------------------------------------------------------------------------
struct IkgatPlan {
    int J, IN, H, L, NH, nedges;
    int LDX, KC, F;          // x' stride; k-chunk of the staged weights; frames per workgroup of a batched launch
    K2B_HD constexpr IkgatLds lds(int frames) const { return ikgat_lds_map((size_t)0, J, IN, H, LDX, nedges, frames, KC); }
    K2B_HD constexpr size_t lds_bytes(int frames) const { return 4 * lds(frames).end; }
};
K2B_HD constexpr IkgatPlan ikgat_plan(const IkgatDims& d, int nedges) {
    IkgatPlan p{d.J, d.IN, d.H, d.L, d.NH, nedges, ikgat_ldx(d.H, d.NH), 0, 1};
    p.KC = ikgat_kc(d.H, p.LDX);
    while (p.F < kIkgatMaxFrames && p.lds_bytes(p.F + 1) <= kIkgatBatchLds) ++p.F;
    return p;
}
// Batched: ceil(B / F) workgroups of F frames; chain: one workgroup walks the frames with F = 1.
struct IkgatLaunch { int F, grid; size_t lds_bytes; };
K2B_HD constexpr IkgatLaunch ikgat_launch(const IkgatPlan& p, int num_frames, bool chain) {
    const int F = chain ? 1 : (p.F < num_frames ? p.F : num_frames);
    return IkgatLaunch{F, chain ? 1 : ceil_div(num_frames, F), p.lds_bytes(F)};
}

// ---- the device image: where each piece of the packed weights lies ----------------------------------------------------------------
// The input layers as given; per layer the projection extended by the attention vectors, [W^T | W^T att_src | W^T att_dst | 0]
// (H rows at stride LDX: columns ikgat_col_src / ikgat_col_dst), then bias and the two LayerNorm vectors; the head with both
// matrices transposed, the second padded to kIkgatOutCols columns.  Every matrix block_mm stages starts at a multiple of 4 floats.
// P: const float* into the uploaded image (the kernel), float* (the packer), or size_t from 0 for offsets in floats.
template <class P>
struct IkgatLayerT { P w, bias, lng, lnb; };        // [H][LDX], then bias [H], LayerNorm weight [H], LayerNorm bias [H]
template <class P>
struct IkgatImageT {
    int H, ldx;
    P w_in, b_in, emb, w_res, b_res;           // [H][IN], [H], [J][H], [H][IN], [H]
    P layers;                                  // the GAT layers, layer_stride apart
    size_t layer_stride;
    P w1t, b1, g1, be1, w2t, b2;               // [H][H/2], [H/2] x 3, [H/2][kIkgatOutCols] (columns 6, 7 zero), [6]
    P end;
    K2B_HD constexpr IkgatLayerT<P> layer(int l) const {
        IkgatLayerT<P> y{};
        y.w = layers + (size_t)l * layer_stride;
        y.bias = y.w + (size_t)H * ldx;
        y.lng = y.bias + H;
        y.lnb = y.lng + H;
        return y;
    }
};
template <class P>
K2B_HD constexpr IkgatImageT<P> ikgat_image(P base, int J, int IN, int H, int L, int ldx) {
    const int H2 = H / 2;
    IkgatImageT<P> m{};
    m.H = H; m.ldx = ldx;
    m.w_in = base;
    m.b_in = m.w_in + (size_t)H * IN;
    m.emb = m.b_in + H;
    m.w_res = m.emb + (size_t)J * H;
    m.b_res = m.w_res + (size_t)H * IN;
    m.layers = m.b_res + H;
    m.layer_stride = (size_t)H * ldx + 3 * (size_t)H;
    m.w1t = m.layers + (size_t)L * m.layer_stride;
    m.b1 = m.w1t + (size_t)H * H2;
    m.g1 = m.b1 + H2;
    m.be1 = m.g1 + H2;
    m.w2t = m.be1 + H2;
    m.b2 = m.w2t + kIkgatOutCols * (size_t)H2;
    m.end = m.b2 + 6;
    return m;
}

// The packer: the caller's array -> the device image.  The attention columns are folded in double, channel by channel in order,
// and rounded once.
inline std::vector<float> ikgat_pack(const IkgatPlan& p, const float* weights) {
    const IkgatDims d{p.J, p.IN, p.H, p.L, p.NH};
    const int H = p.H, NH = p.NH, C = H / NH, H2 = H / 2, LDX = p.LDX;
    const std::vector<int64_t> off = ikgat_segment_offsets(d);
    const auto seg = [&](int i) { return weights + off[i]; };
    const auto copy = [&](float* dst, int first, int count) { for (int64_t i = off[first]; i < off[first + count]; ++i) *dst++ = weights[i]; };
    std::vector<float> dw(ikgat_image((size_t)0, p.J, p.IN, H, p.L, LDX).end, 0.f);
    const IkgatImageT<float*> img = ikgat_image(dw.data(), p.J, p.IN, H, p.L, LDX);
    copy(img.w_in, kSegInW, kIkgatInputSegs);
    for (int l = 0; l < p.L; ++l) {
        const int s0 = kIkgatInputSegs + l * kIkgatLayerSegs;
        const float *W = seg(s0 + kSegLin), *as = seg(s0 + kSegAttSrc), *ad = seg(s0 + kSegAttDst);
        float* ext = img.layer(l).w;
        for (int k = 0; k < H; ++k) {
            for (int c = 0; c < H; ++c) ext[(size_t)k * LDX + c] = W[(size_t)c * H + k];
            for (int hd = 0; hd < NH; ++hd) {
                double a_src = 0.0, a_dst = 0.0;
                for (int c = hd * C; c < (hd + 1) * C; ++c) {
                    a_src += (double)W[(size_t)c * H + k] * as[c];
                    a_dst += (double)W[(size_t)c * H + k] * ad[c];
                }
                ext[(size_t)k * LDX + ikgat_col_src(H, NH) + hd] = (float)a_src;
                ext[(size_t)k * LDX + ikgat_col_dst(H, NH) + hd] = (float)a_dst;
            }
        }
        copy(img.layer(l).bias, s0 + kSegBias, 3);
    }
    const int s0 = kIkgatInputSegs + p.L * kIkgatLayerSegs;
    const float *w1 = seg(s0 + kSegH0W), *w2 = seg(s0 + kSegH4W);
    for (int k = 0; k < H; ++k)
        for (int c = 0; c < H2; ++c) img.w1t[(size_t)k * H2 + c] = w1[(size_t)c * H + k];
    copy(img.b1, s0 + kSegH0B, 3);
    for (int k = 0; k < H2; ++k)
        for (int c = 0; c < 6; ++c) img.w2t[(size_t)k * kIkgatOutCols + c] = w2[(size_t)c * H2 + k];
    copy(img.b2, s0 + kSegH4B, 1);
    return dw;
}

// ---- the graph ---------------------------------------------------------------------------------------------------------------------
// Edges of gan_regressor.py:16-36 (source -> target; both ways between a joint and its parent; the chain i <-> i+1 when no joint
// has one), then PyG's remove_self_loops + add_self_loops.  CSR of in-edges: [J + 1] offsets, then the source of every in-edge.
inline std::vector<int> ikgat_csr(int J, const int32_t* parents) {
    std::vector<std::vector<int>> in_nb(J);
    bool any = false;
    for (int c = 0; c < J; ++c)
        if (parents[c] >= 0) {
            any = true;
            if (parents[c] != c) { in_nb[c].push_back(parents[c]); in_nb[parents[c]].push_back(c); }
        }
    if (!any)
        for (int i = 0; i + 1 < J; ++i) { in_nb[i + 1].push_back(i); in_nb[i].push_back(i + 1); }
    std::vector<int> csr(J + 1, 0);
    for (int i = 0; i < J; ++i) { in_nb[i].push_back(i); csr[i + 1] = csr[i] + (int)in_nb[i].size(); }
    for (int i = 0; i < J; ++i) csr.insert(csr.end(), in_nb[i].begin(), in_nb[i].end());
    return csr;
}

// ---- the rules ---------------------------------------------------------------------------------------------------------------------
// The code and the text of a refusal, and which one wins when a call is wrong in several ways, are part of the ABI: each function
// reads top to bottom in the order its entry has always checked.
struct IkgatVerdict {
    int code = K2B_OK;
    bool nothing = false;                     // accepted, and there is nothing to run: the entry returns K2B_OK at once
    char message[512] = "";
    int refuse(int c, const char* fmt, ...) __attribute__((format(printf, 3, 4))) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(message, sizeof message, fmt, ap);
        va_end(ap);
        return code = c;
    }
};

// k2b_ikgat_create: dimensions -> parents -> num_weights -> graph -> LDS; the entry asks for a device only after all of them pass
inline int ikgat_create_rules(bool out, const IkgatDims& d, const int32_t* parents, bool weights, int64_t num_weights, IkgatVerdict& v) {
    const int J = d.J, IN = d.IN, H = d.H, L = d.L, NH = d.NH;
    if (!out) return v.refuse(K2B_ERR_INVALID_ARGUMENT, "k2b_ikgat_create: out is NULL");
    if (!parents || !weights) return v.refuse(K2B_ERR_INVALID_ARGUMENT, "k2b_ikgat_create: NULL array");
    if (J < 1 || J > 64) return v.refuse(K2B_ERR_UNSUPPORTED, "k2b_ikgat_create: %d joints, supported 1..64", J);
    if (IN != 3 && IN != 9) return v.refuse(K2B_ERR_UNSUPPORTED, "k2b_ikgat_create: input_dim=%d, supported 3 or 9", IN);
    if (H < 16 || H > 256 || H % 16 != 0)
        return v.refuse(K2B_ERR_UNSUPPORTED, "k2b_ikgat_create: hidden_dim=%d, supported multiples of 16 up to 256", H);
    if (L < 1 || L > 8) return v.refuse(K2B_ERR_UNSUPPORTED, "k2b_ikgat_create: num_layers=%d, supported 1..8", L);
    if (NH < 1 || H % NH != 0) return v.refuse(K2B_ERR_UNSUPPORTED, "k2b_ikgat_create: num_heads=%d does not divide hidden_dim=%d", NH, H);
    for (int i = 0; i < J; ++i)
        if (parents[i] >= J) return v.refuse(K2B_ERR_INVALID_ARGUMENT, "k2b_ikgat_create: parents[%d]=%d, only %d joints", i, parents[i], J);
    const int64_t expect = ikgat_segment_offsets(d).back();
    if (num_weights != expect)
        return v.refuse(K2B_ERR_INVALID_ARGUMENT, "k2b_ikgat_create: %lld weights, the dimensions need %lld", (long long)num_weights,
                        (long long)expect);
    const size_t one = ikgat_plan(d, ikgat_csr(J, parents)[J]).lds_bytes(1);
    if (one > kIkgatMaxLds)
        return v.refuse(K2B_ERR_UNSUPPORTED, "k2b_ikgat_create: one frame needs %zu B of LDS (J=%d H=%d heads=%d), the limit is %zu", one, J, H, NH,
                        kIkgatMaxLds);
    return K2B_OK;
}

// k2b_ikgat_predict (plan: the handle's, NULL without one)
inline int ikgat_predict_rules(const IkgatPlan* plan, int32_t num_frames, bool positions, bool quat_in, bool quat_out, IkgatVerdict& v) {
    if (!plan) return v.refuse(K2B_ERR_INVALID_ARGUMENT, "k2b_ikgat_predict: net is NULL");
    if (num_frames < 0) return v.refuse(K2B_ERR_INVALID_ARGUMENT, "k2b_ikgat_predict: num_frames=%d must be >= 0", num_frames);
    if (num_frames == 0) { v.nothing = true; return K2B_OK; }
    if (!positions || !quat_out) return v.refuse(K2B_ERR_INVALID_ARGUMENT, "k2b_ikgat_predict: NULL buffer");
    if (plan->IN == 9 && !quat_in)
        return v.refuse(K2B_ERR_INVALID_ARGUMENT, "k2b_ikgat_predict: the pos-rot6 network (input_dim 9) needs input quaternions");
    return K2B_OK;
}

}  // namespace k2b
