// k2b_api_prior.hip — the pose-prior handle of the C ABI (include/k2b.h): the mixture's images for the fused fit kernel and,
// built on first use, its restriction to a prefix of the pose for the tree fit kernel.
#include <algorithm>
#include <cmath>
#include <memory>

#include "k2b_host.h"

using namespace k2b::host;

namespace k2b {
namespace host {

// the mixture restricted to its first Dv dimensions, the others fixed at 0 (k2b_fit_tree.hip)
int folded_prior(k2b_prior* p, int Dv, const k2b_prior::Folded** out) {
    std::lock_guard<std::mutex> lk(p->mu_lock);
    auto it = p->folded.find(Dv);
    if (it != p->folded.end()) { *out = &it->second; return K2B_OK; }
    const int M = p->M, D = p->D;
    constexpr int MG = k2b::kPriorMaxGauss;
    std::vector<float> A((size_t)MG * 16 * 64 * 4, 0.f), h((size_t)MG * 64, 0.f), b((size_t)MG * 64, 0.f), mu((size_t)MG * 64, 0.f),
        cl(MG, 3.0e38f);                                     // components beyond M: never the arg-min
    for (int m = 0; m < M; ++m) {
        auto P = [&](int i, int j) { return p->Ps[((size_t)m * D + i) * D + j]; };
        double c = 0.0;
        for (int k = Dv; k < D; ++k)
            for (int l = Dv; l < D; ++l) c += p->mu[(size_t)m * D + k] * P(k, l) * p->mu[(size_t)m * D + l];   // d_c = -mu_c
        for (int i = 0; i < Dv; ++i) {
            double bi = 0.0, Amu = 0.0;
            for (int k = Dv; k < D; ++k) bi -= P(i, k) * p->mu[(size_t)m * D + k];
            for (int j = 0; j < Dv; ++j) {
                A[(((size_t)m * 16 + (j >> 2)) * 64 + i) * 4 + (j & 3)] = (float)P(i, j);
                Amu += P(i, j) * p->mu[(size_t)m * D + j];
            }
            b[(size_t)m * 64 + i] = (float)bi;
            h[(size_t)m * 64 + i] = (float)(bi - Amu);
            mu[(size_t)m * 64 + i] = (float)p->mu[(size_t)m * D + i];
        }
        cl[m] = (float)(0.5 * c) - logf(p->nllw[m]);         // a weight that underflowed to 0 gives +inf: never the arg-min
    }
    k2b_prior::Folded f;
    HIP_TRY(f.pA.upload(A.data(), A.size()));
    HIP_TRY(f.ph.upload(h.data(), h.size()));
    HIP_TRY(f.pb.upload(b.data(), b.size()));
    HIP_TRY(f.pmu.upload(mu.data(), mu.size()));
    HIP_TRY(f.pcl.upload(cl.data(), cl.size()));
    *out = &p->folded.emplace(Dv, std::move(f)).first->second;   // (map nodes stay where they are)
    return K2B_OK;
}

}  // namespace host
}  // namespace k2b

extern "C" {

int k2b_prior_create(k2b_prior** out, int32_t M, int32_t D, const float* means, const float* precisions,
                     const float* nll_weights) {
    if (!out) return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_prior_create: out is NULL");
    *out = nullptr;
    if (!means || !precisions || !nll_weights) return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_prior_create: NULL array");
    if (D != k2b::kPriorDim) return fail(K2B_ERR_UNSUPPORTED, "k2b_prior_create: dim=%d, the fit kernel is built for 69-D body poses", D);
    if (M < 1 || M > k2b::kPriorMaxGauss)
        return fail(K2B_ERR_UNSUPPORTED, "k2b_prior_create: num_gaussians=%d, supported 1..%d", M, k2b::kPriorMaxGauss);
    for (int m = 0; m < M; ++m)
        if (!(nll_weights[m] >= 0.f)) return fail(K2B_ERR_INVALID_ARGUMENT, "k2b_prior_create: nll_weights[%d] must be >= 0", m);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(K2B_ERR_NO_DEVICE, "k2b_prior_create: no HIP device visible (this engine has no CPU path)");

    constexpr int MG = k2b::kPriorMaxGauss;
    // symmetrised precisions and c_m = P_m mu_m, in double
    std::vector<double> Ps((size_t)M * D * D), c((size_t)M * D, 0.0);
    for (int m = 0; m < M; ++m)
        for (int i = 0; i < D; ++i)
            for (int j = 0; j < D; ++j)
                Ps[((size_t)m * D + i) * D + j] =
                    0.5 * ((double)precisions[((size_t)m * D + i) * D + j] + (double)precisions[((size_t)m * D + j) * D + i]);
    for (int m = 0; m < M; ++m)
        for (int i = 0; i < D; ++i) {
            double s = 0.0;
            for (int j = 0; j < D; ++j) s += Ps[((size_t)m * D + i) * D + j] * (double)means[m * D + j];
            c[(size_t)m * D + i] = s;
        }
    auto P = [&](int m, int i, int j) -> float { return (float)Ps[((size_t)m * D + i) * D + j]; };

    // LDS image: rim rows 64..68 over the core columns, then mu | c of the core rows (k2b_internal.h)
    constexpr int NC = 64, NR = 5;
    std::vector<float> pa((size_t)k2b::kPriorImageFloats, 0.f);
    float* cmu = pa.data() + 2 * NR * 64 * 4;
    std::vector<float> rc((size_t)8 * 64, 0.f), nlw(MG, 0.f);
    for (int m = 0; m < M; ++m) {
        for (int cc = 0; cc < NR; ++cc)
            for (int col = 0; col < NC; ++col)
                pa[((size_t)m * NR + cc) * NC + col] = P(m, NC + cc, col);       // [m][rim row][column]: lane = column, conflict-free 4-byte reads
        for (int r = 0; r < NC; ++r) {
            cmu[(size_t)m * 2 * NC + r] = means[m * D + r];
            cmu[(size_t)m * 2 * NC + NC + r] = (float)c[(size_t)m * D + r];
        }
        // per-lane constants of the rim rows: lane 8m + s, s < 5 <-> row 64 + s of component m
        for (int s = 0; s < NR; ++s) {
            const int l = 8 * m + s;
            for (int k = 0; k < NR; ++k) rc[(size_t)k * 64 + l] = P(m, NC + s, NC + k);
            rc[(size_t)5 * 64 + l] = (float)c[(size_t)m * D + NC + s];
            double kb = 0.0;
            for (int j = 0; j < NC; ++j) kb += Ps[((size_t)m * D + NC + s) * D + j] * (double)means[m * D + j];
            rc[(size_t)6 * 64 + l] = (float)kb;
            rc[(size_t)7 * 64 + l] = means[m * D + NC + s];
        }
        nlw[m] = -logf(nll_weights[m]);      // a weight that underflowed to 0 gives +inf, as torch.log does in the reference: never the arg-min
    }
    // the 64 x 64 core as MFMA A fragments (v_mfma_f32_16x16x32_f16: lane l holds row l & 15,
    // k = 8 (l >> 4) + j), two f16 terms per entry, scaled by a power of two per component so that the
    // largest entry sits near 2^13 (hi never overflows, lo stays normal for every entry that matters)
    std::vector<k2b::k2b_half> f32((size_t)k2b::kPriorFrag32Halfs, (k2b::k2b_half)0.f);
    std::unique_ptr<k2b_prior> owner(new k2b_prior);          // released with its buffers if an upload fails
    k2b_prior* p = owner.get();
    p->M = M; p->D = D;
    p->Ps = Ps;
    p->mu.assign(means, means + (size_t)M * D);
    p->nllw.assign(nll_weights, nll_weights + M);
    for (int m = 0; m < MG; ++m) p->inv_scale[m] = 1.0f;
    for (int m = 0; m < M; ++m) {
        double maxabs = 0.0;
        for (int row = 0; row < D; ++row)          // core rows and the rim rows 64..68 (their fragments share the scale)
            for (int col = 0; col < NC; ++col) maxabs = std::max(maxabs, std::fabs(Ps[((size_t)m * D + row) * D + col]));
        int e = 0;
        if (maxabs > 0.0 && std::isfinite(maxabs)) e = 13 - (int)std::ceil(std::log2(maxabs));
        e = std::max(-100, std::min(100, e));
        const double scale = std::ldexp(1.0, e);
        p->inv_scale[m] = (float)std::ldexp(1.0, -e);
        for (int t = 0; t < 4; ++t)
            for (int l = 0; l < 64; ++l) {
                const int row = 16 * t + (l & 15), g = l >> 4;
                for (int ks = 0; ks < 2; ++ks)
                    for (int j = 0; j < 8; ++j) {
                        const float x = (float)(Ps[((size_t)m * D + row) * D + 32 * ks + 8 * g + j] * scale);
                        const k2b::k2b_half hi = (k2b::k2b_half)x;
                        f32[((((size_t)m * 4 + t) * 4 + ks) * 64 + l) * 8 + j] = hi;
                        f32[((((size_t)m * 4 + t) * 4 + 2 + ks) * 64 + l) * 8 + j] = (k2b::k2b_half)(x - (float)hi);
                    }
            }
        // rim rows 64..68 over the core columns as a FIFTH row tile (rows 69..79 are zero), kept compact in the LDS image:
        // fragment f = 2 ks + (hi | lo), entry kg * 5 + row = the eight halfs of MFMA lane (row, k-group kg); entry 20 = zeros,
        // read by the lanes of the tile's empty rows (k2b_fit.hip, comp_issue)
        k2b::k2b_half* rf = reinterpret_cast<k2b::k2b_half*>(pa.data() + 2 * NR * 64 * 4 + MG * 2 * NC) + (size_t)m * k2b::kPriorRimFragEntries * 8;
        for (int ks = 0; ks < 2; ++ks)
            for (int g = 0; g < 4; ++g)
                for (int row = 0; row < NR; ++row)
                    for (int j = 0; j < 8; ++j) {
                        const float x = (float)(Ps[((size_t)m * D + NC + row) * D + 32 * ks + 8 * g + j] * scale);
                        const k2b::k2b_half hi = (k2b::k2b_half)x;
                        rf[((size_t)(2 * ks) * 21 + g * 5 + row) * 8 + j] = hi;
                        rf[((size_t)(2 * ks + 1) * 21 + g * 5 + row) * 8 + j] = (k2b::k2b_half)(x - (float)hi);
                    }
    }
    hipError_t e = p->pa_image.upload(pa.data(), pa.size());
    if (e == hipSuccess) e = p->row_const.upload(rc.data(), rc.size());
    if (e == hipSuccess) e = p->nlw.upload(nlw.data(), nlw.size());
    if (e == hipSuccess) e = p->frag32.upload(f32.data(), f32.size());
    if (e != hipSuccess) return fail(K2B_ERR_HIP, "k2b_prior_create: upload failed: %s", hipGetErrorString(e));
    *out = owner.release();
    return K2B_OK;
}

void k2b_prior_destroy(k2b_prior* p) {
    if (!p) return;
    (void)hipDeviceSynchronize();
    delete p;
}

}  // extern "C"
