// Layout constants and index helpers that the kernels and the host's table builders (k2b_model_tables.h) share.  No HIP runtime:
// k2b_internal.h includes this header, and a host-only program may include it alone.
#pragma once
#include <stddef.h>

namespace k2b {

typedef _Float16 k2b_half;

constexpr int kMaxBetas = 16;       // shape coefficients of the 24-joint fused fit kernel
constexpr int kMaxShape = 32;       // shape coefficients (betas | expression) of the LBS kernels and the tree fit kernel
constexpr int kMaxRounds = 4;       // pointer-doubling rounds: tree depth < 2^4
constexpr int kLaneTabStride = 9;   // ints per lane: joint, parent lane, anc[kMaxRounds], subtree size, depth, scan flags
constexpr int kLaneTabScan = 8;     // scan flags of the lane (k2b_scan_plan.h: kScan*), 0 where the model has no scan plan
constexpr int kMaxViews = 8;        // calibrated cameras of a multi-view call (k2b_internal.h, FitView)
constexpr int kSurfMaxTargets = 128;   // surface targets per call (k2b_surface.hip)

// LBS operands are f16 hi/lo pairs in MFMA fragment order: [k-step][row][16 halfs].
constexpr float kPdScale = 256.0f;   // power-of-two scale of the vertex-GEMM B operand (keeps f16 lo terms normal)

// Element (k, row) inside piece number `frag` of a piece-ordered operand: a piece is the
// 1 KiB a wave moves for one 16-deep k-step of one 32-row tile, stored lane-linear:
// [h = (k >> 3) & 1][row & 31][k & 7]  (lane 32 h + row owns 16 contiguous bytes).  (constexpr: host and device in a HIP unit)
constexpr size_t frag_elem(size_t frag, int k, int row) {
    return ((frag * 2 + ((k >> 3) & 1)) * 32 + (row & 31)) * 8 + (k & 7);
}

// k-groups of the tile kernel's transform GEMM (k2b_internal.h, TileArgs): GA = ceil(J / 8), NGP = 2 GA + 2
constexpr int tile_groups_a(int J) { return (J + 7) / 8; }
constexpr int tile_ngp(int GA) { return 2 * GA + 2; }

// ---- fused fit kernel (k2b_fit.hip) ------------------------------------------------------------------------------------------
constexpr int kFitJoints = 24;      // joints of the tree the fused fit kernel is built for (SMPL)
constexpr int kPriorDim = 69;       // 3 * (kFitJoints - 1)
constexpr int kPriorMaxGauss = 8;   // mixture components resident in LDS
constexpr int kFitMaxWaves = 8;     // waves per workgroup of the 8-wave shapes
// LDS image of the prior: rim rows 64..68 over columns 0..63 as [m][5][64], then mu | c = P mu of rows 0..63 as [m][2][64]
constexpr int kPriorRimFragEntries = 4 * 21;   // per component: 4 fragments [k-step 2][hi | lo] of 20 live lanes + one zero entry, 16 B each
constexpr int kPriorImageFloats = 2 * 5 * 64 * 4 + kPriorMaxGauss * 2 * 64 + kPriorMaxGauss * kPriorRimFragEntries * 4;

// LDS of the fused fit kernel (floats), in the order the kernel lays it out.  The launch plan's L-BFGS staging budgets
// (k2b_launch_plan.h) are made of these areas.
namespace fit_lds {
constexpr int MAXS = 16;                // frame slots per workgroup (= MFMA columns)
constexpr int MG = kPriorMaxGauss;      // 8
constexpr int NC = 64;                  // core rows / columns of a component handled by the matrix cores
constexpr int XS = 96;                  // strip: go@0, body@4, betas@76, transl@92, joint loss@95
constexpr int SLOT = 2 * XS + NC + 4;   // 260 floats: the +4 spreads the 16 frame columns of the MFMA-side reads over the banks
constexpr int YX_STRIDE = MG * NC + 4;  // y exchange: [slot][m][64] (+4: b128 stores of the 16 frame columns hit distinct banks)
constexpr int DD_STRIDE_MAX = 52;        // per-lane stride of the J_dirs table in LDS (see the kernel)
constexpr int PLO_FLOATS = MG * 4 * 2 * 64 * 4;   // lo fragments of all components (paired shape): [m][tile][ks][64 lanes][8 halfs]
constexpr int WX_FLOATS = MAXS * 64;                 // rim rows' products: [slot][lane 8 m + s] = (P_m[64 + s][0..63] theta)[s < 5], zeros for s >= 5
constexpr int RC_FLOATS = 8 * 64;                    // per-lane rim constants (FitArgs::row_const) for the 16-wave shapes, which have no registers for them
constexpr int LDS_FLOATS = kPriorImageFloats + MAXS * SLOT + MAXS * MG + MAXS * YX_STRIDE + 64 * DD_STRIDE_MAX + PLO_FLOATS + WX_FLOATS + RC_FLOATS;
constexpr int kLdsBudgetBytes = 163840;              // 160 KiB per workgroup
static_assert(LDS_FLOATS * 4 <= kLdsBudgetBytes, "LDS budget");
}  // namespace fit_lds

}  // namespace k2b
