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

}  // namespace k2b
