// Scan plan of the fused fit kernel's tree pass: where every joint of the kinematic tree sits in the 32 tree lanes, and how its
// subtree sum comes out of two fp32 inclusive prefix scans WITHOUT a difference of prefixes (k2b_lanes.h, chain_end_scans).
// Host only, no device call: a pure function of the parent table (k2b_model_tables.h builds the lane tables from it).
//
// With the lanes in REVERSED DFS pre-order a subtree is the lane range that ENDS at its joint, and every joint is one of two kinds:
//   chain-type  all its descendants form a single-child path down to a leaf.  Its sum is a running sum along its own chain: a prefix
//               scan with shifts 1, 2, 4 whose steps are masked per lane so that it stops at the chain's leaf (at most 8 lanes, and
//               a chain never straddles a 16-lane DPP row: holes are inserted in front of a chain that would).
//   end-type    its DFS window ends at the end of the tree, so its subtree is every lane up to its own: the unmasked prefix scan
//               over the half-wave.
// A hole is a lane beyond the tree (no joint, zero rotation, zero offset, no target): it adds exact zeros to every sum.  Lane 31
// stays free in every plan: it is the identity source of the pointer-doubling rounds.
#pragma once
#include <vector>

#include "k2b_tree.h"

namespace k2b {

constexpr int kScanLanes = 32;          // tree lanes of a half-wave
constexpr int kScanMaxChain = 8;        // lanes a masked scan with shifts 1, 2, 4 covers
// per-lane flags of the plan (lane table, entry kLaneTabScan)
constexpr int kScanStep1 = 1, kScanStep2 = 2, kScanStep4 = 4;   // the chain scan's step with that shift adds the lower lane's value
constexpr int kScanEnd = 8;             // the joint's sum is the unmasked prefix (else the chain scan's)
constexpr int kScanChain = 16;          // the joint is chain-type (it may be end-type as well: the chain scan is taken)

struct ScanPlan {
    bool valid = false;
    const char* why = "";               // what made the plan invalid
    int lanes = 0;                      // lanes used, holes included
    std::vector<int> lane_of;           // [J] lane of joint j
    int joint_at[kScanLanes];           // joint of lane l, -1: hole / beyond the tree
    int flags[kScanLanes];              // kScan* bits of lane l (0 for a hole)
};

// Children are visited in ascending order, as everywhere in the library (k2b_tree.h).
inline ScanPlan fit_scan_plan(const Tree& t) {
    const int J = t.J;
    const auto &parents = t.parents, &order = t.order, &pos = t.pos, &size = t.size;
    const auto& children = t.children;
    ScanPlan p;
    for (int l = 0; l < kScanLanes; ++l) { p.joint_at[l] = -1; p.flags[l] = 0; }
    p.lane_of.assign(J, -1);
    if (J >= kScanLanes) { p.why = "more joints than tree lanes"; return p; }
    // chain position: lanes between the joint and the leaf of its chain, -1 when its subtree is no single-child path
    std::vector<int> chain_pos(J, -1);
    for (int j = J - 1; j >= 0; --j) {
        if (children[j].empty()) chain_pos[j] = 0;
        else if (children[j].size() == 1 && chain_pos[children[j][0]] >= 0) chain_pos[j] = chain_pos[children[j][0]] + 1;
    }
    for (int j = 0; j < J; ++j) {
        const bool end = pos[j] + size[j] == J;
        if (chain_pos[j] < 0 && !end) { p.why = "a joint is neither chain-type nor end-type"; return p; }
        if (chain_pos[j] >= kScanMaxChain) { p.why = "a chain is longer than 8 lanes"; return p; }
    }
    // placement: reversed DFS order; a chain (met at its leaf) that would straddle a 16-lane row starts the next row
    int lane = 0;
    for (int i = J - 1; i >= 0; --i) {
        const int j = order[i];
        if (chain_pos[j] == 0) {
            int top = j;
            while (parents[top] >= 0 && chain_pos[parents[top]] >= 0) top = parents[top];
            const int len = chain_pos[top] + 1;
            if ((lane & 15) + len > 16) lane = (lane | 15) + 1;
        }
        if (lane >= kScanLanes - 1) { p.why = "the placement needs more than 31 lanes"; return p; }
        p.lane_of[j] = lane;
        p.joint_at[lane] = j;
        const int k = chain_pos[j];
        int f = pos[j] + size[j] == J && k < 0 ? kScanEnd : 0;
        if (k >= 0) f |= kScanChain | (k >= 1 ? kScanStep1 : 0) | (k >= 2 ? kScanStep2 : 0) | (k >= 4 ? kScanStep4 : 0);
        p.flags[lane] = f;
        ++lane;
    }
    p.lanes = lane;
    p.valid = true;
    return p;
}

}  // namespace k2b
