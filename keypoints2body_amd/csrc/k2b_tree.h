// The kinematic tree as the host sees it: everything the lane tables of the fit kernels (k2b_model_tables.h) and the scan plan
// (k2b_scan_plan.h) derive from the parent table, computed once.  Host only, no device call.
#pragma once
#include <vector>

namespace k2b {

struct Tree {
    int J = 0, max_depth = 0;
    std::vector<int> parents;                 // [J] parents[0] < 0, parents[j] < j (checked by the caller)
    std::vector<std::vector<int>> children;   // ascending
    std::vector<int> order, pos;              // DFS pre-order (children in ascending order) and every joint's position in it
    std::vector<int> size, depth;             // joints of the subtree (the joint included), levels below the root

    Tree() = default;
    Tree(int num_joints, const int* par) : J(num_joints), parents(par, par + num_joints), children(J), pos(J, 0), size(J, 1), depth(J, 0) {
        for (int j = 1; j < J; ++j) {
            children[parents[j]].push_back(j);
            depth[j] = depth[parents[j]] + 1;
            max_depth = depth[j] > max_depth ? depth[j] : max_depth;
        }
        std::vector<int> stack{0};
        while (!stack.empty()) {
            const int j = stack.back();
            stack.pop_back();
            pos[j] = (int)order.size();
            order.push_back(j);
            for (auto it = children[j].rbegin(); it != children[j].rend(); ++it) stack.push_back(*it);
        }
        for (int j = J - 1; j >= 1; --j) size[parents[j]] += size[j];
    }
    // the joint `levels` parent steps above j, -1 past the root
    int ancestor(int j, int levels) const {
        for (; levels > 0 && j >= 0; --levels) j = parents[j];
        return j;
    }
};

// pointer-doubling rounds that reach every joint down to `depth`: 2^rounds > depth
inline int rounds_for_depth(int depth) {
    int rounds = 0;
    while ((1 << rounds) < depth + 1) ++rounds;
    return rounds;
}

}  // namespace k2b
