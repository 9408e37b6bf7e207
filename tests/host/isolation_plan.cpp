// The launch plans of the isolation cases (tests/isolation_common.py) as csrc/k2b_launch_plan.h makes them: shape, frames per wave
// and per workgroup, grid, L-BFGS scheme.  tests/test_isolation_host.py holds the positions of the poisoned frames to these lines,
// so that a change of the launch policy cannot turn tests/test_gpu_isolation.py into one workgroup per frame unnoticed.
// No HIP call, no device.
// Usage: isolation_plan (<name> <entry> <frames> <cus> <debug_launch_shape> <shape coefficients>)...
//   entry: fused | tree | chain_fused | chain_tree | lbfgs_fused | lbfgs_tree | chain_lbfgs     (a chain: <frames> sequences)
// One line per case: "<name> cus=.. frames=.. scheme=.. launches=.. shape=.. frames_per_wave=.. frames_per_wg=.. grid=.. comp_waves=..".
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "k2b_launch_plan.h"

using namespace k2b;

static const char* scheme_name(LbfgsScheme s) {
    return s == LbfgsScheme::persistent ? "persistent" : s == LbfgsScheme::fused_rounds ? "fused_rounds" : "two_launches";
}

int main(int argc, char** argv) {
    if ((argc - 1) % 6 != 0) {
        std::fprintf(stderr, "usage: isolation_plan (<name> <entry> <frames> <cus> <debug_launch_shape> <shape coefficients>)...\n");
        return 2;
    }
    const int chain_len = 3;
    for (int i = 1; i < argc; i += 6) {
        const char* name = argv[i];
        const char* entry = argv[i + 1];
        const int n = std::atoi(argv[i + 2]), cus = std::atoi(argv[i + 3]), shape = std::atoi(argv[i + 4]), ns = std::atoi(argv[i + 5]);
        if (n < 1 || cus < 1) {
            std::fprintf(stderr, "%s: %d frames on %d compute units\n", name, n, cus);
            return 2;
        }
        const bool tree = !std::strcmp(entry, "tree") || !std::strcmp(entry, "chain_tree") || !std::strcmp(entry, "lbfgs_tree");
        const char* scheme = "-";
        if (tree) {
            if (!std::strcmp(entry, "lbfgs_tree")) scheme = scheme_name(lbfgs_scheme_for(n, cus, false, -1, 0));
            const FitTreePlan p = plan_fit_tree(n, cus, ns, !std::strcmp(entry, "chain_tree"), shape);
            std::printf("%s cus=%d frames=%d scheme=%s launches=1 shape=%d frames_per_wave=1 frames_per_wg=%d grid=%d comp_waves=%d\n", name, cus,
                        n, scheme, shape, p.frames_per_wg, p.grid, p.comp_waves);
            continue;
        }
        int lb = LbMode::none, chain = 1, force = shape;
        if (!std::strcmp(entry, "lbfgs_fused")) {
            const LbfgsScheme s = lbfgs_scheme_for(n, cus, true, -1, 0);
            scheme = scheme_name(s);
            lb = s == LbfgsScheme::persistent ? LbMode::persistent : s == LbfgsScheme::fused_rounds ? LbMode::step : LbMode::none;
        } else if (!std::strcmp(entry, "chain_fused")) {
            chain = chain_len;
        } else if (!std::strcmp(entry, "chain_lbfgs")) {
            chain = chain_len;
            lb = LbMode::persistent;
            scheme = scheme_name(LbfgsScheme::persistent);
        } else if (std::strcmp(entry, "fused")) {
            std::fprintf(stderr, "%s: unknown entry %s\n", name, entry);
            return 2;
        }
        const FitPlan p = plan_fit_world(n, cus, ns, false, force, lb, chain);
        if (!p.ok || p.num_launches < 1) {
            std::printf("%s cus=%d frames=%d scheme=%s launches=0 shape=-1 frames_per_wave=0 frames_per_wg=0 grid=0 comp_waves=0\n", name, cus, n, scheme);
            continue;
        }
        const FitLaunch& l = p.launch[0];
        std::printf("%s cus=%d frames=%d scheme=%s launches=%d shape=%d frames_per_wave=%d frames_per_wg=%d grid=%d comp_waves=0\n", name, cus, n,
                    scheme, p.num_launches, l.shape, fit_shape_desc(l.shape).frames_per_wave, l.frames_per_wg, l.grid);
    }
    return 0;
}
