// k2b_launch_plan.h — the launch policy of the fit kernels and of the device L-BFGS as pure functions: which shape a batch gets,
// how many frames go to a workgroup, when a batch is split, which L-BFGS scheme runs, how many history pairs fit in LDS.  The ONE
// statement of that policy: the launchers execute these plans, the kernels read the same descriptions,
// and tests/host/launch_plan_check.cpp holds them to definitions written out independently, for any CU count, without a GPU.
// No HIP runtime: a plain host C++ program may include this header alone.
#pragma once
#include "k2b_layout.h"

#if defined(__HIPCC__)
#define K2B_HD __host__ __device__
#else
#define K2B_HD
#endif

namespace k2b {

// ---- named values of the launch fields (the fields themselves stay int: kernel-argument layouts do not move) ---------------------
// execution shapes of k2b_fit_world_kernel (its template parameter MODE)
enum FitShape : int { MODE_SPLIT = 0, MODE_SPLIT_PAIRED = 1, MODE_PAIRED = 2, MODE_WIDE = 3, MODE_SPLIT_LBFGS = 4 };   // 4: split + the L-BFGS step
// FitArgs::force_shape = k2b_fit_config::debug_launch_shape
struct ForceShape { enum : int { automatic = 0, split = 1, split_paired = 2, paired = 3, wide = 4 }; };
// FitArgs::lb_mode: the L-BFGS step inside the fit launch
struct LbMode { enum : int { none = 0, step = 1, finalize = 2, persistent = 3 }; };
// FitTreeArgs::debug_shape
struct TreeShape { enum : int { automatic = 0, plain = 1, comp_waves = 2 }; };
// how the rounds of a device L-BFGS fit reach the device (k2b_lbfgs.hip)
enum class LbfgsScheme { two_launches, fused_rounds, persistent };

// One description per shape: waves of the workgroup, frame slots it can carry, frames a wave carries in its row and tree roles.
struct FitShapeDesc { int waves, capacity, frames_per_wave; };
K2B_HD constexpr FitShapeDesc fit_shape_desc(int shape) {
    return shape == MODE_SPLIT || shape == MODE_SPLIT_LBFGS ? FitShapeDesc{kFitMaxWaves, 4, 1}
         : shape == MODE_SPLIT_PAIRED                       ? FitShapeDesc{kFitMaxWaves, 8, 2}
         : shape == MODE_PAIRED                             ? FitShapeDesc{kFitMaxWaves, fit_lds::MAXS, 2}
                                                            : FitShapeDesc{2 * kFitMaxWaves, fit_lds::MAXS, 2};   // wide
}
// the shape a ForceShape value other than `automatic` names
K2B_HD constexpr int forced_fit_shape(int force_shape) {
    return force_shape == ForceShape::split ? MODE_SPLIT : force_shape == ForceShape::split_paired ? MODE_SPLIT_PAIRED
         : force_shape == ForceShape::paired ? MODE_PAIRED : MODE_WIDE;
}
// The shape a batch gets by its frames per CU: up to 4 split (SIMDs would idle, so every frame gets two cooperating waves), up to
// 8 split-paired, beyond that wide.  Never paired: that shape is a test twin.
K2B_HD constexpr int auto_fit_shape(int frames_per_cu) {
    return frames_per_cu <= fit_shape_desc(MODE_SPLIT).capacity ? MODE_SPLIT
         : frames_per_cu <= fit_shape_desc(MODE_SPLIT_PAIRED).capacity ? MODE_SPLIT_PAIRED : MODE_WIDE;
}
// L-BFGS inside the fit launch: the step rides the split shape's row wave (as many frames per CU as that shape holds); the
// persistent launch's optimisers sit on the idle tree waves, two per workgroup
constexpr int kLbfgsFusedFrames = fit_shape_desc(MODE_SPLIT_LBFGS).capacity;
constexpr int kLbfgsPersistentFrames = 2;

K2B_HD constexpr int ceil_div(int a, int b) { return (a + b - 1) / b; }
K2B_HD constexpr int clamp_int(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- k2b_fit_world_kernel ------------------------------------------------------------------------------------------------------
struct FitLaunch {
    int first_frame, num_frames;      // frames [first_frame, first_frame + num_frames) of the call (a chain: sequences)
    int shape, NBT;                   // template arguments MODE and NBT (shape coefficients the tree pass is unrolled for)
    bool scan64;
    int frames_per_wg, grid, block_threads;
};
struct FitPlan {
    bool ok;                          // false: the batch and lb_mode disagree (the caller asks lbfgs_scheme_for first)
    int num_launches;                 // 0 (no frames, or !ok), 1 or 2
    FitLaunch launch[2];
};
K2B_HD constexpr FitLaunch fit_launch(int first_frame, int num_frames, int shape, int num_betas, bool scan64, int frames_per_wg) {
    return FitLaunch{first_frame, num_frames, shape, num_betas <= 10 ? 10 : 16, scan64, frames_per_wg,
                     ceil_div(num_frames, frames_per_wg), fit_shape_desc(shape).waves * 64};
}

K2B_HD constexpr FitPlan plan_fit_world(int num_frames, int num_cus, int num_betas, bool scan64, int force_shape, int lb_mode,
                                        int chain_len) {
    FitPlan p{true, 0, {}};
    if (num_frames <= 0) return p;
    const int per_cu = ceil_div(num_frames, num_cus);
    const int lb_frames = lb_mode == LbMode::persistent ? kLbfgsPersistentFrames : kLbfgsFusedFrames;
    int shape = 0, fpw = per_cu;
    if (chain_len > 1) {
        // warm-start chains: num_frames sequences, one split-shape slot each (the chain is serial, so the shape that gives one
        // frame the most hardware is the one to use); force_shape does not apply
        if (lb_mode != LbMode::none && lb_mode != LbMode::persistent) { p.ok = false; return p; }
        shape = lb_mode == LbMode::persistent ? MODE_SPLIT_LBFGS : MODE_SPLIT;
        if (lb_mode == LbMode::persistent && fpw > lb_frames) fpw = lb_frames;
    } else if (lb_mode != LbMode::none) {
        if (per_cu > lb_frames) { p.ok = false; return p; }
        shape = MODE_SPLIT_LBFGS;
    } else if (force_shape != ForceShape::automatic) {
        // small (test) batches fill the shape's slots; batches of a CU count or more keep one workgroup per CU where the shape can
        shape = forced_fit_shape(force_shape);
        if (num_frames < num_cus) fpw = num_frames;
    } else {
        // More frames than one full-width launch of the densest shape holds (16 per CU): such a launch runs in rounds of num_cus
        // workgroups, each as long as a full one however few workgroups it has (10 000 frames: 625 workgroups = 2.4 rounds, paid
        // as 3).  The whole rounds first, the remainder on its own in the shape that suits ITS size (1 808 frames: split-paired,
        // 0.6 of a wide round).  Frames are independent: results do not change.
        const int full = fit_shape_desc(MODE_WIDE).capacity * num_cus;
        if (num_frames > full && num_frames % full != 0) {
            const int head = num_frames / full * full;
            p.launch[p.num_launches++] = fit_launch(0, head, MODE_WIDE, num_betas, scan64, fit_shape_desc(MODE_WIDE).capacity);
            p.launch[p.num_launches++] = plan_fit_world(num_frames - head, num_cus, num_betas, scan64, force_shape, lb_mode, chain_len).launch[0];
            p.launch[1].first_frame = head;
            return p;
        }
        shape = auto_fit_shape(per_cu);
    }
    p.launch[p.num_launches++] = fit_launch(0, num_frames, shape, num_betas, scan64, clamp_int(fpw, 1, fit_shape_desc(shape).capacity));
    return p;
}

// ---- device L-BFGS -------------------------------------------------------------------------------------------------------------
// fused_ok: the fused kernel takes the call (24-joint model, the prior over the whole pose, kinematic targets only); stage_cap,
// dev_scheme: the development switches K2B_LBFGS_STAGE_PAIRS (< 0: unset) and K2B_LBFGS_SCHEME (1 forces two launches per round,
// 2 the fused rounds wherever they apply).  Agrees with plan_fit_world: fused_rounds and persistent are only named where the
// plan for LbMode::step / LbMode::persistent is ok.
K2B_HD constexpr LbfgsScheme lbfgs_scheme_for(int num_frames, int num_cus, bool fused_ok, int stage_cap, int dev_scheme) {
    const int per_cu = ceil_div(num_frames, num_cus);
    if (!fused_ok || stage_cap >= 0 || dev_scheme == 1 || per_cu > kLbfgsFusedFrames) return LbfgsScheme::two_launches;
    return dev_scheme != 2 && per_cu <= kLbfgsPersistentFrames ? LbfgsScheme::persistent : LbfgsScheme::fused_rounds;
}

// History pairs of one frame that fit into `bytes` of LDS behind the 2 H alphas (doubles): a pair is two vectors of P floats
// padded to whole 64-lane rows.
K2B_HD constexpr int lbfgs_staged_pairs(int bytes, int P, int H) {
    const int PL = (P + 63) / 64 * 64;
    const int head = 2 * H * (int)sizeof(double);
    const int pairs = (bytes - head) / (2 * PL * (int)sizeof(float));
    return pairs < 0 ? 0 : pairs;
}
// The three byte budgets the pairs are staged in.  Step kernel: 48 KiB, so that several frames share a CU.
K2B_HD constexpr int lbfgs_step_lds_bytes() { return 48 * 1024; }
// Fused prologue (LbMode::step / finalize): everything between the y exchange and the rim constants - y, J_dirs table, lo
// fragments, rim products, which nothing has written yet - shared out over the workgroup's frames in 16-byte units.
K2B_HD constexpr int lbfgs_prologue_lds_bytes(int frames_per_wg) {
    return ((fit_lds::MAXS * fit_lds::YX_STRIDE + 64 * fit_lds::DD_STRIDE_MAX + fit_lds::PLO_FLOATS + fit_lds::WX_FLOATS) * 4 / frames_per_wg) & ~15;
}
// Persistent loop: the half of the lo-fragment area the split shape never writes (components 0..3 keep theirs in registers).
K2B_HD constexpr int lbfgs_persistent_lds_bytes(int frames_per_wg) { return (fit_lds::PLO_FLOATS * 4 / 2 / frames_per_wg) & ~15; }

// ---- k2b_fit_tree_kernel ---------------------------------------------------------------------------------------------------------
constexpr int kTreeMaxFrames = 8;      // frames (waves) per workgroup: two per SIMD
struct FitTreePlan { int frames_per_wg, comp_waves, grid, block_threads, NS; bool chain; };
// Frames per workgroup: enough to cover the batch with one workgroup per CU; small batches get fewer waves per CU, so that every
// SIMD hosts at most one frame and all CUs work.  At most one frame per SIMD: four component waves ride along (one per SIMD)
// and take the mixture off the frame waves.  NS: the shape-coefficient capacity of the instantiation (20 = SMPL-X's betas |
// expression: twelve coefficients of padding cost 36 registers in the 32-wide one).
K2B_HD constexpr FitTreePlan plan_fit_tree(int num_frames, int num_cus, int num_shape, bool chain, int debug_shape) {
    int tw = clamp_int(ceil_div(num_frames, num_cus), 1, kTreeMaxFrames);
    const int comp_waves = debug_shape == TreeShape::plain ? 0 : ((tw <= 4 || debug_shape == TreeShape::comp_waves) ? 4 : 0);
    if (debug_shape == TreeShape::comp_waves && tw > 4) tw = 4;
    return FitTreePlan{tw, comp_waves, ceil_div(num_frames, tw), 64 * (tw + comp_waves), num_shape <= 16 ? 16 : (num_shape <= 20 ? 20 : 32), chain};
}

// ---- LBS -------------------------------------------------------------------------------------------------------------------------
// grid of the persistent vertex kernels: one workgroup per CU, a multiple of the 8 XCD labels, no more than the tiles need
K2B_HD constexpr int persistent_grid(int num_cus, long long tiles) {
    const int wgs = num_cus < 8 ? 8 : num_cus / 8 * 8;
    return tiles < wgs ? (int)((tiles + 7) / 8 * 8) : wgs;
}

}  // namespace k2b
