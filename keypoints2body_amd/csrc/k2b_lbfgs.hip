// k2b_lbfgs.hip — device-resident L-BFGS with strong-Wolfe line search, one independent optimiser per frame.
//
// The reference's DEFAULT optimiser is `torch.optim.LBFGS(params, max_iter=num_iters, lr=step_size,
// line_search_fn="strong_wolfe").step(closure)` per frame (keypoints2body/core/fitters/world_space.py:231-247,
// core/fitters/camera_space.py:144-182,229-267; core/config.py:29 `use_lbfgs=True`).  Its closure - loss and gradient at the
// current parameters - is the fused fit kernel in evaluate-only mode.  Rounds 2-3 drove the optimiser from the host (torch's own
// class for one frame: an upload, a launch and a download per closure call, 6.9 ms per fit; a vectorised numpy restatement,
// core/lbfgs_batched.py, for batches).  Here the optimiser's state machine itself runs on the device:
//
//   * torch's algorithm (LBFGS.step, _strong_wolfe, _cubic_interpolate: two-loop recursion, bracket phase, zoom phase with its
//     insufficient-progress rule, the tolerance / max_iter / max_eval exits) restated as a per-frame state machine
//     INIT -> (BRACKET | ZOOM)* -> DONE that consumes ONE closure result per call and names the next point to evaluate;
//   * one wavefront per frame (k2b_lbfgs_device.h): vectors three elements per lane (<= 192 parameters; four, <= 256, in the
//     step kernel's wide form for the 55- and 63-joint models beyond that), in registers for the whole step; state and history
//     (2 H P floats) in global memory between steps, the history staged in LDS for the two-loop
//     recursion; inner products reduced over the wave in double (DPP scan), scalars in double where torch holds Python floats;
//     no FMA contraction (the code is inlined into three kernels and must round alike in each);
//   * the host only ENQUEUES a fixed number of [closure, step] rounds - max_eval + 2, the most any frame can need - without
//     reading anything back: frames that finish early idle at their final point.  No host synchronisation, no PCIe traffic.
//     THREE ways the rounds reach the device, by the batch size, bit-identical (tests/test_gpu_lbfgs.py):
//       - at most two frames per CU: ONE persistent launch of the fused fit kernel (LbMode::persistent) - the closures are
//         iterations of its loop, the optimiser lives on an idle wave of the workgroup with its state resident; with chain_len
//         frames the same launch runs the whole warm-start sequence (k2b_fit_sequence_lbfgs);
//       - at most four: one launch per round, the step as a prologue of the closure's launch (LbMode::step / finalize);
//       - beyond, and for the larger models: two launches per round - the closure's, and k2b_lbfgs_step_kernel below.
//
// CPU twin: keypoints2body_amd/core/lbfgs_batched.py (itself pinned to torch.optim.LBFGS iterate by iterate in float64,
// tests/test_lbfgs_batched.py); tests/test_gpu_lbfgs.py compares the two on the real closure.
#include "k2b_internal.h"
#include "k2b_lbfgs_device.h"

namespace k2b {

using namespace lbfgs_dev;

// EPL = vector elements per lane: kEpl for P <= 192, kEplWide for P <= 256
template <int EPL>
__global__ __launch_bounds__(64) void k2b_lbfgs_step_kernel(const LbfgsArgs a, int lds_pairs) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lbfgs_lds[];
    lbfgs_step_frame<EPL>(a, blockIdx.x, threadIdx.x, lbfgs_lds, lds_pairs);
}

// start of one frame of a warm-start sequence: parameters and preserve pose from their sources (the previous frame's result),
// the optimiser's scalars and integers cleared (phase INIT) - one launch instead of five copies and a memset
__global__ __launch_bounds__(256) void k2b_lbfgs_frame_prep_kernel(float* go, const float* sgo, float* bp, const float* sbp, float* be,
                                                                   const float* sbe, float* tr, const float* str, float* pres, int D, int NB,
                                                                   unsigned int* state, int state_words) {
    const int i = threadIdx.x;
    for (int e = i; e < D; e += 256) { const float v = sbp[e]; bp[e] = v; pres[e] = v; }
    for (int e = i; e < NB; e += 256) be[e] = sbe[e];
    if (i < 3) { go[i] = sgo[i]; tr[i] = str[i]; }
    for (int e = i; e < state_words; e += 256) state[e] = 0u;
}

hipError_t launch_lbfgs_frame_prep(float* go, const float* sgo, float* bp, const float* sbp, float* be, const float* sbe, float* tr,
                                   const float* str, float* pres, int D, int NB, void* state, size_t state_bytes, hipStream_t stream) {
    hipLaunchKernelGGL(k2b_lbfgs_frame_prep_kernel, dim3(1), dim3(256), 0, stream, go, sgo, bp, sbp, be, sbe, tr, str, pres, D, NB,
                       reinterpret_cast<unsigned int*>(state), (int)(state_bytes / 4));
    return hipGetLastError();
}

hipError_t launch_lbfgs_step(const LbfgsArgs& a, hipStream_t stream, int max_staged_pairs) {
    if (a.B <= 0) return hipSuccess;
    const LbfgsStepPlan p = plan_lbfgs_step(a.P, a.H, a.max_iter, max_staged_pairs);
    if (!p.ok) return hipErrorInvalidValue;
    if (!p.wide) hipLaunchKernelGGL(k2b_lbfgs_step_kernel<kEpl>, dim3(a.B), dim3(64), (size_t)p.lds_bytes, stream, a, p.pairs);
    else hipLaunchKernelGGL(k2b_lbfgs_step_kernel<kEplWide>, dim3(a.B), dim3(64), (size_t)p.lds_bytes, stream, a, p.pairs);
    return hipGetLastError();
}

}  // namespace k2b
