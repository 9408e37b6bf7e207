// k2b_shape.hip — the two small kernels around the fused kernel's evaluate-only launch in the batched shape pre-pass
// (k2b_shape_pass_lbfgs, k2b_api_lbfgs.hip): one independent L-BFGS over the betas of every sequence, all sequences together.
//
//   prep:   every frame's parameters from its sequence's current point - the shape row (betas, the model's remaining
//           coefficients 0) and the root-aligned translation  transl = y_root - (J_template[root] + J_dirs[root] beta)
//   reduce: every sequence's loss and gradient over its frames, in frame order (fixed: a sequence's numbers do not depend on
//           the other sequences of the batch), with the chain rule through the root alignment  g_beta - J_dirs[root]^T g_transl,
//           written where the L-BFGS state machine reads a closure result (zero outside the betas: nothing else moves)
#include "k2b_internal.h"

namespace k2b {
namespace {

__global__ __launch_bounds__(64) void k2b_shape_prep_kernel(const ShapePassArgs a) {
    const int s = blockIdx.x, lane = threadIdx.x;
    const int f0 = a.seq_off[s], f1 = a.seq_off[s + 1];
    const float* beta = a.be_state + (size_t)s * a.NB;          // the optimiser's point of sequence s (betas in front)
    float root = 0.f;
    if (lane < 3) {
        float acc = a.jt0[lane];
        for (int k = 0; k < a.nb; ++k) acc += a.jd0[lane * a.NB + k] * beta[k];
        root = acc;
    }
    for (int f = f0; f < f1; ++f) {
        if (lane < 3) a.tr_f[(size_t)f * 3 + lane] = a.root_y[(size_t)f * 3 + lane] - root;
        if (lane < a.NB) a.be_f[(size_t)f * a.NB + lane] = lane < a.nb ? beta[lane] : 0.f;
    }
}

__global__ __launch_bounds__(64) void k2b_shape_reduce_kernel(const ShapePassArgs a) {
    const int s = blockIdx.x, lane = threadIdx.x;
    const int f0 = a.seq_off[s], f1 = a.seq_off[s + 1];
    const int D = a.D, NB = a.NB, P = 3 + D + NB + 3;
    __shared__ float gtr[3];
    // lanes 0..nb-1: d/d beta_k; lanes 32..34: d/d transl_c; lane 40: the loss - each a sum over the frames in frame order
    float acc = 0.f;
    for (int f = f0; f < f1; ++f) {
        const float* g = a.grad_f + (size_t)f * P;
        if (lane < a.nb) acc += g[3 + D + lane];
        else if (lane >= 32 && lane < 35) acc += g[3 + D + NB + (lane - 32)];
        else if (lane == 40) acc += a.loss_f[f];
    }
    if (lane >= 32 && lane < 35) gtr[lane - 32] = acc;
    __syncthreads();
    float* gout = a.grad_state + (size_t)s * P;
    for (int p = lane; p < P; p += 64) gout[p] = 0.f;
    __syncthreads();
    if (lane < a.nb)           // d transl / d beta = -J_dirs[root]
        gout[3 + D + lane] = acc - (a.jd0[0 * NB + lane] * gtr[0] + a.jd0[1 * NB + lane] * gtr[1] + a.jd0[2 * NB + lane] * gtr[2]);
    if (lane == 40) a.loss_state[s] = acc;
}

}  // namespace

hipError_t launch_shape_prep(const ShapePassArgs& a, hipStream_t stream) {
    if (a.S <= 0) return hipSuccess;
    if (a.NB > 64 || a.nb > a.NB) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k2b_shape_prep_kernel, dim3(a.S), dim3(64), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_shape_reduce(const ShapePassArgs& a, hipStream_t stream) {
    if (a.S <= 0) return hipSuccess;
    if (a.nb > 32) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k2b_shape_reduce_kernel, dim3(a.S), dim3(64), 0, stream, a);
    return hipGetLastError();
}

}  // namespace k2b
