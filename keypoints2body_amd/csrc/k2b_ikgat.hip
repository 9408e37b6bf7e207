// k2b_ikgat.hip — batched inference of the IK-GAT rotation regressor (reference
// keypoints2body/core/estimators/ikgat/): joint positions (and, for the pos-rot6 variant, the
// previous quaternions) -> one unit quaternion per joint, xyzw, qw >= 0.
//
// One workgroup (256 threads, 4 waves) runs F frames at once as R = F*J node rows held in LDS:
//   preprocess  positions minus joint 0, quaternion -> rot6 (utils.py:13-26)          thread per row
//   input       h = input_proj(x) + joint_pos_embed                                    wave per row
//   L x GAT     [x' | a_src | a_dst] = h [W^T | W^T att_src | W^T att_dst] (block_mm: the extended projection,
//               transposed at create, staged through LDS in k-chunks and reused by all F frames); per row:
//               softmax over the CSR in-edges (self loop included), aggregation, + bias, ELU, LayerNorm,
//               + prev (l > 0)                                                          wave per row
//   residual    h += residual_proj(x)                                                   wave per row
//   head        Linear -> ReLU -> LayerNorm -> Linear(6)                                block_mm + wave per row
//   output      axes_to_rot6 + rot6 -> quaternion (inference.py:39-43, utils.py:29-52)  thread per row
// Every row's arithmetic depends on its own data and the weights only (the k-order of block_mm is fixed by K and
// KC, which the handle fixes), so a frame's output is bit-identical wherever it sits in the batch and for any B.
// Chain mode: one workgroup walks T frames with F = 1; frame t+1's input quaternions are frame t's outputs, kept in
// LDS (the same preprocessing code reads them), so the chain equals T single-frame calls bit for bit.
#include <hip/hip_runtime.h>

#include "k2b_internal.h"

namespace k2b {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kRT = 8;          // rows per block_mm work item

__device__ __forceinline__ float wave_sum(float v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// out[r][n] = sum_k A[r][k] * Wt[k][n] for r < R, n < N.  Wt is the weight matrix TRANSPOSED (K x N, row-major, laid out
// so by ikgat_pack, k2b_ikgat_plan.h); each k-chunk of KC rows is one contiguous block of at most kIkgatChunkFloats floats, copied into
// wb with 16-byte loads and reused by every row of the workgroup.  N, KC and the chunk offsets are multiples of 4.
// Starts and ends with a barrier.
__device__ void block_mm(const float* A, int lda, int R, int K, const float* __restrict__ Wt, int N, float* out, int ldo,
                         float* wb, int KC) {
    const int tid = threadIdx.x;
    const int items = ((R + kRT - 1) / kRT) * N;
    for (int k0 = 0; k0 < K; k0 += KC) {
        const int kc = min(KC, K - k0);
        __syncthreads();
        const float4* src = reinterpret_cast<const float4*>(Wt + (size_t)k0 * N);
        for (int i = tid; i < kc * N / 4; i += kThreads) reinterpret_cast<float4*>(wb)[i] = src[i];
        __syncthreads();
        for (int it = tid; it < items; it += kThreads) {
            const int n = it % N, r0 = (it / N) * kRT;
            int rows[kRT];
#pragma unroll
            for (int i = 0; i < kRT; ++i) rows[i] = min(r0 + i, R - 1) * lda + k0;
            float acc[kRT];
#pragma unroll
            for (int i = 0; i < kRT; ++i) acc[i] = 0.f;
            for (int k = 0; k < kc; k += 4) {          // K and KC are multiples of 4 (checked at create)
                const float w0 = wb[(k + 0) * N + n], w1 = wb[(k + 1) * N + n];
                const float w2 = wb[(k + 2) * N + n], w3 = wb[(k + 3) * N + n];
#pragma unroll
                for (int i = 0; i < kRT; ++i) {
                    const float4 a = *reinterpret_cast<const float4*>(A + rows[i] + k);
                    acc[i] = fmaf(a.x, w0, acc[i]);
                    acc[i] = fmaf(a.y, w1, acc[i]);
                    acc[i] = fmaf(a.z, w2, acc[i]);
                    acc[i] = fmaf(a.w, w3, acc[i]);
                }
            }
#pragma unroll
            for (int i = 0; i < kRT; ++i) {
                const int r = r0 + i;
                if (r < R) out[r * ldo + n] = (k0 == 0 ? 0.f : out[r * ldo + n]) + acc[i];
            }
        }
    }
    __syncthreads();
}

__device__ __forceinline__ void normalize3(float& x, float& y, float& z) {
    const float n = fmaxf(sqrtf(x * x + y * y + z * z), 1e-12f);      // F.normalize(eps=1e-12)
    x /= n; y /= n; z /= n;
}

// 6-D (two raw axes) -> unit quaternion xyzw: axes_to_rot6 (inference.py:39-43) then rot6_to_quat_torch (utils.py:29-52)
__device__ void rot6_to_quat(const float* o, float* q) {
    float a1x = o[0], a1y = o[1], a1z = o[2];
    normalize3(a1x, a1y, a1z);
    float d = a1x * o[3] + a1y * o[4] + a1z * o[5];
    float a2x = o[3] - d * a1x, a2y = o[4] - d * a1y, a2z = o[5] - d * a1z;
    normalize3(a2x, a2y, a2z);
    // rot6_to_quat_torch normalises both again
    float b1x = a1x, b1y = a1y, b1z = a1z;
    normalize3(b1x, b1y, b1z);
    d = b1x * a2x + b1y * a2y + b1z * a2z;
    float b2x = a2x - d * b1x, b2y = a2y - d * b1y, b2z = a2z - d * b1z;
    normalize3(b2x, b2y, b2z);
    const float b3x = b1y * b2z - b1z * b2y, b3y = b1z * b2x - b1x * b2z, b3z = b1x * b2y - b1y * b2x;
    // R = [b1 b2 b3] as columns: R[i][0] = b1[i], R[i][1] = b2[i], R[i][2] = b3[i]
    const float tr = b1x + b2y + b3z;
    const float qw = sqrtf(fmaxf(1.f + tr, 1e-8f)) * 0.5f;
    const float den = 4.f * qw + 1e-8f;
    const float qx = (b2z - b3y) / den;       // R21 - R12
    const float qy = (b3x - b1z) / den;       // R02 - R20
    const float qz = (b1y - b2x) / den;       // R10 - R01
    const float n = fmaxf(sqrtf(qx * qx + qy * qy + qz * qz + qw * qw), 1e-12f);
    q[0] = qx / n; q[1] = qy / n; q[2] = qz / n; q[3] = qw / n;
}

// quaternion xyzw -> first two columns of its rotation matrix (quat_to_6d, utils.py:13-26)
__device__ void quat_to_rot6(const float* qi, float* r) {
    float x = qi[0], y = qi[1], z = qi[2], w = qi[3];
    const float n = fmaxf(sqrtf(x * x + y * y + z * z + w * w), 1e-12f);
    x /= n; y /= n; z /= n; w /= n;
    r[0] = 1.f - 2.f * (y * y + z * z);
    r[1] = 2.f * (x * y + z * w);
    r[2] = 2.f * (x * z - y * w);
    r[3] = 2.f * (x * y - z * w);
    r[4] = 1.f - 2.f * (x * x + z * z);
    r[5] = 2.f * (y * z + x * w);
}

// LayerNorm over one row held by a wave, up to 4 values per lane (columns lane + 64 q); eps 1e-5 (nn.LayerNorm)
__device__ __forceinline__ void wave_layernorm(float (&v)[4], int lane, int n, const float* __restrict__ g,
                                               const float* __restrict__ b) {
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) if (lane + 64 * q < n) s += v[q];
    const float mean = wave_sum(s) / (float)n;
    float s2 = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) if (lane + 64 * q < n) { const float d = v[q] - mean; s2 += d * d; }
    const float inv = 1.f / sqrtf(wave_sum(s2) / (float)n + 1e-5f);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int c = lane + 64 * q;
        if (c < n) v[q] = (v[q] - mean) * inv * g[c] + b[c];
    }
}

__global__ __launch_bounds__(kThreads) void k2b_ikgat_kernel(IkgatArgs a) {
    extern __shared__ float lds[];
    const int J = a.J, H = a.H, NH = a.heads, C = H / NH, IN = a.in, H2 = H / 2, F = a.F, LDX = a.ldx;
    const int R = F * J;
    // the LDS regions and the weight pointers, once, from the descriptions of k2b_ikgat_plan.h (what each one holds is said there);
    // both before the graph copy: with the weight pointers after it the SGPR spill count moves (profiles/ikgat_plan_ab.txt)
    const IkgatLdsT<float*> map = ikgat_lds_map(lds, J, IN, H, LDX, a.nedges, F, a.KC);
    float *hb = map.hb, *xb = map.xb, *wb = map.wb, *xin = map.xin, *qv = map.qv;
    int* csr = reinterpret_cast<int*>(map.csr);

    const IkgatImageT<const float*> img = ikgat_image(a.w, J, IN, H, a.L, LDX);
    const float *w_in = img.w_in, *b_in = img.b_in, *emb = img.emb, *w_res = img.w_res, *b_res = img.b_res;
    const float *w1t = img.w1t, *b1 = img.b1, *g1 = img.g1, *be1 = img.be1, *w2t = img.w2t, *b2 = img.b2;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ncsr = J + 1 + a.nedges;
    for (int i = tid; i < ncsr; i += kThreads) csr[i] = a.csr[i];

    const int nsteps = a.chain ? a.B : 1;
    for (int step = 0; step < nsteps; ++step) {
        const int frame0 = a.chain ? step : blockIdx.x * F;
        __syncthreads();
        // ---- preprocess: one thread per row
        for (int r = tid; r < R; r += kThreads) {
            const int f = frame0 + r / J, j = r % J;
            const bool valid = f < a.B;
            float p[3] = {0.f, 0.f, 0.f};
            if (valid) {
                const float* P = a.pos + (size_t)f * J * 3;
                p[0] = P[j * 3 + 0] - P[0]; p[1] = P[j * 3 + 1] - P[1]; p[2] = P[j * 3 + 2] - P[2];
            }
            xin[r * IN + 0] = p[0]; xin[r * IN + 1] = p[1]; xin[r * IN + 2] = p[2];
            if (IN == 9) {
                if (!a.chain || step == 0) {
                    float q[4] = {0.f, 0.f, 0.f, 1.f};
                    if (valid) { const float* Q = a.quat_in + ((size_t)f * J + j) * 4; q[0] = Q[0]; q[1] = Q[1]; q[2] = Q[2]; q[3] = Q[3]; }
                    qv[r * 4 + 0] = q[0]; qv[r * 4 + 1] = q[1]; qv[r * 4 + 2] = q[2]; qv[r * 4 + 3] = q[3];
                }
                float r6[6];
                quat_to_rot6(qv + r * 4, r6);
#pragma unroll
                for (int k = 0; k < 6; ++k) xin[r * IN + 3 + k] = r6[k];
            }
        }
        __syncthreads();
        // ---- input projection + joint embedding
        for (int r = wave; r < R; r += kWaves) {
            const int j = r % J;
            for (int c = lane; c < H; c += 64) {
                float s = b_in[c];
                for (int k = 0; k < IN; ++k) s = fmaf(w_in[c * IN + k], xin[r * IN + k], s);
                hb[r * H + c] = s + emb[j * H + c];
            }
        }
        // ---- GAT layers: one block_mm gives x' = h W^T and the attention logits a_src = h (W^T att_src), a_dst likewise
        for (int l = 0; l < a.L; ++l) {
            const IkgatLayerT<const float*> layer = img.layer(l);
            const float *Wl = layer.w, *bias = layer.bias, *lng = layer.lng, *lnb = layer.lnb;
            block_mm(hb, H, R, H, Wl, LDX, xb, LDX, wb, a.KC);
            const float* as = xb + ikgat_col_src(H, NH);
            const float* ad = xb + ikgat_col_dst(H, NH);
            for (int r = wave; r < R; r += kWaves) {
                const int base = (r / J) * J, node = r % J;
                const int e0 = csr[node], e1 = csr[node + 1];
                float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int c = lane + 64 * q;
                    if (c >= H) continue;
                    const int hd = c / C;
                    const float adst = ad[r * LDX + hd];
                    float m = -INFINITY;
                    for (int e = e0; e < e1; ++e) {
                        float s = as[(base + csr[J + 1 + e]) * LDX + hd] + adst;
                        s = s > 0.f ? s : 0.2f * s;
                        m = fmaxf(m, s);
                    }
                    float den = 0.f, acc = 0.f;
                    for (int e = e0; e < e1; ++e) {
                        const int src = base + csr[J + 1 + e];
                        float s = as[src * LDX + hd] + adst;
                        s = s > 0.f ? s : 0.2f * s;
                        const float ex = expf(s - m);
                        den += ex;
                        acc = fmaf(ex, xb[src * LDX + c], acc);
                    }
                    acc /= den + 1e-16f;                         // = sum_j alpha_j x'_j with PyG's alpha = ex / (sum + 1e-16)
                    const float y = acc + bias[c];
                    v[q] = y > 0.f ? y : expm1f(y);              // ELU(alpha = 1)
                }
                wave_layernorm(v, lane, H, lng, lnb);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int c = lane + 64 * q;
                    if (c < H) hb[r * H + c] = l > 0 ? v[q] + hb[r * H + c] : v[q];
                }
            }
        }
        __syncthreads();
        // ---- h += residual_proj(x)
        for (int r = wave; r < R; r += kWaves) {
            for (int c = lane; c < H; c += 64) {
                float s = b_res[c];
                for (int k = 0; k < IN; ++k) s = fmaf(w_res[c * IN + k], xin[r * IN + k], s);
                hb[r * H + c] += s;
            }
        }
        // ---- output head: Linear(H, H/2) -> ReLU -> LayerNorm -> Linear(H/2, 6)
        block_mm(hb, H, R, H, w1t, H2, xb, LDX, wb, a.KC);
        for (int r = wave; r < R; r += kWaves) {
            float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int c = lane + 64 * q;
                if (c < H2) v[q] = fmaxf(xb[r * LDX + c] + b1[c], 0.f);
            }
            wave_layernorm(v, lane, H2, g1, be1);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int c = lane + 64 * q;
                if (c < H2) xb[r * LDX + c] = v[q];
            }
        }
        block_mm(xb, LDX, R, H2, w2t, kIkgatOutCols, hb, kIkgatOutCols, wb, a.KC);
        // ---- 6-D -> quaternion
        for (int r = tid; r < R; r += kThreads) {
            float o[6], q[4];
#pragma unroll
            for (int k = 0; k < 6; ++k) o[k] = hb[r * kIkgatOutCols + k] + b2[k];
            rot6_to_quat(o, q);
            const int f = frame0 + r / J;
            if (f < a.B) {
                float* Q = a.quat_out + ((size_t)f * J + (r % J)) * 4;
                Q[0] = q[0]; Q[1] = q[1]; Q[2] = q[2]; Q[3] = q[3];
            }
            if (a.chain) { qv[r * 4 + 0] = q[0]; qv[r * 4 + 1] = q[1]; qv[r * 4 + 2] = q[2]; qv[r * 4 + 3] = q[3]; }
        }
    }
}

std::atomic<unsigned long long> g_ikgat_lds_done{0};

}  // namespace

hipError_t launch_ikgat(const IkgatArgs& a, const IkgatLaunch& launch, hipStream_t stream) {
    hipError_t e = ensure_dynamic_lds(k2b_ikgat_kernel, g_ikgat_lds_done, kIkgatMaxLds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k2b_ikgat_kernel, dim3(launch.grid), dim3(kThreads), launch.lds_bytes, stream, a);
    return hipGetLastError();
}

}  // namespace k2b
