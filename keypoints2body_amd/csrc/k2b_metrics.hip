// k2b_metrics.hip — the metrics of the evaluation path on the GPU: the pose error (MPJAE) and the positional errors
// (MPJPE / PA-MPJPE / PVE, second half of the file).
//
// MPJAE: one thread per pair of axis-angle rotations: geodesic angle in degrees between them, following the
// reference's float32 arithmetic step by step (keypoints2body/cli/eval.py: rotvec_to_rotmat :88-128,
// compute_angular_error_deg :131-140): R = I + a K + b K^2 with a = sin t / t, b = (1 - cos t) / t^2
// (Taylor series for t <= 1e-8), trace of the elementwise product of the two matrices,
// cos = (trace - 1) / 2 clipped to [-1 + 1e-6, 1 - 1e-6], arccos, degrees.
// Streaming kernel: 24 B in + 4 B out per pair, HBM-bound; precise sinf / cosf / acosf on purpose (the
// metric is compared with the reference's, not timed against a roofline that matters).
#include "k2b_internal.h"

namespace k2b {

namespace {

struct M9 { float m[9]; };

__device__ __forceinline__ M9 rotmat_of(float x, float y, float z) {
    const float t2 = x * x + y * y + z * z;
    const float t = sqrtf(t2);
    float a, b;
    if (t > 1e-8f) {
        a = sinf(t) / t;
        b = (1.0f - cosf(t)) / (t * t);
    } else {
        a = 1.0f - t2 / 6.0f + (t2 * t2) / 120.0f;
        b = 0.5f - t2 / 24.0f + (t2 * t2) / 720.0f;
    }
    const float xy = x * y, xz = x * z, yz = y * z, xx = x * x, yy = y * y, zz = z * z;
    M9 r;
    r.m[0] = 1.0f - b * (yy + zz); r.m[1] = b * xy - a * z;        r.m[2] = b * xz + a * y;
    r.m[3] = b * xy + a * z;        r.m[4] = 1.0f - b * (xx + zz); r.m[5] = b * yz - a * x;
    r.m[6] = b * xz - a * y;        r.m[7] = b * yz + a * x;        r.m[8] = 1.0f - b * (xx + yy);
    return r;
}

__global__ __launch_bounds__(256) void k2b_angular_error_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                                float* __restrict__ out, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const M9 p = rotmat_of(pred[3 * i], pred[3 * i + 1], pred[3 * i + 2]);
    const M9 g = rotmat_of(gt[3 * i], gt[3 * i + 1], gt[3 * i + 2]);
    float tr = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) tr += p.m[k] * g.m[k];
    float c = (tr - 1.0f) * 0.5f;
    c = fminf(fmaxf(c, -1.0f + 1e-6f), 1.0f - 1e-6f);
    out[i] = acosf(c) * 57.29577951308232f;
}

// ---- positional error after an alignment (k2b_point_error) ---------------------------------------------------------------
// Per frame: err = sum_i w_i |a(x_i) - y_i| / sum_i w_i with a = identity, translation, rigid (Kabsch) or similarity (Umeyama).
// Three passes over the frame's points - weighted centroids, centred cross-covariance and variance, residuals - all in float64
// (for the test tolerance of 2^-22 relative; at small N the decomposition is most of the time), one rounding to
// float32 on store.
// The rotation is Horn's closed form: the unit quaternion that maximises q^T N q for the symmetric 4x4 N built from the
// covariance, i.e. the eigenvector of N's largest eigenvalue.  That maximum runs over proper rotations only, so the mirrored
// case needs no separate determinant correction, and the eigenvalue itself is Umeyama's trace(D S): scale = lambda / var(x).
// Eigenvectors by cyclic Jacobi: kJacobiSweeps sweeps of the six plane rotations, a fixed count.  The off-diagonal norm falls
// quadratically once it is small: on the covariances of the test cases and on 3500 random full-rank, scaled and rank-one ones,
// 5 sweeps always brought it below 1e-15 of the largest entry (4 for most); 8 leaves a margin of three sweeps.  No loop
// here runs "until converged": a NaN goes through the same instructions and comes out as that frame's NaN.
// Sums have one fixed order - a lane's points in index order, the xor butterfly over the wave, then the four wave partials
// (w0 + w1) + (w2 + w3) - so a frame's outputs are the same bits in any batch, at any position.
constexpr int kJacobiSweeps = 8;

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);       // every lane ends with the same bits: a + b == b + a
    return v;
}

// sums K values over the frame's lanes: the wave (WAVE) or the workgroup's four waves through `lds` [4][K]
template <bool WAVE, int K>
__device__ __forceinline__ void frame_sum(double (&v)[K], double* lds, int wave, int lane) {
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = wave_sum_f64(v[k]);
    if constexpr (!WAVE) {
        __syncthreads();                                              // the previous sums have been read
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < K; ++k) lds[wave * K + k] = v[k];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] = (lds[k] + lds[K + k]) + (lds[2 * K + k] + lds[3 * K + k]);
    }
}

// the same for maxima of floats (exact, so any order would do; `lds` [4][K])
template <bool WAVE, int K>
__device__ __forceinline__ void frame_max(float (&v)[K], float* lds, int wave, int lane) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[k] = fmaxf(v[k], __shfl_xor(v[k], o, 64));
    }
    if constexpr (!WAVE) {
        __syncthreads();
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < K; ++k) lds[wave * K + k] = v[k];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] = fmaxf(fmaxf(lds[k], lds[K + k]), fmaxf(lds[2 * K + k], lds[3 * K + k]));
    }
}

template <int P, int Q>
__device__ __forceinline__ void jacobi_rotate(double (&a)[4][4], double (&v)[4][4]) {
    const double apq = a[P][Q];
    const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
    const double tt = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double t = apq != 0.0 ? tt : 0.0;                           // (a NaN takes tt, and stays a NaN)
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    a[P][P] -= t * apq;
    a[Q][Q] += t * apq;
    a[P][Q] = a[Q][P] = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (r != P && r != Q) {
            const double arp = a[r][P], arq = a[r][Q];
            a[r][P] = a[P][r] = c * arp - s * arq;
            a[r][Q] = a[Q][r] = s * arp + c * arq;
        }
        const double vrp = v[r][P], vrq = v[r][Q];
        v[r][P] = c * vrp - s * vrq;
        v[r][Q] = s * vrp + c * vrq;
    }
}

// Proper rotation R (row-major) that maximises trace(R S^T), S[a][b] = sum w (x - cx)_a (y - cy)_b; returns the maximum.
__device__ __forceinline__ double horn_rotation(const double (&S)[9], double (&R)[9]) {
    double a[4][4], v[4][4];
    a[0][0] = S[0] + S[4] + S[8];
    a[1][1] = S[0] - S[4] - S[8];
    a[2][2] = -S[0] + S[4] - S[8];
    a[3][3] = -S[0] - S[4] + S[8];
    a[0][1] = a[1][0] = S[5] - S[7];
    a[0][2] = a[2][0] = S[6] - S[2];
    a[0][3] = a[3][0] = S[1] - S[3];
    a[1][2] = a[2][1] = S[1] + S[3];
    a[1][3] = a[3][1] = S[6] + S[2];
    a[2][3] = a[3][2] = S[5] + S[7];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) v[r][c] = r == c ? 1.0 : 0.0;
#pragma unroll 1
    for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
        jacobi_rotate<0, 1>(a, v); jacobi_rotate<0, 2>(a, v); jacobi_rotate<0, 3>(a, v);
        jacobi_rotate<1, 2>(a, v); jacobi_rotate<1, 3>(a, v); jacobi_rotate<2, 3>(a, v);
    }
    double lam = a[0][0], qw = v[0][0], qx = v[1][0], qy = v[2][0], qz = v[3][0];
#pragma unroll
    for (int k = 1; k < 4; ++k) {
        const bool up = a[k][k] > lam;                                // the first of equal maxima, in index order
        lam = up ? a[k][k] : lam;
        qw = up ? v[0][k] : qw; qx = up ? v[1][k] : qx; qy = up ? v[2][k] : qy; qz = up ? v[3][k] : qz;
    }
    const double inv = 1.0 / sqrt(qw * qw + qx * qx + qy * qy + qz * qz);
    qw *= inv; qx *= inv; qy *= inv; qz *= inv;
    R[0] = qw * qw + qx * qx - qy * qy - qz * qz; R[1] = 2.0 * (qx * qy - qw * qz);             R[2] = 2.0 * (qx * qz + qw * qy);
    R[3] = 2.0 * (qx * qy + qw * qz);             R[4] = qw * qw - qx * qx + qy * qy - qz * qz; R[5] = 2.0 * (qy * qz - qw * qx);
    R[6] = 2.0 * (qx * qz - qw * qy);             R[7] = 2.0 * (qy * qz + qw * qx);             R[8] = qw * qw - qx * qx - qy * qy + qz * qz;
    return lam;
}

// A frame's points as its lanes see them.  WAVE: lane l holds points l, l + 64, l + 128, l + 192 in registers (read once; a
// slot past the end is a point at the origin with weight 0).  Otherwise thread t strides over points t, t + 256, ... and
// reads them again in every pass.
template <bool WAVE>
struct FramePoints {
    static constexpr int kSlots = WAVE ? kPointErrorWavePoints / 64 : 1;
    const float *x, *y, *w;
    int n, first;
    float rx[kSlots][3], ry[kSlots][3], rw[kSlots];

    __device__ __forceinline__ void read(int i, float (&px)[3], float (&py)[3], float& pw) const {
        const long long o = 3ll * i;
        px[0] = x[o]; px[1] = x[o + 1]; px[2] = x[o + 2];
        py[0] = y[o]; py[1] = y[o + 1]; py[2] = y[o + 2];
        pw = w ? w[i] : 1.0f;
    }
    __device__ __forceinline__ void load() {
        if constexpr (WAVE) {
#pragma unroll
            for (int k = 0; k < kSlots; ++k) {
                const int i = first + 64 * k;
                rx[k][0] = rx[k][1] = rx[k][2] = ry[k][0] = ry[k][1] = ry[k][2] = rw[k] = 0.0f;
                if (i < n) read(i, rx[k], ry[k], rw[k]);
            }
        }
    }
    // f(i, x, y, w) for each of this lane's points, in index order (WAVE: also for the empty slots, i >= n)
    template <class F>
    __device__ __forceinline__ void each(F&& f) const {
        if constexpr (WAVE) {
#pragma unroll
            for (int k = 0; k < kSlots; ++k) f(first + 64 * k, rx[k], ry[k], rw[k]);
        } else {
            for (int i = first; i < n; i += 256) {
                float px[3], py[3], pw;
                read(i, px, py, pw);
                f(i, px, py, pw);
            }
        }
    }
};

template <bool WAVE>
__global__ __launch_bounds__(256) void k2b_point_error_kernel(const PointErrorArgs a) {
    __shared__ double lds[WAVE ? 1 : 4 * 10];                         // the wave regime never touches LDS (the compiler drops both)
    __shared__ float lds_f[WAVE ? 1 : 4 * 6];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long b = WAVE ? 4ll * blockIdx.x + wave : (long long)blockIdx.x;
    if (b >= a.num_frames) return;                                    // (WAVE only, a whole wave: it meets no barrier)
    const int n = a.num_points, mode = a.align_mode;
    const long long base = b * n;
    FramePoints<WAVE> pts;
    pts.x = a.pred + 3 * base;
    pts.y = a.gt + 3 * base;
    pts.w = a.weights ? a.weights + (a.weights_per_frame ? base : 0ll) : nullptr;
    pts.n = n;
    pts.first = WAVE ? lane : (int)threadIdx.x;
    pts.load();

    // pass 1: total weight and weighted centroids
    double m[7] = {0, 0, 0, 0, 0, 0, 0};
    pts.each([&](int, const float (&x)[3], const float (&y)[3], float w) {
        const double wd = w;
        m[0] += wd;
#pragma unroll
        for (int c = 0; c < 3; ++c) { m[1 + c] += wd * (double)x[c]; m[4 + c] += wd * (double)y[c]; }
    });
    frame_sum<WAVE>(m, lds, wave, lane);
    const double W = m[0];
    const bool empty = W == 0.0;                                      // no weight at all: error 0, identity transform
    double cx[3] = {0, 0, 0}, cy[3] = {0, 0, 0};
    if (mode != 0 && !empty) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { cx[c] = m[1 + c] / W; cy[c] = m[4 + c] / W; }
    }

    // pass 2: centred cross-covariance and the variance of x, then the rotation and the scale
    double s = 1.0, R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (mode >= 2) {                                                  // (uniform over the launch)
        // Do all weighted points of x coincide?  Asked of the float32 inputs themselves (largest == smallest per coordinate,
        // the smallest as the largest negation), because the rounded centroid of equal points need not equal them.
        float ext[6] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY, -INFINITY, -INFINITY};
        pts.each([&](int, const float (&x)[3], const float (&)[3], float w) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                ext[c] = w != 0.0f ? fmaxf(ext[c], x[c]) : ext[c];
                ext[3 + c] = w != 0.0f ? fmaxf(ext[3 + c], -x[c]) : ext[3 + c];
            }
        });
        frame_max<WAVE>(ext, lds_f, wave, lane);
        const bool same = ext[0] == -ext[3] && ext[1] == -ext[4] && ext[2] == -ext[5];
        if (same) { cx[0] = ext[0]; cx[1] = ext[1]; cx[2] = ext[2]; }
        double cv[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        pts.each([&](int, const float (&x)[3], const float (&y)[3], float w) {
            const double wd = w;
            const double dx[3] = {(double)x[0] - cx[0], (double)x[1] - cx[1], (double)x[2] - cx[2]};
            const double dy[3] = {(double)y[0] - cy[0], (double)y[1] - cy[1], (double)y[2] - cy[2]};
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const double wx = wd * dx[r];
#pragma unroll
                for (int c = 0; c < 3; ++c) cv[3 * r + c] += wx * dy[c];
                cv[9] += wx * dx[r];
            }
        });
        frame_sum<WAVE>(cv, lds, wave, lane);
        const double S[9] = {cv[0], cv[1], cv[2], cv[3], cv[4], cv[5], cv[6], cv[7], cv[8]};
        double Rh[9];
        const double lam = horn_rotation(S, Rh);
        const bool flat = same || cv[9] == 0.0 || empty;              // every weighted x at the centroid: R = I, s = 1
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = flat ? R[k] : Rh[k];
        if (mode == 3) s = flat ? 1.0 : lam / cv[9];
    }

    // pass 3: residuals of the centred form s R (x - cx) - (y - cy), which is a(x) - y with t = cy - s R cx
    double e[1] = {0};
    float* pp = a.per_point ? a.per_point + base : nullptr;
    pts.each([&](int i, const float (&x)[3], const float (&y)[3], float w) {
        const double dx[3] = {(double)x[0] - cx[0], (double)x[1] - cx[1], (double)x[2] - cx[2]};
        double d2 = 0.0;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double d = s * (R[3 * r] * dx[0] + R[3 * r + 1] * dx[1] + R[3 * r + 2] * dx[2]) - ((double)y[r] - cy[r]);
            d2 += d * d;
        }
        const double d = empty ? 0.0 : sqrt(d2);
        e[0] += (double)w * d;
        if (pp && i < n) pp[i] = (float)d;
    });
    frame_sum<WAVE>(e, lds, wave, lane);
    const bool writer = WAVE ? lane == 0 : threadIdx.x == 0;
    if (!writer) return;
    a.err[b] = empty ? 0.0f : (float)(e[0] / W);
    if (a.transform) {
        float* t = a.transform + 13 * b;
        t[0] = (float)s;
#pragma unroll
        for (int k = 0; k < 9; ++k) t[1 + k] = (float)R[k];
#pragma unroll
        for (int r = 0; r < 3; ++r) t[10 + r] = (float)(cy[r] - s * (R[3 * r] * cx[0] + R[3 * r + 1] * cx[1] + R[3 * r + 2] * cx[2]));
    }
}

}  // namespace

hipError_t launch_angular_error(const float* pred, const float* gt, float* out, long long n, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    const long long blocks = (n + 255) / 256;
    hipLaunchKernelGGL(k2b_angular_error_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, pred, gt, out, n);
    return hipGetLastError();
}

hipError_t launch_point_error(const PointErrorArgs& a, hipStream_t stream) {
    if (a.num_frames <= 0) return hipSuccess;
    const dim3 grid((unsigned)point_error_workgroups(a.num_frames, a.num_points));
    if (a.num_points <= kPointErrorWavePoints) hipLaunchKernelGGL(k2b_point_error_kernel<true>, grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(k2b_point_error_kernel<false>, grid, dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace k2b
