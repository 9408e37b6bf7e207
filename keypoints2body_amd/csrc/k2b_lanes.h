// LDS-free cross-lane primitives shared by the fit kernels (gfx950 / CDNA4, wave64): DPP row operations,
// v_permlane16/32_swap exchanges, reductions and scans built from them.
#pragma once
#include <hip/hip_runtime.h>

namespace k2b {

// ---- subtree sums of the fit kernel's tree pass: two forms ----------------------------------------
// Both are inclusive prefix sums inside each 32-lane half with DPP (no LDS traffic): Hillis-Steele inside each row of 16
// (row_shr 1, 2, 4, 8; out-of-row sources read 0), then row_bcast:15 into rows 1 and 3.
//
// fp32, no difference (chain_end_scans; models with a scan plan, k2b_scan_plan.h).  The tree lanes are in REVERSED DFS order,
// so a subtree is the lane range that ends at its joint, and every joint takes one of two prefixes as it stands: the unmasked
// prefix U over the half-wave (its subtree is everything up to its lane) or the prefix C along its own chain, whose steps
// (shifts 1, 2, 4) are masked per lane so that it stops at the chain's leaf.  Nothing from outside a subtree enters its sum: the
// error is <= (n - 1) 2^-24 sum |terms of that subtree|, the class of an fp32 autograd sum.
//
// fp64, a difference of two prefixes (half_wave_inclusive_scan(s) + a ds_bpermute per sum; every other tree, lanes in DFS order,
// a subtree = the lane range that STARTS at its joint).  Accumulated in DOUBLE: in fp32 the absolute error of the difference
// (eps x the largest prefix) was visible after Adam's per-parameter normalisation (parity 3e-6 -> up to 9e-5); in double the
// differences are exact to fp32.  An fp64 add issues at half the fp32 rate and moves as two DPP copies: four issue slots per
// scan step against one.

// NS values side by side (3 or 6).  m1, m2, m4: 1.0f where the chain scan's step with that shift adds the lower lane's value, else
// 0.0f (x 1 and x 0 in a fused multiply-add: the sum is that of a plain add, and a masked step adds an exact zero); take_u: the
// lane's sum is U, else C.  One instruction per value and step, in place: v_add_f32_dpp for U, v_fmac_f32_dpp for C (a lane whose
// DPP source lies outside its row, or whose row the row mask leaves out, keeps its value).  Per value the adds are the same in the
// same order wherever this is inlined.
// (Inline asm: the compiler forms neither the fused multiply-add with a DPP operand nor the row-masked add - 84 instructions for
//  six values against 54.  Inside the string nobody inserts the two wait states between a VALU write of a register and a DPP read
//  of it: the leading s_nop covers the values' producers, and the instructions are ordered step by step over all values, U and C
//  alternating, so that at least two others lie between a write and the DPP read of the same register - also from the row_shr:8
//  step to the row_bcast:15 step of three values.)
#define K2B_SCAN_U(u, ctl) "v_add_f32_dpp " u ", " u ", " u " " ctl " bank_mask:0xf bound_ctrl:1\n\t"
#define K2B_SCAN_C(c, m, shr) "v_fmac_f32_dpp " c ", " c ", " m " row_shr:" shr " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
#define K2B_SCAN_STEP3(shr, m) \
    K2B_SCAN_U("%0", "row_shr:" shr " row_mask:0xf") K2B_SCAN_C("%3", m, shr) K2B_SCAN_U("%1", "row_shr:" shr " row_mask:0xf") \
    K2B_SCAN_C("%4", m, shr) K2B_SCAN_U("%2", "row_shr:" shr " row_mask:0xf") K2B_SCAN_C("%5", m, shr)
#define K2B_SCAN_STEP6(shr, m) \
    K2B_SCAN_U("%0", "row_shr:" shr " row_mask:0xf") K2B_SCAN_C("%6", m, shr) K2B_SCAN_U("%1", "row_shr:" shr " row_mask:0xf") \
    K2B_SCAN_C("%7", m, shr) K2B_SCAN_U("%2", "row_shr:" shr " row_mask:0xf") K2B_SCAN_C("%8", m, shr) \
    K2B_SCAN_U("%3", "row_shr:" shr " row_mask:0xf") K2B_SCAN_C("%9", m, shr) K2B_SCAN_U("%4", "row_shr:" shr " row_mask:0xf") \
    K2B_SCAN_C("%10", m, shr) K2B_SCAN_U("%5", "row_shr:" shr " row_mask:0xf") K2B_SCAN_C("%11", m, shr)
template <int NS>
__device__ __forceinline__ void chain_end_scans(const float (&v)[NS], float (&s)[NS], float m1, float m2, float m4, bool take_u) {
    float u[NS], c[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) u[i] = c[i] = v[i];
    if constexpr (NS == 3)
        asm("s_nop 1\n\t" K2B_SCAN_STEP3("1", "%6") K2B_SCAN_STEP3("2", "%7") K2B_SCAN_STEP3("4", "%8")
            K2B_SCAN_U("%0", "row_shr:8 row_mask:0xf") K2B_SCAN_U("%1", "row_shr:8 row_mask:0xf") K2B_SCAN_U("%2", "row_shr:8 row_mask:0xf")
            K2B_SCAN_U("%0", "row_bcast:15 row_mask:0xa") K2B_SCAN_U("%1", "row_bcast:15 row_mask:0xa") K2B_SCAN_U("%2", "row_bcast:15 row_mask:0xa")
            : "+v"(u[0]), "+v"(u[1]), "+v"(u[2]), "+v"(c[0]), "+v"(c[1]), "+v"(c[2])
            : "v"(m1), "v"(m2), "v"(m4));
    else if constexpr (NS == 6)
        asm("s_nop 1\n\t" K2B_SCAN_STEP6("1", "%12") K2B_SCAN_STEP6("2", "%13") K2B_SCAN_STEP6("4", "%14")
            K2B_SCAN_U("%0", "row_shr:8 row_mask:0xf") K2B_SCAN_U("%1", "row_shr:8 row_mask:0xf") K2B_SCAN_U("%2", "row_shr:8 row_mask:0xf")
            K2B_SCAN_U("%3", "row_shr:8 row_mask:0xf") K2B_SCAN_U("%4", "row_shr:8 row_mask:0xf") K2B_SCAN_U("%5", "row_shr:8 row_mask:0xf")
            K2B_SCAN_U("%0", "row_bcast:15 row_mask:0xa") K2B_SCAN_U("%1", "row_bcast:15 row_mask:0xa") K2B_SCAN_U("%2", "row_bcast:15 row_mask:0xa")
            K2B_SCAN_U("%3", "row_bcast:15 row_mask:0xa") K2B_SCAN_U("%4", "row_bcast:15 row_mask:0xa") K2B_SCAN_U("%5", "row_bcast:15 row_mask:0xa")
            : "+v"(u[0]), "+v"(u[1]), "+v"(u[2]), "+v"(u[3]), "+v"(u[4]), "+v"(u[5]), "+v"(c[0]), "+v"(c[1]), "+v"(c[2]), "+v"(c[3]),
              "+v"(c[4]), "+v"(c[5])
            : "v"(m1), "v"(m2), "v"(m4));
    else static_assert(NS < 0, "no scan group of this size");
#pragma unroll
    for (int i = 0; i < NS; ++i) s[i] = take_u ? u[i] : c[i];
}
#undef K2B_SCAN_U
#undef K2B_SCAN_C
#undef K2B_SCAN_STEP3
#undef K2B_SCAN_STEP6

__device__ __forceinline__ double half_wave_inclusive_scan(float v) {
    double s = (double)v;
#define K2B_DPP_ADD64(ctrl, row_mask)                                                                   \
    {                                                                                                   \
        const long long bits = __builtin_bit_cast(long long, s);                                        \
        const int lo = __builtin_amdgcn_update_dpp(0, (int)(bits & 0xffffffffll), ctrl, row_mask, 0xf, true); \
        const int hi = __builtin_amdgcn_update_dpp(0, (int)(bits >> 32), ctrl, row_mask, 0xf, true);    \
        s += __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned int)lo);                      \
    }
    K2B_DPP_ADD64(0x111, 0xf);   // row_shr:1
    K2B_DPP_ADD64(0x112, 0xf);   // row_shr:2
    K2B_DPP_ADD64(0x114, 0xf);   // row_shr:4
    K2B_DPP_ADD64(0x118, 0xf);   // row_shr:8
    K2B_DPP_ADD64(0x142, 0xa);   // row_bcast:15 -> rows 1, 3 (lanes 16..31 and 48..63)
#undef K2B_DPP_ADD64
    return s;
}

__device__ __forceinline__ double bperm64(int byte_addr, double v) {
    const long long bits = __builtin_bit_cast(long long, v);
    const int lo = __builtin_amdgcn_ds_bpermute(byte_addr, (int)(bits & 0xffffffffll));
    const int hi = __builtin_amdgcn_ds_bpermute(byte_addr, (int)(bits >> 32));
    return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned int)lo);
}

__device__ __forceinline__ float bperm(int byte_addr, float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(byte_addr, __builtin_bit_cast(int, v)));
}

// ---- LDS-free cross-lane exchanges (gfx950) ------------------------------------------------------
// v_permlane32_swap: lanes 32..63 of `a` trade places with lanes 0..31 of `b`.
// (Inline asm: the clang builtin of ROCm 7.2 returns the updated first register in BOTH result
//  elements - tools/probe/lanes.hip.  The s_nop covers the two wait states between a VALU write of an
//  operand and the swap reading it, which hipcc does not insert inside asm.)
__device__ __forceinline__ void swap32(float& a, float& b) {
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
}
// v_permlane16_swap: the odd 16-lane rows of `a` trade places with the even rows of `b`.
__device__ __forceinline__ void swap16(float& a, float& b) {
    asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
}
// N v_permlane16_swap of independent register pairs (a[i], b[i]) back to back behind ONE no-op: the two wait states are owed
// between a VALU write of an operand and the swap that reads it, and every operand of the group was written before the group
// starts (a swap must still never read an operand written less than two wait states earlier - inside the string nobody inserts them)
template <int N>
__device__ __forceinline__ void swap16_group(float (&a)[N], float (&b)[N]) {
#define K2B_SW(i, j) "\n\tv_permlane16_swap_b32 %" #i ", %" #j
    if constexpr (N == 5)
        asm volatile("s_nop 1" K2B_SW(0, 1) K2B_SW(2, 3) K2B_SW(4, 5) K2B_SW(6, 7) K2B_SW(8, 9)
                     : "+v"(a[0]), "+v"(b[0]), "+v"(a[1]), "+v"(b[1]), "+v"(a[2]), "+v"(b[2]), "+v"(a[3]), "+v"(b[3]), "+v"(a[4]), "+v"(b[4]));
    else if constexpr (N == 8)
        asm volatile("s_nop 1" K2B_SW(0, 1) K2B_SW(2, 3) K2B_SW(4, 5) K2B_SW(6, 7) K2B_SW(8, 9) K2B_SW(10, 11) K2B_SW(12, 13) K2B_SW(14, 15)
                     : "+v"(a[0]), "+v"(b[0]), "+v"(a[1]), "+v"(b[1]), "+v"(a[2]), "+v"(b[2]), "+v"(a[3]), "+v"(b[3]), "+v"(a[4]), "+v"(b[4]),
                       "+v"(a[5]), "+v"(b[5]), "+v"(a[6]), "+v"(b[6]), "+v"(a[7]), "+v"(b[7]));
    else static_assert(N < 0, "no swap group of this size");
#undef K2B_SW
}
template <int CTRL>
__device__ __forceinline__ float dpp(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
__device__ __forceinline__ float lane_xor1(float v) { return dpp<0xB1>(v); }    // quad_perm [1,0,3,2]
__device__ __forceinline__ float lane_xor2(float v) { return dpp<0x4E>(v); }    // quad_perm [2,3,0,1]
__device__ __forceinline__ float lane_xor8(float v) { return dpp<0x128>(v); }   // row_ror:8
__device__ __forceinline__ float lane_xor4(float v) {                           // row_shr:4 into banks 1,3 ; row_shl:4 into banks 0,2
    const int x = __builtin_bit_cast(int, v);
    const int t = __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xa, true);
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(t, x, 0x104, 0xf, 0x5, true));
}
// sum of v over the lane and its partner lane ^ 32 / ^ 16 (every lane gets the pair sum)
__device__ __forceinline__ float pair_sum32(float v) { float a = v, b = v; swap32(a, b); return a + b; }
__device__ __forceinline__ float pair_sum16(float v) { float a = v, b = v; swap16(a, b); return a + b; }

// v_min_f32 as asm: fminf() costs a canonicalising v_max_f32 per operand on top; NaNs lose against numbers either way
__device__ __forceinline__ float vmin(float a, float b) {
    float r;
    asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// minimum over the lane's group of eight {l ^ 1, l ^ 2, l ^ 4}: quad_perm twice, then the half-row mirror (the s_nop covers the
// two wait states between a VALU write and a DPP read of the same register, which hipcc does not insert inside asm)
__device__ __forceinline__ float group8_min(float v) {
    float r;
    asm("s_nop 1\n\tv_min_f32_dpp %0, %1, %1 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\tv_min_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\tv_min_f32_dpp %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf"
        : "=&v"(r) : "v"(v));
    return r;
}

__device__ __forceinline__ float wave_sum_fast(float v) {
    v = pair_sum32(v);
    v = pair_sum16(v);
    v += lane_xor8(v);
    v += lane_xor4(v);
    v += lane_xor2(v);
    v += lane_xor1(v);
    return v;
}

// 16 per-lane values -> lane l ends with the wave-wide sum of v[(l>>2)&15].
__device__ __forceinline__ float butterfly16_sum(const float (&v)[16], int lane) {
    float w8[8], w4[4], w2[2];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        float a = v[i], b = v[8 + i];
        swap32(a, b);
        w8[i] = a + b;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float a = w8[i], b = w8[4 + i];
        swap16(a, b);
        w4[i] = a + b;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const float s0 = w4[i] + lane_xor8(w4[i]), s1 = w4[2 + i] + lane_xor8(w4[2 + i]);
        w2[i] = (lane & 8) ? s1 : s0;
    }
    const float t0 = w2[0] + lane_xor4(w2[0]), t1 = w2[1] + lane_xor4(w2[1]);
    float r = (lane & 4) ? t1 : t0;
    r += lane_xor2(r);
    r += lane_xor1(r);
    return r;
}

// 4 per-lane values -> every lane of the 16-lane row r ends with the wave-wide sum of v[r]
__device__ __forceinline__ float butterfly4_sum(const float (&v)[4]) {
    float w[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        float a = v[i], b = v[2 + i];
        swap32(a, b);
        w[i] = a + b;                // lanes < 32: v[i] over the lane pair; lanes >= 32: v[2 + i]
    }
    float a = w[0], b = w[1];
    swap16(a, b);
    float r = a + b;                 // even rows: w[0]; odd rows: w[1]
    r += lane_xor8(r);
    r += lane_xor4(r);
    r += lane_xor2(r);
    r += lane_xor1(r);
    return r;
}

// ---- butterfly reduction sized by its value count -------------------------------------------------
// N per-lane values (N even, 10..16) -> one sum per lane over the lane's 32-lane half.  Four halving levels, each pairing
// register i with register i + ceil(n / 2) of the n registers left (an odd one out rides alone), so a value count below 16 costs
// no swap, move or add on a constant zero:
//   v_permlane16_swap (lane bit 4), row_ror:8 (bit 3), row_shl/shr:4 (bit 2), quad_perm xor 2 (bit 1), then + lane ^ 1
// Every sum adds its lanes in the order 16, 8, 4, 2, 1 of the partner distance, own + partner (a commutative add), whatever N is:
// the value of a sum does not depend on the register it rides in.  butterfly_half_index() names the value a lane ends with.
// The two DPP levels in the middle are bank-masked v_add_f32_dpp pairs - lanes with the level's bit clear add the first register,
// lanes with it set the second, into one destination, without a select.  (Inline asm: the compiler has no masked form with two
// sources; the leading s_nop covers the two wait states between a VALU write and a DPP read of the same register, which hipcc
// does not insert inside asm.  Behind the statement it does: its own DPP reads of the results come out padded.)
#define K2B_F8P(r, x, y) "v_add_f32_dpp " r ", " x ", " x " row_ror:8 row_mask:0xf bank_mask:0x3\n\tv_add_f32_dpp " r ", " y ", " y " row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
#define K2B_F8S(r, x) "v_add_f32_dpp " r ", " x ", " x " row_ror:8 row_mask:0xf bank_mask:0xf\n\t"
#define K2B_F4P(r, x, y) "v_add_f32_dpp " r ", " x ", " x " row_shl:4 row_mask:0xf bank_mask:0x5\n\tv_add_f32_dpp " r ", " y ", " y " row_shr:4 row_mask:0xf bank_mask:0xa\n\t"
#define K2B_F4S(r, x) "v_add_f32_dpp " r ", " x ", " x " row_shl:4 row_mask:0xf bank_mask:0x5\n\t"
// lane bit 3: o[i] = w[i] + w[i](lane ^ 8) where the bit is clear, w[H + i] + w[H + i](lane ^ 8) where it is set (H = ceil(N / 2))
template <int N>
__device__ __forceinline__ void butterfly_fold8(const float (&w)[N], float (&o)[(N + 1) / 2]) {
    if constexpr (N == 8)
        asm("s_nop 1\n\t" K2B_F8P("%0", "%4", "%8") K2B_F8P("%1", "%5", "%9") K2B_F8P("%2", "%6", "%10") K2B_F8P("%3", "%7", "%11")
            : "=&v"(o[0]), "=&v"(o[1]), "=&v"(o[2]), "=&v"(o[3])
            : "v"(w[0]), "v"(w[1]), "v"(w[2]), "v"(w[3]), "v"(w[4]), "v"(w[5]), "v"(w[6]), "v"(w[7]));
    else if constexpr (N == 5)
        asm("s_nop 1\n\t" K2B_F8P("%0", "%3", "%6") K2B_F8P("%1", "%4", "%7") K2B_F8S("%2", "%5")
            : "=&v"(o[0]), "=&v"(o[1]), "=&v"(o[2]) : "v"(w[0]), "v"(w[1]), "v"(w[2]), "v"(w[3]), "v"(w[4]));
    else static_assert(N < 0, "no xor-8 level of this size");
}
// lane bit 2, the same with lane ^ 4 (an odd register out is summed in the lanes with the bit clear only: the others hold no value)
template <int N>
__device__ __forceinline__ void butterfly_fold4(const float (&w)[N], float (&o)[(N + 1) / 2]) {
    if constexpr (N == 4)
        asm("s_nop 1\n\t" K2B_F4P("%0", "%2", "%4") K2B_F4P("%1", "%3", "%5") : "=&v"(o[0]), "=&v"(o[1]) : "v"(w[0]), "v"(w[1]), "v"(w[2]), "v"(w[3]));
    else if constexpr (N == 3)
        asm("s_nop 1\n\t" K2B_F4P("%0", "%2", "%4") K2B_F4S("%1", "%3") : "=&v"(o[0]), "=&v"(o[1]) : "v"(w[0]), "v"(w[1]), "v"(w[2]));
    else static_assert(N < 0, "no xor-4 level of this size");
}
#undef K2B_F8P
#undef K2B_F8S
#undef K2B_F4P
#undef K2B_F4S
template <int N>
__device__ __forceinline__ float butterfly_half_sum(const float (&v)[N], int lane) {
    static_assert(N % 2 == 0 && N >= 10 && N <= 16, "four halving levels, no odd register out at the swap level");
    constexpr int N1 = N / 2, N2 = (N1 + 1) / 2, N3 = (N2 + 1) / 2;
    static_assert(N3 == 2, "four halving levels");
    // swap level: w1[i] = v[i] over the row pair in the even 16-lane rows, v[N1 + i] in the odd ones; one no-op for the group
    float a[N1], b[N1], w1[N1], w2[N2], w3[N3];
#pragma unroll
    for (int i = 0; i < N1; ++i) { a[i] = v[i]; b[i] = v[N1 + i]; }
    swap16_group(a, b);
#pragma unroll
    for (int i = 0; i < N1; ++i) w1[i] = a[i] + b[i];
    butterfly_fold8(w1, w2);
    butterfly_fold4(w2, w3);
    const float u0 = w3[0] + lane_xor2(w3[0]), u1 = w3[1] + lane_xor2(w3[1]);
    float r = (lane & 2) ? u1 : u0;
    r += lane_xor1(r);
    return r;
}
// which of the N values lane `lane` ends with in butterfly_half_sum<N> (-1: none).  N = 16: bits 4..1 of the lane.  It follows
// the pairing rule of the levels above: bit set at a level = the second register of the pair, i + ceil(n / 2); a lane whose
// path leaves the registers that exist (the empty side of an odd one out) ends with no value - there the folds write nothing
// defined, and the caller must not store.
template <int N>
__host__ __device__ constexpr int butterfly_half_index(int lane) {
    constexpr int n[5] = {N, (N + 1) / 2, ((N + 1) / 2 + 1) / 2, (((N + 1) / 2 + 1) / 2 + 1) / 2, 1};
    int idx = 0;
    bool ok = true;
    for (int lvl = 3; lvl >= 0; --lvl) {
        const int bit = (lane >> (4 - lvl)) & 1;
        idx += bit * n[lvl + 1];
        ok = ok && idx < n[lvl];
    }
    return ok ? idx : -1;
}
// every value 0..N-1 has exactly one even lane in each 32-lane half, and no lane names a value that does not exist
template <int N>
constexpr bool butterfly_half_index_covers() {
    int seen[16] = {};
    for (int lane = 0; lane < 64; lane += 2) {
        const int k = butterfly_half_index<N>(lane);
        if (k >= N || k != butterfly_half_index<N>(lane + 1)) return false;
        if (k >= 0) ++seen[k];
    }
    for (int k = 0; k < N; ++k)
        if (seen[k] != 2) return false;
    return true;
}
static_assert(butterfly_half_index_covers<10>() && butterfly_half_index_covers<16>(), "lane <-> value map of butterfly_half_sum");
static_assert(butterfly_half_index<16>(0x1e) == 15 && butterfly_half_index<16>(0x12) == 9, "N = 16: bits 4..1 of the lane");
static_assert(butterfly_half_index<10>(0x10) == 5 && butterfly_half_index<10>(0x08) == 3 && butterfly_half_index<10>(0x04) == 2 &&
              butterfly_half_index<10>(0x02) == 1 && butterfly_half_index<10>(0x0c) == -1, "N = 10: b1 + 2 b2 + 3 b3 + 5 b4");

// NS independent half-wave scans (half_wave_inclusive_scan) side by side, step by step: no DPP move reads a register written by
// the instruction before it, and the row_bcast:15 step needs no zeroed destination per scan.  Its move writes rows 1 and 3 and
// keeps the old value in rows 0 and 2, which has to be zero: the first scan starts from a literal, every later one from the pair
// the scan before it moved - zero in rows 0 and 2 by induction, and dead once its own add has read it.  (zlo, zhi) is that pair:
// zero on entry of the first group, handed on from group to group.  Per scan the adds are those of half_wave_inclusive_scan in the
// same order.  Three scans side by side already keep every DPP move two instructions behind the add that wrote its source.
template <int NS>
__device__ __forceinline__ void half_wave_inclusive_scans(const float (&v)[NS], double (&s)[NS], int& zlo, int& zhi) {
#pragma unroll
    for (int i = 0; i < NS; ++i) s[i] = (double)v[i];
#define K2B_DPP_STEP(ctrl)                                                                              \
    _Pragma("unroll") for (int i = 0; i < NS; ++i) {                                                    \
        const long long bits = __builtin_bit_cast(long long, s[i]);                                     \
        const int lo = __builtin_amdgcn_update_dpp(0, (int)(bits & 0xffffffffll), ctrl, 0xf, 0xf, true); \
        const int hi = __builtin_amdgcn_update_dpp(0, (int)(bits >> 32), ctrl, 0xf, 0xf, true);         \
        s[i] += __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned int)lo);                   \
    }
    K2B_DPP_STEP(0x111)   // row_shr:1
    K2B_DPP_STEP(0x112)   // row_shr:2
    K2B_DPP_STEP(0x114)   // row_shr:4
    K2B_DPP_STEP(0x118)   // row_shr:8
#undef K2B_DPP_STEP
#pragma unroll
    for (int i = 0; i < NS; ++i) {   // row_bcast:15 -> rows 1, 3 (lanes 16..31 and 48..63)
        const long long bits = __builtin_bit_cast(long long, s[i]);
        zlo = __builtin_amdgcn_update_dpp(zlo, (int)(bits & 0xffffffffll), 0x142, 0xa, 0xf, true);
        zhi = __builtin_amdgcn_update_dpp(zhi, (int)(bits >> 32), 0x142, 0xa, 0xf, true);
        s[i] += __builtin_bit_cast(double, ((long long)zhi << 32) | (unsigned int)zlo);
    }
}

// inclusive prefix sum over all 64 lanes, in double: the two half-wave scans, then the lower half's total (lane 31) added to the
// upper half with one more DPP step (row_bcast:31 into rows 2, 3)
__device__ __forceinline__ double wave_inclusive_scan(float v, int lane) {
    (void)lane;
    double s = half_wave_inclusive_scan(v);
    const long long bits = __builtin_bit_cast(long long, s);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(bits & 0xffffffffll), 0x143, 0xc, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(bits >> 32), 0x143, 0xc, 0xf, true);
    s += __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned int)lo);
    return s;
}

}  // namespace k2b
