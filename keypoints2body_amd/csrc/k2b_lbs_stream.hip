// k2b_lbs_stream.hip — vertex skinning for SMPL (k2b_lbs_stream_kernel: 17-24 joints, 7 pose k-steps) and SMPL-H / SMPL-X
// (k2b_lbs_stream_x_kernel: 49-56 joints, 16 pose k-steps; k2b_lbs_stream_xw_kernel: the same with 25-32 shape coefficients,
// 17 pose k-steps) on gfx950: ONE kernel body, stream_body<S>, and the descriptions S (Smpl, SmplX, SmplXWide) that hold what
// the kernels do not share - the counted-wait tables among it.  A fourth description, SmplF8 (k2b_lbs_stream_f8_kernel), is Smpl
// with the correction products of the pose k-steps 0..5 on the block-scaled e4m3 MFMA (k2b_lbs_fp8.h): the default of the 23- and
// 24-joint models, the f16 form being their K2B_LBS_POSE_F16 twin.
//
// Same arithmetic as the tile kernel of k2b_lbs.hip (two GEMMs over frames x vertices on v_mfma_f32_16x16x32_f16, operands
// as f16 hi/lo pairs, v = T [v_posed; 1] + t; reference seam: the final forward of world_space.py:258-278, smplx's
// SMPL.forward), and the same 128 frames x 128 vertices per persistent workgroup.  What differs is how the operands travel:
//
//   * a wave owns 16 vertices x 128 frames (eight 16 x 16 accumulator tiles per coordinate).  Its share of the big
//     B operand Pd (posedirs | shapedirs | template, 48 of the 64 KiB a 32-deep k-step needs) is private to it, so it goes
//     global -> REGISTERS with plain 16-byte loads, two k-steps ahead, and never touches LDS or a barrier: k-step ks lives in
//     Pd buffer ks % 3, so the next tile's k-steps 0 and 1 end the tile in the buffers KS % 3 and (KS + 1) % 3 (1 and 2 for 7
//     and 16 k-steps, 2 and 0 for 17) and are handed down to the buffers 0 and 1;
//   * the frame-side operand X (16 KiB per k-step) is fetched by LDS-DMA.  SMPL: X of the WHOLE tile is resident in 7 slots, the
//     pose phase has NO barrier at all, waves drift apart and the stores of one wave overlap the matrix work of another; X of
//     the next tile arrives during the transform phase, one k-step per 16-frame unit.  SMPL-X: 16 k-steps do not fit, so X
//     walks through a FOUR-slot ring of one k-step each, three k-steps ahead, and the pose phase has one barrier per k-step
//     (the barrier at the top of k-step ks publishes X(ks + 1), which every wave has waited for itself, and frees the slot of
//     k-step ks - 1 for X(ks + 3)); the first four k-steps of the next tile arrive during the transform units 0..3;
//   * the transform operand A sits in a two-slot ring of 16-frame units: one workgroup barrier per unit, 8 per tile (tile
//     kernel: 11, and 64 KiB of fills behind each);
//   * per entry of the 3 x 4 transform the A fragments are read ONCE and meet W fragments that stay in registers for the phase:
//       SMPL    A: [hi | t], [lo | 0]     W: [hi | 1], [hi | tag], [lo | 0]           two LDS reads for three MFMAs
//       SMPL-X  A: H0 = hi groups 0-3, H1 = hi 4-6 | PAD (translation terms), L0 = lo 0-3, L1 = lo 4-6 | ZERO
//               W: Wh0, Wh1 | ONES, Wl0, Wl1 | 0, Wh1 | tag                            four LDS reads for six MFMAs
//               T = H0.Wh0 + H1.[Wh1|ONES] + H0.Wl0 + H1.[Wl1|0] + L0.Wh0 + L1.[Wh1|tag]
// Every vector-memory wait is a counted s_waitcnt with a compile-time count (the issue order of a wave is fixed; loads, LDS-DMA
// fills and stores retire in order), so the loads the wave does not need yet stay in flight.  The counts of a kernel stand in
// its description, under the table that justifies them, and nowhere else.
//
// LDS: X slots x 16 KiB + 2 A units = 7 x 16 + 2 x 24 = 4 x 16 + 2 x 48 = 160 KiB.  SMPL: 9 (J - 1) + NB + 2 <= 224 (up to 15
// shape coefficients); SMPL-X: 9 x 54 + NB + 2 <= 512 features (up to 24 shape coefficients) in 16 k-steps, <= 544 (25-32; a
// 56-joint model from 16 coefficients on, 529 at most) in 17; everything else runs the tile kernel.
#include <hip/hip_fp16.h>

#include <type_traits>
#include <utility>

#include "k2b_internal.h"
#include "k2b_lbs_device.h"

namespace k2b {

namespace {

// Diagnostics live in tools/lbs_diag.h (tools/build_lbs_variants.sh); the product build leaves the hooks empty.  Inside the
// body they see its names (S, a, lane, wave); a stamp index is the description's numbering, a negative one is no stamp.
#ifdef K2B_LBS_DIAG_HEADER
#include K2B_LBS_DIAG_HEADER
#else
#define K2B_SDIAG_BEGIN ((void)0)
#define K2B_SDIAG_STAMP(i) ((void)(i))
#define K2B_SDIAG_TILE ((void)0)
#define K2B_SDIAG_END ((void)0)
#define K2B_SDIAG_STORE_ROW(u, i) ((u) * 16 + (i))   // frame row, inside the tile, of a full tile's store
#endif
#ifndef K2B_SX_SKIP
#define K2B_SX_SKIP 0          // timing-only builds (tools/build_lbs_variants.sh name:"-DK2B_SX_SKIP=n"), a bit mask:
#endif                         // 1 no stores, 2 no fills behind the prologue, 4 no Pd loads in the loop, 8 no barriers in the loop,
                               // 16 no LDS reads, 32 Pd of vertex group 0 for every tile (always L2-resident)
                               // (results are wrong on purpose; they answer "what does this part cost")
#ifndef K2B_STREAM_DIAG
#define K2B_STREAM_DIAG 0      // diagnostic level of the SMPL kernel and of the SMPL-X kernel (tools/lbs_diag.h)
#endif
#ifndef K2B_STREAMX_DIAG
#define K2B_STREAMX_DIAG 0
#endif
#ifndef K2B_STREAMX_CHUNK
#define K2B_STREAMX_CHUNK 8
#endif

// 16-byte load global -> register through a scalar base and a per-lane byte offset; the result is only valid behind a
// counted wait that names the register (K2B_PD_READY / w_ready below)
template <int OFF>
__device__ __forceinline__ void gload16(half8& dst, unsigned lane_off, const void* sbase) {
    asm volatile("global_load_dwordx4 %0, %1, %2 offset:%3" : "=v"(dst) : "v"(lane_off), "s"(sbase), "n"(OFF) : "memory");
}
// N consecutive KiB from sbase - BIAS on
template <int BIAS, int... I>
__device__ __forceinline__ void gload_frags(half8 (&dst)[sizeof...(I)], unsigned lane_off, const void* sbase, std::integer_sequence<int, I...>) {
    (gload16<I * 1024 - BIAS>(dst[I], lane_off, sbase), ...);
}

// 16-byte LDS read whose completion the code waits for itself (counted lgkmcnt waits that name the registers): the
// compiler's own waits are lgkmcnt(0) in front of the first use, which stalls a wave on every fragment it has just requested
template <int OFF>
__device__ __forceinline__ void lread16(half8& dst, unsigned addr) {
    if constexpr (K2B_SX_SKIP & 16) asm volatile("" : "=v"(dst) : "v"(addr));
    else asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF) : "memory");
}
// the N fragments of one operand row: consecutive KiB from OFF on
template <int OFF, int... I>
__device__ __forceinline__ void lread_frags(half8 (&dst)[sizeof...(I)], unsigned addr, std::integer_sequence<int, I...>) {
    (lread16<OFF + I * 1024>(dst[I], addr), ...);
}
template <int OFF, int N>
__device__ __forceinline__ void lread_frags(half8 (&dst)[N], unsigned addr) { lread_frags<OFF>(dst, addr, std::make_integer_sequence<int, N>{}); }
// at most N LDS reads in flight: the fragments b have landed.  (One overload per fragment count, here and for w_ready: the
// wait has to NAME every register it guards as an asm operand, and an operand list cannot be made from a pack or a loop.)
template <int N> __device__ __forceinline__ void lds_ready(half8 (&b)[2]) {
    asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(b[0]), "+v"(b[1]) : "n"(N) : "memory");
}
template <int N> __device__ __forceinline__ void lds_ready(half8 (&b)[4]) {
    asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]) : "n"(N) : "memory");
}
// (SmplF8: one fragment, or three - hi, the e4m3 strip, the previous k-step's e4m3 strip)
template <int N> __device__ __forceinline__ void lds_ready(half8& b) { asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(b) : "n"(N) : "memory"); }
template <int N> __device__ __forceinline__ void lds_ready(half8& b0, half8& b1, half8& b2) {
    asm volatile("s_waitcnt lgkmcnt(%3)" : "+v"(b0), "+v"(b1), "+v"(b2) : "n"(N) : "memory");
}
// the 32 bytes a lane gives v_mfma_scale_f32_16x16x128_f8f6f4: the e4m3 strips of the even and of the odd k-step of a pair
typedef int int8v __attribute__((ext_vector_type(8)));
typedef _Float16 half16 __attribute__((ext_vector_type(16)));
__device__ __forceinline__ int8v f8_pair(half8 even, half8 odd) {
    return __builtin_bit_cast(int8v, __builtin_shufflevector(even, odd, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15));
}
// at most N vector-memory operations in flight: the W fragments have landed
template <int N> __device__ __forceinline__ void w_ready(half8 (&w)[3]) {
    asm volatile("s_waitcnt vmcnt(%3)" : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]) : "n"(N) : "memory");
}
template <int N> __device__ __forceinline__ void w_ready(half8 (&w)[5]) {
    asm volatile("s_waitcnt vmcnt(%5)" : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3]), "+v"(w[4]) : "n"(N) : "memory");
}
#define K2B_PD_READY(N, b)                                                                                                  \
    asm volatile("s_waitcnt vmcnt(%6)" : "+v"(b[0][0]), "+v"(b[0][1]), "+v"(b[1][0]), "+v"(b[1][1]), "+v"(b[2][0]), "+v"(b[2][1]) : "n"(N) : "memory")
// 12-byte store through a scalar row base and a per-lane 32-bit byte offset (the compiler's own code adds 64-bit vector addresses
// per store; nobody waits for a store except the end of the kernel)
typedef float float3r __attribute__((ext_vector_type(3)));
__device__ __forceinline__ void gstore12(unsigned lane_off, float3r d, const void* sbase) {
    asm volatile("global_store_dwordx3 %0, %1, %2" ::"v"(lane_off), "v"(d), "s"(sbase) : "memory");
}

// ---- the three descriptions -------------------------------------------------------------------------------------------------------
// Vector-memory operations of a wave in issue order (they retire in order; N of a wait = operations younger than the awaited one):
//   pose phase, top of k-step ks:  [wait] [barrier]  X(ks + 3) (ring only)   W (last k-step)   Pd(ks + 2)
//   transform, top of unit u:      [wait] [barrier]  A(u + 1)   X(next tile, u) (the first units)   ...   stores (full tile)
// Pd(kPoseSteps), Pd(kPoseSteps + 1) are the next tile's k-steps 0 and 1: they ride through the transform phase.
constexpr int kPdLoads = 6;    // Pd of a k-step: [coordinate 3][hi | lo]
constexpr int kXFills = 2;     // a wave's share of one k-step of X: a hi and a lo piece
constexpr int kStores = 4;     // a unit's outputs of a lane: frames 4 g .. 4 g + 3
constexpr int kNoWait = 63;    // the counter's ceiling: ties the registers to the point, waits for nothing - in particular NOT for
                               // the transform phase's last stores, whose acknowledgements take thousands of cycles when every CU
                               // writes at once

struct Smpl {
    static constexpr int kPoseSteps = kStreamKSteps;
    static constexpr int kF8Steps = 0;                      // k-steps whose correction products are e4m3 (SmplF8)
    static constexpr int kXSlots = 7;                       // 16 KiB slots of X in LDS: the whole tile is resident
    static constexpr bool pose_barrier(int) { return false; }
    static constexpr bool pose_x_fill(int) { return false; }
    static constexpr int kXUnits = 7;                       // the transform units u < kXUnits fill X(next tile, u)
    static constexpr int kAFrags = 2, kWFrags = 3, kTagFrag = 1;
    static constexpr int kProducts = 3;                     // T = A0.W0 + A1.W1 + A0.W2
    static constexpr int prod_a(int p) { return p == 1 ? 1 : 0; }
    static constexpr int prod_w(int p) { return p; }
    static constexpr int kChunk = 8;                        // frame groups per L2 chunk of the tile walk (as the tile kernel)
    // | point          | awaited                                          | younger in issue order                                  |
    // | k-steps 0, 1   | Pd(0), Pd(1): loaded at the previous tile's      | covered by the previous tile's unit-1 wait (first tile: |
    // |                | k-steps 5, 6, in front of A(unit 1)              | by the prologue), stored or not: nothing to wait for    |
    // | k-step 2..6    | Pd(ks), loaded at k-step ks - 2                  | Pd(ks + 1)                                              |
    // | unit 0         | W (loaded at k-step 6) and A(unit 0)             | the next tile's Pd(1)                                   |
    // | unit 1..6      | A(u), filled at unit u - 1                       | X fills + stores of unit u - 1 (stores: full tiles only)|
    // | unit 7         | A(7) and EVERY X fill of the next tile (they     | the stores of unit 6 (full tiles only)                  |
    // |                | must be visible before the next pose phase)      |                                                         |
    // The stores of a unit are part of a count ONLY where every one of them is issued: in the predicated path a wave whose lanes
    // are all beyond the mesh or the batch skips the instruction (s_cbranch_execz), so a wave of a partial tile counts the fills
    // alone.  Fewer younger operations than N would leave the awaited fills in flight; more (the rare joint copies) only make
    // the wait stricter.
    static constexpr int pose_wait(int ks) { return ks < 2 ? kNoWait : kPdLoads; }
    static __device__ __forceinline__ void unit_wait(int u, bool full, half8 (&wf)[kWFrags]) {
        if (u == 0) w_ready<kPdLoads>(wf);
        else if (u == 7) { if (full) wait_vmcnt<kStores>(); else wait_vmcnt<0>(); }
        else { if (full) wait_vmcnt<kXFills + kStores>(); else wait_vmcnt<kXFills>(); }
    }
    // stamps of the diagnostics: top of k-step ks = ks, then per unit u kStampUnits + 3 u + (0 before the counted wait, 1 behind
    // the barrier, 2 MFMAs issued, before the stores)
    static constexpr int kStampPoseEnd = 7, kStampUnits = 8, kStampTileEnd = -1;
    [[maybe_unused]] static constexpr int kStampsPerWave = 32, kStampTile = 2;   // stamp slots of a wave; the workgroup's tile that is stamped
    [[maybe_unused]] static constexpr int kDiagLevel = K2B_STREAM_DIAG;
};

struct SmplX {
    static constexpr int kPoseSteps = kStreamXKSteps;
    static constexpr int kF8Steps = 0;
    static constexpr int kXSlots = 4;                       // a ring: k-step ks in slot ks % 4, filled three k-steps ahead
    static constexpr bool pose_barrier(int ks) { return ks >= 1 && ks <= 14; }   // publishes X(ks + 1), frees the slot of X(ks - 1)
    static constexpr bool pose_x_fill(int ks) { return ks >= 1 && ks <= 12; }    // X(ks + 3) into that slot
    static constexpr int kXUnits = 4;
    static constexpr int kAFrags = 4, kWFrags = 5, kTagFrag = 4;
    static constexpr int kProducts = 6;                     // T = A0.W0 + A1.W1 + A0.W2 + A1.W3 + A2.W0 + A3.W4
    static constexpr int prod_a(int p) { return p < 4 ? (p & 1) : p - 2; }
    static constexpr int prod_w(int p) { return p < 4 ? p : p == 4 ? 0 : 4; }
    static constexpr int kChunk = K2B_STREAMX_CHUNK;
    // | point          | awaited                                          | younger in issue order                                  |
    // | k-steps 0, 1   | Pd(0), Pd(1)                                     | covered by the waits of the previous tile's units       |
    // | k-step 2..13   | Pd(ks) (and X(ks + 1), filled in front of it)    | X(ks + 2), Pd(ks + 1)                                   |
    // | k-steps 14, 15 | Pd(ks)                                           | Pd(ks + 1)                                              |
    // | unit 0         | W (loaded at k-step 15) and A(unit 0)            | the next tile's Pd(1)                                   |
    // | unit 1..4      | A(u), filled at unit u - 1                       | X fills + stores of unit u - 1 (stores: full tiles only)|
    // | unit 5..7      | A(u) - and with unit 5 every X fill              | the stores of unit u - 1 (full tiles only)              |
    // (partial tiles: as for SMPL)
    static constexpr int pose_wait(int ks) { return ks < 2 ? kNoWait : ks <= 13 ? kXFills + kPdLoads : kPdLoads; }
    static __device__ __forceinline__ void unit_wait(int u, bool full, half8 (&wf)[kWFrags]) {
        if (u == 0) w_ready<kPdLoads>(wf);
        else if (u <= 4) { if (full) wait_vmcnt<kXFills + kStores>(); else wait_vmcnt<kXFills>(); }
        else { if (full) wait_vmcnt<kStores>(); else wait_vmcnt<0>(); }
    }
    static constexpr int kStampPoseEnd = -1, kStampUnits = 16, kStampTileEnd = 40;
    [[maybe_unused]] static constexpr int kStampsPerWave = 64, kStampTile = 1;
    [[maybe_unused]] static constexpr int kDiagLevel = K2B_STREAMX_DIAG;
};

// SMPL with the correction products of the k-steps 0..5 on the block-scaled e4m3 instruction (k2b_lbs_fp8.h; the route's default
// for 23 and 24 joints, LbsRouteRecord::pose_fp8).  Everything is Smpl's but the product list of the pose phase:
//   k-step 0, 2, 4:  X_hi . Pd_hi (f16, 3 MFMAs per 16-frame tile); the k-step's e4m3 Pd strip stays in its buffer
//   k-step 1, 3, 5:  X_hi . Pd_hi, then ONE v_mfma_scale_f32_16x16x128_f8f6f4 per coordinate over the e4m3 strips of the k-steps
//                    ks - 1 and ks: X_hi8 . Pd_lo8 + X_lo8 . Pd_hi8 of both, into the same accumulator (units Pd x 256: the
//                    scales are X's constants kF8XHiExp / kF8XLoExp and the image's pd8_lo_exp / pd8_hi_exp)
//   k-step 6:        the three f16 products, as Smpl
// The e4m3 strips take the place of the f16 lo strips in X (LDS slots, fills) and in Pd (6 loads per k-step), 16 bytes per lane
// each, so the vector-memory operations of a wave and their order are Smpl's and so are both wait tables.  What moves is LDS
// traffic inside a k-step: an even k-step reads one fragment per tile, an odd one three (its own two and the e4m3 strip of the
// k-step before), and the Pd strip of an even k-step is copied out of its buffer - the buffer of k-step ks - 1 is the one k-step
// ks loads Pd(ks + 2) into - before those loads are issued.  MFMA cycles per tile and SIMD: 2 x (7 x 24 x 16 + 3 x 24 x 32 +
// 2 x 24 x 16 + 288 x 16) = 20.7 k against 25.3 k.
struct SmplF8 : Smpl {
    static constexpr int kF8Steps = kF8PoseSteps;
    static_assert(kF8Steps % 2 == 0 && kF8Steps < kPoseSteps, "pairs of k-steps, and a last k-step in the f16 form");
};

// SMPL-X with 25-32 shape coefficients: 9 x 54 + NB + 2 = 513..520 features, one 32-deep k-step more.  Ring, fragments, products
// and unit waits are SmplX's; the ring runs one k-step longer, and 17 % 3 == 2 hands the Pd buffers over from 2 and 0 (the body).
struct SmplXWide {
    static constexpr int kPoseSteps = kStreamXWKSteps;
    static constexpr int kF8Steps = 0;
    static constexpr int kXSlots = 4;                       // X(16) takes slot 0; the next tile's X(0) follows it behind the barrier of unit 0
    static constexpr bool pose_barrier(int ks) { return ks >= 1 && ks <= 15; }   // publishes X(ks + 1), frees the slot of X(ks - 1)
    static constexpr bool pose_x_fill(int ks) { return ks >= 1 && ks <= 13; }    // X(ks + 3) into that slot; X(16) is the last
    static constexpr int kXUnits = SmplX::kXUnits;
    static constexpr int kAFrags = SmplX::kAFrags, kWFrags = SmplX::kWFrags, kTagFrag = SmplX::kTagFrag;
    static constexpr int kProducts = SmplX::kProducts;
    static constexpr int prod_a(int p) { return SmplX::prod_a(p); }
    static constexpr int prod_w(int p) { return SmplX::prod_w(p); }
    static constexpr int kChunk = SmplX::kChunk;
    // | point          | awaited                                          | younger in issue order                                  |
    // | k-steps 0, 1   | Pd(0), Pd(1)                                     | covered by the waits of the previous tile's units       |
    // | k-step 2..14   | Pd(ks) (and X(ks + 1), filled in front of it)    | X(ks + 2), Pd(ks + 1)   (issued at k-step ks - 1 <= 13) |
    // | k-steps 15, 16 | Pd(ks) (15: and X(16), filled at k-step 13)      | Pd(ks + 1)              (no fill at k-steps 14, 15)     |
    // | unit 0         | W (loaded at k-step 16) and A(unit 0)            | the next tile's Pd(1)                                   |
    // | unit 1..7      | as SmplX (the same fills and stores in the same order): its unit_wait, partial-tile counts included      |
    static constexpr int pose_wait(int ks) { return ks < 2 ? kNoWait : ks <= 14 ? kXFills + kPdLoads : kPdLoads; }
    static __device__ __forceinline__ void unit_wait(int u, bool full, half8 (&wf)[kWFrags]) { SmplX::unit_wait(u, full, wf); }
    // pose stamps 0..16
    static constexpr int kStampPoseEnd = -1, kStampUnits = 17, kStampTileEnd = 41;
    [[maybe_unused]] static constexpr int kStampsPerWave = 64, kStampTile = 1;
    [[maybe_unused]] static constexpr int kDiagLevel = 0;   // (no diagnostics build of this kernel)
};

template <class S> constexpr int stream_x_bytes() { return S::kXSlots * 16 * 1024; }
template <class S> constexpr int stream_unit_bytes() { return 12 * S::kAFrags * 1024; }   // A operand of one 16-frame unit: 12 entries
template <class S> constexpr size_t stream_lds_bytes() { return (size_t)stream_x_bytes<S>() + 2 * stream_unit_bytes<S>(); }

template <int I> using ic = std::integral_constant<int, I>;
// f(ic<0>), f(ic<1>), ... f(ic<N - 1>): a loop whose index is a constant expression inside f
template <class F, int... I> __device__ __forceinline__ void static_for(F&& f, std::integer_sequence<int, I...>) { (f(ic<I>{}), ...); }
template <int N, class F> __device__ __forceinline__ void static_for(F&& f) { static_for(f, std::make_integer_sequence<int, N>{}); }

// ---- the body -----------------------------------------------------------------------------------------------------------------------
// (The arguments arrive BY VALUE and the transform units are an unrolled loop, not a lambda per unit: with a reference, or with
//  the unit as a compile-time index, this compiler places the scalar code differently, and the MFMA / LDS-read interleave of the
//  pose phase and the register count move with it.  Compare the assembly after any change of form.)
template <class S>
__device__ __forceinline__ void stream_body(const StreamArgs a) {
    constexpr int KS = S::kPoseSteps, AF = S::kAFrags, WF = S::kWFrags;
    constexpr int kXBytes = stream_x_bytes<S>(), kUnitBytes = stream_unit_bytes<S>();
    constexpr int AP = 12 * AF / 8;                                        // A pieces a wave moves per unit
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];   // [kXSlots][16 KiB] X | [2][kUnitBytes] A units
    unsigned char* const aslots = lds + kXBytes;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int row = lane & 15, g = lane >> 4;                 // MFMA operand lane: row of the 16-row tile, k-group
    const int f32tiles = a.f32_tiles, f16tiles = 2 * f32tiles, nv16 = a.nv16;
    const unsigned lane16 = (unsigned)lane * 16u;

    Walk<S::kChunk> walk;
    int wt = walk.init(nv16 >> 3, (f32tiles + 3) >> 2, blockIdx.x, a.num_wgs), cfg, cvg;   // cursor, frame group and vertex group of the current tile
    walk.next(wt, cfg, cvg);
    if (cfg < 0) return;
    K2B_SDIAG_BEGIN;

    // ---- issue helpers (all addresses wave-uniform + lane x 16 B) ----------------------------------------------------------
    // X of k-step ks into slot ks % kXSlots: 16 pieces [k-half 2][32-frame tile 4][hi | lo]; wave w moves (k-half w >> 2,
    // frame tile w & 3), hi and lo
    auto issue_x = [&](int fg, int ks) {
        const int kh = wave >> 2, ft = wave & 3;
        int ftc = fg * 4 + ft;
        ftc = ftc < f32tiles ? ftc : f32tiles - 1;
        const size_t o = ((size_t)(2 * ks + kh) * f32tiles + ftc) * 512 + lane * 8;
        unsigned char* dst = lds + (ks % S::kXSlots) * 16384 + (kh * 8 + ft * 2) * 1024;
        __builtin_amdgcn_global_load_lds(a.xh + o, dst, 16, 0, 0);
        __builtin_amdgcn_global_load_lds(a.xl + o, dst + 1024, 16, 0, 0);
    };
    // A of one 16-frame unit: 12 AF contiguous pieces [entry 12][fragment AF]; wave w moves pieces AP w .. AP w + AP - 1
    auto issue_a = [&](int f16, int slot) {
        f16 = f16 < f16tiles ? f16 : f16tiles - 1;
        const k2b_half* src = a.a2 + ((size_t)f16 * 12 * AF + AP * wave) * 512 + lane * 8;
        unsigned char* dst = aslots + slot * kUnitBytes + AP * wave * 1024;
#pragma unroll
        for (int i = 0; i < AP; ++i) __builtin_amdgcn_global_load_lds(src + i * 512, dst + i * 1024, 16, 0, 0);
    };
    // Pd of this wave's 16 vertices for k-step ks: 6 consecutive KiB [coordinate 3][hi | lo]
    auto load_pd = [&](half8 (&buf)[3][2], int vg, int ks) {
        const unsigned char* base = reinterpret_cast<const unsigned char*>(a.pd + ((size_t)ks * nv16 + ((K2B_SX_SKIP & 32) ? 0 : vg) * 8 + wave) * 6 * 512) + 3072;
        gload16<-3072>(buf[0][0], lane16, base); gload16<-2048>(buf[0][1], lane16, base);
        gload16<-1024>(buf[1][0], lane16, base); gload16<0>(buf[1][1], lane16, base);
        gload16<1024>(buf[2][0], lane16, base);  gload16<2048>(buf[2][1], lane16, base);
    };

    const int lx = (g >> 1) * 8192 + (g & 1) * 512 + row * 16;      // lane part of an X fragment address inside a slot
    const unsigned lds0 = (unsigned)(uintptr_t)lds;                  // LDS byte address of the X region
    const unsigned lxa = lds0 + lx, lxb = lxa + 65536;               // (the 16-bit offset field reaches four slots)
    const int la = g * 256 + row * 16;                               // lane part of an A fragment address inside a piece
    const float inv_scale = 1.0f / kPdScale;
    // SmplF8: the E8M0 scale bytes this lane supplies - lane group g scales block g of the K = 128 instruction, the blocks 0, 2 being
    // X_hi8 . Pd_lo8 and 1, 3 X_lo8 . Pd_hi8 (k2b_lbs_fp8.h)
    [[maybe_unused]] int sa = 0, sb = 0;
    if constexpr (S::kF8Steps > 0) {
        sa = e8m0((g & 1) ? kF8XLoExp : kF8XHiExp);
        sb = e8m0((g & 1) ? a.pd8_hi_exp : a.pd8_lo_exp);
        asm volatile("" : "+v"(sa), "+v"(sb));
    }

    // ---- prologue: everything the first tile needs ------------------------------------------------------------------------
    half8 pb[3][3][2];                          // Pd buffers: k-step ks lives in buffer ks % 3
    half8 wf[WF];                               // W fragments of this wave's 16 vertices
#pragma unroll
    for (int ks = 0; ks < S::kXSlots; ++ks) issue_x(cfg, ks);
    issue_a(cfg * 8, 0);
    load_pd(pb[0], cvg, 0);
    load_pd(pb[1], cvg, 1);
    K2B_PD_READY(0, pb[0]);                                         // everything of the prologue has landed (once per launch)
    K2B_PD_READY(0, pb[1]);
    wg_barrier();

    while (cfg >= 0) {
        int nt = wt, nxf, nxv;
        walk.next(nt, nxf, nxv);
        const int nfg = nxf >= 0 ? nxf : cfg, nvg = nxf >= 0 ? nxv : cvg;   // (no next tile: the same addresses again, so that the
                                                                             //  counted waits keep their counts)
        floatx4 vp[8][3];         // [16-frame tile][coordinate]; the first k-step starts every accumulator from zero

        // ---- pose phase: v_posed * kPdScale = X . Pd -----------------------------------------------------------------------------
        // X fragments (hi | lo of one 16-frame tile), two buffers: tile q + 1 of the phase's 8 KS is requested before the nine MFMAs
        // of tile q, and a counted wait leaves those two reads in flight.  (Ring: the first fragment of k-step ks + 1 is read at the
        // end of k-step ks - the barrier at the top of ks published it.)
        half8 xq[2][2];
        auto xread = [&](half8 (&dst)[2], auto ksc, auto fc) {
            constexpr int slot = decltype(ksc)::value % S::kXSlots, f = decltype(fc)::value;
            constexpr int off = (slot & 3) * 16384 + (f >> 1) * 2048 + (f & 1) * 256;
            lread_frags<off>(dst, slot < 4 ? lxa : lxb);
        };
        auto kstep = [&](auto ksc, const half8 (&pd)[3][2]) {
            constexpr int ks = decltype(ksc)::value;
            auto tile = [&](auto fc) {
                constexpr int f = decltype(fc)::value;
                half8 (&cur)[2] = xq[f & 1];
                if constexpr (f < 7) xread(xq[(f + 1) & 1], ksc, ic<f + 1>{});
                else if constexpr (ks < KS - 1) xread(xq[0], ic<ks + 1>{}, ic<0>{});
                if constexpr (f < 7 || ks < KS - 1) lds_ready<2>(cur); else lds_ready<0>(cur);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    if constexpr (ks == 0) vp[f][c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(cur[0], pd[c][0], floatx4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                    else vp[f][c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(cur[0], pd[c][0], vp[f][c], 0, 0, 0);
                    vp[f][c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(cur[0], pd[c][1], vp[f][c], 0, 0, 0);
                    vp[f][c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(cur[1], pd[c][0], vp[f][c], 0, 0, 0);
                }
            };
            static_for<8>(tile);
        };
        // SmplF8, k-steps 0..5: the fragment with the e4m3 strip of k-step ks - 1 (xo, beside xq), the three pair operands of Pd (b8)
        // and the scale bytes of this lane's group (sa, sb).  An even k-step reads and multiplies X_hi alone; an odd one reads its
        // own two fragments and the strip of the k-step before, and adds the pair's corrections with one K = 128 MFMA per coordinate.
        [[maybe_unused]] half8 xo[2];
        [[maybe_unused]] int8v b8[3];
        auto xread8 = [&](auto ksc, auto fc, half8 (&dst)[2], half8& before) {
            constexpr int ks = decltype(ksc)::value, f = decltype(fc)::value;
            constexpr int tile_off = (f >> 1) * 2048 + (f & 1) * 256;
            lread16<(ks & 3) * 16384 + tile_off>(dst[0], ks < 4 ? lxa : lxb);
            if constexpr (ks & 1) {
                lread16<(ks & 3) * 16384 + tile_off + 1024>(dst[1], ks < 4 ? lxa : lxb);
                lread16<((ks - 1) & 3) * 16384 + tile_off + 1024>(before, ks - 1 < 4 ? lxa : lxb);
            }
        };
        auto kstep8 = [&](auto ksc, const half8 (&pd)[3][2]) {
            constexpr int ks = decltype(ksc)::value;
            constexpr bool odd = ks & 1;
            auto tile = [&](auto fc) {
                constexpr int f = decltype(fc)::value;
                half8 (&cur)[2] = xq[f & 1];
                half8& before = xo[f & 1];
                // the next tile's fragments: one (even k-step), three (odd), or the two of the last k-step's f16 form
                if constexpr (f < 7) xread8(ksc, ic<f + 1>{}, xq[(f + 1) & 1], xo[(f + 1) & 1]);
                else if constexpr (ks + 1 < S::kF8Steps) xread8(ic<ks + 1>{}, ic<0>{}, xq[0], xo[0]);
                else xread(xq[0], ic<ks + 1>{}, ic<0>{});
                constexpr int next = f < 7 ? (odd ? 3 : 1) : ks + 1 < S::kF8Steps ? (odd ? 1 : 3) : 2;
                if constexpr (odd) lds_ready<next>(cur[0], cur[1], before); else lds_ready<next>(cur[0]);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    if constexpr (ks == 0) vp[f][c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(cur[0], pd[c][0], floatx4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                    else vp[f][c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(cur[0], pd[c][0], vp[f][c], 0, 0, 0);
                }
                if constexpr (odd) {
                    const int8v a8 = f8_pair(before, cur[1]);
#pragma unroll
                    for (int c = 0; c < 3; ++c) vp[f][c] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a8, b8[c], vp[f][c], 0, 0, 0, sa, 0, sb);
                }
            };
            static_for<8>(tile);
        };
        // top of k-step ks: wait, barrier, fills and loads in the issue order of the description, then the 72 MFMAs
        auto step = [&](auto ksc) {
            constexpr int ks = decltype(ksc)::value;
            half8 (&cur)[3][2] = pb[ks % 3], (&ahead)[3][2] = pb[(ks + 2) % 3];
            K2B_SDIAG_STAMP(ks);
            K2B_PD_READY(S::pose_wait(ks), cur);
            if constexpr (ks < S::kF8Steps && (ks & 1)) {   // the pair's Pd strips, before the loads below take the buffer of k-step ks - 1
#pragma unroll
                for (int c = 0; c < 3; ++c) b8[c] = f8_pair(ahead[c][1], cur[c][1]);
            }
            if constexpr (S::pose_barrier(ks)) if (!(K2B_SX_SKIP & 8)) wg_barrier();
            if constexpr (S::pose_x_fill(ks) && !(K2B_SX_SKIP & 2)) issue_x(cfg, ks + S::kXSlots - 1);
            if constexpr (ks == KS - 1) {              // W fragments of this tile's vertices (needed behind the pose phase: their registers are free until here)
                constexpr int bias = WF > 4 ? WF / 2 * 1024 : 0;                          // (13-bit signed offsets)
                const unsigned char* wbase = reinterpret_cast<const unsigned char*>(a.w + ((size_t)cvg * 8 + wave) * WF * 512) + bias;
                gload_frags<bias>(wf, lane16, wbase, std::make_integer_sequence<int, WF>{});
            }
            if constexpr (!(K2B_SX_SKIP & 4)) { if constexpr (ks + 2 < KS) load_pd(ahead, cvg, ks + 2); else load_pd(ahead, nvg, ks + 2 - KS); }
            if constexpr (ks < S::kF8Steps) kstep8(ksc, cur); else kstep(ksc, cur);
        };
        // the next tile's k-steps 0 and 1 are loaded at the k-steps KS - 2 and KS - 1 into the buffers KS % 3 and (KS + 1) % 3; a
        // remainder 0 would put k-step 0 into buffer 0 itself and k-step 1 into 1: no hand-over, and nothing here is built for it
        static_assert(KS % 3 == 1 || KS % 3 == 2, "the next tile's k-steps 0 and 1 must end the tile in buffers 1, 2 or 2, 0");
        constexpr int kHand0 = KS % 3, kHand1 = (KS + 1) % 3;
        if constexpr (S::kF8Steps > 0) xread8(ic<0>{}, ic<0>{}, xq[0], xo[0]); else xread(xq[0], ic<0>{}, ic<0>{});
        static_for<KS>(step);
        K2B_SDIAG_STAMP(S::kStampPoseEnd);
#pragma unroll
        for (int f = 0; f < 8; ++f)
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int i = 0; i < 4; ++i) { vp[f][c][i] *= inv_scale; asm volatile("" : "+v"(vp[f][c][i])); }

        // ---- transform phase: one 16-frame unit at a time ---------------------------------------------------------------------
        // this wave's vertex, and the output joint it may be (tag = 1 + index, first half of the padding group of fragment kTagFrag)
        const int v = (cvg * 8 + wave) * 16 + row;
        const bool okv = v < a.num_out;
        int jrow = 0;
        bool has_joint = false;
        const size_t row_bytes = (size_t)a.out_stride * 12;                     // one frame of the output
        // a store address = wave-uniform row base (tile's first frame + u 16 + i, scalar arithmetic) + this lane's 32-bit offset
        // (its vertex, and the frames 4 g .. of its k-group): global_store with a scalar base, no 64-bit vector arithmetic per store
        unsigned char* const tbase = reinterpret_cast<unsigned char*>(a.out) + (size_t)(cfg * 128) * row_bytes;
        const unsigned voff = (unsigned)(((size_t)a.out_row0 + v) * 12 + (size_t)(4 * g) * row_bytes);
        const bool tile_full = cfg * 128 + 127 < a.num_frames && (cvg * 8 + wave) * 16 + 15 < a.num_out;   // wave-uniform: a scalar branch
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            // A of this unit has landed (each wave waits for its own pieces, the barrier collects them)
            K2B_SDIAG_STAMP(S::kStampUnits + 3 * u);
            S::unit_wait(u, tile_full, wf);
            if (!(K2B_SX_SKIP & 8)) wg_barrier();
            K2B_SDIAG_STAMP(S::kStampUnits + 3 * u + 1);
            if (u == 0 && a.joints_out) {              // (W fragments are long there: they are older than everything waited for)
                const float tg = (float)wf[S::kTagFrag][0];   // lanes g == 3 hold the tag group of their row
                jrow = (int)__shfl(tg, 48 + row, 64);
                has_joint = __builtin_amdgcn_ballot_w64(jrow != 0) != 0;
            }
            // behind the barrier the other A slot and (from unit 0 on) the X region are free: next unit's A, next tile's X k-step u
            if (!(K2B_SX_SKIP & 2)) {
                if (u < 7) issue_a(cfg * 8 + u + 1, (u + 1) & 1); else issue_a(nfg * 8, 0);
                if (u < S::kXUnits) issue_x(nfg, u);
            }
            floatx4 out[3] = {floatx4{0.f, 0.f, 0.f, 0.f}, floatx4{0.f, 0.f, 0.f, 0.f}, floatx4{0.f, 0.f, 0.f, 0.f}};
            // entries in d-major order (n -> d = n / 3, r = n % 3, entry 4 r + d); fragments of entry n + 1 requested before the
            // MFMAs of entry n, entry n - 1 folded into the outputs while the matrix pipe works on entry n
            half8 af[2][AF];
            floatx4 t[2];
            const unsigned sa = lds0 + kXBytes + (u & 1) * kUnitBytes + la;
            lread_frags<0>(af[0], sa);
            auto entry = [&](auto nc) {
                constexpr int n = decltype(nc)::value;
                if constexpr (n + 1 < 12) {
                    constexpr int e1 = 4 * ((n + 1) % 3) + (n + 1) / 3;
                    lread_frags<e1 * AF * 1024>(af[(n + 1) & 1], sa);
                }
                if constexpr (n + 1 < 12) lds_ready<AF>(af[n & 1]); else if constexpr (n < 12) lds_ready<0>(af[n & 1]);
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (n < 12) {
                    floatx4 acc = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int p = 0; p < S::kProducts; ++p) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[n & 1][S::prod_a(p)], wf[S::prod_w(p)], acc, 0, 0, 0);
                    t[n & 1] = acc;
                }
                __builtin_amdgcn_sched_barrier(0);     // the fold of entry n - 1 behind all MFMAs of entry n: no hazard no-ops on t
                if constexpr (n > 0) {
                    constexpr int d = (n - 1) / 3, r = (n - 1) % 3;
                    // element by element: written on the 4-vectors this becomes v_pk_fma_f32 / v_pk_add_f32, which issue at well under
                    // half the rate of the scalar forms beside MFMAs (MI355X_MICROARCH.md) - and the transform phase is VALU-issue-bound
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        if constexpr (d < 3) out[r][i] = __builtin_fmaf(t[(n - 1) & 1][i], vp[u][d][i], out[r][i]);
                        else out[r][i] += t[(n - 1) & 1][i];
                        asm volatile("" : "+v"(out[r][i]));   // fold NOW (left to itself the compiler keeps all twelve T tiles, 48 registers, for
                    }                                         // the end) and do not re-pack
                }
                __builtin_amdgcn_sched_barrier(0);
            };
            static_for<13>(entry);
            K2B_SDIAG_STAMP(S::kStampUnits + 3 * u + 2);
            // one 12-byte store per (frame, vertex): lane (vertex row, g) holds frames 4 g .. 4 g + 3 of the unit
            const int fbase = (cfg * 8 + u) * 16 + 4 * g;
            if (K2B_SX_SKIP & 1) {
                asm volatile("" ::"v"(out[0]), "v"(out[1]), "v"(out[2]));
            } else if (tile_full) {                    // every (frame, vertex) of the tile exists: lane base + a wave-uniform row offset
#pragma unroll
                for (int i = 0; i < 4; ++i) gstore12(voff, float3r{out[0][i], out[1][i], out[2][i]}, tbase + (size_t)K2B_SDIAG_STORE_ROW(u, i) * row_bytes);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int f = fbase + i;
                    if (okv && f < a.num_frames) gstore12(voff, float3r{out[0][i], out[1][i], out[2][i]}, tbase + (size_t)(u * 16 + i) * row_bytes);
                }
            }
            if (has_joint) {                           // rare (SMPL: 21 of 6890 vertices): the vertex again, into the joints array
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int f = fbase + i;
                    if (jrow != 0 && okv && f < a.num_frames) {
                        float3v x;
                        x.x = out[0][i]; x.y = out[1][i]; x.z = out[2][i];
                        *reinterpret_cast<float3v*>(a.joints_out + ((size_t)f * a.joints_stride + a.joints_row0 + jrow - 1) * 3) = x;
                    }
                }
            }
        }
        // buffers kHand0 and kHand1 hold the next tile's k-steps 0 and 1 (landed long ago: the waits of the units covered them); the
        // empty statement pins the copies behind this point - the compiler takes an asm load's result for ready at once
        {
            half8 (&h0)[3][2] = pb[kHand0], (&h1)[3][2] = pb[kHand1];
            asm volatile("" : "+v"(h0[0][0]), "+v"(h0[0][1]), "+v"(h0[1][0]), "+v"(h0[1][1]), "+v"(h0[2][0]), "+v"(h0[2][1]),
                              "+v"(h1[0][0]), "+v"(h1[0][1]), "+v"(h1[1][0]), "+v"(h1[1][1]), "+v"(h1[2][0]), "+v"(h1[2][1]));
        }
        // down to the buffers 0 and 1, a source never overwritten before it is read: 1, 2 -> 0, 1 in that order; 2, 0 -> 0, 1 moves
        // buffer 0 up first
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if constexpr (kHand0 == 1) { pb[0][c][h] = pb[1][c][h]; pb[1][c][h] = pb[2][c][h]; }
                else { pb[1][c][h] = pb[0][c][h]; pb[0][c][h] = pb[2][c][h]; }
            }
        K2B_SDIAG_STAMP(S::kStampTileEnd);
        wt = nt; cfg = nxf; cvg = nxv;
        K2B_SDIAG_TILE;
    }
    wait_vmcnt<0>();
    K2B_SDIAG_END;
}

// one launcher: the persistent grid, the kernel's dynamic LDS (granted once per device), the launch
template <class S>
hipError_t launch_stream(void (*kernel)(const StreamArgs), const StreamArgs& a_in, int num_cus, hipStream_t stream) {
    if (a_in.num_frames <= 0 || a_in.num_out <= 0) return hipSuccess;
    StreamArgs a = a_in;
    if ((a.nv16 & 7) || a.f32_tiles <= 0) return hipErrorInvalidValue;
    a.num_wgs = lbs_stream_grid(num_cus, a.nv16, a.f32_tiles);
    static std::atomic<unsigned long long> lds_set{0};
    const hipError_t e = ensure_dynamic_lds(kernel, lds_set, stream_lds_bytes<S>());
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(a.num_wgs), dim3(512), stream_lds_bytes<S>(), stream, a);
    return hipGetLastError();
}

}  // namespace

__global__ __launch_bounds__(512) void k2b_lbs_stream_kernel(const StreamArgs a) { stream_body<Smpl>(a); }
__global__ __launch_bounds__(512) void k2b_lbs_stream_f8_kernel(const StreamArgs a) { stream_body<SmplF8>(a); }
__global__ __launch_bounds__(512) void k2b_lbs_stream_x_kernel(const StreamArgs a) { stream_body<SmplX>(a); }
__global__ __launch_bounds__(512) void k2b_lbs_stream_xw_kernel(const StreamArgs a) { stream_body<SmplXWide>(a); }

hipError_t launch_skin_stream(LbsRoute route, const StreamArgs& a, int num_cus, hipStream_t stream) {
    switch (route) {
        case LbsRoute::stream:
            return a.pose_fp8 ? launch_stream<SmplF8>(k2b_lbs_stream_f8_kernel, a, num_cus, stream) : launch_stream<Smpl>(k2b_lbs_stream_kernel, a, num_cus, stream);
        case LbsRoute::stream_x: return launch_stream<SmplX>(k2b_lbs_stream_x_kernel, a, num_cus, stream);
        case LbsRoute::stream_xw: return launch_stream<SmplXWide>(k2b_lbs_stream_xw_kernel, a, num_cus, stream);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace k2b
