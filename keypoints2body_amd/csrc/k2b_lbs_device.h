// k2b_lbs_device.h - what the LBS vertex kernels (k2b_lbs.hip, k2b_lbs_stream.hip) share as device code: the MFMA operand
// types, the two synchronisation primitives, and the walk of a persistent workgroup over its tiles.
#pragma once
#include <hip/hip_runtime.h>

namespace k2b {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float floatx4 __attribute__((ext_vector_type(4)));
struct __attribute__((packed, aligned(4))) float3v { float x, y, z; };

__device__ __forceinline__ void wg_barrier() { asm volatile("s_barrier" ::: "memory"); }
template <int N> __device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// The tiles (frame group, vertex group) of one persistent workgroup.  XCD label x = block % 8 owns a contiguous range of
// (frame chunk, vertex group) items, a chunk = CHUNK frame groups (8: 1024 frames, whose per-frame operands, 2.3 MB for SMPL,
// stay in the XCD's L2 while the vertex groups stream past); inside the range the frame group runs fastest, and the XCD's nx
// workgroups take every nx-th tile.  The object holds what is fixed for the launch; a cursor is the caller's three integers
// (t: index into the XCD's tile sequence, item-major with CHUNK frame slots per item), so a kernel may keep several.
template <int CHUNK>
struct Walk {
    int vgroups, fgroups, item_lo, item_hi, nx;
    // returns the cursor index in front of the workgroup's first tile: next() moves it there
    __device__ int init(int vgroups_, int fgroups_, int block, int nblocks) {
        vgroups = vgroups_; fgroups = fgroups_;
        const int items = ((fgroups + CHUNK - 1) / CHUNK) * vgroups, x = block & 7;
        item_lo = (int)((long long)items * x / 8); item_hi = (int)((long long)items * (x + 1) / 8);
        nx = nblocks >> 3;
        return (block >> 3) - nx;
    }
    // advances t to the next tile and sets (fg, vg); calls end() instead when the workgroup's sequence is exhausted
    template <class End>
    __device__ void next(int& t, int& fg, int& vg, End&& end) const {
        for (;;) {
            t += nx;
            const int item = item_lo + t / CHUNK;
            if (item >= item_hi) { end(); return; }
            const int c = item / vgroups;
            fg = c * CHUNK + t % CHUNK; vg = item - c * vgroups;
            if (fg < fgroups) return;
        }
    }
    // the same with a sentinel: fg = -1 when exhausted
    __device__ void next(int& t, int& fg, int& vg) const { next(t, fg, vg, [&] { fg = -1; vg = 0; }); }
};

}  // namespace k2b
