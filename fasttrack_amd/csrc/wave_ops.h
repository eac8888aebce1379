// Device helpers shared by the gfx950 kernels (wave64): explicit global loads, 24-bit multiplies, DPP reductions, the Hamming
// distance of two descriptors.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// Image rows (and other read-only inputs reached through a pointer that was itself loaded from memory or selected
// between two bases) are read through explicit global-address-space loads: such a pointer is generic to the compiler,
// which then emits flat_load - and a flat load counts on the LDS counter as well, so every LDS wait would also wait
// for the image loads in flight.
template <class T>
__device__ __forceinline__ T gload(const void *p) {
    return *(const __attribute__((address_space(1))) T *)p;
}

template <class T>
__device__ __forceinline__ void gstore(void *p, T v) {
    *(__attribute__((address_space(1))) T *)p = v;
}

// The wave index of a thread, as a scalar: it is uniform by construction, which the compiler cannot see (it derives
// from threadIdx); with it everything a one-item-per-wave kernel looks up for its item becomes SALU work and scalar
// loads instead of 64 identical VALU lanes.
__device__ __forceinline__ int wave_index() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// LDS hand-off between the lanes of ONE wave: the LDS queue of a wave is served in order, so only the
// compiler has to be kept from moving accesses across this point.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// Sum / minimum over the 64 lanes, returned wave-uniform: four DPP steps (lane pairs, quads, half rows, rows of 16;
// all four are permutations inside a row, so no lane reads an invalid source) and one v_readlane per row - instead of
// six shuffles through the LDS crossbar with their address arithmetic.
__device__ __forceinline__ int wave_sum_i32(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true);   // quad_perm [1,0,3,2]
    v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, true);   // quad_perm [2,3,0,1]
    v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, true);  // row_half_mirror
    v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, true);  // row_mirror
    return __builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16) + __builtin_amdgcn_readlane(v, 32) +
           __builtin_amdgcn_readlane(v, 48);
}
__device__ __forceinline__ unsigned wave_min_u32(unsigned v) {
    v = min(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true));
    v = min(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, true));
    v = min(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, true));
    v = min(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, true));
    return min(min((unsigned)__builtin_amdgcn_readlane((int)v, 0), (unsigned)__builtin_amdgcn_readlane((int)v, 16)),
               min((unsigned)__builtin_amdgcn_readlane((int)v, 32), (unsigned)__builtin_amdgcn_readlane((int)v, 48)));
}

// the two smallest of the 2 x 64 keys of a wave whose lanes each hold their own two smallest (x0 <= x1), wave-uniform in x0 <= x1
__device__ __forceinline__ void wave_two_min(unsigned &x0, unsigned &x1) {
    const unsigned m0 = wave_min_u32(x0);
    const unsigned m1 = wave_min_u32(x0 == m0 ? x1 : x0);
    x0 = m0;
    x1 = m1;
}
// lane j's 64-bit value (j wave-uniform) as two v_readlane, wave-uniform
__device__ __forceinline__ unsigned long long wave_readlane_u64(unsigned long long v, int j) {
    return ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(v >> 32), j) << 32) |
           (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, j);
}

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#define FT_MIN64_STEP(ctrl)                                                                                   \
    {                                                                                                         \
        const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)v, ctrl, 0xF, 0xF, true); \
        const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(v >> 32), ctrl, 0xF, 0xF, true);   \
        const unsigned long long w = ((unsigned long long)hi << 32) | lo;                                     \
        v = w < v ? w : v;                                                                                    \
    }
    FT_MIN64_STEP(0xB1) FT_MIN64_STEP(0x4E) FT_MIN64_STEP(0x141) FT_MIN64_STEP(0x140)
#undef FT_MIN64_STEP
    unsigned long long best = ~0ull;
#pragma unroll
    for (int row = 0; row < 64; row += 16) {
        const unsigned long long w = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(v >> 32), row) << 32) |
                                     (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, row);
        best = w < best ? w : best;
    }
    return best;
}

// minimum over the 16 lanes of a ROW, returned in every lane of the row (the four DPP steps above stay inside a row)
__device__ __forceinline__ unsigned long long row_min_u64(unsigned long long v) {
#define FT_MIN64_STEP(ctrl)                                                                                   \
    {                                                                                                         \
        const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)v, ctrl, 0xF, 0xF, true); \
        const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(v >> 32), ctrl, 0xF, 0xF, true);   \
        const unsigned long long w = ((unsigned long long)hi << 32) | lo;                                     \
        v = w < v ? w : v;                                                                                    \
    }
    FT_MIN64_STEP(0xB1) FT_MIN64_STEP(0x4E) FT_MIN64_STEP(0x141) FT_MIN64_STEP(0x140)
#undef FT_MIN64_STEP
    return v;
}

// the same for 32-bit keys
__device__ __forceinline__ unsigned row_min_u32(unsigned v) {
    v = min(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true));   // quad_perm [1,0,3,2]
    v = min(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, true));   // quad_perm [2,3,0,1]
    v = min(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, true));  // row_half_mirror
    v = min(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, true));  // row_mirror
    return v;
}

// sum over the row, in every lane of it
__device__ __forceinline__ int row_sum_i32(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true);   // quad_perm [1,0,3,2]
    v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, true);   // quad_perm [2,3,0,1]
    v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, true);  // row_half_mirror
    v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, true);  // row_mirror
    return v;
}

// maximum over the row of 16 lanes, in every lane of it
__device__ __forceinline__ int row_max_i32(int v) {
    v = max(v, __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xF, 0xF, false));
    v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xF, 0xF, false));
    v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x141, 0xF, 0xF, false));
    v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x140, 0xF, 0xF, false));
    return v;
}

// row i of the descriptors `desc` (32 bytes each) as 4 x uint64
__device__ __forceinline__ void load_desc256(const uint8_t *desc, int i, unsigned long long q[4]) {
    const unsigned long long *d = (const unsigned long long *)(desc + (size_t)i * 32);
    q[0] = d[0]; q[1] = d[1]; q[2] = d[2]; q[3] = d[3];
}

// ORBmatcher::DescriptorDistance (reference src/ORBmatcher.cc:2256-2272) of two 256-bit descriptors as 4 x uint64
__device__ __forceinline__ int hamming256(const unsigned long long a[4], const unsigned long long *b) {
    return __popcll(a[0] ^ b[0]) + __popcll(a[1] ^ b[1]) + __popcll(a[2] ^ b[2]) + __popcll(a[3] ^ b[3]);
}

// Low 32 bits of the product of two operands that fit 24 bits, as ONE full-rate instruction.  (__mul24 is dissolved
// into a plain multiply once the optimiser has proven the operand ranges, and instruction selection then falls back
// to the quarter-rate 32-bit v_mul_lo_u32 whenever it cannot re-derive them.)
__device__ __forceinline__ int vmul24(int a, int b) {
    int r;
    asm("v_mul_i32_i24 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// a * b + c with 24-bit a, b: one full-rate instruction (b wave-uniform)
__device__ __forceinline__ int vmad24(int a, int bUniform, int c) {
    int r;
    asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "s"(bUniform), "v"(c));
    return r;
}
