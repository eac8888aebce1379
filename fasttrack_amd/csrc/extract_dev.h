// Device side of the ORB extractor: what more than one of kernels_pyramid.hip, kernels_fast.hip and kernels_orient_desc.hip
// uses - the division by a small wave-uniform divisor and the base of a pyramid level.  A helper that only one of those files
// uses lives in that file.  Everything here is internal to the including file (an anonymous namespace; the 512-byte table
// c_divMagic gets one copy per file that reads it): nothing links across files.
// Device only: nothing includes this header except those three .hip files and kernels_stereo.hip, the fourth reader of the
// pyramid layout (level_ptr for k_stereo_match's SAD windows; it reads no c_divMagic and gets no copy of it).  No MFMA anywhere
// in them: the path is integer / bitwise.
#pragma once
#include <algorithm>

#include "ft_internal.h"
#include "wave_ops.h"

namespace {

// i / d for small operands with a precomputed magic = floor(2^32 / d) + 1 (exact for i < 2^32 / d);
// d == 1 makes the magic wrap to 0, so it is special-cased.
__host__ __device__ constexpr unsigned div_magic_of(unsigned d) { return d > 1 ? 0xffffffffu / d + 1u : 0u; }
// The divisors that occur per wave (dwords per footprint row, columns behind the 32-column halves of a cell) are
// small: their magics come from a constant table (one scalar load) instead of a ~25-instruction integer division.
struct FtDivMagicTab {
    unsigned m[128];
};
constexpr FtDivMagicTab ft_make_div_magic_tab() {
    FtDivMagicTab t{};
    for (unsigned d = 0; d < 128; d++) t.m[d] = d ? div_magic_of(d) : 0u;
    return t;
}
__constant__ FtDivMagicTab c_divMagic = ft_make_div_magic_tab();
__device__ __forceinline__ unsigned div_magic_small(unsigned d) { return d < 128u ? c_divMagic.m[d] : div_magic_of(d); }
__device__ __forceinline__ int div_by(int i, unsigned magic) { return magic ? (int)__umulhi((unsigned)i, magic) : i; }

__device__ __forceinline__ const uint8_t *level_ptr(const FtGeom &g, int level, int slot, const uint8_t *const *l0,
                                                    int l0pitch, const uint8_t *pyr, int &pitch) {
    if (level == 0) {
        pitch = l0pitch;
        return l0[slot];
    }
    pitch = g.lv[level].pitch;
    return pyr + (size_t)slot * g.pyrPerSlot + g.lv[level].off;
}

}  // namespace
