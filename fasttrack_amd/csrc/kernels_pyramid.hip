// HIP kernels of the ORB extractor's image pyramid for gfx950 (CDNA4, wave64).  All three compute cv::resize INTER_LINEAR 8UC1
// in its fixed point, exact 2x levels as INTER_AREA (reference ORBextractor.cc:1495-1520), bit for bit:
//   k_pyr_down         one level per launch, a wave per 64 x 16 output tile through LDS (batches < 8, unaligned frames)
//   k_pyr_rows<AREA>   one level per launch, a wave per strip of 128 x PR_RB output pixels, no LDS (pyr_rows_strip)
//   k_pyr_cascade      levels 1 .. n - 1 in ONE launch: a workgroup walks a band of an image through the levels with the same strips
// ft_launch_pyramid chooses between them.
#include "extract_dev.h"

namespace {

// ------------------------------------------------------------------------------------------------
// Pyramid: level l from level l-1 (one launch per level; grid.z = image slot)
// ------------------------------------------------------------------------------------------------
// One WAVE per 64 x 8 output tile (no workgroup barrier, like k_fast_cells): the source footprint of the
// tile (rows sy(first)..sy(last)+1, columns sx(first)..sx(last)+1) is staged in LDS with aligned dword
// loads, then every lane produces a 4 x 4 block of outputs from 2x2 taps read from LDS and stores four dwords.
#define PD_TW 64
#define PD_TH 16
#define PD_NLOAD 9  // footprint dwords per lane in flight at once
// A wave's life is a chain of memory round trips, so the chain is kept short: the source footprint of the tile is
// bounded arithmetically (fixed-point scale with a two-pixel margin instead of reading the first and last tap),
// and the taps the outputs need - four in x and four in y per lane - are requested together with the footprint,
// before anything waits.
__global__ __launch_bounds__(64) void k_pyr_down(FtGeom g, int level, const uint8_t *const *l0, int l0pitch,
                                                 uint8_t *pyr, const FtTap *taps, int alignedLoads, int ldsPitch,
                                                 int rowsAlloc, unsigned sxQ16, unsigned syQ16, FtSlotGrid sg, int tilesX,
                                                 unsigned txMagic) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int lane = threadIdx.x;
    // all tiles of an image on one XCD (ft_slot_grid): neighbouring tiles share source lines (footprint margins, 64-B
    // lines), which then come from that XCD's L2 instead of being fetched once per XCD
    int slot, tile;
    if (!ft_slot_block(sg, slot, tile)) return;
    const int tileY = div_by(tile, txMagic), tileX = tile - tileY * tilesX;
    const FtLevelGeom &D = g.lv[level];
    const int dx0 = tileX * PD_TW, dy0 = tileY * PD_TH;
    const int dx1 = min(dx0 + PD_TW, D.w) - 1, dy1 = min(dy0 + PD_TH, D.h) - 1;  // last output col / row
    int spitch;
    const uint8_t *S = level_ptr(g, level - 1, slot, l0, l0pitch, pyr, spitch);
    const int sw = g.lv[level - 1].w, sh = g.lv[level - 1].h;
    int sxa, sxb, sya, syb;  // source footprint (inclusive)
    if (D.area2x) {
        sxa = 2 * dx0; sxb = 2 * dx1 + 1; sya = 2 * dy0; syb = 2 * dy1 + 1;
    } else {
        // first tap of output d is floor((d + 0.5) * scale - 0.5); ((2d + 1) * scaleQ16) >> 17 is within one of it
        sxa = max((int)(((unsigned)(2 * dx0 + 1) * sxQ16) >> 17) - 2, 0);
        sxb = min((int)(((unsigned)(2 * dx1 + 1) * sxQ16) >> 17) + 2, sw - 1);
        sya = max((int)(((unsigned)(2 * dy0 + 1) * syQ16) >> 17) - 2, 0);
        syb = min((int)(((unsigned)(2 * dy1 + 1) * syQ16) >> 17) + 2, sh - 1);
    }
    // compute mapping: lane = (group of 4 output columns, group of 4 output rows): 16 x 4 groups cover the 64 x 16 tile,
    // every lane produces a 4 x 4 block and stores it as four dwords (a row of the tile is 64 B = one store segment)
    const int xg = lane & 15, yg = lane >> 4;
    const int bx = dx0 + 4 * xg, by = dy0 + 4 * yg;
    FtTap xt[4], yt[4];
    if (!D.area2x) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            xt[k] = taps[D.xtab + min(bx + k, dx1)];
            yt[k] = taps[D.ytab + min(by + k, dy1)];
        }
    }
    const int rows = syb - sya + 1;
    int ax = 0;
    if (alignedLoads) {
        ax = sxa & 3;
        const int nd = (sxb - sxa + 1 + ax + 3) >> 2;  // dwords per row; over-read stays inside the aligned row pitch
        const uint8_t *src = S + (size_t)sya * spitch + (sxa - ax);
        // all loads of the footprint are issued before the first LDS store (PD_NLOAD x 64 dwords cover the usual
        // footprint; a larger one takes further rounds).  Element i = lane + 64 j of the (rows x nd) footprint is
        // walked incrementally - 64 elements further is dy rows and dx dwords further, one more row on wrap-around -
        // so a load costs a few full-rate adds instead of a division and 64-bit address arithmetic.
        const int n = nd * rows;
        const int spare = ldsPitch * rowsAlloc;  // one dword behind the tile (see the launcher)
        const unsigned ndMagic = div_magic_small((unsigned)nd);
        const int dy = div_by(64, ndMagic), dx = 64 - dy * nd;
        int x = lane - div_by(lane, ndMagic) * nd;
        unsigned gOff = (unsigned)(div_by(lane, ndMagic) * spitch + 4 * x);
        int lOff = div_by(lane, ndMagic) * ldsPitch + 4 * x;
        const unsigned gStep = (unsigned)(dy * spitch + 4 * dx), gStepW = gStep + (unsigned)(spitch - 4 * nd);
        const int lStep = dy * ldsPitch + 4 * dx, lStepW = lStep + ldsPitch - 4 * nd;
        for (int i0 = 0; i0 < n; i0 += 64 * PD_NLOAD) {
            unsigned v[PD_NLOAD];
            int off[PD_NLOAD];
#pragma unroll
            for (int k = 0; k < PD_NLOAD; k++) {
                // lanes past the footprint re-read its first dword and park it in the spare dword behind the tile:
                // selects instead of exec-mask branches around every load and store
                const bool ok = i0 + 64 * k + lane < n;
                off[k] = ok ? lOff : spare;
                v[k] = gload<unsigned>(src + (ok ? gOff : 0u));
                x += dx;
                const bool wrap = x >= nd;
                x -= wrap ? nd : 0;
                gOff += wrap ? gStepW : gStep;
                lOff += wrap ? lStepW : lStep;
            }
#pragma unroll
            for (int k = 0; k < PD_NLOAD; k++) *(unsigned *)(smem + off[k]) = v[k];
        }
    } else {
        const int cw = sxb - sxa + 1;
        const unsigned cwMagic = div_magic_of((unsigned)cw);
        const uint8_t *src = S + (size_t)sya * spitch + sxa;
        for (int i = lane; i < cw * rows; i += 64) {
            const int y = div_by(i, cwMagic), x = i - y * cw;
            smem[y * ldsPitch + x] = gload<uint8_t>(src + (size_t)y * spitch + x);
        }
    }
    wave_lds_sync();
    const uint8_t *T = smem + ax;  // source pixel (sx, sy) at T[(sy - sya) * ldsPitch + (sx - sxa)]
    if (bx > dx1 || by > dy1) return;
    // uniform level base + 32-bit lane offset (row * pitch + column): scalar-base stores, no 64-bit lane arithmetic
    uint8_t *outLevel = pyr + (size_t)slot * g.pyrPerSlot + D.off;
    // the row pitch of a level is a multiple of 64 B, so the dword store may run past the last column of the level
    // (into the row's padding) but never into the next row
    if (D.area2x) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int dy = by + j;
            if (dy > dy1) break;
            unsigned pk = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int dxk = min(bx + k, dx1);
                const uint8_t *r0 = T + __mul24(2 * dy - sya, ldsPitch) + (2 * dxk - sxa), *r1 = r0 + ldsPitch;
                pk |= (unsigned)((r0[0] + r0[1] + r1[0] + r1[1] + 2) >> 2) << (8 * k);
            }
            gstore<unsigned>(outLevel + (unsigned)vmad24(dy, D.pitch, bx), pk);
        }
        return;
    }
    int cx0[4], cx1[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        cx0[k] = xt[k].s - sxa;
        cx1[k] = min(xt[k].s + 1, sw - 1) - sxa;
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int dy = by + j;
        if (dy > dy1) break;
        const int sy0 = min(max((int)yt[j].s, 0), sh - 1) - sya, sy1 = min(max((int)yt[j].s + 1, 0), sh - 1) - sya;
        const uint8_t *r0 = T + __mul24(sy0, ldsPitch), *r1 = T + __mul24(sy1, ldsPitch);
        unsigned pk = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int h0 = r0[cx0[k]] * xt[k].a0 + r0[cx1[k]] * xt[k].a1;
            const int h1 = r1[cx0[k]] * xt[k].a0 + r1[cx1[k]] * xt[k].a1;
            // weights <= 2^11 and h >> 4 < 2^15: 24-bit multiplies (full rate; the 32-bit v_mul_lo is quarter rate)
            pk |= (unsigned)(((vmul24((int)yt[j].a0, h0 >> 4) >> 16) + (vmul24((int)yt[j].a1, h1 >> 4) >> 16) + 2) >> 2) << (8 * k);
        }
        gstore<unsigned>(outLevel + (unsigned)vmad24(dy, D.pitch, bx), pk);
    }
}

// ------------------------------------------------------------------------------------------------
// Pyramid, row-streaming form (the default): one WAVE per strip of 128 output columns x PR_RB output rows.
// A lane owns two adjacent output columns for the whole strip: their taps (source column, weights) live in registers,
// the eight source bytes that hold both columns' two taps are ONE aligned 8-byte load per source row, and the
// horizontal interpolation of a column is one v_perm (two bytes -> a pair of u16) + one v_dot2_u32_u16.  The wave
// walks the source rows of its strip once, top to bottom: cv::resize needs rows sy and sy + 1 for an output row and
// sy advances by one or two, so the horizontally interpolated row is kept in registers and serves as the lower row of
// one output row and the upper row of the next (1.2 instead of 2 interpolations per output row at scale 1.2).  No LDS,
// no workgroup barrier; row taps are wave-uniform (one lane holds the taps of one output row, v_readlane hands them
// out); the next source row is requested before the current one is used.  Per output pixel ~9 VALU instructions
// instead of ~32 in the tile kernel above, whose arithmetic it repeats bit for bit.
// ------------------------------------------------------------------------------------------------
#define PR_COLS 128
#ifndef PR_RB
#define PR_RB 32
#endif
#ifndef PR_PF
#define PR_PF 4       // source rows in flight ahead of the one being used
#endif
typedef unsigned short ft_us2 __attribute__((ext_vector_type(2)));
typedef unsigned ft_u2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned udot2_u16(unsigned a, unsigned b) {
    return __builtin_amdgcn_udot2(__builtin_bit_cast(ft_us2, a), __builtin_bit_cast(ft_us2, b), 0u, false);
}
// (b * a) >> 16 for a wave-uniform b < 2^11 handed in as b << 16 and a < 2^16: the high half of a 32 x 32-bit product - one
// instruction where a 24-bit multiply and a shift took two
__device__ __forceinline__ unsigned umulhi_su(unsigned bShifted16, unsigned a) {
    unsigned r;
    asm("v_mul_hi_u32 %0, %1, %2" : "=v"(r) : "s"(bShifted16), "v"(a));
    return r;
}
// one strip: columns [tx * PR_COLS, + PR_COLS) x up to PR_RB rows from j0, short of row rowEnd (BAND) or of the level's height,
// of `level` of image `slot`, from the level below at S with row pitch spitch (all wave-uniform)
template <bool AREA, bool BAND>
__device__ __forceinline__ void pyr_rows_strip(const FtGeom &g, int level, int slot, int tx, int j0, int rowEnd, int lane,
                                               const uint8_t *S, int spitch, uint8_t *pyr, const FtTap *taps, int readableEnd) {
    const FtLevelGeom &D = g.lv[level];
    const int sw = g.lv[level - 1].w, sh = g.lv[level - 1].h;
    const int dx = tx * PR_COLS + 2 * lane;  // first of this lane's two output columns
    const int nrows = min(PR_RB, (BAND ? rowEnd : D.h) - j0);
    // row taps: lane r holds the two source rows (clamped to the level, packed sy0 | sy1 << 16) and the two weights
    // (b0 | b1 << 16) of output row j0 + r - unpacked and clamped once here, by the vector unit for all rows at a time;
    // the loop below reads a row's pair with two v_readlane and four scalar instructions
    unsigned rowW0 = 0, rowW1 = 0;
    if constexpr (!AREA) {
        const ft_u2 t = gload<ft_u2>(taps + D.ytab + j0 + min(lane, nrows - 1));
        const int sy = (int)(short)(t.x & 0xffffu);
        rowW0 = (unsigned)min(max(sy, 0), sh - 1) | ((unsigned)min(max(sy + 1, 0), sh - 1) << 16);
        rowW1 = (t.x >> 16) | (t.y << 16);
        // the lane behind the last output row holds a row pair no source row ever matches: the loop below runs out of output
        // rows by reading it, without a clamp and a test per row (nrows <= PR_RB < 64)
        if (lane >= nrows) rowW0 = 0xffffffffu;
    }
    // column taps; columns beyond the level repeat its last column (their stores are masked)
    const int dxa = min(dx, D.w - 1), dxb = min(dx + 1, D.w - 1);
    int sxa, sxb, cxa, cxb;
    unsigned wa, wb;
    if constexpr (AREA) {
        sxa = 2 * dxa; sxb = 2 * dxb; cxa = sxa + 1; cxb = sxb + 1;
        wa = wb = 0x00010001u;  // s0 + s1
    } else {
        const ft_u2 ta = gload<ft_u2>(taps + D.xtab + dxa), tb = gload<ft_u2>(taps + D.xtab + dxb);
        sxa = (int)(short)(ta.x & 0xffffu); sxb = (int)(short)(tb.x & 0xffffu);
        cxa = min(sxa + 1, sw - 1); cxb = min(sxb + 1, sw - 1);
        wa = (ta.x >> 16) | (ta.y << 16);  // a0 | a1 << 16
        wb = (tb.x >> 16) | (tb.y << 16);
    }
    // the 8-byte window [base, base + 8) of a source row that holds all four taps of the lane (the launcher has checked
    // that it does); it never reaches past the readable end of a row
    const int base = min(sxa & ~3, readableEnd - 8);
    const unsigned selA = (unsigned)(sxa - base) | 0x0c00u | ((unsigned)(cxa - base) << 16) | 0x0c000000u;
    const unsigned selB = (unsigned)(sxb - base) | 0x0c00u | ((unsigned)(cxb - base) << 16) | 0x0c000000u;
    auto rowTap = [&](int r, int &sy0, int &sy1, unsigned &b0, unsigned &b1) {
        if constexpr (AREA) {
            sy0 = 2 * (j0 + r); sy1 = r < nrows ? sy0 + 1 : -1; b0 = b1 = 0;
        } else {
            const unsigned w0 = (unsigned)__builtin_amdgcn_readlane((int)rowW0, r), w1 = (unsigned)__builtin_amdgcn_readlane((int)rowW1, r);
            sy0 = (int)(w0 & 0xffffu); sy1 = (int)(w0 >> 16);
            b0 = w1 << 16; b1 = w1 & 0xffff0000u;  // the weights as b << 16 (umulhi_su)
        }
    };
    int jr = 0, sy0, sy1;
    unsigned b0, b1;
    rowTap(0, sy0, sy1, b0, b1);
    int lastSy0, rLast;
    unsigned bx0, bx1;
    rowTap(nrows - 1, lastSy0, rLast, bx0, bx1);
    int r = sy0;
    // Fixed wave-uniform bases + 32-bit offsets (row offset: scalar, lane offset: vector): scalar-base loads and stores, no
    // 64-bit arithmetic in the loop.  The kernel issues MORE scalar than vector instructions per wave (833 against 721 in
    // round 3's profile, and a SIMD issues one of each per slot at best), so the loop's bookkeeping is written for the
    // scalar count: a row's offset is one multiply of its clamped index (pointer += select(pitch, 0) took five
    // instructions), the destination advances by one 32-bit add, the row taps end in a sentinel.
    const uint8_t *srcBase = S;
    uint8_t *dstBase = pyr + (size_t)slot * g.pyrPerSlot + D.off + (size_t)j0 * D.pitch;
    unsigned dOff = 0;
    const unsigned laneSrc = (unsigned)base, laneDst = (unsigned)dx;
    const bool store2 = dx + 1 < D.w, store1 = dx < D.w;
    // PR_PF source rows are in flight ahead of the one being used (a ring of registers, the loop unrolled over it): a
    // wave's life is a chain of dependent row loads, and a store counts on the same counter as a load, so with one row
    // in flight every wait would also wait for the stores just issued.
    // The loop exists twice: for strips inside the level, where every lane stores its two columns (no exec masks in the
    // loop), and for the last strip of a row of strips.
    auto run = [&](auto edgeTag) {
        constexpr bool EDGE = decltype(edgeTag)::value;
        int pfIdx = r;  // the next row to request: min(pfIdx, rLast) (the ring runs up to PR_PF - 1 rows past the strip's last)
        auto prefetch = [&]() -> ft_u2 {
            unsigned offS = laneSrc + (unsigned)min(pfIdx, rLast) * (unsigned)spitch;
            // (the empty asm keeps the zero-extension of the offset inside this block, where instruction selection can fold
            // it into the scalar-base addressing mode)
            asm volatile("" : "+v"(offS));
            const ft_u2 v = gload<ft_u2>(srcBase + offS);
            pfIdx++;
            return v;
        };
        ft_u2 q[PR_PF];
#pragma unroll
        for (int k = 0; k < PR_PF; k++) q[k] = prefetch();
        unsigned hpA = 0, hpB = 0, hcA = 0, hcB = 0;
        // a source row is used up by its two horizontal interpolations; the next row of the ring is requested into the same
        // registers right behind them (requested before, it would need registers of its own and the ring would have to be
        // copied around at the end of every trip - behind a wait for all of its loads)
        auto take = [&](ft_u2 &q) {
            hpA = hcA; hpB = hcB;
            hcA = udot2_u16(__builtin_amdgcn_perm(q.y, q.x, selA), wa);
            hcB = udot2_u16(__builtin_amdgcn_perm(q.y, q.x, selB), wb);
            if constexpr (!AREA) { hcA >>= 4; hcB >>= 4; }
            q = prefetch();
        };
        auto step = [&]() {
            while (sy1 == r) {  // wave-uniform; behind the last output row sy1 matches no row
                // both taps on one source row happens only where cv::resize clamps the rows (top and bottom edge): monotonic,
                // so the upper-row registers may simply be overwritten
                if (__builtin_expect(sy0 == r, 0)) {  // wave-uniform and rare: a branch, not two selects per row
                    hpA = hcA; hpB = hcB;
                    asm volatile("" : "+v"(hpA), "+v"(hpB));
                }
                unsigned oA, oB;
                if constexpr (AREA) {
                    oA = (hpA + hcA + 2u) >> 2; oB = (hpB + hcB + 2u) >> 2;
                } else {
                    // ((b0 * (H0 >> 4)) >> 16) + ((b1 * (H1 >> 4)) >> 16) + 2) >> 2: each product's high half in one instruction
                    // (v_mul_hi_u32 with the weight as b << 16), one three-operand add, one shift - four instructions per
                    // output value where round 5 had six (24-bit multiply-add, shift, multiply, shift, add, shift)
                    oA = (umulhi_su(b0, hpA) + umulhi_su(b1, hcA) + 2u) >> 2;
                    oB = (umulhi_su(b0, hpB) + umulhi_su(b1, hcB) + 2u) >> 2;
                }
                unsigned offD = laneDst + dOff;
                asm volatile("" : "+v"(offD));
                if constexpr (!EDGE) {
                    gstore<unsigned short>(dstBase + offD, (unsigned short)(oA | (oB << 8)));
                } else {
                    if (store2) gstore<unsigned short>(dstBase + offD, (unsigned short)(oA | (oB << 8)));
                    else if (store1) gstore<uint8_t>(dstBase + offD, (uint8_t)oA);
                }
                dOff += (unsigned)D.pitch;
                jr++;
                rowTap(jr, sy0, sy1, b0, b1);  // (row nrows: the sentinel)
            }
            r++;
        };
        // whole trips of PR_PF: the steps behind the last source row see the last row again (the prefetch pointer stops
        // there) and write nothing, since every output row is done by then (sy1 = -1)
        for (int left = rLast - r + 1; left > 0; left -= PR_PF) {
#pragma unroll
            for (int k = 0; k < PR_PF; k++) {
                take(q[k]);
                step();
            }
        }
    };
    if (tx * PR_COLS + PR_COLS <= D.w) run(std::false_type{});  // wave-uniform
    else run(std::true_type{});
}

template <bool AREA>
__global__ __launch_bounds__(64) void k_pyr_rows(FtGeom g, int level, const uint8_t *const *l0, int l0pitch, uint8_t *pyr,
                                                 const FtTap *taps, FtSlotGrid sg, int stripsX, unsigned sxMagic,
                                                 int readableEnd) {
    const int lane = threadIdx.x;
    int slot, tile;
    if (!ft_slot_block(sg, slot, tile)) return;
    const int ty = div_by(tile, sxMagic), tx = tile - ty * stripsX;
    int spitch;
    const uint8_t *S = level_ptr(g, level - 1, slot, l0, l0pitch, pyr, spitch);
    pyr_rows_strip<AREA, false>(g, level, slot, tx, ty * PR_RB, 0, lane, S, spitch, pyr, taps, readableEnd);
}

// ------------------------------------------------------------------------------------------------
// Pyramid, all levels in ONE launch: an image is cut into K horizontal bands (FtPyrBands, planned on the host by
// ft_pyr_bands_of) and a workgroup of PC_WAVES waves walks one band of one image through the levels 1 .. n - 1.  At every
// level the band's row range is the hull of the rows it owns and of the source rows its range one level up reads, so a
// workgroup only ever reads rows that it wrote itself (rows in the overlap of two bands are computed by both, with the
// same bytes): no dependency between workgroups, no waiting on memory.  Inside the workgroup a level is handed to the next
// by a workgroup barrier between a release and an acquire fence; the waves of a workgroup share one CU's vector L1 (the
// Makefile refuses -mtgsplit), so what a wave stored is what the others load.  Pyramid pixels stay on vector loads and
// stores (pyr_rows_strip: gload / gstore), never on scalar loads: the scalar cache is not coherent with them.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * PC_WAVES) void k_pyr_cascade(FtGeom g, const uint8_t *const *l0, int l0pitch, uint8_t *pyr,
                                                              const FtTap *taps, FtSlotGrid sg, FtPyrBands pb,
                                                              int l0ReadableEnd) {
    const int lane = threadIdx.x & 63, wave = wave_index();
    int slot, band;
    if (!ft_slot_block(sg, slot, band)) return;  // (the whole workgroup)
    const uint8_t *const frame = l0[slot];  // read before the first store: a scalar load
    for (int level = 1; level < g.nlevels; level++) {
        const unsigned rr = pb.rows[level][band];
        const int r0 = (int)(rr & 0xffffu), r1 = (int)(rr >> 16);  // an empty range (r0 == r1) runs no strip
        const int stripsX = (g.lv[level].w + PR_COLS - 1) / PR_COLS;
        const unsigned sxMagic = div_magic_small((unsigned)stripsX);
        const int n = stripsX * ((r1 - r0 + PR_RB - 1) / PR_RB);
        const int readableEnd = level == 1 ? l0ReadableEnd : g.lv[level - 1].pitch;
        const int spitch = level == 1 ? l0pitch : g.lv[level - 1].pitch;
        const uint8_t *S = level == 1 ? frame : pyr + (size_t)slot * g.pyrPerSlot + g.lv[level - 1].off;
        for (int s = wave; s < n; s += PC_WAVES) {
            const int ty = div_by(s, sxMagic), tx = s - ty * stripsX;
            const int j0 = r0 + ty * PR_RB;
            if (g.lv[level].area2x) pyr_rows_strip<true, true>(g, level, slot, tx, j0, r1, lane, S, spitch, pyr, taps, readableEnd);
            else pyr_rows_strip<false, true>(g, level, slot, tx, j0, r1, lane, S, spitch, pyr, taps, readableEnd);
        }
        if (level + 1 < g.nlevels) {  // every wave of the workgroup passes here, whatever its band holds at this level
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __syncthreads();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        }
    }
}

}  // namespace

// the row-streaming kernel needs every lane's four taps inside one aligned 8-byte window of a source row
static bool pyr_rows_fits(const FtGeom &g, int level) {
    const FtLevelGeom &D = g.lv[level], &P = g.lv[level - 1];
    // the window starts at sx(dx) & ~3 (<= 3 bytes before the first tap), sx(dx + 1) <= sx(dx) + ceil(scale), and the
    // second tap of column dx + 1 is one further: 3 + ceil(scale) + 1 <= 7 holds for every scale <= 3
    return (double)P.w / (double)D.w < 2.5 && P.w >= 8;
}

int ft_launch_pyramid(hipStream_t st, const FtGeom &g, int batch, const uint8_t *const *l0, int l0pitch,
                      uint8_t *pyr, const FtTap *taps, int alignedLoads, int rowsKernel, const FtPyrBands *bands) {
    const bool rowsOn = rowsKernel != 0;
    // wide launches whose every level the row-streaming strip can produce: all levels in one launch (k_pyr_cascade)
    bool cascade = rowsKernel == 2 && batch >= 8 && alignedLoads && bands && bands->K >= 1 && g.nlevels >= 2;
    for (int level = 1; cascade && level < g.nlevels; level++) cascade = pyr_rows_fits(g, level);
    if (cascade) {
        dim3 grid, block(64 * PC_WAVES, 1, 1);
        const FtSlotGrid sg = ft_slot_grid(bands->K, batch, grid);
        const int readableEnd = std::min((g.lv[0].w + 3) & ~3, l0pitch);  // of a row of the caller's frame (see below)
        for (int rep = ft_debug_repeat("pyr"); rep > 0; rep--)
            hipLaunchKernelGGL(k_pyr_cascade, grid, block, 0, st, g, l0, l0pitch, pyr, taps, sg, *bands, readableEnd);
        FT_HIP(hipGetLastError());
        return FT_OK;
    }
    for (int rep = ft_debug_repeat("pyr"); rep > 0; rep--)
    for (int level = 1; level < g.nlevels; level++) {
        const FtLevelGeom &D = g.lv[level], &P = g.lv[level - 1];
        // a launch of a few images is latency bound: the tile kernel's many short waves finish a level sooner than the
        // row-streaming kernel's few long ones (752x480 frame: 0.19 against 0.23 ms); wide launches take the streaming kernel
        if (rowsOn && batch >= 8 && alignedLoads && pyr_rows_fits(g, level)) {
            const int stripsX = (D.w + PR_COLS - 1) / PR_COLS, stripsY = (D.h + PR_RB - 1) / PR_RB;
            dim3 grid, block(64, 1, 1);
            const FtSlotGrid sg = ft_slot_grid(stripsX * stripsY, batch, grid);
            // bytes of a source row that may be read: the whole pitch of a slot level, the width rounded up to a dword
            // (inside the 4-byte aligned stride) of a caller's frame
            const int readableEnd = level == 1 ? std::min((P.w + 3) & ~3, l0pitch) : P.pitch;
            if (D.area2x)
                hipLaunchKernelGGL(k_pyr_rows<true>, grid, block, 0, st, g, level, l0, l0pitch, pyr, taps, sg, stripsX,
                                   div_magic_of((unsigned)stripsX), readableEnd);
            else
                hipLaunchKernelGGL(k_pyr_rows<false>, grid, block, 0, st, g, level, l0, l0pitch, pyr, taps, sg, stripsX,
                                   div_magic_of((unsigned)stripsX), readableEnd);
            continue;
        }
        // LDS footprint of a 64 x 8 output tile: ceil(tile * scale) + the second tap + the margin of the
        // arithmetic footprint bound + alignment slack
        const int cols = (int)((long long)PD_TW * P.w / D.w) + 8, rowsN = (int)((long long)PD_TH * P.h / D.h) + 8;
        const int ldsPitch = (cols + 3 + 3) & ~3;
        // scale = source size / destination size in 16.16, rounded up (the error stays far below one pixel)
        const unsigned sxQ16 = (unsigned)(((unsigned long long)P.w << 16) / (unsigned)D.w) + 1u;
        const unsigned syQ16 = (unsigned)(((unsigned long long)P.h << 16) / (unsigned)D.h) + 1u;
        const int tilesX = (D.w + PD_TW - 1) / PD_TW, tilesY = (D.h + PD_TH - 1) / PD_TH;
        dim3 grid, block(64, 1, 1);
        const FtSlotGrid sg = ft_slot_grid(tilesX * tilesY, batch, grid);
        hipLaunchKernelGGL(k_pyr_down, grid, block, (size_t)ldsPitch * rowsN + 4, st, g, level, l0, l0pitch, pyr, taps,
                           alignedLoads, ldsPitch, rowsN, sxQ16, syQ16, sg, tilesX, div_magic_of((unsigned)tilesX));
    }
    FT_HIP(hipGetLastError());
    return FT_OK;
}
