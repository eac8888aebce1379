// HIP kernels of the ORB extractor's corner detection for gfx950 (CDNA4, wave64).  Results equal the reference's CPU branch:
//   k_fast_cells<TP, ORDERED>   per-cell cv::FAST-9/16 + NMS + threshold fallback (ORBextractor.cc:1136-1199);
//                               has_arc9 / fast_score / fast_score2 are cv::FAST's arc test and cornerScore<16>
//   k_compact                   cell-row-major ordered candidate list          (ORBextractor.cc:1186-1198)
// ft_launch_fast_cells runs one launch per LDS tile pitch (48 / 64, or the any-size variant TP = 0).
#include "extract_dev.h"

namespace {

// ------------------------------------------------------------------------------------------------
// FAST-9/16 per cell.  One workgroup per (cell, image).  The cell's (wCell+6)x(hCell+6) uint8 tile is
// staged in LDS; scores (largest threshold at which the pixel is still a corner) go to an LDS score
// plane whose zero rim implements "a neighbour belonging to another cell counts as 0"; survivors are
// compacted in row-major order with ballot/popcount prefix sums (no atomics: the octree's result
// depends on candidate order).
// ------------------------------------------------------------------------------------------------
typedef unsigned short fs_us2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned pk_max_u16(unsigned a, unsigned b) {
    return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(fs_us2, a), __builtin_bit_cast(fs_us2, b)));
}
__device__ __forceinline__ unsigned pk_min_u16(unsigned a, unsigned b) {
    return __builtin_bit_cast(unsigned, __builtin_elementwise_min(__builtin_bit_cast(fs_us2, a), __builtin_bit_cast(fs_us2, b)));
}
__device__ __forceinline__ bool has_arc9(unsigned m) {
    unsigned d = m | (m << 16);
    unsigned a = d & (d >> 1);
    a &= a >> 2;
    a &= a >> 4;
    a &= d >> 8;
    return (a & 0xffffu) != 0;
}

// ring offsets (x,y) k = 0..15: ORBextractor.cc:418-419
#define FT_RING(F)                                                                                            \
    F(0, 0, 3) F(1, 1, 3) F(2, 2, 2) F(3, 3, 1) F(4, 3, 0) F(5, 3, -1) F(6, 2, -2) F(7, 1, -3) F(8, 0, -3)    \
    F(9, -1, -3) F(10, -2, -2) F(11, -3, -1) F(12, -3, 0) F(13, -3, 1) F(14, -2, 2) F(15, -1, 3)

__device__ __forceinline__ int fast_score(int v, const int p[16]) {
    // score = max over the 16 arcs of 9 of min(v - p_i) (either polarity) - 1  == cornerScore<16> for corners.
    // min over an arc of (v - p_i) = v - max over the arc of p_i, so the arc extrema are taken on the ring pixels
    // themselves and v enters once at the end: score = max(v - min_k max9_k(p), max_k min9_k(p) - v) - 1.
    // Arc extrema from runs of three: ext9[k] = ext3(ext3[k], ext3[k+3], ext3[k+6]) - v_min3 / v_max3 make every line
    // below one instruction per element (64 in all, plus 16 for the two final reductions).
    int mn3[16], mx3[16];
#pragma unroll
    for (int k = 0; k < 16; k++) {
        mn3[k] = min(min(p[k], p[(k + 1) & 15]), p[(k + 2) & 15]);
        mx3[k] = max(max(p[k], p[(k + 1) & 15]), p[(k + 2) & 15]);
    }
    int mn9[16], mx9[16];
#pragma unroll
    for (int k = 0; k < 16; k++) {
        mn9[k] = min(min(mn3[k], mn3[(k + 3) & 15]), mn3[(k + 6) & 15]);
        mx9[k] = max(max(mx3[k], mx3[(k + 3) & 15]), mx3[(k + 6) & 15]);
    }
    int darkest = max(max(mn9[0], mn9[1]), mn9[2]), brightest = min(min(mx9[0], mx9[1]), mx9[2]);
#pragma unroll
    for (int k = 3; k < 15; k += 2) {
        darkest = max(max(darkest, mn9[k]), mn9[k + 1]);
        brightest = min(min(brightest, mx9[k]), mx9[k + 1]);
    }
    darkest = max(darkest, mn9[15]);      // max over arcs of the arc's darkest pixel
    brightest = min(brightest, mx9[15]);  // min over arcs of the arc's brightest pixel
    return max(v - brightest, darkest - v) - 1;
}

// cornerScore of TWO candidates per lane: their ring pixels travel in the halves of a register, and the arc extrema are
// taken with v_pk_minimum3_f16 / v_pk_maximum3_f16 (gfx950) - three operands AND two halves per instruction, half the
// instructions of the v_min3_u32 / v_max3_u32 network above per candidate.  The bit patterns 0x0000 .. 0x00ff are f16
// denormals n * 2^-24, which order like the integers they are; tools/pkmin3_probe.hip checks on the hardware that neither
// instruction flushes or canonicalises them (all 2 x 16.7 M operand triples, both halves).  v = the two centre pixels.
__device__ __forceinline__ unsigned pk_min3_h(unsigned a, unsigned b, unsigned c) {
    unsigned r;
    asm("v_pk_minimum3_f16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ unsigned pk_max3_h(unsigned a, unsigned b, unsigned c) {
    unsigned r;
    asm("v_pk_maximum3_f16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
typedef short fs_s2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned fast_score2(unsigned v, const unsigned p[16]) {
    unsigned mn3[16], mx3[16];
#pragma unroll
    for (int k = 0; k < 16; k++) {
        mn3[k] = pk_min3_h(p[k], p[(k + 1) & 15], p[(k + 2) & 15]);
        mx3[k] = pk_max3_h(p[k], p[(k + 1) & 15], p[(k + 2) & 15]);
    }
    unsigned mn9[16], mx9[16];
#pragma unroll
    for (int k = 0; k < 16; k++) {
        mn9[k] = pk_min3_h(mn3[k], mn3[(k + 3) & 15], mn3[(k + 6) & 15]);
        mx9[k] = pk_max3_h(mx3[k], mx3[(k + 3) & 15], mx3[(k + 6) & 15]);
    }
    unsigned darkest = pk_max3_h(mn9[0], mn9[1], mn9[2]), brightest = pk_min3_h(mx9[0], mx9[1], mx9[2]);
#pragma unroll
    for (int k = 3; k < 15; k += 2) {
        darkest = pk_max3_h(darkest, mn9[k], mn9[k + 1]);
        brightest = pk_min3_h(brightest, mx9[k], mx9[k + 1]);
    }
    const fs_s2 dk = __builtin_bit_cast(fs_s2, pk_max3_h(darkest, mn9[15], mn9[15]));
    const fs_s2 br = __builtin_bit_cast(fs_s2, pk_min3_h(brightest, mx9[15], mx9[15]));
    const fs_s2 vv = __builtin_bit_cast(fs_s2, v);
    const fs_s2 sc = __builtin_elementwise_max(vv - br, dk - vv) - (fs_s2)(1);
    return __builtin_bit_cast(unsigned, sc);
}

// One WAVE per (cell, image): no workgroup barrier anywhere, so the ~20 cells resident on a CU hide each other's
// load and LDS latency (LDS per wave is kept near 6 KB); measured VALU bound (EXPERIMENTS.md section 3).
// TP = LDS pitch of the tile and of the score plane; TP > 0 makes every ring / neighbour offset an
// instruction immediate, TP == 0 is the any-size fallback.
// LDS carve (bytes): tile th*tp | score (ph+2)*tp | candidate ring FC_CAND u16 | corner list FC_CORN u16 ;
// the survivor flags reuse the tile once the scores are final.
#ifndef FC_CAND
#define FC_CAND 512   // candidates buffered between the rejection test and the score pass
#endif
#ifndef FC_XCD_RUN
#define FC_XCD_RUN 8
#endif
#ifndef FC_UNROLL
#define FC_UNROLL 2
#endif
#ifndef FC_ROWS
#define FC_ROWS 4     // rows per trip of the column-mapped rejection pass (>= 3)
#endif
#ifndef FC_NMS_REG
#define FC_NMS_REG 2  // corner-list chunks (64 corners each) whose NMS flags stay in registers
#endif
#ifndef FC_CORN
#define FC_CORN 384   // corners kept for NMS / emission; a cell with more falls back to scanning the plane (256: the cells of
                      // dense frames, ~330 corners, all took the scan: dense scenes +2.4 % with 384, the headline +0.7 %; 448: -1 %)
#endif
#ifndef FC_WAVES_PER_EU
#define FC_WAVES_PER_EU 1
#endif
__host__ __device__ __forceinline__ int fc_pitch(int wCell, int TP) { return TP ? TP : ((wCell + 12) & ~3); }
__host__ __device__ __forceinline__ int fc_tile_bytes(int wCell, int hCell, int TP) {
    // the flags of the slow path need one byte per tested pixel
    const int t = (hCell + 6) * fc_pitch(wCell, TP), f = wCell * hCell;
    return ((t > f ? t : f) + 15) & ~15;
}
__host__ __device__ __forceinline__ int fc_score_bytes(int wCell, int hCell, int TP) { return (((hCell + 2) * fc_pitch(wCell, TP)) + 15) & ~15; }
__host__ __device__ __forceinline__ int fc_list_bytes() { return 2 * (FC_CAND + FC_CORN) + 16; }  // + the spare entry

// dbg (FT_DEBUG_FAST, a timing probe - results are wrong with 1, 2, 4, 16 (16 drops the candidates: phase A alone); 8 only switches the paired score rounds off): 1 replaces the score network by a three-pixel hash, 2 stops in
// front of NMS / emission, 4 right behind the staging of the tile; tools/fast_probe.py times the kernel with each of them.
// ORDERED = false (device octree, which ranks candidates by their coordinates): the rejection pass is free to
// visit the pixels in any order and uses all 64 lanes (see below); ORDERED = true delivers every cell's
// candidates row-major, as the host octree expects them.
template <int TP, bool ORDERED>
__global__ __launch_bounds__(64, FC_WAVES_PER_EU) void k_fast_cells(FtGeom g, const uint8_t *const *l0, int l0pitch, const uint8_t *pyr,
                                                   int iniTh, int minTh, int alignedLoads, int *cellCount,
                                                   uint32_t *stage, const FtCellRec *cellTab, FtSlotGrid sg, int dbg, int tileBytes,
                                                   int scoreBytesMax, FtCellRanges cr) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int lane = threadIdx.x;
    int slot = blockIdx.y, cellSg = 0;
    if (sg.xcdMap && !ft_slot_block(sg, slot, cellSg)) return;
    const uint8_t *img0 = l0[slot];  // level 0 is the caller's frame; requested before anything depends on the level
    // XCD-aware mapping: workgroup b runs on XCD b % 8 (observed placement, used for speed only).  Launches of eight
    // or more images put all cells of an image on one XCD (ft_slot_grid, above): neighbouring cells - their tiles
    // overlap by 6 px in both directions and share 64-B lines - hit the same private L2, which also still holds what
    // the pyramid kernel wrote for that image.  Smaller launches deal runs of FC_XCD_RUN consecutive cells round-robin
    // to the XCDs, so that at least horizontal neighbours share an L2 while all XCDs stay busy on the few images.
    const int j = (int)(blockIdx.x >> 3), xcd = (int)(blockIdx.x & 7);
    // the launch's cells: one or two runs of consecutive cells of the image's cell table (ft_launch_fast_cells: the levels whose
    // tiles fit this variant's pitch)
    const int cj = sg.xcdMap ? cellSg : ((j / FC_XCD_RUN) * 8 + xcd) * FC_XCD_RUN + (j % FC_XCD_RUN);
    if (cj >= cr.n0 + cr.n1) return;
    const int cell = cj < cr.n0 ? cr.lo0 + cj : cr.lo1 + (cj - cr.n0);
    // the cell's record, built with the extractor: origin, tile size, level, source and staging offsets in one scalar load
    const FtCellRec rec = cellTab[cell];
    const int iniX = (int)(rec.origin & 0xffffu), iniY = (int)(rec.origin >> 16);
    const int tw = (int)(rec.shape & 0xffu), th = (int)((rec.shape >> 8) & 0xffu), level = (int)((rec.shape >> 16) & 0xffu);
    int *cnt = cellCount + (size_t)slot * g.totalCells + cell;
    // ORBextractor.cc:1141,1150 skip rules; cv::FAST finds nothing in a sub-image under 7 px (the record says so)
    if (tw == 0) {
        if (lane == 0) *cnt = 0;
        return;
    }
    const unsigned lv = g.fastLv[level];
    const int cellCap = (int)(lv >> 16);
    const int pw = tw - 6, ph = th - 6;  // tested region
    const int npx = pw * ph;
    // the any-size variant derives its LDS pitch from the level's cell width; the fixed-pitch variants carve the LDS by the
    // launch-wide maxima (the launcher sizes the allocation by them anyway)
    const int tp = TP ? TP : fc_pitch(g.lv[level].wCell, 0);
    // division by the row length: only the any-size variant unpacks pixel codes with it (the fixed-pitch variants
    // need it on the rare score-plane scan alone and compute it there)
    const unsigned pwMagic = TP ? 0u : div_magic_of((unsigned)pw);
    uint8_t *tile = smem;
    uint8_t *score = tile + (TP ? tileBytes : fc_tile_bytes(g.lv[level].wCell, g.lv[level].hCell, 0));
    const int scoreBytes = TP ? ((ph + 2) * TP + 15) & ~15 : fc_score_bytes(g.lv[level].wCell, g.lv[level].hCell, 0);
    unsigned short *cand = (unsigned short *)(score + (TP ? scoreBytesMax : scoreBytes));
    unsigned short *corn = cand + FC_CAND;
    const int pitch = level ? (int)(lv & 0xffffu) : l0pitch;
    // pixel (iniX, iniY) of the level
    const uint8_t *org = level ? pyr + ((size_t)slot * g.pyrPerSlot + rec.srcOff) : img0 + ((size_t)iniY * l0pitch + iniX);
    // ---- stage the tile: aligned dword rows when the level allows it (coalesced 4-byte lanes) ----
    int ax = 0;
    if (alignedLoads) {
        ax = iniX & 3;
        const int nd = (tw + ax + 3) >> 2;
        const uint8_t *src = org - ax;
        if constexpr (TP != 0) {
            // fixed (row, dword) per lane: TP/4 dwords span a tile row, 64 / (TP/4) rows per trip.  Rows and dwords beyond
            // the tile are clamped to its last row / dword instead of being masked: such a lane loads and stores the
            // same element as the lane that owns it, so the whole copy is branch-free - no per-load division, no 64-bit
            // arithmetic, no exec-mask bookkeeping.  Nine trips are in flight before the first LDS store.
            constexpr int DW = TP / 4, RPT = 64 / DW;
            const int rr = lane / DW, cc4 = 4 * min(lane - rr * DW, nd - 1);
            if (th > 8 * RPT && th <= 9 * RPT) {  // wave-uniform
                // the usual cell (41 - 45 tile rows at TP 48): the first eight row groups exist for every lane, so their
                // rows need no clamp - a load is one address add, its LDS store an immediate offset; only the ninth is clamped
                const unsigned goff = (unsigned)vmad24(rr, pitch, cc4);
                unsigned *tl = (unsigned *)(tile + vmad24(rr, TP, cc4));
                const int row8 = min(8 * RPT + rr, th - 1);
                unsigned v[9];
#pragma unroll
                for (int k = 0; k < 8; k++) v[k] = gload<unsigned>(src + (goff + (unsigned)(k * RPT * pitch)));
                v[8] = gload<unsigned>(src + (unsigned)vmad24(row8, pitch, cc4));
#pragma unroll
                for (int k = 0; k < 8; k++) tl[k * RPT * (TP / 4)] = v[k];
                *(unsigned *)(tile + vmad24(row8, TP, cc4)) = v[8];
            } else
            for (int r0 = 0; r0 < th; r0 += 9 * RPT) {
                unsigned v[9];
                int row[9];
#pragma unroll
                for (int k = 0; k < 9; k++) {
                    row[k] = min(r0 + k * RPT + rr, th - 1);
                    v[k] = gload<unsigned>(src + (unsigned)vmad24(row[k], pitch, cc4));
                }
#pragma unroll
                for (int k = 0; k < 9; k++) *(unsigned *)(tile + vmad24(row[k], TP, cc4)) = v[k];
            }
        } else {
            const unsigned ndMagic = div_magic_of((unsigned)nd);
            // every load of the tile is issued before the first LDS store
            for (int i0 = 0; i0 < nd * th; i0 += 64 * 9) {
                unsigned v[9];
                int off[9];
#pragma unroll
                for (int k = 0; k < 9; k++) {
                    const int i = i0 + 64 * k + lane, ic = min(i, nd * th - 1);
                    const int y = div_by(ic, ndMagic), x = ic - y * nd;
                    off[k] = i < nd * th ? y * tp + 4 * x : -1;
                    v[k] = gload<unsigned>(src + (size_t)y * pitch + 4 * x);
                }
#pragma unroll
                for (int k = 0; k < 9; k++)
                    if (off[k] >= 0) *(unsigned *)(tile + off[k]) = v[k];
            }
        }
    } else {
        const unsigned twMagic = div_magic_of((unsigned)tw);
        const uint8_t *src = org;
        for (int i = lane; i < tw * th; i += 64) {
            const int y = div_by(i, twMagic), x = i - y * tw;
            tile[y * tp + x] = gload<uint8_t>(src + (size_t)y * pitch + x);
        }
    }
    // the whole score plane (a multiple of 16 bytes, 16-byte aligned) is cleared with 16-byte stores: two per lane
    for (int i = lane; i < scoreBytes >> 4; i += 64) ((uint4 *)score)[i] = make_uint4(0, 0, 0, 0);
    wave_lds_sync();
    if (dbg & 4) {
        if (lane == 0) *cnt = (int)tile[lane] & 0;
        return;
    }
    const uint8_t *t0 = tile + ax;  // pixel (x, y) of the cell sub-image at t0[y * tp + x]
    // ---- phase A / B rounds.  A: high-speed rejection (OpenCV's opposite-pair test without the
    // polarity): a 9-arc contains one pixel of every opposite pair, so for the two compass pairs (k = 0, 4)
    // max(|d_k|, |d_k+8|) must exceed the threshold; survivors are appended in row-major order to the
    // candidate ring (the any-size variant also tests the two diagonal pairs).  B (whenever the ring fills, and at the end): score = largest threshold at which
    // the pixel is still a corner (cornerScore<16>); corner at minThFAST <=> score >= minThFAST.
    int nc = 0, ncorn = 0;
    // A pixel of the tested region travels through the candidate ring and the corner list as a 16-bit code: with a
    // fixed pitch (pw < 64) that is (y << 6 | x), packed and unpacked with a shift and a mask; the any-size variant
    // keeps the linear index y * pw + x and pays a division per unpack.
    auto pixCode = [&](int y, int x) -> int { return TP > 0 ? ((y << 6) | x) : y * pw + x; };
    auto pixY = [&](int code) -> int { return TP > 0 ? code >> 6 : div_by(code, pwMagic); };
    auto pixX = [&](int code, int y) -> int { return TP > 0 ? (code & 63) : code - y * pw; };
    // phase B over the buffered candidates: score, corner list (row-major), ring reset
    auto flushB = [&]() {
        if (dbg & 16) {  // probe: phase A alone (the candidates are dropped)
            nc = 0;
            return;
        }
        wave_lds_sync();
        // Branch-free rounds: a lane beyond the last candidate repeats the last one (same score, same store) and is kept out
        // of the corner list by its flag; a candidate that is no corner stores 0 over the 0 the plane already holds; a lane
        // with nothing for the corner list writes the spare entry behind the lists.
        int jb = 0;
        if constexpr (TP > 0) {
            // rounds of 128: two candidates per lane through the packed network (fast_score2); the corner list takes the
            // first 64 of a round before the second 64, so its order is the ring's
            for (; nc - jb > 64 && !(dbg & 9); jb += 128) {  // dbg 8: A/B switch, rounds of 64 only
                const int jA = jb + lane, jB = jb + 64 + lane;
                const int cA = cand[jA], cB = cand[min(jB, nc - 1)];
                const int yA = pixY(cA), xA = pixX(cA, yA), yB = pixY(cB), xB = pixX(cB, yB);
                const uint8_t *wA = t0 + yA * tp + xA, *wB = t0 + yB * tp + xB;
                unsigned v2;
                unsigned ring2[16];
                // (Tried, round 3: the 7 x 7 window as seven unaligned ds_read_b64 / _b32 per candidate + v_perm_b32 - 14 LDS
                // instructions per round instead of 34 - is correct and TWICE as slow, 0.63 against 0.34 ms per launch of 128
                // frames: unaligned LDS accesses are replayed.  ds_read_u8 + ds_read_u8_d16_hi into one register, to save the 17
                // packing instructions: gfx950 runs with SRAM ECC, where a d16 load writes the whole register - wrong results.)
                v2 = (unsigned)wA[3 * tp + 3] | ((unsigned)wB[3 * tp + 3] << 16);
#define FT_LD2(k, ox, oy) ring2[k] = (unsigned)wA[((oy) + 3) * tp + (ox) + 3] | ((unsigned)wB[((oy) + 3) * tp + (ox) + 3] << 16);
                FT_RING(FT_LD2)
#undef FT_LD2
                const unsigned sc2 = fast_score2(v2, ring2);
                const int scA = (int)(short)(sc2 & 0xffffu), scB = (int)(short)(sc2 >> 16);
                const bool cornA = scA >= minTh, cornB = scB >= minTh;
                score[(yA + 1) * tp + (xA + 1)] = (uint8_t)(cornA ? scA : 0);
                score[(yB + 1) * tp + (xB + 1)] = (uint8_t)(cornB ? scB : 0);
                const bool isB = cornB && jB < nc;
                const unsigned long long ba = __builtin_amdgcn_ballot_w64(cornA), bb = __builtin_amdgcn_ballot_w64(isB);
                const int posA = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(ba >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)ba, (unsigned)ncorn));
                ncorn += __popcll(ba);
                const int posB = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bb >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bb, (unsigned)ncorn));
                ncorn += __popcll(bb);
                corn[cornA && posA < FC_CORN ? posA : FC_CORN] = (unsigned short)cA;  // corn + FC_CORN = the spare entry
                corn[isB && posB < FC_CORN ? posB : FC_CORN] = (unsigned short)cB;
            }
        }
        for (; jb < nc; jb += 64) {
            const int j = jb + lane;
            const int ci2 = cand[min(j, nc - 1)];
            const int y = pixY(ci2), x = pixX(ci2, y);
            // top-left corner of the pixel's 7 x 7 ring window: with a fixed pitch every ring offset is a non-negative
            // immediate of the LDS read (a negative one costs an address add of its own)
            const uint8_t *win = t0 + y * tp + x;
            const int v = win[3 * tp + 3];
            int ringPx[16];
#define FT_LD(k, ox, oy) ringPx[k] = (int)win[((oy) + 3) * tp + (ox) + 3];
            FT_RING(FT_LD)
#undef FT_LD
            const int sc = (dbg & 1) ? ((v + ringPx[0] + ringPx[5] + ringPx[11]) & 31) : fast_score(v, ringPx);
            const bool corner = sc >= minTh;
            score[(y + 1) * tp + (x + 1)] = (uint8_t)(corner ? sc : 0);
            const bool isCorner = corner && j < nc;
            const unsigned long long cb = __builtin_amdgcn_ballot_w64(isCorner);
            const int pos = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(cb >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)cb, (unsigned)ncorn));
            corn[isCorner && pos < FC_CORN ? pos : FC_CORN] = (unsigned short)ci2;  // corn + FC_CORN = the spare entry
            ncorn += __popcll(cb);
        }
        nc = 0;
        wave_lds_sync();
    };
#define FT_AD(ox, oy) __builtin_amdgcn_sad_u8(v, (unsigned)cpx[(oy)*tp + (ox)], 0u)
    // Appends the lanes of a row whose compass pairs pass to the candidate ring, in lane order, without a branch: the
    // other lanes store to the spare entry behind the lists.  (The two diagonal pairs used to be tested first; on
    // textured images that cost more instructions per row than the few candidates it removed cost in phase B, where
    // a partly filled round of 64 is as expensive as a full one.)
    auto pushRow = [&](bool pass, int code, int n) -> int {
        const unsigned long long b = __ballot(pass);
        const int pos = pass ? (int)__builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, (unsigned)n))
                             : FC_CAND + FC_CORN;
        cand[pos] = (unsigned short)code;
        return n + __popcll(b);
    };
    if constexpr (TP > 0 && !ORDERED) {
        // Two half-cells side by side: lanes 0-31 walk the rows of the upper half, lanes 32-63 the rows of the lower
        // half, 32 columns each (a 36-pixel-wide cell fills 56 % of a 64-lane row, two 32-wide halves fill it); the
        // columns beyond 32 go through the same form in bands of their own (below).  Inside a half the rows slide as in the
        // ordered pass (shared vertical differences, immediates only).
        const int half = lane >> 5, cx = lane & 31;
        const int hRows = (ph + 1) >> 1;          // rows of the upper half; the lower half has ph - hRows
        const int y0h = half * hRows;              // first row of this lane's half
        const int wMain = min(pw, 32);
        const bool actC = cx < wMain;
        const uint8_t *col = t0 + min(cx, wMain - 1) + 3 + y0h * TP;  // (x + 3, tile row y0h)
        const int codeBase = (y0h << 6) | cx;
        unsigned pA = col[3 * TP], pB = col[4 * TP], pC = col[5 * TP];
        // Rows travel in PAIRS (y, y + 1) packed in the halves of a register: v_sad_u8 / v_sad_hi_u8 produce the halves,
        // v_pk_max_u16 / v_pk_min_u16 combine them.  The vertical difference |p(y) - p(y + 3)| is the south difference of
        // row y and the north difference of row y + 3, so a north pair is an alignbit of two earlier south pairs.
        // History: hist0 = [., dS(y - 3)], hist1 = [dS(y - 2), dS(y - 1)].
        unsigned hist0 = __builtin_amdgcn_sad_hi_u8(pA, (unsigned)col[0], 0u);
        unsigned hist1 = __builtin_amdgcn_sad_hi_u8(pC, (unsigned)col[2 * TP], __builtin_amdgcn_sad_u8(pB, (unsigned)col[TP], 0u));
        const unsigned th = (unsigned)minTh;
        const int rowsHalf = actC ? (half ? ph - hRows : hRows) : 0;  // rows of this lane's column (none beyond the cell)
        // a lane's valid verdicts: cnt rows (clamped to 0 .. n; n <= T, both wave-uniform) at the top of a T-bit mask - three instructions
        auto validMask = [](int cnt, int n, int T) -> unsigned {
            int c;
            unsigned m;
            asm("v_med3_i32 %0, %1, 0, %2" : "=v"(c) : "v"(cnt), "s"(n));
            asm("v_bfm_b32 %0, %1, %2" : "=v"(m) : "v"(c), "v"(T - c));
            return m;
        };
        // The columns beyond 32 (wRem of them: 4 to 6 of a 36 to 38 pixel cell) go through the same packed sliding form in
        // a pass of their own: a lane takes (remainder column, band of rows), nbR = 64 / wRem bands of bR = ceil(ph / nbR)
        // rows - one trip of four rows on the usual cells (16 x 3, 12 x 4, 10 x 4), two or more on tall bands.  Every
        // width up to the 23 columns of a 64-byte pitch takes this form, there is no linear pass any more: by instruction
        // count (a trip costs about as much as one and a half 64-pixel rounds of the linear pass did and covers four rows
        // of up to 64 lanes) it is ahead at every wRem.  A band is never taller than a half (nbR >= 2), so the bands walk
        // their rows block by block beside the halves and share every block's scan.
        const int wRem = pw - wMain;
        const unsigned remMagic = div_magic_small((unsigned)wRem);
        int nbR = 0, bR = 0;
        if (wRem > 0) {  // wave-uniform scalar arithmetic, two table loads
            nbR = div_by(64, remMagic);
            bR = div_by(ph + nbR - 1, div_magic_small((unsigned)nbR));
        }
        // four rows of a lane's column: r = the column at the trip's first row, the rest is the lane's sliding state
        auto trip4 = [&](const uint8_t *r, unsigned &pA, unsigned &pB, unsigned &pC, unsigned &hist0, unsigned &hist1, unsigned &cmask) {
            unsigned pv[7];
            pv[0] = pA; pv[1] = pB; pv[2] = pC;
#pragma unroll
            for (int k = 0; k < 4; k++) pv[k + 3] = r[(k + 6) * TP];
            const unsigned ps0 = __builtin_amdgcn_sad_hi_u8(pv[1], pv[4], __builtin_amdgcn_sad_u8(pv[0], pv[3], 0u));
            const unsigned ps1 = __builtin_amdgcn_sad_hi_u8(pv[3], pv[6], __builtin_amdgcn_sad_u8(pv[2], pv[5], 0u));
            const unsigned pn0 = __builtin_amdgcn_alignbit(hist1, hist0, 16);  // [dS(y - 3), dS(y - 2)]
            const unsigned pn1 = __builtin_amdgcn_alignbit(ps0, hist1, 16);    // [dS(y - 1), dS(y)]
            const unsigned pe0 = __builtin_amdgcn_sad_hi_u8(pv[1], (unsigned)r[4 * TP + 3], __builtin_amdgcn_sad_u8(pv[0], (unsigned)r[3 * TP + 3], 0u));
            const unsigned pw0 = __builtin_amdgcn_sad_hi_u8(pv[1], (unsigned)r[4 * TP - 3], __builtin_amdgcn_sad_u8(pv[0], (unsigned)r[3 * TP - 3], 0u));
            const unsigned pe1 = __builtin_amdgcn_sad_hi_u8(pv[3], (unsigned)r[6 * TP + 3], __builtin_amdgcn_sad_u8(pv[2], (unsigned)r[5 * TP + 3], 0u));
            const unsigned pw1 = __builtin_amdgcn_sad_hi_u8(pv[3], (unsigned)r[6 * TP - 3], __builtin_amdgcn_sad_u8(pv[2], (unsigned)r[5 * TP - 3], 0u));
            const unsigned M0 = pk_min_u16(pk_max_u16(pn0, ps0), pk_max_u16(pe0, pw0));
            const unsigned M1 = pk_min_u16(pk_max_u16(pn1, ps1), pk_max_u16(pe1, pw1));
            hist0 = ps0; hist1 = ps1;
            pA = pv[4]; pB = pv[5]; pC = pv[6];
            // Every lane files the verdicts of its column in a bit mask of its own: the compare of a half of M against the
            // threshold lands in vcc and v_addc shifts it into the mask (mask = 2 * mask + vcc) - two vector instructions per row
            // and no scalar work at all, where a ballot per row with its popcount, position arithmetic and exec juggling cost
            // a dozen scalar instructions for every row that holds a candidate.
            asm("v_cmp_gt_u32_sdwa vcc, %1, %2 src0_sel:WORD_0 src1_sel:DWORD\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc\n\t"
                "v_cmp_gt_u32_sdwa vcc, %1, %2 src0_sel:WORD_1 src1_sel:DWORD\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc\n\t"
                "v_cmp_gt_u32_sdwa vcc, %3, %2 src0_sel:WORD_0 src1_sel:DWORD\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc\n\t"
                "v_cmp_gt_u32_sdwa vcc, %3, %2 src0_sel:WORD_1 src1_sel:DWORD\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc"
                : "+v"(cmask)
                : "v"(M0), "v"(th), "v"(M1)
                : "vcc");
        };
        // blocks of at most 28 rows (seven trips): a lane's verdicts of a block fit one 32-bit mask
        for (int yb = 0; yb < hRows; yb += 28) {
        const int yEnd = min(yb + 28, hRows);
        unsigned cmask = 0;
        auto trip = [&](int y) { trip4(col + y * TP, pA, pB, pC, hist0, hist1, cmask); };
        // two trips per iteration: the register rotation (pA / pB / pC, the two history pairs) between them is renaming
        // instead of four moves per trip
        int y = yb;
        for (; y + 4 < yEnd; y += 8) {
            trip(y);
            trip(y + 4);
        }
        if (y < yEnd) trip(y);
        // The remainder bands walk rows yb .. yb + 27 of their own beside the block (a band has no more rows than a half, and
        // on every workload's cells one block holds them all): their verdicts go into a second mask and share the block's
        // scan.  Row yb + r of a band sits at bit TR - 1 - r, as in the halves.
        unsigned rmask = 0;
        int codeTopR = 0;
        if (yb < bR) {  // wave-uniform (bR = 0 without remainder columns)
            // (the lane number is made opaque so that the band arithmetic is not hoisted out of the block loop: it would sit
            // in registers across phase B, where the kernel's register peak is, for a second block that hardly any cell has)
            int laneR = lane;
            asm volatile("" : "+v"(laneR));
            const int band = div_by(laneR, remMagic), rc = vmad24(band, -wRem, laneR);
            const int yy = vmad24(band, bR, yb);  // first row of the band in this block; bands beyond the cell (and the lanes
                                                  // behind the last band: nbR * bR >= ph) walk rows at its end, all masked out
            const uint8_t *rcol = (t0 + 35) + vmad24(min(yy, ph), TP, rc);  // (x + 3, tile row yy), x = 32 + rc
            unsigned qA = rcol[3 * TP], qB = rcol[4 * TP], qC = rcol[5 * TP];
            unsigned h0 = __builtin_amdgcn_sad_hi_u8(qA, (unsigned)rcol[0], 0u);
            unsigned h1 = __builtin_amdgcn_sad_hi_u8(qC, (unsigned)rcol[2 * TP], __builtin_amdgcn_sad_u8(qB, (unsigned)rcol[TP], 0u));
            const int nR = min(bR - yb, 28);
            trip4(rcol, qA, qB, qC, h0, h1, rmask);  // (the usual band is done with it)
            for (int yr = 4; yr < nR; yr += 4) trip4(rcol + (unsigned)(yr * TP), qA, qB, qC, h0, h1, rmask);
            const int TR = (nR + 3) & ~3;
            rmask &= validMask(ph - yy, nR, TR);
            codeTopR = ((yy << 6) + rc) + (((TR - 1) << 6) + 32);
        }
        // row yb + r of a half sits at bit T - 1 - r (T = rows walked in the block, a multiple of four); rows the half does
        // not have and columns beyond the cell are masked out here, once
        const int T = (yEnd - yb + 3) & ~3;
        cmask &= validMask(rowsHalf - yb, T, T);
        const int codeTop = codeBase + ((yb + T - 1) << 6);
        if (__builtin_amdgcn_ballot_w64((cmask | rmask) != 0u)) {  // wave-uniform: a flat block has nothing to scan or append
            // Emission.  The lanes' candidate counts (both masks) are scanned once (six DPP adds), which gives every lane the
            // ring slot of its first candidate; then every lane writes its own candidates one after the other, lowest bit
            // first, those of its half before those of its remainder band - as many rounds as the fullest lane holds
            // candidates (a ballot + popcount + position per round, as the rows used to cost, is what this avoids).
            int incl = __popc(cmask) + __popc(rmask);
            const int own = incl;
            incl += __builtin_amdgcn_update_dpp(0, incl, 0x111, 0xF, 0xF, true);  // row_shr:1
            incl += __builtin_amdgcn_update_dpp(0, incl, 0x112, 0xF, 0xF, true);  // row_shr:2
            incl += __builtin_amdgcn_update_dpp(0, incl, 0x114, 0xF, 0xF, true);  // row_shr:4
            incl += __builtin_amdgcn_update_dpp(0, incl, 0x118, 0xF, 0xF, true);  // row_shr:8
            incl += __builtin_amdgcn_update_dpp(0, incl, 0x142, 0xA, 0xF, true);  // row_bcast:15 into rows 1 and 3
            incl += __builtin_amdgcn_update_dpp(0, incl, 0x143, 0xC, 0xF, true);  // row_bcast:31 into rows 2 and 3
            const int total = __builtin_amdgcn_readlane(incl, 63);
            if (nc + total > FC_CAND - 64) flushB();  // wave-uniform; leaves nc = 0
            if (total <= FC_CAND - 64) {
                unsigned short *slot = cand + (nc + incl - own);
                // A lane leaves the loop (its exec bit) with its last candidate: six vector instructions and a write per round,
                // the exec bookkeeping is scalar.  The slot pointer of a lane ends behind its last main candidate, where its
                // remainder candidates go.
                auto append = [&](unsigned m, int top) {
                    if (m) {
                        do {
                            *slot = (unsigned short)vmad24(__builtin_ctz(m), -64, top);
                            slot++;
                            m &= m - 1u;
                        } while (m);
                    }
                };
                append(cmask, codeTop);
                append(rmask, codeTopR);
                nc += total;
            } else {
                // more candidates in one block than the ring holds (dense texture): a round per candidate rank with a flush
                // whenever the ring fills
                for (int part = 0; part < 2; part++) {
                    unsigned m = part ? rmask : cmask;
                    const int top = part ? codeTopR : codeTop;
                    for (;;) {
                        const unsigned long long b = __builtin_amdgcn_ballot_w64(m != 0u);
                        if (!b) break;  // wave-uniform
                        const int pos = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, (unsigned)nc));
                        const int bit = __builtin_ctz(m | 0x80000000u);
                        if (__builtin_amdgcn_inverse_ballot_w64(b)) cand[pos] = (unsigned short)(top - (bit << 6));
                        m &= m - 1u;
                        nc += __popcll(b);
                        if (nc > FC_CAND - 64) flushB();  // wave-uniform
                    }
                }
            }
        }
        }
        flushB();
    } else if constexpr (TP > 0) {
        // Fixed pitch (pw <= TP - 6 < 64): lane = column, rows walked top to bottom three at a time.  Every tile
        // offset is an immediate; the vertical differences |p(y) - p(y+3)| serve row y (south) and row y + 3
        // (north), and the centre of row y + 3 is the south pixel of row y, so a row costs three LDS reads and
        // seven VALU instructions per lane before the wave-level early out.
        const bool act = lane < pw;
        const uint8_t *col = t0 + min(lane, pw - 1) + 3;  // (x + 3, tile row 0)
        unsigned pA = col[3 * TP], pB = col[4 * TP], pC = col[5 * TP];
        unsigned dA = __builtin_amdgcn_sad_u8(pA, (unsigned)col[0], 0u);
        unsigned dB = __builtin_amdgcn_sad_u8(pB, (unsigned)col[TP], 0u);
        unsigned dC = __builtin_amdgcn_sad_u8(pC, (unsigned)col[2 * TP], 0u);
        // FC_ROWS rows per trip: all their LDS reads are issued before the first use, one wave-level early out
        // covers the trip
        for (int y = 0; y < ph; y += FC_ROWS) {
            const uint8_t *r = col + y * TP;
            unsigned pv[FC_ROWS + 3], m01[FC_ROWS], dSv[FC_ROWS], mAny = 0;
            pv[0] = pA; pv[1] = pB; pv[2] = pC;
#pragma unroll
            for (int k = 0; k < FC_ROWS; k++) pv[k + 3] = r[(k + 6) * TP];
#pragma unroll
            for (int k = 0; k < FC_ROWS; k++) {
                const unsigned v = pv[k];
                const uint8_t *cpx = r + (k + 3) * TP;
                const unsigned dS = dSv[k] = __builtin_amdgcn_sad_u8(v, pv[k + 3], 0u);
                const unsigned dN = k == 0 ? dA : k == 1 ? dB : k == 2 ? dC : dSv[k >= 3 ? k - 3 : 0];
                const unsigned m1 = max(FT_AD(3, 0), FT_AD(-3, 0));
                m01[k] = (act && y + k < ph) ? min(max(dN, dS), m1) : 0u;
                mAny = max(mAny, m01[k]);
            }
            dA = dSv[FC_ROWS - 3]; dB = dSv[FC_ROWS - 2]; dC = dSv[FC_ROWS - 1];
            pA = pv[FC_ROWS]; pB = pv[FC_ROWS + 1]; pC = pv[FC_ROWS + 2];
            if (__any(mAny > (unsigned)minTh)) {
#pragma unroll
                for (int k = 0; k < FC_ROWS; k++) nc = pushRow(m01[k] > (unsigned)minTh, pixCode(y + k, lane), nc);
            }
            if (nc > FC_CAND - FC_ROWS * 64 || y + FC_ROWS >= ph) flushB();  // wave-uniform
        }
    } else {
        // any-size fallback: pixels in linear order, FC_UNROLL 64-pixel chunks per trip
        for (int base = 0; base < npx; base += 64 * FC_UNROLL) {
            unsigned m01[FC_UNROLL];
            const uint8_t *cp[FC_UNROLL];
            unsigned mAny = 0;
#pragma unroll
            for (int u = 0; u < FC_UNROLL; u++) {
                const int i = base + 64 * u + lane;
                const int ii = min(i, npx - 1);
                const int y = div_by(ii, pwMagic), x = ii - y * pw;
                const uint8_t *cpx = t0 + (y + 3) * tp + (x + 3);
                cp[u] = cpx;
                const unsigned v = cpx[0];
                const unsigned m0 = max(FT_AD(0, 3), FT_AD(0, -3));
                const unsigned m1 = max(FT_AD(3, 0), FT_AD(-3, 0));
                m01[u] = i < npx ? min(m0, m1) : 0u;
                mAny = max(mAny, m01[u]);
            }
            // wave-level early out: when the compass pairs already reject every pixel of the trip (flat regions)
            // the two diagonal pairs are not even read
            if (__any(mAny > (unsigned)minTh)) {
#pragma unroll
                for (int u = 0; u < FC_UNROLL; u++) {
                    const int i = base + 64 * u + lane;
                    const uint8_t *cpx = cp[u];
                    const unsigned v = cpx[0];
                    const unsigned m2 = max(FT_AD(2, 2), FT_AD(-2, -2));
                    const unsigned m3 = max(FT_AD(2, -2), FT_AD(-2, 2));
                    const bool pass = min(m01[u], min(m2, m3)) > (unsigned)minTh;
                    const unsigned long long b = __ballot(pass);
                    if (pass) cand[nc + __popcll(b & ((1ull << lane) - 1ull))] = (unsigned short)i;
                    nc += __popcll(b);
                }
            }
            if (nc > FC_CAND - 64 * FC_UNROLL || base + 64 * FC_UNROLL >= npx) flushB();  // wave-uniform
        }
    }
#undef FT_AD
    wave_lds_sync();
    // ---- NMS (strictly greater than the 8 neighbours, cv::FAST), cell-level threshold fallback
    // (ORBextractor.cc:1157-1177: if any survivor reaches iniThFAST only those are emitted, otherwise every
    // minThFAST survivor is) and emission.  The corner list is in row-major order in the ORDERED variant; a cell with more
    // than FC_CORN corners scans the score plane instead (same order).
    if (dbg & 2) {
        if (lane == 0) *cnt = 0;
        return;
    }
    const bool useList = ncorn <= FC_CORN;
    const int nItems = useList ? ncorn : npx;
    auto nms = [&](int item, int &pix) -> int {
        int y, x;
        if (useList) {
            pix = (int)corn[item];
            y = pixY(pix), x = pixX(pix, y);
        } else {  // score-plane scan: item is the linear index of the pixel
            const unsigned mg = TP ? div_magic_of((unsigned)pw) : pwMagic;
            y = div_by(item, mg), x = item - y * pw;
            pix = pixCode(y, x);
        }
        // top-left neighbour of the pixel: every offset below is a non-negative immediate with a fixed pitch
        const uint8_t *s = score + y * tp + x;
        const unsigned v = s[tp + 1];
        // strictly greater than all eight neighbours <=> greater than their maximum (three v_max3 and a v_max, no
        // short-circuit branches); the maximum is >= 0, so a kept pixel has a score
        const unsigned m = max(max(max(max((unsigned)s[0], (unsigned)s[1]), (unsigned)s[2]),
                                   max(max((unsigned)s[tp], (unsigned)s[tp + 2]), (unsigned)s[2 * tp])),
                               max((unsigned)s[2 * tp + 1], (unsigned)s[2 * tp + 2]));
        return v > m ? (v >= (unsigned)iniTh ? 2 : 1) : 0;
    };
    uint32_t *out = stage + ((size_t)slot * g.stagePerSlot + rec.outOff);
    int run = 0;
    auto emit = [&](int fl, int pix, int need) {
        const bool f = fl >= need;
        const unsigned long long b = __builtin_amdgcn_ballot_w64(f);
        const int y = pixY(pix), x = pixX(pix, y);
        const int pos = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, (unsigned)run));
        // keypoint (x+3, y+3) in the cell sub-image, shifted by (j*wCell, i*hCell): ORBextractor.cc:1196-1197
        const uint32_t packed = ft_pack_cand(x + (iniX - 13), y + (iniY - 13), score[(y + 1) * tp + (x + 1)]);
        if (f && pos < cellCap) out[pos] = packed;
        run += __popcll(b);
    };
    if (nItems <= 64 * FC_NMS_REG) {
        // the usual case: the NMS flags of the whole cell stay in registers, the corner list is read once
        int fl[FC_NMS_REG], px[FC_NMS_REG], anyHi = 0;
#pragma unroll
        for (int q = 0; q < FC_NMS_REG; q++) {
            fl[q] = 0;
            px[q] = 0;
            if (q * 64 < nItems) {  // wave-uniform
                // lanes beyond the list look at its last entry and drop the verdict (no divergent branch)
                const int f = nms(min(q * 64 + lane, nItems - 1), px[q]);
                fl[q] = q * 64 + lane < nItems ? f : 0;
                anyHi |= __any(fl[q] == 2);
            }
        }
        const int need = anyHi ? 2 : 1;
#pragma unroll
        for (int q = 0; q < FC_NMS_REG; q++)
            if (q * 64 < nItems) emit(fl[q], px[q], need);
    } else {
        // More corners than the registers hold flags for (dense frames).  The threshold decision needs to know whether ANY
        // survivor reaches iniThFAST before the first one is emitted; round 3 computed every verdict, parked it in LDS and walked
        // the list a second time.  Now: a cell whose best corner is below iniThFAST cannot have such a survivor, and one whose
        // best corner reaches it nearly always has (only ties between neighbouring maxima can take them all out) - so the
        // decision is taken from the maximum score (one read per corner), the verdicts are computed and emitted in ONE walk,
        // and the rare cell where the strong corners all fell to ties is walked again for the weak ones.
        auto itemPix = [&](int it) -> int {
            if (useList) return (int)corn[it];
            const unsigned mg = TP ? div_magic_of((unsigned)pw) : pwMagic;
            const int y = div_by(it, mg);
            return pixCode(y, it - y * pw);
        };
        unsigned mx = 0;
        for (int base = 0; base < nItems; base += 64) {
            const int pix = itemPix(min(base + lane, nItems - 1));
            const int y = pixY(pix), x = pixX(pix, y);
            mx = max(mx, (unsigned)score[(y + 1) * tp + (x + 1)]);
        }
        int need = __any(mx >= (unsigned)iniTh) ? 2 : 1;
        for (;;) {
            int anyHi = 0;
            run = 0;
            for (int base = 0; base < nItems; base += 64) {
                const int it = base + lane;
                int pix = 0;
                const int f = nms(min(it, nItems - 1), pix);
                const int fl = it < nItems ? f : 0;
                anyHi |= __any(fl == 2);
                emit(fl, pix, need);
            }
            if (need == 1 || anyHi) break;  // wave-uniform
            need = 1;                       // every strong corner lost a tie: the cell emits its weak survivors
        }
    }
    if (lane == 0) *cnt = min(run, cellCap);
}

// ------------------------------------------------------------------------------------------------
// Compaction in cell order: one workgroup per (level, image).  Exclusive scan of the cell counts in cell
// order, then a coalesced gather into the dense list (which lives in host-mapped pinned memory so
// the host octree can read it after a single stream sync).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_compact(FtGeom g, const int *cellCount, const uint32_t *stage,
                                                 uint32_t *cand, int *candCount) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    int *offs = (int *)smem;  // nCells + 1
    __shared__ int wsum[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int level = blockIdx.x, slot = blockIdx.y;
    const FtLevelGeom &L = g.lv[level];
    const int nCells = L.nCols * L.nRows;
    const int *cnt = cellCount + (size_t)slot * g.totalCells + L.cellBase;
    const int per = (nCells + 255) / 256;
    const int c0 = tid * per, c1 = min(c0 + per, nCells);
    int local = 0;
    for (int c = c0; c < c1; c++) local += cnt[c];
    int incl = local;  // inclusive scan across the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        int t = __shfl_up(incl, o);
        if (lane >= o) incl += t;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int wbase = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) {
        if (w < wave) wbase += wsum[w];
        total += wsum[w];
    }
    int run = wbase + incl - local;
    for (int c = c0; c < c1; c++) {
        offs[c] = run;
        run += cnt[c];
    }
    if (tid == 0) offs[nCells] = total;
    __syncthreads();
    total = min(total, L.candCap);
    const uint32_t *st = stage + (size_t)slot * g.stagePerSlot + L.stageBase;
    uint32_t *dst = cand + (size_t)slot * g.candPerSlot + L.candBase;
    for (int o = tid; o < total; o += 256) {
        int lo = 0, hi = nCells;  // last cell with offs[cell] <= o
        while (hi - lo > 1) {
            int mid = (lo + hi) >> 1;
            if (offs[mid] <= o) lo = mid;
            else hi = mid;
        }
        dst[o] = st[(size_t)lo * L.cellCap + (o - offs[lo])];
    }
    if (tid == 0) candCount[slot * g.nlevels + level] = total;
}

}  // namespace

static int fast_tile_pitch(const FtGeom &g) {
    // fixed LDS pitch (all ring offsets immediates) when every level's cell fits: wCell + 6 + 3 <= TP
    int need = 0;
    for (int l = 0; l < g.nlevels; l++)
        if (g.lv[l].nCols * g.lv[l].nRows > 0) need = std::max(need, g.lv[l].wCell + 9);
    return need <= 48 ? 48 : (need <= 64 ? 64 : 0);
}

// LDS of a launch over the levels of `mask` at pitch TP (fixed-pitch variants: the largest tile and the largest score plane of
// those levels; the any-size variant: the largest sum)
static size_t fast_smem_of(const FtGeom &g, unsigned mask, int TP, int *tileBytes, int *scoreBytes) {
    size_t mxTile = 0, mxScore = 0, mxSum = 0;
    for (int l = 0; l < g.nlevels; l++) {
        const FtLevelGeom &L = g.lv[l];
        if (!((mask >> l) & 1u) || L.nCols * L.nRows <= 0) continue;
        const size_t t = (size_t)fc_tile_bytes(L.wCell, L.hCell, TP), sc = (size_t)fc_score_bytes(L.wCell, L.hCell, TP);
        mxTile = std::max(mxTile, t);
        mxScore = std::max(mxScore, sc);
        mxSum = std::max(mxSum, t + sc);
    }
    if (tileBytes) *tileBytes = (int)mxTile;
    if (scoreBytes) *scoreBytes = (int)mxScore;
    return (TP ? mxTile + mxScore : mxSum) + fc_list_bytes();
}

// the cells of the levels of `mask` as runs of consecutive cells; false: more than two runs (or none)
static bool fast_cell_ranges(const FtGeom &g, unsigned mask, FtCellRanges &cr) {
    int runs = 0, lo[2] = {0, 0}, n[2] = {0, 0};
    bool open = false;
    for (int l = 0; l < g.nlevels; l++) {
        const int cells = g.lv[l].nCols * g.lv[l].nRows;
        if (cells <= 0) continue;  // (no cells: the level neither starts nor ends a run)
        if ((mask >> l) & 1u) {
            if (!open) {
                if (runs == 2) return false;
                lo[runs] = g.lv[l].cellBase;
                n[runs] = 0;
                runs++;
                open = true;
            }
            n[runs - 1] += cells;
        } else {
            open = false;
        }
    }
    cr.lo0 = lo[0]; cr.n0 = n[0]; cr.lo1 = lo[1]; cr.n1 = n[1];
    return runs > 0;
}

int ft_launch_fast_cells(hipStream_t st, const FtGeom &g, int batch, const uint8_t *const *l0, int l0pitch,
                         const uint8_t *pyr, int iniTh, int minTh, int alignedLoads, int *cellCount,
                         uint32_t *stage, int ordered, const FtCellRec *cellTab) {
    if (g.totalCells == 0) return FT_OK;  // every level is too small for a 35-px cell: no candidates
    typedef void (*FastFn)(FtGeom, const uint8_t *const *, int, const uint8_t *, int, int, int, int *, uint32_t *, const FtCellRec *,
                           FtSlotGrid, int, int, int, FtCellRanges);
    static const int dbg = ft_debug_env("FT_DEBUG_FAST") ? atoi(ft_debug_env("FT_DEBUG_FAST")) : 0;
    static const bool occDbg = ft_debug_env("FT_DEBUG_OCC") != nullptr;  // resident workgroups per CU as the runtime computes them
    static const bool noSplit = ft_debug_env("FT_DEBUG_FAST_NOSPLIT") != nullptr;  // A/B aid: one launch at the widest pitch
    const unsigned all = (1u << g.nlevels) - 1u;
    // One launch per tile pitch.  The pitch of a launch is that of its widest cell (every ring offset an instruction
    // immediate), and with it the LDS per wave: an image size whose small levels need 64 bytes (512 x 512: cells of 44 and 47
    // pixels on levels 5 and 6, 25 of 490 cells) used to put EVERY cell at 64 - 19 waves per CU instead of 25.  Now the
    // levels that fit 48 bytes run at 48 and the few others in a launch of their own (the same stream: no ordering needed,
    // the cells write disjoint staging slots).
    unsigned mask48 = 0, mask64 = 0, maskAny = 0;
    for (int l = 0; l < g.nlevels; l++) {
        if (g.lv[l].nCols * g.lv[l].nRows <= 0) continue;
        const int need = g.lv[l].wCell + 9;
        (need <= 48 ? mask48 : need <= 64 ? mask64 : maskAny) |= 1u << l;
    }
    struct Part { unsigned mask; int TP; };
    Part parts[3];
    int nParts = 0;
    FtCellRanges probe;
    const bool splittable = !noSplit && !maskAny && mask48 && mask64 && fast_cell_ranges(g, mask48, probe) && fast_cell_ranges(g, mask64, probe);
    if (splittable) {
        parts[nParts++] = {mask48, 48};
        parts[nParts++] = {mask64, 64};
    } else {
        parts[nParts++] = {all, fast_tile_pitch(g)};
    }
    const int runBlock = 8 * FC_XCD_RUN;  // grid padded to whole rounds of the XCD mapping
    for (int pi = 0; pi < nParts; pi++) {
        const int TP = parts[pi].TP;
        FtCellRanges cr;
        if (nParts == 1 || !fast_cell_ranges(g, parts[pi].mask, cr)) {  // the unsplit launch: all cells, one run
            cr.lo0 = 0; cr.n0 = g.totalCells; cr.lo1 = 0; cr.n1 = 0;
        }
        const int nCells = cr.n0 + cr.n1;
        // LDS carve of the fixed-pitch variants: the largest tile and score plane of the launch's levels
        int tileBytes = 0, scoreBytes = 0;
        const size_t smem = fast_smem_of(g, parts[pi].mask, TP, &tileBytes, &scoreBytes);
        dim3 grid(((nCells + runBlock - 1) / runBlock) * runBlock, batch, 1), block(64, 1, 1);
        FtSlotGrid sg;
        sg.blocksPerSlot = 0; sg.batch = batch; sg.xcdMap = 0; sg.magic = 0;
        if (batch >= 8) sg = ft_slot_grid(nCells, batch, grid);  // image -> XCD; smaller launches keep the cell-run mapping
        const FastFn fn = TP == 48 ? (ordered ? k_fast_cells<48, true> : k_fast_cells<48, false>)
                          : TP == 64 ? (ordered ? k_fast_cells<64, true> : k_fast_cells<64, false>)
                                     : k_fast_cells<0, true>;  // any-size cells: the linear pass is ordered anyway
        if (smem > 64 * 1024)  // very wide cells (tiny images with one cell column): raise the dynamic LDS limit
            FT_HIP(hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
        if (occDbg) {
            int nb = 0;
            hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void *)fn, 64, smem);
            fprintf(stderr, "[ft] k_fast_cells<%d,%d>: %d cells per image, %zu B of LDS per wave, %d waves per CU\n", TP, ordered, nCells, smem, nb);
        }
        for (int rep = ft_debug_repeat("fast"); rep > 0; rep--)
            hipLaunchKernelGGL(fn, grid, block, smem, st, g, l0, l0pitch, pyr, iniTh, minTh, alignedLoads, cellCount, stage, cellTab, sg, dbg,
                               tileBytes, scoreBytes, cr);
    }
    FT_HIP(hipGetLastError());
    return FT_OK;
}

int ft_launch_compact(hipStream_t st, const FtGeom &g, int batch, const int *cellCount, const uint32_t *stage,
                      uint32_t *cand, int *candCount) {
    int maxCells = 0;
    for (int l = 0; l < g.nlevels; l++) maxCells = std::max(maxCells, g.lv[l].nCols * g.lv[l].nRows);
    dim3 grid2(g.nlevels, batch, 1), block(256, 1, 1);
    for (int rep = ft_debug_repeat("compact"); rep > 0; rep--)
    hipLaunchKernelGGL(k_compact, grid2, block, (size_t)(maxCells + 1) * sizeof(int), st, g, cellCount, stage, cand,
                       candCount);
    FT_HIP(hipGetLastError());
    return FT_OK;
}
