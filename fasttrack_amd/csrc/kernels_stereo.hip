// HIP kernels of the rectified stereo matcher for gfx950 (wave64): 256-bit descriptors as 8 x v_bcnt in one chain, minima on
// packed (distance, index) keys so ties resolve exactly like the reference's sequential "dist < bestDist" scans.
//   k_stereo_rowsort  the row buckets vRowIndices  (reference src/Frame.cc:845-863), and the left keypoints by row
//   k_stereo_match    Frame::ComputeStereoMatches  (src/Frame.cc:835-989)
//   k_stereo_median   the 1.5*1.4*median SAD cut   (src/Frame.cc:991-1004)
// k_stereo_match reads the pyramid the extractor left in HBM: level_ptr is extract_dev.h's (the fourth reader of that layout).
// Host side: stereo_frontend.cpp.
#include "extract_dev.h"

namespace {

// ---- k_stereo_match: one workgroup per group of ST_G = 64 left keypoints taken in row order -----------------------------
// k_stereo_rowsort leaves the right keypoints bucketed by (int)y (`sorted`, `rowStart`) and the left keypoint indices
// ordered by (int)y (`leftOrder`; the ones outside [0, H) last).  Lane l of every wave of workgroup `grp` holds left keypoint
// leftOrder[64 * grp + l]: descriptor, row, level and the disparity window [minU, maxU] in registers.
//   reach / group arithmetic.  The band of right keypoint iR covers row `row` only if |y_R - row| < r + 1 with
//   r = 2 * sf[octave] <= 2 * sf[nlevels - 1], so with reach = ceil(2 * sf[nlevels - 1]) + 1 the buckets
//   [row - reach, row + reach] hold every candidate of the reference's vRowIndices[row].  For the group, rowLo / rowHi = the
//   smallest / largest row of its lanes that can match (row in [0, H), maxU >= 0), and
//   sorted[rowStart[max(rowLo - reach, 0)] .. rowStart[min(rowHi + reach + 1, H)]) is ONE contiguous range that holds every
//   candidate of every lane: ~120 entries for 64 keypoints of a 2 000-keypoint 720-row frame, where 64 separate scans of
//   ~60 entries read 3 800.  Each lane still applies its own exact band, octave and disparity tests to each candidate.
// Hamming phase: the range is staged in LDS ST_CHUNK entries at a time, one entry per thread, the row band of each entry
// (minr, maxr) computed once there; the four waves of the workgroup each walk a quarter of the chunk (candidates wave,
// wave + 4, ...) - every lane of a wave reads the same entry, a broadcast, the next entry read while this one is tested -
// and keep the running minimum of (dist << 16) | iR with the winner's x beside it; the four partial minima meet in LDS.
// The keys contain iR, so the minimum is the reference's first minimum in ascending iR whatever the order of the visits.
// (Wave w serving only keypoints 16 w .. 16 w + 15, four candidates at a time, needs 0.6 of the visits and was not faster:
// EXPERIMENTS 21.)
// SAD phase: after the combine all four waves hold the same keys, so the ballot of `bestDist < thOrbDist` IS the
// workgroup's match list - nothing is stored, no counter: wave w takes matches w, w + 4, ... of the ballot, the matched
// keypoint's data through v_readlane.  The image loads of a wave's next match are issued before the reduction of the
// current one.  Results go to the keypoint's own index; lanes without a match write -1.
#define ST_G 64
#define ST_CHUNK 256
static_assert(sizeof(FtSortedR) == 48 && offsetof(FtSortedR, desc) == 16, "k_stereo_match stages an entry as three uint4");

// two signed 16-bit values in a dword, and both clamped at once (v_pk_max_i16, v_pk_min_i16): v inside [lo, hi] in both halves
// if and only if the clamp returns v
typedef short st_i16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned st_pack16(int lo, int hi) { return ((unsigned)lo & 0xffffu) | ((unsigned)hi << 16); }
__device__ __forceinline__ unsigned st_clamp16x2(unsigned v, unsigned lo, unsigned hi) {
    const st_i16x2 c = __builtin_elementwise_min(__builtin_elementwise_max(__builtin_bit_cast(st_i16x2, v), __builtin_bit_cast(st_i16x2, lo)),
                                                 __builtin_bit_cast(st_i16x2, hi));
    return __builtin_bit_cast(unsigned, c);
}
// popcount(x) + acc as the one instruction it is: the eight words of a distance form one chain, no adds
__device__ __forceinline__ unsigned st_bcnt(unsigned x, unsigned acc) {
    unsigned r;
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(acc));
    return r;
}

// wave-uniform description of one SAD search (src/Frame.cc:921-986)
struct StSad {
    const uint8_t *imL, *imR;
    int pitchL, pitchR;
    int yl0, xl0, xr00;
    int iL, levelL, bestIdxR;
    float uL, scaleduR0;
    bool ok, packed;
};

__device__ __forceinline__ StSad st_sad_setup(const FtGeom &g, const FtStereoArgs &a, int slot, const uint8_t *const *l0L,
                                              const uint8_t *const *l0R, int l0pitchL, int l0pitchR, const uint8_t *pyrL,
                                              const uint8_t *pyrR, float uL, float vL, int levelL, float uR0, int iL, int bestIdxR) {
    StSad m;
    m.iL = iL;
    m.levelL = levelL;
    m.bestIdxR = bestIdxR;
    m.uL = uL;
    const float scaleFactor = g.invsf[levelL];
    const float scaleduL = roundf(__fmul_rn(uL, scaleFactor));
    const float scaledvL = roundf(__fmul_rn(vL, scaleFactor));
    const float scaleduR0 = roundf(__fmul_rn(uR0, scaleFactor));
    m.scaleduR0 = scaleduR0;
    const int w = 5, Ls = 5;
    m.imL = level_ptr(g, levelL, slot, l0L, l0pitchL, pyrL, m.pitchL);
    m.imR = level_ptr(g, levelL, slot, l0R, l0pitchR, pyrR, m.pitchR);
    const int lw = g.lv[levelL].w, lh = g.lv[levelL].h;
    const float iniu = __fsub_rn(__fadd_rn(scaleduR0, (float)Ls), (float)w);
    const float endu = __fadd_rn(__fadd_rn(__fadd_rn(scaleduR0, (float)Ls), (float)w), 1.0f);
    const int yl0 = (int)(scaledvL - w), xl0 = (int)(scaleduL - w), xr00 = (int)scaleduR0 - Ls - w;
    m.yl0 = yl0;
    m.xl0 = xl0;
    m.xr00 = xr00;
    bool ok = !(iniu < 0 || endu >= (float)lw);
    // windows that would leave the level make cv::Mat::rowRange/colRange throw in the reference;
    // unreachable for extractor keypoints (>= 19 px inside), guarded against stray reads
    ok = ok && yl0 >= 0 && yl0 + 2 * w + 1 <= lh && xl0 >= 0 && xl0 + 2 * w + 1 <= lw && xr00 >= 0 &&
         xr00 + 2 * (w + Ls) + 1 <= lw;
    m.ok = ok;
    // the aligned windows (16 bytes of a left row, 24 + 4 of a right row) stay inside the rows
    m.packed = ok && a.alignedLoads && (xl0 & ~3) + 16 <= lw && (xr00 & ~3) + 28 <= lw;
    return m;
}

// ---- SAD search on packed bytes (round 4).  The 11 x 11 left patch and the 11 x 21 right strip are fetched as
// aligned dwords - one load instruction per wave for each (44 and 66 dwords) where every lane used to issue 24
// byte loads - and parked in the wave's 476 bytes of LDS.  Then lane (shift group g = lane / 16, row r =
// lane % 16) takes row r at shift s = 4 k + g in round k = 0, 1, 2: the 11 bytes of the left row and of the
// shifted right row are three dwords each (v_alignbyte cuts them out, the twelfth byte is masked), three
// v_sad_u8 add up the row's absolute differences, four DPP adds inside the row of 16 lanes sum the 11 rows.
__device__ __forceinline__ void st_sad_issue(const StSad &m, int lane, unsigned &vL, unsigned &vR0, unsigned &vR1) {
    const int xl0a = m.xl0 & ~3, xr0a = m.xr00 & ~3;
    const int rl = lane >> 2, dl = lane & 3;  // lanes 0 .. 43
    vL = gload<unsigned>(m.imL + (unsigned)((m.yl0 + min(rl, 10)) * m.pitchL + xl0a + 4 * dl));  // (scalar base + 32-bit lane offset)
    const int rr0 = (lane * 43) >> 8, dr0 = lane - 6 * rr0;  // lane / 6 for lane < 64: rows 0 .. 10
    vR0 = gload<unsigned>(m.imR + (unsigned)((m.yl0 + rr0) * m.pitchR + xr0a + 4 * dr0));
    // dwords 64, 65 (row 10, dwords 4, 5) and the padding dword of every row: lanes 0 .. 12
    vR1 = gload<unsigned>(m.imR + (unsigned)((m.yl0 + (lane < 2 ? 10 : min(lane - 2, 10))) * m.pitchR + xr0a +
                                             (lane < 2 ? 4 * (4 + lane) : 24)));
}

__device__ __forceinline__ void st_sad_park(unsigned *ldsL, int lane, unsigned vL, unsigned vR0, unsigned vR1) {
    unsigned *ldsR = ldsL + 44;  // right rows at a pitch of 7 dwords (the last one: padding)
    const int rr0 = (lane * 43) >> 8, dr0 = lane - 6 * rr0;
    const int i1 = lane < 2 ? 64 + lane : 0;
    if (lane < 44) ldsL[lane] = vL;
    ldsR[rr0 * 7 + dr0] = vR0;
    if (lane < 2) ldsR[10 * 7 + (i1 - 60)] = vR1;
    else if (lane < 13) ldsR[(lane - 2) * 7 + 6] = vR1;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// the eleven SADs of a search (from the parked dwords, or for windows the aligned loads cannot serve from byte loads), the
// parabola through the best one and the three outputs of the match
__device__ __forceinline__ void st_sad_finish(const FtGeom &g, const FtStereoArgs &a, size_t base, const StSad &m, int lane,
                                              const unsigned *ldsL) {
    float outU = -1.0f, outD = -1.0f;
    int outSad = -1;
    const int Ls = 5;
    const float minD = 0.f;
    const float maxD = __fdiv_rn(a.mbf, a.mb);
    const int yl0 = m.yl0, xl0 = m.xl0, xr00 = m.xr00, pitchL = m.pitchL, pitchR = m.pitchR;
    if (m.ok) {
        int bestS = 0x7fffffff, bestinc = 0;
        float dists[11];
        if (m.packed) {
            const unsigned *ldsR = ldsL + 44;
            const int xl0a = xl0 & ~3, xr0a = xr00 & ~3;
            const int g4 = lane >> 4, r = lane & 15, rc = min(r, 10);
            const int offL = xl0 - xl0a, offR = xr00 - xr0a;
            const unsigned l0d = ldsL[rc * 4], l1d = ldsL[rc * 4 + 1], l2d = ldsL[rc * 4 + 2], l3d = ldsL[rc * 4 + 3];
            const unsigned Lw0 = __builtin_amdgcn_alignbyte(l1d, l0d, (unsigned)offL), Lw1 = __builtin_amdgcn_alignbyte(l2d, l1d, (unsigned)offL),
                           Lw2 = __builtin_amdgcn_alignbyte(l3d, l2d, (unsigned)offL) & 0x00ffffffu;
            unsigned sums[3];
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const int sft = min(4 * k + g4, 10);  // (shift 11 does not exist: the fourth group of the last round repeats shift 10)
                const int o = offR + sft;            // byte offset of the shifted row inside the aligned right row: 0 .. 13
                const unsigned *pr = ldsR + rc * 7 + (o >> 2);
                const unsigned r0 = pr[0], r1 = pr[1], r2 = pr[2], r3 = pr[3];
                const unsigned sh = (unsigned)(o & 3);
                const unsigned Rw0 = __builtin_amdgcn_alignbyte(r1, r0, sh), Rw1 = __builtin_amdgcn_alignbyte(r2, r1, sh),
                               Rw2 = __builtin_amdgcn_alignbyte(r3, r2, sh) & 0x00ffffffu;
                unsigned d = __builtin_amdgcn_sad_u8(Lw2, Rw2, __builtin_amdgcn_sad_u8(Lw1, Rw1, __builtin_amdgcn_sad_u8(Lw0, Rw0, 0u)));
                d = r < 11 ? d : 0u;
                // sum over the row of 16 lanes (every lane of the row ends up with it)
                d += (unsigned)__builtin_amdgcn_update_dpp(0, (int)d, 0xB1, 0xF, 0xF, true);   // quad_perm [1,0,3,2]
                d += (unsigned)__builtin_amdgcn_update_dpp(0, (int)d, 0x4E, 0xF, 0xF, true);   // quad_perm [2,3,0,1]
                d += (unsigned)__builtin_amdgcn_update_dpp(0, (int)d, 0x141, 0xF, 0xF, true);  // row_half_mirror
                d += (unsigned)__builtin_amdgcn_update_dpp(0, (int)d, 0x140, 0xF, 0xF, true);  // row_mirror
                sums[k] = d;
            }
#pragma unroll
            for (int sft = 0; sft < 11; sft++) {
                const int dS = __builtin_amdgcn_readlane((int)sums[sft >> 2], 16 * (sft & 3));
                dists[sft] = (float)dS;
                if (dS < bestS) {
                    bestS = dS;
                    bestinc = sft - Ls;
                }
            }
        } else {
            // 11x11 left patch: each lane owns pixels lane and lane+64 (< 121)
            const int p0 = lane, p1 = lane + 64;
            const int r0 = p0 / 11, c0 = p0 - r0 * 11, r1 = p1 / 11, c1 = p1 - r1 * 11;
            // every load of the SAD search is issued before the first reduction: the left patch and, per lane, the 11
            // consecutive right-image bytes its two pixels slide over (a wave used to pay the memory latency 11 times)
            const uint8_t *pl0 = m.imL + (size_t)(yl0 + r0) * pitchL + xl0 + c0;
            const uint8_t *pl1 = m.imL + (size_t)(yl0 + min(r1, 10)) * pitchL + xl0 + c1;
            const uint8_t *pr0 = m.imR + (size_t)(yl0 + r0) * pitchR + xr00 + c0;
            const uint8_t *pr1 = m.imR + (size_t)(yl0 + min(r1, 10)) * pitchR + xr00 + c1;
            // the lanes whose second pixel does not exist (p1 >= 121) carry 0 on both sides
            const bool two = p1 < 121;
            const unsigned a0 = gload<uint8_t>(pl0);
            const unsigned a1r = gload<uint8_t>(pl1);
            unsigned b0[11], b1[11];
#pragma unroll
            for (int s = 0; s < 11; s++) {
                b0[s] = gload<uint8_t>(pr0 + s);
                b1[s] = gload<uint8_t>(pr1 + s);
            }
            const unsigned a1 = two ? a1r : 0u;
#pragma unroll
            for (int s = 0; s < 11; s++) b1[s] = two ? b1[s] : 0u;
            // two shifts per register: v_sad_u8 adds |a - b| to the low half, v_sad_hi_u8 to the high half (a lane's two
            // pixels give at most 510, a wave's sum at most 121 * 255 < 2^16), so six wave sums serve the eleven shifts
#pragma unroll
            for (int s = 0; s < 11; s += 2) {
                unsigned d = __builtin_amdgcn_sad_u8(a1, b1[s], __builtin_amdgcn_sad_u8(a0, b0[s], 0u));
                if (s + 1 < 11) d = __builtin_amdgcn_sad_hi_u8(a1, b1[s + 1], __builtin_amdgcn_sad_hi_u8(a0, b0[s + 1], d));
                const unsigned sum = (unsigned)wave_sum_i32((int)d);
                const int dLo = (int)(sum & 0xffffu), dHi = (int)(sum >> 16);
                dists[s] = (float)dLo;
                if (dLo < bestS) {
                    bestS = dLo;
                    bestinc = s - Ls;
                }
                if (s + 1 < 11) {
                    dists[s + 1] = (float)dHi;
                    if (dHi < bestS) {
                        bestS = dHi;
                        bestinc = s + 1 - Ls;
                    }
                }
            }
        }
        if (!(bestinc == -Ls || bestinc == Ls)) {
            float dist1 = 0, dist2 = 0, dist3 = 0;
#pragma unroll
            for (int s = 1; s < 10; s++)
                if (s == bestinc + Ls) {
                    dist1 = dists[s - 1];
                    dist2 = dists[s];
                    dist3 = dists[s + 1];
                }
            const float den = __fmul_rn(2.0f, __fsub_rn(__fadd_rn(dist1, dist3), __fmul_rn(2.0f, dist2)));
            const float deltaR = __fdiv_rn(__fsub_rn(dist1, dist3), den);
            if (!(deltaR < -1 || deltaR > 1)) {
                float bestuR = __fmul_rn(g.sf[m.levelL], __fadd_rn(__fadd_rn(m.scaleduR0, (float)bestinc), deltaR));
                float disparity = __fsub_rn(m.uL, bestuR);
                if (disparity >= minD && disparity < maxD) {
                    if (disparity <= 0) {
                        disparity = 0.01f;
                        bestuR = (float)((double)m.uL - 0.01);
                    }
                    outD = __fdiv_rn(a.mbf, disparity);
                    outU = bestuR;
                    outSad = bestS;
                }
            }
        }
    }
    if (lane == 0) {
        a.uright[base + m.iL] = outU;
        a.depth[base + m.iL] = outD;
        a.sad[base + m.iL] = outSad;
        if (a.hamIdx) a.hamIdx[base + m.iL] = m.bestIdxR;
    }
}

__global__ __launch_bounds__(256) void k_stereo_match(FtGeom g, const uint8_t *const *l0L, const uint8_t *const *l0R,
                                                      int l0pitchL, int l0pitchR, const uint8_t *pyrL,
                                                      const uint8_t *pyrR, FtStereoArgs a, FtSlotGrid sg) {
    // a staged right keypoint: {x, minr | (octave - 1) << 16, maxr | (octave + 1) << 16, idx} and the descriptor as two more
    // uint4; four spare entries behind the chunk for the walk's read-ahead
    __shared__ uint4 cand[(ST_CHUNK + 4) * 3];
    __shared__ unsigned keyBuf[4][ST_G];
    __shared__ float xBuf[4][ST_G];
    __shared__ unsigned sadBuf[4][44 + 77 + 3];
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_index();
    int slot, grp;
    if (!ft_slot_block(sg, slot, grp)) return;
    const size_t base = (size_t)slot * a.capacity;
    const int nL = a.nL[slot];
    if (grp * ST_G >= nL) return;  // (the whole workgroup)
    const bool valid = grp * ST_G + lane < nL;  // lanes beyond nL repeat the last keypoint and take part in nothing
    const int iL = a.leftOrder[base + min(grp * ST_G + lane, nL - 1)];
    const ft_keypoint *kpL = a.keysL + base + iL;
    const float uL = kpL->x, vL = kpL->y;
    const int levelL = kpL->octave;
    unsigned dL[8];
    {
        const uint4 *p = (const uint4 *)(a.descL + (base + iL) * 32);
        const uint4 p0 = p[0], p1 = p[1];
        dL[0] = p0.x; dL[1] = p0.y; dL[2] = p0.z; dL[3] = p0.w;
        dL[4] = p1.x; dL[5] = p1.y; dL[6] = p1.z; dL[7] = p1.w;
    }
    const int nRows = g.lv[0].h;
    const int row = (int)vL;
    const float minZ = a.mb;
    const float minD = 0.f;
    const float maxD = __fdiv_rn(a.mbf, minZ);
    const float minU = __fsub_rn(uL, maxD);
    const float maxU = __fsub_rn(uL, minD);
    const bool active = valid && row >= 0 && row < nRows && !(maxU < 0);
    const unsigned rowLevel = st_pack16(row, levelL);  // (image sides stay below 4096: ft_pack_cand)
    unsigned best = 0xffffffffu;  // (dist << 16) | iR
    float bestX = 0.f;            // x of this lane's best right keypoint
    // all four waves hold the same 64 keypoints: everything wave-uniform below is workgroup-uniform too
    const unsigned rowLo = wave_min_u32(active ? (unsigned)row : 0xffffffffu);
    if (rowLo != 0xffffffffu) {
        const unsigned rowHi = ~wave_min_u32(active ? ~(unsigned)row : 0xffffffffu);
        const int reach = (int)ceilf(2.0f * g.sf[g.nlevels - 1]) + 1;
        const int *rs = a.rowStart + (size_t)slot * a.rowStride;
        const int t0 = rs[max((int)rowLo - reach, 0)], t1 = rs[min((int)rowHi + reach + 1, nRows)];
        const FtSortedR *srt = a.sorted + base;
        for (int c0 = t0; c0 < t1; c0 += ST_CHUNK) {
            const int n = min(ST_CHUNK, t1 - c0);
            if (tid < n) {
                const uint4 *e = (const uint4 *)(srt + c0 + tid);  // consecutive threads read consecutive 48-byte entries
                const uint4 kpR = e[0];                            // x, y, octave, idx
                // row band of the right keypoint (Frame.cc:852-862): rows floor(y-r) .. ceil(y+r), r = 2*sf[octave]
                const float yR = __uint_as_float(kpR.y), r = __fmul_rn(2.0f, g.sf[(int)kpR.z]);
                const int maxr = (int)ceilf(__fadd_rn(yR, r));
                const int minr = (int)floorf(__fsub_rn(yR, r));
                cand[3 * tid] = make_uint4(kpR.x, st_pack16(minr, (int)kpR.z - 1), st_pack16(maxr, (int)kpR.z + 1), kpR.w);
                cand[3 * tid + 1] = e[1];
                cand[3 * tid + 2] = e[2];
            }
            __syncthreads();
            // one candidate against the 64 keypoints of the wave
            auto visit = [&](const uint4 &h, const uint4 &d0, const uint4 &d1) {
                const float uR = __uint_as_float(h.x);
                // row inside [minr, maxr] and level inside [octave - 1, octave + 1]: one clamp of the packed pair
                if (active && st_clamp16x2(rowLevel, h.y, h.z) == rowLevel && uR >= minU && uR <= maxU) {
                    unsigned dist = st_bcnt(d0.x ^ dL[0], 0u);
                    dist = st_bcnt(d0.y ^ dL[1], dist);
                    dist = st_bcnt(d0.z ^ dL[2], dist);
                    dist = st_bcnt(d0.w ^ dL[3], dist);
                    dist = st_bcnt(d1.x ^ dL[4], dist);
                    dist = st_bcnt(d1.y ^ dL[5], dist);
                    dist = st_bcnt(d1.z ^ dL[6], dist);
                    dist = st_bcnt(d1.w ^ dL[7], dist);
                    const unsigned key = (dist << 16) | h.w;
                    if (key < best) {
                        best = key;
                        bestX = uR;
                    }
                }
            };
            // the next candidate's entry is on its way while this one is tested: two register sets taking turns (the last
            // read goes past the chunk, into the four spare entries: never used)
            uint4 hA = cand[3 * wave], d0A = cand[3 * wave + 1], d1A = cand[3 * wave + 2];
            for (int j = wave; j < n; j += 8) {
                const uint4 hB = cand[3 * (j + 4)], d0B = cand[3 * (j + 4) + 1], d1B = cand[3 * (j + 4) + 2];
                visit(hA, d0A, d1A);
                if (j + 4 >= n) break;
                hA = cand[3 * (j + 8)];
                d0A = cand[3 * (j + 8) + 1];
                d1A = cand[3 * (j + 8) + 2];
                visit(hB, d0B, d1B);
            }
            __syncthreads();
        }
    }
    keyBuf[wave][lane] = best;
    xBuf[wave][lane] = bestX;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < 4; w++) {
        const unsigned k = keyBuf[w][lane];  // (keys are unique: they contain the index)
        if (k < best) {
            best = k;
            bestX = xBuf[w][lane];
        }
    }
    const int thOrbDist = (FT_TH_HIGH + FT_TH_LOW) / 2;
    // bestDist starts at TH_HIGH in the reference, so only dist < TH_HIGH ever registers; < thOrbDist is stricter
    const bool matched = valid && best != 0xffffffffu && (int)(best >> 16) < thOrbDist;
    unsigned long long mm = __ballot(matched);  // the same in all four waves
    if (wave == 0 && valid && !matched) {
        a.uright[base + iL] = -1.0f;
        a.depth[base + iL] = -1.0f;
        a.sad[base + iL] = -1;
        if (a.hamIdx) a.hamIdx[base + iL] = -1;
    }
    auto setup = [&](unsigned long long m) {
        const int ml = (int)__ffsll((long long)m) - 1;  // (scalar)
        const unsigned key = (unsigned)__builtin_amdgcn_readlane((int)best, ml);
        return st_sad_setup(g, a, slot, l0L, l0R, l0pitchL, l0pitchR, pyrL, pyrR, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(uL), ml)),
                            __int_as_float(__builtin_amdgcn_readlane(__float_as_int(vL), ml)), __builtin_amdgcn_readlane(levelL, ml),
                            __int_as_float(__builtin_amdgcn_readlane(__float_as_int(bestX), ml)), __builtin_amdgcn_readlane(iL, ml),
                            (int)(key & 0xffffu));
    };
    for (int k = 0; k < wave; k++) mm &= mm - 1;  // this wave's first match
    if (mm == 0) return;
    unsigned *ldsL = sadBuf[wave];
    StSad cur = setup(mm);
    unsigned pL = 0, pR0 = 0, pR1 = 0;
    if (cur.packed) st_sad_issue(cur, lane, pL, pR0, pR1);
    for (;;) {
        for (int k = 0; k < 4; k++) mm &= mm - 1;  // ... and its next one
        if (cur.packed) st_sad_park(ldsL, lane, pL, pR0, pR1);
        const bool more = mm != 0;
        StSad nxt = cur;
        if (more) {
            nxt = setup(mm);
            if (nxt.packed) st_sad_issue(nxt, lane, pL, pR0, pR1);
        }
        st_sad_finish(g, a, base, cur, lane, ldsL);
        if (!more) break;
        cur = nxt;
        // the reads of this search come before the next one's parking
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

// Counting sort of both sides of one pair by (int)y.  Right keypoints: rowStart[r] .. rowStart[r+1] index `sorted`;
// keypoints outside [0, H) (cannot come from the extractor) are dropped, as the reference's unchecked vRowIndices access
// would be out of bounds for them.  Left keypoints: leftOrder[0 .. nL) holds their indices by (int)y, the ones outside
// [0, H) in one extra bucket at the end (k_stereo_match still owes them their -1 outputs); the order inside a bucket is
// whatever the atomics give, results are written to the keypoint's own index.
// The two histograms lie behind one another - counters [0, H] of the right side (the last one stays 0), [H + 1, 2 H + 1] of
// the left - and ONE scan serves both: the left cursors start at the number of right keypoints sorted, which is what the
// scan leaves in counter H.
__global__ __launch_bounds__(256) void k_stereo_rowsort(FtGeom g, FtStereoArgs a) {
    extern __shared__ __attribute__((aligned(16))) int sh[];  // 2 * (H + 1) counters
    __shared__ int wsum[4];
    const int slot = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int H = g.lv[0].h, nB = 2 * (H + 1);
    const int nR = a.nR[slot], nL = a.nL[slot];
    const size_t base = (size_t)slot * a.capacity;
    int *shL = sh + H + 1;
    for (int i = tid; i < nB; i += 256) sh[i] = 0;
    __syncthreads();
    for (int i = tid; i < nR; i += 256) {
        const int y = (int)a.keysR[base + i].y;
        if (y >= 0 && y < H) atomicAdd(&sh[y], 1);
    }
    for (int i = tid; i < nL; i += 256) {
        const int y = (int)a.keysL[base + i].y;
        atomicAdd(&shL[y >= 0 && y < H ? y : H], 1);
    }
    __syncthreads();
    // exclusive scan of sh[0..nB): each thread owns a contiguous chunk
    const int per = (nB + 255) / 256;
    const int c0 = min(tid * per, nB), c1 = min(c0 + per, nB);
    int local = 0;
    for (int c = c0; c < c1; c++) local += sh[c];
    int incl = local;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o);
        if (lane >= o) incl += t;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int wbase = 0;
    for (int w = 0; w < wave; w++) wbase += wsum[w];
    int run = wbase + incl - local;
    int *rs = a.rowStart + (size_t)slot * a.rowStride;
    for (int c = c0; c < c1; c++) {
        const int n = sh[c];
        if (c <= H) rs[c] = run;  // (rs[H]: the end of the last row)
        sh[c] = run;              // becomes the scatter cursor
        run += n;
    }
    __syncthreads();
    const int sortedR = sh[H];  // no scatter below moves this counter
    FtSortedR *srt = a.sorted + base;
    for (int i = tid; i < nR; i += 256) {
        const ft_keypoint kp = a.keysR[base + i];
        const int y = (int)kp.y;
        if (y >= 0 && y < H) {
            FtSortedR e;
            e.x = kp.x;
            e.y = kp.y;
            e.octave = kp.octave;
            e.idx = i;
            const unsigned long long *d = (const unsigned long long *)(a.descR + (base + i) * 32);
            e.desc[0] = d[0]; e.desc[1] = d[1]; e.desc[2] = d[2]; e.desc[3] = d[3];
            srt[atomicAdd(&sh[y], 1)] = e;
        }
    }
    int *lo = a.leftOrder + base;
    for (int i = tid; i < nL; i += 256) {
        const int y = (int)a.keysL[base + i].y;
        lo[atomicAdd(&shL[y >= 0 && y < H ? y : H], 1) - sortedR] = i;
    }
}

// One WAVE per pair (no barriers, no atomics): the accepted SADs are pulled into registers once, the
// median (element size/2 of the sorted list) is found by a bitwise search on the value with ballot-free
// wave sums, then every match with SAD >= 1.5f*1.4f*median is dropped (src/Frame.cc:991-1004).
#define SM_PER_LANE 40  // 64 * 40 = 2560 left keypoints per pair; larger inputs take the looped path
__global__ __launch_bounds__(64) void k_stereo_median(FtStereoArgs a) {
    const int slot = blockIdx.x, lane = threadIdx.x;
    const int nL = a.nL[slot];
    const size_t base = (size_t)slot * a.capacity;
    const bool inRegs = nL <= 64 * SM_PER_LANE;
    int v[SM_PER_LANE];
    int m = 0;
    if (inRegs) {
#pragma unroll
        for (int k = 0; k < SM_PER_LANE; k++) {
            const int i = k * 64 + lane;
            v[k] = i < nL ? a.sad[base + i] : -1;
            m += v[k] >= 0 ? 1 : 0;
        }
    } else {
        for (int i = lane; i < nL; i += 64) m += a.sad[base + i] >= 0 ? 1 : 0;
    }
    const int total = wave_sum_i32(m);
    if (total == 0 || !a.applyMedianCut) {
        if (lane == 0) a.nMatches[slot] = total;
        return;
    }
    const int k = total / 2;  // 0-based rank in ascending order
    // smallest value with count(sad <= value) >= k + 1; SAD <= 121*255 < 2^15
    int lo = 0;
    for (int bit = 14; bit >= 0; bit--) {
        const int probe = lo + (1 << bit) - 1;  // is the answer <= probe ?
        int c = 0;
        if (inRegs) {
#pragma unroll
            for (int q = 0; q < SM_PER_LANE; q++) c += (v[q] >= 0 && v[q] <= probe) ? 1 : 0;
        } else {
            for (int i = lane; i < nL; i += 64) {
                const int s = a.sad[base + i];
                c += (s >= 0 && s <= probe) ? 1 : 0;
            }
        }
        if (wave_sum_i32(c) < k + 1) lo += 1 << bit;
    }
    const float median = (float)lo;
    const float thDist = __fmul_rn(1.5f * 1.4f, median);
    int removed = 0;
    for (int i = lane; i < nL; i += 64) {
        const int s = a.sad[base + i];
        if (s >= 0 && !((float)s < thDist)) {
            a.uright[base + i] = -1.f;
            a.depth[base + i] = -1.f;
            a.sad[base + i] = -1;
            removed++;
        }
    }
    removed = wave_sum_i32(removed);
    if (lane == 0) a.nMatches[slot] = total - removed;
}

}  // namespace

int ft_launch_stereo_rowsort(hipStream_t st, const FtGeom &g, int batch, const FtStereoArgs &a) {
    for (int rep = ft_debug_repeat("rowsort"); rep > 0; rep--)
    hipLaunchKernelGGL(k_stereo_rowsort, dim3(batch), dim3(256), (size_t)2 * (g.lv[0].h + 1) * sizeof(int), st, g, a);
    FT_HIP(hipGetLastError());
    return FT_OK;
}

int ft_launch_stereo_match(hipStream_t st, const FtGeom &g, int batch, const uint8_t *const *l0L,
                           const uint8_t *const *l0R, int l0pitchL, int l0pitchR, const uint8_t *pyrL,
                           const uint8_t *pyrR, const FtStereoArgs &a) {
    dim3 grid, block(256, 1, 1);
    const FtSlotGrid sg = ft_slot_grid((a.capacity + ST_G - 1) / ST_G, batch, grid);
    for (int rep = ft_debug_repeat("stereo"); rep > 0; rep--)
    hipLaunchKernelGGL(k_stereo_match, grid, block, 0, st, g, l0L, l0R, l0pitchL, l0pitchR, pyrL, pyrR, a, sg);
    FT_HIP(hipGetLastError());
    return FT_OK;
}

int ft_launch_stereo_median(hipStream_t st, int batch, const FtStereoArgs &a) {
    hipLaunchKernelGGL(k_stereo_median, dim3(batch), dim3(64), 0, st, a);
    FT_HIP(hipGetLastError());
    return FT_OK;
}
