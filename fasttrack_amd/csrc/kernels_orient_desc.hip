// HIP kernels of the ORB extractor's orientation and descriptor step for gfx950 (CDNA4, wave64).  Results equal the reference's
// CPU branch:
//   k_orient_desc<KPW>   IC_Angle + 7x7 fixed-point blur + rBRIEF, KPW keypoints per wave
//                        (ORBextractor.cc:39-108, 478-493, 1456-1462)
//   k_blur_level         test tap: cv::GaussianBlur of a whole level through the same blur routines
// The blur is integer dot products on packed bytes (v_dot4 / v_dot2); the matrix-pipe and row-major forms that were measured
// against it are recorded in EXPERIMENTS.md 11.11 and 29.
#include "extract_dev.h"
#include "libm_f32.h"

namespace {

// umax of IC_Angle (ORBextractor.cc:478-493): 15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3

// IC_Angle with v_dot4_u32_u8: row v of the 31-px disc is eight dwords of four pixels, dword j holding
// u = -15 + 4j .. -12 + 4j.  W has u + 16 in the bytes inside the disc (|u| <= umax[|v|]), M has 1 there; both
// are 0 outside, so m10 = sum dot4(D, W) - 16 * dot4(D, M) and m01 = sum v * dot4(D, M).  Row 16 is all zero
// (padding of the 4 x 8-row walk).
struct FtMomentTab {
    unsigned W[17 * 8], M[17 * 8];
};
constexpr FtMomentTab ft_make_moment_tab() {
    constexpr int umax[16] = {15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3};
    FtMomentTab t{};
    for (int av = 0; av < 16; av++)
        for (int j = 0; j < 8; j++)
            for (int k = 0; k < 4; k++) {
                const int u = -15 + 4 * j + k;
                const int au = u < 0 ? -u : u;
                if (u <= 15 && au <= umax[av]) {
                    t.W[av * 8 + j] |= (unsigned)(u + 16) << (8 * k);
                    t.M[av * 8 + j] |= 1u << (8 * k);
                }
            }
    return t;
}
__constant__ FtMomentTab c_mom = ft_make_moment_tab();
// the rBRIEF pattern as floats: (x0, y0, x1, y1) per test
struct FtPatternF {
    float4 p[256];
};
constexpr FtPatternF ft_make_pattern_f() {
    constexpr signed char pat[1024] = {
#include "orb_pattern.inc"
    };
    FtPatternF t{};
    for (int i = 0; i < 256; i++) {
        t.p[i].x = (float)pat[4 * i];
        t.p[i].y = (float)pat[4 * i + 1];
        t.p[i].z = (float)pat[4 * i + 2];
        t.p[i].w = (float)pat[4 * i + 3];
    }
    return t;
}
__constant__ FtPatternF c_patternF = ft_make_pattern_f();
// GaussianBlur(7x7, sigma 2) fixed-point taps {18,34,48,56,48,34,18} (error-diffused, sum 256) are literals in k_orient_desc

// ------------------------------------------------------------------------------------------------
// Orientation + descriptor: one wave per retained keypoint, four keypoints per workgroup.
// The 43x43 unblurred patch (31-px disc for the moments, 37x37 sample window + 3-px blur halo) is
// staged in LDS with BORDER_REFLECT_101 at the level's edges; the 7x7 Gaussian is applied on the fly
// as two integer 7-tap passes in LDS, so no blurred pyramid is ever written to HBM.
// ------------------------------------------------------------------------------------------------
#define OD_R 21                 // patch radius: 18 (max rotated pattern offset) + 3 (blur)
#define OD_P (2 * OD_R + 1)     // 43
#define OD_PP 48                // raw pitch: 12 dwords cover the 43 bytes at any 4-byte phase
#define OD_HP 40                // columns of the horizontally blurred patch: raw byte positions 0..39
#ifndef OD_RP
#define OD_RP 44                // the blurred patch is kept column-major (the seven values of a sample are consecutive: two
#endif                          // ds_read2_b32 + three v_alignbit): u16 slots per column (43 rows + 1: dword-aligned columns)
#define OD_RAW_BYTES (OD_P * OD_PP)                  // 2064
#define OD_HB_BYTES (OD_HP * OD_RP * 2 + 16)         // 3536
#define OD_WAVE_BYTES ((OD_RAW_BYTES + OD_HB_BYTES + 15) & ~15)
#define OD_WAVES 4
#ifndef OD_KPW_WIDE
#define OD_KPW_WIDE 2           // keypoints per wave (1 or 2) in launches of 8+ images: loads of all of them in flight before the first is processed
#endif

__device__ __forceinline__ int reflect101(int i, int n) {
    if (i < 0) i = -i;
    if (i >= n) i = 2 * (n - 1) - i;
    return i;
}

// The 7x7 sigma-2 Gaussian of cv::GaussianBlur (8-bit fixed point, taps {18,34,48,56,48,34,18}) as the
// two routines k_orient_desc applies on the fly; k_blur_level (a test tap) runs the same two routines over a whole level.
// Horizontal: four consecutive outputs h[j] = sum_t k[t] * byte[j + t] (j = 0..3, t = 0..6) from three aligned dwords
// holding bytes 0..11.  The shifted windows of outputs 1 .. 3 are expressed through shifted WEIGHTS on the aligned
// dwords (ten v_dot4 with constant weight vectors) instead of byte-aligning the data first.
__device__ __forceinline__ void od_hblur4(unsigned d0, unsigned d1, unsigned d2, unsigned &h0, unsigned &h1, unsigned &h2, unsigned &h3) {
#define FT_W4(a, b, c, d) ((unsigned)(a) | ((unsigned)(b) << 8) | ((unsigned)(c) << 16) | ((unsigned)(d) << 24))
    const unsigned W0a = FT_W4(18, 34, 48, 56), W0b = FT_W4(48, 34, 18, 0);
    const unsigned W1a = FT_W4(0, 18, 34, 48), W1b = FT_W4(56, 48, 34, 18);
    const unsigned W2a = FT_W4(0, 0, 18, 34), W2b = FT_W4(48, 56, 48, 34), W2c = FT_W4(18, 0, 0, 0);
    const unsigned W3a = FT_W4(0, 0, 0, 18), W3b = FT_W4(34, 48, 56, 48), W3c = FT_W4(34, 18, 0, 0);
#undef FT_W4
    h0 = __builtin_amdgcn_udot4(d1, W0b, __builtin_amdgcn_udot4(d0, W0a, 0u, false), false);
    h1 = __builtin_amdgcn_udot4(d1, W1b, __builtin_amdgcn_udot4(d0, W1a, 0u, false), false);
    h2 = __builtin_amdgcn_udot4(d2, W2c, __builtin_amdgcn_udot4(d1, W2b, __builtin_amdgcn_udot4(d0, W2a, 0u, false), false), false);
    h3 = __builtin_amdgcn_udot4(d2, W3c, __builtin_amdgcn_udot4(d1, W3b, __builtin_amdgcn_udot4(d0, W3a, 0u, false), false), false);
}
// Vertical: blurred pixel = (sum_s k[s] * h[s] + 2^15) >> 16 from the seven horizontally blurred values of its column
// (each <= 255 * 256; the sums stay below 2^24).  The seven values of a column are consecutive u16: four dwords that
// hold them (starting at the dword that holds the first one; sh = 16 if the first value is that dword's high half, else 0)
// -> three v_alignbit + one shift put the pairs (t0,t1) (t2,t3) (t4,t5) (t6,-) into place, four v_dot2_u32_u16 weigh them.
typedef unsigned short od_us2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned od_dot2(unsigned a, unsigned w, unsigned acc) {
    return __builtin_amdgcn_udot2(__builtin_bit_cast(od_us2, a), __builtin_bit_cast(od_us2, w), acc, false);
}
__device__ __forceinline__ unsigned od_vblur7_pairs(unsigned e0, unsigned e1, unsigned e2, unsigned e3) {
    const unsigned W01 = 18u | (34u << 16), W23 = 48u | (56u << 16), W45 = 48u | (34u << 16), W6 = 18u;
    return od_dot2(e3, W6, od_dot2(e2, W45, od_dot2(e1, W23, od_dot2(e0, W01, 32768u)))) >> 16;
}
__device__ __forceinline__ unsigned od_vblur7_dwords(unsigned d0, unsigned d1, unsigned d2, unsigned d3, unsigned sh) {
    return od_vblur7_pairs(__builtin_amdgcn_alignbit(d1, d0, sh), __builtin_amdgcn_alignbit(d2, d1, sh),
                           __builtin_amdgcn_alignbit(d3, d2, sh), d3 >> (sh & 31u));  // (only the low five bits of sh count)
}

// Test tap (a7, GaussianBlur directly): the blurred image of one pyramid level, BORDER_REFLECT_101, computed with
// od_hblur4 / od_vblur7_dwords.  One thread per aligned group of four output pixels; speed is irrelevant here.
__global__ void k_blur_level(const uint8_t *img, int pitch, int w, int h, uint8_t *dst, int dstPitch) {
    const int gx = (blockIdx.x * blockDim.x + threadIdx.x) * 4, y = blockIdx.y;
    if (gx >= w || y >= h) return;
    unsigned hb[7][4];
    for (int s = 0; s < 7; s++) {
        const uint8_t *row = img + (size_t)reflect101(y + s - 3, h) * pitch;
        unsigned d[3] = {0u, 0u, 0u};
        for (int b = 0; b < 12; b++) d[b >> 2] |= (unsigned)row[reflect101(gx - 3 + b, w)] << (8 * (b & 3));
        od_hblur4(d[0], d[1], d[2], hb[s][0], hb[s][1], hb[s][2], hb[s][3]);
    }
    for (int j = 0; j < 4 && gx + j < w; j++) {
        // the column as k_orient_desc keeps it: consecutive u16, once starting in a low half and once in a high half
        const unsigned t[8] = {hb[0][j], hb[1][j], hb[2][j], hb[3][j], hb[4][j], hb[5][j], hb[6][j], 0u};
        unsigned v;
        if ((gx + j + y) & 1) v = od_vblur7_dwords(t[0] << 16, t[1] | (t[2] << 16), t[3] | (t[4] << 16), t[5] | (t[6] << 16), 16u);
        else v = od_vblur7_dwords(t[0] | (t[1] << 16), t[2] | (t[3] << 16), t[4] | (t[5] << 16), t[6], 0u);
        dst[(size_t)y * dstPitch + gx + j] = (uint8_t)v;
    }
}

__device__ __forceinline__ float fast_atan2_deg(float y, float x) {
    // cv::fastAtan2; every operation rounded separately (no FMA contraction)
    const float p1 = 0.9997878412794807f * (float)(180 / 3.14159265358979323846);
    const float p3 = -0.3258083974640975f * (float)(180 / 3.14159265358979323846);
    const float p5 = 0.1555786518463281f * (float)(180 / 3.14159265358979323846);
    const float p7 = -0.04432655554792128f * (float)(180 / 3.14159265358979323846);
    const float eps = (float)2.2204460492503131e-16;
    const float ax = fabsf(x), ay = fabsf(y);
    float a, c, c2;
    if (ax >= ay) {
        c = __fdiv_rn(ay, __fadd_rn(ax, eps));
        c2 = __fmul_rn(c, c);
        a = __fmul_rn(__fadd_rn(__fmul_rn(__fadd_rn(__fmul_rn(__fadd_rn(__fmul_rn(p7, c2), p5), c2), p3), c2), p1), c);
    } else {
        c = __fdiv_rn(ax, __fadd_rn(ay, eps));
        c2 = __fmul_rn(c, c);
        a = __fsub_rn(90.f, __fmul_rn(__fadd_rn(__fmul_rn(__fadd_rn(__fmul_rn(__fadd_rn(__fmul_rn(p7, c2), p5), c2), p3), c2), p1), c));
    }
    if (x < 0) a = __fsub_rn(180.f, a);
    if (y < 0) a = __fsub_rn(360.f, a);
    return a;
}

// FT_DEBUG_OD_PROFILE=1: where a wave of k_orient_desc spends its life - 100 MHz wall-clock stamps at the phase boundaries of
// wave 0 of every 16th workgroup, summed here ([0] = sampled waves, [1 + p] = ticks of phase p); the launcher prints them
__device__ unsigned long long g_odProf[16];
template <int OD_KPW>
__global__ __launch_bounds__(64 * OD_WAVES) void k_orient_desc(FtGeom g, const uint8_t *const *l0, int l0pitch,
                                                               const uint8_t *pyr, int alignedLoads, const FtSelKp *sel,
                                                               const int *selCount, FtOctArgs lay, int *nSel,
                                                               ft_keypoint *keysOut, uint8_t *descOut, FtSlotGrid sg, int prof) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    // the wave index is uniform by construction; as a scalar it makes the keypoint lookup below (level search, entry
    // address, level geometry, image pointer, row addressing) SALU work instead of 64 identical VALU lanes
    const int wave = wave_index();
    int slot, blk;
    if (!ft_slot_block(sg, slot, blk)) return;
    const bool profW = prof && wave == 0 && (blockIdx.x & 15u) == 0;
    unsigned long long tPrev = profW ? wall_clock64() : 0;
    int profIdx = 0;
    auto tick = [&]() {
        if (!profW) return;
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // the phase's memory operations belong to it
        const unsigned long long t = wall_clock64();
        if (lane == 0) atomicAdd(&g_odProf[1 + profIdx], t - tPrev);
        profIdx++;
        tPrev = t;
    };
    // OD_KPW keypoints per wave, one after the other through the same LDS buffers - with the LOADS of all of them issued up
    // front: level lookup, selection entries, image pointers and the nine patch dwords per lane of every keypoint are
    // requested before the first one is processed, so the dependent chain selCount -> sel entry -> image pointer -> patch
    // (three to four memory round trips) is paid once per OD_KPW keypoints and the later patches arrive behind the
    // arithmetic of the earlier ones (SQ counters of round 2: the waves of this kernel waited 42 % of their time, 26 % active).
    // Only the loaded dwords are kept (9 registers per extra keypoint) - no tables are hoisted across keypoints, which is what
    // cost the four-keypoints-per-wave variant of round 2 its occupancy.
    const int kFirst = (blk * OD_WAVES + wave) * OD_KPW;
    // the octree leaves its result per level; keypoint k of the image (level order) is entry k - prefix of
    // the level that contains it
    // Lane l holds the count of level l (one vector load), a DPP scan over the row of 16 lanes turns the counts into
    // inclusive prefixes, and the level of keypoint k is the first lane whose prefix exceeds k (one ballot): a dozen
    // instructions where the scalar unit used to walk the FT_MAX_LEVELS levels one by one (150 scalar instructions per wave -
    // and the CU's four SIMDs share one scalar unit).
    int total = 0;
    const int cnt = lane < g.nlevels ? selCount[slot * g.nlevels + lane] : 0;
    int incl = cnt;
    incl += __builtin_amdgcn_update_dpp(0, incl, 0x111, 0xF, 0xF, true);  // row_shr:1 (lanes shifted in from outside the row read 0)
    incl += __builtin_amdgcn_update_dpp(0, incl, 0x112, 0xF, 0xF, true);  // row_shr:2
    incl += __builtin_amdgcn_update_dpp(0, incl, 0x114, 0xF, 0xF, true);  // row_shr:4
    incl += __builtin_amdgcn_update_dpp(0, incl, 0x118, 0xF, 0xF, true);  // row_shr:8
    total = __builtin_amdgcn_readlane(incl, 15);
    if (kFirst == 0 && lane == 0) nSel[slot] = total;
    if (kFirst >= total) return;  // waves are independent: no workgroup barrier below
    const int nKp = min(OD_KPW, total - kFirst);
    uint8_t *raw = smem + (size_t)wave * OD_WAVE_BYTES;
    unsigned short *hb = (unsigned short *)(raw + OD_RAW_BYTES);
    // per keypoint of the wave: the selection entry and what the patch load needs (all wave-uniform)
    FtSelKp sk[OD_KPW];
    const uint8_t *imgK[OD_KPW];
    int pitchK[OD_KPW];
    bool interiorK[OD_KPW];
    unsigned pv[OD_KPW][9];
    const int rrL = (lane * 43) >> 9, ccL = lane - rrL * 12;  // lane / 12 for lane < 64
#pragma unroll
    for (int q = 0; q < OD_KPW; q++) {
        const int kk = min(kFirst + q, total - 1);  // (a keypoint beyond the last repeats it; its loads are harmless, it is not processed)
        const unsigned below = (unsigned)__builtin_amdgcn_ballot_w64(kk < incl) & 0xffffu;
        const int selLevel = __builtin_ctz(below | 0x8000u);
        const int prefix = __builtin_amdgcn_readlane(incl - cnt, selLevel);
        sk[q] = sel[(size_t)slot * g.maxKp + lay.selOff[selLevel] + (kk - prefix)];
    }
#pragma unroll
    for (int q = 0; q < OD_KPW; q++) {
        const int level = sk[q].level;
        imgK[q] = level_ptr(g, level, slot, l0, l0pitch, pyr, pitchK[q]);
        const int px0 = sk[q].x - OD_R, py0 = sk[q].y - OD_R;
        const int axq = px0 & 3;
        interiorK[q] = alignedLoads && px0 >= 0 && py0 >= 0 && py0 + OD_P <= g.lv[level].h && (px0 - axq) + OD_PP <= g.lv[level].w;
        if (interiorK[q] && lane < 60) {
            // 43 rows x 12 aligned dwords: coalesced 4-byte lanes, pixel (r, c) lands at raw[r*48 + ax + c].  Five rows
            // per step on lanes 0-59 with a fixed (row, dword) per lane, so a step is one load and one LDS store with
            // immediate offsets; all nine row groups are requested before the first LDS store
            const uint8_t *src = imgK[q] + (size_t)py0 * pitchK[q] + (px0 - axq);
            const unsigned laneOff = (unsigned)(rrL * pitchK[q] + 4 * ccL);
#pragma unroll
            for (int it = 0; it < 9; it++)
                pv[q][it] = (it < 8 || rrL < 3) ? gload<unsigned>(src + (laneOff + (unsigned)(it * 5 * pitchK[q]))) : 0u;  // scalar base + 32-bit lane offset
        }
    }
    // The keypoints of the wave go through the LDS buffers one after the other, but the wave-uniform arithmetic between the
    // moments and the samples - fastAtan2, the angle in radians, sin / cos in double: a fifth of the kernel's vector
    // instructions, all 64 lanes computing the same number - is done ONCE for both: keypoint 0's moments on lanes 0-31,
    // keypoint 1's on lanes 32-63.  Order: raw 0 -> moments 0 -> hblur 0 | raw 1 (the raw buffer is free again) -> moments 1 |
    // angles of both | samples 0 (hb 0) | hblur 1 -> samples 1.
    int axK[OD_KPW], m10K[OD_KPW], m01K[OD_KPW];
    auto stage = [&](const int q) {
        const FtSelKp s = sk[q];
        const int level = s.level;
        const int pitch = pitchK[q];
        const uint8_t *img = imgK[q];
        const int w = g.lv[level].w, h = g.lv[level].h;
        const int px0 = s.x - OD_R, py0 = s.y - OD_R;
        int ax = px0 & 3;
        if (interiorK[q]) {
            unsigned *rawLane = (unsigned *)raw + rrL * 12 + ccL;
            if (lane < 60) {
#pragma unroll
                for (int it = 0; it < 9; it++)
                    if (it < 8 || rrL < 3) rawLane[it * 60] = pv[q][it];
            }
        } else {
            // BORDER_REFLECT_101 of the blur at the level's edges (keypoints are >= 19 px inside, the
            // patch reaches 21) or unaligned caller frames
            ax = 0;
            for (int i = lane; i < OD_P * OD_P; i += 64) {
                const int r = i / OD_P, c = i - r * OD_P;
                const int gy = reflect101(py0 + r, h), gx = reflect101(px0 + c, w);
                raw[r * OD_PP + c] = gload<uint8_t>(img + (size_t)gy * pitch + gx);
            }
        }
        axK[q] = ax;
    };
    auto moments = [&](const int q) {
        const int ax = axK[q];
        // IC_Angle: integer moments over the 31-px disc, four pixels per v_dot4 (tables above): lane = (row of an
        // 8-row group, dword of the row), four groups cover rows v = -15 .. 16 (row 16 has zero weights)
        int m10 = 0, m01 = 0;
        {
            const int rsub = lane >> 3, jd = lane & 7;
            const int sh = (ax + 6) & 3;
            // dword j of row v starts at raw byte (v + 21) * 48 + ax + 6 + 4j
            const unsigned *w = (const unsigned *)raw + (rsub + 6) * 12 + ((ax + 6) >> 2) + jd;
            int v = rsub - 15;
#pragma unroll
            for (int it = 0; it < 4; it++) {
                const unsigned lo = w[it * 96], hi = w[it * 96 + 1];
                const unsigned D = __builtin_amdgcn_alignbyte(hi, lo, sh);
                const int av = v < 0 ? -v : v;
                const unsigned dw = __builtin_amdgcn_udot4(D, c_mom.W[av * 8 + jd], 0u, false);
                const unsigned dm = __builtin_amdgcn_udot4(D, c_mom.M[av * 8 + jd], 0u, false);
                m10 += (int)dw - 16 * (int)dm;
                m01 += __mul24(v, (int)dm);  // |v| <= 16, dm <= 4 * 255 * 15
                v += 8;
            }
            m10 = wave_sum_i32(m10);
            m01 = wave_sum_i32(m01);
        }
        m10K[q] = m10;
        m01K[q] = m01;
    };
    auto hblur = [&]() {
        // horizontal 7-tap pass on the packed bytes: a task = (row, aligned group of 4 raw byte positions);
        // two v_dot4_u32_u8 per output on byte windows cut out with v_alignbyte.  hb[r][b] = sum_t k[t] *
        // raw[r][b + t] for raw byte positions b in [0, 40) (16 bit, <= 255 * 256); output column c of the
        // blurred window is b = ax + c.
        {
            // column-major output (hbT[column][row], OD_RP u16 slots per column): a lane takes a PAIR of rows (2P, 2P + 1) of its
            // group of four columns and stores the two values of a column as one dword; six row pairs per step on lanes 0-59
            const int rr = (lane * 13) >> 7, gq = lane - rr * 10;  // lane / 10 for lane < 64
            const unsigned *rwLane = (const unsigned *)(raw + 2 * rr * OD_PP) + gq;
            unsigned *hbLane = (unsigned *)hb + 4 * gq * (OD_RP / 2) + rr;
            if (lane < 60) {
#pragma unroll
                for (int it = 0; it < 4; it++) {
                    if (it == 3 && rr > 3) break;  // row pairs 22, 23 do not exist (rows 0 .. 42; row 43 is a dummy)
                    const unsigned *rw = rwLane + it * (12 * OD_PP / 4);
                    unsigned a0, a1, a2, a3, b0, b1, b2, b3;
                    od_hblur4(rw[0], rw[1], rw[2], a0, a1, a2, a3);
                    od_hblur4(rw[OD_PP / 4], rw[OD_PP / 4 + 1], rw[OD_PP / 4 + 2], b0, b1, b2, b3);
                    unsigned *o = hbLane + it * 6;
                    o[0] = __builtin_amdgcn_perm(b0, a0, 0x05040100u);  // a | b << 16 (both < 2^16)
                    o[OD_RP / 2] = __builtin_amdgcn_perm(b1, a1, 0x05040100u);
                    o[2 * (OD_RP / 2)] = __builtin_amdgcn_perm(b2, a2, 0x05040100u);
                    o[3 * (OD_RP / 2)] = __builtin_amdgcn_perm(b3, a3, 0x05040100u);
                }
            }
        }
    };
    typedef float v2f __attribute__((ext_vector_type(2)));
    auto describe = [&](const int q, const float angle, const float ca, const float sb) {
        const int ax = axK[q];
        const int k = kFirst + q;
        const FtSelKp s = sk[q];
        const int cx = s.x, cy = s.y, level = s.level, response = s.response;
        // vertical 7-tap pass only where the pattern samples (512 of the 1369 window positions): the blurred
        // pixel at offset (r, c) from the keypoint is (sum_s k[s] * hb[18 + r + s][ax + 18 + c] + 2^15) >> 16.
        // The seven values of a sample are consecutive u16 of column ax + 18 + c starting at row 18 + r: byte
        // offset 2 * ((ax + 18 + c) * OD_RP + 18 + r) in the wave's hbT (one shift-add and one 24-bit multiply-add).
        // r and c arrive as the BIT PATTERNS of (offset + 1.5 * 2^23): adding that constant to a float rounds it to the
        // nearest integer, ties to even - cvRound - and leaves 0x4B400000 + offset in the register (|offset| < 2^22), one
        // instruction where v_rndne + v_cvt_i32 took two.  The constant parts come out in the wash: (r << 1) wraps to
        // 2 * offset + 2 * 0x4B400000, the 24-bit multiply sees 0x400000 + c, and both surpluses are folded into hbase.
        // (hbase carries the LDS address of hb itself, and the sample pointer is made from the integer: as smem + offset the
        // compiler adds the base of the dynamic LDS - zero, but a symbol to it - to every sample's address)
        typedef __attribute__((address_space(3))) const unsigned od_lds_u32;
        const int hbase = (int)(unsigned)(uintptr_t)(__attribute__((address_space(3))) uint8_t *)(uint8_t *)hb +
                          2 * ((ax + 18) * OD_RP + 18) - (int)(2u * 0x4B400000u + 0x400000u * (unsigned)(2 * OD_RP));
        auto blurred = [&](unsigned rBits, unsigned cBits) -> unsigned {
            const int byteIdx = vmad24((int)cBits, 2 * OD_RP, (int)((rBits << 1) + (unsigned)hbase));
            od_lds_u32 *p = (od_lds_u32 *)(uintptr_t)(unsigned)(byteIdx & ~3);
            // (bit shift of the window: 16 if the first value is a high half.  byteIdx is even, and both v_alignbit and the
            // shift take the low five bits of their operand: byteIdx << 3 serves without masking bit 1 out first)
            return od_vblur7_dwords(p[0], p[1], p[2], p[3], (unsigned)byteIdx << 3);
        };
        const v2f scPair = {sb, ca}, csPair = {ca, sb};
        unsigned long long words[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int p = q * 64 + lane;  // pair index: byte p/8, bit p%8
            const float4 pt = c_patternF.p[p];
            // (x, y) pairs times (sin, cos) and (cos, sin) pairs: packed fp32 multiplies, every product rounded on its own
            const v2f p0 = {pt.x, pt.y}, p1 = {pt.z, pt.w};
            const v2f a0 = p0 * scPair, b0 = p0 * csPair, a1 = p1 * scPair, b1 = p1 * csPair;
            const float rnd = 12582912.f;  // 1.5 * 2^23
            const unsigned r0 = __float_as_uint(__fadd_rn(__fadd_rn(a0.x, a0.y), rnd));  // cvRound(x0 sin + y0 cos), biased
            const unsigned c0 = __float_as_uint(__fadd_rn(__fsub_rn(b0.x, b0.y), rnd));  // cvRound(x0 cos - y0 sin), biased
            const unsigned r1 = __float_as_uint(__fadd_rn(__fadd_rn(a1.x, a1.y), rnd));
            const unsigned c1 = __float_as_uint(__fadd_rn(__fsub_rn(b1.x, b1.y), rnd));
            words[q] = __ballot(blurred(r0, c0) < blurred(r1, c1));
        }
        if (lane == 0) {
            const size_t o = (size_t)slot * g.maxKp + k;
            // ORBextractor.cc:1209-1221 (octave, size = int(PATCH_SIZE * sf)) and :1472-1475 (pt *= scale)
            const float scale = g.sf[level];
            ft_keypoint kp;
            kp.x = level ? __fmul_rn((float)cx, scale) : (float)cx;
            kp.y = level ? __fmul_rn((float)cy, scale) : (float)cy;
            kp.size = (float)(int)__fmul_rn((float)FT_PATCH_SIZE, scale);
            kp.angle = angle;
            kp.response = (float)response;
            kp.octave = level;
            kp.class_id = -1;
            keysOut[o] = kp;
            unsigned long long *d = (unsigned long long *)(descOut + o * 32);
            d[0] = words[0];
            d[1] = words[1];
            d[2] = words[2];
            d[3] = words[3];
        }
    };
    tick();  // 0: level lookup, selection entries, patch loads (all keypoints of the wave) have arrived
    stage(0);
    wave_lds_sync();
    tick();  // 1: patch 0 staged in LDS
    moments(0);
    tick();  // 2: moments 0
    hblur();
    wave_lds_sync();  // hb 0 is complete, the raw buffer is free
    tick();  // 3: horizontal blur 0
    if constexpr (OD_KPW > 1) {
        if (nKp > 1) {  // wave-uniform
            stage(1);
            wave_lds_sync();
            moments(1);
        }
    }
    tick();  // 4: patch 1 staged + its moments
    // lane group of keypoint q for the shared angle arithmetic: the halves of the wave
    constexpr int GROUP = 32;
    float mY = (float)m01K[0], mX = (float)m10K[0];
    if constexpr (OD_KPW > 1) {
        if (nKp > 1 && lane >= GROUP) {
            mY = (float)m01K[1];
            mX = (float)m10K[1];
        }
    }
    const float angleL = fast_atan2_deg(mY, mX);
    // computeOrbDescriptor (ORBextractor.cc:72-74): angle in radians as float, then std::cos(float) / std::sin(float)
    // = glibc's cosf / sinf, reproduced bit for bit (libm_f32.h)
    const float factorPI = (float)(3.14159265358979323846 / 180.f);
    const float ar = __fmul_rn(angleL, factorPI);
    const float caL = ft_libm::cosf_glibc(ar), sbL = ft_libm::sinf_glibc(ar);
    auto lane_value = [&](float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); };
    tick();  // 5: angles of all keypoints of the wave
    describe(0, lane_value(angleL, 0), lane_value(caL, 0), lane_value(sbL, 0));
    tick();  // 6: samples + stores of keypoint 0
    if constexpr (OD_KPW > 1) {
        if (nKp > 1) {
            wave_lds_sync();  // the samples in front have read hb (and patch 1 is staged)
            hblur();
            wave_lds_sync();
            tick();  // 7: horizontal blur 1
            describe(1, lane_value(angleL, GROUP), lane_value(caL, GROUP), lane_value(sbL, GROUP));
            tick();  // 8: samples + stores of keypoint 1
        }
    }
    if (profW && lane == 0) atomicAdd(&g_odProf[0], 1ull);
}

}  // namespace

int ft_launch_blur_level(hipStream_t st, const uint8_t *img, int pitch, int w, int h, uint8_t *dst, int dstPitch) {
    dim3 grid(((w + 3) / 4 + 63) / 64, h, 1), block(64, 1, 1);
    hipLaunchKernelGGL(k_blur_level, grid, block, 0, st, img, pitch, w, h, dst, dstPitch);
    FT_HIP(hipGetLastError());
    return FT_OK;
}

int ft_launch_orient_desc(hipStream_t st, const FtGeom &g, int batch, const uint8_t *const *l0, int l0pitch,
                          const uint8_t *pyr, int alignedLoads, const FtSelKp *sel, const int *selCount,
                          const FtOctArgs &layout, int *nSel, ft_keypoint *keys, uint8_t *desc) {
    dim3 grid, block(64 * OD_WAVES, 1, 1);
    // Launches that fill the chip (8+ images) give a wave several keypoints, which hides the load chains behind arithmetic;
    // a frame or two at a time (latency mode) leaves SIMDs idle as it is, and a wave that works through two keypoints one
    // after the other only doubles the time to the last result (stereo pair 752x480: 0.284 against 0.244 ms): one each.
    const int kpw = batch >= 8 ? OD_KPW_WIDE : 1;
    const FtSlotGrid sg = ft_slot_grid((g.maxKp + OD_WAVES * kpw - 1) / (OD_WAVES * kpw), batch, grid);
    const size_t smem = OD_WAVES * (size_t)OD_WAVE_BYTES;
    static const bool occDbg = ft_debug_env("FT_DEBUG_OCC") != nullptr;
    if (occDbg) {
        int nb = 0;
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kpw == 1 ? (const void *)k_orient_desc<1> : (const void *)k_orient_desc<OD_KPW_WIDE>,
                                                     64 * OD_WAVES, smem);
        fprintf(stderr, "[ft] k_orient_desc<%d>: %zu B of LDS per workgroup, %d workgroups per CU\n", kpw, smem, nb);
    }
    static const int prof = ft_debug_env("FT_DEBUG_OD_PROFILE") ? 1 : 0;
    for (int rep = ft_debug_repeat("orient"); rep > 0; rep--) {
        if (kpw == 1)
            hipLaunchKernelGGL(k_orient_desc<1>, grid, block, smem, st, g, l0, l0pitch, pyr, alignedLoads, sel, selCount, layout,
                               nSel, keys, desc, sg, 0);
        else
            hipLaunchKernelGGL(k_orient_desc<OD_KPW_WIDE>, grid, block, smem, st, g, l0, l0pitch, pyr, alignedLoads, sel, selCount,
                               layout, nSel, keys, desc, sg, prof);
    }
    if (prof && kpw > 1) {
        static int launches = 0;
        if (++launches % 64 == 0) {  // (synchronises: a debugging aid)
            unsigned long long h[16];
            if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_odProf), sizeof h) == hipSuccess && h[0]) {
                static const char *names[9] = {"loads (level, selection, patches)", "stage 0", "moments 0", "hblur 0", "stage 1 + moments 1",
                                               "angles", "samples 0 + stores", "hblur 1", "samples 1 + stores"};
                double tot = 0;
                for (int k = 0; k < 9; k++) tot += (double)h[1 + k];
                fprintf(stderr, "[ft] k_orient_desc<2> wave life, %llu sampled waves, %.2f us per wave:\n", h[0], tot / h[0] / 100.0);
                for (int k = 0; k < 9; k++) fprintf(stderr, "[ft]   %-36s %6.2f us  %5.1f %%\n", names[k], h[1 + k] / (double)h[0] / 100.0, 100.0 * h[1 + k] / tot);
            }
        }
    }
    FT_HIP(hipGetLastError());
    return FT_OK;
}
