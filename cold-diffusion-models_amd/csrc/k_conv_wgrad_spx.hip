#include "cdf_conv_sp.h"
#include "cdf_wgrad.h"

// weight gradient with both operands pre-split ([pixels][ld] bf16 hi / lo planes).  Block range, pixel walk, bias-gradient fold and pad
// zeroing are the family's (cdf_wgrad.h); the transposing fragment read is cdf_tr_frag (cdf_conv_sp.h).

template <int NS>
__device__ __forceinline__ void cdf_bf16x8_accum(float* acc8, const u32x4_v& h, const u32x4_v& l) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if constexpr (NS == 3) {
            acc8[2 * e] += __uint_as_float(h[e] << 16) + __uint_as_float(l[e] << 16);
            acc8[2 * e + 1] += __uint_as_float(h[e] & 0xFFFF0000u) + __uint_as_float(l[e] & 0xFFFF0000u);
        } else {
            acc8[2 * e] += __uint_as_float(h[e] << 16);
            acc8[2 * e + 1] += __uint_as_float(h[e] & 0xFFFF0000u);
        }
    }
}

// Tile TA (ca) x TB (cb), each 64 or 128; 4 waves as 2 x 2 of (TA/2) x (TB/2); BK = 32 pixels.
// The contraction index (pixels) is the SLOW index of both NHWC operands, so the LDS tiles stay pixel-major,
// [32 px][T + 32] bf16 per plane, written with ds_write_b128 exactly as loaded.  The MFMA fragment (8
// consecutive pixels of one channel per lane) comes out of two ds_read_b64_tr_b16 -- gfx950's transposing LDS
// read: the 16 lanes of a group hand in the addresses of a [4 px][16 ch] block (lane t: pixel t>>2, channels
// 4(t&3)..+3) and lane t receives channel t's 4 pixels.  Pitch T+32 puts the 4 pixel rows of a group 16 banks
// apart and the second group of the 32-lane pass 8 banks further: conflict-free.  (That is the 32 x 32 x 16 geometry; on 16 x 16 x 32 a lane
// holds 8 pixels of the 32-pixel chunk and the image is swizzled: cdf_px_off, cdf_conv_sp.h.)

template <int T>
struct SpxWgradSlot {                  // one operand's share of a thread's loads for a 32-pixel chunk
    static constexpr int VPR = T / 8;              // uint4 per pixel row
    static constexpr int PASS = 32 * VPR / 256;    // T/64
    static constexpr int PPP = 256 / VPR;          // pixels per pass
    static constexpr int PITCH = T + 32;
};

// MFMA shape of the K loops below, per kernel form (32 = v_mfma_f32_32x32x16_bf16, 16 = v_mfma_f32_16x16x32_bf16; cdf_conv_sp.h), chosen like
// cdf_halo_mfma (k_conv_halo.hip): a form is on 16 where that measured faster per launch and keeps its waves per SIMD, and has no instance of
// the other shape.  Schedule, staging, split ranges and stores are the same in both; a 32-pixel chunk is ONE K step of the 16 shape (4 MFMAs
// per 32 x 32 block and term) instead of two k16 steps of one, so the fragments of a whole chunk are live at once.
constexpr int cdf_wgrad_spx_mfma(int TA, int TB, bool STACK2, int NS) {
    // MI355X, B = 64, 16 against 32 per launch (profiles/wgrad_mfma_shape_ab.txt): the 128 x 128 tile in split precision +4.4 ... +5.8 % on the
    // seven 3 x 3 layers that reach it, and it is the only one that wins.  NS = 1: every tile within the parent's own spread (-0.6 ... +1.8 %).
    // The stacked tile: +0.3 %.  128 x 64: 126 -> 138 VGPRs, past the 128 of four waves per SIMD.  64 x 64: +2.4 ... +3.1 % alone, but 0.4 ... 0.9 %
    // slower at the step's own two launches (kernel trace).  64 x 128 unstacked: no 3 x 3 layer reaches it, not measured alone.
    return TA == 128 && TB == 128 && !STACK2 && NS == 3 ? 16 : 32;
}
constexpr int cdf_wgrad_row3_mfma(int TA, int TB, int NS) {
    // the tiles with one 32-channel block per wave along dY run two blocks per CU at <= 128 VGPRs; the whole-chunk fragments take them past that
    // (128 x 64: 128 -> 153, 64 x 128: 126 -> 144 in split precision, 128 x 64: 120 -> 134 in bf16), i.e. to one block per CU: they stay on 32
    if (TA == 128 && TB == 64) return 32;
    if (TA == 64 && TB == 128 && NS == 3) return 32;
    // 128 x 128: +9.3 ... +12.7 % per launch in split precision (deep layers most), +4.7 ... +10.0 % in bf16; 64 x 128 in bf16: +3.1 %
    return 16;
}

// STACK2 (TA = 128 with CA <= 64): a 64-channel A operand would fill only half of the 128 MFMA rows, so the tile takes
// TWO taps -- rows 0..63 = tap 2*blockIdx.y, rows 64..127 = tap 2*blockIdx.y + 1 (all-zero when past the last tap).  The B
// rows are shared: valid when every tap reads B at the same offset (plain convolutions; checked by the host).
template <int TA, int TB, bool STACK2 = false, int NS = 3, int MF = cdf_wgrad_spx_mfma(TA, TB, STACK2, NS)>
__global__ void __launch_bounds__(256, 2) conv_wgrad_spx_kernel(SpxWgradArgs a) {
    using SA = SpxWgradSlot<TA>;
    using SB = SpxWgradSlot<TB>;
    constexpr int BK = 32, MT = TA / 64, NT = TB / 64;
    constexpr int PLANE_A = BK * SA::PITCH, PLANE_B = BK * SB::PITCH;
    constexpr int STAGE = 2 * PLANE_A + 2 * PLANE_B;
    CDF_DYN_SMEM(smem_raw);
    unsigned short* smem = (unsigned short*)smem_raw;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const CdfWgradRange g = cdf_wgrad_range<BK, TB>(a, a.xcd_swizzle);
    const int tile_a = g.tile_a, tile_b = g.tile_b, m_lo = g.m_lo, m_hi = g.m_hi, niter = g.niter;
    const int tap = STACK2 ? 2 * g.tap : g.tap;
    const int dby = a.dby[tap], dbx = a.dbx[tap];
    // load slots: operand X, pass p: pixel (tid / VPR) + PPP p of the chunk, 16-byte channel column (tid % VPR) * 8
    static_assert(!STACK2 || TA == 128, "tap stacking fills a 128-row A tile with two 64-channel taps");
    const int a_half = STACK2 ? ((tid % SA::VPR) >> 3) : 0;                 // which of the two stacked taps this lane loads
    const int tap_l = tap + a_half;
    const bool tap_ok = tap_l < a.ntaps;
    const int day = a.day[tap_ok ? tap_l : tap], dax = a.dax[tap_ok ? tap_l : tap];
    const int ca = STACK2 ? ((tid % SA::VPR) & 7) * 8 : tile_a * TA + (tid % SA::VPR) * 8;
    const int cb = tile_b * TB + (tid % SB::VPR) * 8;
    const CdfPixelWalk<BK> walk(a);
    int qa[SA::PASS][3], qb[SB::PASS][3];
#pragma unroll
    for (int p = 0; p < SA::PASS; ++p) walk.decode(m_lo + tid / SA::VPR + SA::PPP * p, qa[p]);
#pragma unroll
    for (int p = 0; p < SB::PASS; ++p) walk.decode(m_lo + tid / SB::VPR + SB::PPP * p, qb[p]);
    const bool do_bsum = g.bsum(a);
    float bs_acc[SB::PASS][8];
#pragma unroll
    for (int p = 0; p < SB::PASS; ++p)
#pragma unroll
        for (int e = 0; e < 8; ++e) bs_acc[p][e] = 0.f;

    // Everything below is straight-line code on purpose, the (qx, qy, b) carry included (CdfPixelWalk::advance).
    u32x4_v rah[SA::PASS], ral[SA::PASS], rbh[SB::PASS], rbl[SB::PASS];   // (arrays of HIP uint4 structs would live in scratch)
    auto load_global = [&](int it) {
        const int m0 = m_lo + it * BK;
#pragma unroll
        for (int p = 0; p < SA::PASS; ++p) {
            // an operand row is zero when its own tap falls outside its image: the product then vanishes whatever
            // the other side holds (and the B rows stay intact for the fused bias gradient)
            const int m = m0 + tid / SA::VPR + SA::PPP * p;
            const unsigned ay = (unsigned)(qa[p][1] * a.sa + day), ax = (unsigned)(qa[p][0] * a.sa + dax);
            const bool ok = m < m_hi && ay < (unsigned)a.HA && ax < (unsigned)a.WA && ca < a.CA && tap_ok;
            const unsigned pix = ((unsigned)qa[p][2] * (unsigned)a.HA + ay) * (unsigned)a.WA + ax;
            const size_t off = (size_t)pix * (unsigned)a.lda + (unsigned)ca;
            rah[p] = *(const u32x4_v*)(ok ? a.a_hi + off : a.zero);
            if constexpr (NS == 3) ral[p] = *(const u32x4_v*)(ok ? a.a_lo + off : a.zero);
            walk.advance(qa[p]);
        }
#pragma unroll
        for (int p = 0; p < SB::PASS; ++p) {
            const int m = m0 + tid / SB::VPR + SB::PPP * p;
            const unsigned by = (unsigned)(qb[p][1] * a.sb + dby), bx = (unsigned)(qb[p][0] * a.sb + dbx);
            const bool ok = m < m_hi && by < (unsigned)a.HB && bx < (unsigned)a.WB && cb < a.CB;
            const unsigned pix = ((unsigned)qb[p][2] * (unsigned)a.HB + by) * (unsigned)a.WB + bx;
            const size_t off = (size_t)pix * (unsigned)a.ldb + (unsigned)cb;
            rbh[p] = *(const u32x4_v*)(ok ? a.b_hi + off : a.zero);
            if constexpr (NS == 3) rbl[p] = *(const u32x4_v*)(ok ? a.b_lo + off : a.zero);
            walk.advance(qb[p]);
        }
    };
    auto store_lds = [&](int buf) {
        unsigned short* st = smem + buf * STAGE;
#pragma unroll
        for (int p = 0; p < SA::PASS; ++p) {
            const int so = cdf_px_off<MF>(tid / SA::VPR + SA::PPP * p, (tid % SA::VPR) * 8, SA::PITCH);
            *(u32x4_v*)(st + so) = rah[p];
            if constexpr (NS == 3) *(u32x4_v*)(st + PLANE_A + so) = ral[p];
        }
#pragma unroll
        for (int p = 0; p < SB::PASS; ++p) {
            const int so = cdf_px_off<MF>(tid / SB::VPR + SB::PPP * p, (tid % SB::VPR) * 8, SB::PITCH);
            *(u32x4_v*)(st + 2 * PLANE_A + so) = rbh[p];
            if constexpr (NS == 3) *(u32x4_v*)(st + 2 * PLANE_A + PLANE_B + so) = rbl[p];
            if (do_bsum) cdf_bf16x8_accum<NS>(bs_acc[p], rbh[p], rbl[p]);     // here the loads have landed anyway
        }
    };

    typename cdf_acc_of<MF>::type acc[MT][NT];
    cdf_acc_zero(acc);

    const int half = lane >> 5, l31 = lane & 31;
    // transposing-read lane geometry.  MF = 32: group g = lane >> 4 -> channel block 16 (g & 1), pixel block 8 (g >> 1) of the k16 step.
    // MF = 16: group g -> pixel block 8 g of the chunk; the fragment index is the 16-channel half instead of the k16 step (rows 8 g + q and
    // 8 g + 4 + q share bit 3: one offset per half, the second read 4 pitches further)
    const int t16 = lane & 15, g16 = lane >> 4;
    const int tr_row = (MF == 16 ? g16 : g16 >> 1) * 8 + (t16 >> 2), tr_col = (MF == 16 ? 0 : (g16 & 1) * 16) + (t16 & 3) * 4;
    const int tra = cdf_px_off<MF>(tr_row, tr_col, SA::PITCH, wm * (TA / 2));
    const int trb = cdf_px_off<MF>(tr_row, tr_col, SB::PITCH, wn * (TB / 2));
    const int tra1 = cdf_px_off<MF>(tr_row, tr_col + 16, SA::PITCH, wm * (TA / 2));
    const int trb1 = cdf_px_off<MF>(tr_row, tr_col + 16, SB::PITCH, wn * (TB / 2));
    if (niter > 0) {
        load_global(0);
        store_lds(0);
    }
    __syncthreads();
    for (int it = 0; it < niter; ++it) {
        const int buf = it & 1;
        if (it + 1 < niter) load_global(it + 1);
        const unsigned short* sa = smem + buf * STAGE;
        const unsigned short* sb = sa + 2 * PLANE_A;
        if constexpr (MF == 16) {
            bf16x8_v ah[2][MT], al[2][MT], bh[2][NT], bl[2][NT];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
#pragma unroll
                for (int i = 0; i < MT; ++i) cdf_tr_frag<NS>(sa + (h ? tra1 : tra) + i * 32, PLANE_A, SA::PITCH, ah[h][i], al[h][i]);
#pragma unroll
                for (int j = 0; j < NT; ++j) cdf_tr_frag<NS>(sb + (h ? trb1 : trb) + j * 32, PLANE_B, SB::PITCH, bh[h][j], bl[h][j]);
            }
            cdf_mma_tile<NS, MT, NT>(acc, ah, al, bh, bl);
        } else {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                bf16x8_v ah[MT], al[MT], bh[NT], bl[NT];
#pragma unroll
                for (int i = 0; i < MT; ++i) {
                    cdf_tr_frag<NS>(sa + tra + ks * 16 * SA::PITCH + i * 32, PLANE_A, SA::PITCH, ah[i], al[i]);
                }
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    cdf_tr_frag<NS>(sb + trb + ks * 16 * SB::PITCH + j * 32, PLANE_B, SB::PITCH, bh[j], bl[j]);
                }
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int j = 0; j < NT; ++j) {
                        cdf_mma_sp<NS>(acc[i][j], ah[i], al[i], bh[j], bl[j]);
                    }
            }
        }
        if (it + 1 < niter) store_lds(buf ^ 1);
        __syncthreads();
    }

    float* red = (float*)smem_raw;
    if (do_bsum) {                                 // [32 px][TB] partial column sums -> one row
#pragma unroll
        for (int p = 0; p < SB::PASS; ++p)
#pragma unroll
            for (int e = 0; e < 8; ++e) red[(tid / SB::VPR + SB::PPP * p) * TB + (tid % SB::VPR) * 8 + e] = bs_acc[p][e];
        cdf_wgrad_bsum_fold<BK, TB, 256>(a, red, tile_b, g.split, tid);
        __syncthreads();
    }
    // accumulators -> LDS [TA][TB + 8] -> float4 rows of the split's partial-sum slab (see cdf_epilogue.h)
    constexpr int CP = TB + 8;
    cdf_acc_stage(red, CP, wm * (TA / 2), wn * (TB / 2), acc, half, l31);
    __syncthreads();
    float* O = cdf_wgrad_slab(a, g.split, tap);
    constexpr int TPR = TB / 4, RPS = 256 / TPR;
    const int c4 = (tid % TPR) * 4, col = tile_b * TB + c4;
    if (col < a.ldo) {
        for (int r = tid / TPR; r < TA; r += RPS) {
            int row = tile_a * TA + r;
            if (STACK2) {                          // tile row r = (stacked tap r >> 6, channel r & 63): the next tap's slab follows
                if (tap + (r >> 6) >= a.ntaps || (r & 63) >= a.CA) continue;
                row = (r >> 6) * a.CA + (r & 63);
            } else if (row >= a.CA) break;
            float4 v = *(const float4*)(red + r * CP + c4);
            cdf_wgrad_zero_pad(v, col, a.CB);
            *(float4*)(O + (long long)row * a.ldo + col) = v;
        }
    }
}

// ================================================================================================
// Weight gradient of 3 x 3 stride-1 "same" convolutions, one block per ROW OF TAPS (dy fixed; dx = -1, 0, +1).
//
// conv_wgrad_spx_kernel gives every tap its own block, and each of the nine loads the same dY tile and a one-pixel-shifted
// X tile: like the forward GEMM it is bound by the bytes its waves have to push through the vector-memory
// path per MFMA.  Here a 32-pixel chunk (always inside one image row, or two rows of a 16-pixel-wide image) brings in dY ONCE
// and X ONCE with a pixel of halo on either side ([34 or 36 px][TA]), and the three dx taps read their X fragments from that
// tile at pixel offsets 0, 1, 2: a third of the loads (and of the per-chunk address arithmetic) per MFMA.  Pixel addresses are
// linear in the chunk index (no per-tap decode); the row / image borders are a per-lane mask.  8 waves (32 x TB/WB tiles, three
// accumulator sets), one block per CU; grid (tiles, 3 tap rows, splits) in the XCD-aware order of cdf_wgrad_block.
// Split range, bias fold and slab store are this kernel's own, kept on a measurement: see cdf_wgrad.h.
// ================================================================================================
template <int TA, int TB, int NS = 3, int MF = cdf_wgrad_row3_mfma(TA, TB, NS)>
__global__ void __launch_bounds__(512, 1) conv_wgrad_row3_kernel(SpxWgradArgs a) {
    constexpr int BK = 32, NTHR = 512;
    constexpr int WA_ = TA / 32, WB_ = 8 / WA_, TNW = TB / WB_, NT = TNW / 32;
    static_assert(NT >= 1 && NT * 32 == TNW, "wave tile along B must be a multiple of 32 channels");
    constexpr int NRAP = 36;                                   // halo rows: 34 (W >= 32) or 2 x 18 (W = 16)
    constexpr int PITCH_A = TA + 32, PITCH_B = TB + 32;
    constexpr int PLANE_A = NRAP * PITCH_A, PLANE_B = BK * PITCH_B;
    constexpr int STAGE = 2 * PLANE_A + 2 * PLANE_B;
    constexpr int VPR_A = TA / 8, RPP_A = NTHR / VPR_A, PASS_A = (NRAP + RPP_A - 1) / RPP_A;
    constexpr int VPR_B = TB / 8;                              // (512 / VPR_B >= 32 rows: one pass)
    CDF_DYN_SMEM(smem_raw);
    unsigned short* smem = (unsigned short*)smem_raw;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wa = wave / WB_, wb = wave % WB_;
    const int tiles_b = (a.CB + TB - 1) / TB;
    int bx, by, bz;
    cdf_wgrad_block(a.xcd_swizzle, bx, by, bz);
    const int tile_a = bx / tiles_b, tile_b = bx - tile_a * tiles_b;
    const int grp = by, split = bz;                            // tap row: taps 3 grp .. 3 grp + 2 share day
    const int W = a.QW, H = a.QH;
    const int M = a.B * H * W;
    const int m_lo = split * a.m_per_split;
    int m_hi = m_lo + a.m_per_split;
    if (m_hi > M) m_hi = M;
    const int niter = m_hi > m_lo ? (m_hi - m_lo) / BK : 0;    // (M and m_per_split are multiples of 32)
    const int dy = a.day[3 * grp];
    const int cw = W < 32 ? W : 32, rps = cw + 2;              // chunk row width, halo rows per image row
    const int nra = (32 / cw) * rps;

    // ---- load slots.  A: halo row r = (sub-row, xr): pixel (y + sub + dy, x0 + xr - 1); B: chunk pixel pb
    int a_r[PASS_A], a_sub[PASS_A], a_xr[PASS_A];
    const int ca = tile_a * TA + (tid % VPR_A) * 8;
#pragma unroll
    for (int p = 0; p < PASS_A; ++p) {
        a_r[p] = tid / VPR_A + RPP_A * p;
        a_sub[p] = a_r[p] / rps;
        a_xr[p] = a_r[p] - a_sub[p] * rps;
    }
    const int pb = tid / VPR_B;
    const int cb = tile_b * TB + (tid % VPR_B) * 8;
    const bool b_lane = pb < BK;
    // chunk position (wave-uniform): x0 = first pixel's column, yc = its image row
    int x0 = m_lo % W, yc = (m_lo / W) % H;
    const bool do_bsum = a.bsum != nullptr && tile_a == 0 && grp == 0;
    float bs_acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) bs_acc[e] = 0.f;

    // Register-staged operand chunks, TWO ahead of the one being multiplied (round 6; round 3 measured this form at +2.6 ... +10.5 % on the
    // 128 x 128-pixel layers and dropped it for +0.2 % of the step of its day): with one chunk ahead the loads had one chunk's MFMAs to
    // land -- 18 per wave for a 64-channel side, 0.25 us against ~1.5 us of HBM latency, and a third of that in `bf16` mode -- so the two
    // blocks of a CU spent most of their time waiting for each other's loads.  Set s holds chunk c with c % 2 == s; chunk it + 1 goes to
    // LDS between the two k-steps of chunk it, its registers are refilled with chunk it + 3 right behind, and the barrier orders LDS only.
    // (128 x 64 tiles in split precision: the second register set takes the kernel from 125 to 156 VGPRs, i.e. from two resident blocks per
    //  CU to one -- measured -2.5 % -- so that instantiation keeps ONE chunk ahead.)
    constexpr bool X2 = !(TA == 128 && TB == 64 && NS == 3);
    struct Regs {
        u32x4_v ah[PASS_A], al[PASS_A], bh, bl;
    };
    Regs r0, r1;
    auto load_global = [&](Regs& r, int it) {
        const int m0 = m_lo + it * BK;
#pragma unroll
        for (int p = 0; p < PASS_A; ++p) {
            const unsigned ax = (unsigned)(x0 + a_xr[p] - 1), ay = (unsigned)(yc + a_sub[p] + dy);
            const bool ok = a_r[p] < nra && ax < (unsigned)W && ay < (unsigned)H && ca < a.CA;
            const long long pix = (long long)m0 + (a_sub[p] + dy) * W + a_xr[p] - 1;
            const size_t off = (size_t)(ok ? pix : 0) * (unsigned)a.lda + (unsigned)ca;
            r.ah[p] = *(const u32x4_v*)(ok ? a.a_hi + off : a.zero);
            if constexpr (NS == 3) r.al[p] = *(const u32x4_v*)(ok ? a.a_lo + off : a.zero);
        }
        {
            const bool ok = b_lane && cb < a.CB;
            const size_t off = (size_t)(m0 + (b_lane ? pb : 0)) * (unsigned)a.ldb + (unsigned)cb;
            r.bh = *(const u32x4_v*)(ok ? a.b_hi + off : a.zero);
            if constexpr (NS == 3) r.bl = *(const u32x4_v*)(ok ? a.b_lo + off : a.zero);
        }
        // next chunk (uniform scalars, selects only): 32 pixels further -- inside the row, to the next row(s), to the next image
        const int nx = x0 + (W < 32 ? 0 : 32);
        const int wrap = nx >= W ? 1 : 0;
        x0 = wrap ? 0 : nx;
        yc += (W < 32 ? 32 / W : 0) + wrap;
        yc = yc >= H ? yc - H : yc;
    };
    auto store_lds = [&](const Regs& r, int buf) {
        unsigned short* st = smem + buf * STAGE;
#pragma unroll
        for (int p = 0; p < PASS_A; ++p) {
            if (a_r[p] < NRAP) {
                const int so = cdf_px_off<MF>(a_r[p], (tid % VPR_A) * 8, PITCH_A);
                *(u32x4_v*)(st + so) = r.ah[p];
                if constexpr (NS == 3) *(u32x4_v*)(st + PLANE_A + so) = r.al[p];
            }
        }
        if (b_lane) {
            const int so = cdf_px_off<MF>(pb, (tid % VPR_B) * 8, PITCH_B);
            *(u32x4_v*)(st + 2 * PLANE_A + so) = r.bh;
            if constexpr (NS == 3) *(u32x4_v*)(st + 2 * PLANE_A + PLANE_B + so) = r.bl;
            if (do_bsum) cdf_bf16x8_accum<NS>(bs_acc, r.bh, r.bl);
        }
    };

    typename cdf_acc_of<MF>::type acc[3][NT];
    cdf_acc_zero(acc);

    const int half = lane >> 5, l31 = lane & 31;
    // transposing-read lane geometry (see conv_wgrad_spx_kernel): MF = 32: pixels 8 (g >> 1) .. of the k16 step, channels 16 (g & 1) ..;
    // MF = 16: pixels 8 g .. of the chunk, and the fragment index is the 16-channel half
    const int t16 = lane & 15, g16 = lane >> 4;
    const int tr_row = (MF == 16 ? g16 : g16 >> 1) * 8 + (t16 >> 2), tr_col = (MF == 16 ? 0 : (g16 & 1) * 16) + (t16 & 3) * 4;
    const int trb = cdf_px_off<MF>(tr_row, tr_col, PITCH_B, wb * TNW);
    const int trb1 = cdf_px_off<MF>(tr_row, tr_col + 16, PITCH_B, wb * TNW);   // (MF = 16: rows tr_row and tr_row + 4 share bit 3)
    // halo row of chunk pixel p for tap dx: p + 1 + dx (+ 2 from the second image row of a 16-wide chunk on)
    // (MF = 32 only, whose image is plain: cdf_px_off<32> written out -- through the function the 128 x 64 tile compiles to 129 VGPRs instead of
    //  128 and loses its second block per CU; the MF = 16 offsets are tra16 below)
    int tra[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) tra[i] = (tr_row + 1 + (int)a.dax[3 * grp + i]) * PITCH_A + wa * 32 + tr_col;
    const int ks_skip = W < 32 ? 2 * PITCH_A : 0;              // k-step 1 = pixels 16..31 = the second row when W = 16

    auto mma_ks = [&](const unsigned short* sa, const unsigned short* sb, int ks) {
        if constexpr (MF == 32) {
            bf16x8_v bh[NT], bl[NT];
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                cdf_tr_frag<NS>(sb + trb + ks * 16 * PITCH_B + j * 32, PLANE_B, PITCH_B, bh[j], bl[j]);
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                bf16x8_v ah, al;
                cdf_tr_frag<NS>(sa + tra[i] + ks * (16 * PITCH_A + ks_skip), PLANE_A, PITCH_A, ah, al);
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    cdf_mma_sp<NS>(acc[i][j], ah, al, bh[j], bl[j]);
                }
            }
        }
    };
    // MF = 16: the chunk is one K step.  Groups 2 and 3 hold pixels 16 .. 31: the second image row when W = 16, two halo rows further on.  The X
    // rows of a fragment, r and r + 4 with r = pixel + 1 + dx (+ 2), can differ in bit 3: an offset of its own for each (tap, read, half).
    int tra16[3][2][2];
    if constexpr (MF == 16) {
        const int skip = (W < 32 && g16 >= 2) ? 2 : 0;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
                for (int h = 0; h < 2; ++h)
                    tra16[i][q][h] = cdf_px_off<MF>(tr_row + 4 * q + 1 + (int)a.dax[3 * grp + i] + skip, tr_col + 16 * h, PITCH_A, wa * 32);
    }
    // the dY fragments of the chunk, tap 0, `mid` (the staging traffic the two k16 steps of the 32 shape have between them), taps 1 and 2
    auto mma_chunk16 = [&](const unsigned short* sa, const unsigned short* sb, auto&& mid) {
        if constexpr (MF == 16) {
            bf16x8_v bh[2][NT], bl[2][NT];
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int j = 0; j < NT; ++j) cdf_tr_frag<NS>(sb + (h ? trb1 : trb) + j * 32, PLANE_B, PITCH_B, bh[h][j], bl[h][j]);
            auto tap = [&](int i) {
                bf16x8_v ah[2][1], al[2][1];
#pragma unroll
                for (int h = 0; h < 2; ++h) cdf_tr_frag2<NS>(sa + tra16[i][0][h], sa + tra16[i][1][h], PLANE_A, ah[h][0], al[h][0]);
                cdf_mma_tile<NS, 1, NT>(*reinterpret_cast<f32x4q_t(*)[1][NT]>(&acc[i]), ah, al, bh, bl);   // (tap i's row of blocks as a 1 x NT tile)
            };
            tap(0);
            mid();
            tap(1);
            tap(2);
        }
    };
    if constexpr (X2) {
        // one chunk: multiply chunk `it` (stage it & 1); `nxt` holds chunk it + 1 (-> the other stage, then refilled with chunk it + 3)
        auto step = [&](int it, Regs& nxt) {
            const unsigned short* sa = smem + (it & 1) * STAGE;
            const unsigned short* sb = sa + 2 * PLANE_A;
            auto mid = [&]() {
                if (it + 1 < niter) store_lds(nxt, (it + 1) & 1);    // (that stage was last read in chunk it - 1: every wave is past the barrier that ended it)
                if (it + 3 < niter) load_global(nxt, it + 3);
            };
            if constexpr (MF == 16) {
                mma_chunk16(sa, sb, mid);
            } else {
                mma_ks(sa, sb, 0);
                mid();
                mma_ks(sa, sb, 1);
            }
            CDF_LDS_BARRIER();                                   // (LDS traffic only: the chunks in flight stay in flight)
        };
        if (niter > 0) {
            load_global(r0, 0);
            store_lds(r0, 0);
            if (niter > 1) load_global(r1, 1);                   // set 1: odd chunks
            if (niter > 2) load_global(r0, 2);                   // set 0: even chunks
        }
        __syncthreads();
        for (int it = 0; it < niter; it += 2) {
            step(it, r1);
            if (it + 1 < niter) step(it + 1, r0);
        }
    } else {
        if (niter > 0) {
            load_global(r0, 0);
            store_lds(r0, 0);
        }
        __syncthreads();
        for (int it = 0; it < niter; ++it) {
            if (it + 1 < niter) load_global(r0, it + 1);
            const unsigned short* sa = smem + (it & 1) * STAGE;
            const unsigned short* sb = sa + 2 * PLANE_A;
            if constexpr (MF == 16) {
                mma_chunk16(sa, sb, []() {});
            } else {
                mma_ks(sa, sb, 0);
                mma_ks(sa, sb, 1);
            }
            if (it + 1 < niter) store_lds(r0, (it + 1) & 1);
            __syncthreads();
        }
    }

    float* red = (float*)smem_raw;
    if (do_bsum) {                                 // [32 px][TB] partial column sums -> one row
        if (b_lane) {
#pragma unroll
            for (int e = 0; e < 8; ++e) red[pb * TB + (tid % VPR_B) * 8 + e] = bs_acc[e];
        }
        __syncthreads();
        for (int c = tid; c < TB; c += NTHR) {
            float t = 0.f;
            for (int k = 0; k < BK; ++k) t += red[k * TB + c];
            const int cc = tile_b * TB + c;
            if (cc < a.ldo) a.bsum[(long long)split * a.ldo + cc] = cc < a.CB ? t : 0.f;
        }
        __syncthreads();
    }
    // accumulators of one tap -> LDS [TA][TB + 8] -> float4 rows of that tap's slab; three times
    constexpr int CP = TB + 8, TPR = TB / 4, RPS = NTHR / TPR;
    const int c4 = (tid % TPR) * 4, col = tile_b * TB + c4;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        cdf_acc_stage(red, CP, wa * 32, wb * TNW, acc[i], half, l31);
        __syncthreads();
        float* O = a.out + ((long long)split * a.ntaps + 3 * grp + i) * a.CA * a.ldo;
        if (col < a.ldo) {
            for (int r = tid / TPR; r < TA; r += RPS) {
                const int row = tile_a * TA + r;
                if (row >= a.CA) break;
                float4 v = *(const float4*)(red + r * CP + c4);
                cdf_wgrad_zero_pad(v, col, a.CB);
                *(float4*)(O + (long long)row * a.ldo + col) = v;
            }
        }
        __syncthreads();
    }
}

template <int NS, int TA, int TB, bool STACK2 = false>
static int launch_wgrad_spx(const SpxWgradArgs& a, hipStream_t s, CdfPlan* plan) {
    constexpr size_t stage = (size_t)2 * 32 * ((TA + 32) + (TB + 32)) * sizeof(unsigned short);
    constexpr size_t epi = (size_t)TA * (TB + 8) * sizeof(float);
    constexpr size_t lds = 2 * stage > epi ? 2 * stage : epi;
    const int tiles = (STACK2 ? 1 : cdf_cdiv(a.CA, TA)) * cdf_cdiv(a.CB, TB);
    if (plan) return cdf_plan_set(plan, STACK2 ? CDF_FORM_WGRAD_STACK2 : CDF_FORM_WGRAD_SPX, TA, TB, 0, 0, 0, tiles, (long long)tiles * (STACK2 ? cdf_cdiv(a.ntaps, 2) : a.ntaps) * a.nsplit);
    CDF_LAUNCH_LDS((conv_wgrad_spx_kernel<TA, TB, STACK2, NS>), dim3(tiles, STACK2 ? cdf_cdiv(a.ntaps, 2) : a.ntaps, a.nsplit), dim3(256), lds, s, a);
    return cdf_check_launch("conv_wgrad_spx");
}

// The geometry test of the row-of-taps kernel, for the query and the dispatcher alike.  same_size: nine taps of a stride-1 convolution whose
// two operands both have the pixel grid's size (the query is told, the dispatcher looks at its geometry).
static bool wgrad_row3_geom(const cdf_gemm_tuning& T, int QH, int QW, int CA, int CB, int ntaps, bool same_size) {
    return T.wgrad_row3 && same_size && ntaps == 9 && (QW == 16 || QW == 32 || QW == 64 || QW == 128) && (QH * QW) % 32 == 0 &&
           (QW >= 32 || QH % (32 / QW) == 0) && !(CA <= 64 && CB <= 64);
}

// 1 if cdf_conv_wgrad_bf16x takes the row-of-taps kernel for this geometry (the caller sizes the split count by it:
// 3 tap blocks per tile and one block per CU instead of 9 (or 5) and two)
extern "C" int cdf_conv_wgrad_bf16x_is_row3(int QH, int QW, int CA, int CB, int ntaps, int same_size_3x3, const cdf_gemm_tuning* tune) {
    return wgrad_row3_geom(*cdf_tune(tune), QH, QW, CA, CB, ntaps, same_size_3x3 != 0);
}

template <int NS, int TA, int TB>
static int launch_wgrad_row3(const SpxWgradArgs& a, hipStream_t s, CdfPlan* plan) {
    constexpr size_t stage = (size_t)2 * (36 * (TA + 32) + 32 * (TB + 32)) * sizeof(unsigned short);
    constexpr size_t epi = (size_t)TA * (TB + 8) * sizeof(float);
    constexpr size_t lds = 2 * stage > epi ? 2 * stage : epi;
    const int tiles = cdf_cdiv(a.CA, TA) * cdf_cdiv(a.CB, TB);
    if (plan) return cdf_plan_set(plan, CDF_FORM_WGRAD_ROW3, TA, TB, 0, 0, 0, tiles, (long long)tiles * 3 * a.nsplit);
    CDF_LAUNCH_LDS((conv_wgrad_row3_kernel<TA, TB, NS>), dim3(tiles, 3, a.nsplit), dim3(512), lds, s, a);
    return cdf_check_launch("conv_wgrad_row3");
}

template <int NS>
static int dispatch_wgrad_bf16x(SpxWgradArgs& a, int QH, int QW, int HA, int WA, int sa, int HB, int WB, int sb, int CA, int CB, int ntaps,
                                const cdf_gemm_tuning& T, hipStream_t s, CdfPlan* plan = nullptr) {
    // 3 x 3 stride-1 "same" convolutions (X shifted per tap, dY read in place): one block per row of taps.  The tap table is the only
    // condition on top of wgrad_row3_geom: row-major taps, A shifted by (-1 .. 1, -1 .. 1), B in place -- what the query's caller promises
    // with same_size_3x3.
    if (wgrad_row3_geom(T, QH, QW, CA, CB, ntaps, sa == 1 && sb == 1 && HA == QH && WA == QW && HB == QH && WB == QW)) {
        bool ok = true;
        for (int g = 0; g < 3 && ok; ++g) {
            int seen = 0;
            for (int i = 0; i < 3; ++i) {
                const int t = 3 * g + i;
                ok = ok && a.day[t] == a.day[3 * g] && a.dby[t] == 0 && a.dbx[t] == 0 && a.dax[t] >= -1 && a.dax[t] <= 1 && a.day[t] >= -1 && a.day[t] <= 1;
                seen |= 1 << (a.dax[t] + 1);
            }
            ok = ok && seen == 7;
        }
        if (ok) {
            if (CA <= 64) return launch_wgrad_row3<NS, 64, 128>(a, s, plan);
            if (CB <= 64) return launch_wgrad_row3<NS, 128, 64>(a, s, plan);
            return launch_wgrad_row3<NS, 128, 128>(a, s, plan);
        }
    }
    // thin layers get 64-wide tiles so that no half of a tile multiplies padding
    if (CA <= 64 && CB <= 64) return launch_wgrad_spx<NS, 64, 64>(a, s, plan);
    if (CA <= 64) {
        bool same_b = ntaps >= 2;                  // two taps can share the B rows only if B is read at one offset
        for (int t = 1; t < ntaps; ++t) same_b = same_b && a.dby[t] == a.dby[0] && a.dbx[t] == a.dbx[0];
        if (same_b && T.wgrad_stack) return launch_wgrad_spx<NS, 128, 128, true>(a, s, plan);
        return launch_wgrad_spx<NS, 64, 128>(a, s, plan);
    }
    if (CB <= 64) return launch_wgrad_spx<NS, 128, 64>(a, s, plan);
    return launch_wgrad_spx<NS, 128, 128>(a, s, plan);
}

// The kernel a cdf_conv_wgrad_bf16x call of this geometry launches: dispatch_wgrad_bf16x itself, stopped before the launch.
extern "C" int cdf_conv_wgrad_bf16x_form(int QH, int QW, int HA, int WA, int sa, int HB, int WB, int sb, int CA, int CB, int ntaps, const int* tap_desc,
                                         int ns, int nsplit, const cdf_gemm_tuning* tune, int* tiles_grid) {
    CDF_REQUIRE(ns == 1 || ns == 3, "cdf_conv_wgrad_bf16x_form: bad arguments");
    CDF_TUNE_CHECK(tune, "cdf_conv_wgrad_bf16x_form");
    SpxWgradArgs a = {};
    int rc = cdf_fill_wgrad_geom(a, "cdf_conv_wgrad_bf16x_form", 0, QH, QW, HA, WA, sa, HB, WB, sb, CA, CB, ntaps, tap_desc, nsplit, 32);   // (no batch: nothing is launched)
    if (rc) return rc;
    CdfPlan plan = {0, 0, 0};
    rc = ns == 3 ? dispatch_wgrad_bf16x<3>(a, QH, QW, HA, WA, sa, HB, WB, sb, CA, CB, ntaps, *cdf_tune(tune), nullptr, &plan)
                           : dispatch_wgrad_bf16x<1>(a, QH, QW, HA, WA, sa, HB, WB, sb, CA, CB, ntaps, *cdf_tune(tune), nullptr, &plan);
    if (rc) return rc;
    if (tiles_grid) { tiles_grid[0] = plan.tiles; tiles_grid[1] = plan.grid; }
    return plan.code;
}

extern "C" int cdf_conv_wgrad_bf16x(const void* a_hi, const void* a_lo, int lda, const void* b_hi, const void* b_lo, int ldb,
                                    const void* zero, float* ws, int ldo, int B, int QH, int QW, int HA, int WA, int sa, int HB, int WB,
                                    int sb, int CA, int CB, int ntaps, const int* tap_desc, int nsplit, float* bsum, const cdf_gemm_tuning* tune,
                                    void* stream) {
    CDF_REQUIRE(a_hi && b_hi && zero && ws, "cdf_conv_wgrad_bf16x: null pointer");
    CDF_TUNE_CHECK(tune, "cdf_conv_wgrad_bf16x");
    CDF_REQUIRE((a_lo != nullptr) == (b_lo != nullptr), "cdf_conv_wgrad_bf16x: pass both lo planes (split precision) or neither (single-pass bf16)");
    CDF_REQUIRE(((((uintptr_t)a_hi) | ((uintptr_t)a_lo) | ((uintptr_t)b_hi) | ((uintptr_t)b_lo) | ((uintptr_t)zero)) & 15) == 0, "cdf_conv_wgrad_bf16x: operands must be 16B aligned");
    CDF_REQUIRE(lda % 8 == 0 && ldb % 8 == 0 && CA % 8 == 0 && CB % 8 == 0 && lda >= CA && ldb >= CB && ldo % 4 == 0 && ldo >= CB, "cdf_conv_wgrad_bf16x: channels / pitches must be multiples of 8");
    SpxWgradArgs a;
    const int rc = cdf_fill_wgrad_geom(a, "cdf_conv_wgrad_bf16x", B, QH, QW, HA, WA, sa, HB, WB, sb, CA, CB, ntaps, tap_desc, nsplit, 32);
    if (rc) return rc;
    a.a_hi = (const unsigned short*)a_hi; a.a_lo = (const unsigned short*)a_lo; a.b_hi = (const unsigned short*)b_hi;
    a.b_lo = (const unsigned short*)b_lo; a.zero = (const unsigned short*)zero; a.out = ws; a.bsum = bsum;
    a.lda = lda; a.ldb = ldb; a.ldo = ldo; a.xcd_swizzle = cdf_tune(tune)->wgrad_swizzle;
    return a_lo ? dispatch_wgrad_bf16x<3>(a, QH, QW, HA, WA, sa, HB, WB, sb, CA, CB, ntaps, *cdf_tune(tune), CDF_S)
                : dispatch_wgrad_bf16x<1>(a, QH, QW, HA, WA, sa, HB, WB, sb, CA, CB, ntaps, *cdf_tune(tune), CDF_S);
}

