#include "cdf_conv_sp.h"

// ================================================================================================
// 3 x 3 stride-1 convolutions with the INPUT TILE RESIDENT IN LDS ("halo" kernel).
//
// What bounds conv_igemm_spx_kernel is the operand DMA, not the matrix pipe (tools/ablate.py on MI355X, 512 -> 1024 at
// 16 x 16: 0.233 ms; without the DMA 0.131; MFMAs + barriers alone 0.125): every 32-channel K step brings 32 KB into LDS
// for 96 MFMAs, and only ~64 KB per CU are in flight against ~1.1 us of L2 / MALL latency.  Of those bytes half are the
// A tile -- and the nine taps of a 3 x 3 conv fetch the SAME pixels nine times, shifted.  Here the K loop runs channel
// chunk outermost, taps innermost: per 32-channel chunk the tile's pixels plus a one-pixel halo ((TH+2) x (W+2) rows of
// 64 B, both planes) are fetched ONCE, double buffered, and all nine taps read their A fragments out of that image at
// row offset dy (W+2) + dx.  Only the weights still stream per tap (3 stages).  DMA bytes per chunk, 128 x 128 tile:
// 9 x 32 KB -> 144 KB + 24..50 KB.
//
// Tile = TH = 128 / W full image rows (W = 16, 32, 64 or 128: one tile never straddles two images), so the tile's
// pixels are the contiguous range [128 tile_m, 128 tile_m + 128) of the flattened pixel index and the epilogue of the
// generic kernel applies unchanged.  Halo rows outside the image come from the zero page.  8 waves (4 x 2 of 32 x 64).
// XOR swizzle of the 16-byte column by cdf_swz<MF>(row) on both sides (cdf_conv_sp.h).  MF = 32: a lane's 16 fragment rows are
// consecutive halo rows except at an image-row wrap (+2), where a 2-way bank conflict can occur.  MF = 16: a fragment is 16 consecutive
// pixels from a multiple of 16, so (16 | W) it never wraps, and its swizzle is conflict-free from any first row.
// ================================================================================================
// MFMA shape of the K loop, per kernel form: 32 = v_mfma_f32_32x32x16_bf16, 16 = v_mfma_f32_16x16x32_bf16 (cdf_conv_sp.h).  Same output tile
// per wave, same register counts, same products per output; the 16 form issues twice as many MFMAs of half the length.  The K loop is
// matrix-pipe-bound at a clock the chip holds down under load, and the clock it holds depends on the shape: a form is on 16 where that
// measured faster per launch on random data (profiles/mfma_shape_ab.txt), and keeps no instance of the other shape.
// MI355X, B = 64, 16 against 32, median of three alternations (the 32 arm's own repetitions spread 0.0 - 0.9 %; NS = 1 at W = 128: 2.5 %):
//   NS = 3   every W / BN / BM form ahead: 128 -> 64 at 128 pixels +4.2 %, 128 -> 256 and 256 -> 128 at 64 +7.6 %, 256 -> 512 / 512 -> 256 at
//            32 +6.8 / +8.7 %, 512 -> 1024 / 1024 -> 512 / 1024 -> 2048 at 16 +9.2 / +12.6 / +9.0 %; BM = 128: +3.1 ... +11.5 %; the 64-wide N
//            tiles +2.9 ... +3.4 % (at B = 16, 1024 -> 512 at 16 pixels: +4.6 %)
//   NS = 1   W = 64 with BN = 128: 128 -> 256 -1.7 % (BM 256), -1.8 % (BM 128), -3.3 % (B = 16); 256 -> 128 +0.6 / +2.5 / 0.0 % -- no win, stays on 32.
//            Every other form ahead: W = 128 +4.9 %, W = 32 +3.7 / +7.2 %, W = 16 +5.0 / +6.2 %, the 64-wide N tiles +1.3 ... +6.1 %
constexpr int cdf_halo_mfma(int W, int BN, int BM, int NS) {
    (void)BM;
    return NS == 1 && W == 64 && BN == 128 ? 32 : 16;
}
// how many of the halo segments requested in steps t, t-1, ... t-(n-1) (tap index modulo 9) fall on steps with a request (t' < ta)
constexpr int cdf_halo_parts(int t, int n, int ta) {
    int c = 0;
    for (int d = 0; d < n; ++d) c += ((t - d + 9) % 9) < ta ? 1 : 0;
    return c;
}

template <int W, int BN, int NB, int BM, int NS = 3>                    // NB weight stages: NB - 1 tap steps requested ahead; BM = 128 or 256 pixels
__global__ void __launch_bounds__(512, 1) conv_igemm_halo_kernel(SpxArgs a) {
    constexpr int WM = 4, WN = 2, NW = 8, BK = 32, RE = CDF_SP_RE, MT = BM / WM / 32;
    constexpr int MF = cdf_halo_mfma(W, BN, BM, NS);
    using L = HaloLayout<W, BN, BM>;
    using Segs = typename L::Segs;                                        // 16-row DMA segments of the halo image
    static_assert(NB == L::NB, "the launcher instantiates the stage count of the layout");
    constexpr int TH = L::TH, HW2 = L::HW2, HR = L::HR;
    constexpr int TA = Segs::PER_WAVE;                                    // tap steps in which a wave fetches one A segment
    static_assert(NB >= 3 && NB <= 7 && TA <= 11 - NB && TA <= 12 - NB, "the next chunk's halo must be requested before the weights of its first tap");
    constexpr int NT = BN / WN / 32;                                      // 32 x 32 MFMA tiles per wave along N (M: 1)
    constexpr int SB = BN / 16 / NW;                                      // B segments per wave and plane (1 for BN = 128)
    static_assert(SB * NW * 16 == BN || BN == 64, "B tile must split into 16-row segments");
    constexpr int SBI = BN == 64 ? 1 : SB;                                // (BN = 64: waves 0..3 fetch a segment, 4..7 repeat them)
    constexpr int PLANE_A = L::PLANE_A, ABUF = L::ABUF, PLANE_B = L::PLANE_B, BSTAGE = L::BSTAGE;   // (unsigned short units)
    CDF_DYN_SMEM(smem_raw);
    unsigned short* smem = (unsigned short*)smem_raw;
    unsigned short* const abuf0 = smem;
    unsigned short* const bst0 = smem + L::OFF_B;

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int M = a.B * a.QH * a.QW;
    const int tiles_n = (a.Cout + BN - 1) / BN, tiles_m = M / BM;
    const int tile = cdf_xcd_order(blockIdx.x, tiles_m * tiles_n);
    const int tile_m = tile / tiles_n, tile_n = tile - tile_m * tiles_n;
    const CdfPhase& ph = a.ph[0];
    const int tpi = a.H / TH;                                              // tiles per image
    const int img = tile_m / tpi, y0 = (tile_m - img * tpi) * TH;

    // (tap indices are compile-time constants in the unrolled loops below: ph.dy[t] etc. are scalar kernel-argument loads
    // hoisted out of the K loop -- an LDS tap table would put an lgkmcnt(0) wait between the fragment reads and the MFMAs)

    // ---- DMA sources.  A: segments Segs::seg(wave, q), q < TA
    const int srow = cdf_dma_row(lane), q8 = cdf_dma_col<MF>(lane);
    const unsigned short* pa_hi[TA];
    const unsigned short* pa_lo[TA];
    int a_inc[TA], a_seg[TA];
#pragma unroll
    for (int q = 0; q < TA; ++q) {
        const int g = a_seg[q] = Segs::seg(wave, q);
        const int r = g * 16 + srow;
        const int hy = r / HW2, hx = r - hy * HW2;
        const int y = y0 - 1 + hy, x = hx - 1;
        const bool ok = r < HR && (unsigned)y < (unsigned)a.H && (unsigned)x < (unsigned)W;
        const size_t off = ((size_t)((img * a.H + y) * W + x)) * (unsigned)a.ldx + (unsigned)q8;
        pa_hi[q] = ok ? a.x_hi + off : a.zero;
        pa_lo[q] = ok ? a.x_lo + off : a.zero;
        a_inc[q] = ok ? BK : 0;
    }
    int b_row[SBI];
#pragma unroll
    for (int p = 0; p < SBI; ++p) {
        const int seg = BN == 64 ? (wave & 3) : wave * SB + p;
        b_row[p] = cdf_w_row(tile_n * BN + seg * 16 + srow, a.Cout);
    }
    const int nchunks = a.Cin / BK;

    auto fetch_a = [&](int q, int buf) {                     // segment a_seg[q] of the chunk the pointers stand at -> halo buffer buf
        unsigned short* seg = abuf0 + buf * ABUF + a_seg[q] * 16 * RE;
        CDF_GLDS16_K(pa_hi[q], seg);
        if constexpr (NS == 3) CDF_GLDS16_K(pa_lo[q], seg + PLANE_A);
    };
    auto advance_a = [&]() {
#pragma unroll
        for (int q = 0; q < TA; ++q) {
            pa_hi[q] += a_inc[q];
            pa_lo[q] += a_inc[q];
        }
    };
    auto fetch_b = [&](int c, int t, int stage) {            // weights of (chunk c, tap t) -> stage (= step % 3 = t % 3)
        if (c >= nchunks) c = nchunks - 1;                   // past the end: valid weights again, into an idle stage
        const int wi = ph.wi[t];
        unsigned short* st = bst0 + stage * BSTAGE;
#pragma unroll
        for (int p = 0; p < SBI; ++p) {
            const int seg = BN == 64 ? (wave & 3) : wave * SB + p;
            const size_t woff = cdf_w_off(wi, a.Cout, b_row[p], a.ldk, c * BK + q8);
            CDF_GLDS16_K(a.w_hi + woff, st + seg * 16 * RE);
            if constexpr (NS == 3) CDF_GLDS16_K(a.w_lo + woff, st + PLANE_B + seg * 16 * RE);
        }
    };
    constexpr int NPL = NS == 3 ? 2 : 1;                     // operand planes in flight (hi [, lo])
    constexpr int PB = NPL * SBI, PA = NPL;                  // DMA instructions per wave: one B step, one A segment

    typename cdf_acc_of<MF>::type acc[MT][NT];
    cdf_acc_zero(acc);

    const int half = lane >> 5, l31 = lane & 31;
    // this lane's A fragment rows for tap (0, 0): pixels p = (BM/4) wm + 32 i + l31 of the tile (MF = 32: one fragment per k16 step, the
    // same rows) or p = (BM/4) wm + 32 i + 16 f + (lane & 15), f = 0, 1 (MF = 16: one fragment per 16-row half, all 32 channels)
    constexpr int NF = MF == 16 ? 2 : 1;
    const int lrow = MF == 16 ? lane & 15 : l31, kblk = MF == 16 ? lane >> 4 : half;
    int row0[NF][MT];
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const int pix = wm * (BM / WM) + i * 32 + f * 16 + lrow;
            const int py = pix / W, px = pix - py * W;
            row0[f][i] = (py + 1) * HW2 + px + 1;
        }
    const int swb = cdf_swz<MF>(lrow);                       // B rows: tile-local, multiples of 16 apart

    // ---- prologue: halo of chunk 0, weights of steps 0 .. NB-2
#pragma unroll
    for (int q = 0; q < TA; ++q) fetch_a(q, 0);
    if (nchunks > 1) advance_a();                            // the pointers stand at the chunk requested next (the last one, at the end)
#pragma unroll
    for (int u = 0; u < NB - 1; ++u) fetch_b(u / 9, u % 9, u);  // (NB - 1 <= 9: all in chunk 0)
    int rd = 0;                                              // weight stage of the current step
    CDF_WAIT_DMA_LEAVE((NB - 2) * PB);                       // the halo and the weights of step 0 have landed
    CDF_LDS_BARRIER();
    bf16x8_v ah[2][MT], al[2][MT], bh[2][NT], bl[2][NT];
    const bool late = a.dephase != 0 && wave >= NW / 2;      // (wave-uniform)
    if (late) cdf_frag_zero(ah, al, bh, bl);
    auto mma_frags = [&]() { cdf_mma_tile<NS, MT, NT>(acc, ah, al, bh, bl); };
    for (int c = 0; c < nchunks; ++c) {
        const unsigned short* sa = abuf0 + (c & 1) * ABUF;
        // (during the last chunk its own halo is requested again, into the idle buffer: every step issues the same
        // number of DMA instructions, so the wait counts below are compile-time constants)
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            if (t < TA) fetch_a(t, (c + 1) & 1);
            if (t == TA - 1 && c + 2 < nchunks) advance_a();
            fetch_b(t + NB - 1 < 9 ? c : c + 1, (t + NB - 1) % 9, rd == 0 ? NB - 1 : rd - 1);   // step + NB-1 -> the stage read last step
            const int tapoff = (int)ph.dy[t] * HW2 + (int)ph.dx[t];
            const unsigned short* sb = bst0 + rd * BSTAGE;
            rd = rd + 1 == NB ? 0 : rd + 1;
            auto read_frags = [&]() {
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    cdf_read_frags_halo<NS, PLANE_A, MT, MF>(ah[ks], al[ks], sa, ks, kblk, row0[MF == 16 ? ks : 0], tapoff);
                    cdf_read_frags<NS, PLANE_B, NT, MF>(bh[ks], bl[ks], sb, ks, kblk, wn * (BN / WN) + (MF == 16 ? 16 * ks : 0) + lrow, swb);
                }
            };
            cdf_dephased_step(late, read_frags, mma_frags);
            // the weights of step + 1 (requested NB - 2 steps ago) have landed -- and with them, in order, every halo segment
            // requested before them; still in flight: the weight requests of the last NB - 2 steps and the halo segments
            // requested in those steps (a compile-time count per tap index)
            switch (cdf_halo_parts(t, NB - 2, TA)) {
                case 0: CDF_WAIT_DMA_LEAVE((NB - 2) * PB); break;
                case 1: CDF_WAIT_DMA_LEAVE((NB - 2) * PB + PA); break;
                case 2: CDF_WAIT_DMA_LEAVE((NB - 2) * PB + 2 * PA); break;
                case 3: CDF_WAIT_DMA_LEAVE((NB - 2) * PB + 3 * PA); break;
                case 4: CDF_WAIT_DMA_LEAVE((NB - 2) * PB + 4 * PA); break;
                default: CDF_WAIT_DMA_LEAVE((NB - 2) * PB + 5 * PA); break;
            }
            CDF_LDS_BARRIER();
        }
    }
    if (late) mma_frags();                                   // the fragments of the last step
    CDF_WAIT_DMA_LEAVE(0);                                   // the tail requests (never read) must not land in the epilogue tile
    CDF_LDS_BARRIER();

    cdf_sp_epilogue<BM, BN, WM, WN, NS == 1>(a, ph, acc, (float*)smem_raw, tile_m, tile_n, M, tid);
}

template <int NS, int W, int BN, int BM>
static int launch_igemm_halo(const SpxArgs& a, int M, hipStream_t s, CdfPlan* plan) {
    using L = HaloLayout<W, BN, BM>;
    const int tiles = (M / BM) * cdf_cdiv(a.Cout, BN);
    if (plan) return cdf_plan_set(plan, CDF_FORM_HALO, BM, BN, L::NB, 1, W, tiles, tiles);
    CDF_LAUNCH_LDS((conv_igemm_halo_kernel<W, BN, L::NB, BM, NS>), dim3(tiles), dim3(512), L::bytes, s, a);
    return cdf_check_launch("conv_igemm_halo");
}

template <int NS>
static int launch_halo_ns(int W, bool n64, int bm, const SpxArgs& a, int M, hipStream_t s, CdfPlan* plan) {
#define CDF_HALO_CASE(WW)                                                                                              \
    if (W == WW) {                                                                                                     \
        if (bm == 256)                                                                                                 \
            return n64 ? launch_igemm_halo<NS, WW, 64, 256>(a, M, s, plan)                                              \
                       : launch_igemm_halo<NS, WW, 128, WW <= 64 ? 256 : 128>(a, M, s, plan);                           \
        return n64 ? launch_igemm_halo<NS, WW, 64, 128>(a, M, s, plan) : launch_igemm_halo<NS, WW, 128, 128>(a, M, s, plan); \
    }
    CDF_HALO_CASE(128) CDF_HALO_CASE(64) CDF_HALO_CASE(32) CDF_HALO_CASE(16)
#undef CDF_HALO_CASE
    cdf_set_error("conv_igemm_halo: no kernel for image width %d", W);
    return CDF_E_UNSUPPORTED;
}

int cdf_launch_igemm_halo(int ns, int W, bool n64, int bm, const SpxArgs& a, int M, hipStream_t s, CdfPlan* plan) {
    return ns == 3 ? launch_halo_ns<3>(W, n64, bm, a, M, s, plan) : launch_halo_ns<1>(W, n64, bm, a, M, s, plan);
}

// cdf_mfma_bf16_16x16x32 (include/colddiff.h): one CDF_MFMA16_BF16 on one wave, operands and result through the lane maps of cdf_conv_sp.h
__global__ void __launch_bounds__(64) mfma16_probe_kernel(const unsigned short* a, const unsigned short* bt, float* c) {
    const int lane = threadIdx.x, l15 = lane & 15, quarter = lane >> 4;
    const bf16x8_v fa = *(const bf16x8_v*)(a + l15 * 32 + quarter * 8), fb = *(const bf16x8_v*)(bt + l15 * 32 + quarter * 8);
    f32x4_t acc;
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = c[cdf_acc_row16(r, quarter) * 16 + l15];
    acc = CDF_MFMA16_BF16(fa, fb, acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) c[cdf_acc_row16(r, quarter) * 16 + l15] = acc[r];
}

extern "C" int cdf_mfma_bf16_16x16x32(const void* a, const void* bt, float* c, void* stream) {
    CDF_REQUIRE(a && bt && c && ((uintptr_t)a & 15) == 0 && ((uintptr_t)bt & 15) == 0, "cdf_mfma_bf16_16x16x32: null or misaligned pointer");
    CDF_LAUNCH(mfma16_probe_kernel, dim3(1), dim3(64), 0, CDF_S, (const unsigned short*)a, (const unsigned short*)bt, c);
    return cdf_check_launch("mfma16_probe");
}
