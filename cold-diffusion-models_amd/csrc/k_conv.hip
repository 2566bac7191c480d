// k_conv.hip — dense convolutions / linear layers of the UNets as implicit GEMMs on the gfx950
// matrix cores (v_mfma_f32_32x32x2_f32: exact fp32, 64 FLOP/clk/SIMD).
//
// Replaces the ATen/MIOpen ops behind (reference file:line)
//   nn.Conv2d 3x3 / 1x1 / 4x4-s2, nn.ConvTranspose2d 4x4-s2, nn.Linear
//     deblurring_diffusion_pytorch.py:105-109,140-154,173-174,211-216,253 ; Model2.py:36-73,85-112,148-163
// and their autograd backward (dgrad = the same gather-GEMM with a mirrored tap table and the
// [tap][Cout][Cin] weight packing; wgrad = pixel-reduction GEMM with split-K).
//
// One gather-GEMM kernel covers every forward and data-gradient case:
//   Y[m, co] = epilogue( sum_{tap, ci} X[pix(m, tap), ci] * Wp[tap][ci][co] )
//   m = (b, qy, qx) over a per-phase output grid; pix = (qy*is + dy[tap], qx*is + dx[tap]),
//   zero outside the image; output pixel (qy*os + phase.oy, qx*os + phase.ox).
//   Regular convs are one phase; stride-2 transposed convs are 4 output-parity phases of 2x2 taps.
//
// Tiling (wave64): 256 threads = 4 waves, block tile BMxBN, wave tile WMxWN built from 32x32
// MFMA tiles, BK = 16 channels of one tap per main-loop step, operands staged through LDS
// (register prefetch of step i+1 while step i is on the matrix pipe, one barrier per step).
// The MFMA k index is free as long as A and B agree, so lane half h owns k = 8h..8h+7 of the
// chunk: its A fragment is two ds_read_b128 (row stride 20 floats -> conflict-free).
#include <atomic>
#include "cdf_wgrad.h"
#include "colddiff.h"

struct ConvArgs {
    const float* x;
    const float* w;
    float* y;
    const float* bias;   // [Cout] nullable
    const float* sbias;  // [B][ld_sbias] per-sample bias (time embedding) nullable
    const float* res;    // residual, added last, nullable
    float* pre;          // nullable: receives the pre-activation value
    const float* mul;    // nullable: epilogue multiplier source (activation-gradient fusion)
    int ldx, ldw, ldy, ld_sbias, ldr, ldp, ldm;
    int B, H, W, Cin, OH, OW, Cout, QH, QW, os, is;
    int act;         // 0 none, 1 GELU, 2 SiLU, 3 ReLU
    int mul_mode;    // 0 none, 1 v*=gelu'(mul), 2 v*=silu'(mul), 3 v*=mul
    int accumulate;  // y += v
    int nphase, vec;
    unsigned short* ys_hi;   // (unused by the fp32 kernels: always null)
    unsigned short* ys_lo;
    int ld_ys;
    int io_bf;               // CDF_IO_*_BF16 bits (cdf_epilogue.h): always 0 for the fp32 entry points
    long long x_bs, w_bs, y_bs;     // blockIdx.z = outer*batch2 + inner: outer batch strides (elements)
    long long x_bs2, w_bs2, y_bs2;  // inner batch strides (e.g. attention heads)
    int epi_follow;                 // batched launch whose y offsets are whole rows (y_bs % ldy == 0, y_bs2 % ldy == 0) and that has epilogue
                                    // operands: pre / mul / res are addressed like y (row offset added to the pixel index), not from row 0
    int batch2;
    CdfPhase ph[4];
};

template <int BM, int BN, int WM, int WN, bool BT>
__global__ void __launch_bounds__(256, 4) conv_igemm_kernel(ConvArgs a) {
    constexpr int BK = 16, AS = BK + 4;
    constexpr int MT = WM / 32, NT = WN / 32, WAVES_N = BN / WN;
    constexpr int APASS = BM / 64;
    constexpr int BVEC = BK * BN / 4;               // float4 per B tile
    constexpr int BPASS = (BVEC + 255) / 256;
    static_assert((BM / WM) * (BN / WN) == 4, "4 waves per block");
    constexpr int ASZ = BM * AS, BSZ = BK * BN;
    constexpr int EPI_ROWS = (BM / WM) * 32, EPI_SZ = EPI_ROWS * (BN + 8);      // one 32-row slab per wave row, see epilogue
    constexpr int SMEM = 2 * (ASZ + BSZ) > EPI_SZ ? 2 * (ASZ + BSZ) : EPI_SZ;
    __shared__ __attribute__((aligned(16))) float smem[SMEM];
    float (*As)[ASZ] = (float (*)[ASZ])smem;
    float (*Bs)[BSZ] = (float (*)[BSZ])(smem + 2 * ASZ);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    const int M = a.B * a.QH * a.QW;
    const int tiles_n = (a.Cout + BN - 1) / BN, tiles_m = (M + BM - 1) / BM;
    const int tile = cdf_xcd_order(blockIdx.x, tiles_m * tiles_n);
    const int tile_m = tile / tiles_n, tile_n = tile - tile_m * tiles_n;
    const CdfPhase& ph = a.ph[blockIdx.y];
    const int zo = blockIdx.z / a.batch2, zi = blockIdx.z - zo * a.batch2;
    const float* X = a.x + (long long)zo * a.x_bs + (long long)zi * a.x_bs2;
    const float* Wt = a.w + (long long)zo * a.w_bs + (long long)zi * a.w_bs2;
    float* Y = a.y + (long long)zo * a.y_bs + (long long)zi * a.y_bs2;
    long long pix_off = 0;
    if (a.epi_follow) {
        pix_off = ((long long)zo * a.y_bs + (long long)zi * a.y_bs2) / a.ldy;
        Y = a.y;
    }

    // ---- A-operand row bookkeeping ----------------------------------------------------------
    const int a_col = (tid & 3) * 4;
    int a_iy0[APASS], a_ix0[APASS];
    unsigned a_pix[APASS];                                   // pixel index of (b, iy0, ix0); the tap adds dy*W + dx
#pragma unroll
    for (int p = 0; p < APASS; ++p) {
        const int m = tile_m * BM + (tid >> 2) + 64 * p;
        if (m < M) {
            const int qx = m % a.QW, t2 = m / a.QW;
            a_iy0[p] = (t2 % a.QH) * a.is;
            a_ix0[p] = qx * a.is;
            a_pix[p] = (unsigned)(((t2 / a.QH) * a.H + a_iy0[p]) * a.W + a_ix0[p]);
        } else {
            a_iy0[p] = -(1 << 28);
            a_ix0[p] = 0;
            a_pix[p] = 0;
        }
    }
    const int nchunks = (a.Cin + BK - 1) / BK;
    const int niter = ph.ntaps * nchunks;

    // Tap table -> LDS once (a dynamic index into the by-value kernel argument compiles to global byte loads in front
    // of every chunk's tile loads); the next entry is fetched when the tap counter advances, an iteration ahead.
    // CDF_MAX_TAPS + 1 entries: the fetch one past the end is harmless.
    __shared__ int tap_lds[CDF_MAX_TAPS + 1];
    if (tid <= CDF_MAX_TAPS)
        tap_lds[tid] = tid < ph.ntaps ? (ph.dy[tid] & 0xFF) | ((ph.dx[tid] & 0xFF) << 8) | ((ph.wi[tid] & 0xFF) << 16) : 0;
    __syncthreads();
    int tap_cur = tap_lds[0];

    // Straight-line prefetch: every load is unconditional -- an element outside the image / channel range reads the
    // library's zero page instead (pointer select, no value select: hipcc turns "ok ? load : 0" back into a branch, and
    // a load inside a divergent branch waits for everything in flight first).
    f32x4_t ra[APASS], rb[BPASS];                            // (arrays of HIP float4 structs would live in scratch)
    int tap = 0, c0 = 0, issued = 0;                         // (tap, channel chunk) of the NEXT load
    auto load_global = [&]() {
        int tc = tap_cur;                                    // stays in a VGPR (see k_conv_sp.hip)
#ifndef CDF_EMU
        asm volatile("" : "+v"(tc));
#endif
        const int dy = (int)(signed char)(tc & 0xFF), dx = (int)(signed char)((tc >> 8) & 0xFF), wi = (tc >> 16) & 0xFF;
        const int tap_pix = dy * a.W + dx;
#pragma unroll
        for (int p = 0; p < APASS; ++p) {
            const unsigned iy = (unsigned)(a_iy0[p] + dy), ix = (unsigned)(a_ix0[p] + dx);
            const bool ok = iy < (unsigned)a.H && ix < (unsigned)a.W && (c0 + a_col) < a.Cin;
            const size_t off = (size_t)(a_pix[p] + (unsigned)tap_pix) * (unsigned)a.ldx + (unsigned)(c0 + a_col);
            ra[p] = *(const f32x4_t*)(ok ? X + off : cdf_zero_page);
        }
#pragma unroll
        for (int p = 0; p < BPASS; ++p) {
            const int idx = tid + 256 * p;
            if (!BT) {
                const int k = idx / (BN / 4), n4 = idx - k * (BN / 4);
                const int ci = c0 + k, co = tile_n * BN + n4 * 4;
                const bool ok = idx < BVEC && ci < a.Cin && co < a.Cout;
                const size_t off = (size_t)((unsigned)wi * (unsigned)a.Cin + (unsigned)ci) * (unsigned)a.ldw + (unsigned)co;
                rb[p] = *(const f32x4_t*)(ok ? Wt + off : cdf_zero_page);
            } else {
                // B given as [N][K] (K contiguous): read 4 consecutive k of one output column
                const int n = idx / (BK / 4), k4 = idx - n * (BK / 4);
                const int ci = c0 + k4 * 4, co = tile_n * BN + n;
                const bool ok = idx < BVEC && ci < a.Cin && co < a.Cout;
                const size_t off = (size_t)(unsigned)co * (unsigned)a.ldw + (unsigned)ci;
                rb[p] = *(const f32x4_t*)(ok ? Wt + off : cdf_zero_page);
            }
        }
        const bool more = issued + 1 < niter;                // block-uniform
        issued += more ? 1 : 0;
        const int c1 = c0 + BK;
        const bool wrap = c1 >= a.Cin;
        c0 = more ? (wrap ? 0 : c1) : c0;
        tap += (more && wrap) ? 1 : 0;
        tap_cur = tap_lds[tap];
    };
    auto store_lds = [&](int buf) {
#pragma unroll
        for (int p = 0; p < APASS; ++p) *(f32x4_t*)(&As[buf][((tid >> 2) + 64 * p) * AS + a_col]) = ra[p];
#pragma unroll
        for (int p = 0; p < BPASS; ++p) {
            const int idx = tid + 256 * p;
            if (idx < BVEC) {
                if (!BT) {
                    const int k = idx / (BN / 4), n4 = idx - k * (BN / 4);
                    *(f32x4_t*)(&Bs[buf][k * BN + n4 * 4]) = rb[p];
                } else {
                    const int n = idx / (BK / 4), k4 = idx - n * (BK / 4);
                    Bs[buf][(k4 * 4 + 0) * BN + n] = rb[p][0];
                    Bs[buf][(k4 * 4 + 1) * BN + n] = rb[p][1];
                    Bs[buf][(k4 * 4 + 2) * BN + n] = rb[p][2];
                    Bs[buf][(k4 * 4 + 3) * BN + n] = rb[p][3];
                }
            }
        }
    };

    f32x16_t acc[MT][NT];
    cdf_acc_zero(acc);

    const int half = lane >> 5, l31 = lane & 31;
    if (niter > 0) {
        load_global();
        store_lds(0);
    }
    __syncthreads();
    for (int it = 0; it < niter; ++it) {
        const int buf = it & 1;
        load_global();                                       // chunk it + 1 (past the end: the last chunk again, never stored)
        float af[MT][8], bf[NT][8];
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const float* p = &As[buf][(wm * WM + i * 32 + l31) * AS + half * 8];
            const float4 v0 = *(const float4*)p, v1 = *(const float4*)(p + 4);
            af[i][0] = v0.x; af[i][1] = v0.y; af[i][2] = v0.z; af[i][3] = v0.w;
            af[i][4] = v1.x; af[i][5] = v1.y; af[i][6] = v1.z; af[i][7] = v1.w;
        }
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int s = 0; s < 8; ++s) bf[j][s] = Bs[buf][(half * 8 + s) * BN + wn * WN + j * 32 + l31];
#pragma unroll
        for (int s = 0; s < 8; ++s)
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i][s], bf[j][s], acc[i][j], 0, 0, 0);
        if (it + 1 < niter) store_lds(buf ^ 1);
        __syncthreads();
    }

    // ---- epilogue: MT passes of one 32-row slab per wave through LDS, float4 rows out (cdf_epilogue.h) ----
    constexpr int CP = BN + 8;
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        if (i > 0) __syncthreads();          // previous pass fully read (the K loop itself ends with a barrier)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                smem[(wm * 32 + cdf_acc_row(r, half)) * CP + wn * WN + j * 32 + l31] = acc[i][j][r];
        __syncthreads();
        cdf_epilogue_rows<BN, EPI_ROWS>(a, ph, Y, smem, tile_m * BM, tile_n * BN, M, tid,
                                        [i](int p) { return (p >> 5) * WM + i * 32 + (p & 31); }, pix_off);
    }
}

// ------------------------------------------------------------------------------------------------
// wgrad: out[z][tap][ca][cb] = sum_{m in split z} XA[pixA(m,tap)][ca] * XB[pixB(m,tap)][cb]
// m = (b, qy, qx); pixA = (qy*sa + day, qx*sa + dax) in [HA,WA]; pixB likewise. Rows with an
// out-of-range pixel on either side contribute zero.  The kernel keeps its own text around the K loop (cdf_wgrad.h says why).
// ------------------------------------------------------------------------------------------------
struct WgradArgs {
    const float* xa;
    const float* xb;
    float* out;
    int lda, ldb, ldo;
    int B, QH, QW;
    int HA, WA, sa, HB, WB, sb;
    int CA, CB;
    int ntaps;
    int nsplit, m_per_split;
    long long a_bs, b_bs, o_bs;  // batch strides (blockIdx.z / nsplit)
    int nbatch;
    float* bsum;                 // nullable: [nsplit][ldo] column sums of XB (bias gradient), written by tile_a == 0, tap == 0
    signed char day[CDF_MAX_TAPS], dax[CDF_MAX_TAPS], dby[CDF_MAX_TAPS], dbx[CDF_MAX_TAPS];
};

template <int BMC, int BNC, int WM, int WN>
__global__ void __launch_bounds__(256, 4) conv_wgrad_kernel(WgradArgs a) {
    constexpr int BK = 16;
    constexpr int MT = WM / 32, NT = WN / 32, WAVES_N = BNC / WN;
    constexpr int AVEC = BK * BMC / 4, BVEC = BK * BNC / 4;
    constexpr int APASS = (AVEC + 255) / 256, BPASS = (BVEC + 255) / 256;
    static_assert((BMC / WM) * (BNC / WN) == 4, "4 waves per block");
    __shared__ __attribute__((aligned(16))) float Xs[2][BK * BMC];
    __shared__ __attribute__((aligned(16))) float Ys[2][BK * BNC];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    const int tiles_b = (a.CB + BNC - 1) / BNC;
    int bx, by, bz;
    cdf_wgrad_block(1, bx, by, bz);                          // XCD-aware block order: the tiles and taps of one pixel range share an L2
    const int tile_a = bx / tiles_b, tile_b = bx - tile_a * tiles_b;
    const int tap = by;
    const int batch = bz / a.nsplit, split = bz - batch * a.nsplit;
    const float* XA = a.xa + (long long)batch * a.a_bs;
    const float* XB = a.xb + (long long)batch * a.b_bs;
    const int M = a.B * a.QH * a.QW;
    const int m_lo = split * a.m_per_split;
    int m_hi = m_lo + a.m_per_split;
    if (m_hi > M) m_hi = M;
    const int niter = m_hi > m_lo ? (m_hi - m_lo + BK - 1) / BK : 0;
    const int day = a.day[tap], dax = a.dax[tap], dby = a.dby[tap], dbx = a.dbx[tap];

    // per-thread load slots: the pixel (b, qy, qx) of each slot is decoded once and then advanced
    // incrementally by BK rows per main-loop step (no integer divisions in the loop)
    int a_q[APASS][3], b_q[BPASS][3];   // qx, qy, b
    auto decode = [&](int m, int* q) {
        q[0] = m % a.QW;
        const int t2 = m / a.QW;
        q[1] = t2 % a.QH;
        q[2] = t2 / a.QH;
    };
    auto advance = [&](int* q) {
        q[0] += BK;
        while (q[0] >= a.QW) {
            q[0] -= a.QW;
            if (++q[1] >= a.QH) { q[1] = 0; ++q[2]; }
        }
    };
#pragma unroll
    for (int p = 0; p < APASS; ++p) decode(m_lo + (tid + 256 * p) / (BMC / 4), a_q[p]);
#pragma unroll
    for (int p = 0; p < BPASS; ++p) decode(m_lo + (tid + 256 * p) / (BNC / 4), b_q[p]);
    const bool do_bsum = a.bsum != nullptr && tile_a == 0 && tap == 0;
    float4 bs_acc[BPASS];
#pragma unroll
    for (int p = 0; p < BPASS; ++p) bs_acc[p] = make_float4(0.f, 0.f, 0.f, 0.f);

    float4 ra[APASS], rb[BPASS];
    auto load_global = [&](int it) {
        const int m0 = m_lo + it * BK;
#pragma unroll
        for (int p = 0; p < APASS; ++p) {
            const int idx = tid + 256 * p;
            ra[p] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (idx < AVEC) {
                const int k = idx / (BMC / 4), c4 = idx - k * (BMC / 4);
                const int m = m0 + k, ca = tile_a * BMC + c4 * 4;
                const int qx = a_q[p][0], qy = a_q[p][1], b = a_q[p][2];
                const int ay = qy * a.sa + day, ax = qx * a.sa + dax;
                const int by = qy * a.sb + dby, bx = qx * a.sb + dbx;
                const bool ok = m < m_hi && ca < a.CA && ay >= 0 && ay < a.HA && ax >= 0 && ax < a.WA && by >= 0 && by < a.HB && bx >= 0 && bx < a.WB;
                const float* ptr = ok ? XA + (((long long)b * a.HA + ay) * a.WA + ax) * a.lda + ca : XA;   // unconditional load, select after
                const float4 v = *(const float4*)ptr;
                ra[p] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
                advance(a_q[p]);
            }
        }
#pragma unroll
        for (int p = 0; p < BPASS; ++p) {
            const int idx = tid + 256 * p;
            rb[p] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (idx < BVEC) {
                const int k = idx / (BNC / 4), c4 = idx - k * (BNC / 4);
                const int m = m0 + k, cb = tile_b * BNC + c4 * 4;
                const int qx = b_q[p][0], qy = b_q[p][1], b = b_q[p][2];
                const int by = qy * a.sb + dby, bx = qx * a.sb + dbx;
                const bool ok = m < m_hi && cb < a.CB && by >= 0 && by < a.HB && bx >= 0 && bx < a.WB;
                const float* ptr = ok ? XB + (((long long)b * a.HB + by) * a.WB + bx) * a.ldb + cb : XB;
                const float4 v = *(const float4*)ptr;
                rb[p] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
                advance(b_q[p]);
                if (do_bsum) {
                    bs_acc[p].x += rb[p].x; bs_acc[p].y += rb[p].y; bs_acc[p].z += rb[p].z; bs_acc[p].w += rb[p].w;
                }
            }
        }
    };
    auto store_lds = [&](int buf) {
#pragma unroll
        for (int p = 0; p < APASS; ++p) {
            const int idx = tid + 256 * p;
            if (idx < AVEC) *(float4*)(&Xs[buf][idx * 4]) = ra[p];
        }
#pragma unroll
        for (int p = 0; p < BPASS; ++p) {
            const int idx = tid + 256 * p;
            if (idx < BVEC) *(float4*)(&Ys[buf][idx * 4]) = rb[p];
        }
    };

    f32x16_t acc[MT][NT];
    cdf_acc_zero(acc);

    const int half = lane >> 5, l31 = lane & 31;
    if (niter > 0) {
        load_global(0);
        store_lds(0);
    }
    __syncthreads();
    for (int it = 0; it < niter; ++it) {
        const int buf = it & 1;
        if (it + 1 < niter) load_global(it + 1);
        float af[MT][8], bf[NT][8];
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int s = 0; s < 8; ++s) af[i][s] = Xs[buf][(half * 8 + s) * BMC + wm * WM + i * 32 + l31];
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int s = 0; s < 8; ++s) bf[j][s] = Ys[buf][(half * 8 + s) * BNC + wn * WN + j * 32 + l31];
#pragma unroll
        for (int s = 0; s < 8; ++s)
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i][s], bf[j][s], acc[i][j], 0, 0, 0);
        if (it + 1 < niter) store_lds(buf ^ 1);
        __syncthreads();
    }

    if (do_bsum) {
        // column sums of the XB rows this split visited: reduce the BK/… row lanes that share a column quad through LDS
        __syncthreads();
        float* red = &Ys[0][0];                    // reuse: [rows = 256*BPASS / (BNC/4)][BNC]
#pragma unroll
        for (int p = 0; p < BPASS; ++p) {
            const int idx = tid + 256 * p;
            if (idx < BVEC) *(float4*)(red + idx * 4) = bs_acc[p];
        }
        __syncthreads();
        for (int c = tid; c < BNC; c += 256) {
            float t = 0.f;
            for (int k = 0; k < BK; ++k) t += red[k * BNC + c];
            const int cb = tile_b * BNC + c;
            if (cb < a.ldo) a.bsum[(long long)(batch * a.nsplit + split) * a.ldo + cb] = cb < a.CB ? t : 0.f;
        }
    }
    // o_bs >= 0: [batch (stride o_bs)][split][tap][CA][ldo];  o_bs < 0: [split][batch][tap][CA][ldo] -- the per-batch results stay
    // separate and ONE cdf_unpack_reduce(T = nbatch * ntaps) sums the splits of all of them
    float* O = a.o_bs >= 0 ? a.out + (long long)batch * a.o_bs + ((long long)split * a.ntaps + tap) * a.CA * a.ldo
                           : a.out + (((long long)split * a.nbatch + batch) * a.ntaps + tap) * a.CA * a.ldo;
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ca = tile_a * BMC + wm * WM + i * 32 + cdf_acc_row(r, half);
            if (ca >= a.CA) continue;
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int cb = tile_b * BNC + wn * WN + j * 32 + l31;
                if (cb < a.ldo) O[(long long)ca * a.ldo + cb] = cb < a.CB ? acc[i][j][r] : 0.f;
            }
        }
}

// ================================================================================================
// C ABI
// ================================================================================================
static int check_feat(const char* who, const void* p, int ld, int C) {
    CDF_REQUIRE(p != nullptr, "%s: null tensor", who);
    CDF_REQUIRE((((uintptr_t)p) & 15) == 0, "%s: tensor not 16-byte aligned", who);
    CDF_REQUIRE(ld % 4 == 0 && ld >= C, "%s: pitch %d must be a multiple of 4 and >= C=%d", who, ld, C);
    return CDF_OK;
}

template <int BM, int BN, int WM, int WN>
static int launch_conv(const ConvArgs& a, int batch, bool bt, hipStream_t s) {
    const int M = a.B * a.QH * a.QW;
    const int tiles = cdf_cdiv(M, BM) * cdf_cdiv(a.Cout, BN);
    if (bt)
        CDF_LAUNCH((conv_igemm_kernel<BM, BN, WM, WN, true>), dim3(tiles, a.nphase, batch), dim3(256), 0, s, a);
    else
        CDF_LAUNCH((conv_igemm_kernel<BM, BN, WM, WN, false>), dim3(tiles, a.nphase, batch), dim3(256), 0, s, a);
    return cdf_check_launch("conv_igemm");
}

// Generic gather-GEMM.  taps: int array [nphase][1 + 2 + 3*ntaps_max]... see colddiff.h
extern "C" int cdf_conv_gemm_io(const float* x, int ldx, const float* w, int ldw, float* y, int ldy, int B, int H, int W,
                                int Cin, int OH, int OW, int Cout, int QH, int QW, int os, int is, int nphase,
                                const int* phase_desc, const float* bias, const float* sbias, int ld_sbias,
                                const void* res, int ldr, void* pre, int ldp, const void* mul, int ldm, int act,
                                int mul_mode, int accumulate, int b_trans, int batch, long long x_bs, long long w_bs,
                                long long y_bs, int batch2, long long x_bs2, long long w_bs2, long long y_bs2, int io_bf16, void* y_hi,
                                int ld_ys, void* stream);

extern "C" int cdf_conv_gemm(const float* x, int ldx, const float* w, int ldw, float* y, int ldy, int B, int H, int W,
                             int Cin, int OH, int OW, int Cout, int QH, int QW, int os, int is, int nphase,
                             const int* phase_desc, const float* bias, const float* sbias, int ld_sbias,
                             const float* res, int ldr, float* pre, int ldp, const float* mul, int ldm, int act,
                             int mul_mode, int accumulate, int b_trans, int batch, long long x_bs, long long w_bs,
                             long long y_bs, int batch2, long long x_bs2, long long w_bs2, long long y_bs2, void* stream) {
    return cdf_conv_gemm_io(x, ldx, w, ldw, y, ldy, B, H, W, Cin, OH, OW, Cout, QH, QW, os, is, nphase, phase_desc, bias, sbias, ld_sbias, res, ldr,
                            pre, ldp, mul, ldm, act, mul_mode, accumulate, b_trans, batch, x_bs, w_bs, y_bs, batch2, x_bs2, w_bs2, y_bs2, 0, nullptr, 0,
                            stream);
}

// ... with typed epilogue operands (io_bf16: CDF_IO_RES_BF16 | CDF_IO_PRE_BF16 | CDF_IO_MUL_BF16) and an optional bf16 output plane y_hi
// (pitch ld_ys; with it y may be NULL: bf16 activation storage -- the fp32 product's result enters the bf16 stream rounded once, no fp32
// copy).  A batched launch without a y needs the row-offset addressing (an epilogue operand, outputs that are whole rows of one tensor:
// ldy / y_bs / y_bs2 then only describe the row offsets).
extern "C" int cdf_conv_gemm_io(const float* x, int ldx, const float* w, int ldw, float* y, int ldy, int B, int H, int W,
                                int Cin, int OH, int OW, int Cout, int QH, int QW, int os, int is, int nphase,
                                const int* phase_desc, const float* bias, const float* sbias, int ld_sbias,
                                const void* res_, int ldr, void* pre_, int ldp, const void* mul_, int ldm, int act,
                                int mul_mode, int accumulate, int b_trans, int batch, long long x_bs, long long w_bs,
                                long long y_bs, int batch2, long long x_bs2, long long w_bs2, long long y_bs2, int io_bf16, void* y_hi,
                                int ld_ys, void* stream) {
    const float* res = (const float*)res_;
    float* pre = (float*)pre_;
    const float* mul = (const float*)mul_;
    int rc;
    CDF_REQUIRE((io_bf16 & ~7) == 0, "cdf_conv_gemm_io: io_bf16 has unknown bits (%d)", io_bf16);
    CDF_REQUIRE(y || (y_hi && !accumulate), "cdf_conv_gemm_io: no output (y NULL needs y_hi and no accumulate)");
    CDF_REQUIRE(!y_hi || (ld_ys % 4 == 0 && ld_ys >= Cout && Cout % 4 == 0 && (((uintptr_t)y_hi) & 7) == 0), "cdf_conv_gemm_io: the output plane needs Cout %% 4 == 0, ld_ys %% 4 == 0, 8-byte alignment");
    if ((rc = check_feat("cdf_conv_gemm(x)", x, ldx, Cin))) return rc;
    if (y && (rc = check_feat("cdf_conv_gemm(y)", y, 4, 0))) return rc;
    CDF_REQUIRE(w && (((uintptr_t)w) & 15) == 0 && ldw % 4 == 0, "cdf_conv_gemm: weights must be 16B aligned, ldw%%4==0");
    CDF_REQUIRE(ldy >= Cout, "cdf_conv_gemm: ldy < Cout");
    CDF_REQUIRE(nphase >= 1 && nphase <= 4 && phase_desc, "cdf_conv_gemm: nphase must be 1..4");
    CDF_REQUIRE(B > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && QH > 0 && QW > 0 && batch >= 1 && batch2 >= 1, "cdf_conv_gemm: bad shape");
    CDF_REQUIRE(!b_trans || (Cin % 4 == 0), "cdf_conv_gemm: b_trans needs K %% 4 == 0");
    CDF_REQUIRE(!mul_mode || mul, "cdf_conv_gemm: mul_mode without mul tensor");
    ConvArgs a;
    a.x = x; a.w = w; a.ldx = ldx; a.ldw = ldw;
    cdf_fill_gemm_common(a, y, ldy, bias, sbias, ld_sbias, res, ldr, pre, ldp, mul, ldm, B, H, W, Cin, OH, OW, Cout, QH, QW, os, is, nphase, act, mul_mode,
                         accumulate, y_hi, nullptr, ld_ys, io_bf16);
    a.x_bs = x_bs; a.w_bs = w_bs; a.y_bs = y_bs;
    a.x_bs2 = x_bs2; a.w_bs2 = w_bs2; a.y_bs2 = y_bs2; a.batch2 = batch2;
    a.vec = a.vec && y_bs % 4 == 0 && y_bs2 % 4 == 0;
    a.epi_follow = 0;
    if ((long long)batch * batch2 > 1 && (res || pre || mul)) {
        CDF_REQUIRE(y_bs % ldy == 0 && y_bs2 % ldy == 0 && !sbias, "cdf_conv_gemm: batched launches with pre / mul / res operands need per-batch outputs that are whole rows "
                    "of y (y_bs and y_bs2 multiples of ldy) and no per-sample bias");
        a.epi_follow = 1;
    }
    CDF_REQUIRE((!y_hi && !io_bf16) || a.vec, "cdf_conv_gemm_io: bf16 operands / the output plane need the vectorised epilogue (16-byte-aligned pointers, pitches %% 4, Cout %% 4)");
    CDF_REQUIRE(y || (long long)batch * batch2 == 1 || a.epi_follow, "cdf_conv_gemm_io: a batched launch without y needs an epilogue operand (row-offset addressing)");
    batch *= batch2;
    if ((rc = cdf_fill_phases(a.ph, nphase, phase_desc, "cdf_conv_gemm"))) return rc;
    const bool bt = b_trans != 0;
    if (Cout <= 32) return launch_conv<128, 32, 32, 32>(a, batch, bt, CDF_S);
    if (Cout <= 64) return launch_conv<256, 64, 64, 64>(a, batch, bt, CDF_S);
    return launch_conv<128, 128, 64, 64>(a, batch, bt, CDF_S);
}

template <int BMC, int BNC, int WM, int WN>
static int launch_wgrad(const WgradArgs& a, int batch, hipStream_t s) {
    const int tiles = cdf_cdiv(a.CA, BMC) * cdf_cdiv(a.CB, BNC);
    CDF_LAUNCH((conv_wgrad_kernel<BMC, BNC, WM, WN>), dim3(tiles, a.ntaps, batch * a.nsplit), dim3(256), 0, s, a);
    return cdf_check_launch("conv_wgrad");
}

extern "C" int cdf_wgrad_nsplit(int M, int CA, int CB, int ntaps) {
    // One full wave of workgroups: the 128x128 wgrad kernel is resident 4x per CU (1024 slots on 256 CUs).
    // tiles * nsplit must not spill a handful of blocks into a second round (a straggler round costs a whole
    // block time), so round DOWN to fill at most one round; keep >= 256 pixels per split.
    auto tiles_of = [&](int c) { return c <= 64 ? 1 : cdf_cdiv(c, 128); };
    const int tiles = tiles_of(CA) * tiles_of(CB) * ntaps;
    int ns = 1024 / tiles;
    const int max_by_m = M / 256 > 0 ? M / 256 : 1;
    if (ns > max_by_m) ns = max_by_m;
    if (ns < 1) ns = 1;
    if (ns > 256) ns = 256;
    return ns;
}

extern "C" int cdf_conv_wgrad(const float* xa, int lda, const float* xb, int ldb, float* ws, int ldo, int B, int QH,
                              int QW, int HA, int WA, int sa, int HB, int WB, int sb, int CA, int CB, int ntaps,
                              const int* tap_desc, int nsplit, int batch, long long a_bs, long long b_bs,
                              long long o_bs, float* bsum, void* stream) {
    int rc;
    if ((rc = check_feat("cdf_conv_wgrad(xa)", xa, lda, CA))) return rc;
    if ((rc = check_feat("cdf_conv_wgrad(xb)", xb, ldb, CB))) return rc;
    CDF_REQUIRE(ws && ldo % 4 == 0 && ldo >= CB, "cdf_conv_wgrad: bad workspace pitch");
    CDF_REQUIRE(batch >= 1, "cdf_conv_wgrad: bad batch");
    WgradArgs a;
    if ((rc = cdf_fill_wgrad_geom(a, "cdf_conv_wgrad", B, QH, QW, HA, WA, sa, HB, WB, sb, CA, CB, ntaps, tap_desc, nsplit, 16))) return rc;
    a.xa = xa; a.xb = xb; a.out = ws; a.lda = lda; a.ldb = ldb; a.ldo = ldo;
    a.a_bs = a_bs; a.b_bs = b_bs; a.o_bs = o_bs; a.bsum = bsum; a.nbatch = batch;
    if (CA <= 32) {
        if (CB <= 32) return launch_wgrad<64, 64, 32, 32>(a, batch, CDF_S);
        return launch_wgrad<32, 128, 32, 32>(a, batch, CDF_S);
    }
    if (CB <= 32) return launch_wgrad<128, 32, 32, 32>(a, batch, CDF_S);
    if (CA <= 64 && CB <= 64) return launch_wgrad<64, 64, 32, 32>(a, batch, CDF_S);
    if (CA <= 64) return launch_wgrad<64, 128, 32, 64>(a, batch, CDF_S);
    if (CB <= 64) return launch_wgrad<128, 64, 64, 32>(a, batch, CDF_S);
    return launch_wgrad<128, 128, 64, 64>(a, batch, CDF_S);
}
