// k_conv_sp.hip — the dense-conv gather-GEMM on the bf16 matrix cores with SPLIT-PRECISION operands.
//
// gfx950 runs v_mfma_f32_32x32x16_bf16 at 16x the rate of the exact-fp32 MFMA and has no TF32-like
// mode.  To stay inside the fp32 parity budget (1e-4 on UNet outputs) every fp32 operand is split
// into two bf16 terms, x = hi + lo (hi = bf16(x), lo = bf16(x - hi): 16 mantissa bits), and a product
// is evaluated as  a*b ~= ah*bh + ah*bl + al*bh  with fp32 accumulation in the MFMA ("bf16x3",
// relative error ~2^-16 per product instead of bf16's 2^-8): 3 MFMAs at 16x the rate = 5.3x the fp32
// MFMA throughput.  split = 1 uses only the hi terms (plain bf16 operands, fp32 accumulate).
//
// Same tap-table / phase / epilogue semantics as conv_igemm_kernel (k_conv.hip); differences:
//   * weights arrive pre-split and pre-transposed: w_hi / w_lo are bf16 [tap][Cout][ldk] (K contiguous,
//     ldk = Cin rounded up to 32, zero padded) from cdf_pack_weight_bf16, so the B tile is a straight
//     16-byte copy into LDS;
//   * activations stay fp32 in HBM and are split while being written to LDS (VALU work hidden under MFMA);
//   * BK = 32, LDS rows are 40 bf16 (80 B) so that every ds_read_b128 fragment read is conflict-free.
#include "cdf_conv_sp.h"
#include "cdf_wgrad.h"
#include <atomic>

// 256 threads = 4 waves (2x2), block tile 128x128, wave tile 64x64 = 2x2 MFMA 32x32 tiles.
template <int SPLIT>
__global__ void __launch_bounds__(256, 2) conv_igemm_sp_kernel(SpArgs a) {
    constexpr int BM = 128, BN = 128, BK = 32, AS = 40;      // AS: LDS row stride in bf16 elements (80 B)
    constexpr int NPL = SPLIT == 1 ? 1 : 2;                  // operand planes (hi [, lo])
    constexpr int PLANE = BM * AS;                           // elements per plane (BM == BN)
    constexpr int STAGE = 2 * NPL * PLANE;                   // A planes then B planes
    CDF_DYN_SMEM(smem_raw);
    unsigned short* smem = (unsigned short*)smem_raw;        // [2 stages][STAGE]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int M = a.B * a.QH * a.QW;
    const int tiles_n = (a.Cout + BN - 1) / BN, tiles_m = (M + BM - 1) / BM;
    const int tile = cdf_xcd_order(blockIdx.x, tiles_m * tiles_n);
    const int tile_m = tile / tiles_n, tile_n = tile - tile_m * tiles_n;
    const CdfPhase& ph = a.ph[blockIdx.y];

    // A rows of this thread: row = (tid >> 3) + 32 p, float4 column (tid & 7)
    const int a_c4 = (tid & 7) * 4;
    int a_iy0[4], a_ix0[4];
    unsigned a_pix[4];          // pixel index of (b, iy0, ix0); the tap adds a wave-uniform dy*W + dx
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int m = tile_m * BM + (tid >> 3) + 32 * p;
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
    // B rows of this thread: n = brow + 64 p, 16-byte column (tid & 3); brow pairs rows R and R+4 inside each
    // 8-lane ds_write_b128 group (conflict-free stores, see conv_igemm_spx_kernel)
    const int b_q = tid & 3;
    const int bg8 = tid >> 3, brow = ((bg8 >> 2) << 3) + (bg8 & 3) + (((tid >> 2) & 1) << 2);
    const int nchunks = (a.Cin + BK - 1) / BK;
    const int niter = ph.ntaps * nchunks;

    // Loads are UNCONDITIONAL (a load inside a divergent branch makes hipcc wait vmcnt(0) per load and
    // serialises the whole prefetch): out-of-image / tail elements read a clamped, always-valid address and
    // are zeroed by a select when they are written to LDS.  Weight rows/columns outside the tile are clamped
    // too; they only feed output columns that are never stored.
    float4 ra[4];
    uint4 rbh0, rbh1, rbl0, rbl1;          // named registers (an array of HIP vector structs ends up in scratch here)
    rbl0 = rbl1 = make_uint4(0u, 0u, 0u, 0u);
    unsigned a_ok = 0;
    int b_row[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int n = tile_n * BN + brow + 64 * p;
        b_row[p] = n < a.Cout ? n : a.Cout - 1;
    }
    auto load_global = [&](int it) {
        const int tap = it / nchunks, c0 = (it - tap * nchunks) * BK;
        const int dy = ph.dy[tap], dx = ph.dx[tap], wi = ph.wi[tap];
        const int tap_pix = dy * a.W + dx;
        const bool cok = (c0 + a_c4) < a.Cin;
        const float* xc = a.x + c0 + a_c4;
        a_ok = 0;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const unsigned iy = (unsigned)(a_iy0[p] + dy), ix = (unsigned)(a_ix0[p] + dx);     // unsigned compare folds the >= 0 test
            const bool ok = iy < (unsigned)a.H && ix < (unsigned)a.W && cok;
            const float* ptr = ok ? xc + (size_t)(a_pix[p] + (unsigned)tap_pix) * (unsigned)a.ldx : a.x;
            ra[p] = *(const float4*)ptr;
            a_ok |= (ok ? 1u : 0u) << p;
        }
        const long long off0 = ((long long)wi * a.Cout + b_row[0]) * a.ldk + c0 + b_q * 8;
        const long long off1 = ((long long)wi * a.Cout + b_row[1]) * a.ldk + c0 + b_q * 8;
        rbh0 = *(const uint4*)(a.w_hi + off0);
        rbh1 = *(const uint4*)(a.w_hi + off1);
        if (SPLIT > 1) {
            rbl0 = *(const uint4*)(a.w_lo + off0);
            rbl1 = *(const uint4*)(a.w_lo + off1);
        }
    };
    auto store_lds = [&](int buf) {
        unsigned short* st = smem + buf * STAGE;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            uint2 hi, lo;
            const float keep = ((a_ok >> p) & 1u) ? 1.0f : 0.0f;       // loaded values are finite: zeroing by multiplication
            const float4 v = make_float4(ra[p].x * keep, ra[p].y * keep, ra[p].z * keep, ra[p].w * keep);
            if (SPLIT > 1) {
                cdf_split4_trunc(v, hi, lo);
            } else {      // plain bf16 operands: round to nearest even
                hi.x = cdf_f2bf(v.x) | (cdf_f2bf(v.y) << 16);
                hi.y = cdf_f2bf(v.z) | (cdf_f2bf(v.w) << 16);
                lo = hi;
            }
            const int off = ((tid >> 3) + 32 * p) * AS + a_c4;
            *(uint2*)(st + off) = hi;
            if (SPLIT > 1) *(uint2*)(st + PLANE + off) = lo;
        }
        unsigned short* sb = st + NPL * PLANE;
        const int offb0 = brow * AS + b_q * 8, offb1 = (brow + 64) * AS + b_q * 8;
        *(uint4*)(sb + offb0) = rbh0;
        *(uint4*)(sb + offb1) = rbh1;
        if (SPLIT > 1) {
            *(uint4*)(sb + PLANE + offb0) = rbl0;
            *(uint4*)(sb + PLANE + offb1) = rbl1;
        }
    };

    f32x16_t acc[2][2];
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
        const unsigned short* sa = smem + buf * STAGE;
        const unsigned short* sb = sa + NPL * PLANE;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int k0 = ks * 16 + half * 8;
            bf16x8_v ah[2], al[2], bh[2], bl[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int off = (wm * 64 + i * 32 + l31) * AS + k0;
                ah[i] = *(const bf16x8_v*)(sa + off);
                if (SPLIT > 1) al[i] = *(const bf16x8_v*)(sa + PLANE + off);
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int off = (wn * 64 + j * 32 + l31) * AS + k0;
                bh[j] = *(const bf16x8_v*)(sb + off);
                if (SPLIT > 1) bl[j] = *(const bf16x8_v*)(sb + PLANE + off);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    if (SPLIT > 1) {
                        // small cross terms first, the dominant hi*hi term last
                        acc[i][j] = CDF_MFMA_BF16(al[i], bh[j], acc[i][j]);
                        acc[i][j] = CDF_MFMA_BF16(ah[i], bl[j], acc[i][j]);
                    }
                    acc[i][j] = CDF_MFMA_BF16(ah[i], bh[j], acc[i][j]);
                }
        }
        if (it + 1 < niter) store_lds(buf ^ 1);
        __syncthreads();
    }

    cdf_sp_epilogue<128, 128, 2, 2, SPLIT == 1>(a, ph, acc, (float*)smem_raw, tile_m, tile_n, M, tid);
}

// ------------------------------------------------------------------------------------------------
// Weight gradient on the bf16 matrix cores, split precision (same contract as conv_wgrad_kernel):
//   out[z][tap][ca][cb] = sum_{m in split z} XA[pixA(m,tap)][ca] * XB[pixB(m,tap)][cb]
// The contraction runs over PIXELS, which are the slow index of both NHWC operands, so the LDS tiles
// stay pixel-major ([32 px][128 ch] bf16 hi / lo, split while being stored) and each lane assembles
// its 8-pixel MFMA fragment from eight 16-bit LDS reads (32 consecutive channels per half-wave:
// conflict-free).  Tile 128 (ca) x 128 (cb), BK = 32 pixels, 4 waves of 64x64.  Block range, pixel walk, bias-gradient fold: cdf_wgrad.h.
// ------------------------------------------------------------------------------------------------
struct SpWgradArgs {
    const float* xa;
    const float* xb;
    float* out;
    float* bsum;
    int lda, ldb, ldo;
    int B, QH, QW;
    int HA, WA, sa, HB, WB, sb;
    int CA, CB;
    int ntaps, nsplit, m_per_split, xcd_swizzle;
    signed char day[CDF_MAX_TAPS], dax[CDF_MAX_TAPS], dby[CDF_MAX_TAPS], dbx[CDF_MAX_TAPS];
};

__global__ void __launch_bounds__(256, 2) conv_wgrad_sp_kernel(SpWgradArgs a) {
    constexpr int BC = 128, BK = 32;
    constexpr int PLANE = BK * BC;                 // bf16 elements per plane
    constexpr int STAGE = 4 * PLANE;               // A hi, A lo, B hi, B lo
    CDF_DYN_SMEM(smem_raw);
    unsigned short* smem = (unsigned short*)smem_raw;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const CdfWgradRange g = cdf_wgrad_range<BK, BC>(a, a.xcd_swizzle);
    const int tile_a = g.tile_a, tile_b = g.tile_b, tap = g.tap, m_lo = g.m_lo, m_hi = g.m_hi, niter = g.niter;
    const int day = a.day[tap], dax = a.dax[tap], dby = a.dby[tap], dbx = a.dbx[tap];

    // load slots: pixel k = (tid >> 5) + 8 p, channel quad c4 = tid & 31 (both operands)
    const int c4 = (tid & 31) * 4;
    const CdfPixelWalk<BK> walk(a);
    int q[4][3];
#pragma unroll
    for (int p = 0; p < 4; ++p) walk.decode(m_lo + (tid >> 5) + 8 * p, q[p]);
    const bool do_bsum = g.bsum(a);
    float4 bs_acc[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) bs_acc[p] = make_float4(0.f, 0.f, 0.f, 0.f);
    const int ca = tile_a * BC + c4, cb = tile_b * BC + c4;

    float4 ra[4], rb[4];
    const int ca_l = ca < a.CA ? ca : 0, cb_l = cb < a.CB ? cb : 0;      // clamped (always readable) channel offsets
    auto load_global = [&](int it) {
        const int m0 = m_lo + it * BK;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int m = m0 + (tid >> 5) + 8 * p;
            const int qx = q[p][0], qy = q[p][1], b = q[p][2];
            const unsigned ay = (unsigned)(qy * a.sa + day), ax = (unsigned)(qx * a.sa + dax);
            const unsigned by = (unsigned)(qy * a.sb + dby), bx = (unsigned)(qx * a.sb + dbx);
            const bool bok = m < m_hi && by < (unsigned)a.HB && bx < (unsigned)a.WB;
            const bool aok = bok && ay < (unsigned)a.HA && ax < (unsigned)a.WA && ca < a.CA;
            const bool bok2 = bok && cb < a.CB;
            // unconditional loads from clamped addresses, zero-select afterwards (no divergent branch around a load)
            const float* pa = aok ? a.xa + (((long long)b * a.HA + ay) * a.WA + ax) * a.lda + ca_l : a.xa;
            const float* pb = bok2 ? a.xb + (((long long)b * a.HB + by) * a.WB + bx) * a.ldb + cb_l : a.xb;
            const float4 va = *(const float4*)pa, vb = *(const float4*)pb;
            ra[p] = aok ? va : make_float4(0.f, 0.f, 0.f, 0.f);
            rb[p] = bok2 ? vb : make_float4(0.f, 0.f, 0.f, 0.f);
            walk.advance(q[p]);
            if (do_bsum) {
                bs_acc[p].x += rb[p].x; bs_acc[p].y += rb[p].y; bs_acc[p].z += rb[p].z; bs_acc[p].w += rb[p].w;
            }
        }
    };
    auto store_lds = [&](int buf) {
        unsigned short* st = smem + buf * STAGE;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int off = ((tid >> 5) + 8 * p) * BC + c4;
            uint2 hi, lo;
            cdf_split4_trunc(ra[p], hi, lo);
            *(uint2*)(st + off) = hi;
            *(uint2*)(st + PLANE + off) = lo;
            cdf_split4_trunc(rb[p], hi, lo);
            *(uint2*)(st + 2 * PLANE + off) = hi;
            *(uint2*)(st + 3 * PLANE + off) = lo;
        }
    };

    f32x16_t acc[2][2];
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
        const unsigned short* st = smem + buf * STAGE;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int k0 = ks * 16 + half * 8;
            bf16x8_v ah[2], al[2], bh[2], bl[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const unsigned short* pa = st + k0 * BC + wm * 64 + i * 32 + l31;
                const unsigned short* pb = st + 2 * PLANE + k0 * BC + wn * 64 + i * 32 + l31;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    ah[i][e] = (short)pa[e * BC];
                    al[i][e] = (short)pa[PLANE + e * BC];
                    bh[i][e] = (short)pb[e * BC];
                    bl[i][e] = (short)pb[PLANE + e * BC];
                }
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    acc[i][j] = CDF_MFMA_BF16(al[i], bh[j], acc[i][j]);
                    acc[i][j] = CDF_MFMA_BF16(ah[i], bl[j], acc[i][j]);
                    acc[i][j] = CDF_MFMA_BF16(ah[i], bh[j], acc[i][j]);
                }
        }
        if (it + 1 < niter) store_lds(buf ^ 1);
        __syncthreads();
    }

    if (do_bsum) {
        float* red = (float*)smem;                 // [32 px][128] floats = 16 KB (stage 0 is idle now)
#pragma unroll
        for (int p = 0; p < 4; ++p) *(float4*)(red + ((tid >> 5) + 8 * p) * BC + c4) = bs_acc[p];
        cdf_wgrad_bsum_fold<BK, BC, 256>(a, red, tile_b, g.split, tid);
    }
    float* O = cdf_wgrad_slab(a, g.split, tap);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = tile_a * BC + wm * 64 + i * 32 + cdf_acc_row(r, half);
            if (row >= a.CA) continue;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int col = tile_b * BC + wn * 64 + j * 32 + l31;
                if (col < a.ldo) O[(long long)row * a.ldo + col] = col < a.CB ? acc[i][j][r] : 0.f;
            }
        }
}

extern "C" int cdf_conv_gemm_bf16(const float* x, int ldx, const void* w_hi, const void* w_lo, int ldk, float* y, int ldy, int B,
                                  int H, int W, int Cin, int OH, int OW, int Cout, int QH, int QW, int os, int is, int nphase,
                                  const int* phase_desc, const float* bias, const float* sbias, int ld_sbias, const float* res,
                                  int ldr, float* pre, int ldp, const float* mul, int ldm, int act, int mul_mode, int accumulate,
                                  int split, void* stream) {
    CDF_REQUIRE(x && w_hi && y && (((uintptr_t)x) & 15) == 0 && ldx % 4 == 0 && ldx >= Cin, "cdf_conv_gemm_bf16: bad x");
    CDF_REQUIRE((split == 1 || split == 3) && (split == 1 || w_lo), "cdf_conv_gemm_bf16: split must be 1 (bf16) or 3 (hi/lo bf16x3)");
    CDF_REQUIRE((((uintptr_t)w_hi) & 15) == 0 && ldk % 32 == 0 && ldk >= Cin, "cdf_conv_gemm_bf16: weights must be 16B aligned with ldk %% 32 == 0");
    CDF_REQUIRE(nphase >= 1 && nphase <= 4 && phase_desc && ldy >= Cout, "cdf_conv_gemm_bf16: bad geometry");
    CDF_REQUIRE(!mul_mode || mul, "cdf_conv_gemm_bf16: mul_mode without mul tensor");
    SpArgs a;
    a.x = x; a.w_hi = (const unsigned short*)w_hi; a.w_lo = (const unsigned short*)w_lo; a.ldx = ldx; a.ldk = ldk;
    cdf_fill_gemm_common(a, y, ldy, bias, sbias, ld_sbias, res, ldr, pre, ldp, mul, ldm, B, H, W, Cin, OH, OW, Cout, QH, QW, os, is, nphase, act, mul_mode,
                         accumulate, nullptr, nullptr, 0, 0);
    cdf_clear_epi(a);
    a.epi = cdf_epi_select(a);
    const int rc = cdf_fill_phases(a.ph, nphase, phase_desc, "cdf_conv_gemm_bf16");
    if (rc) return rc;
    const int M = B * QH * QW;
    const int tiles = cdf_cdiv(M, 128) * cdf_cdiv(Cout, 128);
    if (split == 1) {
        const size_t lds = CDF_SP_EPI_LDS;                 // operand stages (40 KB) < epilogue tile
        CDF_LAUNCH_LDS((conv_igemm_sp_kernel<1>), dim3(tiles, nphase), dim3(256), lds, CDF_S, a);
    } else {
        const size_t lds = (size_t)2 * 2 * 2 * 128 * 40 * sizeof(unsigned short);   // 80 KB >= CDF_SP_EPI_LDS
        CDF_LAUNCH_LDS((conv_igemm_sp_kernel<3>), dim3(tiles, nphase), dim3(256), lds, CDF_S, a);
    }
    return cdf_check_launch("conv_igemm_sp");
}

extern "C" int cdf_conv_wgrad_bf16(const float* xa, int lda, const float* xb, int ldb, float* ws, int ldo, int B, int QH, int QW,
                                   int HA, int WA, int sa, int HB, int WB, int sb, int CA, int CB, int ntaps, const int* tap_desc,
                                   int nsplit, float* bsum, void* stream) {
    CDF_REQUIRE(xa && xb && ws && (((uintptr_t)xa) & 15) == 0 && (((uintptr_t)xb) & 15) == 0, "cdf_conv_wgrad_bf16: null / unaligned operand");
    CDF_REQUIRE(lda % 4 == 0 && ldb % 4 == 0 && lda >= CA && ldb >= CB && ldo % 4 == 0 && ldo >= CB, "cdf_conv_wgrad_bf16: bad pitch");
    SpWgradArgs a;
    const int rc = cdf_fill_wgrad_geom(a, "cdf_conv_wgrad_bf16", B, QH, QW, HA, WA, sa, HB, WB, sb, CA, CB, ntaps, tap_desc, nsplit, 32);
    if (rc) return rc;
    a.xa = xa; a.xb = xb; a.out = ws; a.bsum = bsum; a.lda = lda; a.ldb = ldb; a.ldo = ldo; a.xcd_swizzle = 1;
    const size_t lds = (size_t)2 * 4 * 32 * 128 * sizeof(unsigned short);
    const int tiles = cdf_cdiv(CA, 128) * cdf_cdiv(CB, 128);
    CDF_LAUNCH_LDS(conv_wgrad_sp_kernel, dim3(tiles, ntaps, nsplit), dim3(256), lds, CDF_S, a);
    return cdf_check_launch("conv_wgrad_sp");
}
