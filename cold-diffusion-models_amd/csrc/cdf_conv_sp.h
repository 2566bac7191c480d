// cdf_conv_sp.h -- what the translation units of the split-precision / bf16 GEMM family share (round 6: k_conv_sp.hip was one 2600-line
// unit of 104 kernel instantiations, 3 minutes to compile; now one unit per kernel family, compiled in parallel):
//   k_conv_sp.hip         in-kernel-split GEMM + weight gradient
//   k_attn_kvctx.hip      the k | v + context kernel of LinearAttention
//   k_conv_spx.hip        generic pre-split gather-GEMM (LDS-DMA), split-K finish, the dispatcher and the C entry points of the pre-split GEMM
//   k_conv_halo.hip       3 x 3 stride-1 GEMM with the input tile + halo resident in LDS
//   k_conv_rowhalo.hip    resident row-halo stream kernel (64 / 128 input channels at 128-pixel width)
//   k_conv_wgrad_spx.hip  pre-split weight gradients (per-tap and row-of-taps kernels), their dispatcher and C entry points
// Here: the argument structs, the MFMA products (cdf_mma_sp / cdf_mma_tile), the tile epilogue (cdf_sp_epilogue), what the K loops of the three
// forward kernels share (DMA slot, weight row / offset, DMA segments, fragment reads, the de-phased step) and their LDS layouts (SpxLayout,
// HaloLayout, RowHaloLayout -- read by the kernel AND its launcher).  Accumulator zeroing / row map / staging and CDF_LAUNCH_LDS: cdf_common.h.
#pragma once
#include "cdf_gemm_args.h"
#include "colddiff.h"

typedef short bf16x8_v __attribute__((ext_vector_type(8)));
typedef short bf16x4_v __attribute__((ext_vector_type(4)));
typedef unsigned u32x4_v __attribute__((ext_vector_type(4)));
// The two bf16 MFMA shapes.  CDF_MFMA_BF16: v_mfma_f32_32x32x16_bf16 (lane l: A[row l & 31][k = 8 (l >> 5) + j], B[k][col l & 31], j < 8;
// C: cdf_acc_row, cdf_common.h).  CDF_MFMA16_BF16: v_mfma_f32_16x16x32_bf16 -- lane l holds A[row l & 15][k = 8 (l >> 4) + j] and
// B[k = 8 (l >> 4) + j][col l & 15], j < 8; C register r of lane l is row 4 (l >> 4) + r, column l & 15 (cdf_acc_row16).  Same FLOPs per
// cycle; a K loop that the chip's clock holds down can run faster on one than on the other (see cdf_halo_mfma, k_conv_halo.hip).
#ifdef CDF_EMU
#define CDF_MFMA_BF16(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0)
// The simulator has no 16 x 16 x 32 product: restated here on its wave exchange (products summed in k order, like its 32 x 32 x 16 form).
static inline f32x4_t cdf_emu_mfma_f32_16x16x32_bf16(bf16x8_v a, bf16x8_v b, f32x4_t c) {
    const int w = hipemu::wave_id(), l = hipemu::lane_id();
    for (int j = 0; j < 8; ++j) {
        hipemu::g.wave_a[w][l * 8 + j] = emu_bf16_to_f32(a[j]);
        hipemu::g.wave_b[w][l * 8 + j] = emu_bf16_to_f32(b[j]);
    }
    hipemu::wave_barrier();
    for (int r = 0; r < 4; ++r) {
        const int row = 4 * (l >> 4) + r, col = l & 15;
        float acc = c[r];
        for (int k = 0; k < 32; ++k) acc += hipemu::g.wave_a[w][((k >> 3) * 16 + row) * 8 + (k & 7)] * hipemu::g.wave_b[w][((k >> 3) * 16 + col) * 8 + (k & 7)];
        c[r] = acc;
    }
    hipemu::wave_barrier();
    return c;
}
#define CDF_MFMA16_BF16(a, b, c) cdf_emu_mfma_f32_16x16x32_bf16(a, b, c)
static inline bf16x4_v cdf_lds_read_tr16(const unsigned short* p) { return hipemu::ds_read_tr16_b64(p); }
#else
typedef __bf16 bf16x8_hw __attribute__((ext_vector_type(8)));
#define CDF_MFMA_BF16(a, b, c) \
    __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_hw, a), __builtin_bit_cast(bf16x8_hw, b), c, 0, 0, 0)
#define CDF_MFMA16_BF16(a, b, c) \
    __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_hw, a), __builtin_bit_cast(bf16x8_hw, b), c, 0, 0, 0)
// ds_read_b64_tr_b16: the 16 lanes of a group pass the addresses of a [4 rows][16 cols] bf16 block (lane t: row t >> 2,
// cols 4 (t & 3) .. +3, 8-byte aligned, any row pitch); lane t gets column t's 4 rows.
__device__ __forceinline__ bf16x4_v cdf_lds_read_tr16(const unsigned short* p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) bf16x4_v*)p);
}
#endif
// One operand's MFMA fragment out of a pixel-major tile: 8 consecutive pixels (two transposing reads, 4 rows apart) of the lane's channel, hi
// plane and -- NS == 3 -- the lo plane `plane` elements behind it.
// (p0: the lane's address in the block of pixels 0..3, p1: in the block of pixels 4..7)
template <int NS>
__device__ __forceinline__ void cdf_tr_frag2(const unsigned short* p0, const unsigned short* p1, int plane, bf16x8_v& hi, bf16x8_v& lo) {
    const bf16x4_v h0 = cdf_lds_read_tr16(p0), h1 = cdf_lds_read_tr16(p1);
    hi = __builtin_shufflevector(h0, h1, 0, 1, 2, 3, 4, 5, 6, 7);
    if constexpr (NS == 3) {
        const bf16x4_v l0 = cdf_lds_read_tr16(p0 + plane), l1 = cdf_lds_read_tr16(p1 + plane);
        lo = __builtin_shufflevector(l0, l1, 0, 1, 2, 3, 4, 5, 6, 7);
    }
}
template <int NS>
__device__ __forceinline__ void cdf_tr_frag(const unsigned short* p, int plane, int pitch, bf16x8_v& hi, bf16x8_v& lo) {
    const bf16x4_v h0 = cdf_lds_read_tr16(p), h1 = cdf_lds_read_tr16(p + 4 * pitch);
    hi = __builtin_shufflevector(h0, h1, 0, 1, 2, 3, 4, 5, 6, 7);
    if constexpr (NS == 3) {
        const bf16x4_v l0 = cdf_lds_read_tr16(p + plane), l1 = cdf_lds_read_tr16(p + plane + 4 * pitch);
        lo = __builtin_shufflevector(l0, l1, 0, 1, 2, 3, 4, 5, 6, 7);
    }
}
// The pixel-major tile image [px][pitch = T + 32] bf16 (T = 64 or 128 channels) of the weight-gradient kernels, by the MFMA shape MF of the K loop
// that reads it: element (row, col) lives at cdf_px_off<MF>(row, col, pitch), for the ds_write_b128 that fills it and for every transposing read.
//   MF = 32: plain.  The 16-lane group g of a fragment read takes the [4 px][16 ch] block at pixels 8 (g >> 1) + {0, 4}, channels 16 (g & 1): the
//     32 lanes the LDS serves together are 4 rows x 64 contiguous bytes, the rows 16 banks apart (pitch 80 or 48 dwords): all 64 banks once.
//   MF = 16: lane l of v_mfma_f32_16x16x32_bf16 holds channel l & 15 at pixels 8 (l >> 4) .. +7 -- both operands, both are pixel-major -- so group
//     g takes pixels 8 g + {0, 4} of ONE 16-channel block, and the two groups of a 32-lane pass are 4 rows x 32 bytes each, 8 pixel rows apart.
//     8 pitches are 0 modulo the 64 banks (so are 8 rows of any 16-byte-aligned pitch that keeps the 4 rows of a group apart): 2-way.  The rows of
//     the two groups, r and r + 8, always differ in bit 3, so XORing bit 3 of the row into bit 4 of the column (in elements: it swaps the 32-byte
//     halves of a 64-byte column block; in 16-byte chunks, chunk ^ ((row >> 3) & 1) << 1) moves one group 8 banks away from the other, from any
//     first row (the row-of-taps kernel reads X at row + 1 + dx): 4 rows x 2 groups x 8 banks, all 64 once.  A 16-byte store chunk and the 8-byte
//     read piece both stay inside their 32-byte half, and the swap stays inside one 32-channel block.  The swap depends on the row: rows r and
//     r + 4 of one fragment can sit in different halves, so every address comes from this function, never from base + q * pitch.
//     Measured (conv_wgrad_row3_kernel<128, 128, 3>, 256 -> 256 at 64 pixels, B = 64): SQ_LDS_BANK_CONFLICT 0 with MF = 32, 1.3 % of
//     SQ_LDS_IDX_ACTIVE with MF = 16 -- not zero; which access keeps a conflict is open (profiles/wgrad_mfma_shape_ab.txt, section 5).
// (col0: a multiple of 32 -- a wave's first column -- that the swap leaves alone; added first, the order the MF = 32 kernels were tuned with: one
//  of them sits exactly at the 128 registers of four waves per SIMD and goes over with the sum associated the other way)
template <int MF>
__device__ __forceinline__ int cdf_px_off(int row, int col, int pitch, int col0 = 0) {
    return row * pitch + col0 + (MF == 16 ? col ^ (((row >> 3) & 1) << 4) : col);
}

// Block tile BM x BN, WM x WN waves of (BM/WM) x (BN/WN): the whole tile goes through LDS in one pass (cdf_epilogue.h).
constexpr int CDF_SP_CPITCH = 136;
constexpr size_t CDF_SP_EPI_LDS = (size_t)128 * CDF_SP_CPITCH * sizeof(float);

// BFF: the kernel's epilogue family (cdf_epilogue.h: ids 1..6 for fp32 tensors, 7..11 for bf16 activation storage = the NS == 1 kernels)
// (Acc: f32x16_t or f32x4q_t -- cdf_acc_stage writes the same staged tile from either)
template <int BM, int BN, int WM = 2, int WN = 2, bool BFF = false, class Args, class Acc>
__device__ __forceinline__ void cdf_sp_epilogue(const Args& a, const CdfPhase& ph, const Acc (&acc)[BM / WM / 32][BN / WN / 32], float* cs,
                                                int tile_m, int tile_n, int M, int tid) {
    constexpr int CP = BN + 8, TM = BM / WM, TN = BN / WN, NTHR = 64 * WM * WN;
    const int lane = tid & 63, wave = tid >> 6, wm = wave / WN, wn = wave % WN, half = lane >> 5, l31 = lane & 31;
    // specialised straight-line form (block-uniform choice): the fused operand loads of the whole tile are issued BEFORE the
    // accumulators go through LDS
    const bool fast = cdf_epi_tile_ok<BM, BN>(a, M) && cdf_epi_family_ok(a.epi, BFF);
    // (the K loop ends with a barrier: every wave is done with the operand tiles)
    auto dump = [&]() { cdf_acc_stage(cs, CP, wm * TM, wn * TN, acc, half, l31); };
    if (a.epi == CDF_EPI_LNBWD) {                            // (block-uniform; the host guarantees whole tiles and Cout == BN)
        cdf_epi_lnbwd<BM, BN, NTHR>(a, cs, tile_m, tid, dump);
        return;
    }
    if (fast) {
        const long long trow = (long long)tile_m * BM;
        cdf_epi_dispatch<BFF>(a.epi, [&](auto spec) {
            using E = cdf_epi_fast<BN, BM, NTHR, decltype(spec)>;
            f32x4_t q[E::NR], bs[2];
            cdf_epi_load_bias<BN, NTHR>(a, bs, trow, tile_n * BN, tid);
            E::load(a, q, trow, tile_n * BN, tid);
            dump();
            CDF_LDS_BARRIER();                               // (LDS only: the operand loads stay in flight)
            E::template finish<false>(a, q, bs, cs, trow, tile_n * BN, tid);
        });
        return;
    }
    dump();
    __syncthreads();
    cdf_epilogue_rows<BN, BM, 64 * WM * WN>(a, ph, a.y, cs, tile_m * BM, tile_n * BN, M, tid, [](int p) { return p; });
}

struct SpArgs {
    const float* x;
    const unsigned short* w_hi;
    const unsigned short* w_lo;
    float* y;
    const float* bias;
    const float* sbias;
    const float* res;
    float* pre;
    const float* mul;
    int ldx, ldk, ldy, ld_sbias, ldr, ldp, ldm;
    int B, H, W, Cin, OH, OW, Cout, QH, QW, os, is;
    int act, mul_mode, accumulate, nphase, vec;
    unsigned short* ys_hi;         // nullable: bf16 hi / lo planes of the output (pitch ld_ys), written by the epilogue
    unsigned short* ys_lo;
    int ld_ys;
    int io_bf;                     // CDF_IO_*_BF16 bits (cdf_epilogue.h)
    int epi;                       // id of the specialised epilogue (cdf_epi_select; 0: the generic run-time-selected form)
    const float* ln_x;             // epi == CDF_EPI_LNBWD: LayerNorm input h (pitch ld_lnx), its statistics [M], the partial-sum output [tiles][2][Cout]
    const float* ln_mean;
    const float* ln_rstd;
    float* ln_part;
    int ld_lnx;
    CdfPhase ph[4];
};


// In-kernel split of an activation quad, kept to ~4 VALU ops per element (the kernel is VALU-, not
// MFMA-bound): hi = x truncated to bf16 (the residual x - hi is exact in fp32 and lands in lo, so
// truncating hi costs nothing), lo = (x - hi) truncated to bf16: x = hi + lo + O(2^-16 |x|).
__device__ __forceinline__ unsigned cdf_pack_hi16(unsigned u0, unsigned u1) { return (u0 >> 16) | (u1 & 0xFFFF0000u); }
__device__ __forceinline__ void cdf_split4_trunc(const float4& v, uint2& hi, uint2& lo) {
    const unsigned u0 = __float_as_uint(v.x), u1 = __float_as_uint(v.y), u2 = __float_as_uint(v.z), u3 = __float_as_uint(v.w);
    hi.x = cdf_pack_hi16(u0, u1);
    hi.y = cdf_pack_hi16(u2, u3);
    const unsigned r0 = __float_as_uint(v.x - __uint_as_float(u0 & 0xFFFF0000u));
    const unsigned r1 = __float_as_uint(v.y - __uint_as_float(u1 & 0xFFFF0000u));
    const unsigned r2 = __float_as_uint(v.z - __uint_as_float(u2 & 0xFFFF0000u));
    const unsigned r3 = __float_as_uint(v.w - __uint_as_float(u3 & 0xFFFF0000u));
    lo.x = cdf_pack_hi16(r0, r1);
    lo.y = cdf_pack_hi16(r2, r3);
}

// One algorithmic product a * b on the matrix cores.  NS = 3: split precision, al*bh + ah*bl + ah*bh (x = hi + lo bf16 terms,
// fp32 accumulate); NS = 1: single-pass bf16 operands (the hi planes only; al / bl are never read and their loads fold away).
template <int NS>
__device__ __forceinline__ void cdf_mma_sp(f32x16_t& acc, const bf16x8_v& ah, const bf16x8_v& al, const bf16x8_v& bh, const bf16x8_v& bl) {
    if constexpr (NS == 3) {
        acc = CDF_MFMA_BF16(al, bh, acc);
        acc = CDF_MFMA_BF16(ah, bl, acc);
    }
    acc = CDF_MFMA_BF16(ah, bh, acc);
}

// All products of one K chunk (two k16 steps) of a wave tile, TERM-MAJOR: consecutive MFMAs go to different accumulators
// (al*bh for every tile, then ah*bl, then ah*bh), so no instruction waits for the result of the one just issued; the
// summation order per accumulator is the same as in cdf_mma_sp.
template <int NS, int MT, int NT>
__device__ __forceinline__ void cdf_mma_tile(f32x16_t (&acc)[MT][NT], const bf16x8_v (&ah)[2][MT], const bf16x8_v (&al)[2][MT],
                                             const bf16x8_v (&bh)[2][NT], const bf16x8_v (&bl)[2][NT]) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        if constexpr (NS == 3) {
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j) acc[i][j] = CDF_MFMA_BF16(al[ks][i], bh[ks][j], acc[i][j]);
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j) acc[i][j] = CDF_MFMA_BF16(ah[ks][i], bl[ks][j], acc[i][j]);
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j) acc[i][j] = CDF_MFMA_BF16(ah[ks][i], bh[ks][j], acc[i][j]);
        } else {
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j) cdf_mma_sp<NS>(acc[i][j], ah[ks][i], al[ks][i], bh[ks][j], bl[ks][j]);
        }
    }
}

// The 16 x 16 x 32 form (f32x4q_t accumulators, same output tile per wave and same register counts): one MFMA spans the whole 32-deep K chunk,
// so the first index of a fragment array is the 16-row half of the 32-row block instead of the k16 step -- ah[a][i] = rows 32 i + 16 a of
// the wave's A tile, bh[b][j] = rows 32 j + 16 b of its B tile -- and a chunk is 4 MFMAs per 32 x 32 block and term instead of 2.  Term-major
// like above; per accumulator the order is al*bh, ah*bl, ah*bh.
template <int NS, int MT, int NT>
__device__ __forceinline__ void cdf_mma_tile(f32x4q_t (&acc)[MT][NT], const bf16x8_v (&ah)[2][MT], const bf16x8_v (&al)[2][MT],
                                             const bf16x8_v (&bh)[2][NT], const bf16x8_v (&bl)[2][NT]) {
    auto term = [&](const bf16x8_v (&x)[2][MT], const bf16x8_v (&y)[2][NT]) {
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int b = 0; b < 2; ++b) acc[i][j].q[a][b] = CDF_MFMA16_BF16(x[a][i], y[b][j], acc[i][j].q[a][b]);
    };
    if constexpr (NS == 3) {
        term(al, bh);
        term(ah, bl);
    }
    term(ah, bh);
}
// the accumulator block of a K loop that runs on MFMA shape MF (32: 32 x 32 x 16, 16: 16 x 16 x 32)
template <int MF> struct cdf_acc_of { typedef f32x16_t type; };
template <> struct cdf_acc_of<16> { typedef f32x4q_t type; };

// ---- what the K loops of the pre-split forward kernels (k_conv_spx / k_conv_halo / k_conv_rowhalo.hip) share --------------------------------
// Operand planes in LDS are [rows][CDF_SP_RE bf16 = 64 B], filled by LDS-DMA in 16-row segments (one wave instruction each) and XOR-swizzled
// on both sides: the 16-byte column c of row r lives at column c ^ cdf_swz<MF>(r), by the MFMA shape MF of the kernel that reads it.
//   MF = 32: (r >> 2) & 3.  A lane reads row r0 + (l & 31) at K block 2 ks + (l >> 5): each ds_read_b128 lane group is 16 rows of ONE K block,
//     four per class r mod 4 with four distinct (r >> 2) & 3 -- all 64 banks once (k_conv_spx.hip).
//   MF = 16: ((r >> 2) & 1) << 1.  A lane reads row r0 + (l & 15) at K block l >> 4.  ds_read_b128 serves the lanes in the groups {0-3, 12-15,
//     20-27}, {4-11, 16-19, 28-31} and the same + 32: a group is rows r0 + {0-3, 12-15} at K block kb and rows r0 + {4-11} at kb ^ 1 (kb = 0,
//     1, 2, 3 for the four groups).  Banks repeat every 256 B = 4 rows, so the 16 lanes are conflict-free iff, in each class r mod 4, the four
//     rows of the group -- one from each quad of rows, T, T + 1, T + 2, T + 3 = r >> 2 -- land in four distinct 16-byte columns:
//         f(T) ^ kb,  f(T + 3) ^ kb,  f(T + 1) ^ kb ^ 1,  f(T + 2) ^ kb ^ 1   all distinct, for every T (r0 is any row of a halo image).
//     (r >> 2) & 3 gives T, T + 3, T, T + 3: 2-way.  Distinctness of f(T + 1), f(T + 2) and of f(T), f(T + 1) ^ 1 for every T says that
//     consecutive quads differ in bit 1 of f; then f(T) and f(T + 2) ^ 1 share bit 1 and must agree in bit 0.  f(T) = (T & 1) << 1 is the
//     simplest such map: the four columns are {0, 2, 3, 1} ^ kb (T even) or {2, 0, 1, 3} ^ kb (T odd).
constexpr int CDF_SP_RE = 32;
template <int MF = 32>
__device__ __forceinline__ int cdf_swz(int row) { return MF == 16 ? ((row >> 2) & 1) << 1 : (row >> 2) & 3; }
// this lane's DMA slot inside a segment: row lane >> 2 (segments start at multiples of 16 rows: cdf_swz(row) = cdf_swz(lane >> 2)), and the
// global 16-byte column (as an element offset) that lands in LDS column lane & 3
__device__ __forceinline__ int cdf_dma_row(int lane) { return lane >> 2; }
template <int MF = 32>
__device__ __forceinline__ int cdf_dma_col(int lane) { return ((lane & 3) ^ cdf_swz<MF>(lane >> 2)) * 8; }
// weight row n of a tile, clamped into the matrix (rows past Cout fetch the last row again; the epilogue never stores them) ...
__device__ __forceinline__ int cdf_w_row(int n, int Cout) { return n < Cout ? n : Cout - 1; }
// ... and the element offset of its K column k for weight slab (tap) wi
__device__ __forceinline__ size_t cdf_w_off(int wi, int Cout, int row, int ldk, int k) {
    return (size_t)((unsigned)wi * (unsigned)Cout + (unsigned)row) * (unsigned)ldk + (unsigned)k;
}
// the 16-row DMA segments of an R-row LDS image shared out over NW waves: wave w takes segments w + NW q, q < PER_WAVE; past NSEG it repeats
// segment g mod NSEG -- same bytes to the same place, so that every wave issues the same number of DMA instructions and one wait count fits all
template <int R, int NW>
struct CdfDmaSegs {
    static constexpr int NSEG = (R + 15) / 16, ROWS = NSEG * 16, PER_WAVE = (NSEG + NW - 1) / NW;
    static __device__ __forceinline__ int seg(int wave, int q) {
        int g = wave + NW * q;
        if (g >= NSEG) g -= (g / NSEG) * NSEG;
        return g;
    }
};
// the first step of a de-phased ("late") wave multiplies zeros
template <int MT, int NT>
__device__ __forceinline__ void cdf_frag_zero(bf16x8_v (&ah)[2][MT], bf16x8_v (&al)[2][MT], bf16x8_v (&bh)[2][NT], bf16x8_v (&bl)[2][NT]) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int e = 0; e < 8; ++e) { ah[ks][i][e] = 0; al[ks][i][e] = 0; }
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int e = 0; e < 8; ++e) { bh[ks][j][e] = 0; bl[ks][j][e] = 0; }
    }
}
// Fragments of k-step ks out of a DMA-filled plane pair (hi at s, lo at s + PLANE): tile rows row + 32 t, t < T, where row = the wave's
// first row + (lane & 31) and sw = ((lane & 31) >> 2) & 3 its swizzle (tile row offsets are multiples of 32).
// MF = 16: ks is the 16-row half of the 32-row blocks instead, row = the wave's first row + 16 ks + (lane & 15), sw = cdf_swz<16>(row),
// and the lane's K block is lane >> 4 = 2 half + (l31 >> 4), passed in place of half.
template <int NS, int PLANE, int T, int MF = 32>
__device__ __forceinline__ void cdf_read_frags(bf16x8_v (&fh)[T], bf16x8_v (&fl)[T], const unsigned short* s, int ks, int half, int row, int sw) {
    const int kc = ((MF == 16 ? half : ks * 2 + half) ^ sw) * 8;
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const int off = (row + t * 32) * CDF_SP_RE + kc;
        fh[t] = *(const bf16x8_v*)(s + off);
        if constexpr (NS == 3) fl[t] = *(const bf16x8_v*)(s + PLANE + off);
    }
}
// ... out of a row-pitched halo image: fragment t reads image rows rows[t] + shift (the tap's pixel offset), each with its own swizzle
// (MF = 16: rows[t] belongs to the lane's 16-row half, and `half` is its K block lane >> 4, as above)
template <int NS, int PLANE, int T, int MF = 32>
__device__ __forceinline__ void cdf_read_frags_halo(bf16x8_v (&fh)[T], bf16x8_v (&fl)[T], const unsigned short* s, int ks, int half, const int (&rows)[T], int shift) {
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const int row = rows[t] + shift;
        const int off = row * CDF_SP_RE + ((MF == 16 ? half : ks * 2 + half) ^ cdf_swz<MF>(row)) * 8;
        fh[t] = *(const bf16x8_v*)(s + off);
        if constexpr (NS == 3) fl[t] = *(const bf16x8_v*)(s + PLANE + off);
    }
}
// One K step of a wave.  De-phased waves (SpxArgs.dephase): the waves 4..7 of an 8-wave block share their SIMDs with waves 0..3 and the step
// barrier keeps all eight in lockstep, so fragment reads / DMA issue (LDS, vector memory) and MFMAs (matrix pipe) of a SIMD's two waves used to
// happen one after the other, never together.  A late wave therefore multiplies the fragments it read in the PREVIOUS step first and reads this
// step's fragments afterwards: while one wave of a SIMD multiplies, the other one reads.  late is wave-uniform.
template <class Read, class Mma>
__device__ __forceinline__ void cdf_dephased_step(bool late, Read&& read, Mma&& mma) {
    if (late) {
        mma();
        CDF_SCHED_FENCE();                                   // (the reads overwrite the fragments just multiplied: hoisting them doubles the live set)
    }
    read();
    if (!late) mma();
}

// ---- LDS layouts: ONE statement per kernel form, read by the kernel (offsets, in bf16 elements) and by its launcher (bytes) --------------------
constexpr size_t CDF_LDS_BYTES = 160 * 1024;
constexpr int CDF_SP_PLANES = 2;                             // operand planes every stage reserves (hi, lo) -- the NS = 1 kernels too
constexpr size_t cdf_max_sz(size_t a, size_t b) { return a > b ? a : b; }
// generic kernel: NSTAGE x (A hi, A lo, B hi, B lo) | tap table; the epilogue tile [BM][BN + 8] floats aliases all of it
template <int BM, int BN, int NSTAGE>
struct SpxLayout {
    static constexpr int PLANE_A = BM * CDF_SP_RE, PLANE_B = BN * CDF_SP_RE;
    static constexpr int OFF_B = CDF_SP_PLANES * PLANE_A, STAGE = OFF_B + CDF_SP_PLANES * PLANE_B;
    static constexpr int OFF_TAPS = NSTAGE * STAGE;          // CDF_MAX_TAPS + 1 ints
    static constexpr size_t bytes = cdf_max_sz((size_t)OFF_TAPS * sizeof(unsigned short) + (CDF_MAX_TAPS + 1) * sizeof(int), (size_t)BM * (BN + 8) * sizeof(float));
    static_assert(bytes <= CDF_LDS_BYTES, "tile does not fit the LDS");   // 128 x 128 x 2 stages: 68 KB (epilogue tile), two blocks per CU;
};                                                                        // 256 x 128 x 3 stages: 144 KB, one block per CU
// halo kernel: halo 0 | halo 1 | NB weight stages (as many as fit, at most 6); the epilogue tile aliases all of it
template <int W, int BN, int BM>
struct HaloLayout {
    static constexpr int TH = BM / W, HW2 = W + 2, HR = (TH + 2) * HW2;   // halo rows (pixels)
    typedef CdfDmaSegs<HR, 8> Segs;
    static constexpr int PLANE_A = Segs::ROWS * CDF_SP_RE, ABUF = CDF_SP_PLANES * PLANE_A;
    static constexpr int PLANE_B = BN * CDF_SP_RE, BSTAGE = CDF_SP_PLANES * PLANE_B;
    static constexpr int OFF_B = 2 * ABUF;
    static constexpr int NBfit = (int)((CDF_LDS_BYTES - 64 - OFF_B * sizeof(unsigned short)) / (BSTAGE * sizeof(unsigned short)));
    static constexpr int NB = NBfit > 6 ? 6 : NBfit;
    static_assert(NB >= 3, "halo tile leaves no room for three weight stages");
    static constexpr size_t bytes = cdf_max_sz((size_t)(OFF_B + NB * BSTAGE) * sizeof(unsigned short) + 16 * sizeof(int), (size_t)BM * (BN + 8) * sizeof(float));
    static_assert(bytes <= CDF_LDS_BYTES, "halo tile does not fit the LDS");
};
// row-halo stream kernel: rows 0 | weights 0 | weights 1 | rows 1 | weights 2 | ...; the staging tile [EROWS][BN + 8] floats starts at "rows 1":
// it aliases only what is idle during the epilogue (rows 1, weights 2 and the tail)
template <int W, int BN, int BM = 256>
struct RowHaloLayout {
    static constexpr int TH = BM / W, HW2 = W + 2, RH = TH * HW2;
    typedef CdfDmaSegs<RH, 8> Segs;
    static constexpr int PLANE_A = Segs::ROWS * CDF_SP_RE, ABUF = CDF_SP_PLANES * PLANE_A;
    static constexpr int PLANE_B = BN * CDF_SP_RE, BSTAGE = CDF_SP_PLANES * PLANE_B;
    static constexpr int OFF_A1 = ABUF + 2 * BSTAGE, OFF_B2 = OFF_A1 + ABUF, OFF_CS = OFF_A1;
    static constexpr int EROWS = BM / 2, CP = BN + 8;        // rows per epilogue pass, staging pitch
    static constexpr int a_off(int buf) { return buf ? OFF_A1 : 0; }
    static constexpr int b_off(int stage) { return stage == 2 ? OFF_B2 : ABUF + stage * BSTAGE; }
    static constexpr size_t bytes = (size_t)OFF_CS * sizeof(unsigned short) + cdf_max_sz((size_t)(ABUF + BSTAGE) * sizeof(unsigned short), (size_t)EROWS * CP * sizeof(float));
    static_assert(bytes <= CDF_LDS_BYTES, "streaming row-halo tile does not fit the LDS");
};

#define CDF_GLDS16_K(g, l) CDF_GLDS16(g, l)

struct SpxArgs {
    const unsigned short* x_hi;
    const unsigned short* x_lo;
    const unsigned short* zero;    // >= 16 zero bytes, 16-byte aligned
    const unsigned short* w_hi;
    const unsigned short* w_lo;
    float* y;
    const float* bias;
    const float* sbias;
    const float* res;
    float* pre;
    const float* mul;
    int ldx, ldk, ldy, ld_sbias, ldr, ldp, ldm;
    int B, H, W, Cin, OH, OW, Cout, QH, QW, os, is;
    int act, mul_mode, accumulate, nphase, vec;
    int taprot;                    // 1: a tile is one image row and the 9 taps are 3 row groups -> per-block row-group order (see kernel)
    int dephase;                   // 1: the two waves of a SIMD run half a K step apart (one reads fragments / issues DMA while the other multiplies)
    unsigned short* ys_hi;         // nullable: bf16 hi / lo planes of the output (pitch ld_ys), written by the epilogue
    unsigned short* ys_lo;
    int ld_ys;
    int ksplit;                    // > 1 (generic kernel, one phase): blockIdx.z takes ntaps / ksplit taps and writes its raw partial
    float* ks_ws;                  //      sums to ks_ws[z][m][ks_ld]; conv_splitk_finish_kernel adds them up and runs the epilogue
    int ks_ld;
    int io_bf;                     // CDF_IO_*_BF16 bits (cdf_epilogue.h): res / pre / mul are bf16 tensors (bf16 activation storage)
    int epi;                       // id of the specialised epilogue (cdf_epi_select; 0: the generic run-time-selected form)
    const float* ln_x;             // epi == CDF_EPI_LNBWD: LayerNorm input h (pitch ld_lnx), its statistics [M], the partial-sum output [tiles][2][Cout]
    const float* ln_mean;
    const float* ln_rstd;
    float* ln_part;
    int ld_lnx;
    CdfPhase ph[4];
};

// what cdf_epilogue_rows reads, for a raw store of the accumulator tile (split-K partial sums): rows m of a [M][ldy] slab
struct RawEpiArgs {
    int Cout, vec, os, QH, QW, OH, OW, ldy, ldp, ldm, ldr, ld_sbias, ld_ys, act, mul_mode, accumulate, io_bf;
    const float* bias;
    const float* sbias;
    float* pre;
    const float* mul;
    const float* res;
    unsigned short* ys_hi;
    unsigned short* ys_lo;
};

struct SpxWgradArgs {
    const unsigned short* a_hi;
    const unsigned short* a_lo;
    const unsigned short* b_hi;
    const unsigned short* b_lo;
    const unsigned short* zero;
    float* out;
    float* bsum;
    int lda, ldb, ldo;
    int B, QH, QW;
    int HA, WA, sa, HB, WB, sb;
    int CA, CB;
    int ntaps, nsplit, m_per_split, xcd_swizzle;
    signed char day[CDF_MAX_TAPS], dax[CDF_MAX_TAPS], dby[CDF_MAX_TAPS], dbx[CDF_MAX_TAPS];
};

// ---- tuning: an explicit, optional argument of the GEMM entry points (include/colddiff.h: cdf_gemm_tuning) -----------------------------
// No mutable process-wide state: a NULL pointer means these defaults, anything else is read once per call.  The choices only select
// between kernels / tile shapes that compute the same sums (fp32 summation order aside).
static const cdf_gemm_tuning kTuneDefault = {(int)sizeof(cdf_gemm_tuning), 0, 0, 0, 1, 1, 1, 47, 1, 0, 1, 1, 1, 1, 1, 0, 1};
static inline const cdf_gemm_tuning* cdf_tune(const cdf_gemm_tuning* t) { return (t && t->size == (int)sizeof(cdf_gemm_tuning)) ? t : &kTuneDefault; }
static inline bool cdf_tune_ok(const cdf_gemm_tuning* t) {
    if (!t) return true;
    const bool bm_ok = t->tile_bm == 0 || t->tile_bm == 64 || t->tile_bm == 128 || (t->tile_bm == 256 && (t->tile_bn == 0 || t->tile_bn == 128));
    const bool bn_ok = t->tile_bn == 0 || t->tile_bn == 64 || t->tile_bn == 128;
    return t->size == (int)sizeof(cdf_gemm_tuning) && bm_ok && bn_ok && (t->max_bm == 0 || t->max_bm == 128 || t->max_bm == 256) &&
           (t->halo_bm == 0 || t->halo_bm == 128 || t->halo_bm == 256) && t->halo >= 0 && t->halo <= 127 && t->halo_min_tiles >= 0 && t->resident_reserve >= 0 && t->resident_reserve <= 248 && (t->rowhalo_stream == 0 || t->rowhalo_stream == 1) && (t->epilogue == 0 || t->epilogue == 1);
}
#define CDF_TUNE_CHECK(t, who)                                                                                                          \
    CDF_REQUIRE(cdf_tune_ok(t), who ": bad cdf_gemm_tuning (size %d, expected %d; tile_bm 0/64/128/256 (256 with tile_bn 0/128), tile_bn 0/64/128, " \
                                    "max_bm 0/128/256, halo_bm 0/128/256, halo 0..127, rowhalo_stream 0/1, resident_reserve 0..248, epilogue 0/1): start from cdf_gemm_tuning_default",            \
                (t) ? (t)->size : 0, (int)sizeof(cdf_gemm_tuning))

static inline int cdf_num_cus() {                                     // CUs of the current device (blocks of the resident kernels), a multiple of 8 XCDs
#ifdef CDF_EMU
    return 8;
#else
    static int n[64] = {0};                                  // per device ordinal (a process may drive several devices)
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    if (!n[dev]) {
        int cus = 0;
        n[dev] = (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus >= 8) ? cus / 8 * 8 : 256;
    }
    return n[dev];
#endif
}


// ---- plan-only dispatch (cdf_conv_gemm_bf16x_form / cdf_conv_wgrad_bf16x_form, include/colddiff.h) ------------------------------------------------
// The form queries run the dispatchers themselves: every launcher that is handed a CdfPlan records the kernel it was about to launch (the
// code colddiff.h documents, its tile count and its grid) and returns before CDF_LAUNCH.  There is no second copy of the conditions.
struct CdfPlan {
    int code, tiles, grid;
};
enum { CDF_FORM_ROWHALO = 1, CDF_FORM_HALO = 2, CDF_FORM_SPX = 3, CDF_FORM_WGRAD_ROW3 = 1, CDF_FORM_WGRAD_SPX = 2, CDF_FORM_WGRAD_STACK2 = 3 };
static inline int cdf_plan_set(CdfPlan* p, int form, int bm, int bn, int stages, int ksplit, int w, long long tiles, long long grid) {
    p->code = form << 24 | (bm / 64) << 20 | (bn / 64) << 16 | stages << 12 | ksplit << 4 | (w / 16);
    p->tiles = (int)tiles;
    p->grid = (int)grid;
    return CDF_OK;
}

// ---- cross-unit launchers (one plain function per kernel family; the template dispatch lives next to the kernels) --------------------------------
// halo kernel: W in {16, 32, 64, 128}, n64: 64-wide N tiles, bm: 128 or 256 pixel rows per tile (the caller has checked that the geometry fits)
int cdf_launch_igemm_halo(int ns, int W, bool n64, int bm, const SpxArgs& a, int M, hipStream_t s, CdfPlan* plan = nullptr);
// resident row-halo stream kernel; returns CDF_E_UNSUPPORTED when this build has no instance for W (the caller then falls through)
int cdf_launch_igemm_rowhalo(int ns, int W, bool n64, const SpxArgs& a, int M, hipStream_t s, int reserve, CdfPlan* plan = nullptr);
