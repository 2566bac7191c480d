// k_attn_kvctx.hip — LinearAttention forward: the k | v projection and the per-head context in one pass over the pixels.  A unit of its
// own next to k_attn.hip because it is a split-precision GEMM: it needs the MFMA and operand-split helpers of cdf_conv_sp.h.
#include "cdf_conv_sp.h"

// ================================================================================================
// LinearAttention forward, k | v projection + context in ONE pass (round 2).
//
// kv = xn . Wkv^T is a K = dim <= 128 GEMM onto 256 channels: as a convolution launch it writes 1 KB per pixel, and the context
// pass (softmax over the pixels of k, then k~^T v per head) reads it all back.  Here a block keeps a 128-pixel x 256-channel
// tile -- ALL of k | v of its pixels -- : in-kernel-split operands exactly as conv_igemm_sp_kernel (xn fp32 -> bf16 hi / lo while it
// is staged, weights pre-split), accumulators -> an LDS staging tile [128][256] that aliases the operand stages, from which
//   * the tile leaves as full 1 KB rows (kv is still needed by the backward pass), and
//   * each head's context partial is updated on the spot (online softmax: running column max m, acc = acc * exp(m_old - m) +
//     exp(k - m)^T v on the fp32 matrix cores, running column sums), two waves per head, 64 pixels each.
// A block walks a contiguous run of tiles of ONE image and writes one partial per head at the end; cdf_linattn_finalize
// (k_attn.hip) folds the partials of an image.  k and v are never re-read: 537 -> 0 MB per micro-batch at 128 x 128.
// 8 waves: GEMM wave (wm = w / 4: pixel half, wn = w % 4: channel quarter), context wave (head w / 2, pixel half w % 2).
// ================================================================================================
struct KvCtxArgs {
    const float* xn;
    const unsigned short* w_hi;
    const unsigned short* w_lo;
    float* kv;
    float* max_part;      // [B][P][HD]
    float* ctx_part;      // [B][P][heads][32][32]
    float* sum_part;      // [B][P][HD]
    int ldx, ldk, ldkv;
    int n, dim, P, tiles_per_block;
};

// BK = 64 when dim % 64 == 0 (a dim = 64 tile is ONE chunk: all of the next tile's operands travel during the current tile's store /
// context phase), else 32.  One LDS operand stage (the next chunk waits in registers), aliased by the staging tile.
template <int SPLIT, int BK>
__global__ void __launch_bounds__(512, 1) linattn_kvctx_kernel(KvCtxArgs a) {
    constexpr int BM = 128, BN = 256, AS = BK + 8;           // AS: LDS row stride in bf16 elements
    constexpr int NPL = SPLIT == 1 ? 1 : 2;
    constexpr int PLANE_A = BM * AS, PLANE_B = BN * AS;
    constexpr int SP = BN + 8;                               // staging row pitch (floats)
    constexpr int HD = 128, LD = 32;
    constexpr int AV = BK / 4, AQ = BM * AV / 512;           // float4 per A row, A loads per thread
    constexpr int BV = BK / 8, BQ = BN * BV / 512;           // uint4 per B row and plane, B loads per thread and plane
    CDF_DYN_SMEM(smem_raw);
    unsigned short* smem = (unsigned short*)smem_raw;        // operand stage [A planes | B planes] ...
    float* stg = (float*)smem_raw;                           // ... aliased by the [128][SP] fp32 staging tile
    float* sstat = (float*)(smem_raw + (size_t)BM * SP * sizeof(float));     // [2 pixel halves][128] column maxima of k

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 2, wn = wave & 3;
    const int half = lane >> 5, l31 = lane & 31;
    const int b = blockIdx.y, p = blockIdx.x;
    const int tiles = a.n / BM;
    const int t_lo = p * a.tiles_per_block;
    int t_hi = t_lo + a.tiles_per_block;
    if (t_hi > tiles) t_hi = tiles;
    const int nch = a.dim / BK;
    const float* xb = a.xn + (size_t)b * a.n * a.ldx;
    float* kvb = a.kv + (size_t)b * a.n * a.ldkv;

    const int a_row = tid / AV, a_c4 = (tid % AV) * 4;       // + (512 / AV) rows per further load
    const int b_row = tid / BV, b_q = tid % BV;
    f32x4_t ra[AQ];
    u32x4_v rbh[BQ], rbl[BQ];
#pragma unroll
    for (int q = 0; q < BQ; ++q) rbl[q] = u32x4_v{0u, 0u, 0u, 0u};
    auto load_chunk = [&](int tile, int c) {
        const float* xa = xb + (size_t)tile * BM * a.ldx + c * BK + a_c4;
#pragma unroll
        for (int q = 0; q < AQ; ++q) ra[q] = *(const f32x4_t*)(xa + (size_t)(a_row + (512 / AV) * q) * a.ldx);
#pragma unroll
        for (int q = 0; q < BQ; ++q) {
            const size_t off = (size_t)(b_row + (512 / BV) * q) * a.ldk + c * BK + b_q * 8;
            rbh[q] = *(const u32x4_v*)(a.w_hi + off);
            if (SPLIT > 1) rbl[q] = *(const u32x4_v*)(a.w_lo + off);
        }
    };
    auto store_lds = [&]() {
#pragma unroll
        for (int q = 0; q < AQ; ++q) {
            uint2 hi, lo;
            const float4 v = make_float4(ra[q].x, ra[q].y, ra[q].z, ra[q].w);
            if (SPLIT > 1) {
                cdf_split4_trunc(v, hi, lo);
            } else {
                hi.x = cdf_f2bf(v.x) | (cdf_f2bf(v.y) << 16);
                hi.y = cdf_f2bf(v.z) | (cdf_f2bf(v.w) << 16);
                lo = hi;
            }
            const int off = (a_row + (512 / AV) * q) * AS + a_c4;
            *(uint2*)(smem + off) = hi;
            if (SPLIT > 1) *(uint2*)(smem + PLANE_A + off) = lo;
        }
        unsigned short* sb = smem + NPL * PLANE_A;
#pragma unroll
        for (int q = 0; q < BQ; ++q) {
            const int off = (b_row + (512 / BV) * q) * AS + b_q * 8;
            *(u32x4_v*)(sb + off) = rbh[q];
            if (SPLIT > 1) *(u32x4_v*)(sb + PLANE_B + off) = rbl[q];
        }
    };

    // ---- context state: waves 0-3 own one head each (all 128 pixels of a tile); waves 4-7 stream the tile out meanwhile
    const bool ctx_wave = wave < 4;
    const int ch = wave & 3;
    f32x16_t cacc;
    cdf_acc_zero(cacc);
    float m_run = -3.0e38f, psum = 0.f;                      // lane (i = l31): column d = i of this head (both pixel parities hold m_run)

    if (t_lo < t_hi) load_chunk(t_lo, 0);
    for (int tile = t_lo; tile < t_hi; ++tile) {
        f32x16_t acc[2][2];
        cdf_acc_zero(acc);
        for (int c = 0; c < nch; ++c) {
            if (c > 0) __syncthreads();                       // every wave is done with the previous chunk's fragments
            store_lds();
            __syncthreads();
            // what is needed next travels during the MFMAs (and, for the last chunk, during the store / context phase)
            if (c + 1 < nch) load_chunk(tile, c + 1);
            else if (tile + 1 < t_hi) load_chunk(tile + 1, 0);
            const unsigned short* sa = smem;
            const unsigned short* sb = sa + NPL * PLANE_A;
#pragma unroll
            for (int ks = 0; ks < BK / 16; ++ks) {
                const int k0 = ks * 16 + half * 8;
                bf16x8_v ah[2], al[2], bh[2], bl[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int off = (wm * 64 + i * 32 + l31) * AS + k0;
                    ah[i] = *(const bf16x8_v*)(sa + off);
                    if (SPLIT > 1) al[i] = *(const bf16x8_v*)(sa + PLANE_A + off);
                }
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int off = (wn * 64 + j * 32 + l31) * AS + k0;
                    bh[j] = *(const bf16x8_v*)(sb + off);
                    if (SPLIT > 1) bl[j] = *(const bf16x8_v*)(sb + PLANE_B + off);
                }
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        if (SPLIT > 1) {
                            acc[i][j] = CDF_MFMA_BF16(al[i], bh[j], acc[i][j]);
                            acc[i][j] = CDF_MFMA_BF16(ah[i], bl[j], acc[i][j]);
                        }
                        acc[i][j] = CDF_MFMA_BF16(ah[i], bh[j], acc[i][j]);
                    }
            }
        }
        __syncthreads();                                      // the operand stage is free: it becomes the staging tile
        // ---- accumulators -> staging tile [pixel][channel]; the k waves (channel quarters 0, 1) leave the column maxima of their
        //      64 pixels next to it
        cdf_acc_stage(stg, SP, wm * 64, wn * 64, acc, half, l31);
        if (wn < 2) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                float m = -3.0e38f;
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) m = fmaxf(m, acc[i][j][r]);
                m = fmaxf(m, __shfl_xor(m, 32));
                if (half == 0) sstat[wm * HD + wn * 64 + j * 32 + l31] = m;
            }
        }
        __syncthreads();
        if (!ctx_wave) {
            // ---- k | v rows out: 64 float4 = one 1 KB row per wave instruction (waves 4-7: the stores' back-pressure stalls nobody else)
            float* dst = kvb + (size_t)tile * BM * a.ldkv;
#pragma unroll 4
            for (int e = tid - 256; e < BM * (BN / 4); e += 256) {
                const int px = e >> 6, c4 = (e & 63) * 4;
                *(float4*)(dst + (size_t)px * a.ldkv + c4) = *(const float4*)(stg + px * SP + c4);
            }
        } else {
            // ---- context of head ch: acc = acc * exp(m_old - m) + exp(k - m)^T v over the tile's 128 pixels
            const float* kcol = stg + half * SP + ch * LD + l31;                       // pixel 2 s + half, column d = l31
            const float* vcol = kcol + HD;
            const float m_new = fmaxf(m_run, fmaxf(sstat[ch * LD + l31], sstat[HD + ch * LD + l31]));
            const float f = expf(m_run - m_new);                                       // (first tile: exp(-inf) = 0 on zero accumulators)
            // the factor of accumulator row d lives in lane d
#pragma unroll
            for (int r = 0; r < 16; ++r) cacc[r] *= __shfl(f, cdf_acc_row(r, half));
            psum *= f;
            m_run = m_new;
#pragma unroll 8
            for (int sx = 0; sx < 64; ++sx) {
                const float pk = expf(kcol[2 * sx * SP] - m_new);
                psum += pk;
                cacc = __builtin_amdgcn_mfma_f32_32x32x2f32(pk, vcol[2 * sx * SP], cacc, 0, 0, 0);
            }
        }
        __syncthreads();                                      // the staging tile (and sstat) are rewritten by the next trip
    }
    // ---- one partial per (block, head)
    psum += __shfl_xor(psum, 32);
    float* fold = stg;                                        // [4 heads][32][32], then [4][32] sums
    if (ctx_wave) {
        cdf_acc_stage(fold, LD, ch * LD, 0, cacc, half, l31);
        if (half == 0) fold[4 * LD * LD + ch * LD + l31] = psum;
    }
    __syncthreads();
    const size_t pb = (size_t)b * a.P + p;
    for (int e = tid; e < 4 * LD * LD; e += 512) a.ctx_part[pb * 4 * (LD * LD) + e] = t_lo < t_hi ? fold[e] : 0.f;
    if (tid < HD) a.sum_part[pb * HD + tid] = t_lo < t_hi ? fold[4 * LD * LD + tid] : 0.f;
    if (ctx_wave && half == 0) a.max_part[pb * HD + ch * LD + l31] = m_run;
}

// ================================================================================================
// blocks per image of cdf_linattn_kvctx (= partials per image and head for cdf_linattn_finalize)
extern "C" int cdf_linattn_kvctx_parts(int B, int n, int slots) {      // slots: target block count per launch (<= 0: the default, 512)
    const int tiles = n / 128;
    if (tiles < 1 || B < 1) return 0;
    int P = (slots > 0 ? slots : 512) / B;                        // default ~2 blocks per CU queued: a block's last tile overlaps another's start
    if (P < 1) P = 1;
    if (P > tiles) P = tiles;
    const int tpb = (tiles + P - 1) / P;
    return (tiles + tpb - 1) / tpb;
}

extern "C" int cdf_linattn_kvctx(const float* xn, int ldx, const void* w_hi, const void* w_lo, int ldk, float* kv, int ldkv, float* ws, int B,
                                 int n, int dim, int heads, int slots, void* stream) {
    CDF_REQUIRE(xn && w_hi && kv && ws && B > 0, "cdf_linattn_kvctx: null pointer");
    CDF_REQUIRE(heads == 4 && n >= 128 && n % 128 == 0 && dim >= 32 && dim % 32 == 0 && dim <= 512,
                "cdf_linattn_kvctx: 4 heads, n %% 128 == 0, dim a multiple of 32 (<= 512); got heads=%d n=%d dim=%d", heads, n, dim);
    CDF_REQUIRE(ldx % 4 == 0 && ldx >= dim && ldk % 8 == 0 && ldk >= dim && ldkv % 4 == 0 && ldkv >= 256 &&
                ((((uintptr_t)xn) | ((uintptr_t)w_hi) | ((uintptr_t)w_lo) | ((uintptr_t)kv)) & 15) == 0,
                "cdf_linattn_kvctx: pitches (xn % 4, weights % 8, kv % 4 and >= 256) / 16-byte alignment");
    const int P = cdf_linattn_kvctx_parts(B, n, slots), tiles = n / 128, HD = 128;
    KvCtxArgs a;
    a.xn = xn; a.w_hi = (const unsigned short*)w_hi; a.w_lo = (const unsigned short*)w_lo; a.kv = kv;
    a.max_part = ws;
    a.ctx_part = ws + (size_t)B * P * HD;
    a.sum_part = a.ctx_part + (size_t)B * P * heads * 1024;
    a.ldx = ldx; a.ldk = ldk; a.ldkv = ldkv; a.n = n; a.dim = dim; a.P = P;
    a.tiles_per_block = (tiles + P - 1) / P;
    const size_t lds = (size_t)128 * (256 + 8) * sizeof(float) + 8 * 32 * sizeof(float);
    if (dim % 64 == 0) {
        if (w_lo) CDF_LAUNCH_LDS((linattn_kvctx_kernel<3, 64>), dim3(P, B), dim3(512), lds, CDF_S, a);
        else CDF_LAUNCH_LDS((linattn_kvctx_kernel<1, 64>), dim3(P, B), dim3(512), lds, CDF_S, a);
    } else {
        if (w_lo) CDF_LAUNCH_LDS((linattn_kvctx_kernel<3, 32>), dim3(P, B), dim3(512), lds, CDF_S, a);
        else CDF_LAUNCH_LDS((linattn_kvctx_kernel<1, 32>), dim3(P, B), dim3(512), lds, CDF_S, a);
    }
    return cdf_check_launch("linattn_kvctx");
}
