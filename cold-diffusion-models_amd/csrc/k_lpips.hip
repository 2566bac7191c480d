// k_lpips.hip — LPIPS v0.1 (Zhang et al. 2018, the `lpips` package, net = 'alex') on the device: the input scaling in front of the
// AlexNet feature stack and the distance arithmetic on its five taps.  The convolutions themselves are the conv GEMM kernels
// (colddiff/lpips.py); everything the metric adds to them is here.
//
// cdf_lpips_prep_nhwc: [B,3,H,W] NCHW in [-1, 1] (from01: in [0, 1], mapped 2 x - 1 first) -> (x - shift_c) / scale_c as the 4-channel
// NHWC map the conv kernels take (channel 3 zero).  The scaling is NOT folded into conv1: conv1 zero-pads in the scaled domain, a folded
// bias would be wrong in the two border rings of its output.
//
// cdf_lpips_layer: one tap of the distance,
//     dist[k][b] += (1 / HW) sum_p sum_c w_c (a_pc / (|a_p| + 1e-10) - b_pc / (|b_p| + 1e-10))^2,      |v_p| = sqrt(sum_c v_pc^2)
// for the originals' map a against K <= 4 candidate maps (the cdf_eval_pairs_partial pattern).  It is memory-bound and every map is read
// once: a group of G = 1 ... 64 lanes (a power of two, the smallest that holds the C / 4 channel quads in one or two float4 per lane) owns
// a pixel and keeps its channel vector of every map in registers for both passes -- norm, then difference.  The original's vector is
// normalised once and every candidate runs against it.  Lanes past C / 4 read quad 0 again and drop it: the pitch padding is never read.
// Per-pixel arithmetic is fp32 in the definition's order (norm, + eps, divide, subtract, square, weight); an all-zero pixel normalises to
// 0 / 1e-10 = 0.  The channel sums are fp32 (lane order, then the xor tree of the group); the sums over pixels are fp64: the group's first
// lane adds its pixels in order, the block folds its 256 lanes in one fixed tree -> partial[k][b][block], lpips_fold_kernel adds a
// pair's partials in block order, divides by HW and accumulates into dist.  No atomics: two runs are bit-identical, and every partial of a
// call is written by that call.
#include "cdf_common.h"
#include "colddiff.h"

#define LPIPS_MAX_BLOCKS 32             // blocks per image
#define LPIPS_EPS 1e-10f
// The loaded quad is used as it is (compile-time only, no instruction): without it the compiler sinks three of the four dwords of a load
// whose value a select may drop into a branch of their own.
#ifdef CDF_EMU
#define LPIPS_KEEP4(v) (void)(v)
#else
#define LPIPS_KEEP4(v) asm volatile("" : "+v"((v).x), "+v"((v).y), "+v"((v).z), "+v"((v).w))
#endif

__global__ void __launch_bounds__(256) lpips_prep_kernel(const float* x, float* y, int ldy, long long npix, int HW, int from01) {
    const float shift[3] = {-.030f, -.088f, -.188f}, scale[3] = {.458f, .448f, .450f};
    CDF_EW_LOOP(i, npix) {
        const long long b = i / HW;
        const float* src = x + (size_t)b * 3 * HW + (size_t)(i - b * HW);
        float v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float t = src[(size_t)c * HW];
            if (from01) t = 2.f * t - 1.f;
            v[c] = (t - shift[c]) / scale[c];
        }
        *(float4*)(y + (size_t)i * ldy) = make_float4(v[0], v[1], v[2], 0.f);
    }
}

// grid (nblk, B).  NV: float4 per lane and map (C <= 256: 1, else 2); K: candidate maps; lg = log2 G.
// Loads are unconditional (a load behind a per-lane condition is split into dwords behind branches): a lane without a quad or a group
// without a pixel reads quad 0 of a pixel of this image and a select drops the value.
template <int NV, int K>
__global__ void __launch_bounds__(256) lpips_layer_kernel(const float* A, const float* C0, const float* C1, const float* C2, const float* C3,
                                                         const float* w, int HW, int C, int ld, int lg, double* partial) {
    __shared__ double red[256];
    const int blk = blockIdx.x, b = blockIdx.y, nblk = gridDim.x, B = gridDim.y, tid = threadIdx.x;
    const int G = 1 << lg, gl = tid & (G - 1), grp = tid >> lg, ppb = 256 >> lg, nq = C >> 2;
    float wv[NV * 4];
    bool own[NV];
    int qoff[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int q = gl + (j << lg);
        own[j] = q < nq;
        qoff[j] = own[j] ? 4 * q : 0;
        const float4 t = *(const float4*)(w + qoff[j]);
        wv[4 * j] = own[j] ? t.x : 0.f; wv[4 * j + 1] = own[j] ? t.y : 0.f; wv[4 * j + 2] = own[j] ? t.z : 0.f; wv[4 * j + 3] = own[j] ? t.w : 0.f;
    }
    double acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
    // (block-uniform trip count: the group sums below are taken by every lane of the block)
    for (int p0 = blk * ppb; p0 < HW; p0 += nblk * ppb) {
        const int p = p0 + grp;
        const bool live = p < HW;
        const size_t off = ((size_t)b * HW + (live ? p : 0)) * ld;
        float4 ra[NV], rb[K][NV];
        // every load of the pixel is issued before the first use
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            ra[j] = *(const float4*)(A + off + qoff[j]);
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const float* ck = k == 0 ? C0 : k == 1 ? C1 : k == 2 ? C2 : C3;
                rb[k][j] = *(const float4*)(ck + off + qoff[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            LPIPS_KEEP4(ra[j]);
#pragma unroll
            for (int k = 0; k < K; ++k) LPIPS_KEEP4(rb[k][j]);
        }
        float av[NV * 4], bv[K][NV * 4];
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const bool ok = live && own[j];
            av[4 * j] = ok ? ra[j].x : 0.f; av[4 * j + 1] = ok ? ra[j].y : 0.f; av[4 * j + 2] = ok ? ra[j].z : 0.f; av[4 * j + 3] = ok ? ra[j].w : 0.f;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                bv[k][4 * j] = ok ? rb[k][j].x : 0.f; bv[k][4 * j + 1] = ok ? rb[k][j].y : 0.f;
                bv[k][4 * j + 2] = ok ? rb[k][j].z : 0.f; bv[k][4 * j + 3] = ok ? rb[k][j].w : 0.f;
            }
        }
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < NV * 4; ++e) s += av[e] * av[e];
        const float na = sqrtf(cdf_group_sum(s, G)) + LPIPS_EPS;
#pragma unroll
        for (int e = 0; e < NV * 4; ++e) av[e] = av[e] / na;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            float t = 0.f;
#pragma unroll
            for (int e = 0; e < NV * 4; ++e) t += bv[k][e] * bv[k][e];
            const float nb = sqrtf(cdf_group_sum(t, G)) + LPIPS_EPS;
            float d = 0.f;
#pragma unroll
            for (int e = 0; e < NV * 4; ++e) {
                const float df = av[e] - bv[k][e] / nb;
                d += wv[e] * (df * df);
            }
            d = cdf_group_sum(d, G);
            acc[k] += gl == 0 && live ? (double)d : 0.0;
        }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double v = cdf_block_sum_f64(red, acc[k]);
        if (tid == 0) partial[((size_t)k * B + b) * nblk + blk] = v;
    }
}

// one thread per (candidate set, image): its partials in block order
__global__ void __launch_bounds__(256) lpips_fold_kernel(const double* partial, int pairs, int nblk, int HW, double* dist) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= pairs) return;
    const double* src = partial + (size_t)i * nblk;
    double s = 0.0;
    for (int j = 0; j < nblk; ++j) s += src[j];
    dist[i] += s / (double)HW;
}

static int lpips_log2_group(int C) {           // lanes per pixel: the smallest power of two that holds C / 4 quads in 1 (C <= 256) or 2 float4 each
    const int nq = C / 4, per = nq > 64 ? (nq + 1) / 2 : nq;
    int lg = 0;
    while ((1 << lg) < per) ++lg;
    return lg;
}

extern "C" int cdf_lpips_layer_blocks(int HW, int C) {
    if (HW < 1 || C < 4 || C > 512 || C % 4) return 0;
    const int b = cdf_cdiv(HW, 256 >> lpips_log2_group(C));
    return b < LPIPS_MAX_BLOCKS ? b : LPIPS_MAX_BLOCKS;
}

extern "C" int cdf_lpips_prep_nhwc(const float* x, float* y, int ldy, int B, int H, int W, int from01, void* stream) {
    CDF_REQUIRE(x && y, "cdf_lpips_prep_nhwc: null pointer");
    CDF_REQUIRE(B >= 1 && H >= 1 && W >= 1, "cdf_lpips_prep_nhwc: B, H and W must be at least 1 (got %d, %d, %d)", B, H, W);
    CDF_REQUIRE(ldy >= 4 && ldy % 4 == 0 && (((uintptr_t)y) & 15) == 0, "cdf_lpips_prep_nhwc: y must be 16B aligned with ldy %% 4 == 0, ldy >= 4 (got ldy = %d)", ldy);
    const long long npix = (long long)B * H * W;
    CDF_LAUNCH(lpips_prep_kernel, dim3(cdf_ew_grid4k(npix)), dim3(256), 0, CDF_S, x, y, ldy, npix, H * W, from01 ? 1 : 0);
    return cdf_check_launch("lpips_prep_nhwc");
}

extern "C" int cdf_lpips_layer(const float* a, const float* c0, const float* c1, const float* c2, const float* c3, int K, int ld,
                               const float* w, int B, int HW, int C, double* partial, double* dist, void* stream) {
    CDF_REQUIRE(K >= 1 && K <= 4, "cdf_lpips_layer: K must be 1...4 candidate maps (got %d)", K);
    const float* c[4] = {c0, c1, c2, c3};
    for (int k = 0; k < K; ++k) CDF_REQUIRE(c[k] && (((uintptr_t)c[k]) & 15) == 0, "cdf_lpips_layer: null or unaligned pointer (candidate %d of %d)", k, K);
    CDF_REQUIRE(a && w && partial && dist, "cdf_lpips_layer: null pointer");
    CDF_REQUIRE(((((uintptr_t)a) | ((uintptr_t)w)) & 15) == 0, "cdf_lpips_layer: a and w must be 16B aligned");
    CDF_REQUIRE(C % 4 == 0 && C >= 4 && C <= 512, "cdf_lpips_layer: C must be a multiple of 4 in [4, 512] (got %d)", C);
    CDF_REQUIRE(ld % 4 == 0 && ld >= C, "cdf_lpips_layer: ld must be a multiple of 4, at least C (got ld = %d, C = %d)", ld, C);
    CDF_REQUIRE(B >= 1 && B <= 65535 && HW >= 1, "cdf_lpips_layer: B must be in [1, 65535] and HW at least 1 (got B = %d, HW = %d)", B, HW);
    const int lg = lpips_log2_group(C), nblk = cdf_lpips_layer_blocks(HW, C);
#define LPIPS_GO(NV, KK) CDF_LAUNCH((lpips_layer_kernel<NV, KK>), dim3(nblk, B), dim3(256), 0, CDF_S, a, c0, c1, c2, c3, w, HW, C, ld, lg, partial)
#define LPIPS_GO_K(NV) do { if (K == 1) LPIPS_GO(NV, 1); else if (K == 2) LPIPS_GO(NV, 2); else if (K == 3) LPIPS_GO(NV, 3); else LPIPS_GO(NV, 4); } while (0)
    if (C > 256) LPIPS_GO_K(2);
    else LPIPS_GO_K(1);
    CDF_LAUNCH(lpips_fold_kernel, dim3(cdf_cdiv((long long)K * B, 256)), dim3(256), 0, CDF_S, (const double*)partial, K * B, nblk, HW, dist);
    return cdf_check_launch("lpips_layer");
}
