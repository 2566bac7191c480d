// k_snow.hip -- the Snow forward process of the snowification package (snowification/diffusion/forward_process_impl.py:220-372):
// the motion-blurred snow planes of every step (cdf_snow_layers) and the degradation itself (cdf_snow_chain).
//
// Snow.forward(x, i, og=) never reads x: the state after any number of steps is a pointwise function of the ORIGINAL image and the
// index of the last step,
//     og_r   = (og + 1) / 2
//     gray   = (0.299 r + 0.587 g) + 0.114 b                     (kornia's rgb_to_grayscale of og_r)
//     gray   = max(og_r, gray * 1.5 + 0.5)                       (per channel)
//     scaled = br[i] * og_r + (1 - br[i]) * gray                 (og_r itself with fix_brightness)
//     D(og, i) = clip((scaled + snow[i]) + snow_rot[i], 0, 1) * 2 - 1
// with snow_rot[i] the plane rotated by 180 degrees, i.e. read at the mirrored index H*W - 1 - p.  The reference walks there through up to
// T passes of about ten elementwise launches each, a torch.stack of every intermediate batch and a gather per row; here q_sample, a reverse
// step of either sampling routine and the forward leg of sample() are one launch each: 12 B of image read, 8 B of snow read from tables
// that stay in L2, 12 B written per pixel.
//
// Arithmetic: plain fp32 in the order written above (the file is compiled with -ffp-contract=off like every other one), so the chain is
// bit-equal to the torch expressions evaluated on the same planes.
#include "cdf_common.h"
#include "colddiff.h"

// ---- the snow planes -------------------------------------------------------------------------------------------------------------------
// One output pixel per lane: out[t][l][y][x] = sum_j w_j * v(src_j), j ascending in fp32, where v = clip(base < thres[t] ? 0 : base, 0, 1)
// is applied as each source pixel is read (no thresholded plane is ever written) and out-of-image sources contribute 0 (padding='same').
// Horizontal: src_j = (y, x + j - k/2), w_j = taps[t][j]; vertical (torch.rot90 of the one-row kernel): src_j = (y + j - k/2, x),
// w_j = taps[t][k - 1 - j].  blockIdx.y = t * L + l, so thres, the taps and the flag are block-uniform.
__global__ void __launch_bounds__(256) snow_layers_kernel(const float* __restrict__ base, const float* __restrict__ thres,
                                                          const float* __restrict__ taps, const unsigned char* __restrict__ vertical,
                                                          float* __restrict__ snow, int H, int W, int L, int k) {
    const int plane = blockIdx.y;
    const int t = plane / L, l = plane - t * L;
    const float th = thres[t];
    const float* w = taps + (size_t)t * k;
    const bool vert = vertical[plane] != 0;
    const int HW = H * W, half = k / 2;
    const float* src = base + (size_t)l * HW;
    float* dst = snow + (size_t)plane * HW;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < HW; p += gridDim.x * blockDim.x) {
        const int y = p / W, x = p - y * W;
        float acc = 0.f;
        for (int j = 0; j < k; ++j) {
            const int yy = vert ? y + j - half : y, xx = vert ? x : x + j - half;
            const bool in = yy >= 0 && yy < H && xx >= 0 && xx < W;
            float v = in ? src[yy * W + xx] : 0.f;
            v = v < th ? 0.f : v;
            v = fminf(fmaxf(v, 0.f), 1.f);
            const float wj = vert ? w[k - 1 - j] : w[j];
            acc = acc + wj * v;
        }
        dst[p] = acc;
    }
}

// ---- the chain -------------------------------------------------------------------------------------------------------------------------
struct SnowArgs {
    const float* og;
    const float* start;    // nullable: og
    float* y;
    float* total;          // nullable
    float* snap;           // nullable
    const float* img;      // nullable: Algorithm-2 combine
    const float* snow;     // [T][L][HW]
    const float* br;       // [T] float32(br_coef)
    const float* omb;      // [T] float32(1.0 - br_coef)
    const int64_t* nb;     // nullable: per-row step counts
    const int64_t* layer;  // nullable: per-row layer
    long long HW;
    int L, T, nsteps, nmax, fix;
};

// D(og, i) on one pixel's three channels; s / r: the plane at the pixel and at its mirror
__device__ __forceinline__ void cdf_snow_px(float (&o)[3], const float (&c)[3], float s, float r, float br, float omb, bool fix) {
    const float r0 = (c[0] + 1.0f) / 2.0f, r1 = (c[1] + 1.0f) / 2.0f, r2 = (c[2] + 1.0f) / 2.0f;
    const float gray = ((0.299f * r0 + 0.587f * r1) + 0.114f * r2) * 1.5f + 0.5f;
    const float rr[3] = {r0, r1, r2};
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float g = fmaxf(rr[ch], gray);
        const float scaled = fix ? rr[ch] : br * rr[ch] + omb * g;
        const float v = (scaled + s) + r;
        o[ch] = fminf(fmaxf(v, 0.0f), 1.0f) * 2.0f - 1.0f;
    }
}

// which state an output holds: count n < 0: the row of og (passed through), 0: start, >= 1: D(og, n - 1)
template <bool VEC>
__device__ __forceinline__ void cdf_snow_state(float (&o)[3][VEC ? 4 : 1], const SnowArgs& a, int n, bool pass, const float* plane0, size_t o3,
                                               long long p, const float (&c)[3][VEC ? 4 : 1]) {
    constexpr int NP = VEC ? 4 : 1;
    const long long HW = a.HW;
    if (pass || (n == 0 && !a.start)) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
#pragma unroll
            for (int j = 0; j < NP; ++j) o[ch][j] = c[ch][j];
        return;
    }
    if (n == 0) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            if constexpr (VEC) {
                const float4 v = *(const float4*)(a.start + o3 + (size_t)ch * HW);
                o[ch][0] = v.x; o[ch][1] = v.y; o[ch][2] = v.z; o[ch][3] = v.w;
            } else {
                o[ch][0] = a.start[o3 + (size_t)ch * HW];
            }
        }
        return;
    }
    const int i = n - 1;
    const float* plane = plane0 + (size_t)i * a.L * (size_t)HW;
    const float br = a.br[i], omb = a.omb[i];
    float s[NP], r[NP];
    if constexpr (VEC) {
        // the four mirrored pixels HW-1-p .. HW-4-p are the aligned group at HW-4-p, reversed in registers
        const float4 sv = *(const float4*)(plane + p);
        const float4 mv = *(const float4*)(plane + (HW - 4 - p));
        s[0] = sv.x; s[1] = sv.y; s[2] = sv.z; s[3] = sv.w;
        r[0] = mv.w; r[1] = mv.z; r[2] = mv.y; r[3] = mv.x;
    } else {
        s[0] = plane[p];
        r[0] = plane[HW - 1 - p];
    }
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const float cc[3] = {c[0][j], c[1][j], c[2][j]};
        float oo[3];
        cdf_snow_px(oo, cc, s[j], r[j], br, omb, a.fix != 0);
        o[0][j] = oo[0]; o[1][j] = oo[1]; o[2][j] = oo[2];
    }
}

// VEC: H * W is a multiple of 4 and every pointer is 16-byte aligned; one lane = all three channels of four consecutive pixels.
// Otherwise one lane = the three channels of one pixel.  blockIdx.y = the row: counts, layer, br and omb are block-uniform.
template <bool VEC>
__global__ void __launch_bounds__(256) snow_chain_kernel(SnowArgs a) {
    constexpr int NP = VEC ? 4 : 1;
    const int b = blockIdx.y;
    const long long raw = a.nb ? (long long)a.nb[b] : (long long)a.nsteps;
    const bool pass = raw < 0;
    const int n = pass ? 0 : (raw < a.T ? (int)raw : a.T);              // (a count beyond the tables would read past them: clamped)
    const int nt = a.nmax;
    int ns = n < a.nmax - 1 ? n : a.nmax - 1;
    ns = ns < 0 ? 0 : ns;
    long long lay = a.layer ? (long long)a.layer[b] : (a.L > 1 ? (long long)b : 0ll);
    lay = lay < 0 ? 0 : (lay >= a.L ? a.L - 1 : lay);                   // (a layer outside the table would read past it: clamped)
    const long long HW = a.HW;
    const float* plane0 = a.snow + (size_t)lay * (size_t)HW;
    const size_t rowbase = (size_t)b * 3 * (size_t)HW;
    const bool want_snap = a.snap || a.img;
    const long long nitems = VEC ? HW >> 2 : HW;
    for (long long it = (long long)blockIdx.x * blockDim.x + threadIdx.x; it < nitems; it += (long long)gridDim.x * blockDim.x) {
        const long long p = it * NP;
        const size_t o3 = rowbase + (size_t)p;
        float c[3][NP], yo[3][NP], so[3][NP], to[3][NP], im[3][NP];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            if constexpr (VEC) {
                const float4 v = *(const float4*)(a.og + o3 + (size_t)ch * HW);
                c[ch][0] = v.x; c[ch][1] = v.y; c[ch][2] = v.z; c[ch][3] = v.w;
                if (a.img) {
                    const float4 w = *(const float4*)(a.img + o3 + (size_t)ch * HW);
                    im[ch][0] = w.x; im[ch][1] = w.y; im[ch][2] = w.z; im[ch][3] = w.w;
                }
            } else {
                c[ch][0] = a.og[o3 + (size_t)ch * HW];
                if (a.img) im[ch][0] = a.img[o3 + (size_t)ch * HW];
            }
        }
        cdf_snow_state<VEC>(yo, a, n, pass, plane0, o3, p, c);
        if (want_snap) {
            if (ns == n) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch)
#pragma unroll
                    for (int j = 0; j < NP; ++j) so[ch][j] = yo[ch][j];
            } else {
                cdf_snow_state<VEC>(so, a, ns, pass, plane0, o3, p, c);
            }
        }
        if (a.total) {
            if (nt == n) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch)
#pragma unroll
                    for (int j = 0; j < NP; ++j) to[ch][j] = yo[ch][j];
            } else {
                cdf_snow_state<VEC>(to, a, nt, pass, plane0, o3, p, c);
            }
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            float out[NP];
#pragma unroll
            for (int j = 0; j < NP; ++j) out[j] = a.img ? (im[ch][j] - yo[ch][j]) + so[ch][j] : yo[ch][j];
            const size_t o = o3 + (size_t)ch * HW;
            if constexpr (VEC) {
                *(float4*)(a.y + o) = make_float4(out[0], out[1], out[2], out[3]);
                if (a.snap) *(float4*)(a.snap + o) = make_float4(so[ch][0], so[ch][1], so[ch][2], so[ch][3]);
                if (a.total) *(float4*)(a.total + o) = make_float4(to[ch][0], to[ch][1], to[ch][2], to[ch][3]);
            } else {
                a.y[o] = out[0];
                if (a.snap) a.snap[o] = so[ch][0];
                if (a.total) a.total[o] = to[ch][0];
            }
        }
    }
}

// ---- C entry points --------------------------------------------------------------------------------------------------------------------
extern "C" int cdf_snow_layers(const float* base, const float* thres, const float* taps, const unsigned char* vertical, float* snow, int H,
                               int W, int L, int T, int k, void* stream) {
    CDF_REQUIRE(base && thres && taps && vertical && snow, "cdf_snow_layers: null pointer");
    CDF_REQUIRE(H > 0 && W > 0 && (long long)H * W < (1ll << 30), "cdf_snow_layers: bad shape (H = %d, W = %d)", H, W);
    CDF_REQUIRE(L > 0 && T > 0 && T <= 1024 && (long long)T * L <= 65535, "cdf_snow_layers: T * L = %d * %d outside 1..65535", T, L);
    CDF_REQUIRE(k > 0 && k <= 63 && (k & 1), "cdf_snow_layers: k = %d is not an odd tap count up to 63", k);
    int gx = cdf_cdiv((long long)H * W, 256);
    gx = gx > 4096 ? 4096 : gx;
    CDF_LAUNCH(snow_layers_kernel, dim3(gx, T * L), dim3(256), 0, CDF_S, base, thres, taps, vertical, snow, H, W, L, k);
    return cdf_check_launch("snow_layers");
}

extern "C" int cdf_snow_chain(const float* og, const float* start, float* y, float* total, float* snap, const float* img, const float* snow,
                              const float* br, const float* omb, const int64_t* nsteps_b, const int64_t* layer_b, int B, long long HW, int L,
                              int T, int nsteps, int nmax, int fix_brightness, void* stream) {
    CDF_REQUIRE(og && y && snow && br && omb, "cdf_snow_chain: null pointer");
    CDF_REQUIRE(B > 0 && B <= 65535 && HW > 0 && HW < (1ll << 40), "cdf_snow_chain: bad shape (B = %d, HW = %lld)", B, HW);
    CDF_REQUIRE(T > 0 && T <= 1024, "cdf_snow_chain: T = %d outside 1..1024", T);
    CDF_REQUIRE(L > 0, "cdf_snow_chain: L = %d layers", L);
    CDF_REQUIRE(layer_b || L == 1 || B <= L, "cdf_snow_chain: %d rows but %d layers and no layer_b", B, L);
    CDF_REQUIRE(nmax >= 0 && nmax <= T, "cdf_snow_chain: nmax = %d exceeds the %d steps of the tables", nmax, T);
    CDF_REQUIRE(nsteps_b || (nsteps <= T), "cdf_snow_chain: nsteps = %d exceeds the %d steps of the tables", nsteps, T);
    CDF_REQUIRE(!(img && total), "cdf_snow_chain: combine and total exclude each other");
    SnowArgs a{og, start, y, total, snap, img, snow, br, omb, nsteps_b, layer_b, HW, L, T, nsteps, nmax, fix_brightness};
    const bool vec = (HW & 3) == 0 && (((uintptr_t)og | (uintptr_t)start | (uintptr_t)y | (uintptr_t)total | (uintptr_t)snap |
                                        (uintptr_t)img | (uintptr_t)snow) & 15) == 0;
    // one item per lane (the body is two dependent loads deep; waves in flight hide them), grid-stride beyond 2048 blocks per row
    int gx = cdf_cdiv(vec ? HW >> 2 : HW, 256);
    gx = gx < 1 ? 1 : (gx > 2048 ? 2048 : gx);
    const dim3 grid(gx, B), block(256);
    if (vec) CDF_LAUNCH(snow_chain_kernel<true>, grid, block, 0, CDF_S, a);
    else CDF_LAUNCH(snow_chain_kernel<false>, grid, block, 0, CDF_S, a);
    return cdf_check_launch("snow_chain");
}
