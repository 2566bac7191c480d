// k_data.hip — device-side input pipeline.
//
// Replaces Dataset_Aug1 / Dataset + DataLoader of deblurring_diffusion_pytorch.py:983-1026, 1094-1096 (8-16 PIL worker
// processes: Resize 1.12x -> RandomCrop / CenterCrop -> RandomHorizontalFlip -> ToTensor -> t * 2 - 1).  The Resize of that
// chain is deterministic, so it is applied ONCE when the dataset is cached: the cache is [N][S][S][C] uint8 in HBM (S =
// int(1.12 image_size); CelebA's 202 599 images at S = 143 are 12.4 GB of the 288 GB).  Per batch ONE kernel does the rest:
// gather B cached images by index, crop at (oy, ox), mirror, and convert with exactly ToTensor's arithmetic
// (float(v) / 255, IEEE division) followed by t * 2 - 1 in fp32, writing the NCHW fp32 batch the diffusion classes take.
// HBM-bound and tiny: 49 KB read + 196 KB written per 128 x 128 image.
#include "cdf_common.h"
#include "colddiff.h"

__global__ void augment_batch_kernel(const unsigned char* cache, const long long* idx, const int* oy, const int* ox, const int* flip,
                                     float* out, int SH, int SW, int C, int pad, int H, int W) {
    // (oy, ox) address the image after RandomCrop's `padding=pad` border (zero fill); pad = 0 for the plain chains
    const int b = blockIdx.y, y = blockIdx.x;
    const int sy = oy[b] + y - pad;
    const bool row_in = sy >= 0 && sy < SH;
    const unsigned char* src = cache + ((size_t)idx[b] * SH + (size_t)(row_in ? sy : 0)) * SW * C;
    const int x0 = ox[b] - pad, fl = flip[b];
    float* dst = out + ((size_t)b * C * H + y) * W;          // + c * H * W + x
    for (int i = threadIdx.x; i < W * C; i += blockDim.x) {
        const int c = i / W, x = i - c * W;                  // consecutive lanes: consecutive x of one channel plane (coalesced stores)
        const int sx = x0 + (fl ? W - 1 - x : x);
        const bool in = row_in && sx >= 0 && sx < SW;
        const unsigned char u = src[(in ? sx : 0) * C + c];  // unconditional load from a clamped address, then select
        const float v = (float)(in ? u : (unsigned char)0) / 255.0f;     // ToTensor: uint8 -> float32, div(255)
        dst[(size_t)c * H * W + x] = v * 2.0f - 1.0f;        // Lambda(t * 2 - 1)   (no FMA contraction: -ffp-contract=off)
    }
}

extern "C" int cdf_augment_batch_pad(const void* cache, long long N, int SH, int SW, int C, int pad, const long long* idx, const int* oy,
                                     const int* ox, const int* flip, float* out, int B, int H, int W, void* stream) {
    CDF_REQUIRE(cache && idx && oy && ox && flip && out, "cdf_augment_batch: null pointer");
    CDF_REQUIRE(N > 0 && B > 0 && C >= 1 && C <= 4 && H > 0 && W > 0 && pad >= 0 && H <= SH + 2 * pad && W <= SW + 2 * pad,
                "cdf_augment_batch: bad geometry (crop %dx%d of %dx%d + %d border, %d channels)", H, W, SH, SW, pad, C);
    CDF_LAUNCH(augment_batch_kernel, dim3(H, B), dim3(256), 0, CDF_S, (const unsigned char*)cache, idx, oy, ox, flip, out, SH, SW, C, pad, H, W);
    return cdf_check_launch("augment_batch");
}

extern "C" int cdf_augment_batch(const void* cache, long long N, int S, int C, const long long* idx, const int* oy, const int* ox,
                                 const int* flip, float* out, int B, int H, int W, void* stream) {
    return cdf_augment_batch_pad(cache, N, S, S, C, 0, idx, oy, ox, flip, out, B, H, W, stream);
}

// ---- RandomResizedCrop -> RandomHorizontalFlip -> RandomApply([ColorJitter]) -> ToTensor -> t * 2 - 1 ------------------------------
// The `random_aug=True` chain of the decolorization / snowification packages (diffusion/diffusion.py:516-526), bit for bit as
// torchvision runs it on PIL images.  One workgroup owns one image, because ImageEnhance.Contrast blends with the grey mean of the WHOLE
// image as it is when the op runs.  The working image is three uint8 planes of H x W in LDS (48 KB at 128 x 128); a thread owns the same
// 4-pixel groups (one dword per plane: consecutive lanes, consecutive banks) from the resize to the store, so the only barriers are
// the ones around the coefficient tables and the grey sum.  Every reduction is an integer sum: run-to-run identical.
//
// Resize = Pillow's ImagingResample for 8-bit bands: per axis, coefficients in double normalised to their sum, rounded to 22 fractional
// bits; horizontal pass, rounded to uint8, then the vertical pass.  The tables (per image and output index) are built on the device into
// LDS; the horizontal taps of the few source rows an output pixel needs are recomputed per pixel, uint8 rounding included, so no
// intermediate image exists and the source size only bounds the tables' pitch.  The filter window is clamped to the CROP (torchvision
// crops, then resizes), not to the cached image.
#define CDF_JITTER_BITS 22
#define CDF_JITTER_LDS_CAP (160 * 1024)

// taps per output index of Pillow's bilinear filter for `in` source pixels at most: ceil(support) * 2 + 1
static inline int jitter_ksize(int in_max, int out) { return in_max <= out ? 3 : 2 * ((in_max + out - 1) / out) + 1; }
static inline size_t jitter_lds_bytes(int SH, int SW, int H, int W) {
    const size_t plane = ((size_t)H * W + 3) / 4 * 4;
    return 3 * plane + sizeof(int) * ((size_t)W * jitter_ksize(SW, W) + (size_t)H * jitter_ksize(SH, H) + 2 * (size_t)(W + H) + 16);
}

// precompute_coeffs + normalize_coeffs_8bpc of Pillow's Resample.c for output index xx (bilinear, box = the whole crop)
__device__ __forceinline__ void jitter_coeffs(int in, int out, int xx, int pitch, int* k, int* first, int* count) {
    if (in == out) {                                         // Pillow skips a pass that does not change the size
        k[0] = 1 << CDF_JITTER_BITS;
        *first = xx;
        *count = 1;
        return;
    }
    const double scale = (double)in / (double)out;
    const double fscale = scale < 1.0 ? 1.0 : scale;
    const double support = fscale, ss = 1.0 / fscale;
    const double center = (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in) xmax = in;
    const int n = xmax - xmin < pitch ? xmax - xmin : pitch;         // (never more than ceil(support) * 2 + 1 <= pitch taps: belt and braces)
    double ww = 0.0;
    for (int x = 0; x < n; ++x) {
        double w = (x + xmin - center + 0.5) * ss;
        w = w < 0.0 ? -w : w;
        ww += w < 1.0 ? 1.0 - w : 0.0;
    }
    for (int x = 0; x < n; ++x) {
        double w = (x + xmin - center + 0.5) * ss;
        w = w < 0.0 ? -w : w;
        w = w < 1.0 ? 1.0 - w : 0.0;
        if (ww != 0.0) w /= ww;
        k[x] = (int)(0.5 + w * (double)(1 << CDF_JITTER_BITS));
    }
    *first = xmin;
    *count = n;
}

__device__ __forceinline__ int jitter_clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
__device__ __forceinline__ int jitter_min(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int jitter_max(int a, int b) { return a > b ? a : b; }

// Image.blend(degenerate, image, alpha) on one band value (Pillow's Blend.c): float32 arithmetic, truncation; clipped only when
// alpha extrapolates
__device__ __forceinline__ int jitter_blend(int deg, int v, float alpha, bool inside) {
    const float t = (float)deg + alpha * (float)(v - deg);
    if (inside) return (int)t;
    return t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (int)t);
}

__device__ __forceinline__ int jitter_luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }   // convert('L')

// convert('HSV') -> h += shift (uint8 wrap) -> convert('RGB'), Pillow's rgb2hsv_row / hsv2rgb_row
__device__ __forceinline__ void jitter_hue(int& r, int& g, int& b, int shift) {
    const int maxc = jitter_max(r, jitter_max(g, b)), minc = jitter_min(r, jitter_min(g, b));
    int uh = 0, us = 0;
    const int uv = maxc;
    if (minc != maxc) {
        const float cr = (float)(maxc - minc);
        const float s = cr / (float)maxc;
        const float rc = (float)(maxc - r) / cr, gc = (float)(maxc - g) / cr, bc = (float)(maxc - b) / cr;
        float h;
        if (r == maxc) h = bc - gc;
        else if (g == maxc) h = (float)(2.0 + (double)rc - (double)bc);
        else h = (float)(4.0 + (double)gc - (double)rc);
        h = (float)fmod((double)h / 6.0 + 1.0, 1.0);
        uh = jitter_clip8((int)((double)h * 255.0));
        us = jitter_clip8((int)(s * 255.0f));
    }
    uh = (uh + shift) & 255;
    if (us == 0) {
        r = g = b = uv;
        return;
    }
    const double h6 = (double)uh * 6.0 / 255.0;
    const double fi = floor(h6);
    const double f = h6 - fi;
    const double fs = (double)us / 255.0;
    const int p = jitter_clip8((int)round((double)uv * (1.0 - fs)));
    const int q = jitter_clip8((int)round((double)uv * (1.0 - fs * f)));
    const int t = jitter_clip8((int)round((double)uv * (1.0 - fs * (1.0 - f))));
    switch ((int)fi % 6) {
        case 0: r = uv; g = t; b = p; break;
        case 1: r = q; g = uv; b = p; break;
        case 2: r = p; g = uv; b = t; break;
        case 3: r = p; g = q; b = uv; break;
        case 4: r = t; g = p; b = uv; break;
        default: r = uv; g = p; b = q; break;
    }
}

__global__ void __launch_bounds__(1024) augment_jitter_kernel(const unsigned char* cache, long long N, const long long* idx, const int* params,
                                                              float* out, int SH, int SW, int H, int W, int KW, int KH) {
    CDF_DYN_SMEM(smem);
    const int HW = H * W, nquad = (HW + 3) >> 2;
    unsigned* plane_r = (unsigned*)smem;                     // [nquad] dwords of 4 pixels each
    unsigned* plane_g = plane_r + nquad;
    unsigned* plane_b = plane_g + nquad;
    int* kx = (int*)(plane_b + nquad);                       // [W][KW]
    int* ky = kx + W * KW;                                   // [H][KH]
    int* x_first = ky + H * KH;                              // [W]
    int* x_count = x_first + W;
    int* y_first = x_count + W;                              // [H]
    int* y_count = y_first + H;
    int* wave_sum = y_count + H;                             // [16]

    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int* prm = params + (size_t)b * CDF_JITTER_STRIDE;
    // the host checked its copy of the parameters; the clamps keep every read inside the image whatever the device copy holds
    const int ch = jitter_min(jitter_max(prm[2], 1), SH), cw = jitter_min(jitter_max(prm[3], 1), SW);
    const int top = jitter_min(jitter_max(prm[0], 0), SH - ch), left = jitter_min(jitter_max(prm[1], 0), SW - cw);
    const int flip = prm[4];
    long long im = idx[b];
    im = im < 0 ? 0 : (im >= N ? N - 1 : im);
    const unsigned char* crop = cache + (((size_t)im * SH + top) * SW + left) * 3;
    const size_t row_pitch = (size_t)SW * 3;

    for (int i = tid; i < W + H; i += nt) {
        if (i < W) jitter_coeffs(cw, W, i, KW, kx + i * KW, x_first + i, x_count + i);
        else jitter_coeffs(ch, H, i - W, KH, ky + (i - W) * KH, y_first + i - W, y_count + i - W);
    }
    __syncthreads();

    // ---- crop + resize + mirror -> LDS -------------------------------------------------------------------------------------
    for (int q = tid; q < nquad; q += nt) {
        unsigned pr = 0, pg = 0, pb = 0;
        for (int e = 0; e < 4; ++e) {
            const int p = 4 * q + e;
            if (p >= HW) break;
            const int y = p / W, xo = p - y * W;
            const int x = flip ? W - 1 - xo : xo;
            const int xf = x_first[x], xn = x_count[x], yf = y_first[y], yn = y_count[y];
            const int* kxx = kx + x * KW;
            const int* kyy = ky + y * KH;
            int a0 = 1 << (CDF_JITTER_BITS - 1), a1 = a0, a2 = a0;
            for (int j = 0; j < yn; ++j) {
                const unsigned char* src = crop + (size_t)(yf + j) * row_pitch + (size_t)xf * 3;
                int h0 = 1 << (CDF_JITTER_BITS - 1), h1 = h0, h2 = h0;
                for (int i = 0; i < xn; ++i) {
                    const int k = kxx[i];
                    h0 += k * (int)src[3 * i];
                    h1 += k * (int)src[3 * i + 1];
                    h2 += k * (int)src[3 * i + 2];
                }
                const int k = kyy[j];                        // the horizontal pass rounds to uint8 before the vertical one reads it
                a0 += k * jitter_clip8(h0 >> CDF_JITTER_BITS);
                a1 += k * jitter_clip8(h1 >> CDF_JITTER_BITS);
                a2 += k * jitter_clip8(h2 >> CDF_JITTER_BITS);
            }
            pr |= (unsigned)jitter_clip8(a0 >> CDF_JITTER_BITS) << (8 * e);
            pg |= (unsigned)jitter_clip8(a1 >> CDF_JITTER_BITS) << (8 * e);
            pb |= (unsigned)jitter_clip8(a2 >> CDF_JITTER_BITS) << (8 * e);
        }
        plane_r[q] = pr;
        plane_g[q] = pg;
        plane_b[q] = pb;
    }

    // ---- ColorJitter: the ops in this image's order, each on the uint8 result of the one before --------------------------------------
    for (int o = 0; o < 4; ++o) {
        const int op = prm[5 + o];                           // block-uniform
        if (op < 0 || op > 3) continue;
        int mean = 0;
        if (op == 1) {                                       // ImageEnhance.Contrast: int(mean(convert('L')) + 0.5)
            int s = 0;
            for (int q = tid; q < nquad; q += nt) {
                const unsigned pr = plane_r[q], pg = plane_g[q], pb = plane_b[q];
                for (int e = 0; e < 4; ++e)
                    if (4 * q + e < HW) s += jitter_luma((pr >> (8 * e)) & 255, (pg >> (8 * e)) & 255, (pb >> (8 * e)) & 255);
            }
#pragma unroll
            for (int m = 32; m > 0; m >>= 1) s += __shfl_xor(s, m);
            __syncthreads();                                 // (the previous readers of wave_sum are done)
            if ((tid & 63) == 0) wave_sum[tid >> 6] = s;
            __syncthreads();
            unsigned total = 0;
            for (int w = 0; w < (nt >> 6); ++w) total += (unsigned)wave_sum[w];
            mean = (int)((2u * total + (unsigned)HW) / (2u * (unsigned)HW));
        }
        const float alpha = op < 3 ? __uint_as_float((unsigned)prm[9 + op]) : 0.0f;
        const bool inside = alpha >= 0.0f && alpha <= 1.0f;
        const int shift = prm[12] & 255;
        for (int q = tid; q < nquad; q += nt) {
            const unsigned pr = plane_r[q], pg = plane_g[q], pb = plane_b[q];
            unsigned nr = 0, ng = 0, nb = 0;
            for (int e = 0; e < 4; ++e) {
                int r = (pr >> (8 * e)) & 255, g = (pg >> (8 * e)) & 255, bl = (pb >> (8 * e)) & 255;
                if (op == 3) {
                    jitter_hue(r, g, bl, shift);
                } else {
                    const int deg = op == 0 ? 0 : (op == 1 ? mean : jitter_luma(r, g, bl));
                    r = jitter_blend(deg, r, alpha, inside);
                    g = jitter_blend(deg, g, alpha, inside);
                    bl = jitter_blend(deg, bl, alpha, inside);
                }
                nr |= (unsigned)r << (8 * e);
                ng |= (unsigned)g << (8 * e);
                nb |= (unsigned)bl << (8 * e);
            }
            plane_r[q] = nr;
            plane_g[q] = ng;
            plane_b[q] = nb;
        }
    }

    // ---- ToTensor, t * 2 - 1: planar fp32, consecutive lanes write consecutive 16 B ------------------------------------------------------
    float* dst = out + (size_t)b * 3 * HW;
    const bool vec = (HW & 3) == 0;                          // (then every plane of every image starts 16 B aligned)
    for (int q = tid; q < nquad; q += nt) {
        const unsigned px[3] = {plane_r[q], plane_g[q], plane_b[q]};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (float)((px[c] >> (8 * e)) & 255) / 255.0f * 2.0f - 1.0f;
            float* d = dst + (size_t)c * HW + 4 * q;
            if (vec) {
                *(float4*)d = make_float4(v[0], v[1], v[2], v[3]);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (4 * q + e < HW) d[e] = v[e];
            }
        }
    }
}

extern "C" int cdf_augment_jitter_batch(const void* cache, long long N, int SH, int SW, int C, const long long* idx, const int* params,
                                        const int* params_host, float* out, int B, int H, int W, void* stream) {
    CDF_REQUIRE(cache && idx && params && params_host && out, "cdf_augment_jitter_batch: null pointer");
    CDF_REQUIRE(C == 3, "cdf_augment_jitter_batch: %d channels (ColorJitter's saturation and hue need RGB)", C);
    CDF_REQUIRE(N > 0 && B > 0 && SH > 0 && SW > 0 && H > 0 && W > 0, "cdf_augment_jitter_batch: bad geometry (%lld images of %dx%d, %d crops to %dx%d)",
                N, SH, SW, B, H, W);
    const size_t lds = jitter_lds_bytes(SH, SW, H, W);
    CDF_REQUIRE(lds <= CDF_JITTER_LDS_CAP, "cdf_augment_jitter_batch: %dx%d from %dx%d needs %zu bytes of LDS (cap %d)", H, W, SH, SW, lds,
                CDF_JITTER_LDS_CAP);
    for (int b = 0; b < B; ++b) {
        const int* p = params_host + (size_t)b * CDF_JITTER_STRIDE;
        CDF_REQUIRE(p[2] >= 1 && p[3] >= 1 && p[0] >= 0 && p[1] >= 0 && p[2] <= SH - p[0] && p[3] <= SW - p[1],
                    "cdf_augment_jitter_batch: crop box of row %d (top %d, left %d, %dx%d) outside the %dx%d image", b, p[0], p[1], p[2], p[3], SH, SW);
        for (int o = 0; o < 4; ++o)
            CDF_REQUIRE(p[5 + o] >= -1 && p[5 + o] <= 3, "cdf_augment_jitter_batch: op code %d in row %d (-1 none, 0 brightness, 1 contrast, 2 saturation, 3 hue)",
                        p[5 + o], b);
    }
    const int nquad = (H * W + 3) / 4;
    const int nt = nquad >= 1024 ? 1024 : (nquad + 63) / 64 * 64;
    CDF_LAUNCH_LDS(augment_jitter_kernel, dim3(B), dim3(nt), lds, CDF_S, (const unsigned char*)cache, N, idx, params, out, SH, SW, H, W,
                   jitter_ksize(SW, W), jitter_ksize(SH, H));
    return cdf_check_launch("augment_jitter_batch");
}
