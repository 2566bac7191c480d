// k_color.hip -- the colour forward process of the decolorization package (decolor-diffusion/diffusion/forward_process_impl.py:131-218):
// a chain of per-pixel 3 x 3 colour mixes, optionally in Lab space, with the pixel's three channels held in registers for the whole
// chain; the stand-alone Lab <-> RGB conversions; the per-image mean shift of UnetConvNextBlock(output_mean_scale=True).
//
// The reference runs the chain as T nn.Conv2d(3, 3, 1) launches plus a torch.stack of every intermediate batch ((t + 1) * 8 B per element
// and a T x B x 3 x H x W stack); here one launch reads each input plane once and writes each requested output once.
//
// Arithmetic: plain fp32 multiplies, adds and IEEE divisions in the order of the torch expressions (the file is compiled with
// -ffp-contract=off like every other one), so the RGB chain differs from torch's 1 x 1 convolution by its summation order only; the Lab
// conversions evaluate powf where torch evaluates torch.pow (a few ulp apart).
#include "cdf_common.h"
#include "colddiff.h"

// ---- Lab <-> RGB, (-1, 1) RGB convention (utils.py:113-222; sRGB <-> linear RGB and RGB <-> XYZ after kornia.color) ----------------
#define CDF_WHITE_X 0.95047f
#define CDF_WHITE_Z 1.08883f

__device__ __forceinline__ float cdf_srgb_to_linear(float v) {          // kornia rgb_to_linear_rgb
    const float p = powf((v + 0.055f) / 1.055f, 2.4f);
    return v > 0.04045f ? p : v / 12.92f;
}
__device__ __forceinline__ float cdf_linear_to_srgb(float v) {          // kornia linear_rgb_to_rgb
    const float thr = 0.0031308f;
    const float p = 1.055f * powf(fmaxf(v, thr), (float)(1.0 / 2.4)) - 0.055f;
    return v > thr ? p : 12.92f * v;
}
__device__ __forceinline__ float cdf_lab_f(float n) {                   // xyz / white -> f(.)
    const float thr = 0.008856f;
    const float p = powf(fmaxf(n, thr), (float)(1.0 / 3.0));
    const float s = 7.787f * n + (float)(4.0 / 29.0);
    return n > thr ? p : s;
}
__device__ __forceinline__ float cdf_lab_finv(float f) {
    const float p = f * f * f;                                          // torch.pow(x, 3.0) is x * x * x
    const float s = (f - (float)(4.0 / 29.0)) / 7.787f;
    return f > 0.2068966f ? p : s;
}
// (r, g, b) in (-1, 1) -> (L, a, b)
__device__ __forceinline__ void cdf_rgb2lab(float& c0, float& c1, float& c2) {
    const float r = cdf_srgb_to_linear((c0 + 1.0f) * 0.5f);
    const float g = cdf_srgb_to_linear((c1 + 1.0f) * 0.5f);
    const float b = cdf_srgb_to_linear((c2 + 1.0f) * 0.5f);
    const float X = (0.412453f * r + 0.357580f * g) + 0.180423f * b;    // kornia rgb_to_xyz
    const float Y = (0.212671f * r + 0.715160f * g) + 0.072169f * b;
    const float Z = (0.019334f * r + 0.119193f * g) + 0.950227f * b;
    const float fx = cdf_lab_f(X / CDF_WHITE_X), fy = cdf_lab_f(Y / 1.0f), fz = cdf_lab_f(Z / CDF_WHITE_Z);
    c0 = 116.0f * fy - 16.0f;
    c1 = 500.0f * (fx - fy);
    c2 = 200.0f * (fy - fz);
}
// (L, a, b) -> (r, g, b) in [-1, 1] (clamped)
__device__ __forceinline__ void cdf_lab2rgb(float& c0, float& c1, float& c2) {
    const float fy = (c0 + 16.0f) / 116.0f;
    const float fx = c1 / 500.0f + fy;
    const float fz = fmaxf(fy - c2 / 200.0f, 0.0f);
    const float X = cdf_lab_finv(fx) * CDF_WHITE_X, Y = cdf_lab_finv(fy) * 1.0f, Z = cdf_lab_finv(fz) * CDF_WHITE_Z;
    const float r = (3.2404813432005266f * X + -1.5371515162713185f * Y) + -0.4985363261688878f * Z;     // kornia xyz_to_rgb
    const float g = (-0.9692549499965682f * X + 1.8759900014898907f * Y) + 0.0415559265582928f * Z;
    const float b = (0.0556466391351772f * X + -0.2040413383665112f * Y) + 1.0573110696453443f * Z;
    c0 = 2.0f * fminf(fmaxf(cdf_linear_to_srgb(r), 0.0f), 1.0f) - 1.0f;
    c1 = 2.0f * fminf(fmaxf(cdf_linear_to_srgb(g), 0.0f), 1.0f) - 1.0f;
    c2 = 2.0f * fminf(fmaxf(cdf_linear_to_srgb(b), 0.0f), 1.0f) - 1.0f;
}

// ---- four consecutive pixels of one plane -----------------------------------------------------------------------------------------
// ALIGNED: H * W is a multiple of 4, every plane starts on a 16-byte boundary.  Otherwise the body still moves 16 bytes per plane and
// lane, from a 4-byte-aligned address (the planes of an odd-sized image are not 16-byte aligned), and the H * W % 4 last pixels of each
// image go through the scalar tail.
struct cdf_px4 { float v[4]; };
template <bool ALIGNED>
__device__ __forceinline__ cdf_px4 cdf_ld_px4(const float* p) {
    cdf_px4 r;
    if (ALIGNED) {
        const float4 t = *(const float4*)p;
        r.v[0] = t.x; r.v[1] = t.y; r.v[2] = t.z; r.v[3] = t.w;
    } else {
        __builtin_memcpy(&r, p, 16);
    }
    return r;
}
template <bool ALIGNED>
__device__ __forceinline__ void cdf_st_px4(float* p, const cdf_px4& r) {
    if (ALIGNED) *(float4*)p = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
    else __builtin_memcpy(p, &r, 16);
}

struct ColorArgs {
    const float* x;
    float* y;
    float* total;          // nullable
    float* snap;           // nullable
    const float* img;      // nullable: Algorithm-2 combine
    const float* w;        // [T][9]
    const int64_t* nb;     // nullable: per-sample step counts
    long long HW;
    int T, nsteps, nmax, lab;
};

// the chain on NP pixels held in registers; sw = this row's weights in LDS ([step][9]); every count is block-uniform
template <int NP, bool LAB>
__device__ __forceinline__ void cdf_color_run(float (&c)[3][NP], float (&yo)[3][NP], float (&so)[3][NP], float (&to)[3][NP], const float* sw,
                                              int n, int ns, int nt, int nloop) {
    for (int s = 0;; ++s) {
        // (uniform branches on register copies; nothing is loaded inside them)
        if (s == n) {
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int p = 0; p < NP; ++p) yo[k][p] = c[k][p];
        }
        if (s == ns) {
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int p = 0; p < NP; ++p) so[k][p] = c[k][p];
        }
        if (s == nt) {
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int p = 0; p < NP; ++p) to[k][p] = c[k][p];
        }
        if (s >= nloop) break;
        const float* ws = sw + s * 9;
        const float w00 = ws[0], w01 = ws[1], w02 = ws[2], w10 = ws[3], w11 = ws[4], w12 = ws[5], w20 = ws[6], w21 = ws[7], w22 = ws[8];
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            float a0 = c[0][p], a1 = c[1][p], a2 = c[2][p];
            if (LAB) cdf_lab2rgb(a0, a1, a2);
            float b0 = (w00 * a0 + w01 * a1) + w02 * a2;
            float b1 = (w10 * a0 + w11 * a1) + w12 * a2;
            float b2 = (w20 * a0 + w21 * a1) + w22 * a2;
            if (LAB) cdf_rgb2lab(b0, b1, b2);
            c[0][p] = b0; c[1][p] = b1; c[2][p] = b2;
        }
    }
}

template <bool LAB, bool ALIGNED>
__global__ void __launch_bounds__(256) color_chain_kernel(ColorArgs a) {
    CDF_DYN_SMEM(smem);
    float* sw = (float*)smem;
    const int b = blockIdx.y;
    // block-uniform counts: n steps for y, ns for snap, nt for total, nloop = how far the chain runs at all
    const long long raw = a.nb ? (long long)a.nb[b] : (long long)a.nsteps;
    const bool pass = raw < 0;                                          // passed-through row: every output = x
    const int n = pass ? 0 : (raw < a.T ? (int)raw : a.T);              // (a count beyond the table would read past it: clamped)
    const int nt = pass ? 0 : a.nmax;
    int ns = n < a.nmax - 1 ? n : a.nmax - 1;
    ns = ns < 0 ? 0 : ns;
    const int nloop = a.total && nt > n ? nt : n;
    for (int i = threadIdx.x; i < nloop * 9; i += blockDim.x) sw[i] = a.w[i];
    __syncthreads();

    const long long HW = a.HW;
    const size_t base = (size_t)b * 3 * (size_t)HW;
    const long long ngroups = HW >> 2;
    for (long long gi = (long long)blockIdx.x * blockDim.x + threadIdx.x; gi < ngroups; gi += (long long)gridDim.x * blockDim.x) {
        const size_t o = base + (size_t)gi * 4;
        float c[3][4], yo[3][4], so[3][4], to[3][4], im[3][4];
        cdf_px4 ld[3], li[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) ld[k] = cdf_ld_px4<ALIGNED>(a.x + o + (size_t)k * HW);
        if (a.img) {
#pragma unroll
            for (int k = 0; k < 3; ++k) li[k] = cdf_ld_px4<ALIGNED>(a.img + o + (size_t)k * HW);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                c[k][p] = ld[k].v[p];
                im[k][p] = a.img ? li[k].v[p] : 0.f;
            }
        cdf_color_run<4, LAB>(c, yo, so, to, sw, n, ns, nt, nloop);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            cdf_px4 r;
            if (a.img) {
#pragma unroll
                for (int p = 0; p < 4; ++p) r.v[p] = (im[k][p] - yo[k][p]) + so[k][p];
            } else {
#pragma unroll
                for (int p = 0; p < 4; ++p) r.v[p] = yo[k][p];
            }
            cdf_st_px4<ALIGNED>(a.y + o + (size_t)k * HW, r);
            if (a.snap) {
#pragma unroll
                for (int p = 0; p < 4; ++p) r.v[p] = so[k][p];
                cdf_st_px4<ALIGNED>(a.snap + o + (size_t)k * HW, r);
            }
            if (a.total) {
#pragma unroll
                for (int p = 0; p < 4; ++p) r.v[p] = to[k][p];
                cdf_st_px4<ALIGNED>(a.total + o + (size_t)k * HW, r);
            }
        }
    }
    // scalar tail: the H * W % 4 last pixels of the image, one lane each, in the first block of the image
    const int tail = (int)(HW & 3);
    if (!ALIGNED && blockIdx.x == 0 && (int)threadIdx.x < tail) {
        const size_t o = base + (size_t)(ngroups * 4) + threadIdx.x;
        float c[3][1], yo[3][1], so[3][1], to[3][1];
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k][0] = a.x[o + (size_t)k * HW];
        float im[3] = {0.f, 0.f, 0.f};
        if (a.img) {
#pragma unroll
            for (int k = 0; k < 3; ++k) im[k] = a.img[o + (size_t)k * HW];
        }
        cdf_color_run<1, LAB>(c, yo, so, to, sw, n, ns, nt, nloop);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            a.y[o + (size_t)k * HW] = a.img ? (im[k] - yo[k][0]) + so[k][0] : yo[k][0];
            if (a.snap) a.snap[o + (size_t)k * HW] = so[k][0];
            if (a.total) a.total[o + (size_t)k * HW] = to[k][0];
        }
    }
}

__global__ void __launch_bounds__(256) lab_convert_kernel(const float* x, float* y, long long HW, long long npix, int to_rgb) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (long long)gridDim.x * blockDim.x) {
        const long long b = i / HW;
        const size_t o = (size_t)b * 3 * (size_t)HW + (size_t)(i - b * HW);
        float c0 = x[o], c1 = x[o + HW], c2 = x[o + 2 * HW];
        if (to_rgb) cdf_lab2rgb(c0, c1, c2);
        else cdf_rgb2lab(c0, c1, c2);
        y[o] = c0;
        y[o + HW] = c1;
        y[o + 2 * HW] = c2;
    }
}

// ---- per-image mean shift ------------------------------------------------------------------------------------------------------------
#define CDF_MS_CHUNK 8192          // elements of one image per block

// stage 1: ws[(b * nchunk + chunk) * 2 + {0, 1}] = the chunk's sums of x and y (x nullable: 0)
__global__ void __launch_bounds__(256) mean_shift_partial_kernel(const float* x, const float* y, float* ws, long long n, int nchunk) {
    __shared__ float red[32];                                           // (cdf_block_sum: 17 floats)
    const int b = blockIdx.y, ch = blockIdx.x;
    const long long lo = (long long)ch * CDF_MS_CHUNK;
    const long long hi = lo + CDF_MS_CHUNK < n ? lo + CDF_MS_CHUNK : n;
    const size_t base = (size_t)b * (size_t)n;
    float sx = 0.f, sy = 0.f;
    for (long long i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        sy += y[base + i];
        if (x) sx += x[base + i];
    }
    const float ty = cdf_block_sum(sy, red);
    const float tx = cdf_block_sum(sx, red);
    if (threadIdx.x == 0) {
        ws[((size_t)b * nchunk + ch) * 2] = tx;
        ws[((size_t)b * nchunk + ch) * 2 + 1] = ty;
    }
}

// stage 2: the image's partials summed in chunk order by every block (deterministic), then out = (y - mean x) + mean y
__global__ void __launch_bounds__(256) mean_shift_apply_kernel(const float* y, float* out, const float* ws, long long n, int nchunk,
                                                               int bwd) {
    const int b = blockIdx.y, ch = blockIdx.x;
    float tx = 0.f, ty = 0.f;
    for (int i = 0; i < nchunk; ++i) {                                  // uniform addresses: the same for every lane
        tx += ws[((size_t)b * nchunk + i) * 2];
        ty += ws[((size_t)b * nchunk + i) * 2 + 1];
    }
    const float mx = tx / (float)n, my = ty / (float)n;
    const long long lo = (long long)ch * CDF_MS_CHUNK;
    const long long hi = lo + CDF_MS_CHUNK < n ? lo + CDF_MS_CHUNK : n;
    const size_t base = (size_t)b * (size_t)n;
    for (long long i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        const float v = y[base + i];
        out[base + i] = bwd ? v + my : (v - mx) + my;
    }
}

// ---- C entry points ------------------------------------------------------------------------------------------------------------------
extern "C" int cdf_color_chain(const float* x, float* y, float* total, float* snap, const float* img, const float* w,
                               const int64_t* nsteps_b, int B, int C, long long HW, int T, int nsteps, int nmax, int lab, void* stream) {
    CDF_REQUIRE(x && y && w, "cdf_color_chain: null pointer");
    CDF_REQUIRE(C == 3, "cdf_color_chain: the colour mix is 3 x 3 (C = %d)", C);
    CDF_REQUIRE(B > 0 && B <= 65535 && HW > 0 && HW < (1ll << 40), "cdf_color_chain: bad shape (B = %d, HW = %lld)", B, HW);
    CDF_REQUIRE(T > 0 && T <= 1024, "cdf_color_chain: T = %d outside 1..1024", T);
    CDF_REQUIRE(nmax >= 0 && nmax <= T, "cdf_color_chain: nmax = %d exceeds the %d steps of the table", nmax, T);
    CDF_REQUIRE(nsteps_b || (nsteps <= T), "cdf_color_chain: nsteps = %d exceeds the %d steps of the table", nsteps, T);
    CDF_REQUIRE(!img || snap, "cdf_color_chain: the Alg. 2 combine needs a snap buffer");
    CDF_REQUIRE(!(img && total), "cdf_color_chain: combine and total exclude each other");
    ColorArgs a{x, y, total, snap, img, w, nsteps_b, HW, T, nsteps, nmax, lab};
    const long long groups = HW >> 2;
    // one float4 group per lane: the chain is a dependent loop of up to T steps (an LDS weight read + ~60 vector instructions each), so
    // what hides its latency is waves in flight, not work per lane; the weight staging is T * 36 bytes per block
    int gx = cdf_cdiv(groups > 0 ? groups : 1, 256);
    gx = gx < 1 ? 1 : (gx > 16384 ? 16384 : gx);
    const size_t lds = (size_t)T * 9 * sizeof(float);
    const bool aligned = (HW & 3) == 0 && (((uintptr_t)x | (uintptr_t)y | (uintptr_t)total | (uintptr_t)snap | (uintptr_t)img) & 15) == 0;
    const dim3 grid(gx, B), block(256);
    if (lab) {
        if (aligned) CDF_LAUNCH((color_chain_kernel<true, true>), grid, block, lds, CDF_S, a);
        else CDF_LAUNCH((color_chain_kernel<true, false>), grid, block, lds, CDF_S, a);
    } else {
        if (aligned) CDF_LAUNCH((color_chain_kernel<false, true>), grid, block, lds, CDF_S, a);
        else CDF_LAUNCH((color_chain_kernel<false, false>), grid, block, lds, CDF_S, a);
    }
    return cdf_check_launch("color_chain");
}

extern "C" int cdf_lab_convert(const float* x, float* y, int B, int C, long long HW, int to_rgb, void* stream) {
    CDF_REQUIRE(x && y, "cdf_lab_convert: null pointer");
    CDF_REQUIRE(C == 3, "cdf_lab_convert: Lab and RGB images have 3 channels (C = %d)", C);
    CDF_REQUIRE(B > 0 && HW > 0, "cdf_lab_convert: bad shape");
    const long long npix = (long long)B * HW;
    int g = cdf_cdiv(npix, 256);
    g = g > 65536 ? 65536 : g;
    CDF_LAUNCH(lab_convert_kernel, dim3(g), dim3(256), 0, CDF_S, x, y, HW, npix, to_rgb);
    return cdf_check_launch("lab_convert");
}

extern "C" int cdf_mean_shift_nchunk(long long n) { return n > 0 ? cdf_cdiv(n, CDF_MS_CHUNK) : 0; }

extern "C" int cdf_mean_shift(const float* x, const float* y, float* out, float* ws, int B, long long n, void* stream) {
    CDF_REQUIRE(x && y && out && ws, "cdf_mean_shift: null pointer");
    CDF_REQUIRE(B > 0 && B <= 65535 && n > 0, "cdf_mean_shift: bad shape");
    const int nchunk = cdf_mean_shift_nchunk(n);
    CDF_LAUNCH(mean_shift_partial_kernel, dim3(nchunk, B), dim3(256), 0, CDF_S, x, y, ws, n, nchunk);
    CDF_LAUNCH(mean_shift_apply_kernel, dim3(nchunk, B), dim3(256), 0, CDF_S, y, out, (const float*)ws, n, nchunk, 0);
    return cdf_check_launch("mean_shift");
}

extern "C" int cdf_mean_shift_bwd(const float* dy, float* dx, float* ws, int B, long long n, void* stream) {
    CDF_REQUIRE(dy && dx && ws, "cdf_mean_shift_bwd: null pointer");
    CDF_REQUIRE(B > 0 && B <= 65535 && n > 0, "cdf_mean_shift_bwd: bad shape");
    const int nchunk = cdf_mean_shift_nchunk(n);
    CDF_LAUNCH(mean_shift_partial_kernel, dim3(nchunk, B), dim3(256), 0, CDF_S, (const float*)nullptr, dy, ws, n, nchunk);
    CDF_LAUNCH(mean_shift_apply_kernel, dim3(nchunk, B), dim3(256), 0, CDF_S, dy, dx, (const float*)ws, n, nchunk, 1);
    return cdf_check_launch("mean_shift_bwd");
}
