// k_pack.hip — operand preparation for the GEMMs: weights between the PyTorch parameter layouts and the GEMM layouts (fp32, or bf16
// hi / lo planes), every cached layout of a model in one launch, activations split into bf16 planes and widened back.
#include "cdf_common.h"
#include "colddiff.h"

// ------------------------------------------------------------------------------------------------
// weight packing from the PyTorch parameter layouts into the GEMM "KN" layout (the way back: cdf_unpack_reduce, k_reduce.hip)
//   pack  : dst[t][r][c] = (c < C) ? src[c*s_c + r*s_r + t*s_t] : 0        (ldc = padded C)
// ------------------------------------------------------------------------------------------------
__global__ void pack_weight_kernel(const float* src, float* dst, int T, int R, int C, int ldc, long long s_t,
                                   long long s_r, long long s_c) {
    const long long n = (long long)T * R * ldc;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % ldc);
        const long long tr = i / ldc;
        const int r = (int)(tr % R), t = (int)(tr / R);
        dst[i] = c < C ? src[c * s_c + r * s_r + t * s_t] : 0.f;
    }
}

__global__ void pack_weight_bf16_kernel(const float* src, unsigned short* dst_hi, unsigned short* dst_lo, int T, int R, int C,
                                        int ldc, long long s_t, long long s_r, long long s_c) {
    const long long n = (long long)T * R * ldc;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % ldc);
        const long long tr = i / ldc;
        const int r = (int)(tr % R), t = (int)(tr / R);
        const float v = c < C ? src[c * s_c + r * s_r + t * s_t] : 0.f;
        const unsigned h = cdf_f2bf(v);
        dst_hi[i] = (unsigned short)h;
        if (dst_lo) dst_lo[i] = (unsigned short)cdf_f2bf(v - cdf_bf2f(h));
    }
}

// The activation split ONCE into bf16 hi / lo planes ([rows][ld] each, same bytes as the fp32 tensor) for the pre-split GEMMs
// (k_conv_spx.hip and its siblings), whose main loops are then pure 16-byte copies global -> LDS plus MFMAs.
__global__ void split_bf16_kernel(const float* x, int ldx, unsigned short* hi, unsigned short* lo, int ldo, long long rows, int C4) {
    const long long n = rows * C4;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C4) * 4;
        const long long r = i / C4;
        const float4 v = *(const float4*)(x + r * ldx + c);
        uint2 h, l;
        cdf_split4(v.x, v.y, v.z, v.w, h, l);
        *(uint2*)(hi + r * ldo + c) = h;
        if (lo) *(uint2*)(lo + r * ldo + c) = l;
    }
}

// the way back (bf16 activation storage): a bf16 tensor widened to fp32 for a kernel that has no bf16-input form (exact conversion)
__global__ void widen_bf16_kernel(const unsigned short* x, int ldx, float* y, int ldy, long long rows, int C4) {
    const long long n = rows * C4;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C4) * 4;
        const long long r = i / C4;
        *(float4*)(y + r * ldy + c) = cdf_quad_cvt(*(const uint2*)(x + r * ldx + c));
    }
}

// Every cached GEMM layout of a model in ONE launch (the weights change once per optimizer step; one launch per layout was ~160
// launches of 2-60 us per step).  Entry e: dst[t][r][c] = (c < C) ? src[c*s_c + r*s_r + t*s_t] : 0 over [T][R][ldc], written as fp32
// (kind 0) or as bf16 hi [/ lo] planes (kind 1; lo == NULL: hi only).  Block b works on entry `e` with first_block[e] <= b <
// first_block[e+1] (cdf_pack_blocks(T, R, ldc, s_t) blocks per entry), elements (b - first_block[e]) * 1024 ... + 1023 of it.
struct CdfPackEntry {
    const float* src;
    void* dst0;
    void* dst1;
    long long s_t, s_r, s_c;
    int T, R, C, ldc, kind, first_block;
};

__global__ void __launch_bounds__(256) pack_many_kernel(const CdfPackEntry* tab, int nentries) {
    int lo = 0, hi = nentries - 1;                          // (wave-uniform binary search over <= a few hundred entries)
    const int b = blockIdx.x;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab[mid].first_block <= b) lo = mid; else hi = mid - 1;
    }
    const CdfPackEntry e = tab[lo];
    if (e.s_t == 1 && e.T > 1 && e.T <= 16) {
        // taps contiguous in the source (conv weights [..][kh][kw]): a thread takes (r, c) pairs and moves ALL T taps of each, so the
        // 4 T-byte runs of neighbouring lanes are consumed whole while they are in flight (one tap per pass fetched every 64-byte line
        // T times: the 56 M-parameter net took 0.7 ms per step).  Block = 1024 (r, c) pairs; cdf_pack_blocks() gives the block count.
        const long long n2 = (long long)e.R * e.ldc;
        const long long j0 = (long long)(b - e.first_block) * 1024 + threadIdx.x;
        const long long plane = (long long)e.R * e.ldc;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long long j = j0 + 256 * k;
            if (j >= n2) break;
            const int c = (int)(j % e.ldc), r = (int)(j / e.ldc);
            const bool ok = c < e.C;
            const float* sp = e.src + (ok ? c * e.s_c + r * e.s_r : 0);
            float v[16];
#pragma unroll
            for (int t = 0; t < 16; ++t) v[t] = sp[t < e.T ? t : 0];
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                if (t >= e.T) break;
                const float x = ok ? v[t] : 0.f;
                const long long i = t * plane + j;
                if (e.kind == 0) {
                    ((float*)e.dst0)[i] = x;
                } else {
                    const unsigned h = cdf_f2bf(x);
                    ((unsigned short*)e.dst0)[i] = (unsigned short)h;
                    if (e.dst1) ((unsigned short*)e.dst1)[i] = (unsigned short)cdf_f2bf(x - cdf_bf2f(h));
                }
            }
        }
        return;
    }
    const long long n = (long long)e.T * e.R * e.ldc;
    const long long i0 = (long long)(b - e.first_block) * 1024 + threadIdx.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long long i = i0 + 256 * k;
        if (i >= n) break;
        const int c = (int)(i % e.ldc);
        const long long tr = i / e.ldc;
        const int r = (int)(tr % e.R), t = (int)(tr / e.R);
        const float v = c < e.C ? e.src[c * e.s_c + r * e.s_r + t * e.s_t] : 0.f;
        if (e.kind == 0) {
            ((float*)e.dst0)[i] = v;
        } else {
            const unsigned h = cdf_f2bf(v);
            ((unsigned short*)e.dst0)[i] = (unsigned short)h;
            if (e.dst1) ((unsigned short*)e.dst1)[i] = (unsigned short)cdf_f2bf(v - cdf_bf2f(h));
        }
    }
}

extern "C" int cdf_pack_entry_bytes(void) { return (int)sizeof(CdfPackEntry); }
// blocks an entry of cdf_pack_many spans (first_block of the next entry = first_block + this)
extern "C" int cdf_pack_blocks(int T, int R, int ldc, long long s_t) {
    const long long n = (s_t == 1 && T > 1 && T <= 16) ? (long long)R * ldc : (long long)T * R * ldc;
    return (int)((n + 1023) / 1024);
}

// table: nentries CdfPackEntry records in DEVICE memory (first_block ascending, entry e spanning ceil(T R ldc / 1024) blocks)
extern "C" int cdf_pack_many(const void* table, int nentries, int nblocks, void* stream) {
    CDF_REQUIRE(table && nentries > 0 && nblocks > 0, "cdf_pack_many: bad args");
    CDF_LAUNCH(pack_many_kernel, dim3(nblocks), dim3(256), 0, CDF_S, (const CdfPackEntry*)table, nentries);
    return cdf_check_launch("pack_many");
}

extern "C" int cdf_pack_weight(const float* src, float* dst, int T, int R, int C, int ldc, long long s_t,
                               long long s_r, long long s_c, void* stream) {
    CDF_REQUIRE(src && dst && T > 0 && R > 0 && C > 0 && ldc >= C && ldc % 4 == 0, "cdf_pack_weight: bad args");
    CDF_LAUNCH(pack_weight_kernel, dim3(cdf_ew_grid4k((long long)T * R * ldc)), dim3(256), 0, CDF_S, src, dst, T, R, C, ldc, s_t, s_r, s_c);
    return cdf_check_launch("pack_weight");
}

extern "C" int cdf_pack_weight_bf16(const float* src, void* dst_hi, void* dst_lo, int T, int R, int C, int ldc, long long s_t,
                                    long long s_r, long long s_c, void* stream) {
    CDF_REQUIRE(src && dst_hi && T > 0 && R > 0 && C > 0 && ldc >= C && ldc % 32 == 0, "cdf_pack_weight_bf16: bad args (ldc must be a multiple of 32)");
    long long g = ((long long)T * R * ldc + 255) / 256;
    if (g > 4096) g = 4096;
    CDF_LAUNCH(pack_weight_bf16_kernel, dim3((int)g), dim3(256), 0, CDF_S, src, (unsigned short*)dst_hi, (unsigned short*)dst_lo, T, R, C, ldc, s_t, s_r, s_c);
    return cdf_check_launch("pack_weight_bf16");
}

// ---- pre-split operand entry points ---------------------------------------------------------------------
extern "C" int cdf_split_bf16(const float* x, int ldx, void* hi, void* lo, int ldo, long long rows, int C, void* stream) {
    CDF_REQUIRE(x && hi && rows > 0 && C > 0 && C % 4 == 0 && ldx % 4 == 0 && ldo % 8 == 0 && ldo >= C, "cdf_split_bf16: bad args (C %% 4, ldo %% 8)");
    long long g = (rows * (C / 4) + 255) / 256;
    if (g > 8192) g = 8192;
    CDF_LAUNCH(split_bf16_kernel, dim3((int)g), dim3(256), 0, CDF_S, x, ldx, (unsigned short*)hi, (unsigned short*)lo, ldo, rows, C / 4);
    return cdf_check_launch("split_bf16");
}

extern "C" int cdf_bf16_to_f32(const void* x, int ldx, float* y, int ldy, long long rows, int C, void* stream) {
    CDF_REQUIRE(x && y && rows > 0 && C > 0 && C % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && ldx >= C && ldy >= C && (((uintptr_t)x) & 7) == 0 &&
                (((uintptr_t)y) & 15) == 0, "cdf_bf16_to_f32: bad args (C %% 4, pitches %% 4, x 8-byte / y 16-byte aligned)");
    long long g = (rows * (C / 4) + 255) / 256;
    if (g > 8192) g = 8192;
    CDF_LAUNCH(widen_bf16_kernel, dim3((int)g), dim3(256), 0, CDF_S, (const unsigned short*)x, ldx, y, ldy, rows, C / 4);
    return cdf_check_launch("bf16_to_f32");
}
