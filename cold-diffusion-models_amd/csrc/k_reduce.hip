// k_reduce.hip — the deterministic reductions behind the weight and bias gradients: split-K slabs of the weight-gradient GEMMs summed
// into the PyTorch parameter layouts, column sums of a pitched matrix.
#include "cdf_common.h"
#include "colddiff.h"

// ------------------------------------------------------------------------------------------------
// GEMM "KN" layout -> PyTorch parameter layout, summed over the split-K slabs (the way there: cdf_pack_weight, k_pack.hip)
//   unpack: g[c*s_c + r*s_r + t*s_t] (+)= scale * sum_z ws[z][t][r][c]
// ------------------------------------------------------------------------------------------------
// block = SL slab lanes x 64 consecutive output elements (element index runs over [T][R][C], C fastest).  A lane adds
// slabs rl, rl + SL, ... in four independent chains (four loads in flight per lane): with 4 lanes x 2 chains the ~230-slab
// reductions of the 128 x 128-pixel layers were ~30 dependent round trips (80 us for 67 MB).  The summation tree is fixed
// by (SL, nsplit): deterministic.
// (bws / gb / bC / bld: optional second reduction folded into the same launch -- the bias-gradient partials [nsplit][bld] that the
// weight-gradient kernels produce next to their slabs: gb[c] (+)= sum_z bws[z][c].  The LAST blockIdx.y row of the grid does it.)
template <int SL>
__global__ void __launch_bounds__(64 * SL) unpack_reduce_kernel(const float* ws, float* g, int nsplit, int T, int R, int C, int ldc,
                                                                long long s_t, long long s_r, long long s_c, int accumulate,
                                                                const float* bws, float* gb, int bC, int bld) {
    __shared__ float red[SL][64];
    if (bws != nullptr && blockIdx.y == 1) {                 // the fused bias reduction: one 1 x 1 x bC "tensor" with unit strides
        ws = bws; g = gb; T = 1; R = 1; C = bC; ldc = bld; s_t = 0; s_r = 0; s_c = 1;
    }
    const long long n = (long long)T * R * C;
    const long long slab = (long long)T * R * ldc;
    const int l = threadIdx.x & 63, rl = threadIdx.x >> 6;
    for (long long base = (long long)blockIdx.x * 64; base < n; base += (long long)gridDim.x * 64) {
        const long long i = base + l;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        int c = 0, r = 0, t = 0;
        if (i < n) {
            c = (int)(i % C);
            const long long tr = i / C;
            r = (int)(tr % R);
            t = (int)(tr / R);
            const float* p = ws + ((long long)t * R + r) * ldc + c;
            int z = rl;
            for (; z + 3 * SL < nsplit; z += 4 * SL) {
                s0 += p[z * slab];
                s1 += p[(z + SL) * slab];
                s2 += p[(z + 2 * SL) * slab];
                s3 += p[(z + 3 * SL) * slab];
            }
            if (z < nsplit) s0 += p[z * slab];
            if (z + SL < nsplit) s1 += p[(z + SL) * slab];
            if (z + 2 * SL < nsplit) s2 += p[(z + 2 * SL) * slab];
        }
        __syncthreads();
        red[rl][l] = (s0 + s1) + (s2 + s3);
        __syncthreads();
        if (rl == 0 && i < n) {
            float tot = 0.f;
#pragma unroll
            for (int q = 0; q < SL; q += 4) tot += (red[q][l] + red[q + 1][l]) + (red[q + 2][l] + red[q + 3][l]);
            float* dst = g + c * s_c + r * s_r + t * s_t;
            *dst = accumulate ? *dst + tot : tot;
        }
    }
}

// Transposing form of the slab reduction for parameter layouts whose fast index is NOT the slab's (conv weights [Cout][Cin][kh][kw]:
// s_c = Cin kh kw).  The kernel above hands 64 consecutive c to a block: every result is a lone 4-byte read-modify-write
// s_c floats from its neighbours -- a 32-byte sector moved each way per 4 useful bytes, neighbours in (r, t) landing on other XCDs.
// Here a block owns a tile of 32 c x RJ r x T taps (J = RJ T <= 36 values per c): 32 c-lanes x 8 slab-lanes, every lane J independent
// loads per slab (128-byte rows over c), the 8 slab-lanes are folded through LDS in a fixed order (deterministic) and the tile leaves
// as runs of J consecutive floats per c (144 B for 3 x 3, the whole [c][t] block for transposed-conv weights).
template <int T_, int RJ>
__device__ __forceinline__ void unpack_tile_body(const float* ws, float* g, int nsplit, int R, int C, int ldc, long long s_t, long long s_r,
                                                 long long s_c, int accumulate, int tile, float* red, int order) {
    constexpr int J = T_ * RJ;
    const int cl = threadIdx.x & 31, zg = threadIdx.x >> 5;
    const int tiles_c = (C + 31) >> 5;
    int tr, tc;
    if (order == 2) {
        // r tiles fastest inside XCD-contiguous runs: the J-float runs of neighbouring r tiles continue each other in the parameter
        // (same c), so the partial 64-byte lines at their edges meet in ONE L2 instead of being merged in memory
        const int tiles_r = (R + RJ - 1) / RJ;
        const int vt = cdf_xcd_order(tile, tiles_c * tiles_r);
        tc = vt / tiles_r;
        tr = vt - tc * tiles_r;
    } else {
        tr = tile / tiles_c;
        tc = tile - tr * tiles_c;
    }
    const int c0 = tc * 32, r0 = tr * RJ;
    const long long slab = (long long)T_ * R * ldc;
    const int cc = c0 + cl < C ? c0 + cl : C - 1;
    int roff[J];
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int r = r0 + j / T_, t = j % T_;
        roff[j] = (t * R + (r < R ? r : R - 1)) * ldc + cc;
    }
    float acc[J];
#pragma unroll
    for (int j = 0; j < J; ++j) acc[j] = 0.f;
    for (int z = zg; z < nsplit; z += 8) {
        const float* p = ws + (long long)z * slab;
        float v[J];
#pragma unroll
        for (int j = 0; j < J; ++j) v[j] = p[roff[j]];
#pragma unroll
        for (int j = 0; j < J; ++j) acc[j] += v[j];
    }
#pragma unroll
    for (int j = 0; j < J; ++j) red[(zg * J + j) * 33 + cl] = acc[j];
    __syncthreads();
    // all of a thread's read-modify-writes in flight together (unconditional loads from a clamped address, predicated stores)
    constexpr int NE = (32 * J + 255) / 256;
    float tot[NE], old[NE];
    float* dst[NE];
    bool ok[NE];
#pragma unroll
    for (int k = 0; k < NE; ++k) {
        const int e = threadIdx.x + 256 * k;
        const int ee = e < 32 * J ? e : 0;
        const int c_l = ee / J, j = ee - c_l * J;
        tot[k] = 0.f;
#pragma unroll
        for (int q = 0; q < 8; q += 4)
            tot[k] += (red[(q * J + j) * 33 + c_l] + red[((q + 1) * J + j) * 33 + c_l]) + (red[((q + 2) * J + j) * 33 + c_l] + red[((q + 3) * J + j) * 33 + c_l]);
        const int c = c0 + c_l, r = r0 + j / T_, t = j % T_;
        ok[k] = e < 32 * J && c < C && r < R;
        dst[k] = ok[k] ? g + c * s_c + r * s_r + t * s_t : g;
    }
    if (accumulate) {
#pragma unroll
        for (int k = 0; k < NE; ++k) old[k] = *dst[k];
#pragma unroll
        for (int k = 0; k < NE; ++k) tot[k] += old[k];
    }
#pragma unroll
    for (int k = 0; k < NE; ++k)
        if (ok[k]) *dst[k] = tot[k];
}

template <int T_, int RJ>
__global__ void __launch_bounds__(256) unpack_reduce_tiled_kernel(const float* ws, float* g, int nsplit, int R, int C, int ldc, long long s_t,
                                                                   long long s_r, long long s_c, int accumulate, const float* bws, float* gb,
                                                                   int bC, int bld, int order) {
    __shared__ float red[8 * T_ * RJ * 33 > 8 * 33 ? 8 * T_ * RJ * 33 : 8 * 33];
    if (blockIdx.y == 1) {                                   // the fused bias reduction: a [1][1][bC] tensor, unit strides
        if ((int)blockIdx.x < (bC + 31) / 32) unpack_tile_body<1, 1>(bws, gb, nsplit, 1, bC, bld, 0, 0, 1, accumulate, blockIdx.x, red, 1);
        return;
    }
    unpack_tile_body<T_, RJ>(ws, g, nsplit, R, C, ldc, s_t, s_r, s_c, accumulate, blockIdx.x, red, order);
}

// column sums of a row-major matrix with pitch, two deterministic stages:
//   stage 1: part[(seg*nchunk + chunk)][c] = sum_{r in chunk of segment} x[r*ld + c]
//   stage 2: out[seg][c] (+)= sum_chunk part
// grid1 = (ceil(C/64), nseg, nchunk); block = 256 = 4 row-lanes x 64 channels
template <bool BF>                                          // BF: x is a bf16 tensor (ld in bf16 elements), widened as it is read
__global__ void colsum_partial_kernel(const void* xv, float* part, int rows_per_seg, int rows_per_chunk, int C, int ld) {
    typedef typename cdf_quad<BF>::elem elem_t;
    const elem_t* x = (const elem_t*)xv;
    __shared__ float red[4][64];
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), rl = threadIdx.x >> 6;
    const int r0 = blockIdx.z * rows_per_chunk;
    int r1 = r0 + rows_per_chunk;
    if (r1 > rows_per_seg) r1 = rows_per_seg;
    const elem_t* p = x + (long long)blockIdx.y * rows_per_seg * ld;
    float s = 0.f;
    if (c < C) {
        // 8 independent rows in flight per lane (a one-load-per-trip loop crawled at 0.6 TB/s)
        elem_t t[8];
        int r = r0 + rl;
        for (; r + 28 < r1; r += 32) {
#pragma unroll
            for (int u = 0; u < 8; ++u) t[u] = p[(long long)(r + 4 * u) * ld + c];
            s += ((cdf_widen(t[0]) + cdf_widen(t[1])) + (cdf_widen(t[2]) + cdf_widen(t[3]))) +
                 ((cdf_widen(t[4]) + cdf_widen(t[5])) + (cdf_widen(t[6]) + cdf_widen(t[7])));
        }
        for (; r < r1; r += 4) s += cdf_widen(p[(long long)r * ld + c]);
    }
    red[rl][threadIdx.x & 63] = s;
    __syncthreads();
    if (rl == 0 && c < C) {
        const int l = threadIdx.x;
        part[((long long)blockIdx.y * gridDim.z + blockIdx.z) * C + c] = (red[0][l] + red[1][l]) + (red[2][l] + red[3][l]);
    }
}
__global__ void __launch_bounds__(1024) colsum_final_kernel(const float* part, float* out, int nchunk, int C, int ldo, int accumulate) {
    __shared__ float red[16][64];               // 16 partial lanes x 64 columns
    const int l = threadIdx.x & 63, rl = threadIdx.x >> 6, c = blockIdx.x * 64 + l;
    float s = 0.f;
    if (c < C) {
        const float* p = part + (long long)blockIdx.y * nchunk * C + c;
        for (int k = rl; k < nchunk; k += 16) s += p[(long long)k * C];
    }
    red[rl][l] = s;
    __syncthreads();
    if (rl == 0 && c < C) {
        float t = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) t += red[r][l];
        float* dst = out + (long long)blockIdx.y * ldo + c;
        *dst = accumulate ? *dst + t : t;
    }
}

static int launch_unpack_reduce(const float* ws, float* g, int nsplit, int T, int R, int C, int ldc, long long s_t, long long s_r,
                                long long s_c, int accumulate, const float* bws, float* gb, int bC, int bld, int tiled, hipStream_t s) {
    const int tiled_mode = tiled ? 1 : 0;                    // (1: c tiles fastest; an r-tiles-fastest-per-XCD order measured no different and is gone)
    if (s_c != 1 && C >= 32 && (T == 1 || T == 9 || T == 16) && tiled_mode) {
        const int RJ = T == 9 ? 4 : (T == 16 ? 2 : 32);
        const long long tiles = (long long)((C + 31) / 32) * ((R + RJ - 1) / RJ);
        if (tiles < (1 << 30) && (!bws || (bC + 31) / 32 <= tiles)) {
            const dim3 tg((unsigned)tiles, bws ? 2 : 1);
            if (T == 9)
                CDF_LAUNCH((unpack_reduce_tiled_kernel<9, 4>), tg, dim3(256), 0, s, ws, g, nsplit, R, C, ldc, s_t, s_r, s_c, accumulate, bws, gb, bC, bld, tiled_mode);
            else if (T == 16)
                CDF_LAUNCH((unpack_reduce_tiled_kernel<16, 2>), tg, dim3(256), 0, s, ws, g, nsplit, R, C, ldc, s_t, s_r, s_c, accumulate, bws, gb, bC, bld, tiled_mode);
            else
                CDF_LAUNCH((unpack_reduce_tiled_kernel<1, 32>), tg, dim3(256), 0, s, ws, g, nsplit, R, C, ldc, s_t, s_r, s_c, accumulate, bws, gb, bC, bld, tiled_mode);
            return cdf_check_launch("unpack_reduce_tiled");
        }
    }
    const dim3 grid(cdf_ew_grid4k((long long)T * R * C * 4), bws ? 2 : 1);
    if (nsplit >= 32)       // 16 slab lanes: every lane still has >= 2 slabs
        CDF_LAUNCH(unpack_reduce_kernel<16>, grid, dim3(1024), 0, s, ws, g, nsplit, T, R, C, ldc, s_t, s_r, s_c, accumulate, bws, gb, bC, bld);
    else
        CDF_LAUNCH(unpack_reduce_kernel<4>, grid, dim3(256), 0, s, ws, g, nsplit, T, R, C, ldc, s_t, s_r, s_c, accumulate, bws, gb, bC, bld);
    return cdf_check_launch("unpack_reduce");
}

extern "C" int cdf_unpack_reduce(const float* ws, float* g, int nsplit, int T, int R, int C, int ldc, long long s_t,
                                 long long s_r, long long s_c, int accumulate, int tiled, void* stream) {
    CDF_REQUIRE(ws && g && nsplit > 0 && T > 0 && R > 0 && C > 0 && ldc >= C, "cdf_unpack_reduce: bad args");
    return launch_unpack_reduce(ws, g, nsplit, T, R, C, ldc, s_t, s_r, s_c, accumulate, nullptr, nullptr, 0, 0, tiled, CDF_S);
}

extern "C" int cdf_unpack_reduce_bias(const float* ws, float* g, int nsplit, int T, int R, int C, int ldc, long long s_t,
                                      long long s_r, long long s_c, const float* bias_ws, float* gbias, int bias_ld, int accumulate,
                                      int tiled, void* stream) {
    CDF_REQUIRE(ws && g && bias_ws && gbias && nsplit > 0 && T > 0 && R > 0 && C > 0 && ldc >= C && bias_ld >= C, "cdf_unpack_reduce_bias: bad args");
    return launch_unpack_reduce(ws, g, nsplit, T, R, C, ldc, s_t, s_r, s_c, accumulate, bias_ws, gbias, C, bias_ld, tiled, CDF_S);
}

extern "C" int cdf_colsum_nchunk(int rows_per_seg) {
    int n = rows_per_seg / 512;
    if (n < 1) n = 1;
    if (n > 1024) n = 1024;
    return n;
}

// ws: >= nseg * cdf_colsum_nchunk(rows_per_seg) * C floats
extern "C" int cdf_colsum_io(const void* x, float* out, float* ws, int nseg, int rows_per_seg, int C, int ld, int ldo,
                             int accumulate, int x_bf16, void* stream) {
    CDF_REQUIRE(x && out && ws && nseg > 0 && rows_per_seg > 0 && C > 0 && ld >= C && ldo >= C, "cdf_colsum: bad args");
    const int nchunk = cdf_colsum_nchunk(rows_per_seg);
    const int rpc = cdf_cdiv(rows_per_seg, nchunk);
    if (x_bf16)
        CDF_LAUNCH(colsum_partial_kernel<true>, dim3(cdf_cdiv(C, 64), nseg, nchunk), dim3(256), 0, CDF_S, x, ws, rows_per_seg, rpc, C, ld);
    else
        CDF_LAUNCH(colsum_partial_kernel<false>, dim3(cdf_cdiv(C, 64), nseg, nchunk), dim3(256), 0, CDF_S, x, ws, rows_per_seg, rpc, C, ld);
    CDF_LAUNCH(colsum_final_kernel, dim3(cdf_cdiv(C, 64), nseg), dim3(1024), 0, CDF_S, (const float*)ws, out, nchunk, C, ldo, accumulate);
    return cdf_check_launch("colsum");
}
extern "C" int cdf_colsum(const float* x, float* out, float* ws, int nseg, int rows_per_seg, int C, int ld, int ldo,
                          int accumulate, void* stream) {
    return cdf_colsum_io(x, out, ws, nseg, rows_per_seg, C, ld, ldo, accumulate, 0, stream);
}
