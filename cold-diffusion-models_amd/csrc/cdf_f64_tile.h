// cdf_f64_tile.h — the 64 x 64 fp64 tile form on v_mfma_f64_16x16x4_f64 that k_fid.hip (moments, GEMM), k_gmm.hip (Cholesky trailing
// update, triangular inverse) and k_kid.hip (polynomial-kernel Gram tiles of index-selected rows) share: 256 threads own a 64 x 64 tile of the result, each wave a 32 x 32 quarter = 2 x 2 MFMA tiles = 16 fp64
// accumulators.  K advances in chunks of FID_BK through two LDS buffers per operand, both kept [k][column of the tile] with a row pitch of
// 80 doubles (see the header of k_fid.hip for the bank arithmetic).
#pragma once
#include "cdf_common.h"

#define FID_T 64     // tile edge
#define FID_BK 16    // K chunk
#define FID_P 80     // LDS row pitch in doubles

// The MFMAs of one K chunk: sa / sb are [FID_BK][FID_P], this wave's quarter starts at column 32 wr of sa and 32 wc of sb.
__device__ __forceinline__ void fid_chunk_mma(const double* sa, const double* sb, f64x4_t (&acc)[2][2], int wr, int wc, int lane) {
    const int c16 = lane & 15, kq = lane >> 4;
#pragma unroll
    for (int ks = 0; ks < FID_BK; ks += 4) {
        double a[2], b[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            a[i] = sa[(ks + kq) * FID_P + wr * 32 + i * 16 + c16];
            b[i] = sb[(ks + kq) * FID_P + wc * 32 + i * 16 + c16];
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = cdf_mfma_f64_16x16x4(a[i], b[j], acc[i][j]);
    }
}

__device__ __forceinline__ void fid_acc_zero(f64x4_t (&acc)[2][2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[i][j][r] = 0.0;
}

// acc += X[xr0 + r][k] Y[yr0 + c][k] over k in [k0, k1) for the tile (r, c) in [0, 64)^2: both operands row-major with k along the row (the
// product X Y^T), rows at or past xrows / yrows are zero.  [k0, k1) must lie inside both operands' rows (the callers' k ranges are whole
// 64-blocks below the matrix size).  s = 4 FID_BK FID_P doubles of LDS (40 KB): two buffers per operand.  Thread -> row tid >> 2 of the
// tile, 4 consecutive k, written transposed as [k][row]; the same register prefetch / one barrier per chunk as gemm_f64_kernel.  Every wave
// is past its LDS reads when this returns (the loop's last barrier), so the caller may overwrite s.
__device__ __forceinline__ void fid_tile_abt(double* s, const double* X, int ldx, int xr0, int xrows, const double* Y, int ldy, int yr0,
                                             int yrows, int k0, int k1, f64x4_t (&acc)[2][2]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
    const int ar = tid >> 2, ak = (tid & 3) * 4;
    const bool xrow = xr0 + ar < xrows, yrow = yr0 + ar < yrows;
    const double* px = X + (size_t)(xrow ? xr0 + ar : 0) * ldx;
    const double* py = Y + (size_t)(yrow ? yr0 + ar : 0) * ldy;
    double* sa = s;
    double* sb = s + 2 * FID_BK * FID_P;
    double ra[4], rb[4];
    const int nchunk = (k1 - k0 + FID_BK - 1) / FID_BK;
#define FID_ABT_FETCH(kk)                                                       \
    do {                                                                        \
        _Pragma("unroll") for (int q = 0; q < 4; ++q) {                         \
            const bool kin = (kk) + ak + q < k1;                                \
            ra[q] = xrow && kin ? px[(kk) + ak + q] : 0.0;                      \
            rb[q] = yrow && kin ? py[(kk) + ak + q] : 0.0;                      \
        }                                                                       \
    } while (0)
#define FID_ABT_PUT(buf)                                                        \
    do {                                                                        \
        _Pragma("unroll") for (int q = 0; q < 4; ++q) {                         \
            sa[(buf) * FID_BK * FID_P + (ak + q) * FID_P + ar] = ra[q];         \
            sb[(buf) * FID_BK * FID_P + (ak + q) * FID_P + ar] = rb[q];         \
        }                                                                       \
    } while (0)
    FID_ABT_FETCH(k0);
    FID_ABT_PUT(0);
    __syncthreads();
    for (int c = 0; c < nchunk; ++c) {
        const int cur = c & 1;
        if (c + 1 < nchunk) FID_ABT_FETCH(k0 + (c + 1) * FID_BK);
        fid_chunk_mma(sa + cur * FID_BK * FID_P, sb + cur * FID_BK * FID_P, acc, wr, wc, lane);
        if (c + 1 < nchunk) FID_ABT_PUT(cur ^ 1);
        __syncthreads();
    }
#undef FID_ABT_FETCH
#undef FID_ABT_PUT
}

// fid_tile_abt with both operands' rows fetched through index arrays: tile row r of the first operand is row ix[xr0 + r] of X, tile row c
// of the second is row iy[yr0 + c] of Y; positions at or past xrows / yrows are zero rows and their index is not read.  k runs over
// [0, d).  The index VALUES are the caller's responsibility (each must be a row of its matrix).  Same LDS, prefetch and barrier form.
__device__ __forceinline__ void fid_tile_abt_indexed(double* s, const double* X, int ldx, const int* ix, int xr0, int xrows, const double* Y,
                                                     int ldy, const int* iy, int yr0, int yrows, int d, f64x4_t (&acc)[2][2]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
    const int ar = tid >> 2, ak = (tid & 3) * 4;
    const bool xrow = xr0 + ar < xrows, yrow = yr0 + ar < yrows;
    const double* px = X + (size_t)(xrow ? ix[xr0 + ar] : 0) * ldx;
    const double* py = Y + (size_t)(yrow ? iy[yr0 + ar] : 0) * ldy;
    double* sa = s;
    double* sb = s + 2 * FID_BK * FID_P;
    double ra[4], rb[4];
    const int nchunk = (d + FID_BK - 1) / FID_BK;
#define FID_ABTI_FETCH(kk)                                                      \
    do {                                                                        \
        _Pragma("unroll") for (int q = 0; q < 4; ++q) {                         \
            const bool kin = (kk) + ak + q < d;                                 \
            ra[q] = xrow && kin ? px[(kk) + ak + q] : 0.0;                      \
            rb[q] = yrow && kin ? py[(kk) + ak + q] : 0.0;                      \
        }                                                                       \
    } while (0)
#define FID_ABTI_PUT(buf)                                                       \
    do {                                                                        \
        _Pragma("unroll") for (int q = 0; q < 4; ++q) {                         \
            sa[(buf) * FID_BK * FID_P + (ak + q) * FID_P + ar] = ra[q];         \
            sb[(buf) * FID_BK * FID_P + (ak + q) * FID_P + ar] = rb[q];         \
        }                                                                       \
    } while (0)
    FID_ABTI_FETCH(0);
    FID_ABTI_PUT(0);
    __syncthreads();
    for (int c = 0; c < nchunk; ++c) {
        const int cur = c & 1;
        if (c + 1 < nchunk) FID_ABTI_FETCH((c + 1) * FID_BK);
        fid_chunk_mma(sa + cur * FID_BK * FID_P, sb + cur * FID_BK * FID_P, acc, wr, wc, lane);
        if (c + 1 < nchunk) FID_ABTI_PUT(cur ^ 1);
        __syncthreads();
    }
#undef FID_ABTI_FETCH
#undef FID_ABTI_PUT
}
