// cdf_f64_tile.h — the one home of the 64 x 64 fp64 tile form on v_mfma_f64_16x16x4_f64.  256 threads own a 64 x 64 tile of the result,
// each wave a 32 x 32 quarter = 2 x 2 MFMA tiles = 16 fp64 accumulators.  K advances in chunks of FID_BK through two LDS buffers per
// operand, both kept [k][column of the tile] with a row pitch of 80 doubles (see the header of k_fid.hip for the bank arithmetic).
// What lives here, and who uses it:
//   fid_k_loop                           the K pipeline (fetch / MFMA / put / one barrier): gemm_f64_kernel of k_fid.hip with a loader of its
//                                        own, everyone else through the X Y^T loader.  (moments_f64_kernel of k_fid.hip keeps the same
//                                        pipeline as macro text of its own: on this loop it measured 1.4 .. 2.5 % slower, see
//                                        profiles/f64_tile_family_ab.txt; it shares fid_chunk_mma and the constants.)
//   fid_tile_abt, fid_tile_abt_indexed   the X Y^T loader on that loop: k_gmm.hip (Cholesky trailing update, triangular inverse), k_prdc.hip
//                                        (distance tiles), k_kid.hip (Gram tiles of index-selected rows)
//   fid_tile_row / fid_tile_col / fid_tile_each   which element of the tile a lane's accumulator (i, j, r) is: every epilogue of the family
//                                        but moments_f64_kernel's
// A kernel keeps only what is its own: which elements it loads, where it puts them and what it does with the tile.
#pragma once
#include "cdf_common.h"

#define FID_T 64     // tile edge
#define FID_BK 16    // K chunk
#define FID_P 80     // LDS row pitch in doubles

// ---- the accumulator map ----------------------------------------------------------------------------------------------------------------
// Wave w owns the quarter (w >> 1, w & 1); accumulator (i, j, r) of a lane is tile row fid_tile_row(i, r), tile column fid_tile_col(j)
// (cdf_mfma_f64_16x16x4: register r of lane l is row (l >> 4) + 4 r, column l & 15 of its 16 x 16 block).
__device__ __forceinline__ int fid_wave_row() { return threadIdx.x >> 7; }
__device__ __forceinline__ int fid_wave_col() { return (threadIdx.x >> 6) & 1; }
__device__ __forceinline__ int fid_tile_row(int i, int r) { return fid_wave_row() * 32 + i * 16 + ((threadIdx.x & 63) >> 4) + 4 * r; }
__device__ __forceinline__ int fid_tile_col(int j) { return fid_wave_col() * 32 + j * 16 + (threadIdx.x & 15); }

// f(tile row, tile column, value) for the lane's 16 accumulators in register order: i, then j, then r.  A kernel that hoists per-column
// work between j and r writes the loops itself on fid_tile_row / fid_tile_col.
template <class F>
__device__ __forceinline__ void fid_tile_each(const f64x4_t (&acc)[2][2], F f) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = fid_tile_col(j);
#pragma unroll
            for (int r = 0; r < 4; ++r) f(fid_tile_row(i, r), col, acc[i][j][r]);
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

// ---- the K pipeline ---------------------------------------------------------------------------------------------------------------------
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

// acc += the product over `nchunk` K chunks.  sa / sb: two buffers of [FID_BK][FID_P] each, back to back.  fetch(k) loads the caller's
// elements of the chunk that starts at k (k = 0, FID_BK, ...; the caller adds its own origin) into its registers, out-of-range ones as
// zeros; put(buf) writes those registers to buffer `buf` of sa and sb.  Chunk c + 1 is fetched before the MFMAs of chunk c and put into
// the other buffer after them: one barrier per chunk.  After that barrier chunk c + 1 is complete and every wave is past its reads of
// buffer c & 1, which chunk c + 2 overwrites.  Every wave is past ALL its LDS reads when this returns (the loop's last barrier), so the
// caller may overwrite the buffers.
template <class Fetch, class Put>
__device__ __forceinline__ void fid_k_loop(const double* sa, const double* sb, int nchunk, f64x4_t (&acc)[2][2], Fetch fetch, Put put) {
    fetch(0);
    put(0);
    __syncthreads();
    for (int c = 0; c < nchunk; ++c) {
        const int cur = c & 1;
        if (c + 1 < nchunk) fetch((c + 1) * FID_BK);
        fid_chunk_mma(sa + cur * FID_BK * FID_P, sb + cur * FID_BK * FID_P, acc, fid_wave_row(), fid_wave_col(), threadIdx.x & 63);
        if (c + 1 < nchunk) put(cur ^ 1);
        __syncthreads();
    }
}

// ---- the X Y^T loader -------------------------------------------------------------------------------------------------------------------
// acc += x[k] y[k] over k in [k0, k1), where thread t brings row t >> 2 of both tiles: px / py point at that row of X / of Y (k along the
// row), xrow / yrow say whether the row exists -- a row that does not is zero and its pointer is not dereferenced.  s = 4 FID_BK FID_P
// doubles of LDS (40 KB): two buffers per operand.  A thread fetches 4 consecutive k (16 rows x 128 B per wave instruction) and writes
// them transposed, [k][row].  [k0, k1) must lie inside both rows.
__device__ __forceinline__ void fid_tile_abt_rows(double* s, const double* px, bool xrow, const double* py, bool yrow, int k0, int k1,
                                                  f64x4_t (&acc)[2][2]) {
    const int ar = threadIdx.x >> 2, ak = (threadIdx.x & 3) * 4;
    double* sa = s;
    double* sb = s + 2 * FID_BK * FID_P;
    double ra[4], rb[4];
    fid_k_loop(
        sa, sb, (k1 - k0 + FID_BK - 1) / FID_BK, acc,
        [&](int k) {
            const int kk = k0 + k + ak;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const bool kin = kk + q < k1;
                ra[q] = xrow && kin ? px[kk + q] : 0.0;
                rb[q] = yrow && kin ? py[kk + q] : 0.0;
            }
        },
        [&](int buf) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                sa[buf * FID_BK * FID_P + (ak + q) * FID_P + ar] = ra[q];
                sb[buf * FID_BK * FID_P + (ak + q) * FID_P + ar] = rb[q];
            }
        });
}

// acc += X[xr0 + r][k] Y[yr0 + c][k] over k in [k0, k1) for the tile (r, c) in [0, 64)^2: both operands row-major with k along the row (the
// product X Y^T), rows at or past xrows / yrows are zero.  [k0, k1) must lie inside both operands' rows (the callers' k ranges are whole
// 64-blocks below the matrix size).
__device__ __forceinline__ void fid_tile_abt(double* s, const double* X, int ldx, int xr0, int xrows, const double* Y, int ldy, int yr0,
                                             int yrows, int k0, int k1, f64x4_t (&acc)[2][2]) {
    const int ar = threadIdx.x >> 2;
    const bool xrow = xr0 + ar < xrows, yrow = yr0 + ar < yrows;
    fid_tile_abt_rows(s, X + (size_t)(xrow ? xr0 + ar : 0) * ldx, xrow, Y + (size_t)(yrow ? yr0 + ar : 0) * ldy, yrow, k0, k1, acc);
}

// fid_tile_abt with both operands' rows fetched through index arrays: tile row r of the first operand is row ix[xr0 + r] of X, tile row c
// of the second is row iy[yr0 + c] of Y; positions at or past xrows / yrows are zero rows and THEIR INDEX IS NOT READ (the arrays end at
// xrows / yrows).  k runs over [0, d).  The index VALUES are the caller's responsibility (each must be a row of its matrix).
__device__ __forceinline__ void fid_tile_abt_indexed(double* s, const double* X, int ldx, const int* ix, int xr0, int xrows, const double* Y,
                                                     int ldy, const int* iy, int yr0, int yrows, int d, f64x4_t (&acc)[2][2]) {
    const int ar = threadIdx.x >> 2;
    const bool xrow = xr0 + ar < xrows, yrow = yr0 + ar < yrows;
    fid_tile_abt_rows(s, X + (size_t)(xrow ? ix[xr0 + ar] : 0) * ldx, xrow, Y + (size_t)(yrow ? iy[yr0 + ar] : 0) * ldy, yrow, 0, d, acc);
}
