// k_prdc.hip — the two k-NN passes behind improved precision / recall (Kynkaanniemi et al. 2019, torch-fidelity's `prc`) and density /
// coverage (Naeem et al. 2020) of two fp64 feature sets, on v_mfma_f64_16x16x4_f64 (the tile form of cdf_f64_tile.h: its X Y^T loader and its accumulator map).
//
// Definitions (include/colddiff.h holds the same text; colddiff/metrics.py prdc_device builds the four numbers from them).  X: n rows,
// Y: m rows, d features, neighbourhood size k.  Every comparison is on SQUARED Euclidean distances in fp64, no square root is taken:
//     D(a, b) = max(0, (|a|^2 + |b|^2) - 2 a.b)
// a.b comes from the matrix cores (k ascending, whichever operand a row is); |a|^2 is the caller's vector, computed once per row per call
// by cdf_rowsumsq_f64.  Every operation of D is commutative in (a, b), so D of a pair of rows is the same number in whichever tile, call
// or operand position it is computed.  Features must be finite (documented, not checked).
//     knn_X[j][0..k) ascending: the k smallest of { D(x_j, x_l) : l != j };   rho_X(j) = knn_X[j][k - 1]
// Self is left out BY POSITION, not by value: a second row with the same values is a neighbour at distance 0.
//     precision = #{ i : exists j, D(y_i, x_j) <= rho_X(j) } / m        recall   = #{ j : exists i, D(x_j, y_i) <= rho_Y(i) } / n
//     density   = sum_i #{ j : D(y_i, x_j) <= rho_X(j) } / (k m)        coverage = #{ j : exists i, D(x_j, y_i) <= rho_X(j) } / n
// `<=` throughout (torch-fidelity's choice; Naeem's reference code has `<`: they differ on exact ties only).
//
// Both main kernels: grid (row tiles of 64, S column splits); block (bi, s) walks the column tiles of its split, one fid_tile_abt per
// tile, and consumes the 64 x 64 tile of D in the epilogue -- nothing of size n^2 goes to memory.  The FULL square is walked by the k-NN
// kernel (the upper-triangle form that updates rows and columns from one tile was not built).  Per-split results go to `partial`, a fold
// kernel joins them.  No atomics, every element of partial and of the outputs is written by the call that owns it, lists are multisets of
// values and counts are integers: two runs are bit-identical.
#include <math.h>

#include "cdf_common.h"
#include "cdf_f64_tile.h"
#include "colddiff.h"

#define PRDC_BLOCKS 1024    // blocks a launch aims at: the 256 CUs four times over
#define PRDC_DP 65          // row pitch of the D tile parked in LDS, in doubles (64 x 65 of the 5120 doubles)
#define PRDC_KMAX 8
#define PRDC_NMAX (1 << 30)  // rows per set: row numbers and 64 bi + r stay inside an int

// Column tiles per split and the number of splits for `rt` row tiles and `ct` column tiles: S = min(ct, PRDC_BLOCKS / rt), at least 1,
// then re-divided so that no split is empty.
static inline int prdc_per_split(int rt, int ct) {
    int s = PRDC_BLOCKS / rt;
    s = s < 1 ? 1 : (s > ct ? ct : s);
    return cdf_cdiv(ct, s);
}
static inline int prdc_splits(int rt, int ct) { return cdf_cdiv(ct, prdc_per_split(rt, ct)); }

// D of the lane's accumulator (i, j, r) is row bi 64 + fid_tile_row(i, r), column bj 64 + fid_tile_col(j); both kernels walk j outermost, with
// what belongs to a column (its norm, its radius) loaded once per j
__device__ __forceinline__ double prdc_dist(double na, double nb, double ab) { return fmax(0.0, (na + nb) - 2.0 * ab); }

// v into the ascending list (the largest element drops out); no branch, no index: the list stays in registers
template <int KL>
__device__ __forceinline__ void prdc_insert(double (&list)[KL], double v) {
#pragma unroll
    for (int q = 0; q < KL; ++q) {
        const double lo = fmin(list[q], v);
        v = fmax(list[q], v);
        list[q] = lo;
    }
}

// grid (ceil(n / 64), S): partial[s][row][0..k) = the k smallest D(x_row, x_l), l != row, over the columns of split s, ascending (+inf
// where the split has fewer than k columns beside row).  The tile of D is parked in the operand LDS (free after fid_tile_abt's last
// barrier); thread t scans the 16 columns (t & 3) + 4 c of row t >> 2 into its own list, the four lists of a row meet once, after the walk.
template <int KL>
__global__ void __launch_bounds__(256) knn_sq_kernel(const double* X, int ldx, int n, int d, int k, int per, const double* norms,
                                                     double* partial) {
    __shared__ double s[4 * FID_BK * FID_P];
    const int bi = blockIdx.x, T = (n - 1) / FID_T + 1;
    const int bj0 = blockIdx.y * per, bj1 = bj0 + per < T ? bj0 + per : T;
    const int tid = threadIdx.x, srow = tid >> 2, sq = tid & 3;
    double rn[2][4];                                            // |x|^2 of this lane's eight accumulator rows
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = bi * FID_T + fid_tile_row(i, r);
            rn[i][r] = row < n ? norms[row] : 0.0;
        }
    double list[KL];
#pragma unroll
    for (int q = 0; q < KL; ++q) list[q] = INFINITY;
    for (int bj = bj0; bj < bj1; ++bj) {
        f64x4_t acc[2][2];
        fid_acc_zero(acc);
        fid_tile_abt(s, X, ldx, bi * FID_T, n, X, ldx, bj * FID_T, n, 0, d, acc);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = bj * FID_T + fid_tile_col(j);
            const double cn = col < n ? norms[col] : 0.0;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = bi * FID_T + fid_tile_row(i, r);
                    s[fid_tile_row(i, r) * PRDC_DP + fid_tile_col(j)] = col < n && col != row ? prdc_dist(rn[i][r], cn, acc[i][j][r]) : INFINITY;
                }
        }
        __syncthreads();
#pragma unroll 4
        for (int c = 0; c < 16; ++c) {
            const double v = s[srow * PRDC_DP + sq + 4 * c];
            if (v < list[KL - 1]) prdc_insert(list, v);
        }
        __syncthreads();                                        // (the next tile's operands overwrite s)
    }
    // the four lists of a row: s[row][quarter][KL]; quarter 0 takes the other three in
#pragma unroll
    for (int q = 0; q < KL; ++q) s[(srow * 4 + sq) * KL + q] = list[q];
    __syncthreads();
    if (sq == 0) {
        for (int o = 1; o < 4; ++o)
#pragma unroll
            for (int q = 0; q < KL; ++q) prdc_insert(list, s[(srow * 4 + o) * KL + q]);
        const int row = bi * FID_T + srow;
        if (row < n) {
            double* dst = partial + ((size_t)blockIdx.y * n + row) * k;
#pragma unroll
            for (int q = 0; q < KL; ++q)
                if (q < k) dst[q] = list[q];
        }
    }
}

// thread per row: the S ascending lists of a row -> knn[row][0..k)
__global__ void __launch_bounds__(256) knn_fold_kernel(const double* partial, int n, int k, int S, double* knn) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= n) return;
    double list[PRDC_KMAX];
#pragma unroll
    for (int q = 0; q < PRDC_KMAX; ++q) list[q] = INFINITY;
    for (int sp = 0; sp < S; ++sp) {
        const double* src = partial + ((size_t)sp * n + row) * k;
        for (int q = 0; q < k; ++q) prdc_insert(list, src[q]);
    }
#pragma unroll
    for (int q = 0; q < PRDC_KMAX; ++q)
        if (q < k) knn[(size_t)row * k + q] = list[q];
}

// grid (ceil(na / 64), S): partial[s][row] = {#{ j in split s : D(a_row, b_j) <= rcol[j] }, #{ j in split s : D(a_row, b_j) <= rrow[row] }}
// (0 for a side whose radius pointer is null).  Both counts come from the lane's 16 accumulators in registers; the 32 lanes that share a
// row meet through LDS once, after the walk.
__global__ void __launch_bounds__(256) ball_counts_kernel(const double* A, int lda, int na, const double* anorm, const double* B, int ldb,
                                                          int nb, const double* bnorm, int d, int per, const double* rcol,
                                                          const double* rrow, int* partial) {
    __shared__ double s[4 * FID_BK * FID_P];
    const int bi = blockIdx.x, T = (nb - 1) / FID_T + 1;
    const int bj0 = blockIdx.y * per, bj1 = bj0 + per < T ? bj0 + per : T;
    double rn[2][4], rr[2][4];                                  // |a|^2 and the row radius of this lane's eight accumulator rows
    int ccol[2][4], crow[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = bi * FID_T + fid_tile_row(i, r);
            rn[i][r] = row < na ? anorm[row] : 0.0;
            rr[i][r] = rrow && row < na ? rrow[row] : -1.0;     // (D >= 0: a radius of -1 counts nothing)
            ccol[i][r] = crow[i][r] = 0;
        }
    for (int bj = bj0; bj < bj1; ++bj) {
        f64x4_t acc[2][2];
        fid_acc_zero(acc);
        fid_tile_abt(s, A, lda, bi * FID_T, na, B, ldb, bj * FID_T, nb, 0, d, acc);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = bj * FID_T + fid_tile_col(j);
            const bool in = col < nb;
            const double cn = in ? bnorm[col] : 0.0;
            const double rc = rcol && in ? rcol[col] : -1.0;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double D = prdc_dist(rn[i][r], cn, acc[i][j][r]);
                    ccol[i][r] += D <= rc ? 1 : 0;
                    crow[i][r] += in && D <= rr[i][r] ? 1 : 0;
                }
        }
    }
    // cnt[row][32 lanes of that row][2] as ints in the operand LDS (every wave is past its reads of s: fid_tile_abt's last barrier; a
    // block without a tile has not touched s)
    int* cnt = (int*)s;
    const int slot = fid_wave_col() * 16 + (threadIdx.x & 15);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            cnt[(fid_tile_row(i, r) * 32 + slot) * 2 + 0] = ccol[i][r];
            cnt[(fid_tile_row(i, r) * 32 + slot) * 2 + 1] = crow[i][r];
        }
    __syncthreads();
    const int tid = threadIdx.x;
    if (tid < 128) {
        const int lrow = tid >> 1, side = tid & 1, row = bi * FID_T + lrow;
        int v = 0;
        for (int o = 0; o < 32; ++o) v += cnt[(lrow * 32 + o) * 2 + side];
        if (row < na) partial[((size_t)blockIdx.y * na + row) * 2 + side] = v;
    }
}

// thread per row: the S partial pairs of a row -> cnt_col[row], cnt_row[row] (a null output is not touched)
__global__ void __launch_bounds__(256) ball_fold_kernel(const int* partial, int na, int S, int* cnt_col, int* cnt_row) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= na) return;
    int c = 0, r = 0;
    for (int sp = 0; sp < S; ++sp) {
        c += partial[((size_t)sp * na + row) * 2 + 0];
        r += partial[((size_t)sp * na + row) * 2 + 1];
    }
    if (cnt_col) cnt_col[row] = c;
    if (cnt_row) cnt_row[row] = r;
}

extern "C" int cdf_knn_splits(int n) {
    if (n < 2 || n > PRDC_NMAX) return 0;
    const int t = cdf_cdiv(n, FID_T);
    return prdc_splits(t, t);
}

extern "C" int cdf_ball_splits(int na, int nb) {
    if (na < 1 || nb < 1 || na > PRDC_NMAX || nb > PRDC_NMAX) return 0;
    return prdc_splits(cdf_cdiv(na, FID_T), cdf_cdiv(nb, FID_T));
}

extern "C" int cdf_knn_sq_f64(const double* x, int ldx, int n, int d, int k, const double* norms, double* partial, double* knn,
                              void* stream) {
    CDF_REQUIRE(x && norms && partial && knn, "cdf_knn_sq_f64: null pointer");
    CDF_REQUIRE(k >= 1 && k <= PRDC_KMAX, "cdf_knn_sq_f64: k must be in [1, %d] (got %d)", PRDC_KMAX, k);
    CDF_REQUIRE(n >= k + 1, "cdf_knn_sq_f64: n must be at least k + 1 (got n = %d, k = %d): a row is not its own neighbour", n, k);
    CDF_REQUIRE(n <= PRDC_NMAX, "cdf_knn_sq_f64: n = %d is more than 2^30 rows", n);
    CDF_REQUIRE(d >= 1, "cdf_knn_sq_f64: d must be at least 1 (got %d)", d);
    CDF_REQUIRE(ldx >= d, "cdf_knn_sq_f64: ldx (%d) is smaller than d (%d)", ldx, d);
    const int T = cdf_cdiv(n, FID_T), per = prdc_per_split(T, T), S = prdc_splits(T, T);
    if (k <= 4)
        CDF_LAUNCH(knn_sq_kernel<4>, dim3(T, S), dim3(256), 0, CDF_S, x, ldx, n, d, k, per, norms, partial);
    else
        CDF_LAUNCH(knn_sq_kernel<8>, dim3(T, S), dim3(256), 0, CDF_S, x, ldx, n, d, k, per, norms, partial);
    CDF_LAUNCH(knn_fold_kernel, dim3(cdf_cdiv(n, 256)), dim3(256), 0, CDF_S, (const double*)partial, n, k, S, knn);
    return cdf_check_launch("knn_sq_f64");
}

extern "C" int cdf_ball_counts_f64(const double* a, int lda, int na, const double* anorm, const double* b, int ldb, int nb,
                                   const double* bnorm, int d, const double* rcol, const double* rrow, int* partial, int* cnt_col,
                                   int* cnt_row, void* stream) {
    CDF_REQUIRE(a && anorm && b && bnorm && partial, "cdf_ball_counts_f64: null pointer");
    CDF_REQUIRE(!rcol || cnt_col, "cdf_ball_counts_f64: rcol without cnt_col (null pointer)");
    CDF_REQUIRE(!rrow || cnt_row, "cdf_ball_counts_f64: rrow without cnt_row (null pointer)");
    CDF_REQUIRE(na >= 1 && nb >= 1 && d >= 1, "cdf_ball_counts_f64: na, nb and d must be at least 1 (got na = %d, nb = %d, d = %d)", na, nb, d);
    CDF_REQUIRE(na <= PRDC_NMAX && nb <= PRDC_NMAX, "cdf_ball_counts_f64: na = %d or nb = %d is more than 2^30 rows", na, nb);
    CDF_REQUIRE(lda >= d, "cdf_ball_counts_f64: lda (%d) is smaller than d (%d)", lda, d);
    CDF_REQUIRE(ldb >= d, "cdf_ball_counts_f64: ldb (%d) is smaller than d (%d)", ldb, d);
    const int Ta = cdf_cdiv(na, FID_T), Tb = cdf_cdiv(nb, FID_T), per = prdc_per_split(Ta, Tb), S = prdc_splits(Ta, Tb);
    CDF_LAUNCH(ball_counts_kernel, dim3(Ta, S), dim3(256), 0, CDF_S, a, lda, na, anorm, b, ldb, nb, bnorm, d, per, rcol, rrow, partial);
    CDF_LAUNCH(ball_fold_kernel, dim3(cdf_cdiv(na, 256)), dim3(256), 0, CDF_S, (const int*)partial, na, S, rcol ? cnt_col : (int*)nullptr,
               rrow ? cnt_row : (int*)nullptr);
    return cdf_check_launch("ball_counts_f64");
}
