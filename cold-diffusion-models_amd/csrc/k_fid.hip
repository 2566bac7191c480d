// k_fid.hip — FID on the device (the half that was still a host program): the fp64 statistics of feature
// batches and the fp64 GEMM behind the matrix square roots of the Frechet distance (Fid/fid_score.py:149-283: np.cov of an [N, 2048]
// host matrix and scipy.linalg.sqrtm of a 2048 x 2048 product).  Both of these kernels run on v_mfma_f64_16x16x4_f64.
//
// One tile form for both: 256 threads own a 64 x 64 tile of the result, each wave a 32 x 32 quarter = 2 x 2 MFMA tiles = 16 fp64
// accumulators (32 VGPRs).  K advances in chunks of 16 through two LDS buffers per operand; both operands are kept [k][column of the
// tile] with a row pitch of 80 doubles, so the fragment read of a k-step -- lanes 0-15 row k, 16-31 row k + 1 of one ds_read_b64 lane
// group, 16 consecutive doubles each -- lands on 2 x 32 distinct banks (80 doubles = 160 dwords = 32 banks past a multiple of 64).
// The next chunk is fetched into registers before the MFMAs of the current one and written to the other buffer after them: one barrier
// per chunk.  Out-of-range operand elements are zero, stores are guarded: any m, n, k.
//
// cdf_moments_f64 is that GEMM with A = Xc^T and B = Xc read from the same row stripes of X (coalesced along d, widened to fp64, pivot
// subtracted in fp64, the n tail and the columns past d zero AFTER the subtraction), restricted to the upper block triangle, and an
// epilogue that adds to the tile it read.  Floor of one call: the read-modify-write of the accumulator's triangle, ~ d^2 * 8 B (half the
// tiles, read and written) = 17 MB at d = 2048, ~4 us at HBM speed if it were alone -- not the 2 n d^2 = 0.42 GFLOP of a batch of 50.
// cdf_gemm_f64 at 2048^3: 17.2 GFLOP; each operand element is read by 32 tiles (2 x 1 GB through L2), C written once (34 MB).
//
// cdf_moments_merge_f64 (the last kernel of the file) joins two such accumulators; it has moments_f64_kernel's tile ownership and no MFMA.
#include "cdf_common.h"
#include "cdf_f64_tile.h"     // the tile form that k_gmm.hip, k_kid.hip and k_prdc.hip share; the loaders here are this file's own
#include "colddiff.h"

// ---- c = alpha a b + diag I --------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) gemm_f64_kernel(const double* A, int lda, const double* B, int ldb, double* C, int ldc, int M, int N,
                                                      int K, double alpha, double diag) {
    __shared__ double sa[2][FID_BK * FID_P], sb[2][FID_BK * FID_P];
    const int tid = threadIdx.x;
    const int m0 = blockIdx.y * FID_T, n0 = blockIdx.x * FID_T;
    // a: thread -> row tid >> 2 of the tile, 4 consecutive k (16 rows x 128 B per wave instruction); written transposed, [k][row]
    const int ar = tid >> 2, ak = (tid & 3) * 4;
    // b: thread -> k row tid >> 4, 4 consecutive columns
    const int bk = tid >> 4, bn = (tid & 15) * 4;
    const bool arow = m0 + ar < M;
    const double* pa = A + (size_t)(arow ? m0 + ar : 0) * lda;
    double ra[4], rb[4];
    f64x4_t acc[2][2];
    fid_acc_zero(acc);
    fid_k_loop(
        sa[0], sb[0], (K + FID_BK - 1) / FID_BK, acc,
        [&](int k0) {
            const bool brow = k0 + bk < K;
            const double* pak = pa + k0 + ak;                  // (one address per operand and chunk, the four loads at immediate offsets)
            const double* pb = B + (size_t)(brow ? k0 + bk : 0) * ldb + n0 + bn;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                ra[q] = arow && k0 + ak + q < K ? pak[q] : 0.0;
                rb[q] = brow && n0 + bn + q < N ? pb[q] : 0.0;
            }
        },
        [&](int buf) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                sa[buf][(ak + q) * FID_P + ar] = ra[q];
                sb[buf][bk * FID_P + bn + q] = rb[q];
            }
        });
    fid_tile_each(acc, [&](int r, int c, double v) {
        const int row = m0 + r, col = n0 + c;
        if (row < M && col < N) C[(size_t)row * ldc + col] = alpha * v + (row == col ? diag : 0.0);
    });
}

// ---- centred moments of a feature batch ------------------------------------------------------------------------------------------
// grid (T, T), T = ceil(d / 64): block (x = bj, y = bi) owns tile (bi, bj) of `outer` and leaves at once when bi > bj.  The diagonal
// blocks also own sum[64 bi ... 64 bi + 63]: each thread keeps the column sums of what it loads, 16 k rows are folded through LDS.
// The K pipeline and the accumulator map are written out here (the text of fid_k_loop / fid_tile_each): on the shared helpers this kernel
// measured slower at n = 50, d = 2048, the shape every FID batch has (profiles/f64_tile_family_ab.txt).
__global__ void __launch_bounds__(256) moments_f64_kernel(const float* X, int ldx, int n, int d, const double* pivot, double* sum,
                                                         double* outer, int ldo) {
    const int bi = blockIdx.y, bj = blockIdx.x;
    if (bi > bj) return;
    __shared__ double sa[2][FID_BK * FID_P], sb[2][FID_BK * FID_P];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
    const int lk = tid >> 4, lc = (tid & 15) * 4;                 // row of the stripe, 4 consecutive columns: 256 B of a row per 16 lanes
    const int ja = bi * FID_T + lc, jb = bj * FID_T + lc;
    double pva[4], pvb[4], ra[4], rb[4], csum[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        pva[q] = ja + q < d ? pivot[ja + q] : 0.0;
        pvb[q] = jb + q < d ? pivot[jb + q] : 0.0;
        csum[q] = 0.0;
    }
    f64x4_t acc[2][2];
    fid_acc_zero(acc);
    const int nchunk = (n + FID_BK - 1) / FID_BK;

#define FID_MOM_FETCH(i0)                                                                         \
    do {                                                                                          \
        const bool row = (i0) + lk < n;                                                           \
        const float* px = X + (size_t)(row ? (i0) + lk : 0) * ldx;                                \
        _Pragma("unroll") for (int q = 0; q < 4; ++q) {                                           \
            ra[q] = row && ja + q < d ? (double)px[ja + q] - pva[q] : 0.0;                        \
            rb[q] = row && jb + q < d ? (double)px[jb + q] - pvb[q] : 0.0;                        \
            csum[q] += ra[q];                                                                     \
        }                                                                                         \
    } while (0)
#define FID_MOM_PUT(buf)                                                                          \
    do {                                                                                          \
        _Pragma("unroll") for (int q = 0; q < 4; ++q) {                                           \
            sa[buf][lk * FID_P + lc + q] = ra[q];                                                 \
            sb[buf][lk * FID_P + lc + q] = rb[q];                                                 \
        }                                                                                         \
    } while (0)

    FID_MOM_FETCH(0);
    FID_MOM_PUT(0);
    __syncthreads();
    for (int c = 0; c < nchunk; ++c) {
        const int cur = c & 1;
        if (c + 1 < nchunk) FID_MOM_FETCH((c + 1) * FID_BK);
        fid_chunk_mma(sa[cur], sb[cur], acc, wr, wc, lane);
        if (c + 1 < nchunk) FID_MOM_PUT(cur ^ 1);
        __syncthreads();
    }
#undef FID_MOM_FETCH
#undef FID_MOM_PUT

#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = bj * FID_T + wc * 32 + j * 16 + (lane & 15);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = bi * FID_T + wr * 32 + i * 16 + (lane >> 4) + 4 * r;
                if (row < d && col < d) outer[(size_t)row * ldo + col] += acc[i][j][r];
            }
        }
    if (bi == bj) {                                               // (block-uniform; every read of sa is behind the loop's last barrier)
#pragma unroll
        for (int q = 0; q < 4; ++q) sa[0][lk * FID_P + lc + q] = csum[q];
        __syncthreads();
        if (tid < FID_T && bi * FID_T + tid < d) {
            double s = 0.0;
            for (int k = 0; k < FID_BK; ++k) s += sa[0][k * FID_P + tid];
            sum[bi * FID_T + tid] += s;
        }
    }
}

extern "C" int cdf_moments_f64(const float* x, int ldx, int n, int d, const double* pivot, double* sum, double* outer, int ldo,
                               void* stream) {
    CDF_REQUIRE(x && pivot && sum && outer, "cdf_moments_f64: null pointer");
    CDF_REQUIRE(n >= 1 && d >= 1, "cdf_moments_f64: n and d must be at least 1 (got n = %d, d = %d)", n, d);
    CDF_REQUIRE(ldx >= d, "cdf_moments_f64: ldx (%d) is smaller than d (%d)", ldx, d);
    CDF_REQUIRE(ldo >= d, "cdf_moments_f64: ldo (%d) is smaller than d (%d)", ldo, d);
    const int t = cdf_cdiv(d, FID_T);
    CDF_REQUIRE(t <= 65535, "cdf_moments_f64: d = %d is more than 65535 tiles of 64", d);
    CDF_LAUNCH(moments_f64_kernel, dim3(t, t), dim3(256), 0, CDF_S, x, ldx, n, d, pivot, sum, outer, ldo);
    return cdf_check_launch("moments_f64");
}

static bool fid_overlap(const double* p, long long rows, int ld, int cols, const double* q, long long qrows, int qld, int qcols) {
    const uintptr_t p0 = (uintptr_t)p, p1 = p0 + ((size_t)(rows - 1) * ld + cols) * sizeof(double);
    const uintptr_t q0 = (uintptr_t)q, q1 = q0 + ((size_t)(qrows - 1) * qld + qcols) * sizeof(double);
    return p0 < q1 && q0 < p1;
}

extern "C" int cdf_gemm_f64(const double* a, int lda, const double* b, int ldb, double* c, int ldc, int m, int n, int k, double alpha,
                            double diag, void* stream) {
    CDF_REQUIRE(a && b && c, "cdf_gemm_f64: null pointer");
    CDF_REQUIRE(m >= 1 && n >= 1 && k >= 1, "cdf_gemm_f64: m, n and k must be at least 1 (got %d, %d, %d)", m, n, k);
    CDF_REQUIRE(lda >= k && ldb >= n && ldc >= n, "cdf_gemm_f64: row pitch smaller than the row (lda %d / k %d, ldb %d / n %d, ldc %d / n %d)",
                lda, k, ldb, n, ldc, n);
    CDF_REQUIRE(!fid_overlap(c, m, ldc, n, a, m, lda, k) && !fid_overlap(c, m, ldc, n, b, k, ldb, n),
                "cdf_gemm_f64: c must not alias a or b");
    const int tx = cdf_cdiv(n, FID_T), ty = cdf_cdiv(m, FID_T);
    CDF_REQUIRE(ty <= 65535, "cdf_gemm_f64: m = %d is more than 65535 tiles of 64", m);
    CDF_LAUNCH(gemm_f64_kernel, dim3(tx, ty), dim3(256), 0, CDF_S, a, lda, b, ldb, c, ldc, m, n, k, alpha, diag);
    return cdf_check_launch("gemm_f64");
}

// ---- merge of two accumulators ---------------------------------------------------------------------------------------------------
// The step that turns the FID statistics of several ranks into one: accumulator b (cdf_moments_f64's n, pivot, sum, outer) added to
// accumulator a, re-centred on a's pivot.  With delta = pivot_b - pivot_a and s = sum_b, every row x of b satisfies
// x - pivot_a = (x - pivot_b) + delta, so over b's n_b rows
//   sum_i (x - pivot_a)_i                = s_i + n_b delta_i
//   sum   (x - pivot_a)_i (x - pivot_a)_j = outer_b[i][j] + delta_i s_j + s_i delta_j + n_b delta_i delta_j
// and both are added to a's.  Plain fp64, one thread per element, no atomics: the result does not depend on the launch.
//
// Ownership is moments_f64_kernel's: grid (T, T), T = ceil(d / 64), block (x = bj, y = bi) owns the 64 x 64 tile (bi, bj) of the upper
// block triangle and leaves at once when bi > bj; a diagonal tile is updated whole and its block also owns sum[64 bi ... + 63].
// A thread keeps one column of the tile (its delta_j and s_j in registers) and walks 16 rows, so a wave instruction reads or writes 64
// consecutive doubles of one row: 512 B.  HBM-bound: both triangles are read and a's is written, 3 x d (d + 64) / 2 x 8 B = 52 MB at d = 2048.
__global__ void __launch_bounds__(256) moments_merge_f64_kernel(double nb, const double* pivot_b, const double* sum_b, const double* outer_b,
                                                               int ldo_b, const double* pivot_a, double* sum_a, double* outer_a, int ldo_a,
                                                               int d) {
    const int bi = blockIdx.y, bj = blockIdx.x;
    if (bi > bj) return;
    const int tid = threadIdx.x;
    const int col = bj * FID_T + (tid & 63), r0 = bi * FID_T + (tid >> 6);
    if (col < d) {
        const double dj = pivot_b[col] - pivot_a[col], sj = sum_b[col];
        // every load of the 16 rows is issued before the first store (32 tile reads in flight per thread); a row past d -- the last tile
        // row only -- reads row d - 1 of the same tile instead and is not stored
        double vb[16], va[16], di[16], si[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = r0 + 4 * r < d ? r0 + 4 * r : d - 1;
            vb[r] = outer_b[(size_t)row * ldo_b + col];
            va[r] = outer_a[(size_t)row * ldo_a + col];
            di[r] = pivot_b[row] - pivot_a[row];
            si[r] = sum_b[row];
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = r0 + 4 * r;
            // (di sj + si dj) and nb (di dj) are symmetric in (i, j) bit for bit: a diagonal tile stays symmetric
            if (row < d) outer_a[(size_t)row * ldo_a + col] = va[r] + (vb[r] + ((di[r] * sj + si[r] * dj) + nb * (di[r] * dj)));
        }
    }
    if (bi == bj && tid < FID_T && col < d)                     // (tid < 64: col = 64 bi + tid, the diagonal block's own 64 entries of sum)
        sum_a[col] += sum_b[col] + nb * (pivot_b[col] - pivot_a[col]);
}

extern "C" int cdf_moments_merge_f64(double n_b, const double* pivot_b, const double* sum_b, const double* outer_b, int ldo_b,
                                     const double* pivot_a, double* sum_a, double* outer_a, int ldo_a, int d, void* stream) {
    CDF_REQUIRE(pivot_b && sum_b && outer_b && pivot_a && sum_a && outer_a, "cdf_moments_merge_f64: null pointer");
    CDF_REQUIRE(d > 0, "cdf_moments_merge_f64: d must be at least 1 (got %d)", d);
    CDF_REQUIRE(ldo_a >= d, "cdf_moments_merge_f64: ldo_a (%d) is smaller than d (%d)", ldo_a, d);
    CDF_REQUIRE(ldo_b >= d, "cdf_moments_merge_f64: ldo_b (%d) is smaller than d (%d)", ldo_b, d);
    CDF_REQUIRE(n_b >= 1.0, "cdf_moments_merge_f64: n_b must be at least 1 (got %g)", n_b);
    CDF_REQUIRE(outer_a != outer_b && sum_a != sum_b, "cdf_moments_merge_f64: accumulator b must not be the accumulator being updated");
    const int t = cdf_cdiv(d, FID_T);
    CDF_REQUIRE(t <= 65535, "cdf_moments_merge_f64: d = %d is more than 65535 tiles of 64", d);
    CDF_LAUNCH(moments_merge_f64_kernel, dim3(t, t), dim3(256), 0, CDF_S, n_b, pivot_b, sum_b, outer_b, ldo_b, pivot_a, sum_a, outer_a,
               ldo_a, d);
    return cdf_check_launch("moments_merge_f64");
}
