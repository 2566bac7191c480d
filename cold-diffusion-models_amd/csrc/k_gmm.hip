// k_gmm.hip — the Gaussian mixture of the generation scripts on the device (colddiff/gmm.py): what an EM iteration needs besides the big
// products, which go through cdf_gemm_f64.  Everything is fp64, row-major with explicit row pitches, batched over components by a count
// and an element stride.  No float atomics; every reduction is a fixed-order tree, so two runs are bit-identical.
//
//   cdf_potrf_f64        blocked right-looking lower Cholesky, 64-wide panels.  Per panel three launches: the 64 x 64 diagonal block is
//                        factored by one workgroup in LDS; the rows below it are solved against it (64 rows per workgroup, block and rows
//                        in LDS); the trailing update A22 -= L21 L21^T runs on the fp64 MFMA tile form of cdf_f64_tile.h, lower block
//                        triangle only.  d^3 / 3 flops, 3 ceil(d / 64) launches.  A non-positive (or NaN) pivot writes info and every later
//                        kernel of that component returns at once.
//   cdf_trtri_lower_f64  P = L^-1, written as P^T.  All diagonal blocks are inverted in LDS in one launch; then block row i, i = 1 ..., one
//                        launch: tile (i, j) = -P_ii (sum_{j <= p < i} L_ip P_pj), the sum and the product both on the MFMA tile form, the
//                        sum handed over through LDS.  d^3 / 3 flops, ceil(d / 64) launches.
//   the small ones       centre-and-scale (with the transposed copy the covariance GEMM needs), row sums of squares, the responsibilities
//                        with their two-stage reductions, log det from the diagonal, a triangle copy / transpose.
// Shared with the other fp64 files: the X Y^T loader and the accumulator walk of cdf_f64_tile.h (trailing update, triangular inverse; the
// inverse's second product has an MFMA loop of its own) and cdf_common.h's fixed-tree block sum (log det, responsibilities).
#include <float.h>
#include <math.h>

#include "cdf_common.h"
#include "cdf_f64_tile.h"
#include "colddiff.h"

#define GMM_NB 64                 // panel width = tile edge
#define GMM_DP 65                 // LDS row pitch of the 64 x 64 diagonal block (odd: a column walk touches every bank pair once)

__device__ __forceinline__ int gmm_min(int a, int b) { return a < b ? a : b; }

// ---- Cholesky -------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) potrf_info_zero_kernel(int* info, int count) {
    for (int k = threadIdx.x; k < count; k += 64) info[k] = 0;
}

// grid (count): the diagonal block at j0, nb = min(64, d - j0) rows.  Lower triangle only.
__global__ void __launch_bounds__(256) potrf_diag_kernel(double* A, int lda, long long stride, int d, int j0, int* info) {
    const int k = blockIdx.x, tid = threadIdx.x;
    if (info[k] != 0) return;
    __shared__ double s[GMM_NB * GMM_DP];
    double* a = A + (size_t)k * stride + (size_t)j0 * lda + j0;
    const int nb = gmm_min(GMM_NB, d - j0);
    const int c = tid & 63, rq = tid >> 6;
    for (int r = rq; r < nb; r += 4)
        if (c <= r) s[r * GMM_DP + c] = a[(size_t)r * lda + c];
    __syncthreads();
    for (int j = 0; j < nb; ++j) {
        const double p = s[j * GMM_DP + j];
        if (!(p > 0.0)) {                                       // (block-uniform: every thread reads the same word)
            if (tid == 0) info[k] = j0 + j + 1;
            return;
        }
        const double lj = sqrt(p);
        __syncthreads();                                        // everyone has read the pivot before it is replaced
        if (tid == 0) s[j * GMM_DP + j] = lj;
        if (tid > j && tid < nb) s[tid * GMM_DP + j] /= lj;
        __syncthreads();
        if (c > j && c < nb) {
            const double lc = s[c * GMM_DP + j];
            for (int r = c + ((rq - c) & 3); r < nb; r += 4) s[r * GMM_DP + c] -= s[r * GMM_DP + j] * lc;   // r = rq (mod 4), r >= c
        }
        __syncthreads();
    }
    for (int r = rq; r < nb; r += 4)
        if (c <= r) a[(size_t)r * lda + c] = s[r * GMM_DP + c];
}

// grid (ceil((d - j0 - 64) / 64), count): 64 rows of the panel below the diagonal block, X L11^T = A21 by forward substitution.
// lt[j][c] = L11[c][j] (a step reads one row of it), xs[r][c] the rows; both pitch 64: a step's accesses are a broadcast and a row.
__global__ void __launch_bounds__(256) potrf_panel_kernel(double* A, int lda, long long stride, int d, int j0, const int* info) {
    const int k = blockIdx.y, tid = threadIdx.x;
    if (info[k] != 0) return;
    __shared__ double lt[GMM_NB * GMM_NB], xs[GMM_NB * GMM_NB];
    double* base = A + (size_t)k * stride;
    const double* l11 = base + (size_t)j0 * lda + j0;
    const int r0 = j0 + GMM_NB + blockIdx.x * GMM_NB, nr = gmm_min(GMM_NB, d - r0);
    double* a21 = base + (size_t)r0 * lda + j0;
    const int c = tid & 63, rq = tid >> 6;
    for (int r = rq; r < GMM_NB; r += 4) {
        if (c <= r) lt[c * GMM_NB + r] = l11[(size_t)r * lda + c];
        xs[r * GMM_NB + c] = r < nr ? a21[(size_t)r * lda + c] : 0.0;
    }
    __syncthreads();
    for (int j = 0; j < GMM_NB; ++j) {
        if (c == j) {
            const double ljj = lt[j * GMM_NB + j];
            for (int r = rq; r < GMM_NB; r += 4) xs[r * GMM_NB + j] /= ljj;
        }
        __syncthreads();
        if (c > j) {
            const double lcj = lt[j * GMM_NB + c];
            for (int r = rq; r < GMM_NB; r += 4) xs[r * GMM_NB + c] -= xs[r * GMM_NB + j] * lcj;
        }
        __syncthreads();
    }
    for (int r = rq; r < nr; r += 4) a21[(size_t)r * lda + c] = xs[r * GMM_NB + c];
}

// grid (T, T, count), T = ceil((d - j0 - 64) / 64): tile (bi, bj), bi >= bj, of A22 -= L21 L21^T; a diagonal tile stores its lower half.
__global__ void __launch_bounds__(256) potrf_syrk_kernel(double* A, int lda, long long stride, int d, int j0, const int* info) {
    const int bi = blockIdx.y, bj = blockIdx.x, k = blockIdx.z;
    if (bj > bi || info[k] != 0) return;
    __shared__ double s[4 * FID_BK * FID_P];
    double* base = A + (size_t)k * stride;
    const int t0 = j0 + GMM_NB;
    const double* l21 = base + j0;                              // column j0 of every row
    f64x4_t acc[2][2];
    fid_acc_zero(acc);
    fid_tile_abt(s, l21, lda, t0 + bi * FID_T, d, l21, lda, t0 + bj * FID_T, d, 0, GMM_NB, acc);
    fid_tile_each(acc, [&](int r, int c, double v) {
        const int row = t0 + bi * FID_T + r, col = t0 + bj * FID_T + c;
        if (row < d && col <= row) base[(size_t)row * lda + col] -= v;
    });
}

extern "C" int cdf_potrf_f64(double* a, int lda, long long stride, int d, int count, int* info, void* stream) {
    CDF_REQUIRE(a && info, "cdf_potrf_f64: null pointer");
    CDF_REQUIRE(d >= 1 && count >= 1, "cdf_potrf_f64: d and count must be at least 1 (got d = %d, count = %d)", d, count);
    CDF_REQUIRE(lda >= d, "cdf_potrf_f64: lda (%d) is smaller than d (%d)", lda, d);
    CDF_REQUIRE(count == 1 || stride >= (long long)(d - 1) * lda + d, "cdf_potrf_f64: stride (%lld) is smaller than one matrix", stride);
    CDF_REQUIRE(count <= 65535, "cdf_potrf_f64: count = %d is more than 65535", count);
    CDF_REQUIRE(cdf_cdiv(d, GMM_NB) <= 65535, "cdf_potrf_f64: d = %d is more than 65535 panels of 64", d);
    CDF_LAUNCH(potrf_info_zero_kernel, dim3(1), dim3(64), 0, CDF_S, info, count);
    for (int j0 = 0; j0 < d; j0 += GMM_NB) {
        CDF_LAUNCH(potrf_diag_kernel, dim3(count), dim3(256), 0, CDF_S, a, lda, stride, d, j0, info);
        const int rest = d - j0 - GMM_NB;
        if (rest <= 0) break;
        const int t = cdf_cdiv(rest, GMM_NB);
        CDF_LAUNCH(potrf_panel_kernel, dim3(t, count), dim3(256), 0, CDF_S, a, lda, stride, d, j0, (const int*)info);
        CDF_LAUNCH(potrf_syrk_kernel, dim3(t, t, count), dim3(256), 0, CDF_S, a, lda, stride, d, j0, (const int*)info);
    }
    return cdf_check_launch("potrf_f64");
}

// ---- triangular inverse ------------------------------------------------------------------------------------------------------------
// grid (T, count), 64 threads: thread c solves column c of the inverse of diagonal block bi by forward substitution (ls[r][p] is a
// broadcast read, xs[p][c] a row).  The whole tile of P^T is written: element (c, r) = X[r][c] for r >= c, zeros below the diagonal --
// the off-diagonal kernel reads the tile as a full operand.
__global__ void __launch_bounds__(64) trtri_diag_kernel(const double* L, int ldl, long long stride_l, double* PT, int ldp, long long stride_p,
                                                       int d) {
    __shared__ double ls[GMM_NB * GMM_NB], xs[GMM_NB * GMM_NB];
    const int i0 = blockIdx.x * GMM_NB, k = blockIdx.y, c = threadIdx.x;
    const int nb = gmm_min(GMM_NB, d - i0);
    const double* l = L + (size_t)k * stride_l + (size_t)i0 * ldl + i0;
    double* pt = PT + (size_t)k * stride_p + (size_t)i0 * ldp + i0;
    for (int r = 0; r < nb; ++r)
        if (c <= r) ls[r * GMM_NB + c] = l[(size_t)r * ldl + c];
    __syncthreads();
    if (c < nb) {
        for (int r = 0; r < c; ++r) xs[r * GMM_NB + c] = 0.0;
        for (int r = c; r < nb; ++r) {
            double v = r == c ? 1.0 : 0.0;
            for (int p = c; p < r; ++p) v -= ls[r * GMM_NB + p] * xs[p * GMM_NB + c];
            xs[r * GMM_NB + c] = v / ls[r * GMM_NB + r];
        }
    }
    __syncthreads();
    if (c < nb)                                                 // thread c writes column c of the tile of P^T (= row c of X^T), coalesced per row
        for (int r = 0; r < nb; ++r) pt[(size_t)r * ldp + c] = xs[c * GMM_NB + r];
}

// grid (bi, count) for block row bi >= 1: tile (bi, bj) of P.  W = sum_{bj <= p < bi} L[bi][p] P[p][bj] = L-rows times (P^T-rows)^T over
// k in [64 bj, 64 bi); then P[bi][bj] = -P[bi][bi] W with W as the [k][column] operand in LDS and P[bi][bi] read from its tile of P^T
// (row k of that tile is column k of P[bi][bi]: 16 consecutive doubles per fragment).  Writes the tile transposed into the upper
// triangle and zeros into its mirror below.
__global__ void __launch_bounds__(256) trtri_offdiag_kernel(const double* L, int ldl, long long stride_l, double* PT, int ldp,
                                                           long long stride_p, int d, int bi) {
    __shared__ double s[4 * FID_BK * FID_P];                    // = FID_T * FID_P: phase 2 keeps W here as [64][FID_P]
    const int bj = blockIdx.x, k = blockIdx.y;
    const int i0 = bi * FID_T, j0 = bj * FID_T;
    const double* l = L + (size_t)k * stride_l;
    double* pt = PT + (size_t)k * stride_p;
    f64x4_t acc[2][2];
    fid_acc_zero(acc);
    fid_tile_abt(s, l, ldl, i0, d, pt, ldp, j0, d, j0, i0, acc);
    fid_tile_each(acc, [&](int r, int c, double v) { s[r * FID_P + c] = v; });
    __syncthreads();
    fid_acc_zero(acc);
    const double* pii = pt + (size_t)i0 * ldp + i0;
    const int nb = gmm_min(FID_T, d - i0);
    // the second product keeps a loop of its own: P[bi][bi] comes from global memory, not through the shared loader's LDS buffers
    const int wr = fid_wave_row(), wc = fid_wave_col(), c16 = threadIdx.x & 15, kq = (threadIdx.x & 63) >> 4;
    for (int ks = 0; ks < nb; ks += 4) {                        // (rows of W at or past nb are zero: L's rows past d were loaded as zeros)
        double a[2], b[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int row = wr * 32 + i * 16 + c16;
            a[i] = ks + kq < nb && row < nb ? pii[(size_t)(ks + kq) * ldp + row] : 0.0;
            b[i] = s[(ks + kq) * FID_P + wc * 32 + i * 16 + c16];
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = cdf_mfma_f64_16x16x4(a[i], b[j], acc[i][j]);
    }
    fid_tile_each(acc, [&](int r, int c, double v) {
        const int row = i0 + r, col = j0 + c;                   // (col < i0 <= d)
        if (row < d) {
            pt[(size_t)col * ldp + row] = -v;
            pt[(size_t)row * ldp + col] = 0.0;
        }
    });
}

extern "C" int cdf_trtri_lower_f64(const double* l, int ldl, long long stride_l, double* pt, int ldp, long long stride_p, int d, int count,
                                   void* stream) {
    CDF_REQUIRE(l && pt, "cdf_trtri_lower_f64: null pointer");
    CDF_REQUIRE(d >= 1 && count >= 1, "cdf_trtri_lower_f64: d and count must be at least 1 (got d = %d, count = %d)", d, count);
    CDF_REQUIRE(ldl >= d && ldp >= d, "cdf_trtri_lower_f64: row pitch smaller than d (ldl %d, ldp %d, d %d)", ldl, ldp, d);
    CDF_REQUIRE(count == 1 || (stride_l >= (long long)(d - 1) * ldl + d && stride_p >= (long long)(d - 1) * ldp + d),
                "cdf_trtri_lower_f64: stride smaller than one matrix (%lld, %lld)", stride_l, stride_p);
    CDF_REQUIRE(count <= 65535, "cdf_trtri_lower_f64: count = %d is more than 65535", count);
    {
        const uintptr_t a0 = (uintptr_t)l, a1 = a0 + ((size_t)(count - 1) * stride_l + (size_t)(d - 1) * ldl + d) * sizeof(double);
        const uintptr_t b0 = (uintptr_t)pt, b1 = b0 + ((size_t)(count - 1) * stride_p + (size_t)(d - 1) * ldp + d) * sizeof(double);
        CDF_REQUIRE(!(a0 < b1 && b0 < a1), "cdf_trtri_lower_f64: pt must not alias l");
    }
    const int t = cdf_cdiv(d, GMM_NB);
    CDF_LAUNCH(trtri_diag_kernel, dim3(t, count), dim3(64), 0, CDF_S, l, ldl, stride_l, pt, ldp, stride_p, d);
    for (int bi = 1; bi < t; ++bi)
        CDF_LAUNCH(trtri_offdiag_kernel, dim3(bi, count), dim3(256), 0, CDF_S, l, ldl, stride_l, pt, ldp, stride_p, d, bi);
    return cdf_check_launch("trtri_lower_f64");
}

// ---- triangle copy / transpose, log det -----------------------------------------------------------------------------------------------
// out = tril(a) (transpose == 0) or tril(a)^T, the other triangle zero.  Only the lower triangle of a is read.
__global__ void __launch_bounds__(256) tril_copy_kernel(const double* A, int lda, long long stride_a, double* O, int ldo, long long stride_o,
                                                       int d, int transpose) {
    const double* a = A + (size_t)blockIdx.y * stride_a;
    double* o = O + (size_t)blockIdx.y * stride_o;
    const long long total = (long long)d * d;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const int r = (int)(e / d), c = (int)(e % d);
        const int lo = transpose ? c : r, hi = transpose ? r : c;                   // the element of a is (lo, hi) when it is in the triangle
        o[(size_t)r * ldo + c] = hi <= lo ? a[(size_t)lo * lda + hi] : 0.0;
    }
}

extern "C" int cdf_tril_copy_f64(const double* a, int lda, long long stride_a, double* out, int ldo, long long stride_o, int d, int count,
                                 int transpose, void* stream) {
    CDF_REQUIRE(a && out, "cdf_tril_copy_f64: null pointer");
    CDF_REQUIRE(d >= 1 && count >= 1, "cdf_tril_copy_f64: d and count must be at least 1 (got d = %d, count = %d)", d, count);
    CDF_REQUIRE(lda >= d && ldo >= d, "cdf_tril_copy_f64: row pitch smaller than d (lda %d, ldo %d, d %d)", lda, ldo, d);
    CDF_REQUIRE(count <= 65535, "cdf_tril_copy_f64: count = %d is more than 65535", count);
    CDF_REQUIRE(a != out, "cdf_tril_copy_f64: out must not alias a");
    CDF_LAUNCH(tril_copy_kernel, dim3(cdf_ew_grid4k((long long)d * d), count), dim3(256), 0, CDF_S, a, lda, stride_a, out, ldo, stride_o, d,
               transpose);
    return cdf_check_launch("tril_copy_f64");
}

// out[k] = sum_j log m_k[j][j]: thread t sums j = t, t + 256, ... in order, then the tree
__global__ void __launch_bounds__(256) logdet_diag_kernel(const double* M, int ld, long long stride, int d, double* out) {
    __shared__ double red[256];
    const double* m = M + (size_t)blockIdx.x * stride;
    double v = 0.0;
    for (int j = threadIdx.x; j < d; j += 256) v += log(m[(size_t)j * ld + j]);
    v = cdf_block_sum_f64(red, v);
    if (threadIdx.x == 0) out[blockIdx.x] = v;
}

extern "C" int cdf_logdet_diag_f64(const double* m, int ld, long long stride, int d, int count, double* out, void* stream) {
    CDF_REQUIRE(m && out, "cdf_logdet_diag_f64: null pointer");
    CDF_REQUIRE(d >= 1 && count >= 1, "cdf_logdet_diag_f64: d and count must be at least 1 (got d = %d, count = %d)", d, count);
    CDF_REQUIRE(ld >= d, "cdf_logdet_diag_f64: ld (%d) is smaller than d (%d)", ld, d);
    CDF_LAUNCH(logdet_diag_kernel, dim3(count), dim3(256), 0, CDF_S, m, ld, stride, d, out);
    return cdf_check_launch("logdet_diag_f64");
}

// ---- z = s (x - mean), z^T ------------------------------------------------------------------------------------------------------------
// grid (ceil(n / 64), ceil(d / 64)): a 64 x 64 tile; the transposed copy goes through LDS so that both stores run along rows.
template <class T>
__global__ void __launch_bounds__(256) center_scale_kernel(const T* X, int ldx, int n, int d, const double* mean, const double* resp,
                                                          const double* nk, double* Z, int ldz, double* ZT, int ldzt) {
    __shared__ double tile[GMM_NB * GMM_DP];
    const int n0 = blockIdx.x * GMM_NB, j0 = blockIdx.y * GMM_NB;
    const int c = threadIdx.x & 63, rq = threadIdx.x >> 6;
    const int j = j0 + c;
    const double mu = j < d ? mean[j] : 0.0;
    const double den = resp ? nk[0] : 1.0;
    for (int r = rq; r < GMM_NB; r += 4) {
        const int row = n0 + r;
        double v = 0.0;
        if (row < n && j < d) {
            v = (double)X[(size_t)row * ldx + j] - mu;
            if (resp) v *= sqrt(resp[row] / den);
            Z[(size_t)row * ldz + j] = v;
        }
        tile[r * GMM_DP + c] = v;
    }
    if (!ZT) return;
    __syncthreads();
    for (int r = rq; r < GMM_NB; r += 4)                        // r: feature of the tile, c: row of x
        if (j0 + r < d && n0 + c < n) ZT[(size_t)(j0 + r) * ldzt + n0 + c] = tile[c * GMM_DP + r];
}

extern "C" int cdf_gmm_center_scale_f64(const void* x, int x_is_f64, int ldx, int n, int d, const double* mean, const double* resp,
                                        const double* nk, double* z, int ldz, double* zt, int ldzt, void* stream) {
    CDF_REQUIRE(x && mean && z, "cdf_gmm_center_scale_f64: null pointer");
    CDF_REQUIRE((resp == nullptr) == (nk == nullptr), "cdf_gmm_center_scale_f64: resp and nk come together (both or neither)");
    CDF_REQUIRE(n >= 1 && d >= 1, "cdf_gmm_center_scale_f64: n and d must be at least 1 (got n = %d, d = %d)", n, d);
    CDF_REQUIRE(ldx >= d && ldz >= d, "cdf_gmm_center_scale_f64: row pitch smaller than d (ldx %d, ldz %d, d %d)", ldx, ldz, d);
    CDF_REQUIRE(!zt || ldzt >= n, "cdf_gmm_center_scale_f64: ldzt (%d) is smaller than n (%d)", ldzt, n);
    CDF_REQUIRE(x_is_f64 == 0 || x_is_f64 == 1, "cdf_gmm_center_scale_f64: x_is_f64 is 0 or 1 (got %d)", x_is_f64);
    CDF_REQUIRE((const void*)z != x && (const void*)zt != x && z != zt, "cdf_gmm_center_scale_f64: z and zt must not alias x or each other");
    const int ty = cdf_cdiv(d, GMM_NB);
    CDF_REQUIRE(ty <= 65535, "cdf_gmm_center_scale_f64: d = %d is more than 65535 tiles of 64", d);
    const dim3 grid(cdf_cdiv(n, GMM_NB), ty);
    if (x_is_f64)
        CDF_LAUNCH(center_scale_kernel<double>, grid, dim3(256), 0, CDF_S, (const double*)x, ldx, n, d, mean, resp, nk, z, ldz, zt, ldzt);
    else
        CDF_LAUNCH(center_scale_kernel<float>, grid, dim3(256), 0, CDF_S, (const float*)x, ldx, n, d, mean, resp, nk, z, ldz, zt, ldzt);
    return cdf_check_launch("gmm_center_scale_f64");
}

// ---- out[n] = sum_j y[n][j]^2 -----------------------------------------------------------------------------------------------------------
// `lanes` (a power of two <= 256, chosen from d alone) threads per row, 256 / lanes rows per workgroup: a lane sums j = lane, lane + lanes,
// ... in order, then one tree over the row's lanes.  d = 12 288 -> 256 lanes, coalesced; d = 3 -> one lane, 256 rows per workgroup.
__global__ void __launch_bounds__(256) rowsumsq_kernel(const double* Y, int ldy, int n, int d, double* out, int lanes) {
    __shared__ double red[256];
    const int tid = threadIdx.x, lane = tid & (lanes - 1);
    const long long row = (long long)blockIdx.x * (256 / lanes) + tid / lanes;
    double v = 0.0;
    if (row < n) {
        const double* y = Y + (size_t)row * ldy;
        for (int j = lane; j < d; j += lanes) v += y[j] * y[j];
    }
    red[tid] = v;
    for (int o = lanes >> 1; o > 0; o >>= 1) {
        __syncthreads();
        if (lane < o) red[tid] += red[tid + o];
    }
    if (lane == 0 && row < n) out[row] = red[tid];
}

static int gmm_row_lanes(int d) {
    int lanes = 1;
    while (lanes < 256 && lanes * 8 < d) lanes *= 2;
    return lanes;
}

extern "C" int cdf_rowsumsq_f64(const double* y, int ldy, int n, int d, double* out, void* stream) {
    CDF_REQUIRE(y && out, "cdf_rowsumsq_f64: null pointer");
    CDF_REQUIRE(n >= 1 && d >= 1, "cdf_rowsumsq_f64: n and d must be at least 1 (got n = %d, d = %d)", n, d);
    CDF_REQUIRE(ldy >= d, "cdf_rowsumsq_f64: ldy (%d) is smaller than d (%d)", ldy, d);
    const int lanes = gmm_row_lanes(d);
    CDF_LAUNCH(rowsumsq_kernel, dim3(cdf_cdiv(n, 256 / lanes)), dim3(256), 0, CDF_S, y, ldy, n, d, out, lanes);
    return cdf_check_launch("rowsumsq_f64");
}

// ---- responsibilities --------------------------------------------------------------------------------------------------------------
// Stage 1, grid (ceil(n / 256)): one row per thread.  lp_k = -(d log 2 pi + maha_k) / 2 + logdet_k + logw_k is evaluated the same way in
// every pass (bit-identical), so nothing per-k is kept in registers and K is unbounded.  partial[block][0 .. K - 1] = the block's sums of
// resp_k, partial[block][K] = its sum of lse.  Stage 2, grid (K + 1): thread t sums blocks t, t + 256, ... in order, then the tree.
__device__ __forceinline__ double gmm_lp(const double* maha, int ldm, const double* logdet, const double* logw, double dlog2pi, int k,
                                         long long row) {
    return -0.5 * (dlog2pi + maha[(size_t)k * ldm + row]) + (logdet ? logdet[k] : 0.0) + (logw ? logw[k] : 0.0);
}

__global__ void __launch_bounds__(256) gmm_resp_kernel(const double* maha, int ldm, const double* logdet, const double* logw, int n, int d,
                                                      int K, int hard, double* resp, int ldr, double* partial) {
    __shared__ double red[256];
    const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool in = row < n;
    const double dlog2pi = (double)d * 1.8378770664093453;      // log(2 pi)
    double best = -INFINITY, lse = 0.0;
    int arg = 0;
    if (in) {
        for (int k = 0; k < K; ++k) {
            const double lp = gmm_lp(maha, ldm, logdet, logw, dlog2pi, k, row);
            if (lp > best) best = lp, arg = k;                  // (strict: the lowest index wins a tie)
        }
        if (!hard) {
            double s = 0.0;
            for (int k = 0; k < K; ++k) s += exp(gmm_lp(maha, ldm, logdet, logw, dlog2pi, k, row) - best);
            lse = best + log(s);
        }
    }
    for (int k = 0; k < K; ++k) {
        double r = 0.0;
        if (in) {
            r = hard ? (k == arg ? 1.0 : 0.0) : exp(gmm_lp(maha, ldm, logdet, logw, dlog2pi, k, row) - lse);
            resp[(size_t)k * ldr + row] = r;
        }
        const double t = cdf_block_sum_f64(red, r);
        if (threadIdx.x == 0) partial[(size_t)blockIdx.x * (K + 1) + k] = t;
    }
    const double t = cdf_block_sum_f64(red, in ? lse : 0.0);
    if (threadIdx.x == 0) partial[(size_t)blockIdx.x * (K + 1) + K] = t;
}

__global__ void __launch_bounds__(256) gmm_resp_fold_kernel(const double* partial, int nblk, int K, double* nk, double* lse_sum) {
    __shared__ double red[256];
    const int k = blockIdx.x;
    double v = 0.0;
    for (int b = threadIdx.x; b < nblk; b += 256) v += partial[(size_t)b * (K + 1) + k];
    v = cdf_block_sum_f64(red, v);
    if (threadIdx.x == 0) {
        if (k < K) nk[k] = v + 10.0 * DBL_EPSILON;
        else lse_sum[0] = v;
    }
}

extern "C" int cdf_gmm_resp_blocks(int n) { return n < 1 ? 0 : cdf_cdiv(n, 256); }

extern "C" int cdf_gmm_resp_f64(const double* maha, int ldm, const double* logdet, const double* logw, int n, int d, int K, int hard,
                                double* resp, int ldr, double* nk, double* lse_sum, double* partial, void* stream) {
    CDF_REQUIRE(maha && resp && nk && lse_sum && partial, "cdf_gmm_resp_f64: null pointer");
    CDF_REQUIRE(n >= 1 && d >= 1 && K >= 1, "cdf_gmm_resp_f64: n, d and K must be at least 1 (got %d, %d, %d)", n, d, K);
    CDF_REQUIRE(ldm >= n && ldr >= n, "cdf_gmm_resp_f64: row pitch smaller than n (ldm %d, ldr %d, n %d)", ldm, ldr, n);
    CDF_REQUIRE(hard == 0 || hard == 1, "cdf_gmm_resp_f64: hard is 0 or 1 (got %d)", hard);
    CDF_REQUIRE(hard || (logdet && logw), "cdf_gmm_resp_f64: logdet and logw may be null only with hard = 1");
    CDF_REQUIRE(resp != maha, "cdf_gmm_resp_f64: resp must not alias maha");
    const int nblk = cdf_gmm_resp_blocks(n);
    CDF_LAUNCH(gmm_resp_kernel, dim3(nblk), dim3(256), 0, CDF_S, maha, ldm, logdet, logw, n, d, K, hard, resp, ldr, partial);
    CDF_LAUNCH(gmm_resp_fold_kernel, dim3(K + 1), dim3(256), 0, CDF_S, (const double*)partial, nblk, K, nk, lse_sum);
    return cdf_check_launch("gmm_resp_f64");
}
