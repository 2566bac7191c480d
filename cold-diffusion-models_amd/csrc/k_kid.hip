// k_kid.hip — Kernel Inception Distance on the device: the unbiased MMD^2 with the polynomial kernel k(a, b) = (gamma a.b + coef0)^3 between
// random subsets of two feature sets (torch-fidelity / clean-fid `kid`), all subsets in one launch pair.
//
// Per subset s the three Gram matrices Xs Xs^T, Ys Ys^T, Xs Ys^T (Xs = rows ix[s][0..m) of x, Ys = rows iy[s][0..m) of y) are walked in
// 64 x 64 tiles on v_mfma_f64_16x16x4_f64, the tile form of cdf_f64_tile.h: its X Y^T loader with the operand rows fetched through the index
// arrays, its accumulator walk for the epilogue; the block sum is cdf_common.h's.  A Gram matrix never goes to memory: the epilogue cubes
// the 16 accumulators of each lane, masks and sums them.
//   * rows / columns at or past m are masked IN THE EPILOGUE: a padded row has Gram value 0, hence kernel value coef0^3, not 0;
//   * XX and YY leave out position i == j (positions, not row numbers: a source row named twice counts off the diagonal);
//   * XX and YY are symmetric: only tiles with bj >= bi are computed, an off-diagonal tile counts twice (an exact doubling); the blocks
//     of the other tiles write a zero partial and leave, so every partial of a call is written by that call.
// Reduction: lane (its 16 values in register order) -> the 256 lanes of the block through LDS (one fixed tree) -> partial[s][pair][tile];
// kid_fold_kernel sums a subset's partials (thread t: tiles t, t + 256, ... in order, then the same tree).  No atomics: two runs are
// bit-identical.  Work: 3 m^2 d MACs per subset less the skipped halves, 2 m^2 d; every operand row is read by T tiles (through L2).
#include "cdf_common.h"
#include "cdf_f64_tile.h"
#include "colddiff.h"

#define KID_MAX_T 46340     // T^2 tiles is grid.x: T^2 <= 2^31 - 1

// grid (T T, 3, nsub), T = ceil(m / 64): block x = tile bi T + bj, y = pair (0: XX, 1: YY, 2: XY), z = subset.
__global__ void __launch_bounds__(256) kid_poly3_kernel(const double* X, int ldx, const int* IX, const double* Y, int ldy, const int* IY, int m,
                                                       int d, int T, double gamma, double coef0, double* partial) {
    const int tile = blockIdx.x, pair = blockIdx.y, sub = blockIdx.z;
    const int bi = tile / T, bj = tile - bi * T;
    const bool sym = pair < 2;
    double* dst = partial + ((size_t)sub * 3 + pair) * gridDim.x + tile;
    if (sym && bj < bi) {                                       // (block-uniform) the mirror of a tile that is counted twice
        if (threadIdx.x == 0) *dst = 0.0;
        return;
    }
    __shared__ double s[4 * FID_BK * FID_P];
    const double* A = pair == 1 ? Y : X;
    const double* B = pair == 0 ? X : Y;
    const int lda = pair == 1 ? ldy : ldx, ldb = pair == 0 ? ldx : ldy;
    const int* ia = (pair == 1 ? IY : IX) + (size_t)sub * m;
    const int* ib = (pair == 0 ? IX : IY) + (size_t)sub * m;
    f64x4_t acc[2][2];
    fid_acc_zero(acc);
    fid_tile_abt_indexed(s, A, lda, ia, bi * FID_T, m, B, ldb, ib, bj * FID_T, m, d, acc);
    double v = 0.0;
    fid_tile_each(acc, [&](int r, int c, double g) {           // (the walk's order is the lane's order of summation)
        const int row = bi * FID_T + r, col = bj * FID_T + c;
        const double z = gamma * g + coef0;
        const double k3 = z * z * z;
        v += row < m && col < m && !(sym && row == col) ? k3 : 0.0;
    });
    v = cdf_block_sum_f64(s, v);                                // (every wave is past its reads of s: fid_k_loop's last barrier)
    if (threadIdx.x == 0) *dst = sym && bi < bj ? 2.0 * v : v;
}

// grid (nsub): out[s] = {sxx, syy, sxy, mmd2}
__global__ void __launch_bounds__(256) kid_fold_kernel(const double* partial, long long tiles, int m, double* out) {
    __shared__ double red[256];
    const int sub = blockIdx.x;
    double sum[3];
    for (int p = 0; p < 3; ++p) {
        const double* src = partial + ((size_t)sub * 3 + p) * tiles;
        double v = 0.0;
        for (long long t = threadIdx.x; t < tiles; t += 256) v += src[t];
        sum[p] = cdf_block_sum_f64(red, v);
    }
    if (threadIdx.x == 0) {
        const double mm = (double)m;
        double* o = out + (size_t)sub * 4;
        o[0] = sum[0];
        o[1] = sum[1];
        o[2] = sum[2];
        o[3] = (sum[0] + sum[1]) / (mm * (mm - 1.0)) - 2.0 * sum[2] / (mm * mm);
    }
}

extern "C" int cdf_kid_tiles(int m) {
    const int t = m < 2 ? 0 : cdf_cdiv(m, FID_T);
    return t > KID_MAX_T ? 0 : t * t;
}

extern "C" int cdf_kid_poly3_f64(const double* x, int ldx, const int* ix, const double* y, int ldy, const int* iy, int nsub, int m, int d,
                                 double gamma, double coef0, double* partial, double* out, void* stream) {
    CDF_REQUIRE(x && ix && y && iy && partial && out, "cdf_kid_poly3_f64: null pointer");
    CDF_REQUIRE(m >= 2, "cdf_kid_poly3_f64: m must be at least 2 (got %d): the unbiased estimator divides by m (m - 1)", m);
    CDF_REQUIRE(nsub >= 1 && d >= 1, "cdf_kid_poly3_f64: nsub and d must be at least 1 (got nsub = %d, d = %d)", nsub, d);
    CDF_REQUIRE(ldx >= d, "cdf_kid_poly3_f64: ldx (%d) is smaller than d (%d)", ldx, d);
    CDF_REQUIRE(ldy >= d, "cdf_kid_poly3_f64: ldy (%d) is smaller than d (%d)", ldy, d);
    CDF_REQUIRE(nsub <= 65535, "cdf_kid_poly3_f64: nsub = %d is more than 65535 subsets", nsub);
    const int T = cdf_cdiv(m, FID_T);
    CDF_REQUIRE(T <= KID_MAX_T, "cdf_kid_poly3_f64: m = %d is more than %d tiles of 64 on a side", m, KID_MAX_T);
    CDF_LAUNCH(kid_poly3_kernel, dim3(T * T, 3, nsub), dim3(256), 0, CDF_S, x, ldx, ix, y, ldy, iy, m, d, T, gamma, coef0, partial);
    CDF_LAUNCH(kid_fold_kernel, dim3(nsub), dim3(256), 0, CDF_S, (const double*)partial, (long long)T * T, m, out);
    return cdf_check_launch("kid_poly3_f64");
}
