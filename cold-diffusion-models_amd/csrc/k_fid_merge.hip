// k_fid_merge.hip — the step that turns the FID statistics of several ranks into one: accumulator b (cdf_moments_f64's n, pivot, sum, outer)
// added to accumulator a, re-centred on a's pivot.  With delta = pivot_b - pivot_a and s = sum_b, every row x of b satisfies
// x - pivot_a = (x - pivot_b) + delta, so over b's n_b rows
//   sum_i (x - pivot_a)_i                = s_i + n_b delta_i
//   sum   (x - pivot_a)_i (x - pivot_a)_j = outer_b[i][j] + delta_i s_j + s_i delta_j + n_b delta_i delta_j
// and both are added to a's.  Plain fp64, one thread per element, no atomics: the result does not depend on the launch.
//
// Ownership is moments_f64_kernel's (k_fid.hip): grid (T, T), T = ceil(d / 64), block (x = bj, y = bi) owns the 64 x 64 tile (bi, bj) of
// the upper block triangle and leaves at once when bi > bj; a diagonal tile is updated whole and its block also owns sum[64 bi ... + 63].
// A thread keeps one column of the tile (its delta_j and s_j in registers) and walks 16 rows, so a wave instruction reads or writes 64
// consecutive doubles of one row: 512 B.  HBM-bound: both triangles are read and a's is written, 3 x d (d + 64) / 2 x 8 B = 52 MB at d = 2048.
//
// The kernel has a file of its own because tests/test_fid_kernels.py pins k_fid.hip to its two matrix-core kernels.
#include "cdf_common.h"
#include "colddiff.h"

#define FIDM_T 64     // tile edge, as FID_T of k_fid.hip

__global__ void __launch_bounds__(256) moments_merge_f64_kernel(double nb, const double* pivot_b, const double* sum_b, const double* outer_b,
                                                               int ldo_b, const double* pivot_a, double* sum_a, double* outer_a, int ldo_a,
                                                               int d) {
    const int bi = blockIdx.y, bj = blockIdx.x;
    if (bi > bj) return;
    const int tid = threadIdx.x;
    const int col = bj * FIDM_T + (tid & 63), r0 = bi * FIDM_T + (tid >> 6);
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
    if (bi == bj && tid < FIDM_T && col < d)                     // (tid < 64: col = 64 bi + tid, the diagonal block's own 64 entries of sum)
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
    const int t = cdf_cdiv(d, FIDM_T);
    CDF_REQUIRE(t <= 65535, "cdf_moments_merge_f64: d = %d is more than 65535 tiles of 64", d);
    CDF_LAUNCH(moments_merge_f64_kernel, dim3(t, t), dim3(256), 0, CDF_S, n_b, pivot_b, sum_b, outer_b, ldo_b, pivot_a, sum_a, outer_a,
               ldo_a, d);
    return cdf_check_launch("moments_merge_f64");
}
