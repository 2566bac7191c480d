// k_metrics.hip — the metric step after sampling: SSIM of two image batches.
//
// Replaces pytorch_msssim.ssim(X, Y, data_range, size_average=True) as called by the reference's evaluation code
// (deblurring_diffusion_pytorch.py:1677-1702): 11-tap Gaussian window (sigma 1.5), "valid" separable filtering of X, Y, X^2, Y^2,
// XY per channel plane, ssim_map = (2 mu1 mu2 + C1)/(mu1^2 + mu2^2 + C1) * (2 s12 + C2)/(s1 + s2 + C2), mean over the
// (H-10) x (W-10) valid positions of every plane.  pytorch_msssim does this with ten grouped conv2d launches and a dozen
// elementwise kernels, every intermediate (5 filtered maps x 2 passes) round-tripping through HBM; here a workgroup keeps a
// 42 x 42 tile of both images in LDS, filters the five products along H then along W (the library's order) on chip and
// reduces its 32 x 32 SSIM values to one partial sum: the images are read once (8 B / pixel), nothing else is written.
// RMSE is cdf_loss_fwd(l2 = 1) followed by a square root (k_degrade.hip).
#include "cdf_common.h"
#include "colddiff.h"

#define SSIM_WIN 11
#define SSIM_T 32                       // output tile edge
#define SSIM_IN (SSIM_T + SSIM_WIN - 1) // 42

struct SsimWin { float w[SSIM_WIN]; };

// The two filter passes and the SSIM sum of one tile whose inputs are in sx / sy: this thread's share of the tile's SSIM values.
// One copy for both kernels below (same expressions, same order: their results are bit-equal).  Ends after the last read of v.
__device__ __forceinline__ float ssim_tile_body(const float (*sx)[SSIM_IN + 1], const float (*sy)[SSIM_IN + 1],
                                                float (*v)[SSIM_T][SSIM_IN + 1], int y0, int x0, int OH, int OW, float C1, float C2,
                                                const SsimWin& win, int tid) {
    // pass along H (dim 2 first, as pytorch_msssim's gaussian_filter does): out row r, input column c
    for (int i = tid; i < SSIM_T * SSIM_IN; i += 256) {
        const int r = i / SSIM_IN, c = i - r * SSIM_IN;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f;
#pragma unroll
        for (int k = 0; k < SSIM_WIN; ++k) {
            const float xv = sx[r + k][c], yv = sy[r + k][c], w = win.w[k];
            a0 += w * xv;
            a1 += w * yv;
            a2 += w * (xv * xv);
            a3 += w * (yv * yv);
            a4 += w * (xv * yv);
        }
        v[0][r][c] = a0; v[1][r][c] = a1; v[2][r][c] = a2; v[3][r][c] = a3; v[4][r][c] = a4;
    }
    __syncthreads();
    // pass along W, SSIM value, tile sum
    float acc = 0.f;
    for (int i = tid; i < SSIM_T * SSIM_T; i += 256) {
        const int r = i / SSIM_T, c = i - r * SSIM_T;
        if (y0 + r < OH && x0 + c < OW) {
            float m1 = 0.f, m2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
#pragma unroll
            for (int k = 0; k < SSIM_WIN; ++k) {
                const float w = win.w[k];
                m1 += w * v[0][r][c + k];
                m2 += w * v[1][r][c + k];
                e11 += w * v[2][r][c + k];
                e22 += w * v[3][r][c + k];
                e12 += w * v[4][r][c + k];
            }
            const float mu1_sq = m1 * m1, mu2_sq = m2 * m2, mu12 = m1 * m2;
            const float s1 = e11 - mu1_sq, s2 = e22 - mu2_sq, s12 = e12 - mu12;       // (compensation = 1.0)
            const float cs = (2.f * s12 + C2) / (s1 + s2 + C2);
            acc += ((2.f * mu12 + C1) / (mu1_sq + mu2_sq + C1)) * cs;
        }
    }
    return acc;
}

__global__ void __launch_bounds__(256) ssim_partial_kernel(const float* X, const float* Y, float* partial, int H, int W, int tiles_x,
                                                          int tiles_y, float C1, float C2, SsimWin win) {
    __shared__ float sx[SSIM_IN][SSIM_IN + 1], sy[SSIM_IN][SSIM_IN + 1];
    __shared__ float v[5][SSIM_T][SSIM_IN + 1];            // after the pass along H: [quantity][out row][in col]
    __shared__ float red[4];
    const int plane = blockIdx.z, ty = blockIdx.y, tx = blockIdx.x, tid = threadIdx.x;
    const int OH = H - SSIM_WIN + 1, OW = W - SSIM_WIN + 1;
    const int y0 = ty * SSIM_T, x0 = tx * SSIM_T;
    const float* px = X + (size_t)plane * H * W;
    const float* py = Y + (size_t)plane * H * W;
    for (int i = tid; i < SSIM_IN * SSIM_IN; i += 256) {
        const int r = i / SSIM_IN, c = i - r * SSIM_IN;
        const int gy = y0 + r, gx = x0 + c;
        const bool ok = gy < H && gx < W;
        sx[r][c] = ok ? px[(size_t)gy * W + gx] : 0.f;
        sy[r][c] = ok ? py[(size_t)gy * W + gx] : 0.f;
    }
    __syncthreads();
    float acc = ssim_tile_body(sx, sy, v, y0, x0, OH, OW, C1, C2, win, tid);
    acc = cdf_wave_sum(acc);
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) partial[((size_t)plane * tiles_y + ty) * tiles_x + tx] = red[0] + red[1] + red[2] + red[3];
}

// The evaluation sweep's metric step (diffusion.py:1121-1143 of the decolorization / snowification packages): the ORIGINALS against up to
// four candidate sets in one pass.  A block owns one 32 x 32 output tile of one plane as above; the original's 42 x 42 tile is loaded
// into LDS once, then every candidate in turn goes through the second buffer, the two filter passes (v is reused) and the SSIM sum, and
// leaves its squared error on the way in.  HBM traffic: 4 (1 + K) B / pixel; LDS as ssim_partial_kernel (~42 KB).
// Squared-error ownership: the 42-wide input windows of neighbouring tiles overlap by 10 and the output tiles stop 10 short of the right
// and bottom edges, so a tile owns input rows / columns [32 t, 32 (t + 1)) and the LAST tile of a row / column owns through the image
// edge (at most 42): every pixel is counted exactly once.
// shift: every value becomes (v + 1) * 0.5 as it is loaded (stored form [-1, 1], metrics on [0, 1]); positions outside the image stay 0.
__global__ void __launch_bounds__(256) eval_pairs_kernel(const float* X, const float* Y0, const float* Y1, const float* Y2, const float* Y3,
                                                        int K, int shift, float* ssim_partial, float* sse_partial, int planes, int H, int W,
                                                        int tiles_x, int tiles_y, float C1, float C2, SsimWin win) {
    __shared__ float sx[SSIM_IN][SSIM_IN + 1], sy[SSIM_IN][SSIM_IN + 1];
    __shared__ float v[5][SSIM_T][SSIM_IN + 1];
    __shared__ float red[8];
    const int plane = blockIdx.z, ty = blockIdx.y, tx = blockIdx.x, tid = threadIdx.x;
    const int OH = H - SSIM_WIN + 1, OW = W - SSIM_WIN + 1;
    const int y0 = ty * SSIM_T, x0 = tx * SSIM_T;
    const int own_h = ty == tiles_y - 1 ? SSIM_IN : SSIM_T, own_w = tx == tiles_x - 1 ? SSIM_IN : SSIM_T;
    const size_t base = (size_t)plane * H * W;
    const float* px = X + base;
    for (int i = tid; i < SSIM_IN * SSIM_IN; i += 256) {
        const int r = i / SSIM_IN, c = i - r * SSIM_IN;
        const int gy = y0 + r, gx = x0 + c;
        float xv = 0.f;
        if (gy < H && gx < W) {
            xv = px[(size_t)gy * W + gx];
            if (shift) xv = (xv + 1.f) * 0.5f;
        }
        sx[r][c] = xv;
    }
    __syncthreads();
    for (int k = 0; k < K; ++k) {
        const float* py = (k == 0 ? Y0 : k == 1 ? Y1 : k == 2 ? Y2 : Y3) + base;
        float sse = 0.f;
        for (int i = tid; i < SSIM_IN * SSIM_IN; i += 256) {
            const int r = i / SSIM_IN, c = i - r * SSIM_IN;
            const int gy = y0 + r, gx = x0 + c;
            float yv = 0.f;
            if (gy < H && gx < W) {
                yv = py[(size_t)gy * W + gx];
                if (shift) yv = (yv + 1.f) * 0.5f;
                if (r < own_h && c < own_w) {
                    const float d = sx[r][c] - yv;
                    sse += d * d;
                }
            }
            sy[r][c] = yv;
        }
        __syncthreads();
        float acc = ssim_tile_body(sx, sy, v, y0, x0, OH, OW, C1, C2, win, tid);
        acc = cdf_wave_sum(acc);
        sse = cdf_wave_sum(sse);
        if ((tid & 63) == 0) { red[tid >> 6] = acc; red[4 + (tid >> 6)] = sse; }
        __syncthreads();                      // also: every thread is past its last read of v and sy before the next candidate is loaded
        if (tid == 0) {
            const size_t o = (((size_t)k * planes + plane) * tiles_y + ty) * tiles_x + tx;
            ssim_partial[o] = red[0] + red[1] + red[2] + red[3];
            sse_partial[o] = red[4] + red[5] + red[6] + red[7];
        }
    }
}

extern "C" int cdf_ssim_tiles(int H, int W) {
    if (H < SSIM_WIN || W < SSIM_WIN) return 0;
    return cdf_cdiv(H - SSIM_WIN + 1, SSIM_T) * cdf_cdiv(W - SSIM_WIN + 1, SSIM_T);
}

extern "C" int cdf_ssim_partial(const float* x, const float* y, float* partial, int planes, int H, int W, const float* window11,
                                float C1, float C2, void* stream) {
    CDF_REQUIRE(x && y && partial && window11 && planes > 0, "cdf_ssim_partial: null pointer");
    CDF_REQUIRE(H >= SSIM_WIN && W >= SSIM_WIN, "cdf_ssim_partial: images must be at least 11 x 11 (got %d x %d)", H, W);
    SsimWin win;
    for (int k = 0; k < SSIM_WIN; ++k) win.w[k] = window11[k];      // (host pointer: 11 taps by value)
    const int tx = cdf_cdiv(W - SSIM_WIN + 1, SSIM_T), ty = cdf_cdiv(H - SSIM_WIN + 1, SSIM_T);
    CDF_LAUNCH(ssim_partial_kernel, dim3(tx, ty, planes), dim3(256), 0, CDF_S, x, y, partial, H, W, tx, ty, C1, C2, win);
    return cdf_check_launch("ssim_partial");
}

extern "C" int cdf_eval_pairs_partial(const float* x, const float* c0, const float* c1, const float* c2, const float* c3, int K, int shift,
                                      float* ssim_partial, float* sse_partial, int planes, int H, int W, const float* window11, float C1,
                                      float C2, void* stream) {
    CDF_REQUIRE(K >= 1 && K <= 4, "cdf_eval_pairs_partial: K must be 1...4 candidate sets (got %d)", K);
    const float* c[4] = {c0, c1, c2, c3};
    for (int k = 0; k < K; ++k) CDF_REQUIRE(c[k], "cdf_eval_pairs_partial: null pointer (candidate %d of %d)", k, K);
    CDF_REQUIRE(x && ssim_partial && sse_partial && window11 && planes > 0, "cdf_eval_pairs_partial: null pointer");
    CDF_REQUIRE(H >= SSIM_WIN && W >= SSIM_WIN, "cdf_eval_pairs_partial: images must be at least 11 x 11 (got %d x %d)", H, W);
    SsimWin win;
    for (int k = 0; k < SSIM_WIN; ++k) win.w[k] = window11[k];
    const int tx = cdf_cdiv(W - SSIM_WIN + 1, SSIM_T), ty = cdf_cdiv(H - SSIM_WIN + 1, SSIM_T);
    CDF_LAUNCH(eval_pairs_kernel, dim3(tx, ty, planes), dim3(256), 0, CDF_S, x, c0, c1, c2, c3, K, shift ? 1 : 0, ssim_partial, sse_partial,
               planes, H, W, tx, ty, C1, C2, win);
    return cdf_check_launch("eval_pairs_partial");
}
