// cdf_wgrad.h -- what the weight-gradient GEMM kernels share around their K loops: conv_wgrad_kernel (k_conv.hip, exact fp32),
// conv_wgrad_sp_kernel (k_conv_sp.hip, in-kernel split), conv_wgrad_spx_kernel and conv_wgrad_row3_kernel (k_conv_wgrad_spx.hip, pre-split
// planes).  All four compute  out[split][tap][ca][cb] = sum_{m in split} XA[pixA(m, tap)][ca] * XB[pixB(m, tap)][cb],  m = (b, qy, qx).
// Here: the geometry filler of their argument structs (host), a block's tile / tap / split / pixel range, the pixel walk, the fold of the
// fused bias gradient, a split's slab and the pad zeroing of the float4 stores, as templates over the argument struct (WgradArgs, SpWgradArgs,
// SpxWgradArgs stay apart: their layout is the kernarg layout).  Kept per kernel, each on a measurement (profiles/wgrad_family_ab.txt):
//   conv_wgrad_row3_kernel   its own range, bias fold and staged store (it shares cdf_wgrad_zero_pad and cdf_tr_frag);
//   conv_wgrad_kernel        all of its text, the carry as a loop: each shared form put one of its instantiations above the parent's range;
// so the scalar store has no second user and stays with conv_wgrad_sp_kernel, the staged one with conv_wgrad_spx_kernel (STACK2 row map).
#pragma once
#include "cdf_gemm_args.h"

// The pixel walk below is exact while QW + BK and QH + BK stay below this (BK <= 32); cdf_fill_wgrad_geom refuses the rest.  (The widest
// plans of the Python layer are the 1 x n ones of the batched fp32 form, QW = n <= 16384.)
#define CDF_WGRAD_MAX_Q (1 << 21)

// Geometry, tap table (tap_desc: per tap [day, dax, dby, dbx]) and split of a weight-gradient launch; bk = the kernel's pixels per K step
// (a split is a whole number of steps).
template <class Args>
static inline int cdf_fill_wgrad_geom(Args& a, const char* who, int B, int QH, int QW, int HA, int WA, int sa, int HB, int WB, int sb, int CA,
                                      int CB, int ntaps, const int* tap_desc, int nsplit, int bk) {
    CDF_REQUIRE(ntaps >= 1 && ntaps <= CDF_MAX_TAPS && tap_desc && nsplit >= 1, "%s: bad tap / split count", who);
    CDF_REQUIRE(QH >= 1 && QW >= 1 && QH < CDF_WGRAD_MAX_Q && QW < CDF_WGRAD_MAX_Q, "%s: pixel grid %d x %d outside 1 .. 2^21 - 1", who, QH, QW);
    a.B = B; a.QH = QH; a.QW = QW; a.HA = HA; a.WA = WA; a.sa = sa; a.HB = HB; a.WB = WB; a.sb = sb;
    a.CA = CA; a.CB = CB; a.ntaps = ntaps; a.nsplit = nsplit;
    a.m_per_split = cdf_cdiv(cdf_cdiv(B * QH * QW, nsplit), bk) * bk;
    for (int t = 0; t < ntaps; ++t) {
        a.day[t] = (signed char)tap_desc[4 * t + 0];
        a.dax[t] = (signed char)tap_desc[4 * t + 1];
        a.dby[t] = (signed char)tap_desc[4 * t + 2];
        a.dbx[t] = (signed char)tap_desc[4 * t + 3];
    }
    return CDF_OK;
}

// ---- block and split range.  Grid (tiles, taps or tap groups, splits) in the XCD-aware order of cdf_wgrad_block.  T: the tile
// width along cb.
struct CdfWgradRange {
    int tile_a, tile_b, tap, split;            // tap: grid y as it is (a tap, a pair of taps, a row of taps)
    int m_lo, m_hi, niter;                     // pixels [m_lo, m_hi) in niter steps of BK
    // this block also sums the XB rows of its split
    template <class Args> __device__ __forceinline__ bool bsum(const Args& a) const { return a.bsum != nullptr && tile_a == 0 && tap == 0; }
};
template <int BK, int T, class Args>
__device__ __forceinline__ CdfWgradRange cdf_wgrad_range(const Args& a, int xcd_swizzle) {
    CdfWgradRange g;
    const int tiles_b = (a.CB + T - 1) / T;
    int bx;
    cdf_wgrad_block(xcd_swizzle, bx, g.tap, g.split);
    g.tile_a = bx / tiles_b;
    g.tile_b = bx - g.tile_a * tiles_b;
    const int M = a.B * a.QH * a.QW;
    g.m_lo = g.split * a.m_per_split;
    g.m_hi = g.m_lo + a.m_per_split;
    if (g.m_hi > M) g.m_hi = M;
    g.niter = g.m_hi > g.m_lo ? (g.m_hi - g.m_lo + BK - 1) / BK : 0;
    return g;
}

// ---- the pixel walk.  q = (qx, qy, b) of pixel m, decoded once per load slot and then advanced by BK pixels per K step -- however many
// image rows and images that crosses.  advance is straight-line code on purpose: a divergent branch or loop between the loads makes hipcc
// wait for the loads already in flight before it.  The carries are quotients by a float reciprocal: x = qx + BK < QW + BK, the true
// quotient (x + 0.5) / QW is at least 1 / (2 QW) away from every integer, and the computed one is off by at most 2^-23 of its value (one
// rounding of the reciprocal, one of the product; x + 0.5 itself is exact below 2^23), i.e. by less than (QW + BK) 2^-23 / QW: the
// truncation is exact while QW + BK < 2^22, and likewise for qy + carry < QH + BK.  CDF_WGRAD_MAX_Q keeps a factor of two below that, which
// also covers a 2.5-ulp reciprocal (a build without correctly rounded fp32 division): 3 2^-23 (QW + BK) / QW < 1 / (2 QW) up to 2^21.
template <int BK>
struct CdfPixelWalk {
    int QW, QH;
    float rcp_qw, rcp_qh;
    template <class Args>
    __device__ __forceinline__ explicit CdfPixelWalk(const Args& a) : QW(a.QW), QH(a.QH), rcp_qw(1.0f / (float)a.QW), rcp_qh(1.0f / (float)a.QH) {}
    __device__ __forceinline__ void decode(int m, int* q) const {
        q[0] = m % QW;
        const int t2 = m / QW;
        q[1] = t2 % QH;
        q[2] = t2 / QH;
    }
    __device__ __forceinline__ void advance(int* q) const {
        const int x = q[0] + BK;
        const int cx = (int)(((float)x + 0.5f) * rcp_qw);
        q[0] = x - cx * QW;
        const int y = q[1] + cx;
        const int cy = (int)(((float)y + 0.5f) * rcp_qh);
        q[1] = y - cy * QH;
        q[2] += cy;
    }
};

// ---- the bias-gradient fold (blocks with g.bsum(a)).  The lanes' partial sums lie in LDS as red[BK][T]; column c is summed in ascending k --
// the order is part of the result -- and goes to bsum[row][tile_b T + c], pad columns zeroed.  NTHR: threads of the block.  A caller that
// reuses red afterwards adds its own barrier.
template <int BK, int T, int NTHR, class Args>
__device__ __forceinline__ void cdf_wgrad_bsum_fold(const Args& a, const float* red, int tile_b, int row, int tid) {
    __syncthreads();
    for (int c = tid; c < T; c += NTHR) {
        float t = 0.f;
        for (int k = 0; k < BK; ++k) t += red[k * T + c];
        const int cc = tile_b * T + c;
        if (cc < a.ldo) a.bsum[(long long)row * a.ldo + cc] = cc < a.CB ? t : 0.f;
    }
}

// ---- the slab of (split, tap): out[split][tap][CA][ldo].  
template <class Args>
__device__ __forceinline__ float* cdf_wgrad_slab(const Args& a, int split, int tap) {
    return a.out + ((long long)split * a.ntaps + tap) * a.CA * a.ldo;
}

// ---- the staged float4 stores (spx, row3) zero the pitch padding with this; ldo % 4 == 0 keeps the store itself in bounds.
__device__ __forceinline__ void cdf_wgrad_zero_pad(float4& v, int col, int CB) {
    if (col + 3 >= CB) {
        if (col + 0 >= CB) v.x = 0.f;
        if (col + 1 >= CB) v.y = 0.f;
        if (col + 2 >= CB) v.z = 0.f;
        v.w = 0.f;
    }
}
