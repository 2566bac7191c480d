// cdf_gemm_args.h -- host-side marshalling the gather-GEMM entry points share: the phase record of the kernel argument structs and its
// parser, the filler of the fields ConvArgs (k_conv.hip), SpArgs and SpxArgs (cdf_conv_sp.h) have in common.  The structs themselves
// stay apart: their layout is the kernels' kernarg layout.  (The weight-gradient argument structs' geometry filler: cdf_wgrad.h.)
#pragma once
#include "cdf_common.h"
#include "cdf_epilogue.h"

#define CDF_MAX_TAPS 16

struct CdfPhase {
    int oy, ox, ntaps;
    signed char dy[CDF_MAX_TAPS], dx[CDF_MAX_TAPS], wi[CDF_MAX_TAPS];
};

// phase_desc: per phase [oy, ox, ntaps, (dy, dx, wi) * ntaps]
static inline int cdf_fill_phases(CdfPhase* ph, int nphase, const int* pd, const char* who) {
    for (int p = 0; p < nphase; ++p) {
        ph[p].oy = pd[0]; ph[p].ox = pd[1]; ph[p].ntaps = pd[2];
        CDF_REQUIRE(pd[2] >= 0 && pd[2] <= CDF_MAX_TAPS, "%s: too many taps (%d)", who, pd[2]);
        for (int t = 0; t < pd[2]; ++t) {
            ph[p].dy[t] = (signed char)pd[3 + 3 * t];
            ph[p].dx[t] = (signed char)pd[4 + 3 * t];
            ph[p].wi[t] = (signed char)pd[5 + 3 * t];
        }
        pd += 3 + 3 * pd[2];
    }
    return CDF_OK;
}

// Output, epilogue operands, geometry and epilogue modes of a gather-GEMM launch.  vec is the layout test alone (cdf_epi_vec_ok); the
// operand tensors, their pitches and whatever else an entry point's own rules decide stay with the entry point.
template <class Args>
static inline void cdf_fill_gemm_common(Args& a, float* y, int ldy, const float* bias, const float* sbias, int ld_sbias, const float* res, int ldr,
                                        float* pre, int ldp, const float* mul, int ldm, int B, int H, int W, int Cin, int OH, int OW, int Cout,
                                        int QH, int QW, int os, int is, int nphase, int act, int mul_mode, int accumulate, void* ys_hi,
                                        void* ys_lo, int ld_ys, int io_bf) {
    a.y = y; a.bias = bias; a.sbias = sbias; a.res = res; a.pre = pre; a.mul = mul;
    a.ldy = ldy; a.ld_sbias = ld_sbias; a.ldr = ldr; a.ldp = ldp; a.ldm = ldm;
    a.B = B; a.H = H; a.W = W; a.Cin = Cin; a.OH = OH; a.OW = OW; a.Cout = Cout; a.QH = QH; a.QW = QW; a.os = os; a.is = is;
    a.act = act; a.mul_mode = mul_mode; a.accumulate = accumulate; a.nphase = nphase;
    a.vec = cdf_epi_vec_ok(Cout, y, ldy, bias, sbias, ld_sbias, res, ldr, pre, ldp, mul, ldm);
    a.ys_hi = (unsigned short*)ys_hi; a.ys_lo = (unsigned short*)ys_lo; a.ld_ys = ld_ys; a.io_bf = io_bf;
}
// SpArgs / SpxArgs: the generic epilogue, no LayerNorm backward
template <class Args>
static inline void cdf_clear_epi(Args& a) {
    a.epi = 0;
    a.ln_x = nullptr; a.ln_mean = nullptr; a.ln_rstd = nullptr; a.ln_part = nullptr; a.ld_lnx = 0;
}
