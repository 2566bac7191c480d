"""The pre-split GEMM family (cdf_conv_gemm_bf16x[_io], cdf_conv_gemm_bf16x_lnbwd, cdf_conv_wgrad_bf16x) at the shapes, epilogues and split
counts the product launches -- one case for every kernel FORM the dispatchers reach there (include/colddiff.h: cdf_conv_gemm_bf16x_form,
cdf_conv_wgrad_bf16x_form), at the shape it was recorded at.  Conventions of test_kernels_production.py: poisoned outputs, two launches
that must agree bit for bit, a stated bound, every worst error / bound printed.

Shapes: BENCH_GEMM / BENCH_WGRAD below are rows of a test_gpu_invariance.Recorder recording on the MI355X of one bench step in each
arithmetic mode (bf16x3, bf16), one sampler step (B = 16) and one forward + backward pass of BASELINE config 2's network (B = 128,
32 x 32): one row per distinct (kernel form, NS, epilogue operand list).  test_gpu_invariance.py::test_coverage_guard records again and
fails when a form is reached that no row resolves to, or when a row is no longer launched.

Reference: the SAME operation in float64 on the operands the kernel gets.  Activations are split by cdf_split_bf16 and weights by
cdf_pack_weight_bf16 (both tested bit-exactly elsewhere), the planes are widened to float64 and
    sum a_hi b_hi + a_hi b_lo + a_lo b_hi     (NS = 3)          sum a_hi b_hi     (NS = 1)
is evaluated with F.conv2d / F.conv_transpose2d / torch.nn.grad.conv2d_weight in float64 (a_hi (b_hi + b_lo) is one convolution: the
sum of the two planes is exact in float64), followed by the epilogue in float64.  On the GPU backend the float64 reference runs on the
device with torch ops, a few images at a time, for EVERY image -- a wrong tile is the failure these tests exist for -- and the CPU
float64 evaluation of sample(B) images cross-checks it.  No cdf_* GEMM is ever the reference.

Bound: the kernel may differ from that reference by fp32 accumulation only: test_kernels_production's model
    K_SUM 2^-24 sqrt(n) max ||terms||_2,     n = NS taps Cin (outputs),   n = NS M (weight gradients)
plus one fp32 rounding of each epilogue operand's magnitude; the non-linear epilogue stages carry the error through their Lipschitz
constants (|GELU'| <= 1.13, |SiLU'| <= 1.1, |GELU''| <= 0.8) and add the documented error of the library's erf (Abramowitz & Stegun
7.1.26: 1.5e-7 absolute, csrc/cdf_common.h) -- see _epilogue64.  Second assertion, unchanged from test_kernels.py::_spx_case: the
distance to the TRUE float64 convolution of the unsplit operands stays within 3e-5 max(1, |ref|max) (2e-2 for NS = 1).

K_SUM stays 4 for the GEMMs.  Worst error / bound over all cases of this module on the MI355X (144 GPU cases):
    GEMM outputs                y 0.41 (NS = 3), 0.29 (NS = 1);   pre-activation / GELU' output 0.37, 0.55 (bf16 storage)
    GEMM output planes          hi + lo 0.29;   hi only 0.87 (the bound there is bf16's own half ulp, 2^-8 |v|)
    true float64 convolution    0.26 of 3e-5 max (NS = 3), 0.20 of 2e-2 max (NS = 1)
    LayerNorm-backward epilogue dh 0.007, dg 0.003, db 0.13
    weight gradients            dW 0.069 (NS = 3), 0.059 (NS = 1), 0.058 (fp32 kernel, 995 slabs);   db 0.034
    device float64 reference against the CPU float64 evaluation of sample(B) images: 8.9e-16
"""
import ctypes
import math
from typing import NamedTuple

import pytest
import torch
import torch.nn.functional as F

from colddiff import convdesc as cd
from poison import nan_empty
from test_kernels import P, _split, r4
from test_kernels_production import K_SUM, U, bits_equal, check, sample, sum_bound, twice

# ---------------------------------------------------------------------------------------------------------------------------------
# kernel-form codes (include/colddiff.h)
# ---------------------------------------------------------------------------------------------------------------------------------
ROWHALO, HALO, SPX = 1, 2, 3


def decode(code):
    assert code > 0, code
    return dict(form=code >> 24, bm=((code >> 20) & 15) * 64, bn=((code >> 16) & 15) * 64, stages=(code >> 12) & 15, ksplit=(code >> 4) & 255,
                w=(code & 15) * 16)


def _pads(pad):
    """(top, left, bottom, right).  pad >= 0: symmetric; -1: one row / column at the bottom / right only (the strided 3 x 3 downsampling
    convolution of config 2); a pair (ph, pw): ph rows above and below, pw columns left and right (the 1 x 7 / 7 x 1 layers of the FID
    extractor)."""
    if isinstance(pad, tuple):
        return (pad[0], pad[1], pad[0], pad[1])
    return (0, 0, 1, 1) if pad == -1 else (pad, pad, pad, pad)


class TapSubset(NamedTuple):
    """The `k` of a row that launches taps lo .. hi-1 (row-major, tap = ky kw + kx) of a kh x kw convolution over the weight packed with
    all kh kw taps -- the plans colddiff.inception._tap_parts cuts a 25-tap layer into (0 .. 15, then 16 .. 24, accumulating).  Such a row
    computes the convolution whose absent taps have zero weights."""
    kh: int
    kw: int
    lo: int
    hi: int

    def __str__(self):
        return f"{self.kh}x{self.kw}taps{self.lo}to{self.hi}"


def _khw(k):
    """(kh, kw) of a row's k: an int (square), a pair, or a TapSubset."""
    return (k, k) if isinstance(k, int) else (k[0], k[1])


def tap_mask(w, k):
    """w [.][.][kh][kw] with the taps a TapSubset row does not launch set to zero (any other k: w itself)."""
    if not isinstance(k, TapSubset):
        return w
    keep = torch.zeros(k.kh * k.kw, dtype=torch.bool)
    keep[k.lo:k.hi] = True
    return w * keep.view(k.kh, k.kw).to(w.device, w.dtype)


def gemm_plan(kind, H, W, k, s, pad):
    """H, W: the arguments of the colddiff.convdesc constructor `kind` (the convolution's own input size).  k, pad: an int or an (h, w)
    pair; k a TapSubset (conv_fwd only): the full plan's geometry with that slice of its taps, weight indices unchanged."""
    kh, kw = _khw(k)
    if isinstance(k, TapSubset):
        assert kind == "conv_fwd"
        full = cd.conv_fwd(H, W, kh, kw, s, *_pads(pad))
        d = list(full.desc)
        taps = [tuple(d[3 + 3 * t:6 + 3 * t]) for t in range(d[2])][k.lo:k.hi]
        return cd.GemmPlan(full.H, full.W, full.OH, full.OW, full.QH, full.QW, full.os, full.istride, [(0, 0, taps)], full.ntaps_w)
    if kind in ("conv_fwd", "conv_dgrad"):
        return getattr(cd, kind)(H, W, kh, kw, s, *_pads(pad))
    return getattr(cd, kind)(H, W, kh, kw, s, pad)


def wgrad_plan(kind, H, W, k, s, pad):
    return cd.conv_wgrad(H, W, k, k, s, *_pads(pad)) if kind == "conv_wgrad" else cd.convT_wgrad(H, W, k, k, s, pad)


def _identify(kinds, make, geom, desc):
    """The (kind, H, W, k, s, pad) whose plan reproduces a recorded geometry + descriptor."""
    for kind in kinds:
        for k in (1, 3, 4, 2, 5, 7):
            for s in (1, 2):
                for pad in (0, 1, -1, 2, 3):
                    if pad == -1 and not kind.startswith("conv_"):
                        continue
                    for (H, W) in geom["sizes"]:
                        try:
                            pl = make(kind, H, W, k, s, pad)
                        except (AssertionError, ValueError, ZeroDivisionError):
                            continue
                        if geom["match"](pl) and list(pl.desc) == desc:
                            return kind, H, W, k, s, pad
    raise LookupError("no colddiff.convdesc plan reproduces %r %r" % (geom["what"], desc))


def _ndesc(nphase, desc):
    n, p = 0, 0
    for _ in range(nphase):
        n += 3 + 3 * desc[p + 2]
        p = n
    return n


def gemm_row(name, a):
    """A recorded cdf_conv_gemm_bf16x / _io / _lnbwd call (name, args) -> its BENCH_GEMM row:
    (entry, kind, B, H, W, Cin, Cout, k, s, pad, nphase, operands, act, mul_mode, accumulate, io_bf16, planes, y, ws, NS)
    operands: letters of the epilogue operands present (b bias, s per-sample bias, r residual, p pre-activation output, m multiplier);
    planes: 0 none, 1 hi, 2 hi + lo; y: an fp32 output is written; ws: a split-K workspace is passed."""
    ns = 3 if a[1] else 1
    if name == "cdf_conv_gemm_bf16x_lnbwd":
        B, H, W, Cin, Cout = a[7:12]
        geo, desc = (H, W, H, W, H, W, 1, 1, 1), list(a[12][:_ndesc(1, a[12])])
        rest = ("", 0, 0, 0, 0, 0, 1, 0)
    else:
        io = name.endswith("_io")
        B, H, W, Cin, OH, OW, Cout, QH, QW, os_, is_, nphase = a[9:21]
        geo, desc = (H, W, OH, OW, QH, QW, os_, is_, nphase), list(a[21][:_ndesc(nphase, a[21])])
        bias, sbias, res, pre, mul = a[22], a[23], a[25], a[27], a[29]
        act, mm, acc = a[31:34]
        t = a[34 + io:]
        ops = "".join(c for c, v in zip("bsrpm", (bias, sbias, res, pre, mul)) if v)
        rest = (ops, act, mm, acc, a[34] if io else 0, (1 if t[0] else 0) + (1 if t[1] else 0), 1 if a[7] else 0, 1 if t[3] else 0)
    geom = dict(what=geo, sizes=sorted({(geo[0], geo[1]), (geo[2], geo[3])}),
                match=lambda pl: (pl.H, pl.W, pl.OH, pl.OW, pl.QH, pl.QW, pl.os, pl.istride, pl.nphase) == geo)
    kind, Hc, Wc, k, s, pad = _identify(("conv_fwd", "conv_dgrad", "convT_fwd", "convT_dgrad"), gemm_plan, geom, desc)
    return ("lnbwd" if name.endswith("lnbwd") else "gemm", kind, B, Hc, Wc, Cin, Cout, k, s, pad, geo[8]) + rest + (ns,)


def wgrad_row(name, a):
    """A recorded cdf_conv_wgrad_bf16x call -> its BENCH_WGRAD row: (kind, B, H, W, CA, CB, k, s, pad, nsplit, bsum, NS)."""
    B, QH, QW, HA, WA, sa, HB, WB, sb, CA, CB, ntaps = a[9:21]
    desc, geo = list(a[21][:4 * ntaps]), (QH, QW, HA, WA, sa, HB, WB, sb)
    geom = dict(what=geo, sizes=sorted({(HA, WA), (QH, QW)}), match=lambda pl: (pl.QH, pl.QW, pl.HA, pl.WA, pl.sa, pl.HB, pl.WB, pl.sb) == geo)
    kind, Hc, Wc, k, s, pad = _identify(("conv_wgrad", "convT_wgrad"), wgrad_plan, geom, desc)
    return (kind, B, Hc, Wc, CA, CB, k, s, pad, a[22], 1 if a[23] else 0, 3 if a[1] else 1)


def gemm_form(L, row, tune=0):
    """(form code, tiles, blocks) of the launch a BENCH_GEMM row makes."""
    entry, kind, B, H, W, Cin, Cout, k, s, pad, nphase, ops, act, mm, acc, io, planes, has_y, ws, ns = row
    pl = gemm_plan(kind, H, W, k, s, pad)
    tg = (ctypes.c_int * 2)()
    code = L.cdf_conv_gemm_bf16x_form(B, pl.H, pl.W, Cin, Cout, pl.QH, pl.QW, pl.os, pl.istride, pl.nphase, pl.desc, ns,
                                      (1 << 40) if ws else 0, 1 if entry == "lnbwd" else 0, tune, ctypes.addressof(tg))
    assert code > 0, (row, L.cdf_last_error())
    return code, tg[0], tg[1]


def wgrad_form(L, row, tune=0):
    kind, B, H, W, CA, CB, k, s, pad, nsplit, bsum, ns = row
    wp = wgrad_plan(kind, H, W, k, s, pad)
    tg = (ctypes.c_int * 2)()
    code = L.cdf_conv_wgrad_bf16x_form(wp.QH, wp.QW, wp.HA, wp.WA, wp.sa, wp.HB, wp.WB, wp.sb, CA, CB, wp.ntaps, wp.desc, ns, nsplit, tune,
                                       ctypes.addressof(tg))
    assert code > 0, (row, L.cdf_last_error())
    return code, tg[0], tg[1]


# ---------------------------------------------------------------------------------------------------------------------------------
# recorded rows (see the module docstring; regenerate with test_gpu_invariance._guard_calls + gemm_row / wgrad_row)
# ---------------------------------------------------------------------------------------------------------------------------------
BENCH_GEMM = [
    ('gemm', 'conv_dgrad', 64, 128, 128, 64, 128, 3, 1, 1, 1, 'm', 0, 1, 0, 0, 0, 1, 0, 1),
    ('gemm', 'conv_dgrad', 64, 128, 128, 64, 128, 3, 1, 1, 1, 'm', 0, 1, 0, 0, 0, 1, 0, 3),
    ('gemm', 'conv_dgrad', 64, 128, 128, 64, 128, 3, 1, 1, 1, 'm', 0, 1, 0, 0, 2, 0, 0, 3),
    ('gemm', 'conv_dgrad', 64, 128, 128, 64, 128, 3, 1, 1, 1, 'm', 0, 1, 0, 4, 1, 0, 0, 1),
    ('gemm', 'conv_dgrad', 64, 128, 128, 128, 64, 3, 1, 1, 1, '', 0, 0, 0, 0, 1, 0, 0, 1),
    ('gemm', 'conv_fwd', 64, 128, 128, 64, 64, 4, 2, 1, 1, '', 0, 0, 0, 0, 0, 1, 0, 3),
    ('gemm', 'conv_fwd', 64, 128, 128, 64, 64, 4, 2, 1, 1, '', 0, 0, 0, 0, 1, 0, 0, 1),
    ('gemm', 'conv_fwd', 64, 128, 128, 64, 64, 4, 2, 1, 1, 'b', 0, 0, 0, 0, 0, 1, 0, 3),
    ('gemm', 'conv_fwd', 64, 128, 128, 64, 64, 4, 2, 1, 1, 'b', 0, 0, 0, 0, 1, 0, 0, 1),
    ('gemm', 'conv_fwd', 64, 128, 128, 64, 128, 3, 1, 1, 1, 'bp', 1, 0, 0, 0, 2, 0, 0, 3),
    ('gemm', 'conv_fwd', 64, 128, 128, 64, 128, 3, 1, 1, 1, 'bp', 1, 0, 0, 2, 1, 0, 0, 1),
    ('gemm', 'conv_fwd', 64, 128, 128, 128, 64, 3, 1, 1, 1, 'br', 0, 0, 0, 0, 0, 1, 0, 1),
    ('gemm', 'conv_fwd', 64, 128, 128, 128, 64, 3, 1, 1, 1, 'br', 0, 0, 0, 0, 0, 1, 0, 3),
    ('gemm', 'conv_fwd', 64, 128, 128, 128, 64, 3, 1, 1, 1, 'br', 0, 0, 0, 1, 1, 0, 0, 1),
    ('gemm', 'conv_fwd', 64, 128, 128, 256, 64, 1, 1, 0, 1, '', 0, 0, 1, 0, 0, 1, 0, 1),
    ('gemm', 'conv_fwd', 64, 128, 128, 256, 64, 1, 1, 0, 1, '', 0, 0, 1, 0, 0, 1, 0, 3),
    ('lnbwd', 'conv_dgrad', 64, 128, 128, 128, 64, 3, 1, 1, 1, '', 0, 0, 0, 0, 0, 1, 0, 3),
    ('gemm', 'conv_dgrad', 64, 64, 64, 128, 256, 3, 1, 1, 1, '', 0, 0, 0, 0, 0, 1, 0, 3),
    ('gemm', 'conv_dgrad', 64, 64, 64, 128, 256, 3, 1, 1, 1, '', 0, 0, 0, 0, 1, 0, 0, 1),
    ('gemm', 'conv_dgrad', 64, 64, 64, 128, 256, 3, 1, 1, 1, 'm', 0, 1, 0, 0, 2, 0, 0, 3),
    ('gemm', 'conv_dgrad', 64, 64, 64, 128, 256, 3, 1, 1, 1, 'm', 0, 1, 0, 4, 1, 0, 0, 1),
    ('gemm', 'conv_dgrad', 64, 64, 64, 256, 64, 3, 1, 1, 1, '', 0, 0, 0, 0, 1, 0, 0, 1),
    ('gemm', 'conv_fwd', 64, 64, 64, 64, 256, 1, 1, 0, 1, '', 0, 0, 0, 0, 1, 0, 0, 1),
    ('gemm', 'conv_fwd', 64, 64, 64, 128, 64, 3, 1, 1, 1, 'br', 0, 0, 0, 0, 0, 1, 0, 3),
    ('gemm', 'conv_fwd', 64, 64, 64, 128, 64, 3, 1, 1, 1, 'br', 0, 0, 0, 1, 1, 0, 0, 1),
    ('gemm', 'conv_fwd', 64, 64, 64, 128, 128, 4, 2, 1, 1, '', 0, 0, 0, 0, 0, 1, 0, 3),
    ('gemm', 'conv_fwd', 64, 64, 64, 128, 128, 4, 2, 1, 1, '', 0, 0, 0, 0, 1, 0, 0, 1),
    ('gemm', 'conv_fwd', 64, 64, 64, 128, 128, 4, 2, 1, 1, 'b', 0, 0, 0, 0, 0, 1, 0, 3),
    ('gemm', 'conv_fwd', 64, 64, 64, 128, 128, 4, 2, 1, 1, 'b', 0, 0, 0, 0, 1, 0, 0, 1),
    ('gemm', 'conv_fwd', 64, 64, 64, 128, 256, 3, 1, 1, 1, 'bp', 1, 0, 0, 0, 2, 0, 0, 3),
    ('gemm', 'conv_fwd', 64, 64, 64, 128, 256, 3, 1, 1, 1, 'bp', 1, 0, 0, 2, 1, 0, 0, 1),
    ('gemm', 'conv_fwd', 64, 64, 64, 256, 128, 1, 1, 0, 1, '', 0, 0, 1, 0, 0, 1, 0, 1),
    ('gemm', 'conv_fwd', 64, 64, 64, 256, 128, 1, 1, 0, 1, '', 0, 0, 1, 0, 0, 1, 0, 3),
    ('gemm', 'conv_fwd', 64, 64, 64, 256, 128, 3, 1, 1, 1, 'br', 0, 0, 0, 0, 0, 1, 0, 3),
    ('gemm', 'conv_fwd', 64, 64, 64, 256, 128, 3, 1, 1, 1, 'br', 0, 0, 0, 1, 1, 0, 0, 1),
    ('lnbwd', 'conv_dgrad', 64, 64, 64, 256, 64, 3, 1, 1, 1, '', 0, 0, 0, 0, 0, 1, 0, 3),
    ('lnbwd', 'conv_dgrad', 64, 64, 64, 256, 128, 3, 1, 1, 1, '', 0, 0, 0, 0, 0, 1, 0, 3),
    ('gemm', 'conv_fwd', 128, 32, 32, 256, 256, 3, 1, 1, 1, 'b', 0, 0, 0, 0, 0, 1, 0, 3),
    ('gemm', 'conv_fwd', 128, 32, 32, 384, 128, 3, 1, 1, 1, 'bs', 0, 0, 0, 0, 0, 1, 0, 3),
    ('gemm', 'conv_dgrad', 64, 32, 32, 256, 256, 4, 2, 1, 4, '', 0, 0, 0, 0, 0, 1, 0, 3),
    ('gemm', 'conv_dgrad', 64, 32, 32, 256, 256, 4, 2, 1, 4, 'b', 0, 0, 0, 0, 0, 1, 0, 3),
    ('gemm', 'conv_dgrad', 64, 32, 32, 256, 256, 4, 2, 1, 4, 'b', 0, 0, 0, 0, 1, 0, 0, 1),
    ('gemm', 'conv_dgrad', 64, 32, 32, 256, 512, 3, 1, 1, 1, '', 0, 0, 0, 0, 0, 1, 0, 3),
    ('gemm', 'conv_dgrad', 64, 32, 32, 256, 512, 3, 1, 1, 1, '', 0, 0, 0, 0, 1, 0, 0, 1),
    ('gemm', 'conv_dgrad', 64, 32, 32, 256, 512, 3, 1, 1, 1, 'm', 0, 1, 0, 0, 2, 0, 0, 3),
    ('gemm', 'conv_dgrad', 64, 32, 32, 256, 512, 3, 1, 1, 1, 'm', 0, 1, 0, 4, 1, 0, 0, 1),
    ('gemm', 'conv_fwd', 64, 32, 32, 256, 128, 1, 1, 0, 1, '', 0, 0, 1, 0, 0, 1, 0, 1),
    ('gemm', 'conv_fwd', 64, 32, 32, 256, 128, 1, 1, 0, 1, '', 0, 0, 1, 0, 0, 1, 0, 3),
    ('gemm', 'conv_fwd', 64, 32, 32, 256, 256, 4, 2, 1, 1, '', 0, 0, 0, 0, 0, 1, 0, 3),
    ('gemm', 'conv_fwd', 64, 32, 32, 256, 256, 4, 2, 1, 1, '', 0, 0, 0, 0, 1, 0, 0, 1),
    ('gemm', 'conv_fwd', 64, 32, 32, 256, 256, 4, 2, 1, 1, 'b', 0, 0, 0, 0, 0, 1, 0, 3),
    ('gemm', 'conv_fwd', 64, 32, 32, 256, 256, 4, 2, 1, 1, 'b', 0, 0, 0, 0, 1, 0, 0, 1),
    ('gemm', 'conv_fwd', 64, 32, 32, 256, 512, 3, 1, 1, 1, 'bp', 1, 0, 0, 0, 2, 0, 0, 3),
    ('gemm', 'conv_fwd', 64, 32, 32, 256, 512, 3, 1, 1, 1, 'bp', 1, 0, 0, 2, 1, 0, 0, 1),
    ('gemm', 'conv_fwd', 64, 32, 32, 512, 256, 3, 1, 1, 1, 'br', 0, 0, 0, 0, 0, 1, 0, 3),
    ('gemm', 'conv_fwd', 64, 32, 32, 512, 256, 3, 1, 1, 1, 'br', 0, 0, 0, 1, 1, 0, 0, 1),
    ('lnbwd', 'conv_dgrad', 64, 32, 32, 512, 128, 3, 1, 1, 1, '', 0, 0, 0, 0, 0, 1, 0, 3),
    ('gemm', 'conv_fwd', 128, 16, 16, 256, 256, 3, 1, 1, 1, 'b', 0, 0, 0, 0, 0, 1, 0, 3),
    ('gemm', 'conv_fwd', 128, 16, 16, 256, 256, 3, 2, -1, 1, 'b', 0, 0, 0, 0, 0, 1, 0, 3),
    ('gemm', 'conv_fwd', 128, 16, 16, 512, 256, 3, 1, 1, 1, 'bs', 0, 0, 0, 0, 0, 1, 0, 3),
    ('gemm', 'conv_dgrad', 64, 16, 16, 512, 1024, 3, 1, 1, 1, '', 0, 0, 0, 0, 0, 1, 0, 3),
    ('gemm', 'conv_dgrad', 64, 16, 16, 512, 1024, 3, 1, 1, 1, '', 0, 0, 0, 0, 1, 0, 0, 1),
    ('gemm', 'conv_dgrad', 64, 16, 16, 512, 1024, 3, 1, 1, 1, 'm', 0, 1, 0, 0, 2, 0, 0, 3),
    ('gemm', 'conv_dgrad', 64, 16, 16, 512, 1024, 3, 1, 1, 1, 'm', 0, 1, 0, 4, 1, 0, 0, 1),
    ('gemm', 'conv_dgrad', 64, 16, 16, 1024, 256, 3, 1, 1, 1, '', 0, 0, 0, 0, 0, 1, 0, 3),
    ('gemm', 'conv_dgrad', 64, 16, 16, 1024, 256, 3, 1, 1, 1, '', 0, 0, 0, 0, 1, 0, 0, 1),
    ('gemm', 'conv_fwd', 16, 32, 32, 256, 128, 3, 1, 1, 1, 'br', 0, 0, 0, 0, 0, 1, 0, 3),
    ('gemm', 'conv_fwd', 16, 32, 32, 256, 256, 4, 2, 1, 1, 'b', 0, 0, 0, 0, 0, 1, 1, 3),
    ('gemm', 'conv_fwd', 16, 32, 32, 512, 256, 3, 1, 1, 1, 'bp', 1, 0, 0, 0, 2, 0, 0, 3),
    ('gemm', 'conv_fwd', 16, 32, 32, 512, 256, 3, 1, 1, 1, 'br', 0, 0, 0, 0, 0, 1, 0, 3),
    ('gemm', 'conv_fwd', 64, 16, 16, 512, 256, 3, 1, 1, 1, 'br', 0, 0, 0, 0, 0, 1, 0, 3),
    ('gemm', 'conv_fwd', 64, 16, 16, 512, 256, 3, 1, 1, 1, 'br', 0, 0, 0, 1, 1, 0, 0, 1),
    ('gemm', 'conv_fwd', 64, 16, 16, 512, 1024, 3, 1, 1, 1, 'bp', 1, 0, 0, 0, 2, 0, 0, 3),
    ('gemm', 'conv_fwd', 64, 16, 16, 512, 1024, 3, 1, 1, 1, 'bp', 1, 0, 0, 2, 1, 0, 0, 1),
    ('gemm', 'conv_fwd', 64, 16, 16, 1024, 512, 3, 1, 1, 1, 'br', 0, 0, 0, 0, 0, 1, 0, 3),
    ('gemm', 'conv_fwd', 64, 16, 16, 1024, 512, 3, 1, 1, 1, 'br', 0, 0, 0, 1, 1, 0, 0, 1),
    ('gemm', 'conv_dgrad', 128, 8, 8, 256, 256, 3, 1, 1, 1, '', 0, 0, 0, 0, 0, 1, 0, 3),
    ('gemm', 'conv_fwd', 128, 8, 8, 256, 256, 3, 1, 1, 1, 'br', 0, 0, 0, 0, 0, 1, 0, 3),
    ('gemm', 'conv_fwd', 128, 8, 8, 256, 256, 3, 2, -1, 1, 'b', 0, 0, 0, 0, 0, 1, 1, 3),
    ('gemm', 'conv_fwd', 128, 8, 8, 512, 256, 3, 1, 1, 1, 'bs', 0, 0, 0, 0, 0, 1, 0, 3),
    ('gemm', 'conv_fwd', 16, 16, 16, 512, 256, 3, 1, 1, 1, 'br', 0, 0, 0, 0, 0, 1, 1, 3),
    ('gemm', 'conv_fwd', 16, 16, 16, 512, 1024, 3, 1, 1, 1, 'bp', 1, 0, 0, 0, 2, 0, 0, 3),
    ('gemm', 'conv_fwd', 16, 16, 16, 1024, 512, 3, 1, 1, 1, 'bp', 1, 0, 0, 0, 2, 0, 0, 3),
    ('gemm', 'conv_fwd', 16, 16, 16, 1024, 512, 3, 1, 1, 1, 'br', 0, 0, 0, 0, 0, 1, 0, 3),
    ('gemm', 'conv_dgrad', 128, 4, 4, 256, 512, 3, 1, 1, 1, '', 0, 0, 0, 0, 0, 1, 1, 3),
    ('gemm', 'conv_fwd', 128, 4, 4, 256, 256, 3, 1, 1, 1, 'br', 0, 0, 0, 0, 0, 1, 1, 3),
    ('gemm', 'conv_fwd', 128, 4, 4, 512, 256, 3, 1, 1, 1, 'bs', 0, 0, 0, 0, 0, 1, 1, 3),
]
BENCH_WGRAD = [
    ('conv_wgrad', 64, 128, 128, 64, 64, 4, 2, 1, 32, 1, 1),
    ('conv_wgrad', 64, 128, 128, 64, 64, 4, 2, 1, 32, 1, 3),
    ('conv_wgrad', 64, 128, 128, 64, 128, 3, 1, 1, 83, 1, 1),
    ('conv_wgrad', 64, 128, 128, 64, 128, 3, 1, 1, 83, 1, 3),
    ('conv_wgrad', 64, 128, 128, 64, 256, 1, 1, 0, 249, 0, 1),
    ('conv_wgrad', 64, 128, 128, 64, 256, 1, 1, 0, 249, 0, 3),
    ('conv_wgrad', 64, 128, 128, 128, 64, 3, 1, 1, 83, 1, 1),
    ('conv_wgrad', 64, 128, 128, 128, 64, 3, 1, 1, 83, 1, 3),
    ('convT_wgrad', 64, 64, 64, 64, 64, 4, 2, 1, 32, 0, 1),
    ('convT_wgrad', 64, 64, 64, 64, 64, 4, 2, 1, 32, 0, 3),
    ('conv_wgrad', 64, 64, 64, 64, 128, 1, 1, 0, 249, 1, 1),
    ('conv_wgrad', 64, 64, 64, 64, 256, 1, 1, 0, 249, 0, 1),
    ('conv_wgrad', 64, 64, 64, 64, 256, 1, 1, 0, 249, 0, 3),
    ('conv_wgrad', 64, 64, 64, 128, 256, 1, 1, 0, 249, 0, 1),
    ('conv_wgrad', 64, 64, 64, 128, 256, 1, 1, 0, 249, 0, 3),
    ('conv_wgrad', 64, 64, 64, 256, 64, 1, 1, 0, 249, 1, 1),
    ('conv_wgrad', 64, 64, 64, 256, 128, 3, 1, 1, 42, 1, 1),
    ('conv_wgrad', 64, 64, 64, 256, 128, 3, 1, 1, 42, 1, 3),
    ('conv_wgrad', 128, 32, 32, 128, 128, 3, 1, 1, 83, 1, 3),
    ('conv_wgrad', 64, 32, 32, 256, 256, 4, 2, 1, 8, 1, 3),
    ('conv_wgrad', 64, 32, 32, 512, 128, 1, 1, 0, 125, 1, 1),
]


# ---------------------------------------------------------------------------------------------------------------------------------
# float64 reference
# ---------------------------------------------------------------------------------------------------------------------------------
def _wide(plane, C):
    """bf16 plane [..., ld] (int16 bits) -> float64 [..., C]."""
    return plane.view(torch.bfloat16)[..., :C].double()


def _conv64(kind, x, w, k, s, pad, out_hw):
    """The convolution behind a `kind` plan in float64: x NCHW, w in the orientation _weights makes ([out][in][k][k] for the gathering
    kinds conv_fwd / convT_dgrad, [in][out][k][k] for the scattering kinds conv_dgrad / convT_fwd).  The kernel size is w's own, so a
    rectangular w and a pad pair (_pads) need nothing more; a TapSubset row passes w with its absent taps zeroed (tap_mask)."""
    pt, pl, pb, pr = _pads(pad)
    if kind in ("conv_fwd", "convT_dgrad"):
        return F.conv2d(F.pad(x, (pl, pr, pt, pb)), w, stride=s)
    y = F.conv_transpose2d(x, w, stride=s)                  # (full size; the padding is cropped away)
    OH, OW = out_hw
    y = F.pad(y, (0, max(0, pl + OW - y.shape[3]), 0, max(0, pt + OH - y.shape[2])))
    return y[:, :, pt:pt + OH, pl:pl + OW]


def _act64(v, act):
    return F.gelu(v) if act == 1 else (v * torch.sigmoid(v) if act == 2 else (v.clamp_min(0) if act == 3 else v))


def _actgrad64(u, act):
    if act == 1:
        return 0.5 * (1 + torch.erf(u / math.sqrt(2))) + u * torch.exp(-u * u / 2) / math.sqrt(2 * math.pi)
    sg = torch.sigmoid(u)
    return sg * (1 + u * (1 - sg))


def _epilogue64(v, e, o, act, mm, pre_grad):
    """cdf_epilogue_rows in float64 on the NCHW sums v whose error is bounded by e: -> (y, pre or None, error bound of y, of pre).
    o: float64 NCHW operands (bias [C], sbias [B][C], res, mul, y0).  Each line of the bound is the line of the epilogue next to it."""
    amax = lambda t: t.abs().max().item()
    if o.get("bias") is not None:
        v = v + o["bias"][None, :, None, None]
        e += U * amax(v)
    if o.get("sbias") is not None:
        v = v + o["sbias"][:, :, None, None]
        e += U * amax(v)
    pre, e_pre = None, 0.0
    if o.get("pre"):
        # pre = v, or act'(v) (CDF_IO_PRE_GRAD): |GELU''| <= 0.8, |SiLU''| <= 0.5; erf formula 1.5e-7 / 2, the exp and the sums a few roundings
        pre, e_pre = (_actgrad64(v, act), 0.8 * e + 0.75e-7 + 8 * U * (1 + amax(v))) if pre_grad else (v, e)
    if act:
        # |GELU'| <= 1.13, |SiLU'| <= 1.1, ReLU 1; GELU = 0.5 x (1 + erf): 0.75e-7 |x| from the erf formula; a few roundings of the result
        e = 1.13 * e + (0.75e-7 if act == 1 else 0.0) * amax(v) + 8 * U * amax(v)
        v = _act64(v, act)
    if mm:
        m = o["mul"] if mm == 3 else _actgrad64(o["mul"], mm)
        # the multiplier's own error (act' of a loaded value: erf formula + a few roundings), then one rounding of the product
        e = e * amax(m) + amax(v) * (0.0 if mm == 3 else 0.75e-7 + 8 * U * (1 + amax(o["mul"])))
        v = v * m
        e += U * amax(v)
    if o.get("res") is not None:
        v = v + o["res"]
        e += U * amax(v)
    if o.get("y0") is not None:
        v = v + o["y0"]
        e += U * amax(v)
    return v, pre, e, e_pre


def _dist(a, b):
    """max |a - b|; inf when anything is not finite (a poisoned element the kernel never wrote must not vanish in a max())."""
    d = (a.double() - b).abs().max().item()
    return d if math.isfinite(d) else math.inf


def _nchw(t, C):
    return t[..., :C].permute(0, 3, 1, 2)


def _weights(be, kind, Cin, Cout, k, ns, seed):
    """A weight in the orientation its convolution kind stores it, packed by cdf_pack_weight_bf16 the way the product packs it for this
    GEMM; returns (fp32 weight, hi plane, lo plane or None, ldk, the float64 weights the planes hold: hi, lo).  k: an int, a (kh, kw) pair or
    a TapSubset -- then every tap is packed, as the product packs it, and the three returned weights have the absent taps zeroed: they
    are the reference's operands, the planes are the kernel's."""
    kh, kw = _khw(k)
    KK = kh * kw
    g = torch.Generator().manual_seed(seed)
    gather = kind in ("conv_fwd", "convT_dgrad")
    w = torch.randn((Cout, Cin, kh, kw) if gather else (Cin, Cout, kh, kw), generator=g) / math.sqrt(Cin * KK)
    ldk = (Cin + 31) // 32 * 32
    hi = nan_empty(be, KK, Cout, ldk, dtype=torch.int16)
    lo = nan_empty(be, KK, Cout, ldk, dtype=torch.int16) if ns == 3 else None
    s_n, s_k = (Cin * KK, KK) if gather else (KK, Cout * KK)
    be.L.cdf_pack_weight_bf16(P(be.to(w)), P(hi), P(lo), KK, Cout, Cin, ldk, 1, s_n, s_k, be.stream())
    be._keep += [hi, lo]

    def unpack(plane):                                       # [tap][N][K] -> the weight's own layout
        t = _wide(plane, Cin)
        return (t.permute(1, 2, 0) if gather else t.permute(2, 1, 0)).reshape(w.shape).contiguous()
    return tap_mask(w, k), hi, lo, ldk, tap_mask(unpack(hi), k), (tap_mask(unpack(lo), k) if ns == 3 else None)


def _ref_chunks(B, per_image_bytes):
    n = max(1, min(B, int((2 << 30) // max(1, per_image_bytes))))
    return [(i, min(B, i + n)) for i in range(0, B, n)]


def _gemm_sums64(kind, k, s, pad, out_hw, xh, xl, wh, wl, x_true, w_true, imgs, dev):
    """float64 on `dev` for the images `imgs` (a slice or index list): the split-operand sums, max ||terms||_2 over the outputs, and the true
    convolution of the unsplit operands.  xh / xl: bf16 planes (NHWC, any device), wh / wl: float64 weights of the planes."""
    C = wh.shape[1] if kind in ("conv_fwd", "convT_dgrad") else wh.shape[0]
    a_hi = _nchw(_wide(xh[imgs].to(dev), C), C)
    b_hi = wh.to(dev)
    cv = lambda a, b: _conv64(kind, a, b, k, s, pad, out_hw)
    if xl is not None:
        a_lo, b_lo = _nchw(_wide(xl[imgs].to(dev), C), C), wl.to(dev)
        v = cv(a_hi, b_hi + b_lo) + cv(a_lo, b_hi)
        sq = cv(a_hi * a_hi, b_hi * b_hi + b_lo * b_lo) + cv(a_lo * a_lo, b_hi * b_hi)
    else:
        v, sq = cv(a_hi, b_hi), cv(a_hi * a_hi, b_hi * b_hi)
    true = cv(_nchw(x_true[imgs].to(dev).double(), C), w_true.to(dev).double())
    return v, sq.max().sqrt().item(), true


def _gemm_case(be, row, tune=None):
    entry, kind, B, H, W, Cin, Cout, k, s, pad, nphase, ops, act, mm, acc, io, planes, has_y, use_ws, ns = row
    L = be.L
    pl = gemm_plan(kind, H, W, k, s, pad)
    assert pl.nphase == nphase
    old = {f: be.tune.get(f) for f in (tune or {})}
    be.tune.set(**(tune or {}))
    try:
        code, tiles, grid = gemm_form(L, row, be.tune.ptr)
        tag = f"{entry} {kind} B={B} {pl.H}x{pl.W} {Cin}->{Cout} k{k}s{s} ops={ops or '-'} act={act} mul={mm} acc={acc} io={io} planes={planes} NS={ns}"
        print(f"{tag}: form {decode(code)} tiles {tiles} grid {grid}" + (f" tune {tune}" if tune else ""))
        torch.manual_seed(Cin + Cout + k)
        dev = be.device
        x = torch.randn(B, pl.H, pl.W, Cin)
        w, whi, wlo, ldk, wh64, wl64 = _weights(be, kind, Cin, Cout, k, ns, Cin * 7 + Cout)
        xd = be.to(x)
        xs = _split(be, xd, ns == 1)
        zero = be.zeros(16)
        ldo, ld8 = r4(Cout), (Cout + 7) // 8 * 8
        oshape = (B, pl.OH, pl.OW)
        if entry == "lnbwd":
            return _lnbwd_check(be, tag, row, pl, xs, x, w, whi, wlo, ldk, wh64, wl64, zero)
        bfbits = lambda t: t.bfloat16().view(torch.int16)
        o32 = {}                                             # fp32 / bf16 operands as the kernel reads them, widened for the reference
        bias = be.to(torch.randn(Cout)) if "b" in ops else None
        sbias = be.to(torch.randn(B, Cout)) if "s" in ops else None
        res = mul = None
        if "r" in ops:
            t = torch.randn(*oshape, Cout)
            res, o32["res"] = (be.to(bfbits(t)), t.bfloat16().float()) if io & 1 else (be.to(t), t)
        if "m" in ops:
            t = torch.randn(*oshape, Cout)
            mul, o32["mul"] = (be.to(bfbits(t)), t.bfloat16().float()) if io & 4 else (be.to(t), t)
        y0 = torch.randn(*oshape, Cout) if acc else None
        y = nan_empty(be, *oshape, ldo) if has_y else None
        pre = nan_empty(be, *oshape, Cout, dtype=torch.int16 if io & 2 else torch.float32) if "p" in ops else None
        yh = nan_empty(be, *oshape, ld8, dtype=torch.int16) if planes >= 1 else None
        yl = nan_empty(be, *oshape, ld8, dtype=torch.int16) if planes == 2 else None
        Mq = B * pl.QH * pl.QW
        # the workspace ops.conv_gemm_presplit passes: sized by cdf_conv_gemm_bf16x_ksplit, whether or not the dispatcher then takes a
        # split-K form (a layer the LDS-resident-input kernel serves leaves it untouched)
        ks = L.cdf_conv_gemm_bf16x_ksplit(Mq, Cout, pl.nphase, pl.desc[2], be.tune.ptr) if use_ws else 1
        assert decode(code)["ksplit"] in (1, ks)
        nws = ks * Mq * ldo if ks > 1 else 0
        ws = nan_empty(be, nws) if nws else None
        y0d = be.to(F.pad(y0, (0, ldo - Cout))) if acc else None

        def launch():
            if acc:
                y.copy_(y0d)                                 # (accumulate reads y: its previous contents are an input)
            L.cdf_conv_gemm_bf16x_io(P(xs[0]), P(xs[1]), xs[0].shape[-1], P(zero), P(whi), P(wlo), ldk, P(y), ldo if has_y else 0, B, pl.H, pl.W, Cin,
                                     pl.OH, pl.OW, Cout, pl.QH, pl.QW, pl.os, pl.istride, pl.nphase, pl.desc, P(bias), P(sbias), Cout if sbias is not None else 0,
                                     P(res), Cout, P(pre), Cout, P(mul), Cout, act, mm, acc, io, P(yh), P(yl), ld8 if planes else 0, P(ws), nws,
                                     be.tune.ptr, be.stream())
        outs = [t for t in (y, pre, yh, yl, ws) if t is not None]
        got = dict(zip([n for n, t in zip(("y", "pre", "yh", "yl", "ws"), (y, pre, yh, yl, ws)) if t is not None], twice(launch, outs)))

        # ---- reference, every image, in float64 on the backend's device; the CPU evaluation of sample(B) images cross-checks it
        ops64 = lambda lo_, hi_, d: dict(bias=None if bias is None else bias.to(d).double(), sbias=None if sbias is None else sbias[lo_:hi_].to(d).double(),
                                         res=None if res is None else _nchw(o32["res"][lo_:hi_].to(d).double(), Cout),
                                         mul=None if mul is None else _nchw(o32["mul"][lo_:hi_].to(d).double(), Cout),
                                         y0=None if y0 is None else _nchw(y0[lo_:hi_].to(d).double(), Cout), pre="p" in ops)
        n_terms = ns * pl.desc[2] * Cin
        worst = {}

        def compare(name, value, ref, bound):
            err = _dist(value, ref)
            w_ = worst.setdefault(name, [0.0, 0.0])
            w_[0], w_[1] = max(w_[0], err), max(w_[1], bound)

        per_img = 8 * (Cin * pl.H * pl.W * 4 + Cout * pl.OH * pl.OW * 8)
        tmax = [0.0, 0.0]
        for lo_, hi_ in _ref_chunks(B, per_img):
            v, tnorm, true = _gemm_sums64(kind, k, s, pad, (pl.OH, pl.OW), xs[0], xs[1], wh64, wl64, x, w, slice(lo_, hi_), dev)
            e0 = K_SUM * U * math.sqrt(n_terms) * tnorm
            o = ops64(lo_, hi_, dev)
            yr, prer, e_y, e_pre = _epilogue64(v, e0, o, act, mm, bool(io & 8))
            yt = _epilogue64(true, 0.0, o, act, mm, bool(io & 8))[0]
            tmax = [max(tmax[0], yt.abs().max().item()), tmax[1]]
            if has_y:
                gy = _nchw(got["y"][lo_:hi_].to(dev), Cout)
                compare("y", gy, yr, e_y)
                tmax[1] = max(tmax[1], _dist(gy, yt))
            if pre is not None:
                gp = got["pre"][lo_:hi_].to(dev)
                gp = gp.view(torch.bfloat16) if io & 2 else gp
                compare("pre", _nchw(gp, Cout), prer, e_pre + (2.0 ** -8 * prer.abs().max().item() if io & 2 else 0.0))   # (bf16: 8 significant bits)
            if planes:
                # the planes hold the stored value: hi = bf16(v) (8 significant bits, half an ulp <= 2^-8 |v|), hi + lo = v to 2^-16 |v|
                gh = _wide(got["yh"][lo_:hi_].to(dev), Cout)
                val = gh + _wide(got["yl"][lo_:hi_].to(dev), Cout) if planes == 2 else gh
                compare("planes", _nchw(val, Cout), yr, e_y + 2.0 ** (-16 if planes == 2 else -8) * yr.abs().max().item())
                if not has_y:
                    tmax[1] = max(tmax[1], _dist(_nchw(val, Cout), yt))
            if be.kind == "hip" and lo_ == 0:
                here = [i for i in sample(B) if lo_ <= i < hi_]
                vc = _gemm_sums64(kind, k, s, pad, (pl.OH, pl.OW), xs[0][here].cpu(), None if xs[1] is None else xs[1][here].cpu(), wh64, wl64, x[here], w,
                                  slice(None), "cpu")[0]
                dref = (v[[i - lo_ for i in here]].cpu() - vc).abs().max().item()
                print(f"{tag}: device float64 reference vs CPU float64 on images {here}: {dref:.3e}")
                assert dref <= 1e-12 * max(1.0, vc.abs().max().item())
        for name, (err, bound) in worst.items():
            print(f"{tag} {name}: worst error {err:.3e} / bound {bound:.3e} = {err / bound:.3f}")
            assert math.isfinite(err) and err <= bound, (tag, name, err, bound)
        tol = (3e-5 if ns == 3 else 2e-2) * max(1.0, tmax[0])
        print(f"{tag}: distance to the true float64 convolution {tmax[1]:.3e} / {tol:.3e} = {tmax[1] / tol:.3f}")
        assert tmax[1] <= tol, (tag, tmax, tol)
        # fused planes next to an fp32 output: cdf_split_bf16 of it, bit for bit
        if planes and has_y:
            rh, rl = _split(be, be.to(got["y"][..., :Cout]), planes == 1)
            assert torch.equal(got["yh"][..., :Cout], rh.cpu()[..., :Cout]), tag
            assert planes == 1 or torch.equal(got["yl"][..., :Cout], rl.cpu()[..., :Cout]), tag
        if decode(code)["ksplit"] > 1:
            assert torch.isfinite(got["ws"]).all(), (tag, "split-K workspace")
        return code
    finally:
        be.tune.set(**old)


def _lnbwd_check(be, tag, row, pl, xs, x, w, whi, wlo, ldk, wh64, wl64, zero):
    """cdf_conv_gemm_bf16x_lnbwd: dh = LayerNorm'(h)[the data-gradient sums], dg / db += the parameter gradients."""
    entry, kind, B, H, W, Cin, Cout, k, s, pad, nphase, ops, act, mm, acc, io, planes, has_y, use_ws, ns = row
    L, dev, M, C = be.L, be.device, B * H * W, Cout
    h, g = torch.randn(B, H, W, C) * 1.5 + 0.3, torch.randn(C)
    mean = h.mean(-1).reshape(M)
    rstd = (h.var(-1, unbiased=False) + 1e-5).rsqrt().reshape(M)
    hd, gd, md, rd = be.to(h), be.to(g), be.to(mean), be.to(rstd)
    dh, dg, db, part = nan_empty(be, B, H, W, C), nan_empty(be, C), nan_empty(be, C), nan_empty(be, M // 64 * 2 * C)
    dg0, db0 = torch.full((C,), 2.0), torch.full((C,), -3.0)
    dg0d, db0d = be.to(dg0), be.to(db0)

    def launch():
        dg.copy_(dg0d), db.copy_(db0d)                       # (the parameter gradients accumulate)
        L.cdf_conv_gemm_bf16x_lnbwd(P(xs[0]), P(xs[1]), xs[0].shape[-1], P(zero), P(whi), P(wlo), ldk, B, H, W, Cin, C, pl.desc, P(hd), C, P(md), P(rd),
                                    P(gd), P(dh), C, P(dg), P(db), P(part), be.tune.ptr, be.stream())
    dho, dgo, dbo, _ = twice(launch, [dh, dg, db, part])
    code = gemm_form(L, row, be.tune.ptr)[0]
    # the kernel uses the mean / rstd it is handed: the float64 LayerNorm backward on those statistics
    e_dh, e_dg = 0.0, 0.0
    dg_r, db_r = torch.zeros(C, dtype=torch.float64, device=dev), torch.zeros(C, dtype=torch.float64, device=dev)
    dg_t2, db_t2 = torch.zeros(C, dtype=torch.float64, device=dev), torch.zeros(C, dtype=torch.float64, device=dev)
    worst = [0.0, 0.0]
    for lo_, hi_ in _ref_chunks(B, 8 * (Cin + 6 * C) * H * W):
        v, tnorm, _ = _gemm_sums64(kind, k, s, pad, (H, W), xs[0], xs[1], wh64, wl64, x, w, slice(lo_, hi_), dev)
        e0 = K_SUM * U * math.sqrt(ns * 9 * Cin) * tnorm
        dhn = v.permute(0, 2, 3, 1).reshape(-1, C)
        h64, g64 = hd[lo_:hi_].double().reshape(-1, C), gd.double()
        mu, rs = md.double().view(B, -1)[lo_:hi_].reshape(-1, 1), rd.double().view(B, -1)[lo_:hi_].reshape(-1, 1)
        xh = (h64 - mu) * rs
        dxh = dhn * g64
        dx = rs * (dxh - dxh.mean(1, keepdim=True) - xh * (dxh * xh).mean(1, keepdim=True))
        # dh is linear in the sums with gain <= rstd |g| (2 + |xh|max |xh|): the sums' bound times that, plus the LayerNorm arithmetic's own
        # rounding (test_layernorm_production's 1e-5 at this scale)
        gain = (rs.max() * g64.abs().max() * (2 + xh.abs().max() ** 2)).item()
        bound = gain * e0 + 1e-5 * max(1.0, dx.abs().max().item())
        err = _dist(dho[lo_:hi_].to(dev).reshape(-1, C), dx)
        worst = [max(worst[0], err), max(worst[1], bound)]
        tg_, tb_ = dhn * xh, dhn
        dg_r += tg_.sum(0); db_r += tb_.sum(0)
        dg_t2 += (tg_ * tg_).sum(0); db_t2 += (tb_ * tb_).sum(0)
        e_dg = max(e_dg, e0 * xh.abs().max().item())
        e_dh = max(e_dh, e0)
    print(f"{tag} dh: worst error {worst[0]:.3e} / bound {worst[1]:.3e} = {worst[0] / worst[1]:.3f}")
    assert worst[0] <= worst[1], (tag, worst)
    # dg / db: fp32 sums of M terms (K_SUM model) of values that each carry the GEMM's error (zero-mean, independent: sqrt(M) of it)
    for name, got_, init, ref, t2, e1 in (("dg", dgo, 2.0, dg_r, dg_t2, e_dg), ("db", dbo, -3.0, db_r, db_t2, e_dh)):
        bound = K_SUM * U * math.sqrt(M) * t2.max().sqrt().item() + K_SUM * math.sqrt(M) * e1 + U * (abs(init) + ref.abs().max().item())
        check(f"{tag} {name}", got_.double() - init, ref.cpu(), bound)
    return code


# ---------------------------------------------------------------------------------------------------------------------------------
# weight gradient
# ---------------------------------------------------------------------------------------------------------------------------------
def _wgrad_ref64(kind, k, s, pad, a, b, CA, CB, dev):
    """dW in the parameter's layout ([CB][CA][k][k] for a convolution, [CA][CB][k][k] for a transposed one) of float64 NCHW a, b."""
    if kind == "conv_wgrad":
        pt, pl, pb, pr = _pads(pad)
        return torch.nn.grad.conv2d_weight(F.pad(a, (pl, pr, pt, pb)), (CB, CA, k, k), b, stride=s)
    return torch.nn.grad.conv2d_weight(b, (CA, CB, k, k), a, stride=s, padding=pad)


def _wgrad_case(be, row, f32=False, tune=None):
    old = {f: be.tune.get(f) for f in (tune or {})}
    be.tune.set(**(tune or {}))
    try:
        return _wgrad_case_tuned(be, row, f32)
    finally:
        be.tune.set(**old)


def _wgrad_case_tuned(be, row, f32):
    """cdf_conv_wgrad_bf16x (f32: the exact-fp32 cdf_conv_wgrad, for its split counts only) at a recorded shape and split count: every slab
    and bsum row finite after the poisoned launch (wholly empty trailing slabs included), the slabs' sum in the product's fixed order
    (cdf_unpack_reduce_bias) against float64."""
    kind, B, H, W, CA, CB, k, s, pad, nsplit, has_bsum, ns = row
    L, dev = be.L, be.device
    wp = wgrad_plan(kind, H, W, k, s, pad)
    KK, M, ldo = k * k, B * wp.QH * wp.QW, r4(CB)
    rnd = 16 if f32 else 32                                  # (the kernels round a slab's pixel count up to their K step)
    mps = -(-(-(-M // nsplit)) // rnd) * rnd
    empty = nsplit - -(-M // mps)
    tag = f"wgrad{'_f32' if f32 else ''} {kind} B={B} {wp.HA}x{wp.WA} {CA}x{CB} k{k}s{s} nsplit={nsplit} ({empty} empty slabs) bsum={has_bsum} NS={ns}"
    if not f32:
        code, tiles, grid = wgrad_form(L, row, be.tune.ptr)
        print(f"{tag}: form {decode(code)} tiles {tiles} grid {grid}")
    else:
        code = 0
    torch.manual_seed(CA + CB + nsplit)
    a, b = torch.randn(B, wp.HA, wp.WA, CA), torch.randn(B, wp.HB, wp.WB, CB)
    ad, bd = be.to(F.pad(a, (0, r4(CA) - CA))), be.to(F.pad(b, (0, r4(CB) - CB)))       # (fp32 feature maps have pitch roundup4(C), pad zero)
    zero = be.zeros(16)
    ws, bsum = nan_empty(be, nsplit, KK, CA, ldo), (nan_empty(be, nsplit, ldo) if has_bsum else None)
    conv = kind == "conv_wgrad"
    gw, gb = nan_empty(be, *((CB, CA, k, k) if conv else (CA, CB, k, k))), nan_empty(be, CB)
    s_r, s_c = (KK, CA * KK) if conv else (CB * KK, KK)
    if f32:
        as_, bs_ = (ad, None), (bd, None)
    else:
        as_, bs_ = _split(be, ad[..., :CA].contiguous(), ns == 1), _split(be, bd[..., :CB].contiguous(), ns == 1)

    def launch():
        if f32:
            L.cdf_conv_wgrad(P(ad), r4(CA), P(bd), r4(CB), P(ws), ldo, B, wp.QH, wp.QW, wp.HA, wp.WA, wp.sa, wp.HB, wp.WB, wp.sb, CA, CB, wp.ntaps, wp.desc,
                             nsplit, 1, 0, 0, 0, P(bsum), be.stream())
        else:
            L.cdf_conv_wgrad_bf16x(P(as_[0]), P(as_[1]), as_[0].shape[-1], P(bs_[0]), P(bs_[1]), bs_[0].shape[-1], P(zero), P(ws), ldo, B, wp.QH, wp.QW,
                                   wp.HA, wp.WA, wp.sa, wp.HB, wp.WB, wp.sb, CA, CB, wp.ntaps, wp.desc, nsplit, P(bsum), be.tune.ptr, be.stream())
        if has_bsum:
            L.cdf_unpack_reduce_bias(P(ws), P(gw), nsplit, KK, CA, CB, ldo, 1, s_r, s_c, P(bsum), P(gb), ldo, 0, 1, be.stream())
        else:
            L.cdf_unpack_reduce(P(ws), P(gw), nsplit, KK, CA, CB, ldo, 1, s_r, s_c, 0, 1, be.stream())
    outs = [ws, gw] + ([bsum, gb] if has_bsum else [])
    got = twice(launch, outs)
    assert torch.isfinite(got[0][..., :CB]).all(), (tag, "a slab was left unwritten")
    if has_bsum:
        assert torch.isfinite(got[2][:, :CB]).all(), (tag, "a bsum row was left unwritten")
    if empty:
        assert (got[0][nsplit - empty:, ..., :CB] == 0).all() and (not has_bsum or (got[2][nsplit - empty:, :CB] == 0).all()), (tag, "empty slabs")
    # float64 reference on the device, all images
    n64 = lambda t, C: _nchw(t.to(dev).double(), C)
    if f32:
        terms = [(n64(a, CA), n64(b, CB))]
    else:
        ah, bh = _nchw(_wide(as_[0], CA), CA), _nchw(_wide(bs_[0], CB), CB)
        terms = [(ah, bh)]
        if ns == 3:
            al, bl = _nchw(_wide(as_[1], CA), CA), _nchw(_wide(bs_[1], CB), CB)
            terms = [(ah, bh + bl), (al, bh)]
    ref = sum(_wgrad_ref64(kind, k, s, pad, p, q, CA, CB, dev) for p, q in terms)
    if f32 or ns == 1:
        sq = _wgrad_ref64(kind, k, s, pad, terms[0][0] ** 2, terms[0][1] ** 2, CA, CB, dev)
    else:
        sq = _wgrad_ref64(kind, k, s, pad, ah ** 2, bh ** 2 + bl ** 2, CA, CB, dev) + _wgrad_ref64(kind, k, s, pad, al ** 2, bh ** 2, CA, CB, dev)
    n = (1 if f32 else ns) * M
    bound = K_SUM * U * math.sqrt(n) * sq.max().sqrt().item()
    check(f"{tag} dW", got[1], ref.cpu(), bound)
    true = _wgrad_ref64(kind, k, s, pad, n64(a, CA), n64(b, CB), CA, CB, dev).cpu()
    tol = (3e-5 if (f32 or ns == 3) else 2e-2) * max(1.0, true.abs().max().item()) * math.sqrt(M / 16)
    check(f"{tag} dW against the true float64 gradient (the bound of test_kernels.py::_spx_case)", got[1], true, tol)
    if has_bsum:
        bsrc = n64(b, CB) if f32 else _nchw(_wide(bs_[0], CB) + (_wide(bs_[1], CB) if ns == 3 else 0), CB)
        t = bsrc.permute(1, 0, 2, 3).reshape(CB, -1)
        check(f"{tag} db", got[3], t.sum(1).cpu(), sum_bound(t, 1))
    return code


# ---------------------------------------------------------------------------------------------------------------------------------
# the tests
# ---------------------------------------------------------------------------------------------------------------------------------
def _hip():
    from conftest import Backend
    return Backend("hip")


@pytest.mark.gpu
@pytest.mark.parametrize("row", BENCH_GEMM, ids=lambda r: "-".join(map(str, r)))
def test_gemm_bench_forms(row):
    """Every (kernel form, NS, epilogue operand list) of the recordings at its recorded shape; the resident row-halo rows again with
    resident_reserve = 32 (224 blocks: an uneven number of tiles per block, the grid of every multi-rank step)."""
    be = _hip()
    code = _gemm_case(be, row)
    if decode(code)["form"] == ROWHALO:
        _, tiles, grid = gemm_form(be.L, row, be.tune.ptr)
        assert tiles > grid, "the resident kernel's rows must walk several tiles per block"
        _gemm_case(be, row, tune=dict(resident_reserve=32))


# Kernel instantiations of the device build that neither a recording (BENCH_GEMM) nor another hardware test launches (kernel trace of this
# module, test_kernels.py and test_kernels_production.py against the build's instantiation list): (row, tuning, (form, bm, bn, stages)), at the
# smallest batch that dispatches there -- width and channel counts are template parameters.  The resident kernel's rows take B = 5: 320 tiles
# on 256 blocks, an uneven walk.  Its 64-wide N tile is reached through cdf_gemm_tuning.halo bit 64 only.
UNRECORDED_GEMM = [
    *[(("gemm", "conv_fwd", 5, 128, 128, 128, 128, 3, 1, 1, 1, "b", 0, 0, 0, 0, 0, 1, 0, ns), None, (ROWHALO, 256, 128, 4)) for ns in (1, 3)],
    *[(("gemm", "conv_fwd", 5, 128, 128, cin, 64, 3, 1, 1, 1, "b", 0, 0, 0, 0, 0, 1, 0, ns), dict(halo=64 | 47), (ROWHALO, 256, 64, cin // 32))
      for cin in (64, 128) for ns in (1, 3)],
    *[(("gemm", "conv_fwd", 2, 128, 128, 64, 64, 1, 1, 0, 1, "b", 0, 0, 0, 0, 0, 1, 0, ns), None, (SPX, 64, 64, 2)) for ns in (1, 3)],
    (("gemm", "conv_fwd", 1, 32, 32, 64, 96, 3, 1, 1, 1, "b", 0, 0, 0, 0, 0, 1, 0, 1), None, (HALO, 128, 128, 6)),
]


@pytest.mark.gpu
@pytest.mark.parametrize("row,tune,form", UNRECORDED_GEMM, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_gemm_instances_no_recording_reaches(row, tune, form):
    d = decode(_gemm_case(_hip(), row, tune=dict(tune or {})))
    assert (d["form"], d["bm"], d["bn"], d["stages"]) == form


def test_bench_gemm_reaches_resident_blocks_with_several_tiles():
    """At least one BENCH_GEMM row is a resident row-halo launch whose blocks walk more than one tile (host-side query only)."""
    from colddiff import _lib
    L = _lib.get()
    hits = []
    for row in BENCH_GEMM:
        code, tiles, grid = gemm_form(L, row)
        if decode(code)["form"] == ROWHALO:
            print(row, "tiles", tiles, "grid", grid)
            hits.append(tiles > grid)
    assert any(hits)


def test_wgrad_row3_query_agrees_with_the_dispatcher(be):
    """cdf_conv_wgrad_bf16x_is_row3 -- asked the way ops.wgrad_into asks it, same_size_3x3 = the plan's own same3x3 -- against the form
    cdf_conv_wgrad_bf16x_form's dispatch takes, over the rows of both weight-gradient tables, with the row-of-taps kernel on and off, and at
    a few geometries on either side of each term of the test.  ops.wgrad_into sizes the split count by the query.  Host side: no launch."""
    L = be.L
    extra = [("conv_wgrad", 1, H, W, CA, CB, k, s, pad, 1, 0, 3)
             for (H, W, k, s, pad) in ((16, 16, 3, 1, 1), (6, 16, 3, 1, 1), (7, 16, 3, 1, 1), (5, 32, 3, 1, 1), (24, 24, 3, 1, 1), (16, 48, 3, 1, 1),
                                       (32, 32, 3, 2, 1), (32, 32, 1, 1, 0), (16, 16, 3, 1, 0), (256, 256, 3, 1, 1))
             for (CA, CB) in ((64, 64), (64, 128), (128, 64), (136, 136))]
    extra += [("convT_wgrad", 1, 16, 16, 128, 128, 4, 2, 1, 1, 0, 3)]
    seen = set()
    for row in BENCH_WGRAD + EMU_WGRAD + extra:
        kind, B, H, W, CA, CB, k, s, pad = row[:9]
        wp = wgrad_plan(kind, H, W, k, s, pad)
        for on in (1, 0):
            old = be.tune.get("wgrad_row3")
            be.tune.set(wgrad_row3=on)
            try:
                q = L.cdf_conv_wgrad_bf16x_is_row3(wp.QH, wp.QW, CA, CB, wp.ntaps, 1 if wp.same3x3 else 0, be.tune.ptr)
                form = decode(wgrad_form(L, row, be.tune.ptr)[0])["form"]
            finally:
                be.tune.set(wgrad_row3=old)
            assert (q != 0) == (form == 1), (row, on, q, form)
            seen.add((on, form == 1))
    assert seen == {(1, True), (1, False), (0, False)}


@pytest.mark.gpu
@pytest.mark.parametrize("row", BENCH_WGRAD, ids=lambda r: "-".join(map(str, r)))
def test_wgrad_bench_forms_and_split_counts(row):
    _wgrad_case(_hip(), row)


@pytest.mark.gpu
def test_wgrad_stacked_two_tap_form():
    """conv_wgrad_spx_kernel's stacked form (two taps per 128-row tile, CA <= 64 < CB): the recordings never reach it -- the row-of-taps
    kernel takes its layers -- so it runs at the 64 -> 128 layer of the 128 x 128 level with wgrad_row3 = 0, at the split count
    ops.wgrad_into's expressions give it there (5 tap blocks of one tile on 512 slots)."""
    from colddiff import ops
    be = _hip()
    M = 64 * 128 * 128
    ns = ops.best_nsplit(1 * 1 * 5, 512, M // 512)
    code = _wgrad_case(be, ("conv_wgrad", 64, 128, 128, 64, 128, 3, 1, 1, ns, 1, 3), tune=dict(wgrad_row3=0))
    assert decode(code)["form"] == 3


@pytest.mark.gpu
@pytest.mark.parametrize("row", [("conv_wgrad", 64, 128, 128, 64, 3, 1, 1, 0, 995, 1, 3), ("conv_wgrad", 64, 64, 64, 64, 128, 1, 1, 0, 995, 1, 3)],
                         ids=lambda r: "-".join(map(str, r)))
def test_wgrad_f32_995_slabs_two_empty(row):
    """cdf_conv_wgrad at the 995 slabs ops.best_nsplit gives the bench step's one-tile 1 x 1 layers (recorded): at M = 1,048,576
    m_per_split = 1056, so slabs 993 and 994 get no pixels; at M = 262,144 it is 272 and the last 31 slabs get none -- and each must
    still be written (zeros), with its bsum row."""
    _wgrad_case(_hip(), row, f32=True)


# simulator companions: small shapes, both backends -- each kernel form through the three-product float64 reference and the K_SUM bound
EMU_GEMM = [
    # (row, tuning): the forced-tile shapes of test_conv_presplit_forced_tiles (ragged M and N tiles) ...
    *[(("gemm", "conv_fwd", 3, 7, 7, 40, 72, 3, 1, 1, 1, "b", 0, 0, 0, 0, 0, 1, 0, ns), dict(tile_bm=bm, tile_bn=bn))
      for (bm, bn) in ((256, 128), (128, 128), (128, 64), (64, 128), (64, 64)) for ns in (3, 1)],
    # ... the LDS-resident-input kernel at both tile heights (test_conv_presplit_halo), data-gradient taps too
    (("gemm", "conv_fwd", 1, 16, 16, 64, 96, 3, 1, 1, 1, "b", 1, 0, 0, 0, 2, 1, 0, 3), dict(halo=31, halo_bm=128)),
    (("gemm", "conv_dgrad", 2, 16, 16, 96, 40, 3, 1, 1, 1, "", 0, 0, 0, 0, 0, 1, 0, 3), dict(halo=31, halo_bm=256)),
    (("gemm", "conv_fwd", 1, 32, 32, 64, 72, 3, 1, 1, 1, "br", 0, 0, 0, 0, 0, 1, 0, 1), dict(halo=31, halo_bm=256)),
    # ... the resident row-halo kernel with several tiles per block (test_conv_presplit_rowhalo_emu / _resident_reserve_emu)
    (("gemm", "conv_fwd", 5, 16, 16, 64, 136, 3, 1, 1, 1, "b", 0, 0, 0, 0, 0, 1, 0, 3), dict(halo=64 | 47)),
    (("gemm", "conv_dgrad", 9, 16, 16, 128, 40, 3, 1, 1, 1, "", 0, 0, 0, 0, 0, 1, 0, 3), dict(halo=64 | 47, resident_reserve=5)),
    (("gemm", "conv_fwd", 5, 16, 16, 64, 136, 3, 1, 1, 1, "bm", 0, 1, 0, 0, 1, 1, 0, 1), dict(halo=64 | 47, resident_reserve=32)),
    # ... split-K over the taps + the finish kernel, strided and transposed layers, the LayerNorm-backward epilogue
    (("gemm", "conv_fwd", 2, 4, 4, 64, 72, 3, 1, 1, 1, "bs", 2, 0, 0, 0, 0, 1, 1, 3), None),
    (("gemm", "conv_fwd", 1, 32, 32, 32, 32, 4, 2, 1, 1, "b", 0, 0, 0, 0, 0, 1, 0, 3), None),
    (("gemm", "convT_fwd", 1, 8, 8, 32, 40, 4, 2, 1, 4, "b", 0, 0, 0, 0, 0, 1, 0, 3), None),
    (("gemm", "conv_fwd", 1, 16, 16, 64, 64, 3, 1, 1, 1, "b", 0, 0, 1, 0, 0, 1, 0, 3), None),
    (("lnbwd", "conv_dgrad", 2, 16, 16, 128, 64, 3, 1, 1, 1, "", 0, 0, 0, 0, 0, 1, 0, 3), None),
]


@pytest.mark.parametrize("row,tune", EMU_GEMM, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_gemm_forms_small(be, row, tune):
    tune = dict(tune or {})
    code = _gemm_case(be, row, tune=tune)
    d = decode(code)
    if "tile_bm" in tune:
        assert (d["form"], d["bm"], d["bn"]) == (SPX, tune["tile_bm"], tune["tile_bn"])
    if tune.get("halo", 0) & 64:
        # (the device build carries the resident kernel at width 128 only -- test_gemm_bench_forms runs it there -- and hands these
        #  16-pixel-wide layers to the LDS-resident-input kernel)
        assert d["form"] == (ROWHALO if be.kind == "emu" else HALO)
    elif "halo_bm" in tune:
        assert (d["form"], d["bm"]) == (HALO, tune["halo_bm"])
    if row[18]:
        assert d["ksplit"] > 1


EMU_WGRAD = [
    # wholly empty trailing slabs: M = 1152 in 33 slabs -> m_per_split = 64, 18 slabs with pixels, 15 without (both kernels, + stacked taps)
    ("conv_wgrad", 2, 24, 24, 72, 40, 3, 1, 1, 33, 1, 3),        # per-tap kernel (24-wide rows)
    ("conv_wgrad", 1, 32, 32, 136, 40, 3, 1, 1, 31, 1, 3),       # row-of-taps kernel: M = 1024, m_per_split = 64, 16 slabs with pixels
    ("conv_wgrad", 1, 24, 24, 40, 136, 3, 1, 1, 7, 1, 1),        # stacked two-tap form (CA <= 64 < CB), hi-only planes
    ("conv_wgrad", 1, 16, 16, 64, 64, 4, 2, 1, 3, 0, 3),
    ("convT_wgrad", 1, 8, 8, 72, 40, 4, 2, 1, 2, 0, 3),
    # the pixel walk of the per-tap kernel on 4 x 4 images: one 32-pixel step is eight image rows and two images.  B = 3 (M = 48) in three
    # slabs of 32 | 16 | none: every slab is a single step, the decode alone places its pixels (at M = 48 a slab of two steps, 64 pixels,
    # leaves no split without pixels: a split count <= 1).  B = 7 (M = 112) in three slabs of 64 | 48 | none: the second step of either
    # slab comes out of the advance, which carries over several rows and over an image boundary
    ("conv_wgrad", 3, 4, 4, 72, 40, 3, 1, 1, 3, 1, 3),
    ("conv_wgrad", 7, 4, 4, 72, 40, 3, 1, 1, 3, 1, 3),
]


@pytest.mark.parametrize("row", EMU_WGRAD, ids=lambda r: "-".join(map(str, r)))
def test_wgrad_forms_small(be, row):
    _wgrad_case(be, row)


def test_wgrad_f32_empty_trailing_slabs_small(be):
    """cdf_conv_wgrad with slabs that get no pixels (the 995-slab launch of the bench step, at a simulator-sized M)."""
    _wgrad_case(be, ("conv_wgrad", 1, 24, 24, 8, 16, 1, 1, 0, 13, 1, 3), f32=True)
