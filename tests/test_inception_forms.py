"""The conv GEMM launches of the FID feature extractor (colddiff/inception.py: 94 BasicConv2d layers, every FID / KID / PRDC number goes
through them) in every form the extractor reaches, on its three paths: cdf_conv_gemm_bf16 (conv_igemm_sp_kernel<3>, the layers with
K >= 64 and Cout >= 64 in the default mode), cdf_conv_gemm in the default mode (the stem and the 32- / 48-channel branches) and
cdf_conv_gemm in f32 mode (every layer).  What the extractor asks of these kernels and the U-Net never does: the folded-BatchNorm bias with
the ReLU epilogue (act = 3); 1 x 7, 7 x 1, 1 x 3 and 3 x 1 tap sets; 3 x 3 stride 2 without padding on odd images; the 5 x 5 layers as a
16-tap launch and an accumulating 9-tap launch over one 25-tap packed weight, ReLU afterwards (cdf_act_fwd); Cin = 3 (pitch 4), 48, 80;
Cout = 32, 48, 80, 96, 160, 320, 448; every branch writing its channel slice of the block's concatenated output.

Conventions of test_gemm_sp_forms.py / test_gemm_f32_forms.py / test_gemm_production.py, whose case functions run the rows here
(_sp_gemm_case, _igemm_case): every output NaN-poisoned before each of two launches that must agree bit for bit; the float64 reference
on the operands the kernel multiplies (the packed bf16 planes read back, the in-kernel activation split restated in integer ops; the
exact-fp32 kernel's operands as they are); the columns on both sides of a sliced y must still hold the poison bit pattern; the in-quad
pad channel of the 3-channel stem holds 1e30.  A tap-subset row (test_gemm_production.TapSubset) packs all 25 taps and its reference is
the convolution with the absent taps' weights set to zero; the 5 x 5 pair (_pair_case) runs the three launches of BasicConv2d.run and
ends with ReLU.

Bounds, no new constant: first assertion, fp32 accumulation only -- K_SUM 2^-24 sqrt(n) max ||terms||_2, n = NS x taps x Cin, plus the
epilogue lines of test_gemm_production._epilogue64 (bias: one rounding; ReLU: Lipschitz 1); the pair adds the first launch's bound to the
second's (the second accumulates onto the first's output) and cdf_act_fwd's ReLU is exact.  Second assertion (split path): the distance
to the true float64 convolution of the unsplit operands within 3e-5 max(1, |ref|max), and -- on the CPU, whatever the kernel does -- the
float64 sum of the split operands alone within half of that, or the row's inputs are wrong.  On the exact-fp32 path the operands are
not split and the first reference is the true one.

Shapes are the smallest that contain the hazard (FORM rows: one per reached form, so that a form cannot lose its only test silently;
HAZARD rows: what a form does not tell -- H != W with at least 9 pixels along a 7-tap direction, so that columns 3 .. 5 have all seven
taps inside and 0 .. 2 / 6 .. 8 lose 1 to 3; windows of the stride-2 layers ending exactly on the last row and column; one, several and
ragged 128-row tiles per geometry; the extractor's own 8 x 8 stage at B = 1 and B = 2; slices at the column residues the blocks
produce (32 mod 64, 64 mod 128, 0) and at FIDInceptionE's own offsets 0 / 320 / 704 / 1088 / 1472 / 1856 of 2048), and PROD rows
(gpu): one per reached form at a shape of the recording with B = 1 or 2, the largest 147 x 147, 32 -> 64, 3 x 3.

Recording (extractor_calls): one forward of InceptionV3([0, 1, 2, 3], resize_input=True) on 64 x 64 images at B = 50 (the metrics'
default batch) and B = 1, in bf16x3 (the default), bf16 (which the extractor runs as bf16x3: asserted) and f32.  It reaches, by
sp_gemm_form / f32_gemm_form of the recorded arguments:
    default / bf16   cdf_conv_gemm_bf16   27 forms at B = 50, 24 at B = 1, 31 together (M = B OH OW is whole at the 8 x 8 stage for even B only)
    default / bf16   cdf_conv_gemm        4 forms (stem 3 -> 32 stride 2, 32 -> 32, the 32- and 48-channel 1 x 1 branches)
    f32              cdf_conv_gemm        15 forms (the four above among them)
test_recorded_extractor_forms_dry makes the recording without a GPU (launches stubbed out);
test_gpu_invariance.py::test_coverage_guard makes it on the MI355X.  Both hold: every recorded form has a FORM row and a PROD row, every
form flagged as reached (REACHED_*) is recorded.

Worst error / bound per group (61 + 40 FORM and HAZARD rows and 6 pairs on both backends: 37 s on the simulator in one process, a
second on the MI355X; 31 + 15 PROD rows, MI355X, 0.11 s at most each).  The simulator column is a run of the kernel sources on the host
simulator, not a measurement of the kernel:
                                                              simulator      MI355X
    split path   y (bias + ReLU, tap subsets)                 0.40           0.19
                 true float64 convolution                     0.39 of 3e-5 max (the split operands alone: 0.79 of half of it), both backends
                 5 x 5 pair: pre-activation / ReLU output     0.26 / 0.22    0.16 / 0.16
    exact fp32   y                                            0.44           0.44
                 5 x 5 pair: pre-activation / ReLU output     0.40 / 0.32    0.40 / 0.32
    production shapes (MI355X)   split path y 0.24, true convolution 0.41 of 3e-5 max (the split alone 0.82 of half);   exact fp32 y 0.62
As in the sibling modules the exact-fp32 columns agree because the results do, and the matrix core's split sums are closer to float64
than the simulator's one-by-one fp32 additions.  No row of this module has failed on either backend.
"""
import ctypes
import math

import pytest
import torch

from poison import nan_empty
from test_kernels import P, r4
from test_kernels_production import K_SUM, U, check, twice
from test_gemm_production import TapSubset, _conv64, _epilogue64, _hip, _nchw, _weights, gemm_plan, tap_mask
import test_gemm_sp_forms as sf
import test_gemm_f32_forms as ff

ACT_RELU = 3
T16, T9 = TapSubset(5, 5, 0, 16), TapSubset(5, 5, 16, 25)     # the two launches colddiff.inception._tap_parts cuts a 5 x 5 layer into
SPLIT_MARGIN = 0.5                                           # the split operands alone: within half of the second assertion's tolerance


def S(B, H, W, cin, cout, k, s, pad, ops="b", act=ACT_RELU, acc=0, yld=0, yoff=0):
    """A cdf_conv_gemm_bf16 row (split = 3) the way BasicConv2d.run launches: x contiguous, y contiguous or a slice."""
    return sf.GS("conv_fwd", B, H, W, cin, cout, k, s, pad, ops, act, 0, acc, 0, 0, yld, yoff)


def F(B, H, W, cin, cout, k, s, pad, ops="b", act=ACT_RELU, acc=0, yld=0, yoff=0):
    """A cdf_conv_gemm row; the 3-channel image lies in a pitch-4 buffer (its pad channel: 1e30, test_gemm_f32_forms._padded)."""
    return ff.GR("conv_fwd", B, H, W, cin, cout, k, s, pad, ops, act, 0, acc, 0, 0, 1, r4(cin) if cin % 4 else 0, 0, yld, yoff)


# ---------------------------------------------------------------------------------------------------------------------------------
# the forms the recording reaches (regenerate: the listing test_recorded_extractor_forms_dry prints)
# ---------------------------------------------------------------------------------------------------------------------------------
_V = lambda geom, ops, act, acc, m, n, kt, yp: (3, geom, "vec", ops, act, 0, acc, m, n, kt, 0, yp, 0)
_1x7, _7x1, _1x3, _3x1 = (1, 7, 1, 1, 0, -3), (1, 7, 1, 1, -3, 0), (1, 3, 1, 1, 0, -1), (1, 3, 1, 1, -1, 0)
_P1, _P0, _S2, _G16, _G9 = (1, 9, 1, 1, -1, -1), (1, 9, 1, 1, 0, 0), (1, 9, 1, 2, 0, 0), (1, 16, 1, 1, -2, -2), (1, 9, 1, 1, 1, -1)
REACHED_SP_B50 = {
    *[_V("1tap", "b", 3, 0, m, n, 0, yp) for m, n, yp in (("ragged", "half", 0), ("ragged", "half", 1), ("ragged", "ragged", 0), ("ragged", "whole", 0),
                                                           ("whole", "half", 0), ("whole", "half", 1), ("whole", "whole", 0))],
    _V(_G16, "b", 0, 0, "ragged", "half", 1, 0), _V(_G9, "", 0, 1, "ragged", "half", 1, 0),
    _V(_3x1, "b", 3, 0, "whole", "whole", 0, 1), _V(_1x3, "b", 3, 0, "whole", "whole", 0, 1),
    *[_V(g, "b", 3, 0, "ragged", n, 0, yp) for g in (_7x1, _1x7) for n, yp in (("half", 0), ("half", 1), ("ragged", 0), ("whole", 0))],
    _V(_P1, "b", 3, 0, "ragged", "half", 0, 0), _V(_P1, "b", 3, 0, "ragged", "ragged", 0, 0), _V(_P1, "b", 3, 0, "ragged", "ragged", 0, 1),
    _V(_P1, "b", 3, 0, "whole", "whole", 0, 0), _V(_P0, "b", 3, 0, "ragged", "half", 1, 0),
    _V(_S2, "b", 3, 0, "ragged", "ragged", 0, 1), _V(_S2, "b", 3, 0, "ragged", "whole", 0, 1), _V(_S2, "b", 3, 0, "whole", "half", 0, 1),
}
REACHED_SP_B1 = {f for f in REACHED_SP_B50 if f[7] == "ragged"} | {
    _V(_3x1, "b", 3, 0, "ragged", "whole", 0, 1), _V(_1x3, "b", 3, 0, "ragged", "whole", 0, 1), _V(_P1, "b", 3, 0, "ragged", "whole", 0, 0),
    _V(_S2, "b", 3, 0, "ragged", "half", 0, 1)}
REACHED_SP = REACHED_SP_B50 | REACHED_SP_B1
_W = lambda tile, geom, ops="b", act=3, acc=0: (tile, 0, geom, "none", "", 0, ops, act, 0, acc, 1, 0, 1, 0)
REACHED_F32_DEFAULT = {_W("128x32", "1tap"), _W("128x32", _P0), _W("128x32", _S2), _W("256x64", "1tap")}
REACHED_F32 = REACHED_F32_DEFAULT | {
    *[_W("128x128", g) for g in ("1tap", _3x1, _1x3, _7x1, _1x7, _P1, _P0, _S2)],
    _W("256x64", _P1), _W("256x64", _G16, "b", 0), _W("256x64", _G9, "", 0, 1)}


# ---------------------------------------------------------------------------------------------------------------------------------
# rows.  FORM: one per reached form at the smallest shape with the hazard;  HAZARD: see the module docstring;  PROD: recorded shapes
# ---------------------------------------------------------------------------------------------------------------------------------
SP_FORM_ROWS = [
    # 1 x 1: M = 45 / 90 (ragged), 128 and 256 (whole); Cout 192, 64, 448, 320 half, 80 ragged, 128 whole; the slices of FIDInceptionA / E
    S(1, 5, 9, 96, 192, 1, 1, 0), S(1, 5, 9, 64, 64, 1, 1, 0, yld=256, yoff=64), S(1, 9, 5, 64, 80, 1, 1, 0), S(2, 5, 9, 32, 128, 1, 1, 0),
    S(2, 8, 8, 64, 448, 1, 1, 0), S(2, 8, 8, 96, 192, 1, 1, 0, yld=2048, yoff=1856), S(4, 8, 8, 64, 128, 1, 1, 0),
    # the 5 x 5 layer's two launches, each alone: Cin = 48 (a K tail of 16 inside ldk = 64), 6 x 7 with pad 2 -- every one of the 25 taps
    # is outside the image for some pixel and inside for another
    S(1, 6, 7, 48, 64, T16, 1, 2, "b", 0), S(1, 6, 7, 48, 64, T9, 1, 2, "", 0, 1),
    # 3 x 1 and 1 x 3 into slices: the 8 x 8 stage's whole tile at even B as a non-square map (4 x 16, 16 x 4), a ragged one
    S(2, 16, 4, 64, 128, (3, 1), 1, (1, 0), yld=288, yoff=32), S(2, 4, 16, 96, 128, (1, 3), 1, (0, 1), yld=256, yoff=64),
    S(1, 9, 5, 96, 128, (3, 1), 1, (1, 0), yld=256, yoff=64), S(1, 5, 9, 64, 128, (1, 3), 1, (0, 1), yld=256, yoff=0),
    # 7 x 1 on 9 x 5, 1 x 7 on 5 x 9: Cin 32 / 64 / 96 (1, 2, 3 K steps per tap: both parities of the lookahead), Cout half / ragged / whole
    S(1, 9, 5, 64, 192, (7, 1), 1, (3, 0)), S(2, 9, 5, 32, 192, (7, 1), 1, (3, 0), yld=768, yoff=192), S(1, 9, 5, 96, 160, (7, 1), 1, (3, 0)),
    S(2, 9, 5, 64, 128, (7, 1), 1, (3, 0)),
    S(1, 5, 9, 96, 192, (1, 7), 1, (0, 3)), S(2, 5, 9, 64, 192, (1, 7), 1, (0, 3), yld=768, yoff=384), S(1, 5, 9, 32, 160, (1, 7), 1, (0, 3)),
    S(2, 5, 9, 96, 128, (1, 7), 1, (0, 3)),
    # 3 x 3 with padding; the 8 x 8 stage at B = 1 (ragged: 64 rows) and B = 2 (one whole tile)
    S(1, 9, 7, 32, 64, 3, 1, 1), S(1, 9, 7, 64, 96, 3, 1, 1), S(1, 7, 9, 96, 96, 3, 1, 1, yld=256, yoff=128), S(1, 8, 8, 64, 128, 3, 1, 1),
    S(2, 8, 8, 64, 128, 3, 1, 1),
    # 3 x 3 without padding: 9 x 7 -> 7 x 5, Cin = 80 (a K tail of 16 inside ldk = 96)
    S(1, 9, 7, 80, 192, 3, 1, 0),
    # 3 x 3 stride 2 without padding on odd sizes: 9 x 7 -> 4 x 3, 7 x 9 -> 3 x 4, 17 x 9 -> 8 x 4 (B = 4: M = 128); the last window ends on
    # the last row and column; into the slices of InceptionB (768) and InceptionD (1280)
    S(1, 9, 7, 64, 192, 3, 2, 0, yld=1280, yoff=320), S(1, 7, 9, 96, 96, 3, 2, 0, yld=768, yoff=384), S(2, 9, 7, 32, 128, 3, 2, 0, yld=768, yoff=0),
    S(4, 17, 9, 64, 192, 3, 2, 0, yld=1280, yoff=320),
]
SP_HAZARD_ROWS = [
    # FIDInceptionE's own slices: offsets 0 / 320 / 704 / 1088 / 1472 / 1856 of 2048, at the 8 x 8 stage with B = 1 (ragged) and B = 2 (whole)
    S(2, 8, 8, 32, 320, 1, 1, 0, yld=2048, yoff=0), S(1, 8, 8, 64, 384, (1, 3), 1, (0, 1), yld=2048, yoff=320),
    S(2, 8, 8, 32, 384, (3, 1), 1, (1, 0), yld=2048, yoff=704), S(2, 8, 8, 64, 384, (1, 3), 1, (0, 1), yld=2048, yoff=1088),
    S(1, 8, 8, 32, 384, (3, 1), 1, (1, 0), yld=2048, yoff=1472), S(1, 8, 8, 64, 192, 1, 1, 0, yld=2048, yoff=1856),
    # 7 taps over one whole tile (8 x 16, 16 x 8), two whole tiles, and a whole tile followed by 7 rows (B = 3: M = 135)
    S(1, 8, 16, 64, 192, (1, 7), 1, (0, 3)), S(1, 16, 8, 96, 160, (7, 1), 1, (3, 0)), S(2, 8, 16, 32, 128, (1, 7), 1, (0, 3), yld=768, yoff=576),
    S(2, 16, 8, 32, 192, (7, 1), 1, (3, 0), yld=768, yoff=192), S(3, 5, 9, 64, 160, (1, 7), 1, (0, 3)), S(3, 9, 5, 64, 192, (7, 1), 1, (3, 0)),
    # stride 2 in the other orientation, the extractor's own 17 x 17 -> 8 x 8 at B = 2 (whole) and B = 3 (a whole tile and a half)
    S(1, 7, 9, 64, 192, 3, 2, 0, yld=1280, yoff=0), S(2, 17, 17, 32, 320, 3, 2, 0, yld=1280, yoff=0), S(3, 17, 17, 32, 192, 3, 2, 0, yld=1280, yoff=320),
    # 3 x 3 without padding in the other orientation and over several tiles (B = 4: M = 140)
    S(1, 7, 9, 80, 192, 3, 1, 0), S(4, 9, 7, 48, 192, 3, 1, 0),
    # FIDInceptionA's slices (0 / 64 / 128 of 256; the 32-wide one at 224 is the exact-fp32 kernel's), 1 x 1 with Cin = 80 and Cout = 80
    S(1, 5, 9, 64, 64, 1, 1, 0, yld=256, yoff=0), S(3, 9, 7, 64, 96, 3, 1, 1, yld=256, yoff=128), S(1, 9, 7, 80, 80, 1, 1, 0),
    # two whole tiles (M = 256) for the tap sets that have none above; 3 x 3 without padding on 10 x 10 -> 8 x 8 (M = 128, 256); the 5 x 5
    # part launches over one whole tile (8 x 16) and two (16 x 8, B = 2)
    S(4, 4, 16, 32, 128, (1, 3), 1, (0, 1), yld=256, yoff=64), S(4, 16, 4, 32, 128, (3, 1), 1, (1, 0), yld=288, yoff=32), S(4, 8, 8, 32, 128, 3, 1, 1),
    S(2, 10, 10, 48, 192, 3, 1, 0), S(4, 10, 10, 32, 64, 3, 1, 0), S(4, 17, 17, 32, 128, 3, 2, 0, yld=768, yoff=0),
    S(1, 8, 16, 48, 64, T16, 1, 2, "b", 0), S(2, 16, 8, 48, 64, T16, 1, 2, "b", 0), S(1, 8, 16, 48, 64, T9, 1, 2, "", 0, 1),
    S(2, 16, 8, 48, 64, T9, 1, 2, "", 0, 1),
]
F32_FORM_ROWS = [
    # <128,128>: every geometry; Cin = 80 (16 + 16 + ... the K-chunk wrap), Cout 80 / 96 / 160 ragged
    F(1, 5, 9, 64, 80, 1, 1, 0), F(1, 9, 5, 32, 128, (3, 1), 1, (1, 0), yld=256, yoff=64), F(2, 4, 16, 64, 128, (1, 3), 1, (0, 1), yld=256, yoff=0),
    F(1, 9, 5, 96, 160, (7, 1), 1, (3, 0)), F(1, 5, 9, 64, 192, (1, 7), 1, (0, 3), yld=768, yoff=384), F(1, 9, 7, 64, 96, 3, 1, 1),
    F(1, 9, 7, 80, 192, 3, 1, 0), F(1, 7, 9, 96, 96, 3, 2, 0, yld=768, yoff=384),
    # <128,32>: the stem -- Cin = 3 in a pitch-4 buffer, stride 2 without padding; 32 -> 32 without padding; the 32-wide slice at 224 of 256
    F(1, 5, 9, 64, 32, 1, 1, 0, yld=256, yoff=224), F(1, 9, 7, 32, 32, 3, 1, 0), F(2, 9, 7, 3, 32, 3, 2, 0),
    # <256,64>: Cout = 48, the padded 3 x 3 of the stem, the 5 x 5 layer's two launches
    F(1, 5, 9, 64, 48, 1, 1, 0), F(1, 9, 7, 32, 64, 3, 1, 1), F(1, 6, 7, 48, 64, T16, 1, 2, "b", 0), F(1, 6, 7, 48, 64, T9, 1, 2, "", 0, 1),
]
F32_HAZARD_ROWS = [
    # the stem in the other orientation and over several 128-row tiles (17 x 17 -> 8 x 8, B = 3: M = 192), 32 -> 32 over two tiles
    F(1, 7, 9, 3, 32, 3, 2, 0), F(3, 17, 17, 3, 32, 3, 2, 0), F(2, 10, 10, 32, 32, 3, 1, 0),
    # <256,64> with M = 256 (one whole tile) and 320; <128,128> with one whole tile, two, and ragged ones, 7 taps
    F(4, 8, 8, 32, 48, 1, 1, 0), F(5, 8, 8, 32, 64, 3, 1, 1), F(1, 8, 16, 64, 192, (1, 7), 1, (0, 3)), F(2, 16, 8, 32, 128, (7, 1), 1, (3, 0)),
    F(2, 8, 16, 96, 128, (1, 7), 1, (0, 3)), F(1, 16, 8, 64, 160, (7, 1), 1, (3, 0)),
    F(3, 5, 9, 32, 160, (1, 7), 1, (0, 3)), F(3, 9, 5, 64, 192, (7, 1), 1, (3, 0), yld=768, yoff=192),
    # stride 2: 9 x 7 -> 4 x 3, 17 x 9 -> 8 x 4 (B = 4: M = 128), the extractor's 17 x 17 -> 8 x 8 into InceptionD's slices
    F(1, 9, 7, 64, 192, 3, 2, 0, yld=1280, yoff=320), F(4, 17, 9, 32, 128, 3, 2, 0, yld=768, yoff=0), F(2, 17, 17, 32, 320, 3, 2, 0, yld=1280, yoff=0),
    # FIDInceptionE's own slices in f32 mode, at the 8 x 8 stage with B = 1 and B = 2
    F(2, 8, 8, 32, 320, 1, 1, 0, yld=2048, yoff=0), F(1, 8, 8, 64, 384, (1, 3), 1, (0, 1), yld=2048, yoff=320),
    F(2, 8, 8, 32, 384, (3, 1), 1, (1, 0), yld=2048, yoff=704), F(1, 8, 8, 32, 384, (1, 3), 1, (0, 1), yld=2048, yoff=1088),
    F(2, 8, 8, 32, 384, (3, 1), 1, (1, 0), yld=2048, yoff=1472), F(1, 8, 8, 64, 192, 1, 1, 0, yld=2048, yoff=1856),
    F(1, 7, 9, 80, 192, 3, 1, 0), F(1, 9, 7, 80, 448, 1, 1, 0),
    # the padded 3 x 3 over one whole 128-row tile, the 5 x 5 part launches over one whole 256-row tile (B = 2, 8 x 16)
    F(2, 8, 8, 32, 96, 3, 1, 1), F(2, 8, 16, 48, 64, T16, 1, 2, "b", 0), F(2, 16, 8, 48, 64, T9, 1, 2, "", 0, 1),
]
# the 5 x 5 layer as BasicConv2d.run launches it: (path, B, H, W, Cin, Cout, pitch and column offset of the block's output)
PAIR_ROWS = [("sp", 1, 6, 7, 48, 64, 256, 64), ("sp", 3, 7, 6, 48, 64, 288, 64), ("sp", 2, 8, 16, 48, 64, 256, 64),
             ("f32", 1, 6, 7, 48, 64, 256, 64), ("f32", 7, 7, 6, 48, 64, 288, 64), ("f32", 2, 8, 16, 48, 64, 256, 64)]
# recorded shapes, B = 1 or 2 (whichever keeps the form's M class): one row per reached form
SP_PROD_ROWS = [
    S(1, 35, 35, 192, 64, 1, 1, 0), S(1, 35, 35, 192, 64, 1, 1, 0, yld=256, yoff=0), S(1, 73, 73, 64, 80, 1, 1, 0), S(1, 17, 17, 768, 128, 1, 1, 0),
    S(2, 8, 8, 1280, 448, 1, 1, 0), S(2, 8, 8, 1280, 192, 1, 1, 0, yld=2048, yoff=1856), S(2, 8, 8, 1280, 384, 1, 1, 0),
    S(1, 35, 35, 48, 64, T16, 1, 2, "b", 0), S(1, 35, 35, 48, 64, T9, 1, 2, "", 0, 1),
    S(1, 8, 8, 384, 384, (3, 1), 1, (1, 0), yld=2048, yoff=704), S(2, 8, 8, 384, 384, (3, 1), 1, (1, 0), yld=2048, yoff=704),
    S(1, 8, 8, 384, 384, (1, 3), 1, (0, 1), yld=2048, yoff=320), S(2, 8, 8, 384, 384, (1, 3), 1, (0, 1), yld=2048, yoff=320),
    S(1, 17, 17, 192, 192, (7, 1), 1, (3, 0)), S(1, 17, 17, 128, 192, (7, 1), 1, (3, 0), yld=768, yoff=192), S(1, 17, 17, 160, 160, (7, 1), 1, (3, 0)),
    S(1, 17, 17, 128, 128, (7, 1), 1, (3, 0)),
    S(1, 17, 17, 192, 192, (1, 7), 1, (0, 3)), S(1, 17, 17, 128, 192, (1, 7), 1, (0, 3), yld=768, yoff=384), S(1, 17, 17, 160, 160, (1, 7), 1, (0, 3)),
    S(1, 17, 17, 128, 128, (1, 7), 1, (0, 3)),
    S(1, 147, 147, 32, 64, 3, 1, 1), S(1, 35, 35, 64, 96, 3, 1, 1), S(1, 35, 35, 96, 96, 3, 1, 1, yld=256, yoff=128), S(1, 8, 8, 448, 384, 3, 1, 1),
    S(2, 8, 8, 448, 384, 3, 1, 1), S(1, 73, 73, 80, 192, 3, 1, 0),
    S(1, 17, 17, 192, 192, 3, 2, 0, yld=1280, yoff=320), S(1, 35, 35, 96, 96, 3, 2, 0, yld=768, yoff=384), S(1, 35, 35, 288, 384, 3, 2, 0, yld=768, yoff=0),
    S(2, 17, 17, 192, 192, 3, 2, 0, yld=1280, yoff=320),
]
F32_PROD_ROWS = [
    F(1, 8, 8, 1280, 192, 1, 1, 0, yld=2048, yoff=1856), F(1, 8, 8, 384, 384, (3, 1), 1, (1, 0), yld=2048, yoff=704),
    F(1, 8, 8, 384, 384, (1, 3), 1, (0, 1), yld=2048, yoff=320), F(1, 17, 17, 128, 128, (7, 1), 1, (3, 0)), F(1, 17, 17, 128, 128, (1, 7), 1, (0, 3)),
    F(1, 35, 35, 64, 96, 3, 1, 1), F(1, 73, 73, 80, 192, 3, 1, 0), F(1, 17, 17, 192, 192, 3, 2, 0, yld=1280, yoff=320),
    F(1, 35, 35, 192, 32, 1, 1, 0, yld=256, yoff=224), F(1, 149, 149, 32, 32, 3, 1, 0), F(1, 299, 299, 3, 32, 3, 2, 0), F(1, 35, 35, 192, 48, 1, 1, 0),
    F(1, 35, 35, 48, 64, T16, 1, 2, "b", 0), F(1, 147, 147, 32, 64, 3, 1, 1), F(1, 35, 35, 48, 64, T9, 1, 2, "", 0, 1),
]
_rid = lambda r: "-".join(str(v).replace(" ", "") for v in r)


def sp_forms(rows):
    return {sf.sp_gemm_form(sf.gs_args(r)) for r in rows}


def f32_forms(rows):
    return {ff.f32_gemm_form(*ff.gr_args(r)) for r in rows}


def test_form_tables():
    """The tables keep what they were built for.  FORM and PROD rows: exactly one row per reached form (a row taken out leaves its form
    without a test, and test_recorded_extractor_forms_dry names it).  Every row but the 5 x 5 part launches carries bias + ReLU.  The
    tap-subset plans are the ones colddiff.inception._tap_parts makes.  HAZARD rows: every tap set over one, several and ragged 128-row
    tiles on non-square maps; FIDInceptionE's six slices; the 8 x 8 stage at B = 1 and B = 2."""
    from colddiff import inception as I
    for rows, forms, reached in ((SP_FORM_ROWS, sp_forms, REACHED_SP), (SP_PROD_ROWS, sp_forms, REACHED_SP),
                                 (F32_FORM_ROWS, f32_forms, REACHED_F32), (F32_PROD_ROWS, f32_forms, REACHED_F32)):
        assert forms(rows) == reached and len(rows) == len(reached), (sorted(forms(rows) ^ reached, key=repr), len(rows), len(reached))
    assert len(REACHED_SP_B50) == 27 and len(REACHED_SP_B1) == 24 and len(REACHED_SP) == 31 and len(REACHED_F32_DEFAULT) == 4 and len(REACHED_F32) == 15
    for r in SP_FORM_ROWS + SP_HAZARD_ROWS + SP_PROD_ROWS + F32_FORM_ROWS + F32_HAZARD_ROWS + F32_PROD_ROWS:
        part = isinstance(r.k, TapSubset)
        assert (r.ops, r.act, r.acc) == (("b", ACT_RELU, 0) if not part else (("b", 0, 0) if r.k.lo == 0 else ("", 0, 1))), r
        assert r.B * r.H * r.W * r.Cin <= (1 << 16) or r in SP_PROD_ROWS + F32_PROD_ROWS, ("a small row that is not small", r)
    for (H, W) in ((6, 7), (35, 35)):
        mine = [gemm_plan("conv_fwd", H, W, k, 1, 2) for k in (T16, T9)]
        theirs = I._tap_parts(H, W, (5, 5), 1, (2, 2))
        assert [(list(p.desc), p.ntaps_w, p.OH, p.OW) for p in mine] == [(list(p.desc), p.ntaps_w, p.OH, p.OW) for p in theirs]
    assert I.MAX_TAPS == 16 and T16.hi - T16.lo == 16 and T9.hi == 25
    for rows in (SP_FORM_ROWS + SP_HAZARD_ROWS, F32_FORM_ROWS + F32_HAZARD_ROWS):
        for k, along in (((1, 7), "W"), ((7, 1), "H"), ((1, 3), "W"), ((3, 1), "H")):
            rs = [r for r in rows if r.k == k]
            assert all(r.H != r.W or (r.H, r.W) == (8, 8) for r in rs), k
            if k[0] * k[1] == 7:                             # at least 9 pixels along the taps: columns 3 .. 5 have all seven inside
                assert all(getattr(r, along) >= 9 for r in rs), k
                m = {(r.B * r.H * r.W) for r in rs}
                assert 128 in m and 256 in m and any(v < 128 for v in m) and any(v > 128 and v % 128 for v in m), (k, m)
                assert {r.Cin for r in rs} >= {32, 64, 96}, k
        s2 = {(r.H, r.W) for r in rows if r.s == 2}
        assert s2 >= {(9, 7), (7, 9), (17, 17)} and all((h - 3) % 2 == 0 and (w - 3) % 2 == 0 for h, w in s2), s2
        assert {r.yoff for r in rows if r.yld == 2048} == {0, 320, 704, 1088, 1472, 1856}
        assert {r.B for r in rows if (r.H, r.W) == (8, 8) and r.yld == 2048} == {1, 2}
        offs = {r.yoff for r in rows if r.yld}                # the residues the blocks' widths produce: 32 mod 64, 64 mod 128, 0
        assert 0 in offs and any(o % 64 == 32 for o in offs) and any(o % 128 == 64 for o in offs), offs
    tiles = {}                                               # the split kernel's M tile is 128 rows: per tap set one whole tile, several, ragged
    for r in SP_FORM_ROWS + SP_HAZARD_ROWS:
        pl = gemm_plan(r.kind, r.H, r.W, r.k, r.s, r.pad)
        tiles.setdefault(sf.sp_gemm_form(sf.gs_args(r))[1], set()).add(r.B * pl.OH * pl.OW)
    assert set(tiles) == {"1tap", _1x7, _7x1, _1x3, _3x1, _P1, _P0, _S2, _G16, _G9}
    for geom, m in tiles.items():
        assert 128 in m and any(v > 128 and v % 128 == 0 for v in m) and any(v % 128 for v in m), (geom, m)
    assert {r.Cin for r in F32_FORM_ROWS} >= {3, 48, 80} and {r.Cout for r in F32_FORM_ROWS} >= {32, 48, 80, 96, 160}
    assert {r.Cin for r in SP_FORM_ROWS} >= {48, 80} and {r.Cout for r in SP_FORM_ROWS + SP_HAZARD_ROWS} >= {80, 96, 160, 320, 448}


# ---------------------------------------------------------------------------------------------------------------------------------
# the 5 x 5 layer: 16-tap launch with bias, 9-tap launch accumulating onto it, ReLU by cdf_act_fwd into the block's slice
# ---------------------------------------------------------------------------------------------------------------------------------
def _pair_case(be, path, B, H, W, Cin, Cout, yld, yoff):
    L, sp = be.L, path == "sp"
    ns = 3 if sp else 1
    tag = f"5x5 pair {path} B={B} {H}x{W} {Cin}->{Cout} slice {yoff} of {yld}"
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + W + ns)
    x, bias = torch.randn(B, H, W, Cin, generator=g), torch.randn(Cout, generator=g)
    ldo = r4(Cout)
    pre, out = nan_empty(be, B, H, W, ldo), nan_empty(be, B, H, W, yld)
    t = dict(x=be.to(x), y=pre, bias=be.to(bias))
    if sp:
        w, t["whi"], t["wlo"], _, wh, wl = _weights(be, "conv_fwd", Cin, Cout, (5, 5), 3, Cin * 7 + Cout)
        wh, wl = wh.cpu(), wl.cpu()
        rows = [S(B, H, W, Cin, Cout, T16, 1, 2, "b", 0), S(B, H, W, Cin, Cout, T9, 1, 2, "", 0, 1)]
        ad = {k_: P(v) for k_, v in t.items()}
        calls = [(L.cdf_conv_gemm_bf16, sf.gs_args(r, ad, be.stream())) for r in rows]
        forms = [sf.sp_gemm_form(a) for _, a in calls]
        assert forms == [sf.sp_gemm_form(sf.gs_args(r)) for r in rows], (tag, "the launches are not the forms the rows claim", forms)
        assert set(forms) <= REACHED_SP or (B * H * W) % 128 == 0, (tag, forms)      # (the extractor's 35 x 35 maps never fill whole tiles)
        ah, al = (_nchw(p_, Cin) for p_ in sf._planes(x, 3))
        cv = lambda a_, b_: _conv64("conv_fwd", a_, b_, (5, 5), 1, 2, (H, W))
        sums = lambda m: (cv(ah, m(wh) + m(wl)) + cv(al, m(wh)), cv(ah * ah, m(wh) ** 2 + m(wl) ** 2) + cv(al * al, m(wh) ** 2))
    else:
        w = torch.randn(Cout, Cin, 5, 5, generator=g) / math.sqrt(Cin * 25)
        wp = torch.zeros(25, Cin, ldo)
        wp[..., :Cout] = w.permute(2, 3, 1, 0).reshape(25, Cin, Cout)
        t["w"] = be.to(wp)
        rows = [F(B, H, W, Cin, Cout, T16, 1, 2, "b", 0), F(B, H, W, Cin, Cout, T9, 1, 2, "", 0, 1)]
        ad = {k_: P(v) for k_, v in t.items()}
        calls = [(L.cdf_conv_gemm, ff.gr_args(r, ad, be.stream())[1]) for r in rows]
        forms = [ff.f32_gemm_form("cdf_conv_gemm", a) for _, a in calls]
        assert forms == [ff.f32_gemm_form(*ff.gr_args(r)) for r in rows], (tag, "the launches are not the forms the rows claim", forms)
        assert set(forms) <= REACHED_F32, (tag, forms)
        x64 = _nchw(x.double(), Cin)
        cv = lambda a_, b_: _conv64("conv_fwd", a_, b_, (5, 5), 1, 2, (H, W))
        sums = lambda m: (cv(x64, m(w.double())), cv(x64 * x64, m(w.double()) ** 2))
    print(f"{tag}: forms {forms}")

    def launch():
        for fn, a in calls:
            fn(*a)
        L.cdf_act_fwd(P(pre), ldo, P(out) + 4 * yoff, yld, B * H * W, Cout, ACT_RELU, be.stream())
    gpre, gout = twice(launch, [pre, out])
    (v1, q1), (v2, q2) = sums(lambda m_: tap_mask(m_, T16)), sums(lambda m_: tap_mask(m_, T9))
    e1 = K_SUM * U * math.sqrt(ns * 16 * Cin) * q1.max().sqrt().item()
    e2 = K_SUM * U * math.sqrt(ns * 9 * Cin) * q2.max().sqrt().item()
    y1, _, e_y1, _ = _epilogue64(v1, e1, dict(bias=bias.double()), 0, 0, False)
    y2, _, e_y2, _ = _epilogue64(v2, e2, dict(y0=y1), 0, 0, False)   # (the second launch adds onto the first's output: that output's bound is added)
    e = e_y1 + e_y2
    check(f"{tag} pre-activation (16 + 9 taps)", _nchw(gpre, Cout), y2, e)
    check(f"{tag} ReLU output", _nchw(gout[..., yoff:], Cout), y2.clamp_min(0), e)     # (cdf_act_fwd's ReLU: exact, Lipschitz 1)
    assert torch.equal(gout[..., yoff:yoff + Cout], gpre[..., :Cout].clamp_min(0)), (tag, "ReLU of the stored pre-activation, bit for bit")
    assert sf._poison_outside(gout, yoff, yoff + Cout), (tag, "an element outside the slice changed")
    assert sf._poison_outside(gpre, 0, Cout), (tag, "a pad column of the pre-activation changed")
    true = (cv(_nchw(x.double(), Cin), w.double()) + bias.double()[None, :, None, None]).clamp_min(0)
    tol = 3e-5 * max(1.0, true.abs().max().item())
    if sp:
        check(f"{tag} split operands alone against the true float64 convolution", y2.clamp_min(0), true, SPLIT_MARGIN * tol)
    check(f"{tag} true float64 convolution", _nchw(gout[..., yoff:], Cout), true, tol)


# ---------------------------------------------------------------------------------------------------------------------------------
# the recording
# ---------------------------------------------------------------------------------------------------------------------------------
RECORDED = (("bf16x3", 50), ("bf16x3", 1), ("bf16", 50), ("bf16", 1), ("f32", 50), ("f32", 1))


def extractor_calls(dev):
    """One forward of the extractor on 64 x 64 images (resized to 299 x 299) per (mode, B) of RECORDED on `dev`: [((mode, B), name,
    arguments)] of every conv GEMM call, the descriptors copied."""
    from colddiff import runtime as rt
    from colddiff.inception import InceptionV3
    from test_gpu_invariance import Recorder
    torch.manual_seed(6)
    net = InceptionV3([0, 1, 2, 3], resize_input=True, weights="random").to(dev)
    calls = []
    for mode, B in RECORDED:
        x = torch.rand(B, 3, 64, 64).to(dev)
        with rt.precision_scope(mode), Recorder(rt.lib()) as rec, torch.no_grad():
            out = net(x)
            if x.is_cuda:
                torch.cuda.synchronize()
        assert [tuple(o.shape[1:]) for o in out] == [(64, 73, 73), (192, 35, 35), (768, 17, 17), (2048, 1, 1)]
        calls += [((mode, B), n, tuple(tuple(v) if hasattr(v, "_length_") else v for v in a)) for n, a in rec.calls if n.startswith("cdf_conv_")]
    return calls


def check_recording(calls):
    """The two assertions of the guard on a recording of extractor_calls: every recorded form is a tested form (a FORM row and a PROD
    row), every form flagged as reached is recorded.  Prints the reached forms per mode and batch size."""
    sp, f32 = {}, {}
    for src, name, a in calls:
        assert name in ("cdf_conv_gemm_bf16", "cdf_conv_gemm"), (src, name)     # (no other GEMM entry point serves the extractor)
        if name == "cdf_conv_gemm_bf16":
            # the metric must not depend on the training arithmetic: bf16 mode runs the extractor split in three, lo plane present
            assert src[0] != "f32" and a[32] == 3 and a[3], (src, "the extractor's split GEMM must run as bf16x3", a[32])
            sp.setdefault(src, set()).add(sf.sp_gemm_form(a))
        else:
            f32.setdefault(src, set()).add(ff.f32_gemm_form(name, a))
    for src in RECORDED:
        print(f"extractor, {src[0]}, B = {src[1]}: {len(sp.get(src, ()))} cdf_conv_gemm_bf16 forms, {len(f32.get(src, ()))} cdf_conv_gemm forms")
        for what, forms in (("cdf_conv_gemm_bf16", sp.get(src, ())), ("cdf_conv_gemm", f32.get(src, ()))):
            for k in sorted(forms, key=repr):
                print(f"    {what} {k!r},")
    for B, flagged in ((50, REACHED_SP_B50), (1, REACHED_SP_B1)):
        assert sp[("bf16", B)] == sp[("bf16x3", B)] and f32[("bf16", B)] == f32[("bf16x3", B)], ("bf16 mode must launch what the default mode launches", B)
        stale = sorted(flagged - sp[("bf16x3", B)], key=repr)
        assert not stale, "forms flagged as reached at B = %d that the recording no longer contains: %s" % (B, stale)
    reached_sp = set().union(*sp.values())
    reached_fd = set().union(*(v for k, v in f32.items() if k[0] != "f32"))
    reached_f = set().union(*(v for k, v in f32.items() if k[0] == "f32"))
    assert not any(k[0] == "f32" for k in sp)
    for what, reached, flagged, tables in (("cdf_conv_gemm_bf16", reached_sp, REACHED_SP, (sp_forms(SP_FORM_ROWS), sp_forms(SP_PROD_ROWS))),
                                           ("cdf_conv_gemm (default mode)", reached_fd, REACHED_F32_DEFAULT, (f32_forms(F32_FORM_ROWS), f32_forms(F32_PROD_ROWS))),
                                           ("cdf_conv_gemm (f32 mode)", reached_f, REACHED_F32, (f32_forms(F32_FORM_ROWS), f32_forms(F32_PROD_ROWS)))):
        for tname, tested in zip(("FORM", "PROD"), tables):
            untested = sorted(reached - tested, key=repr)
            assert not untested, "%s forms the extractor reaches without a test_inception_forms %s row: %s" % (what, tname, untested)
        stale = sorted(flagged - reached, key=repr)
        assert not stale, "test_inception_forms flags %s forms as reached that the recording no longer contains: %s" % (what, stale)


def test_recorded_extractor_forms_dry(monkeypatch):
    """The recording without a GPU, the technique of test_gemm_sp_forms.py::test_recorded_sp_forms_dry: the extractor's forwards at their
    real shapes on CPU tensors with every launching entry point replaced by a stub that returns 0.  Which entry point is called with
    which arguments is decided by the Python layer from shapes and modes alone."""
    import types
    from colddiff import _lib, runtime as rt
    from emu_util import emu_lib
    real, stub = emu_lib(), types.SimpleNamespace()
    for name, (restype, _) in real.protos.items():
        launches = restype is ctypes.c_int and not _lib._QUERY.search(name) and name != "cdf_gemm_tuning_default"
        setattr(stub, name, (lambda *a: 0) if launches else getattr(real, name))
    monkeypatch.setattr(rt, "_lib_override", stub)
    check_recording(extractor_calls("cpu"))


# ---------------------------------------------------------------------------------------------------------------------------------
# the tests over the case tables
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", SP_FORM_ROWS + SP_HAZARD_ROWS, ids=_rid)
def test_extractor_sp_forms(be, r):
    _check_sp(be, r)


def _check_sp(be, r):
    form = sf._sp_gemm_case(be, r, split_margin=SPLIT_MARGIN)
    assert form == sf.sp_gemm_form(sf.gs_args(r)) and (form in REACHED_SP or r in SP_HAZARD_ROWS), (r, form)


@pytest.mark.parametrize("r", F32_FORM_ROWS + F32_HAZARD_ROWS, ids=_rid)
def test_extractor_f32_forms(be, r):
    ff._igemm_case(be, r)


@pytest.mark.parametrize("row", PAIR_ROWS, ids=_rid)
def test_extractor_5x5_pair(be, row):
    _pair_case(be, *row)


@pytest.mark.gpu
@pytest.mark.parametrize("r", SP_PROD_ROWS, ids=_rid)
def test_extractor_sp_production_shapes(r):
    _check_sp(_hip(), r)


@pytest.mark.gpu
@pytest.mark.parametrize("r", F32_PROD_ROWS, ids=_rid)
def test_extractor_f32_production_shapes(r):
    ff._igemm_case(_hip(), r)
