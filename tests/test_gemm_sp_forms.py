"""The in-kernel-split bf16 GEMM pair of csrc/k_conv_sp.hip -- conv_igemm_sp_kernel<1|3> (cdf_conv_gemm_bf16: every attention and
projection 1 x 1 of the training step and every 1 x 1 data gradient, in both arithmetic modes) and conv_wgrad_sp_kernel
(cdf_conv_wgrad_bf16) -- in every form the product launches.  Conventions of test_kernels_production.py / test_gemm_production.py /
test_gemm_f32_forms.py: every output, workspace and bsum NaN-poisoned before each of two launches that must agree bit for bit, a float64
reference, a derived bound, every worst error / bound printed.

Shapes are the smallest that reach the hazard, not the workload's: all addressing in both kernels is 64-bit, or 32-bit within a pass of
at most 128 rows, so what can go wrong is a tile edge, the K tail, the parity of the two-stage lookahead, the block order (cdf_xcd_order
with a remainder: 22 blocks at Cout = 136, M = 1296), the split walk and the epilogue choice.

Reference: the same operation in float64 on the operands the kernel multiplies.  Weights: the planes cdf_pack_weight_bf16 produced, read
back and widened (test_gemm_production._weights; that function is tested bit-exactly elsewhere).  Activations: the in-kernel split,
restated here in torch integer ops (_split_trunc: hi = bits & 0xFFFF0000, lo = bits(x - hi) & 0xFFFF0000 -- cdf_split4_trunc; split = 1:
x.bfloat16(), round to nearest even).  Sum: split = 3 per tap  sum a_hi (b_hi + b_lo) + a_lo b_hi,  split = 1  sum a_hi b_hi,  weight
gradient always three terms; the epilogue follows in float64 (test_gemm_production._epilogue64).  The weight gradient's reference is the
contract of include/colddiff.h written out as a gather (_wgrad_taps: per tap the rows XA[pixA(m, tap)], XB[pixB(m, tap)], zero outside),
so every slab has its own reference whatever the plan; its sum over all pixels must equal torch.nn.grad.conv2d_weight in float64
(test_gemm_production._wgrad_ref64) to 1e-12.  No cdf_* GEMM is the reference.

Bound, no new constant: first assertion, fp32 accumulation only --  K_SUM 2^-24 sqrt(n) max ||terms||_2  with n = NS x taps x Cin for
outputs and n = 3 x the slab's pixels for slabs and for the sum of the slabs, plus one fp32 rounding per epilogue operand and the
Lipschitz / erf terms of _epilogue64; bsum rows: sum_bound over the slab's pixels.  Second assertion, kept from test_kernels.py::_sp_case:
the distance to the true float64 convolution of the unsplit operands stays within 3e-5 max(1, |ref|max) (2e-2 for split = 1; weight
gradient 3e-5 max(1, |ref|max) sqrt(M / 16)).

Poison: y is allocated with its neighbours (a pitched or sliced y lies inside a wider poisoned buffer); the columns of a pitched y beyond
Cout, the columns on both sides of a slice target and the pad of `pre` must still hold the poison bit pattern afterwards.  The pad columns
CB .. ldo-1 of slabs and bsum rows, and every slab and bsum row of a split without pixels, are exact zeros.  Inputs: whatever a launch
must not read is NaN (the columns of x / xa / xb beyond the last channel quad, res / mul / sbias columns beyond Cout); the in-quad pad
channels C .. r4(C)-1 hold 1e30 (include/colddiff.h: they must be finite, and no finite value may change a result).

Forms: the pair has no dispatcher to query, so sp_gemm_form / sp_wgrad_form are pure functions of a call's argument tuple -- the epilogue
path ('fast', id / 'vec' / 'scalar') derived exactly as cdf_epi_select + cdf_epi_tile_ok + cdf_epi_family_ok decide it.  Every row builds
its tuple through one helper (gs_args / ws_args), the tested forms are those functions applied to the rows, each case asserts that its
real argument tuple has the form its stand-in tuple claims.  test_gpu_invariance.py::test_coverage_guard holds the recorded calls of the
bench step (bf16x3, bf16), the sampler step and config 2's pass against them; test_recorded_sp_forms_dry makes the same recording
without a GPU.  The recordings reach (REACHED_SP_GEMM / REACHED_SP_WGRAD): one-tap geometry only, both splits, the operand sets none /
bias / bias + residual / accumulate on whole M tiles with whole and half N tiles, x as a slice, y pitched, a residual pitch different from
ldy; of the weight gradient one-tap plans on whole tiles with pitched operands, with and without bsum, with and without empty slabs.

Worst error / bound per group (136 GEMM + 32 weight-gradient cases; the simulator runs the module in 49 s in one process, the MI355X in
4 s).  The simulator column is a run of the kernel sources on the host simulator, not a measurement of the kernel:
                                                      simulator    MI355X
    GEMM             y, split = 3                     0.53         0.22
                     y, split = 1                     0.47         0.21
                     pre-activation                   0.25         0.12
                     true float64 convolution         0.50 of 3e-5 max (split = 3), 0.15 of 2e-2 max (split = 1), both backends
    weight gradient  slab by slab                     0.48         0.20
                     sum of the slabs                 0.33         0.15
                     bsum rows                        0.34         0.34
                     true float64 weight gradient     0.61 of 3e-5 max sqrt(M / 16), both backends
The MI355X's sums are closer to float64 than the simulator's: the simulator adds the 16 products of an MFMA one by one in fp32
(tests/emu/hipemu.h), and the lower ratios say the matrix core rounds less often inside that dot product.  The distances to the true
results are the operand split's own error and agree to three digits.
"""
import math
from typing import NamedTuple

import pytest
import torch

from poison import nan_empty
from test_kernels import P, r4
from test_kernels_production import K_SUM, U, check, sum_bound, twice
from test_gemm_production import _conv64, _dist, _epilogue64, _khw, _nchw, _weights, _wgrad_ref64, gemm_plan, wgrad_plan

BIG = 1.0e30                                                 # the finite value of in-quad pad channels (include/colddiff.h: cdf_conv_gemm)
NAN32 = torch.tensor(float("nan")).view(torch.int32).item()  # the poison bit pattern of tests/poison.py
_STANDIN = 1 << 20                                           # a 16-byte-aligned stand-in address (form of a row without buffers)


# ---------------------------------------------------------------------------------------------------------------------------------
# kernel forms: pure functions of a call's argument tuple (a recorded one, or the one a case row builds)
# ---------------------------------------------------------------------------------------------------------------------------------
def _addr(v):
    return 0 if v is None else int(getattr(v, "value", v) or 0)


def sp_gemm_form(a):
    """The form of a cdf_conv_gemm_bf16 call, from its arguments alone (csrc/k_conv_sp.hip, csrc/cdf_epilogue.h):
    (split, geometry, epilogue path, operand letters, act, mul_mode, accumulate, M edge, N class, K tail, x sliced, y pitched, ldr != ldy).
    geometry: '1tap', or (nphase, taps of phase 0, os, is, first tap's dy, dx);
    epilogue path: ('fast', id) -- cdf_epi_select's id where the block tiles are whole (cdf_epi_tile_ok) and the kernel's family takes
    the id (cdf_epi_family_ok: conv_igemm_sp_kernel<1> is the bf16-storage family and rejects ids 1..6) -- else 'vec' or 'scalar', the
    generic epilogue with float4 or per-element accesses;
    M edge: 'whole' / 'ragged' 128-row tiles;  N class: 'whole' 128-column tiles, 'half' (the last one holds 64), 'ragged';
    K tail: Cin is no multiple of the 32-channel K step."""
    ldx, y, ldy = a[1], _addr(a[5]), a[6]
    B, H, W, Cin, OH, OW, Cout, QH, QW, os_, is_, nphase = a[7:19]
    desc = list(a[19])
    bias, sbias, ld_sb, res, ldr, pre, ldp, mul, ldm = _addr(a[20]), _addr(a[21]), a[22], _addr(a[23]), a[24], _addr(a[25]), a[26], _addr(a[27]), a[28]
    act, mm, acc, split = a[29:33]
    M = B * QH * QW
    geom = "1tap" if (nphase == 1 and desc[2] == 1) else (nphase, desc[2], os_, is_, desc[3], desc[4])
    ops = "".join(c for c, v in zip("bsrpm", (bias, sbias, res, pre, mul)) if v)
    # cdf_epi_vec_ok
    ptrs = y | bias | sbias | res | pre | mul
    pitches = ldy | (ld_sb if sbias else 0) | (ldr if res else 0) | (ldp if pre else 0) | (ldm if mul else 0)
    vec = Cout % 4 == 0 and ptrs & 15 == 0 and pitches & 3 == 0
    # cdf_epi_select (no output planes, no typed operands on this entry point: ids 1, 2 and 6 are the ones it can return)
    eid = 0
    if vec and os_ == 1 and QH == OH and QW == OW and act == 0 and not pre and mm == 0:
        eid = {(False, False): 1, (True, False): 2, (False, True): 6}.get((bool(res), bool(acc)), 0)
    # cdf_epi_tile_ok, cdf_epi_family_ok(id, SPLIT == 1)
    fast = eid != 0 and M % 128 == 0 and Cout % 128 == 0 and (not sbias or (QH * QW) % 128 == 0) and split == 3
    path = ("fast", eid) if fast else ("vec" if vec else "scalar")
    nclass = "whole" if Cout % 128 == 0 else ("half" if Cout % 128 == 64 else "ragged")
    return (split, geom, path, ops, act, mm, acc, "whole" if M % 128 == 0 else "ragged", nclass, int(Cin % 32 != 0), int(ldx > r4(Cin)),
            int(ldy > r4(Cout)), int(bool(res) and ldr != ldy))


def _m_per_split(M, nsplit):
    return -(-(-(-M // nsplit)) // 32) * 32                  # (cdf_fill_wgrad_geom: a slab's pixel count is rounded up to the kernel's 32-pixel step)


def sp_wgrad_form(a):
    """The form of a cdf_conv_wgrad_bf16 call: (plan class, CA tiles, CB tiles, pitched operands, bsum, an empty slab, a ragged step).
    plan class: '1tap', ('convT', taps) when XB is the strided side, ('conv', taps, stride) otherwise;  tiles: 'whole' / 'ragged' 128-channel
    tiles;  pitched: 'a' / 'b' where lda / ldb exceed the channel count's quad;  ragged step: M is no multiple of the 32-pixel step."""
    lda, ldb, B, QH, QW = a[1], a[3], a[6], a[7], a[8]
    sa, sb, CA, CB, ntaps, nsplit, bsum = a[11], a[14], a[15], a[16], a[17], a[19], _addr(a[20])
    M = B * QH * QW
    plan = "1tap" if ntaps == 1 else (("convT", ntaps) if sb > 1 else ("conv", ntaps, sa))
    tile = lambda C: "whole" if C % 128 == 0 else "ragged"
    pitched = ("a" if lda > r4(CA) else "") + ("b" if ldb > r4(CB) else "")
    return (plan, tile(CA), tile(CB), pitched, int(bool(bsum)), int((nsplit - 1) * _m_per_split(M, nsplit) >= M), int(M % 32 != 0))


# ---------------------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------------------
def _poison_outside(t, lo, hi):
    """Every element of host tensor t (fp32) outside columns lo .. hi-1 of its last dimension still holds the poison bit pattern."""
    bits = t.view(torch.int32)
    return bool((bits[..., :lo] == NAN32).all() and (bits[..., hi:] == NAN32).all())


def _padded(t, ld, off=0, quad_pad=None):
    """t [..., C] inside a [..., ld] buffer at channel offset off: NaN everywhere else, except the pad channels of t's last channel quad
    (quad_pad: finite -- the kernels load whole quads and rely on zero weight rows / unsaved output rows for them)."""
    C = t.shape[-1]
    buf = torch.full(t.shape[:-1] + (ld,), float("nan"), dtype=t.dtype)
    buf[..., off:off + C] = t
    if quad_pad is not None:
        buf[..., off + C:off + r4(C)] = quad_pad
    return buf


def _split_trunc(x):
    """cdf_split4_trunc (csrc/cdf_conv_sp.h) in torch integer ops: hi = x truncated to its upper 16 bits, lo = (x - hi) -- exact in
    fp32 -- truncated likewise.  Returns the two fp32 tensors whose upper halves are the bf16 terms."""
    hi = (x.view(torch.int32) & -65536).view(torch.float32)
    lo = ((x - hi).view(torch.int32) & -65536).view(torch.float32)
    return hi, lo


def _planes(x, split):
    """The bf16 terms (as float64) conv_igemm_sp_kernel<split> multiplies for the fp32 activations x: (hi, lo or None)."""
    if split == 3:
        hi, lo = _split_trunc(x)
        return hi.double(), lo.double()
    return x.bfloat16().double(), None                       # (round to nearest even: cdf_f2bf)


def _max_taps(pl):
    n, p = 0, 0
    for _ in range(pl.nphase):
        n, p = max(n, pl.desc[p + 2]), p + 3 + 3 * pl.desc[p + 2]
    return n


# ---------------------------------------------------------------------------------------------------------------------------------
# conv_igemm_sp_kernel
# ---------------------------------------------------------------------------------------------------------------------------------
class GS(NamedTuple):
    """kind / H / W / k / s / pad: the arguments of test_gemm_production.gemm_plan (H, W: the convolution's own input size); Cin, Cout: K and N
    of the GEMM; ops: letters of the epilogue operands (b bias, s per-sample bias, r residual, p pre-activation output, m multiplier);
    x / y: channel slices [off, off + C) of buffers of pitch ld (0: r4(C)); ldr / ldp: pitch of the residual / pre-activation (0: r4(Cout))."""
    kind: str
    B: int
    H: int
    W: int
    Cin: int
    Cout: int
    k: int
    s: int
    pad: int
    ops: str = ""
    act: int = 0
    mm: int = 0
    acc: int = 0
    xld: int = 0
    xoff: int = 0
    yld: int = 0
    yoff: int = 0
    ldr: int = 0
    ldp: int = 0
    split: int = 3


def gs_args(r, ad=None, stream=0):
    """The argument tuple of a GS row, the way ops.conv_gemm writes the call; ad: the buffers' addresses (None: aligned stand-ins, for
    the form alone)."""
    pl = gemm_plan(r.kind, r.H, r.W, r.k, r.s, r.pad)
    ldx, ldo, ldk = r.xld or r4(r.Cin), r4(r.Cout), (r.Cin + 31) // 32 * 32
    ldy = r.yld or ldo
    at = lambda key, on=True: ((ad[key] if ad else _STANDIN) if on else 0)
    has = lambda c: c in r.ops
    return (at("x") + 4 * r.xoff, ldx, at("whi"), at("wlo", r.split == 3), ldk, at("y") + 4 * r.yoff, ldy, r.B, pl.H, pl.W, r.Cin, pl.OH, pl.OW,
            r.Cout, pl.QH, pl.QW, pl.os, pl.istride, pl.nphase, pl.desc, at("bias", has("b")), at("sbias", has("s")), ldo if has("s") else 0,
            at("res", has("r")), (r.ldr or ldo) if has("r") else 0, at("pre", has("p")), (r.ldp or ldo) if has("p") else 0, at("mul", has("m")),
            ldo if has("m") else 0, r.act, r.mm, r.acc, r.split, stream)


def _sp_gemm_case(be, r, split_margin=None):
    """r.k, r.pad: an int, an (h, w) pair, or (k) a TapSubset (test_gemm_production.gemm_plan).  split_margin: when given, the float64
    sum of the split operands alone must lie within that fraction of the second assertion's tolerance of the true convolution -- a row
    that misses it has inputs the operand split cannot carry, whatever the kernel does."""
    pl = gemm_plan(r.kind, r.H, r.W, r.k, r.s, r.pad)
    B, Cin, Cout, k, ns = r.B, r.Cin, r.Cout, r.k, r.split
    ldx, ldo = r.xld or r4(Cin), r4(Cout)
    ldy, ldr, ldp = r.yld or ldo, r.ldr or ldo, r.ldp or ldo
    assert r.xoff % 4 == 0 and r.yoff % 4 == 0 and r.xoff + r4(Cin) <= ldx and r.yoff + Cout <= ldy and ldr >= Cout and ldp >= Cout
    tag = "sp gemm " + "-".join(map(str, r))
    g = torch.Generator().manual_seed(Cin * 131 + Cout * 7 + _khw(k)[0] + r.H)
    rn = lambda *s_: torch.randn(*s_, generator=g)
    x = rn(B, pl.H, pl.W, Cin)
    w, whi, wlo, ldk, wh64, wl64 = _weights(be, r.kind, Cin, Cout, k, ns, Cin * 7 + Cout)
    wh64, wl64 = wh64.cpu(), (None if wl64 is None else wl64.cpu())   # (the reference runs on the host for both backends)
    osh = (B, pl.OH, pl.OW)
    t, o32 = dict(x=be.to(_padded(x, ldx, r.xoff, BIG)), whi=whi, wlo=wlo), {}
    if "b" in r.ops:
        o32["bias"] = rn(Cout)
        t["bias"] = be.to(o32["bias"])
    if "s" in r.ops:
        o32["sbias"] = rn(B, Cout)
        t["sbias"] = be.to(_padded(o32["sbias"], ldo))
    for key, letter, ld in (("res", "r", ldr), ("mul", "m", ldo)):
        if letter in r.ops:
            o32[key] = rn(*osh, Cout)
            t[key] = be.to(_padded(o32[key], ld))
    y0 = rn(*osh, Cout) if r.acc else None
    y0d = be.to(_padded(y0, ldy, r.yoff)) if r.acc else None
    t["y"] = nan_empty(be, *osh, ldy)
    if "p" in r.ops:
        t["pre"] = nan_empty(be, *osh, ldp)
    args = gs_args(r, {k_: P(v) for k_, v in t.items()}, be.stream())
    form = sp_gemm_form(args)
    print(f"{tag}: form {form}")
    assert form == sp_gemm_form(gs_args(r)), (tag, "the launch is not the form the table claims (pointer alignment)")

    def launch():
        if r.acc:
            t["y"].copy_(y0d)                                # (accumulate reads y: its previous contents are an input)
        be.L.cdf_conv_gemm_bf16(*args)
    names = [n for n in ("y", "pre") if n in t]
    got = dict(zip(names, twice(launch, [t[n] for n in names])))

    # ---- float64: the sums of the split operands' products, max ||terms||_2 over the outputs, the true convolution
    cv = lambda a_, b_: _conv64(r.kind, a_, b_, k, r.s, r.pad, (pl.OH, pl.OW))
    xh, xl = _planes(x, ns)
    ah = _nchw(xh, Cin)
    if ns == 3:
        al = _nchw(xl, Cin)
        v = cv(ah, wh64 + wl64) + cv(al, wh64)
        sq = cv(ah * ah, wh64 * wh64 + wl64 * wl64) + cv(al * al, wh64 * wh64)
    else:
        v, sq = cv(ah, wh64), cv(ah * ah, wh64 * wh64)
    true = cv(_nchw(x.double(), Cin), w.double())
    e0 = K_SUM * U * math.sqrt(ns * _max_taps(pl) * Cin) * sq.max().sqrt().item()
    n64 = lambda key: None if key not in o32 else _nchw(o32[key].double(), Cout)
    o = dict(bias=None if "bias" not in o32 else o32["bias"].double(), sbias=None if "sbias" not in o32 else o32["sbias"].double(),
             res=n64("res"), mul=n64("mul"), y0=None if y0 is None else _nchw(y0.double(), Cout), pre="p" in r.ops)
    yr, prer, e_y, e_pre = _epilogue64(v, e0, o, r.act, r.mm, False)
    yt = _epilogue64(true, 0.0, o, r.act, r.mm, False)[0]
    gy = _nchw(got["y"][..., r.yoff:], Cout)
    check(f"{tag} y (split {ns})", gy, yr, e_y)
    assert _poison_outside(got["y"], r.yoff, r.yoff + Cout), (tag, "y: an element outside the output's channels changed")
    if "p" in r.ops:
        check(f"{tag} pre", _nchw(got["pre"], Cout), prer, e_pre)
        assert _poison_outside(got["pre"], 0, Cout), (tag, "pre: a pad column changed")
    tol = (3e-5 if ns == 3 else 2e-2) * max(1.0, yt.abs().max().item())
    if split_margin is not None:
        check(f"{tag} split operands alone against the true float64 convolution", yr, yt, split_margin * tol)
    check(f"{tag} true float64 convolution (split {ns})", gy, yt, tol)
    return form


# geometry: (kind, k, s, pad, the convolution's input size for an 8 x 8 / 16 x 16 / 9 x 9 grid of GEMM rows)
_GEOM = [("conv_fwd", 1, 1, 0, (8, 16, 9)), ("conv_fwd", 3, 1, 1, (8, 16, 9)), ("conv_dgrad", 3, 1, 1, (8, 16, 9)), ("conv_fwd", 4, 2, 1, (16, 32, 18)),
         ("conv_dgrad", 4, 2, 1, (16, 32, 18)), ("convT_fwd", 4, 2, 1, (8, 16, 9)), ("convT_dgrad", 4, 2, 1, (8, 16, 9)), ("conv_fwd", 3, 2, -1, (16, 32, 18))]
# K: 32 one K step; 64, 96, 160: 2, 3, 5 steps (both parities of the two-stage lookahead); 40, 36: a tail of 8 / 4 channels inside the
# zero-padded ldk = 64; 38 (pitch 40): two in-quad pad channels, finite, against zero weight columns
_CINS = [32, 64, 96, 160, 40, 36, 38]
# N: 64 half a tile (as launched), 128, 256 two tiles, 136 a ragged second tile (vector epilogue), 130 the scalar epilogue
_COUTS = [64, 128, 256, 136, 130]
# epilogue operand sets the product reaches: (ops, accumulate)
_EPI_REACHED = [("", 0), ("b", 0), ("br", 0), ("", 1)]


def _gemm_rows():
    rows = []
    # every geometry with three different (M, K, N, reached operand set) combinations; M index 0: one whole tile, 1: four whole tiles, 2: ragged
    for gi, (kind, k, s, pad, sizes) in enumerate(_GEOM):
        for j in range(3):
            i = 3 * gi + j
            mi = (gi + j) % 3
            ops, acc = _EPI_REACHED[i % 4]
            cin = _CINS[i % 7] if (k == 1 or _CINS[i % 7] != 160) else 96   # (160 channels with the one-tap rows only: simulator time)
            rows.append(GS(kind, 2, sizes[mi], sizes[mi], cin, _COUTS[(i + gi) % 5], k, s, pad, ops, acc=acc))
    one = lambda B, n, cin, cout, *a, **kw: GS("conv_fwd", B, n, n, cin, cout, 1, 1, 0, *a, **kw)
    # one tap, every Cin and Cout not met above in that geometry, at each M
    rows += [one(2, (8, 16, 9)[i % 3], cin, _COUTS[i % 5], *_EPI_REACHED[(i + 1) % 4][:1], acc=_EPI_REACHED[(i + 1) % 4][1]) for i, cin in enumerate(_CINS)]
    # the reached operand sets, each where the tile is whole (the fast form under split = 3), where M is ragged and where N is half a tile
    for ops, acc in _EPI_REACHED:
        rows += [one(2, 8, 64, 128, ops, acc=acc), one(2, 9, 64, 128, ops, acc=acc), one(2, 8, 64, 64, ops, acc=acc), one(2, 16, 128, 256, ops, acc=acc)]
    # 11 x 2 = 22 blocks: cdf_xcd_order with a remainder
    rows += [one(1, 36, 32, 136, "b")]
    # operand sets the entry point accepts and no recording reaches: per-sample bias with one image per tile (fast) and with an image
    # boundary inside a tile (generic), bias + pre-activation + GELU, the multiplier with GELU' and plain, SiLU, ReLU
    rows += [one(2, 16, 64, 128, "s"), one(2, 8, 64, 128, "bs"), one(2, 9, 40, 136, "bp", 1), one(2, 8, 64, 128, "m", 0, 1), one(2, 9, 32, 136, "m", 0, 3),
             one(2, 8, 32, 130, "b", 2), one(2, 9, 36, 64, "b", 3)]
    # layout: x a slice (pitch 96 for 64 channels), y a slice at a 16-byte-aligned column offset of a wider buffer, y pitched with a
    # residual of its own pitch, the pre-activation's pitch different from ldy; on the fast and on the generic form
    rows += [one(2, 8, 64, 128, "", xld=96, xoff=16, yld=160, yoff=8),
             one(2, 9, 64, 136, "b", xld=96, xoff=16, yld=160, yoff=8),
             one(2, 16, 64, 128, "br", xld=96, yld=256, ldr=128), one(2, 9, 64, 128, "br", yld=256, ldr=128), one(2, 8, 64, 128, "br", ldr=136),
             one(2, 8, 64, 128, "", acc=1, yld=256, yoff=64), one(2, 9, 64, 64, "", acc=1, xld=96, yld=256, yoff=64),
             one(2, 8, 64, 128, "bp", 1, yld=160, yoff=8, ldp=136), one(2, 9, 96, 130, "br", yld=144, yoff=8, ldr=136),
             GS("convT_fwd", 2, 8, 8, 64, 128, 4, 2, 1, "br", xld=96, xoff=16, yld=160, yoff=8, ldr=136)]
    return [r._replace(split=s) for r in rows for s in (3, 1)]


GEMM_ROWS = _gemm_rows()


# ---------------------------------------------------------------------------------------------------------------------------------
# conv_wgrad_sp_kernel
# ---------------------------------------------------------------------------------------------------------------------------------
class WS(NamedTuple):
    """A convolution's weight gradient: kind / H / W / k / s / pad as in test_gemm_production.wgrad_plan; lda / ldb: pitches of xa / xb
    (0: r4(C))."""
    kind: str
    B: int
    H: int
    W: int
    CA: int
    CB: int
    k: int
    s: int
    pad: int
    nsplit: int
    bsum: int
    lda: int = 0
    ldb: int = 0


def ws_args(r, ad=None, stream=0):
    wp = wgrad_plan(r.kind, r.H, r.W, r.k, r.s, r.pad)
    at = lambda key, on=True: ((ad[key] if ad else _STANDIN) if on else 0)
    return (at("xa"), r.lda or r4(r.CA), at("xb"), r.ldb or r4(r.CB), at("ws"), r4(r.CB), r.B, wp.QH, wp.QW, wp.HA, wp.WA, wp.sa, wp.HB, wp.WB, wp.sb,
            r.CA, r.CB, wp.ntaps, wp.desc, r.nsplit, at("bsum", r.bsum), stream)


def _wgrad_taps(wp, B, a, b):
    """The contract of include/colddiff.h as a gather: per tap the rows (XA[pixA(m, tap)] [M][CA], XB[pixB(m, tap)] [M][CB]) of NHWC
    float64 a, b -- pixA = (qy sa + day, qx sa + dax), pixB = (qy sb + dby, qx sb + dbx), a row outside its image is zero."""
    M = B * wp.QH * wp.QW
    m = torch.arange(M)
    qx, qy, bi = m % wp.QW, (m // wp.QW) % wp.QH, m // (wp.QW * wp.QH)
    desc, out = list(wp.desc), []
    for t in range(wp.ntaps):
        day, dax, dby, dbx = desc[4 * t:4 * t + 4]
        ay, ax, by, bx = qy * wp.sa + day, qx * wp.sa + dax, qy * wp.sb + dby, qx * wp.sb + dbx
        bok = (by >= 0) & (by < wp.HB) & (bx >= 0) & (bx < wp.WB)
        aok = bok & (ay >= 0) & (ay < wp.HA) & (ax >= 0) & (ax < wp.WA)
        A = a[bi, ay.clamp(0, wp.HA - 1), ax.clamp(0, wp.WA - 1)] * aok[:, None]
        Bm = b[bi, by.clamp(0, wp.HB - 1), bx.clamp(0, wp.WB - 1)] * bok[:, None]
        out.append((A, Bm))
    return out


def _sp_wgrad_case(be, r):
    wp = wgrad_plan(r.kind, r.H, r.W, r.k, r.s, r.pad)
    B, CA, CB, k, KK, ns = r.B, r.CA, r.CB, r.k, r.k * r.k, r.nsplit
    lda, ldb, ldo = r.lda or r4(CA), r.ldb or r4(CB), r4(CB)
    M = B * wp.QH * wp.QW
    mps = _m_per_split(M, ns)
    sl = [(z * mps, min((z + 1) * mps, M)) for z in range(ns)]
    tag = "sp wgrad " + "-".join(map(str, r)) + f" (M={M}, {mps} pixels per slab, {sum(lo >= M for lo, _ in sl)} empty)"
    g = torch.Generator().manual_seed(CA * 17 + CB + ns + k + wp.QW)
    a, b = torch.randn(B, wp.HA, wp.WA, CA, generator=g), torch.randn(B, wp.HB, wp.WB, CB, generator=g)
    t = dict(xa=be.to(_padded(a, lda, 0, BIG)), xb=be.to(_padded(b, ldb, 0, BIG)), ws=nan_empty(be, ns, KK, CA, ldo))
    if r.bsum:
        t["bsum"] = nan_empty(be, ns, ldo)
    args = ws_args(r, {k_: P(v) for k_, v in t.items()}, be.stream())
    form = sp_wgrad_form(args)
    print(f"{tag}: form {form}")
    assert form == sp_wgrad_form(ws_args(r)), tag
    outs = [t["ws"]] + ([t["bsum"]] if r.bsum else [])
    got = twice(lambda: be.L.cdf_conv_wgrad_bf16(*args), outs)
    ws, bsum = got[0], (got[1] if r.bsum else None)

    # ---- float64: per tap and slab  A_hi^T (B_hi + B_lo) + A_lo^T B_hi  over the slab's pixels
    (ah, al), (bh, bl) = _split_trunc(a), _split_trunc(b)
    hi_taps, lo_taps = _wgrad_taps(wp, B, ah.double(), bh.double()), _wgrad_taps(wp, B, al.double(), bl.double())
    true_taps = _wgrad_taps(wp, B, a.double(), b.double())

    def sums(lo, hi):
        """([tap][CA][CB] sums over pixels lo .. hi-1, max ||terms||_2 over the outputs)"""
        v, sq = [], 0.0
        for (Ah, Bh), (Al, Bl) in zip(hi_taps, lo_taps):
            Ah, Bh, Al, Bl = Ah[lo:hi], Bh[lo:hi], Al[lo:hi], Bl[lo:hi]
            v.append(Ah.t() @ (Bh + Bl) + Al.t() @ Bh)
            sq = max(sq, ((Ah * Ah).t() @ (Bh * Bh + Bl * Bl) + (Al * Al).t() @ (Bh * Bh)).max().item())
        return torch.stack(v), math.sqrt(sq)
    worst = 0.0
    for z, (lo, hi) in enumerate(sl):
        if lo >= M:                                          # a slab without pixels is written as zeros
            assert bool((ws[z] == 0).all()) and (bsum is None or bool((bsum[z] == 0).all())), (tag, "empty slab", z)
            continue
        ref, norm = sums(lo, hi)
        e = K_SUM * U * math.sqrt(3 * (hi - lo)) * norm
        err = _dist(ws[z][..., :CB], ref)
        worst = max(worst, err / e)
        assert err <= e, (tag, "slab", z, err, e)
    print(f"{tag} slab by slab: worst error / bound = {worst:.3f}")
    ref, norm = sums(0, M)
    tot = ws[..., :CB].double().sum(0)
    check(f"{tag} sum of the slabs", tot, ref, K_SUM * U * math.sqrt(3 * M) * norm)
    assert bool((ws[..., CB:] == 0).all()) and not bool(torch.signbit(ws[..., CB:]).any()), (tag, "pad columns of the slabs must be +0")
    # ... the true weight gradient of the unsplit operands: the gather against torch's own, then the kernel against it
    true = torch.stack([A.t() @ Bm for A, Bm in true_taps])  # [tap][CA][CB]
    tref = _wgrad_ref64(r.kind, k, r.s, r.pad, _nchw(a.double(), CA), _nchw(b.double(), CB), CA, CB, "cpu")
    lay = lambda v: (v.permute(2, 1, 0) if r.kind == "conv_wgrad" else v.permute(1, 2, 0)).reshape(tref.shape)   # -> the parameter's layout
    assert _dist(lay(true), tref) <= 1e-12 * max(1.0, tref.abs().max().item()), (tag, "the gather reference is not the weight gradient")
    check(f"{tag} true float64 weight gradient", lay(tot), tref, 3e-5 * max(1.0, tref.abs().max().item()) * math.sqrt(M / 16))
    if r.bsum:                                               # row z = the column sums of tap 0's XB rows over slab z's pixels (fp32 values, unsplit)
        b0 = true_taps[0][1]
        for z, (lo, hi) in enumerate(sl):
            if hi > lo:
                check(f"{tag} bsum row {z}", bsum[z, :CB], b0[lo:hi].sum(0), sum_bound(b0[lo:hi], 0))
        assert bool((bsum[:, CB:] == 0).all()), (tag, "pad columns of bsum must be zero")
    return form


def _wgrad_rows():
    c1 = lambda B, n, CA, CB, ns, bsum, **kw: WS("conv_wgrad", B, n, n, CA, CB, 1, 1, 0, ns, bsum, **kw)
    rows = [
        # one tap.  QW = 4 (a 32-pixel step spans two images), B = 6: M = 96, three steps (an odd number) in one slab; five slabs of 32
        # (one step each) leave slabs 3 and 4 empty
        c1(6, 4, 128, 128, 1, 0), c1(6, 4, 128, 128, 5, 1), c1(6, 4, 256, 128, 5, 0, lda=384, ldb=512), c1(6, 4, 256, 256, 2, 1, lda=384, ldb=512),
        # QW = 5: M = 50 is no multiple of 32 (the m < m_hi guard decides): one slab of 32 + 18, two slabs 32 | 18, three 32 | 18 | none
        c1(2, 5, 136, 136, 1, 1), c1(2, 5, 128, 136, 2, 0, lda=132), c1(2, 5, 130, 70, 3, 1), c1(2, 5, 128, 128, 2, 1),
        # QW = 8: M = 128; three slabs 64 | 64 | none, four of one step
        c1(2, 8, 130, 70, 3, 1, lda=136, ldb=80), c1(2, 8, 136, 128, 4, 0), c1(2, 8, 384, 128, 1, 1), c1(2, 8, 128, 384, 3, 0, ldb=512),
        # QW = 36 (a step inside one row): M = 1296; seven slabs of 192 (six steps), the last one 144 pixels = four steps and a half
        c1(1, 36, 384, 128, 7, 1), c1(1, 36, 128, 136, 9, 0, lda=384),
    ]
    for kind, k, s, pad, sizes in (("conv_wgrad", 3, 1, 1, (4, 5, 8)), ("conv_wgrad", 4, 2, 1, (8, 10, 16)), ("convT_wgrad", 4, 2, 1, (4, 5, 8))):
        bs = int(kind == "conv_wgrad")                       # (the transposed plan reads XB at strided offsets: no bsum)
        n4, n5, n8 = sizes
        rows += [WS(kind, 6, n4, n4, 128, 128, k, s, pad, 5, bs), WS(kind, 2, n5, n5, 136, 256, k, s, pad, 2, 0, lda=144, ldb=384),
                 WS(kind, 2, n5, n5, 130, 70, k, s, pad, 1, bs), WS(kind, 2, n8, n8, 256, 136, k, s, pad, 3, bs, lda=384)]
    rows += [WS("conv_wgrad", 1, 36, 36, 128, 128, 3, 1, 1, 9, 1)]   # QW = 36 with taps: nine slabs, 8 of 160 pixels and one of 16
    # the pixel walk on 4 x 4 images with taps (a 32-pixel step: eight rows, two images).  B = 3, M = 48: slabs 32 | 16 | none, one step each
    # (the decode alone; a two-step slab would be all of M = 48).  B = 7, M = 112: slabs 64 | 48 | none, the second step of a slab comes out
    # of the advance, over several rows and an image boundary
    rows += [WS("conv_wgrad", 3, 4, 4, 136, 128, 3, 1, 1, 3, 1), WS("conv_wgrad", 7, 4, 4, 136, 128, 3, 1, 1, 3, 1)]
    return rows


WGRAD_ROWS = _wgrad_rows()


# ---------------------------------------------------------------------------------------------------------------------------------
# the tested forms; the forms the recordings reach
# ---------------------------------------------------------------------------------------------------------------------------------
def forms_of_gemm_rows():
    return {sp_gemm_form(gs_args(r)) for r in GEMM_ROWS}


def forms_of_wgrad_rows():
    return {sp_wgrad_form(ws_args(r)) for r in WGRAD_ROWS}


# The forms the recordings of test_gpu_invariance.py::test_coverage_guard reach: one bench step in bf16x3 and in bf16, one sampler step at
# B = 16 and one forward + backward pass of config 2's network.  The guard fails when a recording reaches a form no row has, and when a
# form listed here is no longer reached.  Every other tested form is one no recording reaches (taps, ragged tiles, K tails, the scalar
# epilogue, activations and multipliers, ...).
REACHED_SP_GEMM = {
    (1, '1tap', 'vec', '', 0, 0, 0, 'whole', 'whole', 0, 0, 0, 0),
    (1, '1tap', 'vec', 'br', 0, 0, 0, 'whole', 'whole', 0, 0, 0, 0),
    (3, '1tap', 'vec', '', 0, 0, 0, 'whole', 'half', 0, 0, 0, 0),
    (3, '1tap', 'vec', 'b', 0, 0, 0, 'whole', 'half', 0, 0, 0, 0),
    (3, '1tap', ('fast', 1), '', 0, 0, 0, 'whole', 'whole', 0, 0, 0, 0),
    (3, '1tap', ('fast', 1), '', 0, 0, 0, 'whole', 'whole', 0, 1, 0, 0),
    (3, '1tap', ('fast', 1), 'b', 0, 0, 0, 'whole', 'whole', 0, 0, 0, 0),
    (3, '1tap', ('fast', 1), 'b', 0, 0, 0, 'whole', 'whole', 0, 1, 0, 0),
    (3, '1tap', ('fast', 2), 'br', 0, 0, 0, 'whole', 'whole', 0, 0, 0, 0),
    (3, '1tap', ('fast', 2), 'br', 0, 0, 0, 'whole', 'whole', 0, 0, 1, 1),
    (3, '1tap', ('fast', 6), '', 0, 0, 1, 'whole', 'whole', 0, 0, 0, 0),
}
REACHED_SP_WGRAD = {
    ('1tap', 'whole', 'whole', '', 0, 1, 0),
    ('1tap', 'whole', 'whole', '', 1, 0, 0),
    ('1tap', 'whole', 'whole', '', 1, 1, 0),
    ('1tap', 'whole', 'whole', 'a', 1, 1, 0),
    ('1tap', 'whole', 'whole', 'b', 1, 0, 0),
    ('1tap', 'whole', 'whole', 'b', 1, 1, 0),
}
# ... with a row, at the small shapes above, for each reached form the crossed tables lack:
_one = lambda B, n, cin, cout, *a, **kw: GS("conv_fwd", B, n, n, cin, cout, 1, 1, 0, *a, **kw)
GEMM_ROWS += [r._replace(split=s) for r in (
    _one(2, 8, 64, 128, "", xld=96, xoff=16),                # x a slice, y contiguous (the attention block's q / k / v slices)
    _one(2, 16, 64, 256, "b", xld=96),
    _one(2, 8, 64, 128, "br", yld=256, ldr=128),             # y pitched, the residual contiguous, on the fast form
) for s in (3, 1)]
_c1 = lambda B, n, CA, CB, ns, bsum, **kw: WS("conv_wgrad", B, n, n, CA, CB, 1, 1, 0, ns, bsum, **kw)
WGRAD_ROWS += [_c1(6, 4, 128, 256, 5, 0), _c1(2, 8, 128, 128, 4, 1), _c1(6, 4, 256, 128, 5, 1, lda=384), _c1(2, 8, 128, 128, 2, 1, ldb=512),
               _c1(2, 8, 128, 256, 3, 1, ldb=512)]


def test_form_tables():
    """The tables keep what they were built for: every geometry, K form, N class and M edge with both splits; every reached operand set
    on the fast and on the generic form; every weight-gradient plan class with ragged tiles, pitched operands, empty slabs and ragged
    steps; the forms flagged as reached are tested forms; some tested form is unreached."""
    for split in (3, 1):
        rows = [r for r in GEMM_ROWS if r.split == split]
        assert {(r.kind, r.k, r.s, r.pad) for r in rows} == {g[:4] for g in _GEOM}
        assert {r.Cin for r in rows if r.k == 1} >= set(_CINS) and {r.Cout for r in rows} >= set(_COUTS)
        forms = {sp_gemm_form(gs_args(r)) for r in rows}
        paths = {(f[2], f[3], f[6]) for f in forms}
        fast = {(("fast", 1), "", 0), (("fast", 1), "b", 0), (("fast", 2), "br", 0), (("fast", 6), "", 1), (("fast", 1), "s", 0)}
        assert (paths >= fast) if split == 3 else not any(p[0] != "vec" and p[0] != "scalar" for p in paths), paths
        assert paths >= {("vec", o, a_) for o, a_ in _EPI_REACHED} | {("scalar", "b", 0), ("scalar", "br", 0), ("vec", "bs", 0)}, paths
        assert {(f[4], f[5]) for f in forms} >= {(0, 0), (1, 0), (2, 0), (3, 0), (0, 1), (0, 3)}
        assert {f[7] for f in forms} == {"whole", "ragged"} and {f[8] for f in forms} == {"whole", "half", "ragged"} and {f[9] for f in forms} == {0, 1}
        assert {f[10:] for f in forms} >= {(0, 0, 0), (1, 1, 0), (1, 1, 1), (0, 1, 1), (0, 0, 1)}
    assert sum(1 for r in GEMM_ROWS if r.B * r.H * r.W == 1296 and r.Cout == 136) == 2
    tw = forms_of_wgrad_rows()
    for plan in ("1tap", ("conv", 9, 1), ("conv", 16, 2), ("convT", 16)):
        fs = {f[1:] for f in tw if f[0] == plan}
        assert {f[:2] for f in fs} >= {("whole", "whole"), ("ragged", "ragged")} and {f[2] for f in fs} >= {"", "a", "ab"}, (plan, fs)
        assert {f[3] for f in fs} == ({0, 1} if plan[0] != "convT" else {0}) and {f[4] for f in fs} == {0, 1} and {f[5] for f in fs} == {0, 1}, (plan, fs)
    tg = forms_of_gemm_rows()
    assert REACHED_SP_GEMM <= tg and REACHED_SP_WGRAD <= tw
    assert (tg - REACHED_SP_GEMM) and (tw - REACHED_SP_WGRAD)


def test_recorded_sp_forms_dry(monkeypatch):
    """The recordings of test_gpu_invariance.py::test_coverage_guard without a GPU, the technique of
    test_gemm_f32_forms.py::test_recorded_forms_dry: the same four runs at their real shapes on CPU tensors with every launching entry
    point replaced by a stub that returns 0.  Which entry point is called with which arguments is decided by the Python layer from
    shapes and modes alone: every recorded form of this pair must be a tested form, and every form flagged as reached must be recorded
    (the guard's two assertions)."""
    import ctypes
    import types
    from colddiff import _lib, runtime as rt
    from emu_util import emu_lib
    import test_gpu_invariance as gi
    import test_gpu_parity2 as p2
    real, stub = emu_lib(), types.SimpleNamespace()
    for name, (restype, _) in real.protos.items():
        launches = restype is ctypes.c_int and not _lib._QUERY.search(name) and name != "cdf_gemm_tuning_default"
        setattr(stub, name, (lambda *a: 0) if launches else getattr(real, name))
    monkeypatch.setattr(rt, "_lib_override", stub)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    monkeypatch.setattr(gi, "DEV", "cpu")
    monkeypatch.setattr(p2, "DEV", "cpu")
    monkeypatch.setattr(gi, "_GEMM_FAMILY", gi._SP_GEMM)
    _, _, calls = gi._guard_calls(p2.bench_step_inputs())
    reached_g = {sp_gemm_form(a) for _, n, a in calls if n == "cdf_conv_gemm_bf16"}
    reached_w = {sp_wgrad_form(a) for _, n, a in calls if n == "cdf_conv_wgrad_bf16"}
    print("in-kernel-split GEMM forms reached:", *sorted(reached_g, key=repr), sep="\n    ")
    print("in-kernel-split weight-gradient forms reached:", *sorted(reached_w, key=repr), sep="\n    ")
    assert reached_g and reached_w
    assert reached_g <= forms_of_gemm_rows(), sorted(reached_g - forms_of_gemm_rows(), key=repr)
    assert reached_w <= forms_of_wgrad_rows(), sorted(reached_w - forms_of_wgrad_rows(), key=repr)
    assert REACHED_SP_GEMM <= reached_g and REACHED_SP_WGRAD <= reached_w, (sorted(REACHED_SP_GEMM - reached_g, key=repr),
                                                                          sorted(REACHED_SP_WGRAD - reached_w, key=repr))


# ---------------------------------------------------------------------------------------------------------------------------------
# the tests over the case tables (both backends)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", GEMM_ROWS, ids=lambda r: "-".join(map(str, r)))
def test_sp_gemm_forms(be, r):
    _sp_gemm_case(be, r)


@pytest.mark.parametrize("r", WGRAD_ROWS, ids=lambda r: "-".join(map(str, r)))
def test_sp_wgrad_plans_and_splits(be, r):
    _sp_wgrad_case(be, r)
