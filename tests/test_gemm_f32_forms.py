"""The exact-fp32 MFMA GEMM pair of csrc/k_conv.hip -- conv_igemm_kernel (cdf_conv_gemm, cdf_conv_gemm_io: forward, data gradient, every
one-tap batched product of the linear-attention block) and conv_wgrad_kernel (cdf_conv_wgrad) -- in every tile and batched form the product
launches.  Conventions of test_kernels_production.py / test_gemm_production.py: every output, workspace and bsum NaN-poisoned before each
of two launches that must agree bit for bit, a float64 reference, a derived bound, every worst error / bound printed.

Shapes are the smallest that reach the hazard, not the workload's: all addressing in both kernels is 64-bit, so what can go wrong is a
tile edge, the K-chunk wrap, the block swizzle (cdf_xcd_swizzle with more than 8 tiles and a remainder: 22 blocks at Cout = 136, M = 1296)
and the batch / head / slab indexing.

Reference: the same operation in float64 on the CPU from the very fp32 operands the kernel gets (F.conv2d / F.conv_transpose2d /
torch.nn.grad.conv2d_weight through test_gemm_production's helpers, matrix products for the one-tap forms), then the epilogue in float64
(test_gemm_production._epilogue64).  The operands are not split here, so this is also the true result.  No cdf_* function is the reference.

Bound: test_kernels_production's model, no new constant:  K_SUM 2^-24 sqrt(n) max ||terms||_2  with n = taps x Cin for outputs and n = the
pixels of the slab (or of the sum) for weight gradients, plus one fp32 rounding per epilogue operand magnitude and the Lipschitz / erf
terms of _epilogue64; a bf16 plane or bf16 pre-activation adds bf16's own 2^-8 |v|.

Poison: elements a call does not own must still hold the poison bit pattern afterwards -- the columns >= Cout of a pitched y, the
neighbouring channels of a slice target, the other heads' columns, the rows of other batch entries; the pad columns CB .. ldo-1 of weight-
gradient slabs and bsum rows are exact zeros (the kernel writes them); a slab without pixels is written as zeros.
Inputs: whatever a launch does not read is NaN (the columns beyond the last channel quad of a pitched x / xa / xb, the other tensors of
a (q|k|v) row); the pad channels C .. r4(C)-1 inside the last quad hold 1e30 -- the kernels load whole quads and rely on zero weight
rows / unsaved output rows (include/colddiff.h: they must be finite).  No finite pad value changes a result.

Forms: f32_gemm_form / f32_wgrad_form are pure functions of a call's argument tuple; every row builds its tuple through one helper
(gr_args / br_args / wr_args / wb_args), and the tested forms are those functions applied to the rows (forms_of_gemm_rows,
forms_of_wgrad_rows), so the tables and the set of tested forms cannot drift apart; each case asserts that its real argument tuple has
the form its stand-in tuple claims.  test_gpu_invariance.py::test_coverage_guard holds the recorded calls of the bench step, the sampler
step and config 2's pass against them; test_recorded_forms_dry makes the same recording without a GPU (launches stubbed out).
The recordings reach (REACHED_GEMM / REACHED_WGRAD, 22 + 11 forms): only one-tap geometries and the 3 x 3 stride-1 convolution with its
data gradient; every batched launch of the linear-attention block (heads, shared A / W, b_trans, bias + res with row-offset addressing,
the bf16 plane without y); the scalar epilogue at the 3-channel layers; of the weight gradient every tile but <64,64> at CA, CB <= 32,
one-tap / 3 x 3 / head-split plans, [split][batch] slabs with bsum.  No strided or transposed geometry, no activation, multiplier or
accumulate epilogue reaches this pair from those four runs (the pre-split family takes those layers).

Worst error / bound per group (160 cases; the simulator runs the module in 1.7 minutes in one process, the MI355X in 3 s):
                                            simulator    MI355X
    single launch      y                    0.73         0.73
                       pre-activation       0.79         0.79
                       bf16 plane           0.65         0.65
    batched call sites y / bf16 plane       0.57         0.57
    weight gradient    sum of the slabs     0.58         0.58
                       slab by slab         0.55         0.55
                       bsum rows            0.28         0.28
The two columns agree because the results do: fp32 MFMA accumulation in a fixed order is what the simulator executes too, and of the 379
printed errors only two differ between the backends (both through GELU' of the multiplier: 0.197 against 0.209 at the larger one).
"""
import ctypes
import math
from typing import NamedTuple

import pytest
import torch

from colddiff import convdesc as cd
from poison import nan_empty
from test_kernels import P, r4
from test_kernels_production import K_SUM, U, check, sum_bound, twice
from test_gemm_production import _conv64, _dist, _epilogue64, _khw, _nchw, _wgrad_ref64, gemm_plan, tap_mask, wgrad_plan

BIG = 1.0e30                                                 # the finite value of in-quad pad channels (include/colddiff.h: cdf_conv_gemm)
NAN32 = torch.tensor(float("nan")).view(torch.int32).item()  # the poison bit patterns of tests/poison.py
NAN16 = 0x7FC0


# ---------------------------------------------------------------------------------------------------------------------------------
# kernel forms: pure functions of a call's argument tuple (a recorded one, or the one a case row builds)
# ---------------------------------------------------------------------------------------------------------------------------------
def _addr(v):
    return 0 if v is None else int(getattr(v, "value", v) or 0)


def f32_gemm_form(name, a):
    """The form of a cdf_conv_gemm / cdf_conv_gemm_io call, from its arguments alone (csrc/k_conv.hip: cdf_conv_gemm_io):
    (tile, b_trans, geometry, batch class, shared operands, epi_follow, operand letters, act, mul_mode, accumulate, vec, io_bf16, y, y_hi).
    geometry: '1tap', or (nphase, taps of phase 0, os, is, first tap's dy, dx) -- the last two tell the one-sided padding of config 2's
    strided 3 x 3 from the symmetric one;  shared operands: 'A' / 'W' the outer batch stride of x / w is 0, 'a' / 'w' the inner one."""
    io = name.endswith("_io")
    ldy, Cout, os_, is_, nphase, desc = a[5], a[12], a[15], a[16], a[17], list(a[18])
    y, bias, sbias, ld_sb, res, ldr, pre, ldp, mul, ldm = _addr(a[4]), _addr(a[19]), _addr(a[20]), a[21], _addr(a[22]), a[23], _addr(a[24]), a[25], \
        _addr(a[26]), a[27]
    act, mm, acc, bt, batch, x_bs, w_bs, y_bs, batch2, x_bs2, w_bs2, y_bs2 = a[28:40]
    io_bf, y_hi = (a[40], _addr(a[41])) if io else (0, 0)
    tile = "128x32" if Cout <= 32 else ("256x64" if Cout <= 64 else "128x128")
    geom = "1tap" if (nphase == 1 and desc[2] == 1) else (nphase, desc[2], os_, is_, desc[3], desc[4])
    batched = batch * batch2 > 1
    bclass = "none" if not batched else ("outer" if batch2 == 1 else "outer+inner")
    shared = "".join(c for c, on in (("A", batch > 1 and x_bs == 0), ("W", batch > 1 and w_bs == 0), ("a", batch2 > 1 and x_bs2 == 0),
                                     ("w", batch2 > 1 and w_bs2 == 0)) if on)
    ops = "".join(c for c, v in zip("bsrpm", (bias, sbias, res, pre, mul)) if v)
    ptrs = y | bias | sbias | res | pre | mul
    pitches = ldy | (ld_sb if sbias else 0) | (ldr if res else 0) | (ldp if pre else 0) | (ldm if mul else 0)
    vec = int(Cout % 4 == 0 and ptrs & 15 == 0 and pitches & 3 == 0 and y_bs % 4 == 0 and y_bs2 % 4 == 0)
    follow = int(batched and bool(res or pre or mul))
    return (tile, int(bool(bt)), geom, bclass, shared, follow, ops, act, mm, acc, vec, io_bf, int(bool(y)), int(bool(y_hi)))


def f32_wgrad_form(a):
    """The form of a cdf_conv_wgrad call: (tile, dispatch class, plan class, batched, o_bs < 0, bsum).
    tile: the (BMC, BNC) of the conv_wgrad_kernel instantiation;  dispatch class: (CA <= 32, CA <= 64, CB <= 32, CB <= 64) -- cdf_conv_wgrad
    has seven dispatch branches over six instantiations (<64,64> serves CA, CB <= 32 and 32 < CA, CB <= 64), the class tells the two apart;
    plan class: '1tap', 'heads' (the taps are heads: ops._headsplit_plan), ('convT', taps) when XB is the strided side, ('conv', taps,
    stride) otherwise."""
    sa, sb, CA, CB, ntaps = a[11], a[14], a[15], a[16], a[17]
    desc, batch, o_bs, bsum = list(a[18])[:4 * ntaps], a[20], a[23], _addr(a[24])
    if CA <= 32:
        tile = (64, 64) if CB <= 32 else (32, 128)
    elif CB <= 32:
        tile = (128, 32)
    elif CA <= 64 and CB <= 64:
        tile = (64, 64)
    elif CA <= 64:
        tile = (64, 128)
    else:
        tile = (128, 64) if CB <= 64 else (128, 128)
    taps = [tuple(desc[4 * t:4 * t + 4]) for t in range(ntaps)]
    if ntaps == 1:
        plan = "1tap"
    elif taps == [(h, 0, h, 0) for h in range(ntaps)]:
        plan = "heads"
    else:
        plan = ("convT", ntaps) if sb > 1 else ("conv", ntaps, sa)
    return (tile, (CA <= 32, CA <= 64, CB <= 32, CB <= 64), plan, int(batch > 1), int(o_bs < 0), int(bool(bsum)))


def _poison_outside(t, lo, hi):
    """Every element of host tensor t outside columns lo .. hi-1 of its last dimension still holds the poison bit pattern."""
    bits, pat = (t.view(torch.int32), NAN32) if t.dtype == torch.float32 else (t, NAN16)
    return bool((bits[..., :lo] == pat).all() and (bits[..., hi:] == pat).all())


def _padded(t, ld, off=0, quad_pad=None):
    """t [..., C] inside a [..., ld] buffer at channel offset off: NaN everywhere else, except the pad channels of t's last channel quad
    (quad_pad: finite -- the kernels load whole quads and rely on zero weights / unsaved rows for them)."""
    C = t.shape[-1]
    buf = torch.full(t.shape[:-1] + (ld,), NAN16 if t.dtype == torch.int16 else float("nan"), dtype=t.dtype)
    buf[..., off:off + C] = t
    if quad_pad is not None:
        buf[..., off + C:off + r4(C)] = quad_pad
    return buf


def _bf(t):
    """(int16 bit pattern, the float32 values it holds) of t rounded to bf16."""
    b = t.bfloat16()
    return b.view(torch.int16), b.float()


# ---------------------------------------------------------------------------------------------------------------------------------
# conv_igemm_kernel, single launch
# ---------------------------------------------------------------------------------------------------------------------------------
class GR(NamedTuple):
    """kind / H / W / k / s / pad: the arguments of test_gemm_production.gemm_plan (H, W: the convolution's own input size); Cin, Cout: K and N
    of the GEMM; ops: letters of the epilogue operands (b bias, s per-sample bias, r residual, p pre-activation output, m multiplier);
    io: io_bf16 bits; yhi: a bf16 output plane; has_y: an fp32 output; x / y: channel slices [off, off + C) of buffers of pitch ld
    (0: r4(C))."""
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
    io: int = 0
    yhi: int = 0
    has_y: int = 1
    xld: int = 0
    xoff: int = 0
    yld: int = 0
    yoff: int = 0


_STANDIN = 1 << 20                                           # a 16-byte-aligned stand-in address (form of a row without buffers)


def gr_args(r, ad=None, stream=0):
    """(entry point, argument tuple) of a GR row; ad: the buffers' addresses (None: aligned stand-ins, for the form alone)."""
    pl = gemm_plan(r.kind, r.H, r.W, r.k, r.s, r.pad)
    ldx, ldo, ldh = r.xld or r4(r.Cin), r4(r.Cout), r4(r.Cout) + 8
    ldy = (r.yld or ldo) if r.has_y else ldh
    at = lambda key, on: ((ad[key] if ad else _STANDIN) if on else 0)
    io = bool(r.io or r.yhi)
    a = (at("x", 1) + 4 * r.xoff, ldx, at("w", 1), ldo, at("y", r.has_y) + (4 * r.yoff if r.has_y else 0), ldy, r.B, pl.H, pl.W, r.Cin, pl.OH, pl.OW,
         r.Cout, pl.QH, pl.QW, pl.os, pl.istride, pl.nphase, pl.desc, at("bias", "b" in r.ops), at("sbias", "s" in r.ops), ldo if "s" in r.ops else 0,
         at("res", "r" in r.ops), ldo, at("pre", "p" in r.ops), ldo, at("mul", "m" in r.ops), ldo, r.act, r.mm, r.acc, 0, 1, 0, 0, 0, 1, 0, 0, 0)
    if io:
        a += (r.io, at("yhi", r.yhi), ldh if r.yhi else 0)
    return ("cdf_conv_gemm_io" if io else "cdf_conv_gemm"), a + (stream,)


def _max_taps(pl):
    n, p = 0, 0
    for _ in range(pl.nphase):
        n, p = max(n, pl.desc[p + 2]), p + 3 + 3 * pl.desc[p + 2]
    return n


def _igemm_case(be, r):
    pl = gemm_plan(r.kind, r.H, r.W, r.k, r.s, r.pad)
    B, Cin, Cout, k = r.B, r.Cin, r.Cout, r.k
    kh, kw = _khw(k)                                         # (k: an int, a (kh, kw) pair or a TapSubset -- test_gemm_production.gemm_plan)
    KK = kh * kw
    ldx, ldo, ldh = r.xld or r4(Cin), r4(Cout), r4(Cout) + 8
    ldy = r.yld or ldo
    tag = "igemm " + "-".join(map(str, r[:20]))
    g = torch.Generator().manual_seed(Cin * 131 + Cout * 7 + kh + r.H)
    rn = lambda *s_: torch.randn(*s_, generator=g)
    x = rn(B, pl.H, pl.W, Cin)
    gather = r.kind in ("conv_fwd", "convT_dgrad")
    w = rn(*((Cout, Cin, kh, kw) if gather else (Cin, Cout, kh, kw))) / math.sqrt(Cin * KK)
    wp = torch.zeros(KK, Cin, ldo)                           # [tap][Cin][ldw], pad columns zero (cdf_pack_weight's contract)
    wp[..., :Cout] = (w.permute(2, 3, 1, 0) if gather else w.permute(2, 3, 0, 1)).reshape(KK, Cin, Cout)
    w = tap_mask(w, k)                                       # (a tap subset: every tap is packed, the reference has the absent ones zeroed)
    osh = (B, pl.OH, pl.OW)
    t, o32, ad = {}, {}, {}
    t["x"], t["w"] = be.to(_padded(x, ldx, r.xoff, BIG)), be.to(wp)
    if "b" in r.ops:
        o32["bias"] = rn(Cout)
        t["bias"] = be.to(o32["bias"])
    if "s" in r.ops:
        o32["sbias"] = rn(B, Cout)
        t["sbias"] = be.to(_padded(o32["sbias"], ldo))
    for key, letter, bit in (("res", "r", 1), ("mul", "m", 4)):
        if letter in r.ops:
            v = rn(*osh, Cout)
            if r.io & bit:
                bits, v = _bf(v)
                t[key] = be.to(_padded(bits, ldo))
            else:
                t[key] = be.to(_padded(v, ldo))
            o32[key] = v
    y0 = rn(*osh, Cout) if r.acc else None
    y0d = be.to(_padded(y0, ldy, r.yoff)) if r.acc else None
    if r.has_y:
        t["y"] = nan_empty(be, *osh, ldy)
    if "p" in r.ops:
        t["pre"] = nan_empty(be, *osh, ldo, dtype=torch.int16 if r.io & 2 else torch.float32)
    if r.yhi:
        t["yhi"] = nan_empty(be, *osh, ldh, dtype=torch.int16)
    name, args = gr_args(r, {k_: P(v) for k_, v in t.items()}, be.stream())
    print(f"{tag}: form {f32_gemm_form(name, args)}")
    assert f32_gemm_form(name, args) == f32_gemm_form(*gr_args(r)), (tag, "the launch is not the form the table claims (pointer alignment)")
    fn = getattr(be.L, name)

    def launch():
        if r.acc:
            t["y"].copy_(y0d)                                # (accumulate reads y: its previous contents are an input)
        fn(*args)
    names = [n for n in ("y", "pre", "yhi") if n in t]
    got = dict(zip(names, twice(launch, [t[n] for n in names])))

    x64, w64 = _nchw(x.double(), Cin), w.double()
    cv = lambda a_, b_: _conv64(r.kind, a_, b_, k, r.s, r.pad, (pl.OH, pl.OW))
    v = cv(x64, w64)
    e0 = K_SUM * U * math.sqrt(_max_taps(pl) * Cin) * cv(x64 * x64, w64 * w64).max().sqrt().item()
    n64 = lambda key: None if key not in o32 else _nchw(o32[key].double(), Cout)
    o = dict(bias=None if "bias" not in o32 else o32["bias"].double(), sbias=None if "sbias" not in o32 else o32["sbias"].double(),
             res=n64("res"), mul=n64("mul"), y0=None if y0 is None else _nchw(y0.double(), Cout), pre="p" in r.ops)
    yr, prer, e_y, e_pre = _epilogue64(v, e0, o, r.act, r.mm, False)
    if r.has_y:
        check(f"{tag} y", _nchw(got["y"][..., r.yoff:], Cout), yr, e_y)
        assert _poison_outside(got["y"], r.yoff, r.yoff + Cout), (tag, "y: an element outside the output's channels changed")
    if "p" in r.ops:
        gp = got["pre"].view(torch.bfloat16) if r.io & 2 else got["pre"]
        check(f"{tag} pre", _nchw(gp, Cout), prer, e_pre + (2.0 ** -8 * prer.abs().max().item() if r.io & 2 else 0.0))
        assert _poison_outside(got["pre"], 0, Cout), (tag, "pre: a pad column changed")
    if r.yhi:
        # the plane holds bf16(v): 8 significant bits, half an ulp <= 2^-8 |v| (test_gemm_production._gemm_case)
        check(f"{tag} y_hi", _nchw(got["yhi"].view(torch.bfloat16), Cout), yr, e_y + 2.0 ** -8 * yr.abs().max().item())
        assert _poison_outside(got["yhi"], 0, Cout), (tag, "y_hi: a pad column changed")
        if r.has_y:                                          # ... and next to an fp32 output, that output rounded to nearest even, bit for bit
            assert torch.equal(got["yhi"][..., :Cout], got["y"][..., r.yoff:r.yoff + Cout].bfloat16().view(torch.int16)), tag


# geometry: (kind, k, s, pad, size of the convolution's input for a 36 x 36 / a 13 x 13 GEMM row grid)
_GEOM = [("conv_fwd", 1, 1, 0, 36, 13), ("conv_fwd", 3, 1, 1, 36, 13), ("conv_fwd", 4, 2, 1, 72, 26), ("conv_fwd", 3, 2, -1, 72, 26),
         ("convT_fwd", 4, 2, 1, 36, 13), ("conv_dgrad", 4, 2, 1, 72, 26), ("convT_dgrad", 4, 2, 1, 36, 13)]
# K: (Cin, x pitch, x channel offset): 16 + 16 + 8 per tap (the chunk wrap), exactly one chunk, 3 of a quad, a slice of a 32-wide buffer
_KS = [(40, 0, 0), (16, 0, 0), (3, 4, 0), (20, 32, 4)]
# epilogue operand sets of the product: (ops, act, mul_mode, accumulate, io_bf16, y_hi, has_y)
_EPI_F32 = [("", 0, 0, 0, 0, 0, 1), ("b", 0, 0, 0, 0, 0, 1), ("bsp", 1, 0, 0, 0, 0, 1), ("br", 0, 0, 0, 0, 0, 1), ("m", 0, 1, 0, 0, 0, 1),
            ("m", 0, 2, 0, 0, 0, 1), ("m", 0, 3, 0, 0, 0, 1), ("", 0, 0, 1, 0, 0, 1), ("", 3, 0, 1, 0, 0, 1)]
_EPI_IO = [("br", 0, 0, 0, 1, 0, 1), ("bp", 1, 0, 0, 2, 0, 1), ("m", 0, 1, 0, 4, 0, 1), ("b", 0, 0, 0, 0, 1, 1), ("br", 0, 0, 0, 1, 1, 0)]


def _igemm_rows():
    """Every epilogue set on every tile (the typed ones need the vector epilogue), and with each tile every geometry, K form and M."""
    rows = []
    for ti, (couts, epis) in enumerate((((24, 32), _EPI_F32 + _EPI_IO), ((56,), _EPI_F32 + _EPI_IO), ((136,), _EPI_F32 + _EPI_IO), ((3, 30), _EPI_F32))):
        for i, e in enumerate(epis):
            kind, k, s, pad, big, small = _GEOM[(i + ti) % 7]
            cin, xld, xoff = _KS[(i + 2 * ti) % 4]
            one = (i + i // 4 + ti) % 2 == 0                 # B = 1, 36 x 36 rows (11 / 6 row tiles) or B = 2, 13 x 13 (a ragged tile, two images)
            cout = couts[i % len(couts)]
            # a slice of a wider output buffer where the vector layout allows it (pitch and offset multiples of 4), for the scalar one too
            yld, yoff = ((r4(cout) + 12, 8) if i % 3 == 1 else (0, 0))
            rows.append(GR(kind, 1 if one else 2, big if one else small, big if one else small, cin, cout, k, s, pad, *e, xld, xoff, yld, yoff))
    return rows


IGEMM_ROWS = _igemm_rows()


# ---------------------------------------------------------------------------------------------------------------------------------
# conv_igemm_kernel, one-tap launches of ops._bgemm: batched, shared operands, b_trans, row-offset epilogue addressing
# ---------------------------------------------------------------------------------------------------------------------------------
class BR(NamedTuple):
    """y[z] = a[z] ([n x K], pitch lda) . w[z] ([K x ldw >= N], or with bt [N x ldw >= K]) + bias + res, z = outer * batch2 + inner.
    Each operand: buffer size, the pointer's offset into it, pitch, outer and inner batch stride (all in elements) -- the numbers of the
    ops.py call site named by `site`.  res: 0 none, 1 fp32, 2 bf16 (pitch ldr; addressed by output row: epi_follow);  ybf: no fp32 y, the
    result goes out as a bf16 plane."""
    site: str
    n: int
    K: int
    N: int
    bt: int
    batch: int
    batch2: int
    asz: int
    aoff: int
    lda: int
    a_bs: int
    a_bs2: int
    wsz: int
    woff: int
    ldw: int
    w_bs: int
    w_bs2: int
    ysz: int
    yoff: int
    ldy: int
    y_bs: int
    y_bs2: int
    bias: int = 0
    res: int = 0
    ldr: int = 0
    ybf: int = 0


def br_args(r, ad=None, stream=0):
    """(entry point, argument tuple) of a BR row, the way ops._bgemm writes the call."""
    at = lambda key, on=True: ((ad[key] if ad else _STANDIN) if on else 0)
    desc = cd.conv_fwd(1, r.n, 1, 1, 1, 0, 0, 0, 0).desc
    a = (at("a") + 4 * r.aoff, r.lda, at("w") + 4 * r.woff, r.ldw, 0 if r.ybf else at("y") + 4 * r.yoff, r.ldy, 1, 1, r.n, r.K, 1, r.n, r.N, 1, r.n, 1, 1, 1,
         desc, at("bias", r.bias), 0, 0, at("res", r.res), r.ldr, 0, 0, 0, 0, 0, 0, 0, r.bt, r.batch, r.a_bs, r.w_bs, r.y_bs, r.batch2, r.a_bs2, r.w_bs2,
         r.y_bs2)
    if r.ybf:
        return "cdf_conv_gemm_io", a + (1 if r.res == 2 else 0, at("y") + 2 * r.yoff, r.ldy, stream)
    return "cdf_conv_gemm", a + (stream,)


def _view(buf, off, rows, cols, ld):
    return buf.as_strided((rows, cols), (ld, 1), off)


def _bgemm_case(be, r):
    n, K, N = r.n, r.K, r.N
    tag = "bgemm " + r.site
    g = torch.Generator().manual_seed(n + 3 * K + 5 * N + r.batch2)
    a, w = torch.randn(r.asz, generator=g), torch.randn(r.wsz, generator=g) / math.sqrt(K)
    zs = [(zo, zi) for zo in range(r.batch) for zi in range(r.batch2)]
    aoff = lambda zo, zi: r.aoff + zo * r.a_bs + zi * r.a_bs2
    woff = lambda zo, zi: r.woff + zo * r.w_bs + zi * r.w_bs2
    yoff = lambda zo, zi: r.yoff + zo * r.y_bs + zi * r.y_bs2
    wshape = (N, K) if r.bt else (K, N)
    # what no GEMM of the launch reads is NaN; the pad channels of A's last quad are finite (loaded, times a zero weight row); the pad
    # columns of a [K][N] weight are zero (cdf_pack_weight's contract)
    for buf, off, shape, ld, pad in ((a, aoff, (n, K), r.lda, BIG), (w, woff, wshape, r.ldw, 0.0)):
        used, quad = torch.zeros(buf.numel(), dtype=torch.bool), torch.zeros(buf.numel(), dtype=torch.bool)
        for z in zs:
            _view(used, off(*z), shape[0], shape[1], ld).fill_(True)
            _view(quad, off(*z), shape[0], r4(shape[1]), ld).fill_(True)
        buf[~quad] = float("nan")
        buf[quad & ~used] = pad
    bias = torch.randn(N, generator=g) if r.bias else None
    rows_y = r.ysz // r.ldy
    res = res32 = None
    if r.res:
        res32 = torch.randn(rows_y * r.ldr, generator=g)
        res, res32 = _bf(res32) if r.res == 2 else (res32, res32)
    t = dict(a=be.to(a), w=be.to(w), y=nan_empty(be, r.ysz, dtype=torch.int16 if r.ybf else torch.float32))
    if r.bias:
        t["bias"] = be.to(bias)
    if r.res:
        t["res"] = be.to(res)
    name, args = br_args(r, {k_: P(v) for k_, v in t.items()}, be.stream())
    form = f32_gemm_form(name, args)
    print(f"{tag}: form {form}")
    assert form == f32_gemm_form(*br_args(r)), (tag, "the launch is not the form the table claims (pointer alignment)")
    fn = getattr(be.L, name)
    got = twice(lambda: fn(*args), [t["y"]])[0]
    gv = got.view(torch.bfloat16).double() if r.ybf else got.double()
    a64, w64 = a.double(), w.double()
    owned = torch.zeros(r.ysz, dtype=torch.bool)
    worst = [0.0, 0.0]
    for zo, zi in zs:
        A = _view(a64, aoff(zo, zi), n, K, r.lda)
        Wm = _view(w64, woff(zo, zi), *wshape, r.ldw)
        Wm = Wm.t() if r.bt else Wm
        v = (A @ Wm).t()[None, :, :, None]                   # (as test_gemm_production._epilogue64 takes it: NCHW)
        e0 = K_SUM * U * math.sqrt(K) * ((A * A) @ (Wm * Wm)).max().sqrt().item()
        o = dict(bias=None if bias is None else bias.double())
        if r.res:                                            # addressed like y: from the tensor's own base, by the output row
            assert form[5] == 1 and (yoff(zo, zi) - r.yoff) % r.ldy == 0
            o["res"] = _view(res32.double(), (yoff(zo, zi) - r.yoff) // r.ldy * r.ldr, n, N, r.ldr).t()[None, :, :, None]
        yr, _, e, _ = _epilogue64(v, e0, o, 0, 0, False)
        if r.ybf:
            e += 2.0 ** -8 * yr.abs().max().item()           # bf16: 8 significant bits
        err = _dist(_view(gv, yoff(zo, zi), n, N, r.ldy), yr[0, :, :, 0].t())
        worst = [max(worst[0], err), max(worst[1], e)]
        assert err <= e, (tag, (zo, zi), err, e)
        assert not _view(owned, yoff(zo, zi), n, N, r.ldy).any(), "the row's own outputs overlap"
        _view(owned, yoff(zo, zi), n, N, r.ldy).fill_(True)
    print(f"{tag}: worst error {worst[0]:.3e} / bound {worst[1]:.3e} = {worst[0] / worst[1]:.3f}")
    bits = got if r.ybf else got.view(torch.int32)
    assert bool((bits[~owned] == (NAN16 if r.ybf else NAN32)).all()), (tag, "an element no GEMM of the launch owns changed")
    return form


def _bgemm_rows(B=3, n=70):
    rows = []
    for heads, bts in ((4, (0, 1)), (1, (0,))):
        HD = 32 * heads
        L3 = 3 * HD
        for bt in bts:                                       # ops._head_gemm: the v / dv slices (offset 2 HD) of (q|k|v) rows
            rows.append(BR(f"_head_gemm heads={heads} b_trans={bt}", n, 32, 32, bt, B, heads, B * n * L3, 2 * HD, L3, n * L3, 32,
                           B * heads * 1024, 0, 32, heads * 1024, 1024, B * n * L3, 2 * HD, L3, n * L3, 32))
    heads, HD = 4, 128
    for dim in (48, 136):
        ldw, LD = dim, dim + 16
        rows += [
            BR(f"_out_matrix dim={dim}", 32, 32, dim, 0, B, heads, B * heads * 1024, 0, 32, heads * 1024, 1024, HD * ldw, 0, ldw, 0, 32 * ldw,
               B * HD * ldw, 0, ldw, HD * ldw, 32 * ldw),
            BR(f"linattn_project dim={dim} (bias + res, y a channel slice)", n, HD, dim, 0, B, 1, B * n * 3 * HD, 0, 3 * HD, n * 3 * HD, 0,
               B * HD * ldw, 0, ldw, HD * ldw, 0, B * n * LD, 8, LD, n * LD, 0, bias=1, res=1, ldr=dim),
            BR(f"linattn_fold dim={dim} (bf16 stream: y NULL, bf16 res)", n, dim, dim, 0, B, 1, B * n * dim, 0, dim, n * dim, 0,
               B * dim * ldw, 0, ldw, dim * ldw, 0, B * n * (dim + 8), 0, dim + 8, n * (dim + 8), 0, bias=1, res=2, ldr=dim, ybf=1),
            BR(f"linattn_fold Nb dim={dim} (shared A)", dim, HD, dim, 0, B, 1, dim * 3 * HD, 0, 3 * HD, 0, 0, B * HD * ldw, 0, ldw, HD * ldw, 0,
               B * dim * ldw, 0, ldw, dim * ldw, 0),
            BR(f"linattn_fold_bwd dMb dim={dim} (shared A)", HD, dim, dim, 0, B, 1, 3 * HD * dim, 0, dim, 0, 0, B * dim * ldw, 0, ldw, dim * ldw, 0,
               B * HD * ldw, 0, ldw, HD * ldw, 0),
            BR(f"linattn_project_bwd dq dim={dim} (b_trans)", n, dim, HD, 1, B, 1, B * n * dim, 0, dim, n * dim, 0, B * HD * ldw, 0, ldw, HD * ldw, 0,
               B * n * 3 * HD, 0, 3 * HD, n * 3 * HD, 0),
            BR(f"_linattn_out_bwd raw dim={dim} (b_trans, heads)", 32, dim, 32, 1, B, heads, B * HD * ldw, 0, ldw, HD * ldw, 32 * ldw,
               HD * ldw, 0, ldw, 0, 32 * ldw, B * heads * 1024, 0, 32, heads * 1024, 1024),
            BR(f"linattn_fold_bwd dxn dim={dim} (b_trans)", n, dim, dim, 1, B, 1, B * n * dim, 0, dim, n * dim, 0, B * dim * ldw, 0, ldw, dim * ldw, 0,
               B * n * dim, 0, dim, n * dim, 0),
            BR(f"linattn_fold_bwd T dim={dim} (b_trans)", HD, dim, dim, 1, B, 1, B * HD * ldw, 0, ldw, HD * ldw, 0, B * dim * ldw, 0, ldw, dim * ldw, 0,
               B * HD * ldw, 0, ldw, HD * ldw, 0),
        ]
    C = 40                                                   # the generic helpers on slices of a (q|k|v) tensor [nb, n, 3 C]: strides 3 C n, pitch 3 C
    #                                                          (K = 40 with b_trans: the last 16-channel chunk of a weight row ends in the k slice's NaN neighbour)
    rows += [
        BR("bgemm_nt q k^T (slices, N = 70: scalar epilogue)", n, C, n, 1, B, 1, B * n * 3 * C, 0, 3 * C, n * 3 * C, 0, B * n * 3 * C, C, 3 * C, n * 3 * C, 0,
           B * n * r4(n), 0, r4(n), n * r4(n), 0),
        BR("bgemm_nn P v (K = 70 of pitch 72, v a slice)", n, n, C, 0, B, 1, B * n * r4(n), 0, r4(n), n * r4(n), 0, B * n * 3 * C, 2 * C, 3 * C, n * 3 * C, 0,
           B * n * C, 0, C, n * C, 0),
        # single launches of the two layouts of a Linear layer's weight [N = 100][K = 48]: read in place as [N][K] (b_trans), and as the
        # [1][Cin = 100][Cout = 48] "packed" weight of its data gradient (functions.py: Linear.backward)
        BR("Linear forward, weight in place (b_trans, single launch)", n, 48, 100, 1, 1, 1, n * 48, 0, 48, 0, 0, 100 * 48, 0, 48, 0, 0, n * 100, 0, 100, 0, 0),
        BR("Linear data gradient (single launch)", n, 100, 48, 0, 1, 1, n * 100, 0, 100, 0, 0, 100 * 48, 0, 48, 0, 0, n * 48, 0, 48, 0, 0),
    ]
    return rows


BGEMM_ROWS = _bgemm_rows()


# ---------------------------------------------------------------------------------------------------------------------------------
# conv_wgrad_kernel
# ---------------------------------------------------------------------------------------------------------------------------------
def _m_per_split(M, nsplit):
    return -(-(-(-M // nsplit)) // 16) * 16                  # (cdf_conv_wgrad: a slab's pixel count is rounded up to the kernel's K step)


class WR(NamedTuple):
    """A convolution's weight gradient (batch = 1): kind / H / W / k / s / pad as in test_gemm_production.wgrad_plan."""
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


def wr_args(r, ad=None, stream=0):
    wp = wgrad_plan(r.kind, r.H, r.W, r.k, r.s, r.pad)
    at = lambda key, on=True: ((ad[key] if ad else _STANDIN) if on else 0)
    return (at("xa"), r4(r.CA), at("xb"), r4(r.CB), at("ws"), r4(r.CB), r.B, wp.QH, wp.QW, wp.HA, wp.WA, wp.sa, wp.HB, wp.WB, wp.sb, r.CA, r.CB,
            wp.ntaps, wp.desc, r.nsplit, 1, 0, 0, 0, at("bsum", r.bsum), stream)


def _check_slabs(tag, ws, bsum, slabs, bcols, CB, ldo):
    """ws [nslab][taps][CA][ldo] (host) against the float64 partial sums `slabs` [nslab][taps][CA][CB] with the bounds e [nslab] (a slab
    without pixels: zeros, bound 0); bsum [nslab][ldo] against bcols = (sums [nslab][CB], bounds); pad columns CB .. ldo-1 exact zeros."""
    ref, e = slabs
    for z in range(ref.shape[0]):
        err = _dist(ws[z][..., :CB], ref[z])
        assert err <= e[z], (tag, "slab", z, err, e[z])
    worst = max((_dist(ws[z][..., :CB], ref[z]) / e[z] for z in range(ref.shape[0]) if e[z] > 0), default=0.0)
    print(f"{tag}: slab by slab, worst error / bound = {worst:.3f}")
    assert bool((ws[..., CB:] == 0).all()) and not bool(torch.signbit(ws[..., CB:]).any()), (tag, "pad columns of the slabs must be +0")
    if bsum is not None:
        bref, be_ = bcols
        for z in range(bref.shape[0]):
            err = _dist(bsum[z, :CB], bref[z])
            assert err <= be_[z], (tag, "bsum row", z, err, be_[z])
        assert bool((bsum[:, CB:] == 0).all()), (tag, "pad columns of bsum must be zero")


def _wgrad_conv_case(be, r):
    wp = wgrad_plan(r.kind, r.H, r.W, r.k, r.s, r.pad)
    B, CA, CB, k, KK, ns = r.B, r.CA, r.CB, r.k, r.k * r.k, r.nsplit
    M, ldo = B * wp.QH * wp.QW, r4(CB)
    mps = _m_per_split(M, ns)
    tag = "wgrad " + "-".join(map(str, r[:11])) + f" (M={M}, {mps} pixels per slab, {ns - -(-M // mps)} empty)"
    g = torch.Generator().manual_seed(CA * 17 + CB + ns + k)
    a, b = torch.randn(B, wp.HA, wp.WA, CA, generator=g), torch.randn(B, wp.HB, wp.WB, CB, generator=g)
    t = dict(xa=be.to(_padded(a, r4(CA), 0, BIG)), xb=be.to(_padded(b, r4(CB), 0, BIG)), ws=nan_empty(be, ns, KK, CA, ldo))
    if r.bsum:
        t["bsum"] = nan_empty(be, ns, ldo)
    args = wr_args(r, {k_: P(v) for k_, v in t.items()}, be.stream())
    print(f"{tag}: form {f32_wgrad_form(args)}")
    assert f32_wgrad_form(args) == f32_wgrad_form(wr_args(r)), tag
    outs = [t["ws"]] + ([t["bsum"]] if r.bsum else [])
    got = twice(lambda: be.L.cdf_conv_wgrad(*args), outs)
    ws, bsum = got[0], (got[1] if r.bsum else None)
    a64, b64 = _nchw(a.double(), CA), _nchw(b.double(), CB)
    ref = _wgrad_ref64(r.kind, k, r.s, r.pad, a64, b64, CA, CB, "cpu")
    bound = K_SUM * U * math.sqrt(M) * _wgrad_ref64(r.kind, k, r.s, r.pad, a64 * a64, b64 * b64, CA, CB, "cpu").max().sqrt().item()
    tot = ws[..., :CB].double().sum(0)                       # [tap][CA][CB] -> the parameter's layout
    tot = (tot.permute(2, 1, 0) if r.kind == "conv_wgrad" else tot.permute(1, 2, 0)).reshape(ref.shape)
    check(f"{tag} sum of the slabs", tot, ref, bound)
    assert bool((ws[..., CB:] == 0).all()), (tag, "pad columns of the slabs must be zero")
    for z in range(ns):                                      # a slab without pixels is written as zeros
        if z * mps >= M:
            assert bool((ws[z] == 0).all()) and (bsum is None or bool((bsum[z] == 0).all())), (tag, "empty slab", z)
    bflat = b.double().reshape(M, CB) if r.kind == "conv_wgrad" else None
    if KK == 1 and r.kind == "conv_wgrad":                   # one tap: every slab is the product over its own pixel range
        aflat = a.double().reshape(M, CA)
        sl = [(z * mps, min((z + 1) * mps, M)) for z in range(ns)]
        slabs = torch.stack([(aflat[lo:hi].t() @ bflat[lo:hi]) if hi > lo else torch.zeros(CA, CB, dtype=torch.float64) for lo, hi in sl])[:, None]
        e = [K_SUM * U * math.sqrt(hi - lo) * ((aflat[lo:hi] ** 2).t() @ (bflat[lo:hi] ** 2)).max().sqrt().item() if hi > lo else 0.0 for lo, hi in sl]
        _check_slabs(tag, ws, None, (slabs, e), None, CB, ldo)
    if r.bsum:                                               # XB = dY with sb = 1, zero tap offset: row z = the column sums of slab z's pixels
        assert r.kind == "conv_wgrad"
        for z in range(ns):
            lo, hi = z * mps, min((z + 1) * mps, M)
            if hi > lo:
                check(f"{tag} bsum row {z}", bsum[z, :CB], bflat[lo:hi].sum(0), sum_bound(bflat[lo:hi], 0))
        assert bool((bsum[:, CB:] == 0).all()), (tag, "pad columns of bsum must be zero")


def _wgrad_rows():
    tiles = [(24, 24), (56, 56), (24, 136), (136, 24), (56, 136), (136, 56), (136, 136), (3, 64), (64, 3)]
    plans = [("conv_wgrad", 3, 1, 1), ("conv_wgrad", 4, 2, 1), ("convT_wgrad", 4, 2, 1), ("conv_wgrad", 1, 1, 0)]
    rows = []
    for i, (CA, CB) in enumerate(tiles):                     # every tile with every plan and split count, bsum on and off
        for j, (kind, k, s, pad) in enumerate(plans):
            ns = (1, 3, 7)[(i + j) % 3]                      # (M = 288: 7 slabs of 48 pixels leave the last one empty)
            H = 24 if (kind, k) == ("conv_wgrad", 4) else 12   # M = 2 x 12 x 12 = 288 pixels of the output (transposed: the input) grid
            rows.append(WR(kind, 2, H, H, CA, CB, k, s, pad, ns, int(kind == "conv_wgrad" and (i + j) % 2 == 0)))
    # ... and one tap at every split count on every tile (the slab-by-slab comparison)
    rows += [WR("conv_wgrad", 2, 12, 12, CA, CB, 1, 1, 0, ns, 1) for (CA, CB) in tiles for ns in (1, 3, 7)
             if WR("conv_wgrad", 2, 12, 12, CA, CB, 1, 1, 0, ns, 1) not in rows and WR("conv_wgrad", 2, 12, 12, CA, CB, 1, 1, 0, ns, 0) not in rows]
    return rows


WGRAD_ROWS = _wgrad_rows()


class WB(NamedTuple):
    """One-tap / head-split launches of ops._bwgrad: per batch entry, out[split][tap] = xa[rows of the split]^T xb[the same rows].
    rows: contraction rows per batch entry;  heads: 0 = one tap over `rows` pixels (cd.conv_wgrad(1, rows, 1, 1, ...), B = 1), else
    ops._headsplit_plan(heads) over B = rows / 32 images (xa = ctxs [B][heads][32][32], xb = dM [B][heads * 32][ldb]);
    olay: +1 slabs laid out [batch (stride o_bs)][split][tap], -1 (o_bs < 0) [split][batch][tap];  bsum rows are [batch * nsplit + split]."""
    site: str
    batch: int
    rows: int
    CA: int
    CB: int
    lda: int
    aoff: int
    a_bs: int
    ldb: int
    boff: int
    b_bs: int
    nsplit: int
    olay: int
    bsum: int
    heads: int = 0


def _wb_plan(r):
    if not r.heads:
        return cd.conv_wgrad(1, r.rows, 1, 1, 1, 0, 0, 0, 0)
    return cd.WgradPlan(1, 32, r.heads, 32, 1, r.heads, 32, 1, [(h, 0, h, 0) for h in range(r.heads)])


def wb_args(r, ad=None, stream=0):
    wp, ldo = _wb_plan(r), r4(r.CB)
    at = lambda key, on=True: ((ad[key] if ad else _STANDIN) if on else 0)
    o_bs = r.nsplit * wp.ntaps * r.CA * ldo if r.olay > 0 else -1
    return (at("xa") + 4 * r.aoff, r.lda, at("xb") + 4 * r.boff, r.ldb, at("ws"), ldo, (r.rows // 32) if r.heads else 1, wp.QH, wp.QW, wp.HA, wp.WA, wp.sa,
            wp.HB, wp.WB, wp.sb, r.CA, r.CB, wp.ntaps, wp.desc, r.nsplit, r.batch, r.a_bs, r.b_bs, o_bs, at("bsum", r.bsum), stream)


def _wgrad_batched_case(be, r):
    wp, CA, CB, ns, nb, T = _wb_plan(r), r.CA, r.CB, r.nsplit, r.batch, max(1, r.heads)
    ldo, M = r4(CB), r.rows
    mps = _m_per_split(M, ns)
    tag = f"wgrad {r.site} ({mps} rows per slab, {ns - -(-M // mps)} empty)"
    g = torch.Generator().manual_seed(CA + 3 * CB + ns + M)
    # rows of xa / xb per (batch entry, tap): tap h of the head-split plan reads rows (b, h, d) of both, m = b * 32 + d
    arows, brows = M * T, M * T
    asz = r.aoff + (nb - 1) * r.a_bs + arows * r.lda
    bsz = r.boff + (nb - 1) * r.b_bs + brows * r.ldb
    xa, xb = torch.full((asz,), float("nan")), torch.full((bsz,), float("nan"))
    A = lambda buf, z, C, ld, off, bs: _view(buf, off + z * bs, M * T, C, ld)
    for z in range(nb):                                      # (what the launch reads: randn, the pad channels of the last quad finite, the rest NaN)
        for buf, C, ld, off, bs in ((xa, CA, r.lda, r.aoff, r.a_bs), (xb, CB, r.ldb, r.boff, r.b_bs)):
            _view(buf, off + z * bs, M * T, r4(C), ld).fill_(BIG)
            A(buf, z, C, ld, off, bs).copy_(torch.randn(M * T, C, generator=g))
    t = dict(xa=be.to(xa), xb=be.to(xb), ws=nan_empty(be, ns * nb, T, CA, ldo))
    if r.bsum:
        t["bsum"] = nan_empty(be, nb * ns, ldo)
    args = wb_args(r, {k_: P(v) for k_, v in t.items()}, be.stream())
    print(f"{tag}: form {f32_wgrad_form(args)}")
    assert f32_wgrad_form(args) == f32_wgrad_form(wb_args(r)), tag
    outs = [t["ws"]] + ([t["bsum"]] if r.bsum else [])
    got = twice(lambda: be.L.cdf_conv_wgrad(*args), outs)
    # slabs as [batch][split]
    ws = got[0].view(nb, ns, T, CA, ldo) if r.olay > 0 else got[0].view(ns, nb, T, CA, ldo).transpose(0, 1)
    bsum = got[1].view(nb, ns, ldo) if r.bsum else None
    for z in range(nb):
        a64 = A(xa, z, CA, r.lda, r.aoff, r.a_bs).double()
        b64 = A(xb, z, CB, r.ldb, r.boff, r.b_bs).double()
        if r.heads:                                          # [B][heads][32][C] -> per tap h the rows m = (b, d)
            a64 = a64.view(M // 32, T, 32, CA).transpose(0, 1).reshape(T, M, CA)
            b64 = b64.view(M // 32, T, 32, CB).transpose(0, 1).reshape(T, M, CB)
        else:
            a64, b64 = a64[None], b64[None]
        sl = [(s_ * mps, min((s_ + 1) * mps, M)) for s_ in range(ns)]
        slabs = torch.stack([torch.einsum("tma,tmb->tab", a64[:, lo:hi], b64[:, lo:hi]) if hi > lo else torch.zeros(T, CA, CB, dtype=torch.float64)
                             for lo, hi in sl])
        e = [K_SUM * U * math.sqrt(hi - lo) * torch.einsum("tma,tmb->tab", a64[:, lo:hi] ** 2, b64[:, lo:hi] ** 2).max().sqrt().item() if hi > lo else 0.0
             for lo, hi in sl]
        bcols = None
        if r.bsum:                                           # tap 0's rows of xb
            bcols = (torch.stack([b64[0, lo:hi].sum(0) for lo, hi in sl]), [sum_bound(b64[0, lo:hi], 0) if hi > lo else 0.0 for lo, hi in sl])
        _check_slabs(f"{tag} batch entry {z}", ws[z], None if bsum is None else bsum[z], (slabs, e), bcols, CB, ldo)
        full = torch.einsum("tma,tmb->tab", a64, b64)
        check(f"{tag} batch entry {z}: sum of the slabs", ws[z][..., :CB].double().sum(0), full,
              K_SUM * U * math.sqrt(M) * torch.einsum("tma,tmb->tab", a64 ** 2, b64 ** 2).max().sqrt().item())


def _wgrad_batched_rows(B=3):
    rows = []
    HD = 128
    for n, ns in ((256, 9), (300, 7)):                       # ops._image_wgrad: 256 rows in 9 slabs of 32 (slab 8 empty), 300 in 7 of 48 (the last: 12)
        for CA, CB in ((HD, 48), (48, 136)):
            for olay in (-1, 1):
                rows.append(WB(f"_image_wgrad n={n} nsplit={ns} {CA}x{CB} o_bs{'<0' if olay < 0 else '>=0'}", B, n, CA, CB, r4(CA) + 4, 0, n * (r4(CA) + 4),
                               CB, 0, n * CB, ns, olay, 1))
    for heads in (1, 4):                                     # ops._linattn_out_bwd: the taps are heads, B * 32 contraction rows
        for dim in (48, 136):
            for nsw in (1, 3):
                rows.append(WB(f"_headsplit_plan heads={heads} dim={dim} nsw={nsw}", 1, B * 32, 32, dim, 32, 0, 0, dim, 0, 0, nsw, 1, 0, heads))
    C = 48                                                   # ops.bgemm_tn on slices of a [nb, K, 3 C] tensor: a = columns C .., b = columns 2 C ..
    rows.append(WB("bgemm_tn (non-contiguous batch strides)", B, 70, C, C, 3 * C, C, 70 * 3 * C, 3 * C, 2 * C, 70 * 3 * C, 1, 1, 0))
    return rows


WGRAD_BATCHED_ROWS = _wgrad_batched_rows()


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals: rejected on the host before any launch -- negative return code, a message, every output still poisoned
# ---------------------------------------------------------------------------------------------------------------------------------
def _refused(be, name, args, outs, what):
    dll = be.L._dll
    dll.cdf_last_error.restype = ctypes.c_char_p
    rc = getattr(dll, name)(*args)                           # (the unchecked entry point: be.L's wrapper raises on a non-zero code)
    if be.kind == "hip":
        torch.cuda.synchronize()
    msg = dll.cdf_last_error().decode()
    print(f"{what}: rc {rc}, {msg!r}")
    assert rc < 0 and msg, (what, rc, msg)
    for o in outs:
        bits = o.cpu()
        assert _poison_outside(bits, 0, 0), (what, "output written")


def _with(args, **kw):
    """args with the named arguments of cdf_conv_gemm[_io] replaced."""
    idx = dict(x=0, ldx=1, y=4, ldy=5, Cin=9, Cout=12, nphase=17, desc=18, sbias=20, ld_sbias=21, mul_mode=29, acc=30, y_bs=35, io=40, y_hi=41, ld_ys=42)
    a = list(args)
    for k_, v in kw.items():
        a[idx[k_]] = v
    return tuple(a)


def test_refusals(be):
    S = be.stream()
    # single launch: 3 x 3, 16 -> 24 channels, bias, an fp32 output and a bf16 plane
    r = GR("conv_fwd", 1, 8, 8, 16, 24, 3, 1, 1, "b", yhi=1)
    x, w, bias = be.to(torch.randn(1, 8, 8, 16)), be.to(torch.randn(9, 16, 24)), be.to(torch.randn(24))
    y, yh, extra = nan_empty(be, 1, 8, 8, 24), nan_empty(be, 1, 8, 8, 32, dtype=torch.int16), be.to(torch.randn(1, 8, 8, 24))
    outs = [y, yh]
    name, io_args = gr_args(r, dict(x=P(x), w=P(w), y=P(y), bias=P(bias), yhi=P(yh)), S)
    assert name == "cdf_conv_gemm_io"
    f32_args = io_args[:40] + (S,)
    be.L.cdf_conv_gemm_io(*io_args)                          # (the unmodified call is accepted)
    for o in outs:
        o.fill_(float("nan")) if o.dtype == torch.float32 else o.fill_(NAN16)
    taps17 = (ctypes.c_int * (3 + 3 * 17))(0, 0, 17, *([0, 0, 0] * 17))
    for what, nm, a in (
            ("ntaps = 17", "cdf_conv_gemm", _with(f32_args, desc=taps17)),
            ("a misaligned x", "cdf_conv_gemm", _with(f32_args, x=P(x) + 4)),
            ("ldy < Cout", "cdf_conv_gemm", _with(f32_args, ldy=20)),
            ("y = NULL without y_hi", "cdf_conv_gemm_io", _with(io_args, y=0, y_hi=0, ld_ys=0)),
            ("y = NULL with accumulate", "cdf_conv_gemm_io", _with(io_args, y=0, acc=1)),
            ("y_hi with Cout % 4 != 0", "cdf_conv_gemm_io", _with(io_args, Cout=22)),
            ("mul_mode without mul", "cdf_conv_gemm", _with(f32_args, mul_mode=3)),
            ("io_bf16 with an unknown bit", "cdf_conv_gemm_io", _with(io_args, io=16))):
        _refused(be, nm, a, outs, what)
    # batched, bias + res (row-offset addressing): 2 GEMMs of 16 x 32 x 24
    b = BR("refusals", 16, 32, 24, 0, 2, 1, 2 * 16 * 32, 0, 32, 16 * 32, 0, 2 * 32 * 24, 0, 24, 32 * 24, 0, 2 * 16 * 24, 0, 24, 16 * 24, 0, bias=1, res=1, ldr=24)
    a_, w_, res, yb = be.to(torch.randn(b.asz)), be.to(torch.randn(b.wsz)), be.to(torch.randn(b.ysz)), nan_empty(be, b.ysz + 64)
    sb = be.to(torch.randn(2, 24))
    name, bargs = br_args(b, dict(a=P(a_), w=P(w_), y=P(yb), bias=P(bias), res=P(res)), S)
    be.L.cdf_conv_gemm(*bargs)
    yb.fill_(float("nan"))
    _refused(be, name, _with(bargs, y_bs=16 * 24 + 4), [yb], "a batched launch with res and y_bs % ldy != 0")
    _refused(be, name, _with(bargs, sbias=P(sb), ld_sbias=24), [yb], "a batched launch with res and sbias")
    # b_trans with Cin % 4 != 0: the Linear weight in place, K = 46 of pitch 48
    lt = BR("refusals b_trans", 16, 46, 24, 1, 1, 1, 16 * 48, 0, 48, 0, 0, 24 * 48, 0, 48, 0, 0, 16 * 24, 0, 24, 0, 0)
    name, targs = br_args(lt, dict(a=P(a_), w=P(w_), y=P(yb)), S)
    _refused(be, name, targs, [yb], "b_trans with Cin % 4 != 0")
    # weight gradient
    wr = WR("conv_wgrad", 1, 8, 8, 16, 24, 1, 1, 0, 2, 1)
    xa, xb, ws, bsum = be.to(torch.randn(64, 16)), be.to(torch.randn(64, 24)), nan_empty(be, 2, 16, 24), nan_empty(be, 2, 24)
    wargs = wr_args(wr, dict(xa=P(xa), xb=P(xb), ws=P(ws), bsum=P(bsum)), S)
    be.L.cdf_conv_wgrad(*wargs)
    ws.fill_(float("nan")), bsum.fill_(float("nan"))
    _refused(be, "cdf_conv_wgrad", wargs[:5] + (20,) + wargs[6:], [ws, bsum], "a weight gradient with ldo < CB")
    _refused(be, "cdf_conv_wgrad", wargs[:19] + (0,) + wargs[20:], [ws, bsum], "nsplit = 0")
    _refused(be, "cdf_conv_wgrad", wargs[:8] + (1 << 21,) + wargs[9:], [ws, bsum], "QW past the exact range of the pixel walk")
    assert "pixel grid" in be.L._dll.cdf_last_error().decode()


# ---------------------------------------------------------------------------------------------------------------------------------
# the tested forms: f32_gemm_form / f32_wgrad_form of the argument tuples the rows above build (stand-in addresses of the rows' alignment)
# ---------------------------------------------------------------------------------------------------------------------------------
def forms_of_gemm_rows():
    return {f32_gemm_form(*gr_args(r)) for r in IGEMM_ROWS} | {f32_gemm_form(*br_args(r)) for r in BGEMM_ROWS}


def forms_of_wgrad_rows():
    return {f32_wgrad_form(wr_args(r)) for r in WGRAD_ROWS} | {f32_wgrad_form(wb_args(r)) for r in WGRAD_BATCHED_ROWS}


# The forms the recordings of test_gpu_invariance.py::test_coverage_guard reach: one bench step in bf16x3 and in bf16 (the linear-attention
# block's batched launches, the thin layers), one sampler step at B = 16 and one forward + backward pass of config 2's network (its
# attention's generic batched products, the 3-channel layers).  The guard fails when a recording reaches a form no row has, and when a
# form listed here is no longer reached.  Every other tested form is one no recording reaches (most epilogue sets of the single launch,
# the strided and transposed geometries, ...), like test_gemm_production.UNRECORDED_GEMM.
REACHED_GEMM = {
    ('128x128', 0, '1tap', 'outer', '', 0, '', 0, 0, 0, 1, 0, 1, 0),
    ('128x128', 0, '1tap', 'outer', '', 1, 'br', 0, 0, 0, 1, 0, 1, 0),
    ('128x128', 0, '1tap', 'outer', '', 1, 'br', 0, 0, 0, 1, 1, 0, 1),
    ('128x128', 0, '1tap', 'outer', 'A', 0, '', 0, 0, 0, 1, 0, 1, 0),
    ('128x128', 0, '1tap', 'outer+inner', 'W', 0, '', 0, 0, 0, 1, 0, 1, 0),
    ('128x128', 0, (1, 9, 1, 1, -1, -1), 'none', '', 0, 'b', 0, 0, 0, 1, 0, 1, 0),
    ('128x128', 0, (1, 9, 1, 1, 1, 1), 'none', '', 0, '', 0, 0, 0, 1, 0, 1, 0),
    ('128x128', 1, '1tap', 'outer', '', 0, '', 0, 0, 0, 1, 0, 1, 0),
    ('128x32', 0, '1tap', 'none', '', 0, '', 0, 0, 0, 0, 0, 1, 0),
    ('128x32', 0, '1tap', 'none', '', 0, 'b', 0, 0, 0, 0, 0, 1, 0),
    ('128x32', 0, '1tap', 'outer+inner', '', 0, '', 0, 0, 0, 1, 0, 1, 0),
    ('128x32', 0, (1, 9, 1, 1, -1, -1), 'none', '', 0, 'b', 0, 0, 0, 0, 0, 1, 0),
    ('128x32', 0, (1, 9, 1, 1, 1, 1), 'none', '', 0, '', 0, 0, 0, 0, 0, 1, 0),
    ('128x32', 1, '1tap', 'outer', '', 0, '', 0, 0, 0, 1, 0, 1, 0),
    ('128x32', 1, '1tap', 'outer+inner', '', 0, '', 0, 0, 0, 1, 0, 1, 0),
    ('128x32', 1, '1tap', 'outer+inner', 'W', 0, '', 0, 0, 0, 1, 0, 1, 0),
    ('256x64', 0, '1tap', 'none', '', 0, '', 0, 0, 0, 1, 0, 1, 0),
    ('256x64', 0, '1tap', 'outer', '', 1, 'br', 0, 0, 0, 1, 0, 1, 0),
    ('256x64', 0, '1tap', 'outer', '', 1, 'br', 0, 0, 0, 1, 1, 0, 1),
    ('256x64', 0, '1tap', 'outer', 'A', 0, '', 0, 0, 0, 1, 0, 1, 0),
    ('256x64', 0, '1tap', 'outer+inner', 'W', 0, '', 0, 0, 0, 1, 0, 1, 0),
    ('256x64', 1, '1tap', 'outer', '', 0, '', 0, 0, 0, 1, 0, 1, 0),
}
REACHED_WGRAD = {
    ((128, 128), (False, False, False, False), '1tap', 1, 0, 0),
    ((128, 128), (False, False, False, False), '1tap', 1, 1, 1),
    ((128, 32), (False, False, True, True), ('conv', 9, 1), 0, 0, 1),
    ((128, 32), (False, True, True, True), '1tap', 0, 0, 1),
    ((128, 64), (False, False, False, True), '1tap', 0, 0, 1),
    ((32, 128), (True, True, False, False), '1tap', 1, 0, 0),
    ((32, 128), (True, True, False, False), 'heads', 0, 0, 0),
    ((32, 128), (True, True, False, False), ('conv', 9, 1), 0, 0, 1),
    ((32, 128), (True, True, False, True), 'heads', 0, 0, 0),
    ((64, 128), (False, True, False, False), '1tap', 0, 0, 1),
    ((64, 64), (False, True, False, True), '1tap', 1, 1, 1),
}
# ... with a row, at the small shapes above, for each reached form the crossed tables lack:
IGEMM_ROWS += [
    GR("conv_fwd", 2, 13, 13, 40, 136, 3, 1, 1, "b"),        # config 2: 3 x 3 with bias on the <128,128> tile
    GR("conv_dgrad", 2, 13, 13, 40, 136, 3, 1, 1),           # ... and its data gradient
    GR("conv_fwd", 2, 13, 13, 40, 30, 3, 1, 1, "b"),         # the convolution back to the image's channels: scalar epilogue
    GR("conv_dgrad", 2, 13, 13, 40, 30, 3, 1, 1),
    GR("conv_fwd", 2, 13, 13, 40, 30, 1, 1, 0),              # the 1 x 1 of the same kind, without and with bias
    GR("conv_fwd", 2, 13, 13, 40, 30, 1, 1, 0, "b"),
]
BGEMM_ROWS += [
    BR("bgemm_nn, m = 136 (contiguous batch)", 70, 40, 136, 0, 3, 1, 3 * 70 * 40, 0, 40, 70 * 40, 0, 3 * 40 * 136, 0, 136, 40 * 136, 0,
       3 * 70 * 136, 0, 136, 70 * 136, 0),
    BR("bgemm_nt, m = 24 (contiguous batch)", 70, 40, 24, 1, 3, 1, 3 * 70 * 40, 0, 40, 70 * 40, 0, 3 * 24 * 40, 0, 40, 24 * 40, 0,
       3 * 70 * 24, 0, 24, 70 * 24, 0),
]
WGRAD_ROWS += [WR("conv_wgrad", 2, 12, 12, 136, 24, 3, 1, 1, 3, 1)]
# The pixel walk on 4 x 4 images (a 16-pixel step: four rows, a whole image), with taps and with one tap (slab by slab).  B = 3, M = 48 in
# four slabs of 16 | 16 | 16 | none: one step each, the decode alone (a slab of two steps leaves no split of M = 48 without pixels).  B = 5,
# M = 80 in four slabs of 32 | 32 | 16 | none: the second step of a slab comes out of the advance, over four rows and an image boundary.
WGRAD_ROWS += [WR("conv_wgrad", B, 4, 4, 56, 136, k, 1, k // 2, 4, 1) for B in (3, 5) for k in (3, 1)]
WGRAD_BATCHED_ROWS += [
    WB("bgemm_tn 136x136", 3, 96, 136, 136, 136, 0, 96 * 136, 136, 0, 96 * 136, 3, 1, 0),
    WB("bgemm_tn 24x136", 3, 96, 24, 136, 24, 0, 96 * 24, 136, 0, 96 * 136, 3, 1, 0),
    WB("_image_wgrad 136x136 o_bs<0", 3, 96, 136, 136, 136, 0, 96 * 136, 136, 0, 96 * 136, 3, -1, 1),
    WB("_image_wgrad 56x56 o_bs<0", 3, 96, 56, 56, 56, 0, 96 * 56, 56, 0, 96 * 56, 3, -1, 1),
]


def test_form_tables():
    """The tables keep what they were built for: with every tile every geometry, K form, row count and epilogue operand set (the typed
    ones on the vector epilogue only); all seven dispatch branches of the weight gradient (six kernel instantiations) with every plan
    class and split count; the forms flagged as reached are tested forms; some tested form is unreached."""
    tiles = {}
    for r in IGEMM_ROWS:
        f = f32_gemm_form(*gr_args(r))
        t = tiles.setdefault((f[0], f[10]) if f[10] else "scalar", dict(geom=set(), k=set(), m=set(), epi=set()))
        t["geom"].add((r.kind, r.k, r.s, r.pad)), t["k"].add((r.Cin, r.xld, r.xoff)), t["m"].add(r.B), t["epi"].add(tuple(r[9:16]))
    assert set(tiles) == {("128x32", 1), ("256x64", 1), ("128x128", 1), "scalar"}
    for name, t in tiles.items():
        assert t["geom"] >= {g[:4] for g in _GEOM} and t["k"] >= set(_KS) and t["m"] == {1, 2}, (name, t)
        assert t["epi"] >= set(_EPI_F32 + (_EPI_IO if name != "scalar" else [])), (name, t["epi"])
    tw = forms_of_wgrad_rows()
    assert {f[1] for f in tw} >= {(True, True, True, True), (False, True, False, True), (True, True, False, False), (False, False, True, True),
                                  (False, True, False, False), (False, False, False, True), (False, False, False, False)}
    for cls in {f[1] for f in tw if f[3] == 0 and f[2] != "heads"}:
        assert {f[2] for f in tw if f[1] == cls} >= {"1tap", ("conv", 9, 1), ("conv", 16, 2), ("convT", 16)}, cls
    tg = forms_of_gemm_rows()
    assert REACHED_GEMM <= tg and REACHED_WGRAD <= tw
    assert (tg - REACHED_GEMM) and (tw - REACHED_WGRAD)


def test_recorded_forms_dry(monkeypatch):
    """The recordings of test_gpu_invariance.py::test_coverage_guard without a GPU: the same four runs at their real shapes (bench step in
    bf16x3 and bf16, sampler step at B = 16, config 2's pass at B = 128) on CPU tensors, with every launching entry point replaced by a
    stub that returns 0 -- host-side queries run, nothing is computed, torch.empty's pages are never touched.  Which entry point is
    called with which arguments is decided by the Python layer from shapes and modes alone, and the forms are the ones the MI355X
    recording of the guard prints (22 + 11, the same sets): every one must be a tested form, and every form flagged as reached must be
    among them (the guard's two assertions)."""
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
    monkeypatch.setattr(gi, "_GEMM_FAMILY", ("cdf_conv_gemm", "cdf_conv_gemm_io", "cdf_conv_wgrad"))
    _, _, calls = gi._guard_calls(p2.bench_step_inputs())
    reached_g = {f32_gemm_form(n, a) for _, n, a in calls if n != "cdf_conv_wgrad"}
    reached_w = {f32_wgrad_form(a) for _, n, a in calls if n == "cdf_conv_wgrad"}
    print("exact-fp32 GEMM forms reached:", *sorted(reached_g, key=repr), sep="\n    ")
    print("exact-fp32 weight-gradient forms reached:", *sorted(reached_w, key=repr), sep="\n    ")
    assert reached_g and reached_w
    assert reached_g <= forms_of_gemm_rows(), sorted(reached_g - forms_of_gemm_rows(), key=repr)
    assert reached_w <= forms_of_wgrad_rows(), sorted(reached_w - forms_of_wgrad_rows(), key=repr)
    assert REACHED_GEMM <= reached_g and REACHED_WGRAD <= reached_w, (sorted(REACHED_GEMM - reached_g, key=repr), sorted(REACHED_WGRAD - reached_w, key=repr))


# ---------------------------------------------------------------------------------------------------------------------------------
# the tests over the case tables (both backends)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", IGEMM_ROWS, ids=lambda r: "-".join(map(str, r[:20])))
def test_igemm_single_launch(be, r):
    _igemm_case(be, r)


@pytest.mark.parametrize("r", BGEMM_ROWS, ids=lambda r: r.site.replace(" ", "_"))
def test_igemm_batched_call_sites(be, r):
    _bgemm_case(be, r)


@pytest.mark.parametrize("r", WGRAD_ROWS, ids=lambda r: "-".join(map(str, r[:11])))
def test_wgrad_tiles_plans_splits(be, r):
    _wgrad_conv_case(be, r)


@pytest.mark.parametrize("r", WGRAD_BATCHED_ROWS, ids=lambda r: r.site.replace(" ", "_"))
def test_wgrad_batched_and_head_split(be, r):
    _wgrad_batched_case(be, r)
