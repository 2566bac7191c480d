"""The kernels between the GEMMs -- csrc/k_dwconv.hip (depthwise 7 x 7 forward / data gradient, weight gradient) and csrc/k_norm.hip
(channel LayerNorm, GroupNorm (+ SiLU + dropout), forward and backward) -- in every argument form the product launches.  Conventions of
test_gemm_sp_forms.py: a form is a pure function of a call's argument tuple (no pointer values, only which pointers are null); every row
of a case table builds its tuple through one helper and the case asserts that the launch has the form the table claims; every output and
workspace is NaN-poisoned before each of two launches that must agree bit for bit; float64 CPU references; every worst error / bound is
printed.  test_gpu_invariance.py::test_coverage_guard holds the recorded calls of the bench step (both modes), the sampler step and
config 2's pass (dropout 0.1) against the tables; test_recorded_norm_dw_forms_dry makes the same recordings, and those of two small
networks, without a GPU.

What the older tests of these kernels (test_kernels.py, test_kernels_production.py, test_bf16_storage.py) never pass and the product
does: a pitch larger than the channel count (slices of a concatenation, the per-sample bias as a slice of the 420-wide time-embedding
matrix), null optional pointers, the accumulate flags (onto RANDOM earlier contents here: from zeros "accumulate" and "overwrite" agree),
H != W, inputs with a large mean.

Inputs: pad columns of every pitched input are NaN; the in-quad pad channels C .. r4(C)-1 of the depthwise tensors are zero, which the
product guarantees (poison.nan_empty states the rule).  Pad columns of pitched outputs must still hold the poison afterwards.

References (float64, CPU): F.conv2d / F.conv_transpose2d / torch.nn.grad.conv2d_weight; test_kernels_production._ln_ref / _gn_ref; the
dropout mask from test_small_kernels_production._hash32 at element index (b HW + r) C + c -- C, not the pitch -- so no kernel states the
index.  bf16 / planes forms by the existing contracts: planes equal cdf_split_bf16 of the fp32 output bit for bit, a bf16 output equals
the fp32 kernel's result (same pitches, widened inputs) rounded once, an fp32 output from bf16 inputs equals it bit for bit.

Bounds, no new constant (test_kernels_production.py's for the same kernels):
  depthwise   y: min(1e-5, K_SUM 2^-24 7 (7 |x|max |w|max + |bias|max + |sbias|max)), twice that with a residual;
              dw: min(K_SUM 2^-24 sqrt(n) |x|max max||dy||_2, 5e-5 max(1, |ref|max)); dbias, dsb: min(sum_bound, 5e-5 max(1, |ref|max))
  LayerNorm   y: min(5e-6, 4 K_SUM 2^-24 sqrt(C) |y|max); dx: 1e-5; dg, db: sum_bound
  GroupNorm   y: 1e-5 g, dx: 2e-5 g, dgamma, dbeta: 1e-4 r with g = sqrt(max(1, n_group / 900)), r = sqrt(max(1, B HW / 600))
  accumulate  the expected value is old + grad, the bound grows by one rounding 2^-24 |old + grad|max
  dropout     the mask scales kept values by 1 / (1 - p): every bound times that factor (forward: plus the product's own rounding)
  offset rows (a per-(sample, channel) offset of +-4 under unit noise: a wrong row's or group's mean errs by O(4)): LayerNorm's bounds
              times |x|max; GroupNorm: the larger of the bound above and the error of F.group_norm in float32 on the CPU against float64
              on the same inputs, margin 1x -- the kernel (E[x^2] - mean^2 from fp32 partial sums) must be no worse than torch's fp32.

Two caps are further out than their names say, and the tables go where they take effect: cdf_groupnorm_nchunk(16384 + 37) is exactly 64
(the cap cuts from HW = 65 x 256: the rows with HW = 16640 + 37), and a LayerNorm wave takes U row groups per round (U = 4 / 2 forward,
2 / 1 backward), so a wave's second round starts U times past the row count at which cdf_layernorm_blocks reaches 1024 (rows '2nd+37';
the bench step's LayerNorms at 128 x 128 are there).

Cases: depthwise 106, weight gradient 33, LayerNorm forward 71 / backward 74, GroupNorm forward 67 / backward 68; with the table and
dry-guard tests 421 on the simulator (122 s in one process) and 419 on the MI355X (12 s).  No row is GPU-only: the rows past the apply
grid's cap (B = 2, HW = 8200, C = 256 and the reached B = 513 / B = 65 forms) take about a second each on the simulator.
Worst error / bound per output, simulator | MI355X (equal: these kernels are plain fp32 loops without matrix cores, the simulator follows
them operation for operation; 20 of the 897 printed figures differ at all, all behind SiLU's exp):
    depthwise        y 0.14    dw 0.02    dbias 0.07    dsb 0.11
    LayerNorm        y 0.42    mean 0.03  rstd 0.03     dx 0.28    dg 0.36    db 0.25
    GroupNorm        y 0.22    dx 0.27    dgamma 0.17   dbeta 0.16
    GroupNorm, offset 4 (B = 2, HW = 1024, C = 64; kernel error | F.group_norm float32 | bound without it), both backends:
                     y 6.4e-6 | 1.6e-5 | 1.5e-5      dx 3.7e-6 | 1.7e-5 | 3.0e-5      dgamma 1.7e-5 | 2.2e-4 .. 4.0e-4 | 1.8e-4
                     (the MI355X's figures are the simulator's to three digits: the kernel is no worse than torch's fp32 there either)
Seeded faults (simulator only; each changes values, not addresses outside a buffer), all caught here; of the older tests
(test_kernels.py, test_kernels_production.py, test_bf16_storage.py, test_modules.py) the ones that failed too are named, the rest stayed green:
    1 dwconv7_wgrad_final_kernel ignores `accumulate`                28 weight-gradient rows; older: 6 module-level tests of test_modules.py
                                                                     (fused accumulation, trainer), no kernel-level test
    2 GroupNorm backward dropout index with the pitch ldx, not C     the 3 backward rows with dropout and a pitched x; older: none
    3 dwconv7_kernel reads sbias with pitch ldy, not ld_sbias        35 depthwise rows; older: 24 module-level tests (goldens), no kernel-level test
    4 groupnorm_partial_kernel (mode 0) reads x with pitch C         11 forward rows; older: 3 module-level tests of the Model network
    5 groupnorm_bwd_param_kernel ignores `accumulate`                56 backward rows; older: none
    6 LayerNorm backward NV = 3 launched as the NV = 2 kernel        19 backward rows; older: none
"""
import functools
import math
from typing import NamedTuple

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from poison import BF16_NAN_BITS, nan_empty
from test_kernels import P, _split, r4
from test_kernels_production import K_SUM, U, _gn_ref, _ln_ref, bits_equal, check, sum_bound, twice
from test_small_kernels_production import _hash32

NAN32 = torch.tensor(float("nan")).view(torch.int32).item()  # the poison bit pattern of tests/poison.py
NAN = float("nan")
SEED = (1 << 40) + 12345                                     # a live dropout seed (64-bit)
cdiv = lambda a, b: -(-a // b)


def _null(v):
    return not int(getattr(v, "value", v) or 0)


def _letters(names, flags):
    return "".join(c for c, f in zip(names, flags) if f)


# ---------------------------------------------------------------------------------------------------------------------------------
# forms: pure functions of (entry point, argument tuple)
# ---------------------------------------------------------------------------------------------------------------------------------
DW_NAMES = ("cdf_dwconv7", "cdf_dwconv7_io", "cdf_dwconv7_planes")
DW_WGRAD_NAMES = ("cdf_dwconv7_wgrad", "cdf_dwconv7_wgrad_io")
LN_FWD_NAMES = ("cdf_layernorm_c_fwd", "cdf_layernorm_c_fwd_io")
LN_BWD_NAMES = ("cdf_layernorm_c_bwd", "cdf_layernorm_c_bwd_io", "cdf_layernorm_c_bwd_planes")
GN_FWD_NAMES = ("cdf_groupnorm_fwd", "cdf_groupnorm_fwd_ex")
GN_BWD_NAMES = ("cdf_groupnorm_bwd", "cdf_groupnorm_bwd_ex")


def dw_form(name, a):
    """cdf_dwconv7 / _io / _planes: (io: 0, 1, 2 or 'planes'; tile '16x16' (W <= 16) or '32x8'; flip; accumulate; present optional operands
    of b(ias) s(bias) r(es); operands of x y w s r whose pitch exceeds r4(C); more than one 8-quad channel group; a ragged last group)."""
    ldx, ldw, bias, sbias, lds, ldy = a[1], a[3], a[4], a[5], a[6], a[8]
    B, H, W, C, flip, acc, res, ldr = a[9:17]
    io = a[17] if name == "cdf_dwconv7_io" else ("planes" if name == "cdf_dwconv7_planes" and not _null(a[17]) else 0)
    Cp = r4(C)
    C4 = Cp // 4
    on = (True, True, True, not _null(sbias), not _null(res))
    return (io, "16x16" if W <= 16 else "32x8", int(flip), int(acc), _letters("bsr", (not _null(bias), on[3], on[4])),
            _letters("xywsr", (o and ld > Cp for o, ld in zip(on, (ldx, ldy, ldw, lds, ldr)))), int(C4 > 8), int(C4 % 8 != 0))


def dw_wgrad_form(name, a):
    """cdf_dwconv7_wgrad / _io: (io; 'narrow' (W < 32) or 'wide' partial kernel; chunk count capped at 32; an empty chunk; accumulate;
    present outputs of b (dbias) s (dsb); pitched x d(y) s (dsb); C % 4 != 0)."""
    ldx, lddy, dbias, dsb, ld_dsb = a[1], a[3], a[5], a[6], a[7]
    B, H, W, C, acc = a[9:14]
    io = a[14] if name == "cdf_dwconv7_wgrad_io" else 0
    nch = min(32, max(1, H // 4))
    rpc = cdiv(H, nch)
    return (int(io), "narrow" if W < 32 else "wide", int(H // 4 > 32), int((nch - 1) * rpc >= H), int(acc), _letters("bs", (not _null(dbias), not _null(dsb))),
            _letters("xds", (ldx > r4(C), lddy > r4(C), not _null(dsb) and ld_dsb > r4(C))), int(C % 4 != 0))


def ln_geom(C):
    """(LP lanes per row, NV float4 per lane, rows per 256-thread block): ln_geometry / cdf_layernorm_blocks of csrc/k_norm.hip."""
    lp = 1
    while lp < 64 and lp * 4 < C:
        lp <<= 1
    return lp, cdiv(C, 4 * lp), 4 * (64 // lp)


def _ln_common(M, C, bwd):
    """(NV; idle lanes; the block count is at its cap of 1024; a wave walks a second round of rows -- each wave takes U row groups per
    round, U = 4 / 2 forward and 2 / 1 backward for NV <= 2 / NV > 2, so that starts U times further out than the cap)."""
    lp, nv, gpb = ln_geom(C)
    unroll = (2 if nv <= 2 else 1) * (1 if bwd else 2)
    nb = min(1024, cdiv(M, gpb))
    return nv, int(4 * lp * nv > C), int(cdiv(M, gpb) >= 1024), int(cdiv(M, 64 // lp) > nb * 4 * unroll)


def ln_fwd_form(name, a):
    """cdf_layernorm_c_fwd / _io: (NV; idle lanes; x bf16; present outputs of y h(i) l(o) s(tatistics); pitched x y p(lanes); block count
    at its cap of 1024; a second round of rows per wave)."""
    ldx, y, ldy, mean, M, C, hi, lo, lds = a[1], a[2], a[3], a[6], a[8], a[9], a[11], a[12], a[13]
    io = int(bool(a[14])) if name == "cdf_layernorm_c_fwd_io" else 0
    nv, idle, capped, second = _ln_common(M, C, False)
    return (nv, idle, io, _letters("yhls", (not _null(y), not _null(hi), not _null(lo), not _null(mean))),
            _letters("xyp", (ldx > C, not _null(y) and ldy > C, not _null(hi) and lds > C)), capped, second)


def ln_bwd_form(name, a):
    """cdf_layernorm_c_bwd / _io / _planes: (NV; idle lanes; io: 0, 7, 14 or 'planes'; add present; accumulate_dx; accumulate_param;
    pitched d(y) x o (dx) a(dd) p(lanes); block count at its cap; a second round of rows per wave)."""
    lddy, ldx, lddx, add, ldadd, M, C, accdx, accp = a[1], a[3], a[8], a[9], a[10], a[14], a[15], a[16], a[17]
    io = a[18] if name == "cdf_layernorm_c_bwd_io" else ("planes" if name == "cdf_layernorm_c_bwd_planes" and not _null(a[18]) else 0)
    nv, idle, capped, second = _ln_common(M, C, True)
    return (nv, idle, io, int(not _null(add)), int(accdx), int(accp),
            _letters("dxoap", (lddy > C, ldx > C, lddx > C, not _null(add) and ldadd > C, io == "planes" and a[20] > C)), capped, second)


def _gn_common(B, HW, C, groups):
    """(channels per group 1, 2, 3 or 4 (= 4 or more; 3: a float4 straddles two groups); more than one 64-channel block; a ragged one;
    chunks '1' / 'many' / 'capped' (64); a shorter last chunk; a chunk length that leaves the 16-row unrolled loop a tail; the apply
    kernels' grid capped at 4096 blocks)."""
    nch = min(64, max(1, HW // 256))
    rpc = cdiv(HW, nch)
    return (min(C // groups, 4), int(C > 64), int(C % 64 != 0), "1" if nch == 1 else ("capped" if HW // 256 > 64 else "many"), int(HW % rpc != 0),
            int(rpc % 16 != 0), int(B * HW * (C // 4) > 4096 * 256))


def gn_fwd_form(name, a):
    """cdf_groupnorm_fwd / _ex: _gn_common + (silu; dropout; present outputs of y h(i) l(o); pitched x y p(lanes))."""
    ldx, y, ldy, B, HW, C, groups, silu = a[1], a[2], a[3], a[9], a[10], a[11], a[12], a[14]
    p, hi, lo, lds = (a[15], a[17], a[18], a[19]) if name == "cdf_groupnorm_fwd_ex" else (0.0, 0, 0, 0)
    return _gn_common(B, HW, C, groups) + (int(silu), int(p > 0), _letters("yhl", (not _null(y), not _null(hi), not _null(lo))),
                                          _letters("xyp", (ldx > C, not _null(y) and ldy > C, not _null(hi) and lds > C)))


def gn_bwd_form(name, a):
    """cdf_groupnorm_bwd / _ex: _gn_common + (silu; dropout; accumulate_dx; accumulate_param; pitched d(y) x o (dx))."""
    lddy, ldx, lddx, B, HW, C, groups, silu, accdx, accp = a[1], a[3], a[9], a[13], a[14], a[15], a[16], a[17], a[18], a[19]
    p = a[20] if name == "cdf_groupnorm_bwd_ex" else 0.0
    return _gn_common(B, HW, C, groups) + (int(silu), int(p > 0), int(accdx), int(accp), _letters("dxo", (lddy > C, ldx > C, lddx > C)))


# ---------------------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------------------
def _pitched(t, ld):
    """t [..., C] in the first columns of a [..., ld] tensor of its dtype, NaN in the pad columns."""
    buf = torch.full(t.shape[:-1] + (ld,), NAN, dtype=t.dtype)
    buf[..., :t.shape[-1]] = t
    return buf


def _pads_poisoned(t, C):
    """The columns C .. of host tensor t (fp32, or int16 bf16 bits) still hold the poison bit pattern."""
    if t.dtype == torch.int16:
        return bool((t[..., C:] == BF16_NAN_BITS).all())
    return bool((t.view(torch.int32)[..., C:] == NAN32).all())


def _bf(t):
    return t.bfloat16().view(torch.int16)


def _at(ad, key, on=True):
    return (ad[key] if ad else 1) if on else 0


def _chk(group, name, got, ref, bound):
    check(f"[{group}] {name}", got, ref, bound)


def _keep(B, HW, C, p):
    """(the kept-element mask [B, HW, C] of dropout probability p under SEED, 1 / (1 - p) as the kernels compute it in fp32)."""
    pf = np.float32(p)
    thr = np.uint32(int(float(pf) * 4294967296.0))
    keep = torch.from_numpy(_hash32(SEED, np.arange(B * HW * C)) >= thr).view(B, HW, C)      # idx = (b HW + r) C + c
    return keep, torch.tensor(np.float32(1.0) / (np.float32(1.0) - pf))


def _offset(shape_rows, C, per, g):
    """+-4 per (sample, channel), a sample = `per` consecutive rows."""
    n = cdiv(shape_rows, per)
    sign = torch.where(torch.rand(n, C, generator=g) < 0.5, -4.0, 4.0)
    return sign.repeat_interleave(per, 0)[:shape_rows]


# ---------------------------------------------------------------------------------------------------------------------------------
# depthwise 7 x 7: forward and data gradient
# ---------------------------------------------------------------------------------------------------------------------------------
class DW(NamedTuple):
    """io: 0, 1 (bf16 x / res / y), 2 (bf16 x / res, fp32 y) or 'planes'; ops: letters of b(ias), s (per-sample bias), r(esidual);
    ld*: pitches of x, y, w, sbias, res, planes (0: r4(C))."""
    io: object
    B: int
    H: int
    W: int
    C: int
    flip: int = 0
    acc: int = 0
    ops: str = "bs"
    ldx: int = 0
    ldy: int = 0
    ldw: int = 0
    lds: int = 0
    ldr: int = 0
    ldp: int = 0


def dw_call(r, ad=None, stream=0, io=None):
    """(entry point, argument tuple) of a DW row the way ops.dwconv7 / dwconv7_bf write the call (C rounded up to 4); ad: addresses."""
    io = r.io if io is None else io
    Cp = r4(r.C)
    has = lambda c: c in r.ops
    base = (_at(ad, "x"), r.ldx or Cp, _at(ad, "w"), r.ldw or Cp, _at(ad, "bias", has("b")), _at(ad, "sbias", has("s")), (r.lds or Cp) if has("s") else 0,
            _at(ad, "y"), r.ldy or Cp, r.B, r.H, r.W, Cp, r.flip, r.acc, _at(ad, "res", has("r")), (r.ldr or Cp) if has("r") else 0)
    if io == "planes":
        return "cdf_dwconv7_planes", base + (_at(ad, "hi"), _at(ad, "lo"), r.ldp or Cp, stream)
    if io:
        return "cdf_dwconv7_io", base + (io, stream)
    return "cdf_dwconv7", base + (stream,)


def _dw_case(be, r):
    B, H, W, C = r.B, r.H, r.W, r.C
    Cp = r4(C)
    ldx, ldy, ldw, lds, ldr, ldp = (v or Cp for v in (r.ldx, r.ldy, r.ldw, r.lds, r.ldr, r.ldp))
    tag = "dwconv7 " + "-".join(map(str, r))
    g = torch.Generator().manual_seed(C * 131 + H * 7 + W)
    rn = lambda *s: torch.randn(*s, generator=g)
    q = (lambda t: t.bfloat16().float()) if r.io in (1, 2) else (lambda t: t)
    x = q(rn(B, H, W, Cp))
    x[..., C:] = 0                                           # (in-quad pad channels: zero, the product's guarantee)
    w = torch.zeros(Cp, 1, 7, 7)
    w[:C] = rn(C, 1, 7, 7) / 7
    bias, sb = torch.zeros(Cp), torch.zeros(B, Cp)
    bias[:C], sb[:, :C] = rn(C), rn(B, C)
    res, y0 = q(rn(B, H, W, Cp)), rn(B, H, W, Cp)
    if r.io == 1:
        y0 = q(y0)
    has = lambda c: c in r.ops
    wd, bd, sbd = be.to(_pitched(w.reshape(Cp, 49).t().contiguous(), ldw)), be.to(bias), be.to(_pitched(sb, lds))   # [49][ldw]: tap ky * 7 + kx
    xp, rp, y0p = _pitched(x, ldx), _pitched(res, ldr), _pitched(y0, ldy)

    def go(io):
        bf, ybf = io in (1, 2), io == 1
        xin, rin = be.to(_bf(xp) if bf else xp), be.to(_bf(rp) if bf else rp)
        y = nan_empty(be, B, H, W, ldy, dtype=torch.int16 if ybf else torch.float32)
        old = be.to(_bf(y0p) if ybf else y0p)
        outs = [y]
        ad = dict(x=P(xin), w=P(wd), bias=P(bd), sbias=P(sbd), y=P(y), res=P(rin))
        if io == "planes":
            outs += [nan_empty(be, B, H, W, ldp, dtype=torch.int16), nan_empty(be, B, H, W, ldp, dtype=torch.int16)]
            ad.update(hi=P(outs[1]), lo=P(outs[2]))
        name, args = dw_call(r, ad, be.stream(), io)
        assert dw_form(name, args) == dw_form(*dw_call(r, io=io)), tag

        def launch():
            if r.acc:
                y.copy_(old)                                 # (accumulate reads y: its previous contents are an input)
            getattr(be.L, name)(*args)
        return twice(launch, outs)
    form = dw_form(*dw_call(r))
    print(f"{tag}: form {form}")
    yf = go(0)[0]
    # ---- float64
    xn, w64 = x.permute(0, 3, 1, 2).double(), w.double()
    ref = (F.conv_transpose2d(xn, w64, padding=3, groups=Cp) if r.flip else F.conv2d(xn, w64, padding=3, groups=Cp)).permute(0, 2, 3, 1)
    tb = K_SUM * U * 7 * (x.abs().max().item() * w.abs().max().item() * 7 + (bias.abs().max().item() if has("b") else 0.0) + (sb.abs().max().item() if has("s") else 0.0))
    if has("b"):
        ref = ref + bias.double()
    if has("s"):
        ref = ref + sb.double()[:, None, None, :]
    if has("r"):
        ref, tb = ref + res.double(), 2 * tb
    bound = min(1e-5, tb)
    if r.acc:
        ref = ref + y0.double()
        bound += U * ref.abs().max().item()
    _chk("dw", f"{tag} y", yf[..., :Cp], ref, bound)
    assert _pads_poisoned(yf, Cp), (tag, "a pad column of y changed")
    if r.io == 1:
        yb = go(1)[0]
        assert torch.equal(yb[..., :Cp].view(torch.bfloat16), yf[..., :Cp].bfloat16()), (tag, "bf16 y is not the fp32 result rounded once")
        assert _pads_poisoned(yb, Cp), (tag, "a pad column of the bf16 y changed")
    elif r.io == 2:
        y2 = go(2)[0]
        assert bits_equal(y2, yf), (tag, "fp32 y from bf16 operands differs from the fp32 kernel on the widened values")
    elif r.io == "planes":
        y2, hi, lo = go("planes")
        assert bits_equal(y2, yf), (tag, "y of the planes form differs")
        rh, rl = _split(be, be.to(yf[..., :Cp]).view(-1, Cp))
        ld8 = rh.shape[-1]
        assert torch.equal(hi.view(-1, ldp)[:, :Cp], rh.cpu()[:, :Cp]) and torch.equal(lo.view(-1, ldp)[:, :Cp], rl.cpu()[:, :Cp]), (tag, "planes", ld8)
        assert _pads_poisoned(hi, Cp) and _pads_poisoned(lo, Cp), (tag, "a pad column of the planes changed")
    return form


def _dw_rows():
    shapes = [(5, 16), (16, 17), (9, 33), (12, 40), (40, 12)]
    Cs = [3, 36, 68]
    pit = lambda C: dict(ldx=r4(C) + 8, ldy=r4(C) + 12, ldw=r4(C) + 4, ldr=r4(C) + 16, lds=420)
    pats = [lambda C: dict(ops="bsr", **pit(C)),                                   # every pitch different and larger than r4(C)
            lambda C: dict(ops="b"),                                               # bias without a per-sample bias
            lambda C: dict(flip=1, acc=1, ops=""),                                 # data gradient accumulated
            lambda C: dict(flip=1, acc=1, ops="r", ldr=r4(C) + 16),                # ... with a (pitched) residual as well
            lambda C: dict(ops="bs", lds=420),                                     # the per-sample bias as a slice of the time-embedding matrix
            lambda C: dict(flip=1, ops="r", ldx=r4(C) + 64),                       # x a slice of a concatenation
            lambda C: dict(ops="bsr", acc=1, **pit(C))]
    rows = []
    for si, (H, W) in enumerate(shapes):
        for ci, C in enumerate(Cs):
            for k in range(3):
                rows.append(DW(0, 2 + (si + ci + k) % 2, H, W, C, **pats[(3 * (si + ci) + k) % 7](C)))
            # the bf16 forms and the planes form, each with a pitched residual
            j = si + ci
            rows.append(DW((1, 2, "planes")[j % 3], 2 + j % 2, H, W, C, flip=1, ops="r", ldr=r4(C) + 16))
            rows.append(DW((2, "planes", 1)[j % 3], 2, H, W, C, ops="bsr" if j % 2 else "r", ldr=r4(C) + 8, lds=420 if j % 2 else 0, acc=(j // 2) % 2))
    return rows


DW_ROWS = _dw_rows()


# ---------------------------------------------------------------------------------------------------------------------------------
# depthwise 7 x 7: weight gradient
# ---------------------------------------------------------------------------------------------------------------------------------
class WG(NamedTuple):
    """outs: letters of b (dbias), s (dsb); ld*: pitches of x, dy, dsb (0: r4(C))."""
    io: int
    B: int
    H: int
    W: int
    C: int
    acc: int = 1
    outs: str = "bs"
    ldx: int = 0
    lddy: int = 0
    ld_dsb: int = 0


def wg_call(r, ad=None, stream=0, io=None):
    io = r.io if io is None else io
    Cp = r4(r.C)
    s = "s" in r.outs
    base = (_at(ad, "x"), r.ldx or Cp, _at(ad, "dy"), r.lddy or Cp, _at(ad, "dw"), _at(ad, "dbias", "b" in r.outs), _at(ad, "dsb", s),
            (r.ld_dsb or Cp) if s else 0, _at(ad, "ws"), r.B, r.H, r.W, r.C, r.acc)
    return ("cdf_dwconv7_wgrad_io", base + (1, stream)) if io else ("cdf_dwconv7_wgrad", base + (stream,))


def _wg_case(be, r):
    B, H, W, C = r.B, r.H, r.W, r.C
    Cp = r4(C)
    ldx, lddy, ld_dsb = r.ldx or Cp, r.lddy or Cp, r.ld_dsb or Cp
    tag = "dwconv7 wgrad " + "-".join(map(str, r))
    g = torch.Generator().manual_seed(C * 17 + H * 3 + W)
    rn = lambda *s: torch.randn(*s, generator=g)
    q = (lambda t: t.bfloat16().float()) if r.io else (lambda t: t)
    x, dy = q(rn(B, H, W, Cp)), q(rn(B, H, W, Cp))
    x[..., C:], dy[..., C:] = 0, 0
    dw0, db0 = rn(C, 1, 7, 7), rn(C)
    nch = be.L.cdf_dwconv7_wgrad_nchunk(H)
    assert nch == min(32, max(1, H // 4))
    xp, dyp = _pitched(x, ldx), _pitched(dy, lddy)
    dw0d, db0d = be.to(dw0), be.to(db0)

    def go(io):
        xin, din = be.to(_bf(xp) if io else xp), be.to(_bf(dyp) if io else dyp)
        ws, dw, dbias, dsb = nan_empty(be, B * nch * 50 * C), nan_empty(be, C, 1, 7, 7), nan_empty(be, C), nan_empty(be, B, ld_dsb)
        name, args = wg_call(r, dict(x=P(xin), dy=P(din), dw=P(dw), dbias=P(dbias), dsb=P(dsb), ws=P(ws)), be.stream(), io)
        assert dw_wgrad_form(name, args) == dw_wgrad_form(*wg_call(r, io=io)), tag

        def launch():
            if r.acc:
                dw.copy_(dw0d)
                if "b" in r.outs:
                    dbias.copy_(db0d)
            getattr(be.L, name)(*args)
        return twice(launch, [dw, dbias, dsb, ws])[:3]
    form = dw_wgrad_form(*wg_call(r))
    print(f"{tag}: form {form} ({nch} chunks of {cdiv(H, nch)} rows)")
    dwo, dbo, dsbo = go(0)
    xx, dd = x[..., :C].permute(0, 3, 1, 2).double(), dy[..., :C].permute(0, 3, 1, 2).double()
    dw_r = torch.nn.grad.conv2d_weight(xx, (C, 1, 7, 7), dd, padding=3, groups=C)
    db_r, dsb_r = dd.sum((0, 2, 3)), dd.sum((2, 3))
    gb = min(K_SUM * U * math.sqrt(B * H * W) * xx.abs().max().item() * dd.pow(2).sum((0, 2, 3)).sqrt().max().item(), 5e-5 * max(1.0, dw_r.abs().max().item()))
    bb = min(sum_bound(dd.permute(1, 0, 2, 3).reshape(C, -1), 1), 5e-5 * max(1.0, db_r.abs().max().item()))
    if r.acc:
        dw_r, db_r = dw_r + dw0.double(), db_r + db0.double()
        gb, bb = gb + U * dw_r.abs().max().item(), bb + U * db_r.abs().max().item()
    _chk("dw wgrad", f"{tag} dw", dwo, dw_r, gb)
    if "b" in r.outs:
        _chk("dw wgrad", f"{tag} dbias", dbo, db_r, bb)
    else:
        assert _pads_poisoned(dbo, 0), (tag, "dbias is null in this call: its stand-in buffer must be untouched")
    if "s" in r.outs:                                        # dsb is overwritten whatever `accumulate` says (include/colddiff.h)
        _chk("dw wgrad", f"{tag} dsb", dsbo[:, :C], dsb_r, min(sum_bound(dd.reshape(B, C, -1), 2), 5e-5 * max(1.0, dsb_r.abs().max().item())))
        assert _pads_poisoned(dsbo, C), (tag, "a pad column of dsb changed")
    else:
        assert _pads_poisoned(dsbo, 0), (tag, "dsb is null in this call")
    if r.io:
        got = go(1)
        assert all(bits_equal(a_, b_) for a_, b_ in zip(got, (dwo, dbo, dsbo))), (tag, "bf16 operands: differs from the fp32 kernel on the widened values")
    return form


def _wg_rows():
    rows = []
    for i, W in enumerate((31, 32, 33)):                     # the kernel switch: narrow | wide | wide with a ragged second tile
        rows += [WG(i % 2, 2, 9, W, 3), WG((i + 1) % 2, 2, 9, W, 36, ldx=r4(36) + 28, lddy=r4(36) + 4, ld_dsb=420),
                 WG(0, 2, 9, W, 36, acc=0, outs="b"), WG(i % 2, 3, 9, W, 68, outs="")]
    # H = 37: 9 chunks of 5 rows, the last one empty; H = 132: the chunk count capped at 32, 5 rows each, the last five empty
    rows += [WG(0, 2, 37, 8, 36), WG(1, 2, 37, 33, 3, outs="b"), WG(0, 1, 132, 8, 3, ld_dsb=420), WG(1, 1, 132, 32, 3, ldx=12, lddy=8)]
    for (H, W) in ((12, 40), (40, 12)):                      # H != W: the kernel depends on W only, the chunks on H only
        rows += [WG(0, 2, H, W, 68, ldx=128, lddy=72), WG(1, 2, H, W, 130, ld_dsb=420), WG(0, 3, H, W, 130, outs="b", ldx=136), WG(1, 2, H, W, 36, acc=0)]
    return rows


WG_ROWS = _wg_rows()


# ---------------------------------------------------------------------------------------------------------------------------------
# channel LayerNorm
# ---------------------------------------------------------------------------------------------------------------------------------
def _ln_M(C, M, bwd=False):
    """M as a number: '1', 'g-1' / 'g+1' (one short of / past the rows of one block), 'cap+37' (37 rows past the smallest M that has
    cdf_layernorm_blocks(M, C) == 1024), '2nd+37' (37 rows into the second round of the waves of 1024 blocks)."""
    _, nv, gpb = ln_geom(C)
    unroll = (2 if nv <= 2 else 1) * (1 if bwd else 2)
    return {"1": 1, "g-1": gpb - 1, "g+1": gpb + 1, "cap+37": 1023 * gpb + 1 + 37, "2nd+37": 1024 * gpb * unroll + 37}[M] if isinstance(M, str) else M


class LF(NamedTuple):
    """out: present outputs of y, h (hi plane), l (lo plane), s (mean / rstd); io: x is bf16; off: per-(sample, channel) offset."""
    C: int
    M: object
    io: int = 0
    out: str = "ys"
    ldx: int = 0
    ldy: int = 0
    ldp: int = 0
    off: int = 0


def lf_call(r, ad=None, stream=0, io=None, out=None):
    io, out = (r.io if io is None else io), (r.out if out is None else out)
    C, M = r.C, _ln_M(r.C, r.M)
    h = "h" in out
    base = (_at(ad, "x"), r.ldx or C, _at(ad, "y", "y" in out), r.ldy or C, _at(ad, "g"), _at(ad, "b"), _at(ad, "mean", "s" in out), _at(ad, "rstd", "s" in out),
            M, C, 1e-5, _at(ad, "hi", h), _at(ad, "lo", "l" in out), (r.ldp or C) if h else 0)
    return ("cdf_layernorm_c_fwd_io", base + (1, stream)) if io else ("cdf_layernorm_c_fwd", base + (stream,))


def _ln_inputs(C, M, off, io_round):
    g_ = torch.Generator().manual_seed(C * 7 + M % 1000 + off)
    rn = lambda *s: torch.randn(*s, generator=g_)
    x, g, b, dy, add = rn(M, C), rn(C), rn(C), rn(M, C), rn(M, C)
    if off:
        x = x + _offset(M, C, 16, g_)
    if io_round:
        x = x.bfloat16().float()
    return x, g, b, dy, add


def _lf_case(be, r):
    C, M = r.C, _ln_M(r.C, r.M)
    ldx, ldy, ldp = r.ldx or C, r.ldy or C, r.ldp or C
    tag = "layernorm fwd " + "-".join(map(str, r)) + f" (M={M})"
    if isinstance(r.M, str) and r.M.startswith("cap"):
        assert be.L.cdf_layernorm_blocks(M - 38, C) < 1024 == be.L.cdf_layernorm_blocks(M - 37, C)
    x, g, b, _, _ = _ln_inputs(C, M, r.off, r.io)
    xp, gd, bd = _pitched(x, ldx), be.to(g), be.to(b)

    def go(io, out):
        xin = be.to(_bf(xp) if io else xp)
        y, mean, rstd = nan_empty(be, M, ldy), nan_empty(be, M), nan_empty(be, M)
        hi, lo = nan_empty(be, M, ldp, dtype=torch.int16), nan_empty(be, M, ldp, dtype=torch.int16)
        name, args = lf_call(r, dict(x=P(xin), y=P(y), g=P(gd), b=P(bd), mean=P(mean), rstd=P(rstd), hi=P(hi), lo=P(lo)), be.stream(), io, out)
        assert ln_fwd_form(name, args) == ln_fwd_form(*lf_call(r, io=io, out=out)), tag
        return twice(lambda: getattr(be.L, name)(*args), [y, mean, rstd, hi, lo])
    form = ln_fwd_form(*lf_call(r))
    print(f"{tag}: form {form}")
    yo, mo, ro, hi0, lo0 = go(0, "ys")
    y_r, mean_r, rstd_r = _ln_ref(x, g, b, x)[:3]
    scale = x.abs().max().item() if r.off else 1.0
    _chk("ln fwd", f"{tag} y", yo[:, :C], y_r, scale * min(5e-6, K_SUM * U * math.sqrt(C) * y_r.abs().max().item() * 4))
    _chk("ln fwd", f"{tag} mean", mo, mean_r, scale * 5e-6)
    _chk("ln fwd", f"{tag} rstd", ro, rstd_r, scale * 5e-6 * max(1.0, rstd_r.abs().max().item()))
    assert _pads_poisoned(yo, C) and _pads_poisoned(hi0, 0) and _pads_poisoned(lo0, 0), (tag, "a pad column of y, or a null plane's stand-in, changed")
    if (r.io, r.out) != (0, "ys"):
        y2, m2, r2, hi, lo = go(r.io, r.out)
        rh, rl = _split(be, be.to(yo[:, :C]))
        for letter, got, want, width in (("y", y2, yo, C), ("s", m2, mo, 0), ("s", r2, ro, 0), ("h", hi, rh.cpu(), C), ("l", lo, rl.cpu(), C)):
            if letter in r.out:
                assert bits_equal(got[..., :width], want[..., :width]) if width else bits_equal(got, want), (tag, letter, "differs from the fp32 y / its cdf_split_bf16")
                assert width == 0 or _pads_poisoned(got, C), (tag, letter, "a pad column changed")
            else:
                assert _pads_poisoned(got, 0), (tag, letter, "a null output's stand-in buffer changed")
    return form


def _lf_rows():
    rows = []
    for i, C in enumerate((8, 96, 260, 640, 768, 1024)):
        Ms = ("1", "g-1", "g+1")
        rows += [LF(C, Ms[i % 3]), LF(C, Ms[(i + 1) % 3], 0, "hl"), LF(C, Ms[(i + 2) % 3], 1, "h"), LF(C, Ms[i % 3], 1, "yhs", ldx=C + 8, ldy=C + 4, ldp=C + 16),
                 LF(C, Ms[(i + 1) % 3], 0, "y"), LF(C, "g+1", 0, "yhls", ldx=C + 64, ldp=C + 8), LF(C, "g-1", 1, "ys", ldx=C + 8)]
    rows += [LF(8, "cap+37", 0, "yhls"), LF(8, "cap+37", 1, "h", ldx=16), LF(8, "2nd+37", 0, "yhls", ldy=12)]
    rows += [LF(64, 256, 0, "ys", off=4), LF(640, 37, 0, "yhls", off=4)]
    return rows


LF_ROWS = _lf_rows()


class LB(NamedTuple):
    """io: 0, 7 (dy, x, dx bf16), 14 (x, dx, add bf16) or 'planes'; add: dx = grad + add; ld*: pitches of dy, x, dx, add, planes."""
    C: int
    M: object
    io: object = 0
    add: int = 0
    accdx: int = 0
    accp: int = 1
    lddy: int = 0
    ldx: int = 0
    lddx: int = 0
    ldadd: int = 0
    ldp: int = 0
    off: int = 0


def lb_call(r, ad=None, stream=0, io=None):
    io = r.io if io is None else io
    C, M = r.C, _ln_M(r.C, r.M, True)
    base = (_at(ad, "dy"), r.lddy or C, _at(ad, "x"), r.ldx or C, _at(ad, "g"), _at(ad, "mean"), _at(ad, "rstd"), _at(ad, "dx"), r.lddx or C,
            _at(ad, "add", r.add), (r.ldadd or C) if r.add else 0, _at(ad, "dg"), _at(ad, "db"), _at(ad, "part"), M, C, r.accdx, r.accp)
    if io == "planes":
        return "cdf_layernorm_c_bwd_planes", base + (_at(ad, "hi"), _at(ad, "lo"), r.ldp or C, stream)
    return ("cdf_layernorm_c_bwd_io", base + (io, stream)) if io else ("cdf_layernorm_c_bwd", base + (stream,))


def _lb_case(be, r):
    C, M = r.C, _ln_M(r.C, r.M, True)
    lddy, ldx, lddx, ldadd, ldp = (v or C for v in (r.lddy, r.ldx, r.lddx, r.ldadd, r.ldp))
    tag = "layernorm bwd " + "-".join(map(str, r)) + f" (M={M})"
    bf = r.io in (7, 14)
    x, g, b, dy, add = _ln_inputs(C, M, r.off, bf)
    q = lambda t: t.bfloat16().float()
    if r.io == 7:
        dy = q(dy)
    if r.io == 14:
        add = q(add)
    g_ = torch.Generator().manual_seed(C + 1)
    dx0, dg0, db0 = torch.randn(M, C, generator=g_), torch.randn(C, generator=g_), torch.randn(C, generator=g_)
    _, mean_r, rstd_r, dx_r, dg_terms, db_terms = _ln_ref(x, g, b, dy)
    gd, md, rd = be.to(g), be.to(mean_r.float()), be.to(rstd_r.float())          # (the statistics of the float64 reference, rounded once)
    dyp, xp, addp, dx0p = _pitched(dy, lddy), _pitched(x, ldx), _pitched(add, ldadd), _pitched(dx0, lddx)
    dg0d, db0d = be.to(dg0), be.to(db0)
    nb = be.L.cdf_layernorm_blocks(M, C)

    def go(io):
        dyin = be.to(_bf(dyp) if io == 7 else dyp)
        xin = be.to(_bf(xp) if io in (7, 14) else xp)
        addin = be.to(_bf(addp) if io == 14 else addp)
        dxb = io in (7, 14)
        dx = nan_empty(be, M, lddx, dtype=torch.int16 if dxb else torch.float32)
        old = be.to(_bf(dx0p) if dxb else dx0p)
        dg, db, part = nan_empty(be, C), nan_empty(be, C), nan_empty(be, nb * 2 * C)
        hi, lo = nan_empty(be, M, ldp, dtype=torch.int16), nan_empty(be, M, ldp, dtype=torch.int16)
        name, args = lb_call(r, dict(dy=P(dyin), x=P(xin), g=P(gd), mean=P(md), rstd=P(rd), dx=P(dx), add=P(addin), dg=P(dg), db=P(db), part=P(part),
                                     hi=P(hi), lo=P(lo)), be.stream(), io)
        assert ln_bwd_form(name, args) == ln_bwd_form(*lb_call(r, io=io)), tag

        def launch():
            if r.accdx:
                dx.copy_(old)
            if r.accp:
                dg.copy_(dg0d), db.copy_(db0d)
            getattr(be.L, name)(*args)
        return twice(launch, [dx, dg, db, hi, lo, part])[:5]
    form = ln_bwd_form(*lb_call(r))
    print(f"{tag}: form {form} ({nb} blocks)")
    dxo, dgo, dbo, hi0, lo0 = go(0)
    scale = x.abs().max().item() if r.off else 1.0
    dg_r, db_r, bdx = dg_terms.sum(0), db_terms.sum(0), scale * 1e-5
    bdg, bdb = scale * sum_bound(dg_terms, 0), sum_bound(db_terms, 0)
    if r.add:
        dx_r = dx_r + add.double()
    if r.accdx:
        dx_r = dx_r + dx0.double()
    if r.add or r.accdx:
        bdx += U * dx_r.abs().max().item()
    if r.accp:
        dg_r, db_r = dg_r + dg0.double(), db_r + db0.double()
        bdg, bdb = bdg + U * dg_r.abs().max().item(), bdb + U * db_r.abs().max().item()
    _chk("ln bwd", f"{tag} dx", dxo[:, :C], dx_r, bdx)
    _chk("ln bwd", f"{tag} dg", dgo, dg_r, bdg)
    _chk("ln bwd", f"{tag} db", dbo, db_r, bdb)
    assert _pads_poisoned(dxo, C) and _pads_poisoned(hi0, 0) and _pads_poisoned(lo0, 0), (tag, "a pad column of dx changed")
    if r.io:
        dx2, dg2, db2, hi, lo = go(r.io)
        assert bits_equal(dg2, dgo) and bits_equal(db2, dbo), (tag, "dg / db differ from the fp32 kernel on the widened values")
        assert _pads_poisoned(dx2, C), (tag, "a pad column of dx changed")
        if bf:
            assert torch.equal(dx2[:, :C].view(torch.bfloat16), dxo[:, :C].bfloat16()), (tag, "bf16 dx is not the fp32 result rounded once")
        else:
            assert bits_equal(dx2, dxo), (tag, "dx of the planes form differs")
            rh, rl = _split(be, be.to(dxo[:, :C]))
            assert torch.equal(hi[:, :C], rh.cpu()[:, :C]) and torch.equal(lo[:, :C], rl.cpu()[:, :C]), (tag, "planes are not cdf_split_bf16 of dx")
            assert _pads_poisoned(hi, C) and _pads_poisoned(lo, C), (tag, "a pad column of the planes changed")
    return form


def _lb_rows():
    rows = []
    for i, C in enumerate((8, 96, 260, 640, 768, 1024)):
        Ms = ("1", "g-1", "g+1")
        pl = "planes" if C % 8 == 0 else 0
        rows += [LB(C, Ms[i % 3]), LB(C, Ms[(i + 1) % 3], pl, add=1, ldadd=C + 8, ldp=C + 16), LB(C, Ms[(i + 2) % 3], 0, accdx=1, lddx=C + 4),
                 LB(C, Ms[i % 3], 7, lddy=C + 8, ldx=C + 4), LB(C, Ms[(i + 1) % 3], 14, add=1, ldx=C + 64), LB(C, "g+1", pl, accdx=1, lddy=C + 4, ldx=C + 8),
                 LB(C, "g-1", 0, accp=0), LB(C, "g+1", 14, add=1, ldadd=C + 8, lddx=C + 8), LB(C, "g-1", pl, ldx=C + 64)]
    rows += [LB(8, "cap+37", 0, add=1), LB(8, "cap+37", "planes", accdx=1, ldx=16), LB(8, "cap+37", 7), LB(8, "2nd+37", 0, add=1, lddx=12)]
    rows += [LB(64, 256, 0, off=4), LB(640, 37, "planes", add=1, off=4)]
    return rows


LB_ROWS = _lb_rows()


# ---------------------------------------------------------------------------------------------------------------------------------
# GroupNorm (+ SiLU + dropout)
# ---------------------------------------------------------------------------------------------------------------------------------
class GF(NamedTuple):
    """out: present outputs of y, h (hi plane), l (lo plane); p: dropout probability (seed SEED); off: per-(sample, channel) offset."""
    B: int
    HW: int
    C: int
    silu: int = 1
    p: float = 0.0
    out: str = "y"
    ldx: int = 0
    ldy: int = 0
    ldp: int = 0
    off: int = 0


GROUPS, GN_EPS = 32, 1e-6


def gf_call(r, ad=None, stream=0, out=None):
    out = r.out if out is None else out
    C, h = r.C, "h" in out
    return "cdf_groupnorm_fwd_ex", (_at(ad, "x"), r.ldx or C, _at(ad, "y", "y" in out), r.ldy or C, _at(ad, "ga"), _at(ad, "bt"), _at(ad, "mean"), _at(ad, "rstd"),
                                    _at(ad, "ws"), r.B, r.HW, C, GROUPS, GN_EPS, r.silu, float(r.p), SEED if r.p else 0, _at(ad, "hi", h), _at(ad, "lo", "l" in out),
                                    (r.ldp or C) if h else 0, stream)


def _gn_torch(x, ga, bt, dy, silu, dtype):
    """F.group_norm (+ SiLU) and its gradients in `dtype` on the CPU: (y, dx, dgamma, dbeta) -- in float32 the arithmetic whose own error
    the offset rows allow the kernel."""
    B, HW, C = x.shape
    xx, gad, btd = (t.to(dtype).requires_grad_(True) for t in (x, ga, bt))
    z = F.group_norm(xx.permute(0, 2, 1).reshape(B, C, HW, 1), GROUPS, gad, btd, eps=GN_EPS)
    y = (z * torch.sigmoid(z) if silu else z).reshape(B, C, HW).permute(0, 2, 1)
    y.backward(dy.to(dtype))
    return y.detach(), xx.grad, gad.grad, btd.grad


@functools.lru_cache(maxsize=3)
def _gn_data(B, HW, C, silu, p, off):
    """Inputs and float64 references of one (shape, silu, dropout, offset), shared by the forward and the backward rows (left unchanged):
    x, gamma, beta, dy, the dy the norm sees (masked and scaled), the kept mask, 1 / (1 - p), y, dx, dgamma, dbeta, mean, rstd."""
    g_ = torch.Generator().manual_seed(HW * 3 + C + off)
    rn = lambda *s: torch.randn(*s, generator=g_)
    x, ga, bt, dy = rn(B, HW, C), rn(C), rn(C), rn(B, HW, C)
    if off:
        x = x + _offset(B, C, 1, g_)[:, None, :]
    keep, inv = (_keep(B, HW, C, p) if p else (None, torch.tensor(1.0)))
    dye = torch.where(keep, dy * inv, torch.zeros(())) if p else dy               # (fp32 product, as the kernel forms it: exact agreement)
    y_r, dx_r, dga_r, dbt_r = _gn_ref(x, ga, bt, dye, GROUPS, silu)
    if p:
        y_r = torch.where(keep, y_r * inv.double(), torch.zeros((), dtype=torch.float64))
    xg = x.double().view(B, HW, GROUPS, C // GROUPS)
    mean = xg.mean((1, 3))
    rstd = (((xg - mean[:, None, :, None]) ** 2).mean((1, 3)) + GN_EPS).rsqrt()
    t32 = None
    if off:                                                  # the float32 reference arithmetic's own error on these inputs
        got = _gn_torch(x, ga, bt, dye, silu, torch.float32)
        t32 = [(a_.double() - b_).abs().max().item() for a_, b_ in zip(got, (y_r, dx_r, dga_r, dbt_r))]
    return dict(x=x, ga=ga, bt=bt, dy=dy, keep=keep, inv=inv.item(), y=y_r, dx=dx_r, dga=dga_r, dbt=dbt_r, mean=mean, rstd=rstd, t32=t32)


def _gn_bounds(B, HW, C, d):
    """(y, dx, dgamma / dbeta) bounds of test_kernels_production.test_groupnorm_production, times the dropout scale; offset rows: the larger
    of that and the float32 reference's own error."""
    grow_g, grow_r = math.sqrt(max(1.0, HW * C // GROUPS / 900)), math.sqrt(max(1.0, B * HW / 600))
    by, bdx, bp = 1e-5 * grow_g * d["inv"], 2e-5 * grow_g * d["inv"], 1e-4 * grow_r * d["inv"]
    if d["inv"] != 1.0:
        by += U * d["y"].abs().max().item()
    if d["t32"]:
        print(f"    F.group_norm float32 vs float64 on these inputs: y {d['t32'][0]:.2e}, dx {d['t32'][1]:.2e}, dgamma {d['t32'][2]:.2e}, dbeta {d['t32'][3]:.2e}"
              f" (the bounds without them: {by:.2e}, {bdx:.2e}, {bp:.2e})")
        return max(by, d["t32"][0]), max(bdx, d["t32"][1]), max(bp, d["t32"][2]), max(bp, d["t32"][3])
    return by, bdx, bp, bp


def _gf_case(be, r):
    B, HW, C = r.B, r.HW, r.C
    ldx, ldy, ldp = r.ldx or C, r.ldy or C, r.ldp or C
    tag = "groupnorm fwd " + "-".join(map(str, r))
    d = _gn_data(B, HW, C, r.silu, r.p, r.off)
    nch = be.L.cdf_groupnorm_nchunk(HW)
    assert nch == min(64, max(1, HW // 256))
    xd, gd, bd = be.to(_pitched(d["x"], ldx)), be.to(d["ga"]), be.to(d["bt"])

    def go(out):
        y, mean, rstd, ws = nan_empty(be, B, HW, ldy), nan_empty(be, B * GROUPS), nan_empty(be, B * GROUPS), nan_empty(be, B * nch * 2 * C)
        hi, lo = nan_empty(be, B, HW, ldp, dtype=torch.int16), nan_empty(be, B, HW, ldp, dtype=torch.int16)
        name, args = gf_call(r, dict(x=P(xd), y=P(y), ga=P(gd), bt=P(bd), mean=P(mean), rstd=P(rstd), ws=P(ws), hi=P(hi), lo=P(lo)), be.stream(), out)
        assert gn_fwd_form(name, args) == gn_fwd_form(*gf_call(r, out=out)), tag
        return twice(lambda: getattr(be.L, name)(*args), [y, mean, rstd, hi, lo, ws])[:5]
    form = gn_fwd_form(*gf_call(r))
    print(f"{tag}: form {form} ({nch} chunks of {cdiv(HW, nch)} rows)")
    yo, mo, ro, hi0, lo0 = go("y")
    by = _gn_bounds(B, HW, C, d)[0]
    _chk("gn fwd offset" if r.off else "gn fwd", f"{tag} y", yo[..., :C], d["y"], by)
    if r.p:
        assert bool(((yo[..., :C] == 0) | d["keep"]).all()), (tag, "a dropped element is not zero")
    assert _pads_poisoned(yo, C) and _pads_poisoned(hi0, 0) and _pads_poisoned(lo0, 0), (tag, "a pad column of y, or a null plane's stand-in, changed")
    if r.out != "y":
        y2, m2, r2, hi, lo = go(r.out)
        assert bits_equal(m2, mo) and bits_equal(r2, ro), (tag, "statistics differ between output forms")
        rh, rl = _split(be, be.to(yo[..., :C]).view(-1, C))
        for letter, got, want in (("y", y2.view(-1, ldy), yo.view(-1, ldy)), ("h", hi.view(-1, ldp), rh.cpu()), ("l", lo.view(-1, ldp), rl.cpu())):
            if letter in r.out:
                assert bits_equal(got[:, :C], want[:, :C]), (tag, letter, "differs from the fp32 y / its cdf_split_bf16")
                assert _pads_poisoned(got, C), (tag, letter, "a pad column changed")
            else:
                assert _pads_poisoned(got, 0), (tag, letter, "a null output's stand-in buffer changed")
    return form


# (B, HW): one chunk; two ragged chunks of 259 / 258 rows; 64 chunks of 257 rows, the last one short (16384 + 37 is exactly AT the cap:
# 16421 // 256 = 64; the cap takes effect from 65 x 256 rows, the rows with HW = 16640 + 37 below).  C: 1, 2, 3, 4, 8 channels per group
_GN_SHAPES = [(3, 64), (2, 517), (2, 16384 + 37)]
_GN_CS = [32, 64, 96, 128, 256]


def _gf_rows():
    rows = []
    for i, C in enumerate(_GN_CS):
        for j, (B, HW) in enumerate(_GN_SHAPES[:2]):
            rows += [GF(B, HW, C, silu=(i + j) % 2), GF(B, HW, C, silu=(i + j + 1) % 2, out=("yhl", "h", "hl")[(i + j) % 3], ldp=C + 8 * (j % 2)),
                     GF(B, HW, C, 1, (0.1, 0.25)[(i + j) % 2], out=("y", "yhl", "h")[(i + j) % 3])]
    # concat slices: the pitch of x exceeds C, y contiguous
    rows += [GF(3, 64, 32, ldx=96), GF(2, 517, 64, ldx=128, out="yhl"), GF(2, 517, 32, 0, 0.1, out="h", ldx=128), GF(3, 64, 64, ldx=96, ldy=72, out="yhl", ldp=80)]
    # past the chunk cap (the smallest channel counts: simulator time)
    rows += [GF(2, 16384 + 37, 32, 1, 0.1, out="yhl"), GF(2, 16384 + 37, 64, 0, ldx=96), GF(2, 16640 + 37, 32, 1, 0.1, out="hl"), GF(1, 16640 + 37, 64, 0)]
    # dropout in its three output forms at one shape
    rows += [GF(2, 517, 128, 1, 0.1, out=o) for o in ("y", "yhl", "h")]
    rows += [GF(2, 8200, 256, 1, 0.1, out="yhl")]            # past the apply-grid cap (4096 blocks of 256 float4)
    rows += [GF(2, 1024, 64, 1, off=4), GF(2, 1024, 64, 0, off=4, ldx=128)]
    return rows


GF_ROWS = _gf_rows()


class GB(NamedTuple):
    B: int
    HW: int
    C: int
    silu: int = 1
    p: float = 0.0
    accdx: int = 0
    accp: int = 0
    ldx: int = 0
    lddy: int = 0
    lddx: int = 0
    off: int = 0


def gb_call(r, ad=None, stream=0):
    C = r.C
    return "cdf_groupnorm_bwd_ex", (_at(ad, "dy"), r.lddy or C, _at(ad, "x"), r.ldx or C, _at(ad, "ga"), _at(ad, "bt"), _at(ad, "mean"), _at(ad, "rstd"), _at(ad, "dx"),
                                    r.lddx or C, _at(ad, "dga"), _at(ad, "dbt"), _at(ad, "ws"), r.B, r.HW, C, GROUPS, r.silu, r.accdx, r.accp, float(r.p),
                                    SEED if r.p else 0, stream)


def _gb_case(be, r):
    B, HW, C = r.B, r.HW, r.C
    ldx, lddy, lddx = r.ldx or C, r.lddy or C, r.lddx or C
    tag = "groupnorm bwd " + "-".join(map(str, r))
    d = _gn_data(B, HW, C, r.silu, r.p, r.off)
    nch = be.L.cdf_groupnorm_nchunk(HW)
    g_ = torch.Generator().manual_seed(C + HW)
    dx0, dga0, dbt0 = torch.randn(B, HW, C, generator=g_), torch.randn(C, generator=g_), torch.randn(C, generator=g_)
    xd, dyd, gd, bd = be.to(_pitched(d["x"], ldx)), be.to(_pitched(d["dy"], lddy)), be.to(d["ga"]), be.to(d["bt"])
    md, rd = be.to(d["mean"].float().reshape(-1)), be.to(d["rstd"].float().reshape(-1))      # (the float64 statistics, rounded once)
    old, dga0d, dbt0d = be.to(_pitched(dx0, lddx)), be.to(dga0), be.to(dbt0)
    dx, dga, dbt, ws = nan_empty(be, B, HW, lddx), nan_empty(be, C), nan_empty(be, C), nan_empty(be, B * nch * 2 * C + B * 2 * C + B * GROUPS * 2)
    name, args = gb_call(r, dict(dy=P(dyd), x=P(xd), ga=P(gd), bt=P(bd), mean=P(md), rstd=P(rd), dx=P(dx), dga=P(dga), dbt=P(dbt), ws=P(ws)), be.stream())
    form = gn_bwd_form(name, args)
    assert form == gn_bwd_form(*gb_call(r)), tag
    print(f"{tag}: form {form} ({nch} chunks of {cdiv(HW, nch)} rows)")

    def launch():
        if r.accdx:
            dx.copy_(old)
        if r.accp:
            dga.copy_(dga0d), dbt.copy_(dbt0d)
        getattr(be.L, name)(*args)
    dxo, dgo, dbo = twice(launch, [dx, dga, dbt, ws])[:3]
    _, bdx, bdg, bdb = _gn_bounds(B, HW, C, d)
    dx_r, dg_r, db_r = d["dx"], d["dga"], d["dbt"]
    if r.accdx:
        dx_r = dx_r + dx0.double()
        bdx += U * dx_r.abs().max().item()
    if r.accp:
        dg_r, db_r = dg_r + dga0.double(), db_r + dbt0.double()
        bdg, bdb = bdg + U * dg_r.abs().max().item(), bdb + U * db_r.abs().max().item()
    grp = "gn bwd offset" if r.off else "gn bwd"
    _chk(grp, f"{tag} dx", dxo[..., :C], dx_r, bdx)
    _chk(grp, f"{tag} dgamma", dgo, dg_r, bdg)
    _chk(grp, f"{tag} dbeta", dbo, db_r, bdb)
    assert _pads_poisoned(dxo, C), (tag, "a pad column of dx changed")
    return form


def _gb_rows():
    rows = []
    for i, C in enumerate(_GN_CS):
        for j, (B, HW) in enumerate(_GN_SHAPES[:2]):
            rows += [GB(B, HW, C, silu=(i + j) % 2), GB(B, HW, C, (i + j + 1) % 2, 0.0, 1, 1), GB(B, HW, C, 1, (0.1, 0.25)[(i + j) % 2], 1, 1),
                     GB(B, HW, C, (i + j) % 2, 0.0, 0, 1)]
    # the pitch of x exceeds C while dy and dx are contiguous (x a concat slice); and every tensor pitched
    rows += [GB(3, 64, 32, 1, 0.0, 1, 1, ldx=96), GB(2, 517, 64, 1, 0.1, 1, 1, ldx=128), GB(2, 517, 32, 0, 0.0, 1, 1, ldx=64), GB(3, 64, 64, 1, 0.25, 1, 1, ldx=96),
             GB(2, 517, 64, 0, 0.0, 1, 1, ldx=128, lddy=72, lddx=80), GB(2, 517, 32, 1, 0.1, 0, 0, ldx=96, lddy=40, lddx=36)]
    rows += [GB(2, 16384 + 37, 32, 1, 0.1, 1, 1), GB(2, 16384 + 37, 64, 0, 0.0, 1, 1, ldx=96), GB(2, 16640 + 37, 32, 1, 0.1, 1, 1), GB(1, 16640 + 37, 64, 0, 0.0, 0, 1)]
    rows += [GB(2, 8200, 256, 1, 0.1, 1, 1)]          # past the apply-grid cap, with dropout
    rows += [GB(2, 1024, 64, 1, off=4), GB(2, 1024, 64, 0, 0.0, 1, 1, off=4, ldx=128)]
    return rows


GB_ROWS = _gb_rows()


# ---------------------------------------------------------------------------------------------------------------------------------
# the tested forms; the forms the recordings reach
# ---------------------------------------------------------------------------------------------------------------------------------
CLASSIFIERS = {            # what -> (entry points, form function, rows, the row's (name, stand-in arguments))
    "dw": (DW_NAMES, dw_form, lambda: DW_ROWS, dw_call),
    "dw_wgrad": (DW_WGRAD_NAMES, dw_wgrad_form, lambda: WG_ROWS, wg_call),
    "ln_fwd": (LN_FWD_NAMES, ln_fwd_form, lambda: LF_ROWS, lf_call),
    "ln_bwd": (LN_BWD_NAMES, ln_bwd_form, lambda: LB_ROWS, lb_call),
    "gn_fwd": (GN_FWD_NAMES, gn_fwd_form, lambda: GF_ROWS, gf_call),
    "gn_bwd": (GN_BWD_NAMES, gn_bwd_form, lambda: GB_ROWS, gb_call),
}
ALL_NAMES = tuple(n for names, *_ in CLASSIFIERS.values() for n in names)


def forms_of_rows(what):
    _, form, rows, call = CLASSIFIERS[what]
    return {form(*call(r)) for r in rows()}


def reached_forms(calls):
    """{what: {form: (recording, name)}} of recorded (recording, name, arguments) calls."""
    out = {what: {} for what in CLASSIFIERS}
    for src, name, a in calls:
        for what, (names, form, _, _) in CLASSIFIERS.items():
            if name in names:
                out[what].setdefault(form(name, a), (src, name))
    return out


# The forms the recordings of test_gpu_invariance.py::test_coverage_guard reach (one bench step in bf16x3 and in bf16, one sampler step at
# B = 16, one forward + backward pass of config 2's network with dropout 0.1).  The guard fails when a recording reaches a form no row
# has, and when a form listed here is no longer reached.  Every other tested form is one no recording reaches.
REACHED = {
    "dw": {
        ('planes', '16x16', 1, 0, 'r', '', 1, 0),
        ('planes', '16x16', 1, 1, '', '', 1, 0),
        ('planes', '32x8', 1, 0, 'r', '', 1, 0),
        ('planes', '32x8', 1, 1, '', '', 1, 0),
        (0, '16x16', 0, 0, 'bs', 's', 1, 0),
        (0, '16x16', 0, 0, 'bs', 'xs', 1, 0),
        (0, '16x16', 1, 0, 'r', '', 1, 0),
        (0, '16x16', 1, 0, 'r', 'r', 1, 0),
        (0, '16x16', 1, 1, '', '', 1, 0),
        (0, '32x8', 0, 0, 'b', '', 1, 0),
        (0, '32x8', 0, 0, 'bs', 's', 0, 1),
        (0, '32x8', 0, 0, 'bs', 's', 1, 0),
        (0, '32x8', 1, 1, '', '', 1, 0),
        (1, '16x16', 0, 0, 'bs', 's', 1, 0),
        (1, '16x16', 0, 0, 'bs', 'xs', 1, 0),
        (1, '16x16', 1, 0, 'r', '', 1, 0),
        (1, '16x16', 1, 0, 'r', 'r', 1, 0),
        (1, '16x16', 1, 1, '', '', 1, 0),
        (1, '32x8', 0, 0, 'b', '', 1, 0),
        (1, '32x8', 0, 0, 'bs', 's', 1, 0),
        (1, '32x8', 1, 0, 'r', '', 1, 0),
        (1, '32x8', 1, 1, '', '', 1, 0),
        (2, '32x8', 1, 0, 'r', '', 1, 0),
    },
    "dw_wgrad": {
        (0, 'narrow', 0, 0, 1, 'bs', 's', 0),
        (0, 'narrow', 0, 0, 1, 'bs', 'xs', 0),
        (0, 'wide', 0, 0, 1, 'b', '', 0),
        (0, 'wide', 0, 0, 1, 'bs', 's', 0),
        (0, 'wide', 0, 0, 1, 'bs', 's', 1),
        (1, 'narrow', 0, 0, 1, 'bs', 's', 0),
        (1, 'narrow', 0, 0, 1, 'bs', 'xs', 0),
        (1, 'wide', 0, 0, 1, 'b', '', 0),
        (1, 'wide', 0, 0, 1, 'bs', 's', 0),
    },
    "ln_fwd": {
        (1, 0, 0, 'hls', '', 1, 0),
        (1, 0, 0, 'hls', '', 1, 1),
        (1, 0, 0, 'yhls', '', 1, 0),
        (1, 0, 0, 'yhls', '', 1, 1),
        (1, 0, 0, 'ys', '', 1, 0),
        (1, 0, 0, 'ys', '', 1, 1),
        (1, 0, 1, 'hs', '', 1, 0),
        (1, 0, 1, 'hs', '', 1, 1),
        (1, 0, 1, 'yhs', '', 1, 1),
        (1, 0, 1, 'ys', '', 1, 0),
        (1, 0, 1, 'ys', '', 1, 1),
        (2, 0, 0, 'hls', '', 1, 0),
        (2, 0, 0, 'hls', '', 1, 1),
        (2, 0, 0, 'ys', '', 1, 0),
        (2, 0, 1, 'hs', '', 1, 0),
        (2, 0, 1, 'hs', '', 1, 1),
        (2, 0, 1, 'ys', '', 1, 0),
        (4, 0, 0, 'hls', '', 1, 0),
        (4, 0, 0, 'hls', '', 1, 1),
        (4, 0, 1, 'hs', '', 1, 1),
    },
    "ln_bwd": {
        (1, 0, 'planes', 1, 0, 1, '', 1, 1),
        (1, 0, 0, 0, 0, 1, '', 1, 1),
        (1, 0, 14, 1, 0, 1, '', 1, 1),
        (1, 0, 7, 0, 0, 1, '', 1, 1),
        (2, 0, 'planes', 1, 0, 1, '', 1, 1),
        (2, 0, 0, 0, 0, 1, '', 1, 1),
        (2, 0, 14, 1, 0, 1, '', 1, 1),
        (2, 0, 7, 0, 0, 1, '', 1, 1),
        (4, 0, 0, 0, 0, 1, '', 1, 1),
        (4, 0, 7, 0, 0, 1, '', 1, 1),
    },
    "gn_fwd": {
        (4, 1, 0, '1', 0, 0, 0, 0, 0, 'y', ''),
        (4, 1, 0, '1', 0, 0, 0, 1, 0, 'hl', ''),
        (4, 1, 0, '1', 0, 0, 0, 1, 0, 'hl', 'x'),
        (4, 1, 0, '1', 0, 0, 0, 1, 1, 'hl', ''),
        (4, 1, 0, '1', 0, 0, 1, 0, 0, 'y', ''),
        (4, 1, 0, '1', 0, 0, 1, 1, 0, 'hl', ''),
        (4, 1, 0, '1', 0, 0, 1, 1, 0, 'hl', 'x'),
        (4, 1, 0, '1', 0, 0, 1, 1, 1, 'hl', ''),
        (4, 1, 0, 'many', 0, 0, 1, 1, 0, 'hl', ''),
        (4, 1, 0, 'many', 0, 0, 1, 1, 0, 'hl', 'x'),
        (4, 1, 0, 'many', 0, 0, 1, 1, 0, 'y', ''),
        (4, 1, 0, 'many', 0, 0, 1, 1, 1, 'hl', ''),
    },
    "gn_bwd": {
        (4, 1, 0, '1', 0, 0, 0, 0, 0, 1, 1, ''),
        (4, 1, 0, '1', 0, 0, 0, 1, 0, 1, 1, ''),
        (4, 1, 0, '1', 0, 0, 0, 1, 0, 1, 1, 'x'),
        (4, 1, 0, '1', 0, 0, 0, 1, 1, 0, 1, ''),
        (4, 1, 0, '1', 0, 0, 1, 0, 0, 1, 1, ''),
        (4, 1, 0, '1', 0, 0, 1, 1, 0, 1, 1, ''),
        (4, 1, 0, '1', 0, 0, 1, 1, 0, 1, 1, 'x'),
        (4, 1, 0, '1', 0, 0, 1, 1, 1, 0, 1, ''),
        (4, 1, 0, 'many', 0, 0, 1, 1, 0, 0, 1, ''),
        (4, 1, 0, 'many', 0, 0, 1, 1, 0, 1, 1, ''),
        (4, 1, 0, 'many', 0, 0, 1, 1, 0, 1, 1, 'x'),
        (4, 1, 0, 'many', 0, 0, 1, 1, 1, 0, 1, ''),
    },
}
# ... and the forms that one forward + backward pass of two small networks (test_recorded_norm_dw_forms_dry) reaches besides
SMALL_NETWORKS = {
    "dw": {
        (0, '32x8', 0, 0, 'b', '', 0, 0),
        (0, '32x8', 0, 0, 'bs', 's', 0, 0),
        (0, '32x8', 1, 0, 'r', '', 0, 0),
        (0, '32x8', 1, 1, '', '', 0, 0),
        (0, '32x8', 1, 1, '', '', 0, 1),
        (1, '32x8', 0, 0, 'b', '', 0, 0),
        (1, '32x8', 0, 0, 'bs', 's', 0, 0),
        (1, '32x8', 1, 0, 'r', '', 0, 0),
        (1, '32x8', 1, 1, '', '', 0, 0),
        (2, '32x8', 1, 0, 'r', '', 0, 0),
    },
    "dw_wgrad": set(),
    "ln_fwd": {
        (1, 0, 0, 'hls', '', 0, 0),
        (1, 0, 0, 'yhls', '', 0, 0),
        (1, 0, 0, 'ys', '', 0, 0),
        (1, 0, 1, 'hs', '', 0, 0),
        (1, 0, 1, 'yhs', '', 0, 0),
        (1, 0, 1, 'ys', '', 0, 0),
    },
    "ln_bwd": {
        (1, 0, 'planes', 1, 0, 1, '', 0, 0),
        (1, 0, 0, 0, 0, 1, '', 0, 0),
        (1, 0, 0, 1, 0, 1, '', 0, 0),
        (1, 0, 14, 1, 0, 1, '', 0, 0),
        (1, 0, 7, 0, 0, 1, '', 0, 0),
    },
    "gn_fwd": {
        (1, 0, 1, '1', 0, 0, 0, 1, 0, 'y', ''),
        (1, 0, 1, '1', 0, 0, 0, 1, 0, 'y', 'x'),
        (1, 0, 1, '1', 0, 0, 0, 1, 1, 'y', ''),
        (2, 0, 0, '1', 0, 0, 0, 0, 0, 'y', ''),
        (2, 0, 0, '1', 0, 0, 0, 1, 0, 'y', ''),
        (2, 0, 0, '1', 0, 0, 0, 1, 0, 'yh', ''),
        (2, 0, 0, '1', 0, 0, 0, 1, 0, 'yh', 'x'),
        (2, 0, 0, '1', 0, 0, 0, 1, 0, 'yhl', ''),
        (2, 0, 0, '1', 0, 0, 0, 1, 0, 'yhl', 'x'),
        (2, 0, 0, '1', 0, 0, 0, 1, 1, 'yh', ''),
        (2, 0, 0, '1', 0, 0, 0, 1, 1, 'yhl', ''),
        (3, 1, 1, '1', 0, 0, 0, 1, 0, 'y', ''),
        (3, 1, 1, '1', 0, 0, 0, 1, 0, 'yh', ''),
        (3, 1, 1, '1', 0, 0, 0, 1, 0, 'yhl', ''),
        (4, 1, 0, '1', 0, 0, 0, 1, 0, 'yh', ''),
        (4, 1, 0, '1', 0, 0, 0, 1, 0, 'yhl', ''),
    },
    "gn_bwd": {
        (1, 0, 1, '1', 0, 0, 0, 1, 0, 0, 1, ''),
        (1, 0, 1, '1', 0, 0, 0, 1, 0, 1, 1, 'x'),
        (1, 0, 1, '1', 0, 0, 0, 1, 1, 0, 1, ''),
        (2, 0, 0, '1', 0, 0, 0, 0, 0, 1, 1, ''),
        (2, 0, 0, '1', 0, 0, 0, 1, 0, 1, 1, ''),
        (2, 0, 0, '1', 0, 0, 0, 1, 0, 1, 1, 'x'),
        (2, 0, 0, '1', 0, 0, 0, 1, 1, 0, 1, ''),
        (3, 1, 1, '1', 0, 0, 0, 1, 0, 1, 1, ''),
    },
}


# ... with a row for each of them: the smallest shape of the form, built from the form itself (each builder is the inverse of its
# classifier; the assertion below holds it to that)
def _pitch(letters, c, C, step=8):
    """0 (the default pitch) or a pitch of its own beyond C for the operand with letter c."""
    return C + step * (1 + letters.index(c)) if c in letters else 0


def _dw_row_of(f):
    io, tile, flip, acc, ops, pit, multi, ragged = f
    C = {(0, 0): 32, (0, 1): 12, (1, 0): 64, (1, 1): 36}[(multi, ragged)]
    H, W = (18, 12) if tile == "16x16" else (10, 20)         # (H != W; more than one tile along H / W)
    return DW(io, 2, H, W, C, flip, acc, ops, _pitch(pit, "x", C, 32), _pitch(pit, "y", C), _pitch(pit, "w", C), 420 if "s" in pit else 0, _pitch(pit, "r", C))


def _wg_row_of(f):
    io, kind, capped, empty, acc, outs, pit, c4 = f
    H = {(0, 0): 8, (0, 1): 37, (1, 0): 160, (1, 1): 132}[(capped, empty)]
    C = 3 if c4 else 36
    return WG(io, 1 if capped else 2, H, 12 if kind == "narrow" else 36, C, acc, outs, _pitch(pit, "x", r4(C), 28), _pitch(pit, "d", r4(C)), 420 if "s" in pit else 0)


_LN_ROWS = {(0, 0): "g+1", (1, 0): "cap+37", (1, 1): "2nd+37"}
_LN_C = {(1, 0): 64, (1, 1): 96, (2, 0): 512, (2, 1): 260, (3, 0): 768, (3, 1): 640, (4, 0): 1024, (4, 1): 900}


def _lf_row_of(f):
    nv, idle, io, out, pit, capped, second = f
    C = _LN_C[(nv, idle)]
    return LF(C, _LN_ROWS[(capped, second)], io, out, _pitch(pit, "x", C, 32), _pitch(pit, "y", C), _pitch(pit, "p", C))


def _lb_row_of(f):
    nv, idle, io, add, accdx, accp, pit, capped, second = f
    C = _LN_C[(nv, idle)]
    return LB(C, _LN_ROWS[(capped, second)], io, add, accdx, accp, _pitch(pit, "d", C), _pitch(pit, "x", C, 32), _pitch(pit, "o", C), _pitch(pit, "a", C), _pitch(pit, "p", C))


def _gn_shape_of(f):
    cgc, cb, cragged, nclass, ragged, tail, capped = f[:7]
    C = {(1, 0, 1): 32, (2, 0, 0): 64, (3, 1, 1): 96, (4, 1, 0): 128}[(cgc, cb, cragged)]
    HW = {("1", 0, 0): 64, ("many", 0, 0): 512, ("many", 1, 1): 517, ("capped", 1, 1): 16640 + 37}[(nclass, ragged, tail)]
    B = 4096 * 256 // (HW * (C // 4)) + 1 if capped else 2   # (capped: the apply kernels' grid-stride walk, one element past 4096 blocks)
    return B, HW, C


def _gf_row_of(f):
    silu, drop, out, pit = f[7:]
    B, HW, C = _gn_shape_of(f)
    return GF(B, HW, C, silu, 0.1 if drop else 0.0, out, _pitch(pit, "x", C, 32), _pitch(pit, "y", C), _pitch(pit, "p", C))


def _gb_row_of(f):
    silu, drop, accdx, accp, pit = f[7:]
    B, HW, C = _gn_shape_of(f)
    return GB(B, HW, C, silu, 0.1 if drop else 0.0, accdx, accp, _pitch(pit, "x", C, 32), _pitch(pit, "d", C), _pitch(pit, "o", C))


for _what, _rows, _of in (("dw", DW_ROWS, _dw_row_of), ("dw_wgrad", WG_ROWS, _wg_row_of), ("ln_fwd", LF_ROWS, _lf_row_of), ("ln_bwd", LB_ROWS, _lb_row_of),
                          ("gn_fwd", GF_ROWS, _gf_row_of), ("gn_bwd", GB_ROWS, _gb_row_of)):
    for _f in sorted(REACHED[_what] | SMALL_NETWORKS[_what], key=repr):
        if _f not in forms_of_rows(_what):
            _rows.append(_of(_f))
            assert CLASSIFIERS[_what][1](*CLASSIFIERS[_what][3](_rows[-1])) == _f, (_what, _f, _rows[-1])


def test_form_tables():
    """The tables keep what they were built for, and the forms flagged as reached are tested forms."""
    for what in CLASSIFIERS:
        t = forms_of_rows(what)
        assert REACHED[what] | SMALL_NETWORKS[what] <= t, (what, sorted((REACHED[what] | SMALL_NETWORKS[what]) - t, key=repr))
        assert t - REACHED[what], what
    dw = forms_of_rows("dw")
    for tile in ("16x16", "32x8"):
        fs = {f for f in dw if f[1] == tile}
        assert {f[0] for f in fs} == {0, 1, 2, "planes"} and {f[2:4] for f in fs} >= {(0, 0), (1, 1), (1, 0), (0, 1)}, tile
        assert {f[4] for f in fs} >= {"", "b", "bs", "r", "bsr"} and any(f[5] == "xywsr" for f in fs), tile
        assert any("r" in f[5] and f[0] == io for f in fs for io in (1, 2, "planes")) and {f[6:] for f in fs} >= {(0, 1), (1, 1)}, tile
    assert {(r.H, r.W) for r in DW_ROWS} >= {(5, 16), (16, 17), (9, 33), (12, 40), (40, 12)} and {r.C for r in DW_ROWS} >= {3, 36, 68}
    wg = forms_of_rows("dw_wgrad")
    assert {f[:2] for f in wg} == {(0, "narrow"), (0, "wide"), (1, "narrow"), (1, "wide")} and {f[2:4] for f in wg} == {(0, 0), (0, 1), (1, 1)}
    assert {f[4] for f in wg} == {0, 1} and {f[5] for f in wg} == {"", "b", "bs"} and {f[6] for f in wg} >= {"", "xd", "s", "xds"} and {f[7] for f in wg} == {0, 1}
    assert {r.W for r in WG_ROWS} >= {31, 32, 33} and {r.H for r in WG_ROWS} >= {37, 132} and {r.C for r in WG_ROWS} >= {3, 36, 68, 130}
    lf, lb = forms_of_rows("ln_fwd"), forms_of_rows("ln_bwd")
    for fs in (lf, lb):
        assert {f[:2] for f in fs} >= {(1, 0), (1, 1), (2, 0), (2, 1), (3, 1), (3, 0), (4, 0)} and {f[-2:] for f in fs} == {(0, 0), (1, 0), (1, 1)}
    assert {f[2:4] for f in lf} >= {(0, "hl"), (1, "h"), (1, "yhs"), (0, "y"), (0, "ys"), (0, "yhls")} and any(f[4] == "xyp" for f in lf)
    assert {f[2] for f in lb} == {0, 7, 14, "planes"} and {f[3:6] for f in lb} >= {(0, 0, 1), (1, 0, 1), (0, 1, 1), (0, 0, 0)}
    assert {(14, 1), ("planes", 1)} <= {f[2:4] for f in lb} and set("dxoap") <= set("".join(f[6] for f in lb))
    for what, at in (("gn_fwd", 7), ("gn_bwd", 7)):
        fs = forms_of_rows(what)
        assert {f[0] for f in fs} == {1, 2, 3, 4} and {f[1:3] for f in fs} == {(0, 0), (0, 1), (1, 0), (1, 1)} and {f[3] for f in fs} == {"1", "many", "capped"}
        assert {f[6] for f in fs} == {0, 1} and {f[at:at + 2] for f in fs} >= {(0, 0), (1, 0), (1, 1)}
    assert {f[9] for f in forms_of_rows("gn_fwd")} >= {"y", "yhl", "h", "hl"} and {f[8:10] for f in forms_of_rows("gn_fwd")} >= {(1, "y"), (1, "yhl"), (1, "h")}
    gb = forms_of_rows("gn_bwd")
    assert {f[8:11] for f in gb} >= {(0, 0, 0), (0, 1, 1), (1, 1, 1), (0, 0, 1)} and {f[11] for f in gb} >= {"", "x", "dxo"}
    assert any(f[7] == 0 and f[9:11] == (1, 1) for f in gb)


def _small_networks():
    """One forward + backward pass of a small Unet (dim 32, 48 x 48) and of a small Model (ch 32, 16 x 16, dropout 0.1, training mode)."""
    import test_gpu_invariance as gi
    from denoising_diffusion_pytorch import Unet
    from deblurring_diffusion_pytorch import Model
    torch.manual_seed(3)
    for net, x in ((gi.quiet(Unet, dim=32, dim_mults=(1, 2, 4), channels=3), torch.randn(2, 3, 48, 48)),
                   (gi.quiet(Model, resolution=16, in_channels=3, out_ch=3, ch=32, ch_mult=(1, 2), num_res_blocks=1, attn_resolutions=(8,), dropout=0.1),
                    torch.randn(2, 3, 16, 16))):
        net.train()
        x = x.requires_grad_(True)
        net(x, torch.randint(0, 1000, (2,))).backward(torch.randn(2, 3, *x.shape[2:]) / 100)


def test_recorded_norm_dw_forms_dry(monkeypatch):
    """The recordings of test_gpu_invariance.py::test_coverage_guard without a GPU (the technique of
    test_gemm_f32_forms.py::test_recorded_forms_dry: real shapes, CPU tensors, every launching entry point a stub that returns 0 -- the
    argument tuples are decided by the Python layer from shapes and modes alone), held to the guard's two assertions; and the same for
    two small networks in both arithmetic modes, whose forms must be tested forms and agree with the flagged sets wherever both record."""
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
    monkeypatch.setattr(gi, "_GEMM_FAMILY", ALL_NAMES)
    _, _, calls = gi._guard_calls(p2.bench_step_inputs())
    reached = reached_forms([c for c in calls if c[1] in ALL_NAMES])
    small = []
    for mode in ("bf16x3", "bf16"):
        with rt.precision_scope(mode), gi.Recorder(stub) as rec:
            _small_networks()
        small += [("small " + mode, n, a) for n, a in rec.calls if n in ALL_NAMES]
    small = reached_forms(small)
    for what in CLASSIFIERS:
        print(f"{what} forms reached:", *sorted(reached[what], key=repr), sep="\n    ")
        print(f"{what} forms the small networks reach besides:", *sorted(set(small[what]) - set(reached[what]), key=repr), sep="\n    ")
    for what in CLASSIFIERS:
        tested = forms_of_rows(what)
        assert reached[what] and small[what], what
        for src, r_ in (("the recordings", reached[what]), ("the small networks", small[what])):
            assert set(r_) <= tested, (what, src, sorted(set(r_) - tested, key=repr))
        assert REACHED[what] == set(reached[what]), (what, sorted(REACHED[what] ^ set(reached[what]), key=repr))


# ---------------------------------------------------------------------------------------------------------------------------------
# the tests over the case tables (both backends)
# ---------------------------------------------------------------------------------------------------------------------------------
_ids = lambda r: "-".join(map(str, r))


@pytest.mark.parametrize("r", DW_ROWS, ids=_ids)
def test_dwconv7_forms(be, r):
    _dw_case(be, r)


@pytest.mark.parametrize("r", WG_ROWS, ids=_ids)
def test_dwconv7_wgrad_forms(be, r):
    _wg_case(be, r)


@pytest.mark.parametrize("r", LF_ROWS, ids=_ids)
def test_layernorm_fwd_forms(be, r):
    _lf_case(be, r)


@pytest.mark.parametrize("r", LB_ROWS, ids=_ids)
def test_layernorm_bwd_forms(be, r):
    _lb_case(be, r)


@pytest.mark.parametrize("r", GF_ROWS, ids=_ids)
def test_groupnorm_fwd_forms(be, r):
    _gf_case(be, r)


@pytest.mark.parametrize("r", GB_ROWS, ids=_ids)
def test_groupnorm_bwd_forms(be, r):
    _gb_case(be, r)
