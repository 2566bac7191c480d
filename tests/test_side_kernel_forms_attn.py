"""The side kernels between the GEMMs, second half -- csrc/k_attn.hip and csrc/k_attn_kvctx.hip (linear attention: context forward and
backward, the k / v backward in fp32 and as bf16 planes, the fused k | v projection + context and the fold of its partials, the dctx
finish, the unfused softk / dk pair; the attention block's row softmax) -- in every argument form the product launches.  Conventions,
helpers, recordings and the guard: test_side_kernel_forms.py (which holds the seeded-fault table and the totals of both modules).

What the older tests of these kernels never pass and the product does: the (k|v) layout (koff = 0) at a ragged n -- the small Unet reaches
cdf_linattn_context(ld = 256, koff = 0) at n = 2304 / 576 / 144; besides, pitched operands (ld = width + 8) with NaN pads, dk | dv written
inside a wider poisoned tensor or at another channel offset than k's, 1 to 3 heads, more than 32 splits / partials (n = 33 x 256 + 44; the
finalize kernel strides its statistics over 32 split lanes), the two-pass context kernels, kvctx at dim = 96 (BK = 32) and with slots that
give one part of several tiles, parts of unequal length and 34 parts, finalize on synthetic partials whose maxima are up to 12 apart.
Softmax corner columns (every context and softk row): k column 0 constant -- kmax = the value and ksum = n EXACTLY (exp(0) = 1 sums exactly
in fp32); column 1 with its maximum in the last row (the ragged tile), 60 above the rest; column 2 with one pixel 40 above all others --
its context row is that pixel's v row within ctx's bound.

References (float64, CPU): plain softmaxes, sums and einsums.  Bounds, no new constant:
  context, kvctx, finalize   kmax exact, ksum 1e-5 |ksum|max, ctx / ctxs 2e-5 max(1, |ctx|max); kv (3e-5, hi-only 2e-2) |kv|max
                             (test_kernels_production.py::test_linattn_kvctx_production)
  bwd_kv                     dk, dv 2e-5 max(1, |ref|max); planes bit-equal cdf_split_bf16 of the fp32 result (test_linattn_bwd_kv_planes_production)
  dctx_finish                dctx 2^-24 |dctx|max, rvec sum_bound + dctx's rounding through |ctx| (test_linattn_dctx_finish_production)
  dcontext                   dctx: a sum over n, sum_bound's model, times the scale, plus one rounding; rvec: dctx_finish's bound with that
                             error in place of one rounding
  softk, row softmax         1e-6 absolute (test_kernels.py's row softmax: values <= 1); dk: the subtraction and the product, one rounding
                             each, of the P the kernel wrote: 2 2^-24 |P| (|dP| + |r|)

Cases: context 36, dcontext 24, bwd_kv 54, kvctx 17, finalize 8, dctx_finish 7, softk + dk 7, row softmax 10; with the table and dry tests
165 on the simulator (45 s in one process) and 163 on the MI355X (2 s).  GPU-only: 1 row, softk / dk past the 8192-block grid cap
(B = 17, n = 4093: 8.9M elements).
Worst error / bound per output, simulator | MI355X:
    (equal to two digits except where noted)
    context       ksum 0.01  ctx 0.01  ctxs 0.00  the one-pixel row 0.00          dcontext   dctx 0.19  rvec 0.02
    bwd_kv        dk 0.00    dv 0.01                                              finalize   ksum 0.03  ctx 0.00  ctxs 0.00
    kvctx         kv 0.71    ksum 0.04 | 0.03     ctx 0.06 | 0.07    ctxs 0.01    dctx_finish  dctx 0.84  rvec 0.12
    softk         pn 0.03    dk 0.48                                              row softmax  p 0.08  ds 0.01
Reached forms: REACHED / SMALL_NETWORKS below (context 2 + 3, dcontext 2, bwd_kv 6 + 5, kvctx 7, finalize 1, dctx_finish 1 + 1, row softmax 4 + 2;
the unfused softk / dk pair is a switch of the Python layer that no recording turns on).
"""
import math
from typing import NamedTuple

import pytest
import torch

from poison import nan_empty
from test_kernels import P, _split
from test_kernels_production import K_SUM, U, bits_equal, skip_emu, sum_bound, twice
from test_side_kernel_forms import _amax, _at, _chk, _letters, _null, _pitched, _poisoned, cdiv

LA_NAMES = ("cdf_linattn_context", "cdf_linattn_dcontext", "cdf_linattn_bwd_kv", "cdf_linattn_bwd_kv_planes", "cdf_linattn_kvctx", "cdf_linattn_finalize",
            "cdf_linattn_dctx_finish", "cdf_linattn_softk", "cdf_linattn_dk", "cdf_softmax_rows_fwd", "cdf_softmax_rows_bwd")
SCALE = 32 ** -0.5


# ---------------------------------------------------------------------------------------------------------------------------------
# forms: pure functions of (entry point, argument tuple)
# ---------------------------------------------------------------------------------------------------------------------------------
def _count(n):
    """'1' / 'several' / '>32': the finalize kernel strides its statistics over 32 split lanes, so the 33rd partial is a lane's second."""
    return "1" if n == 1 else ("several" if n <= 32 else ">32")


def _layout(koff, HD):
    return "qkv" if koff == HD else ("kv" if koff == 0 else "other")


def la_context_form(name, a):
    """cdf_linattn_context: (layout '(q|k|v)' with koff = HD or '(k|v)' with koff = 0; heads; the pitch exceeds koff + 2 HD; onepass;
    splits of 256 rows '1' / 'several' / '>32'; a ragged last 256-row tile)."""
    ld, koff, B, n, heads, onepass = a[1], a[2], a[8], a[9], a[10], a[12]
    HD = heads * 32
    ns = cdiv(n, 256)
    return (_layout(koff, HD), heads, int(ld > koff + 2 * HD), int(bool(onepass) and ns <= 1024), _count(ns), int(n % 256 != 0))


def la_dcontext_form(name, a):
    """cdf_linattn_dcontext: (heads; q's pitch 'hd' (= HD), '3hd' (the (q|k|v) tensor) or 'other'; dout pitched; splits; a ragged last split)."""
    ld, lddo, B, n, heads = a[1], a[3], a[8], a[9], a[10]
    HD = heads * 32
    return (heads, "hd" if ld == HD else ("3hd" if ld == 3 * HD else "other"), int(lddo > HD), _count(cdiv(n, 256)), int(n % 256 != 0))


def la_bwd_kv_form(name, a):
    """cdf_linattn_bwd_kv / _planes: (output 'f32', 'hl' (both planes) or 'h' (lo null); layout of the input; heads; pitched i(nput) o(utput)
    beyond offset + 2 HD; dk | dv at the input's channel offset; blocks of 256 pixels '1' / 'several' / '>32'; a ragged last block;
    a ragged last 32-pixel tile)."""
    ld, koff = a[1], a[2]
    if name == "cdf_linattn_bwd_kv_planes":
        out, ldo, dkoff, B, n, heads = ("h" if _null(a[8]) else "hl"), a[9], a[10], a[11], a[12], a[13]
    else:
        out, ldo, dkoff, B, n, heads = "f32", a[8], a[9], a[10], a[11], a[12]
    HD = heads * 32
    return (out, _layout(koff, HD), heads, _letters("io", (ld > koff + 2 * HD, ldo > dkoff + 2 * HD)), int(dkoff == koff), _count(cdiv(n, 256)), int(n % 256 != 0),
            int(n % 32 != 0))


def kvctx_parts(B, n, slots):
    """(parts per image, tiles per block) of cdf_linattn_kvctx_parts / cdf_linattn_kvctx."""
    tiles = n // 128
    p = min(tiles, max(1, (slots if slots > 0 else 512) // B))
    tpb = cdiv(tiles, p)
    return cdiv(tiles, tpb), tpb


def la_kvctx_form(name, a):
    """cdf_linattn_kvctx: (lo plane null; BK 64 or 32 (dim % 64); K chunks per tile '1' / 'several'; pitched x w k(v); parts per image '1' /
    'several' / '>32'; tiles per block '1' / 'several'; a shorter last block)."""
    ldx, lo, ldk, ldkv, B, n, dim, heads, slots = a[1], a[3], a[4], a[6], a[8], a[9], a[10], a[11], a[12]
    parts, tpb = kvctx_parts(B, n, slots)
    bk = 64 if dim % 64 == 0 else 32
    return (int(_null(lo)), bk, "1" if dim == bk else "several", _letters("xwk", (ldx > dim, ldk > dim, ldkv > 256)), _count(parts),
            "1" if tpb == 1 else "several", int((n // 128) % tpb != 0))


def la_finalize_form(name, a):
    """cdf_linattn_finalize: (heads; parts '1' / 'several' / '>32'; parts % 4 != 0: the context fold's four chains have a tail)."""
    return (a[7], _count(a[1]), int(a[1] % 4 != 0))


def la_dctx_finish_form(name, a):
    """cdf_linattn_dctx_finish: (blocks of 8 rows '1' / 'several' / '>32'; a ragged last block)."""
    return (_count(cdiv(a[4], 8)), int(a[4] % 8 != 0))


def _ew_capped(B, n, HD):
    return int(cdiv(B * n * HD // 4, 256) > 8192)


def la_softk_form(name, a):
    """cdf_linattn_softk: (heads; pitched i(nput) beyond 3 HD, o(utput) beyond HD; grid capped at 8192 blocks)."""
    ld, ldp, B, n, heads = a[1], a[5], a[6], a[7], a[8]
    return (heads, _letters("io", (ld > 3 * heads * 32, ldp > heads * 32)), _ew_capped(B, n, heads * 32))


def la_dk_form(name, a):
    """cdf_linattn_dk: (heads; pitched p d(p) o (dk) beyond HD; grid capped at 8192 blocks)."""
    ldp, lddp, lddk, B, n, heads = a[1], a[3], a[6], a[7], a[8], a[9]
    HD = heads * 32
    return (heads, _letters("pdo", (ldp > HD, lddp > HD, lddk > HD)), _ew_capped(B, n, HD))


def softmax_rows_form(name, a):
    """cdf_softmax_rows_fwd / _bwd: ('fwd' / 'bwd'; n '<=64' (one trip per lane) or '>64'; n % 64 != 0; pitched; grid capped at 4096 blocks of
    four rows)."""
    rows, n, ld = (a[2], a[3], a[4]) if name == "cdf_softmax_rows_fwd" else (a[3], a[4], a[5])
    return (name[-3:], "<=64" if n <= 64 else ">64", int(n % 64 != 0), int(ld > n), int(cdiv(rows, 4) > 4096))


# ---------------------------------------------------------------------------------------------------------------------------------
# context (forward): cdf_linattn_context, with the softmax corner columns
# ---------------------------------------------------------------------------------------------------------------------------------
def _kv_inputs(B, n, heads, layout, ld, seed, corner=True):
    """A (q|k|v) or (k|v) tensor [B, n, ld] with NaN pad columns, and k, v [B, n, HD].  corner: three k columns of head 0 are special --
    column 0 constant (kmax = the value and ksum = n exactly: exp(0) = 1 sums exactly in fp32), column 1 with its maximum in the LAST row
    (the ragged tile when there is one), 60 above the rest, column 2 with one pixel 40 above all others (its context row is that pixel's v row)."""
    HD = heads * 32
    g = torch.Generator().manual_seed(seed)
    width = (3 if layout == "qkv" else 2) * HD
    t = torch.randn(B, n, width, generator=g)
    koff = HD if layout == "qkv" else 0
    k, v = t[..., koff:koff + HD], t[..., koff + HD:koff + 2 * HD]
    if corner:
        k[..., 0] = 0.75
        k[:, n - 1, 1] = k[..., 1].max() + 60
        k[:, n // 3, 2] = k[..., 2].max() + 40
    return _pitched(t, ld or width), k, v, koff


def _ctx_ref(k, v, heads):
    """float64: (kmax, ksum, ctx [B, heads, 32, 32]) of k, v [B, n, HD]."""
    B, n, HD = k.shape
    kd, vd = k.double(), v.double()
    kmax = kd.max(1).values
    e = torch.exp(kd - kmax[:, None])
    ksum = e.sum(1)
    ctx = torch.einsum("bnhd,bnhe->bhde", (e / ksum[:, None]).view(B, n, heads, 32), vd.view(B, n, heads, 32))
    return kmax, ksum, ctx


def _ctx_checks(group, tag, ctxo, ctxso, kmaxo, ksumo, kmax_r, ksum_r, ctx_r):
    """The bounds of test_kernels_production.py::test_linattn_kvctx_production: kmax exact, ksum 1e-5 of its max, ctx / ctxs 2e-5 of max(1, |ctx|max)."""
    assert torch.equal(kmaxo, kmax_r.float()), (tag, "kmax")
    _chk(group, f"{tag} ksum", ksumo, ksum_r, 1e-5 * _amax(ksum_r))
    _chk(group, f"{tag} ctx", ctxo, ctx_r, 2e-5 * max(1.0, _amax(ctx_r)))
    _chk(group, f"{tag} ctxs", ctxso, ctx_r * torch.tensor(SCALE, dtype=torch.float32).double(), 2e-5 * max(1.0, _amax(ctx_r)))


class AC(NamedTuple):
    B: int
    n: int
    layout: str = "kv"
    ld: int = 0
    onepass: int = 1
    heads: int = 4
    big: bool = False


def ac_call(r, ad=None, stream=0):
    HD = r.heads * 32
    width = (3 if r.layout == "qkv" else 2) * HD
    return "cdf_linattn_context", (_at(ad, "qkv"), r.ld or width, HD if r.layout == "qkv" else 0, _at(ad, "ctx"), _at(ad, "ctxs"), _at(ad, "kmax"), _at(ad, "ksum"),
                                   _at(ad, "ws"), r.B, r.n, r.heads, SCALE, r.onepass, stream)


def _ac_case(be, r):
    skip_emu(be, r.big)
    B, n, heads = r.B, r.n, r.heads
    HD = heads * 32
    tag = "linattn context " + "-".join(map(str, r))
    t, k, v, _ = _kv_inputs(B, n, heads, r.layout, r.ld, n * 3 + heads + r.onepass)
    td = be.to(t)
    ctx, ctxs, kmax, ksum = nan_empty(be, B, heads, 32, 32), nan_empty(be, B, heads, 32, 32), nan_empty(be, B, HD), nan_empty(be, B, HD)
    ws = nan_empty(be, be.L.cdf_linattn_ws_floats(B, n, heads))
    assert be.L.cdf_linattn_nsplit(n) == cdiv(n, 256)
    name, args = ac_call(r, dict(qkv=P(td), ctx=P(ctx), ctxs=P(ctxs), kmax=P(kmax), ksum=P(ksum), ws=P(ws)), be.stream())
    form = la_context_form(*ac_call(r))
    assert la_context_form(name, args) == form, tag
    print(f"{tag}: form {form}")
    ctxo, ctxso, kmaxo, ksumo = twice(lambda: getattr(be.L, name)(*args), [ctx, ctxs, kmax, ksum, ws])[:4]
    kmax_r, ksum_r, ctx_r = _ctx_ref(k, v, heads)
    _ctx_checks("context", tag, ctxo, ctxso, kmaxo, ksumo, kmax_r, ksum_r, ctx_r)
    assert (kmaxo[:, 0] == 0.75).all() and (ksumo[:, 0] == float(n)).all(), (tag, "the constant column: kmax = the value, ksum = n, exactly")
    _chk("context", f"{tag} the one-pixel column's context row", ctxo[:, 0, 2], v[:, n // 3, :32].double(), 2e-5 * max(1.0, _amax(ctx_r)))
    return form


AC_ROWS = ([AC(2, n, lay, ld, op) for n in (16, 144, 256, 300, 576) for lay, ld, op in (("kv", 0, 1), ("qkv", 0, 1), ("kv", 264, 1), ("qkv", 392, 1), ("kv", 0, 0), ("qkv", 392, 0))]
           + [AC(1, 33 * 256 + 44, "kv", 264, 1), AC(1, 33 * 256 + 44, "qkv", 0, 0), AC(2, 300, "kv", 136, 1, 2), AC(2, 300, "qkv", 0, 1, 2)])


# ---------------------------------------------------------------------------------------------------------------------------------
# context (backward): cdf_linattn_dcontext
# ---------------------------------------------------------------------------------------------------------------------------------
class AD(NamedTuple):
    B: int
    n: int
    ld: int = 0        # 0: the (q|k|v) tensor, 3 HD
    lddo: int = 0
    heads: int = 4


def ad_call(r, ad=None, stream=0):
    HD = r.heads * 32
    return "cdf_linattn_dcontext", (_at(ad, "q"), r.ld or 3 * HD, _at(ad, "do"), r.lddo or HD, _at(ad, "ctx"), _at(ad, "dctx"), _at(ad, "rvec"), _at(ad, "ws"),
                                    r.B, r.n, r.heads, SCALE, stream)


def _ad_case(be, r):
    B, n, heads = r.B, r.n, r.heads
    HD = heads * 32
    tag = "linattn dcontext " + "-".join(map(str, r))
    g = torch.Generator().manual_seed(n + heads)
    q, do, ctx = torch.randn(B, n, HD, generator=g), torch.randn(B, n, HD, generator=g), torch.randn(B, heads, 32, 32, generator=g)
    qd, dod, ctxd = be.to(_pitched(q, r.ld or 3 * HD)), be.to(_pitched(do, r.lddo or HD)), be.to(ctx)     # (k | v of a (q|k|v) tensor are never read: NaN)
    dctx, rvec, ws = nan_empty(be, B, heads, 32, 32), nan_empty(be, B, HD), nan_empty(be, be.L.cdf_linattn_ws_floats(B, n, heads))
    name, args = ad_call(r, dict(q=P(qd), do=P(dod), ctx=P(ctxd), dctx=P(dctx), rvec=P(rvec), ws=P(ws)), be.stream())
    form = la_dcontext_form(*ad_call(r))
    assert la_dcontext_form(name, args) == form, tag
    print(f"{tag}: form {form}")
    dctxo, rveco = twice(lambda: getattr(be.L, name)(*args), [dctx, rvec])
    sc = torch.tensor(SCALE, dtype=torch.float32).double()
    qh, dh = q.double().view(B, n, heads, 32), do.double().view(B, n, heads, 32)
    dctx_r = torch.einsum("bnhd,bnhe->bhde", qh, dh) * sc
    # a sum over n of the terms q[n,d] dout[n,e] (sum_bound's K_SUM model, the terms' 2-norms without materialising them), scaled: one more rounding
    bd = SCALE * K_SUM * U * math.sqrt(n) * torch.einsum("bnhd,bnhe->bhde", qh ** 2, dh ** 2).sqrt().max().item() + U * _amax(dctx_r)
    _chk("dcontext", f"{tag} dctx", dctxo, dctx_r, bd)
    rt_ = dctx_r * ctx.double()
    # rvec: 32 terms dctx * ctx (K_SUM model), plus dctx's own error carried through |ctx| (bound of test_linattn_dctx_finish_production, with
    # the error of a summed dctx in place of one rounding)
    _chk("dcontext", f"{tag} rvec", rveco, rt_.sum(-1).reshape(B, HD), sum_bound(rt_, 3) + bd * math.sqrt(32) * ctx.double().pow(2).sum(-1).sqrt().max().item())
    return form


AD_ROWS = ([AD(2, n, ld, lddo) for n in (16, 144, 256, 300, 576) for ld, lddo in ((0, 0), (128, 0), (392, 136), (136, 136))]
           + [AD(1, 33 * 256 + 44), AD(2, 300, 0, 0, 2), AD(2, 300, 72, 72, 2)])


# ---------------------------------------------------------------------------------------------------------------------------------
# the k / v backward: cdf_linattn_bwd_kv, cdf_linattn_bwd_kv_planes
# ---------------------------------------------------------------------------------------------------------------------------------
class AB(NamedTuple):
    out: str           # 'f32', 'hl', 'h'
    B: int
    n: int
    layout: str = "kv"
    ld: int = 0
    ldo: int = 0
    dkoff: int = -1    # -1: the input's channel offset
    heads: int = 4
    big: bool = False


def ab_call(r, ad=None, stream=0):
    HD = r.heads * 32
    width = (3 if r.layout == "qkv" else 2) * HD
    koff = HD if r.layout == "qkv" else 0
    dkoff = koff if r.dkoff < 0 else r.dkoff
    ldo = r.ldo or dkoff + 2 * HD
    head = (_at(ad, "qkv"), r.ld or width, koff, _at(ad, "dctx"), _at(ad, "rvec"), _at(ad, "kmax"), _at(ad, "ksum"))
    if r.out == "f32":
        return "cdf_linattn_bwd_kv", head + (_at(ad, "out"), ldo, dkoff, r.B, r.n, r.heads, stream)
    return "cdf_linattn_bwd_kv_planes", head + (_at(ad, "hi"), _at(ad, "lo", r.out == "hl"), ldo, dkoff, r.B, r.n, r.heads, stream)


def _ab_case(be, r):
    skip_emu(be, r.big)
    B, n, heads = r.B, r.n, r.heads
    HD = heads * 32
    tag = "linattn bwd_kv " + "-".join(map(str, r))
    t, k, v, koff = _kv_inputs(B, n, heads, r.layout, r.ld, n * 5 + heads, corner=False)
    dkoff = koff if r.dkoff < 0 else r.dkoff
    ldo = r.ldo or dkoff + 2 * HD
    g = torch.Generator().manual_seed(n + 1)
    kmax = k.max(1).values
    ksum = torch.exp(k - kmax[:, None]).sum(1)
    dctx, ctx = torch.randn(B, heads, 32, 32, generator=g) * 0.3, torch.randn(B, heads, 32, 32, generator=g)
    rvec = (dctx * ctx).sum(-1).reshape(B, HD)
    td, dctxd, rvecd, kmd, ksd = be.to(t), be.to(dctx), be.to(rvec), be.to(kmax), be.to(ksum)

    def go(out):
        o, hi, lo = nan_empty(be, B, n, ldo), nan_empty(be, B, n, ldo, dtype=torch.int16), nan_empty(be, B, n, ldo, dtype=torch.int16)
        name, args = ab_call(r._replace(out=out), dict(qkv=P(td), dctx=P(dctxd), rvec=P(rvecd), kmax=P(kmd), ksum=P(ksd), out=P(o), hi=P(hi), lo=P(lo)), be.stream())
        assert la_bwd_kv_form(name, args) == la_bwd_kv_form(*ab_call(r._replace(out=out))), tag
        return twice(lambda: getattr(be.L, name)(*args), [o, hi, lo])
    form = la_bwd_kv_form(*ab_call(r))
    print(f"{tag}: form {form}")
    oo, hi0, lo0 = go("f32")
    kd, vd = k.double(), v.double()
    Pn = torch.exp(kd - kmax.double()[:, None]) / ksum.double()[:, None]
    Ph, vh, dc = Pn.view(B, n, heads, 32), vd.view(B, n, heads, 32), dctx.double()
    dP = torch.einsum("bnhe,bhde->bnhd", vh, dc)
    dk_ref = (Ph * (dP - rvec.double().view(B, 1, heads, 32))).reshape(B, n, HD)
    dv_ref = torch.einsum("bnhd,bhde->bnhe", Ph, dc).reshape(B, n, HD)
    sl = slice(dkoff, dkoff + 2 * HD)
    # (bound of test_kernels_production.py::test_linattn_bwd_kv_planes_production)
    _chk("bwd_kv", f"{tag} dk", oo[..., dkoff:dkoff + HD], dk_ref, 2e-5 * max(1.0, _amax(dk_ref)))
    _chk("bwd_kv", f"{tag} dv", oo[..., dkoff + HD:dkoff + 2 * HD], dv_ref, 2e-5 * max(1.0, _amax(dv_ref)))
    assert _poisoned(oo[..., :dkoff]) and _poisoned(oo[..., dkoff + 2 * HD:]) and _poisoned(hi0) and _poisoned(lo0), (tag, "a column outside dk | dv changed")
    if r.out != "f32":
        o2, hi, lo = go(r.out)
        rh, rl = _split(be, be.to(oo[..., sl].reshape(-1, 2 * HD)))
        assert torch.equal(hi[..., sl].reshape(-1, 2 * HD), rh.cpu()), (tag, "the hi plane is not cdf_split_bf16 of the fp32 result")
        assert torch.equal(lo[..., sl].reshape(-1, 2 * HD), rl.cpu()) if r.out == "hl" else _poisoned(lo), (tag, "the lo plane")
        assert _poisoned(o2) and _poisoned(hi[..., :dkoff]) and _poisoned(hi[..., dkoff + 2 * HD:]), (tag, "a column outside dk | dv changed")
        assert r.out == "h" or (_poisoned(lo[..., :dkoff]) and _poisoned(lo[..., dkoff + 2 * HD:])), (tag, "a column outside dk | dv changed (lo)")
    return form


def _ab_rows():
    rows = []
    for i, n in enumerate((16, 144, 256, 300, 576)):
        rows += [AB("f32", 2, n), AB("f32", 2, n, "qkv"), AB("f32", 2, n, "kv", 264, 264), AB("f32", 2, n, "qkv", 392, 392),
                 AB("hl", 2, n), AB("h", 2, n), AB(("hl", "h")[i % 2], 2, n, "kv", 264, 264), AB(("h", "hl")[i % 2], 2, n, "qkv", 392, 392)]
    rows += [AB("f32", 2, 300, "kv", 0, 392, 128), AB("hl", 2, 300, "qkv", 0, 264, 0), AB("f32", 1, 33 * 256 + 44, "kv", 264), AB("h", 1, 33 * 256 + 44, "kv", 0, 264),
             AB("f32", 2, 300, "kv", 0, 0, -1, 2), AB("hl", 2, 300, "qkv", 200, 200, -1, 2), AB("f32", 2, 300, "kv", 0, 0, -1, 1), AB("h", 2, 144, "qkv", 0, 0, -1, 3)]
    return rows


AB_ROWS = _ab_rows()


# ---------------------------------------------------------------------------------------------------------------------------------
# the fused k | v projection + context, and the fold of its partials
# ---------------------------------------------------------------------------------------------------------------------------------
class AK(NamedTuple):
    B: int
    n: int
    dim: int
    split: int = 3
    slots: int = 0
    ldx: int = 0
    ldk: int = 0       # 0: dim rounded up to 32 (cdf_pack_weight_bf16's pitch in the product)
    ldkv: int = 0
    big: bool = False


def ak_call(r, ad=None, stream=0):
    return "cdf_linattn_kvctx", (_at(ad, "xn"), r.ldx or r.dim, _at(ad, "whi"), _at(ad, "wlo", r.split == 3), r.ldk or cdiv(r.dim, 32) * 32, _at(ad, "kv"), r.ldkv or 256,
                                 _at(ad, "ws"), r.B, r.n, r.dim, 4, r.slots, stream)


def _ak_case(be, r):
    skip_emu(be, r.big)
    B, n, dim = r.B, r.n, r.dim
    heads, HD = 4, 128
    ldx, ldk, ldkv = r.ldx or dim, r.ldk or cdiv(dim, 32) * 32, r.ldkv or 256
    tag = "linattn kvctx " + "-".join(map(str, r))
    g = torch.Generator().manual_seed(n + dim)
    xn = torch.randn(B, n, dim, generator=g)
    w = torch.randn(2 * HD, dim, generator=g) / math.sqrt(dim)
    w[:HD] *= 3.0
    xn[..., 0] += torch.linspace(-6, 6, n)
    whi = torch.full((2 * HD, ldk), 0x7FC0, dtype=torch.int16, device=be.device)       # (pad columns of the weight planes: bf16 NaN)
    wlo = torch.full_like(whi, 0x7FC0) if r.split == 3 else None
    whc, wlc = torch.zeros(1, 2 * HD, dim, dtype=torch.int16, device=be.device), (torch.zeros(1, 2 * HD, dim, dtype=torch.int16, device=be.device) if r.split == 3 else None)
    assert dim % 8 == 0
    be.L.cdf_pack_weight_bf16(P(be.to(w)), P(whc), P(wlc), 1, 2 * HD, dim, dim, 1, dim, 1, be.stream())
    whi[:, :dim] = whc[0]
    if wlo is not None:
        wlo[:, :dim] = wlc[0]
    be._keep += [whi, wlo, whc, wlc]
    parts, tpb = kvctx_parts(B, n, r.slots)
    assert parts == be.L.cdf_linattn_kvctx_parts(B, n, r.slots)
    xd = be.to(_pitched(xn, ldx))
    kv, ws = nan_empty(be, B, n, ldkv), nan_empty(be, B * parts * (2 * HD + heads * 1024))
    ctx, ctxs, kmax, ksum = nan_empty(be, B, heads, 32, 32), nan_empty(be, B, heads, 32, 32), nan_empty(be, B, HD), nan_empty(be, B, HD)
    name, args = ak_call(r, dict(xn=P(xd), whi=P(whi), wlo=P(wlo), kv=P(kv), ws=P(ws)), be.stream())
    fname, fargs = "cdf_linattn_finalize", (P(ws), parts, P(ctx), P(ctxs), P(kmax), P(ksum), B, heads, SCALE, be.stream())
    form = la_kvctx_form(*ak_call(r))
    assert la_kvctx_form(name, args) == form, tag
    print(f"{tag}: form {form} ({parts} parts of {tpb} tiles), folded as {la_finalize_form(fname, fargs)}")

    def launch():
        getattr(be.L, name)(*args)
        getattr(be.L, fname)(*fargs)
    kvo, ctxo, ctxso, kmaxo, ksumo = twice(launch, [kv, ctx, ctxs, kmax, ksum, ws])[:5]
    kv_ref = xn.double() @ w.double().t()
    # (bounds of test_kernels_production.py::test_linattn_kvctx_production)
    _chk("kvctx", f"{tag} kv", kvo[..., :2 * HD], kv_ref, (3e-5 if r.split == 3 else 2e-2) * _amax(kv_ref))
    assert _poisoned(kvo[..., 2 * HD:]), (tag, "a pad column of kv changed")
    kmax_r, ksum_r, ctx_r = _ctx_ref(kvo[..., :HD], kvo[..., HD:2 * HD], heads)          # (the context of the kv written)
    _ctx_checks("kvctx", tag, ctxo, ctxso, kmaxo, ksumo, kmax_r, ksum_r, ctx_r)
    return form


def ak_finalize_form(r):
    return la_finalize_form("cdf_linattn_finalize", (1, kvctx_parts(r.B, r.n, r.slots)[0], 1, 1, 1, 1, r.B, 4, SCALE, 0))


AK_ROWS = [AK(2, 384, 64), AK(2, 384, 64, 1), AK(2, 384, 96, 3, 0, 104, 128, 264), AK(2, 384, 96, 1), AK(2, 384, 128, 3, 0, 136, 136), AK(2, 384, 128, 1, 0, 0, 0, 264),
           AK(2, 640, 64, 3, 2), AK(1, 640, 96, 1, 2, 104), AK(2, 512, 128, 3, 2),                    # P = 1 with several tiles; 2 parts of 3 + 2 tiles
           AK(1, 34 * 128, 64, 3, 64), AK(1, 34 * 128, 96, 1, 64, 0, 0, 264)]     # P = tiles = 34 > 32


class AF(NamedTuple):
    nparts: int
    B: int = 2
    heads: int = 4


def af_call(r, ad=None, stream=0):
    return "cdf_linattn_finalize", (_at(ad, "ws"), r.nparts, _at(ad, "ctx"), _at(ad, "ctxs"), _at(ad, "kmax"), _at(ad, "ksum"), r.B, r.heads, SCALE, stream)


def _af_case(be, r):
    """Synthetic partials (max | ctx | sum, the workspace layout): column maxima up to 12 apart, so the rescaling weights span e^-12 .. 1."""
    nparts, B, heads = r
    HD = heads * 32
    tag = "linattn finalize " + "-".join(map(str, r))
    g = torch.Generator().manual_seed(nparts + heads)
    mx = torch.randn(B, nparts, HD, generator=g) * 3
    sm = torch.rand(B, nparts, HD, generator=g) * 200 + 1
    cp = torch.randn(B, nparts, heads, 32, 32, generator=g) * sm.view(B, nparts, heads, 32, 1) / 16
    wsd = be.to(torch.cat([mx.reshape(-1), cp.reshape(-1), sm.reshape(-1)]))
    ctx, ctxs, kmax, ksum = nan_empty(be, B, heads, 32, 32), nan_empty(be, B, heads, 32, 32), nan_empty(be, B, HD), nan_empty(be, B, HD)
    name, args = af_call(r, dict(ws=P(wsd), ctx=P(ctx), ctxs=P(ctxs), kmax=P(kmax), ksum=P(ksum)), be.stream())
    form = la_finalize_form(*af_call(r))
    assert la_finalize_form(name, args) == form, tag
    print(f"{tag}: form {form}")
    ctxo, ctxso, kmaxo, ksumo = twice(lambda: getattr(be.L, name)(*args), [ctx, ctxs, kmax, ksum])
    kmax_r = mx.double().max(1).values
    wgt = torch.exp(mx.double() - kmax_r[:, None])
    ksum_r = (wgt * sm.double()).sum(1)
    ctx_r = (wgt.view(B, nparts, heads, 32, 1) * cp.double()).sum(1) / ksum_r.view(B, heads, 32, 1)
    _ctx_checks("finalize", tag, ctxo, ctxso, kmaxo, ksumo, kmax_r, ksum_r, ctx_r)
    return form


AF_ROWS = [AF(1), AF(8), AF(33), AF(3), AF(32), AF(70), AF(33, 3, 2), AF(7, 1, 1)]


class AX(NamedTuple):
    rows: int


def ax_call(r, ad=None, stream=0):
    return "cdf_linattn_dctx_finish", (_at(ad, "raw"), _at(ad, "ctx"), _at(ad, "dctx"), _at(ad, "rvec"), r.rows, SCALE, stream)


def _ax_case(be, r):
    rows = r.rows
    tag = f"linattn dctx_finish {rows}"
    g = torch.Generator().manual_seed(rows)
    raw, ctx = torch.randn(rows, 32, generator=g) * 3, torch.randn(rows, 32, generator=g)
    rawd, ctxd = be.to(raw), be.to(ctx)
    dctx, rvec = nan_empty(be, rows, 32), nan_empty(be, rows)
    name, args = ax_call(r, dict(raw=P(rawd), ctx=P(ctxd), dctx=P(dctx), rvec=P(rvec)), be.stream())
    form = la_dctx_finish_form(*ax_call(r))
    assert la_dctx_finish_form(name, args) == form, tag
    print(f"{tag}: form {form}")
    dctxo, rveco = twice(lambda: getattr(be.L, name)(*args), [dctx, rvec])
    sc = torch.tensor(SCALE, dtype=torch.float32).double()
    dctx_r = raw.double() * sc
    terms = dctx_r * ctx.double()                            # (bounds of test_kernels_production.py::test_linattn_dctx_finish_production)
    _chk("dctx_finish", f"{tag} dctx", dctxo, dctx_r, U * _amax(dctx_r))
    _chk("dctx_finish", f"{tag} rvec", rveco, terms.sum(1), sum_bound(terms, 1) + U * math.sqrt(32) * (dctx_r.abs() * ctx.double().abs()).pow(2).sum(1).sqrt().max().item())
    return form


AX_ROWS = [AX(1), AX(8), AX(13), AX(256), AX(261), AX(64 * 4 * 32 + 5)]


# ---------------------------------------------------------------------------------------------------------------------------------
# the unfused k backward (cdf_linattn_softk, cdf_linattn_dk) and the row softmax of the attention block
# ---------------------------------------------------------------------------------------------------------------------------------
class AS(NamedTuple):
    B: int
    n: int
    ld: int = 0
    ldp: int = 0
    heads: int = 4
    big: bool = False


def as_call(r, ad=None, stream=0):
    HD = r.heads * 32
    return "cdf_linattn_softk", (_at(ad, "qkv"), r.ld or 3 * HD, _at(ad, "kmax"), _at(ad, "ksum"), _at(ad, "pn"), r.ldp or HD, r.B, r.n, r.heads, stream)


def ak2_call(r, ad=None, stream=0):
    """cdf_linattn_dk of the same row: pn with the row's ldp, dp and dk with the pitch ld (the (q|k|v) gradient tensor in the product)."""
    HD = r.heads * 32
    return "cdf_linattn_dk", (_at(ad, "pn"), r.ldp or HD, _at(ad, "dp"), r.ldp or HD, _at(ad, "rvec"), _at(ad, "dk"), r.ld or 3 * HD, r.B, r.n, r.heads, stream)


def _as_case(be, r):
    skip_emu(be, r.big)
    B, n, heads = r.B, r.n, r.heads
    HD = heads * 32
    ld, ldp = r.ld or 3 * HD, r.ldp or HD
    tag = "linattn softk / dk " + "-".join(map(str, r))
    t, k, _, _ = _kv_inputs(B, n, heads, "qkv", ld, n + 7, corner=not r.big)
    g = torch.Generator().manual_seed(n)
    kmax = k.max(1).values
    ksum = torch.exp(k - kmax[:, None]).sum(1)
    dp, rvec = torch.randn(B, n, HD, generator=g), torch.randn(B, HD, generator=g)
    td, kmd, ksd, dpd, rvd = be.to(t), be.to(kmax), be.to(ksum), be.to(_pitched(dp, ldp)), be.to(rvec)
    pn, dk = nan_empty(be, B, n, ldp), nan_empty(be, B, n, ld)
    ad = dict(qkv=P(td), kmax=P(kmd), ksum=P(ksd), pn=P(pn), dp=P(dpd), rvec=P(rvd), dk=P(dk) + 4 * HD)     # dk: the k columns of a (q|k|v) gradient
    name, args = as_call(r, ad, be.stream())
    dname, dargs = ak2_call(r, ad, be.stream())
    form = la_softk_form(*as_call(r))
    assert la_softk_form(name, args) == form and la_dk_form(dname, dargs) == la_dk_form(*ak2_call(r)), tag
    print(f"{tag}: forms {form}, {la_dk_form(dname, dargs)}")

    def launch():
        getattr(be.L, name)(*args)
        getattr(be.L, dname)(*dargs)
    pno, dko = twice(launch, [pn, dk])
    pn_r = torch.exp(k.double() - kmax.double()[:, None]) / ksum.double()[:, None]
    # P <= 1 is expf of an exact difference divided once: a few roundings of a value <= 1 -- the absolute 1e-6 of test_kernels.py's row softmax
    _chk("softk", f"{tag} pn", pno[..., :HD], pn_r, 1e-6)
    assert _poisoned(pno[..., HD:]), (tag, "a pad column of pn changed")
    # dk = P (dP - r) from the P the kernel wrote: one subtraction and one product, each rounded once
    dk_r = pno[..., :HD].double() * (dp.double() - rvec.double()[:, None])
    _chk("dk", f"{tag} dk", dko[..., HD:2 * HD], dk_r, 2 * U * max(1e-30, (pno[..., :HD].double().abs() * (dp.double().abs() + rvec.double().abs()[:, None])).max().item()))
    assert _poisoned(dko[..., :HD]) and _poisoned(dko[..., 2 * HD:]), (tag, "a column of the gradient tensor outside dk changed")
    return form


AS_ROWS = [AS(2, 16), AS(2, 144, 392, 136), AS(2, 300), AS(2, 300, 0, 136), AS(2, 300, 392), AS(2, 300, 200, 72, 2), AS(17, 128 * 128 // 4 - 3, big=True)]


class SR(NamedTuple):
    rows: int
    n: int
    ld: int = 0


def sr_call(r, ad=None, stream=0, bwd=False):
    scale = 128 ** -0.5
    if bwd:
        return "cdf_softmax_rows_bwd", (_at(ad, "p"), _at(ad, "dp"), _at(ad, "ds"), r.rows, r.n, r.ld or r.n, scale, stream)
    return "cdf_softmax_rows_fwd", (_at(ad, "s"), _at(ad, "p"), r.rows, r.n, r.ld or r.n, scale, stream)


def _sr_case(be, r):
    rows, n = r.rows, r.n
    ld = r.ld or n
    tag = "softmax rows " + "-".join(map(str, r))
    g = torch.Generator().manual_seed(rows + n)
    s, dp = torch.randn(rows, n, generator=g) * 4, torch.randn(rows, n, generator=g)
    s[0] = 1.5                                               # a constant row: p = 1 / n
    s[rows - 1, n - 1] += 60                                 # a row whose maximum is its last element, 60 above the rest
    sd, dpd = be.to(_pitched(s, ld)), be.to(_pitched(dp, ld))
    p, ds = nan_empty(be, rows, ld), nan_empty(be, rows, ld)
    ad = dict(s=P(sd), p=P(p), dp=P(dpd), ds=P(ds))
    name, args = sr_call(r, ad, be.stream())
    bname, bargs = sr_call(r, ad, be.stream(), True)
    form = softmax_rows_form(*sr_call(r))
    assert softmax_rows_form(name, args) == form and softmax_rows_form(bname, bargs) == softmax_rows_form(*sr_call(r, bwd=True)), tag
    print(f"{tag}: forms {form}, {softmax_rows_form(bname, bargs)}")

    def launch():
        getattr(be.L, name)(*args)
        getattr(be.L, bname)(*bargs)
    po, dso = twice(launch, [p, ds])
    sc = torch.tensor(128 ** -0.5, dtype=torch.float32).double()
    p_r = (s.double() * sc).softmax(1)
    _chk("softmax rows", f"{tag} p", po[:, :n], p_r, 1e-6)   # (the absolute bounds of test_kernels.py's row softmax)
    pk = po[:, :n].double()                                  # the gradient through the p the kernel wrote
    ds_r = sc * pk * (dp.double() - (pk * dp.double()).sum(1, keepdim=True))
    _chk("softmax rows", f"{tag} ds", dso[:, :n], ds_r, 1e-6)
    assert _poisoned(po[:, n:]) and _poisoned(dso[:, n:]), (tag, "a pad column changed")
    assert (po[0, :n] - 1.0 / n).abs().max().item() <= 2 * U, (tag, "the constant row")
    return form


SR_ROWS = [SR(150, 16), SR(150, 16, 24), SR(37, 64), SR(37, 64, 72), SR(150, 50, 52), SR(37, 65), SR(9, 144, 152), SR(5, 300), SR(16384 + 5, 70, 72)]


# ---------------------------------------------------------------------------------------------------------------------------------
# the tested forms; the forms the recordings reach
# ---------------------------------------------------------------------------------------------------------------------------------
CLASSIFIERS = {            # what -> (entry points, form function, rows, the row's (name, stand-in arguments))
    "la_context": (("cdf_linattn_context",), la_context_form, lambda: AC_ROWS, ac_call),
    "la_dcontext": (("cdf_linattn_dcontext",), la_dcontext_form, lambda: AD_ROWS, ad_call),
    "la_bwd_kv": (("cdf_linattn_bwd_kv", "cdf_linattn_bwd_kv_planes"), la_bwd_kv_form, lambda: AB_ROWS, ab_call),
    "la_kvctx": (("cdf_linattn_kvctx",), la_kvctx_form, lambda: AK_ROWS, ak_call),
    "la_finalize": (("cdf_linattn_finalize",), la_finalize_form, lambda: AF_ROWS, af_call),
    "la_dctx_finish": (("cdf_linattn_dctx_finish",), la_dctx_finish_form, lambda: AX_ROWS, ax_call),
    "la_softk": (("cdf_linattn_softk",), la_softk_form, lambda: AS_ROWS, as_call),
    "la_dk": (("cdf_linattn_dk",), la_dk_form, lambda: AS_ROWS, ak2_call),
    "softmax_rows": (("cdf_softmax_rows_fwd", "cdf_softmax_rows_bwd"), softmax_rows_form, lambda: SR_ROWS, sr_call),
}
ALL_NAMES = tuple(n for names, *_ in CLASSIFIERS.values() for n in names)
assert set(ALL_NAMES) == set(LA_NAMES)


def forms_of_rows(what):
    _, form, rows, call = CLASSIFIERS[what]
    out = {form(*call(r)) for r in rows()}
    if what == "la_finalize":                                # a kvctx row folds its partials with the finalize kernel as well
        out |= {ak_finalize_form(r) for r in AK_ROWS}
    if what == "softmax_rows":
        out |= {form(*call(r, bwd=True)) for r in rows()}
    return out


def reached_forms(calls):
    """{what: {form: (recording, name)}} of recorded (recording, name, arguments) calls."""
    out = {what: {} for what in CLASSIFIERS}
    for src, name, a in calls:
        for what, (names, form, _, _) in CLASSIFIERS.items():
            if name in names:
                out[what].setdefault(form(name, a), (src, name))
    return out


# The forms the recordings of test_gpu_invariance.py::test_coverage_guard reach (one bench step in bf16x3 and in bf16, one sampler step at
# B = 16, one forward + backward pass of config 2's network).  The guard fails when a recording reaches a form no row has, and when a form
# listed here is no longer reached.  Every other tested form is one no recording reaches.
REACHED = {
    "la_context": {
        ('qkv', 4, 0, 1, '1', 0),
        ('qkv', 4, 0, 1, 'several', 0),
    },
    "la_dcontext": {
        (4, '3hd', 0, '1', 0),
        (4, '3hd', 0, 'several', 0),
    },
    "la_bwd_kv": {
        ('f32', 'qkv', 4, '', 1, '1', 0, 0),
        ('f32', 'qkv', 4, '', 1, 'several', 0, 0),
        ('h', 'kv', 4, '', 1, '>32', 0, 0),
        ('h', 'kv', 4, '', 1, 'several', 0, 0),
        ('hl', 'kv', 4, '', 1, '>32', 0, 0),
        ('hl', 'kv', 4, '', 1, 'several', 0, 0),
    },
    "la_kvctx": {
        (0, 64, '1', '', 'several', '1', 0),
        (0, 64, '1', '', 'several', 'several', 0),
        (0, 64, 'several', '', 'several', '1', 0),
        (0, 64, 'several', '', 'several', 'several', 0),
        (1, 64, '1', '', 'several', 'several', 0),
        (1, 64, 'several', '', 'several', '1', 0),
        (1, 64, 'several', '', 'several', 'several', 0),
    },
    "la_finalize": {
        (4, 'several', 0),
    },
    "la_dctx_finish": {
        ('>32', 0),
    },
    "la_softk": set(),                                       # (the unfused k backward is a switch of the Python layer, off in every recording)
    "la_dk": set(),
    "softmax_rows": {
        ('bwd', '<=64', 1, 0, 0),
        ('bwd', '>64', 0, 0, 1),
        ('fwd', '<=64', 1, 0, 0),
        ('fwd', '>64', 0, 0, 1),
    },
}
# ... and the forms that one forward + backward pass of two small networks (test_recorded_attn_forms_dry; bf16x3, bf16 and f32) reaches
# besides: the small Unet's attention runs on a (k|v) tensor at n = 2304 / 576 / 144
SMALL_NETWORKS = {
    "la_context": {
        ('kv', 4, 0, 1, '1', 1),
        ('kv', 4, 0, 1, 'several', 0),
        ('kv', 4, 0, 1, 'several', 1),
    },
    "la_dcontext": set(),
    "la_bwd_kv": {
        ('f32', 'kv', 4, '', 1, '1', 1, 1),
        ('f32', 'kv', 4, '', 1, 'several', 0, 0),
        ('f32', 'kv', 4, '', 1, 'several', 1, 0),
        ('h', 'kv', 4, '', 1, 'several', 1, 0),
        ('hl', 'kv', 4, '', 1, 'several', 1, 0),
    },
    "la_kvctx": set(),
    "la_finalize": set(),
    "la_dctx_finish": {
        ('several', 0),
    },
    "la_softk": set(),
    "la_dk": set(),
    "softmax_rows": {
        ('bwd', '<=64', 0, 0, 0),
        ('fwd', '<=64', 0, 0, 0),
    },
}


# ... with a row for each of them: the smallest shape of the form, built from the form itself (each builder is the inverse of its
# classifier; the assertion below holds it to that)
_N_OF = {("1", 0): 256, ("1", 1): 144, ("several", 0): 512, ("several", 1): 576, (">32", 0): 33 * 256, (">32", 1): 33 * 256 + 44}


def _ac_row_of(f):
    layout, heads, pitched, onepass, count, ragged = f
    width = (3 if layout == "qkv" else 2) * heads * 32
    return AC(1 if count == ">32" else 2, _N_OF[(count, ragged)], layout, width + 8 if pitched else 0, onepass, heads)


def _ad_row_of(f):
    heads, ldc, dop, count, ragged = f
    HD = heads * 32
    return AD(1 if count == ">32" else 2, _N_OF[(count, ragged)], {"hd": HD, "3hd": 0, "other": 3 * HD + 8}[ldc], HD + 8 if dop else 0, heads)


def _ab_row_of(f):
    out, layout, heads, pit, same, count, r256, r32 = f
    HD = heads * 32
    n = {("1", 0, 0): 256, ("1", 1, 0): 160, ("1", 1, 1): 144, ("several", 0, 0): 512, ("several", 1, 0): 576, ("several", 1, 1): 300,
         (">32", 0, 0): 33 * 256, (">32", 1, 0): 33 * 256 + 32, (">32", 1, 1): 33 * 256 + 44}[(count, r256, r32)]
    koff = HD if layout == "qkv" else 0
    dkoff = koff if same else koff + 8
    return AB(out, 1 if count == ">32" else 2, n, layout, koff + 2 * HD + 8 if "i" in pit else 0, dkoff + 2 * HD + 8 if "o" in pit else 0, -1 if same else dkoff, heads)


def _ak_row_of(f):
    lo_null, bk, chunks, pit, parts, tpb, short = f
    dim = bk if chunks == "1" else (128 if bk == 64 else 96)
    B, n, slots = {("1", "1", 0): (2, 128, 0), ("1", "several", 0): (2, 512, 2), ("several", "1", 0): (2, 384, 0), ("several", "several", 0): (2, 512, 4),
                   ("several", "several", 1): (2, 640, 4), (">32", "1", 0): (1, 34 * 128, 64)}[(parts, tpb, short)]
    return AK(B, n, dim, 1 if lo_null else 3, slots, dim + 8 if "x" in pit else 0, dim + 8 if "w" in pit else 0, 264 if "k" in pit else 0)


def _af_row_of(f):
    heads, count, mod4 = f
    return AF({("1", 1): 1, ("several", 0): 8, ("several", 1): 7, (">32", 0): 36, (">32", 1): 33}[(count, mod4)], 2, heads)


def _ax_row_of(f):
    return AX({("1", 0): 8, ("1", 1): 5, ("several", 0): 64, ("several", 1): 61, (">32", 0): 8192, (">32", 1): 8197}[f])


def _sr_row_of(f):
    _, ncls, mod, pitched, capped = f
    n = {("<=64", 0): 64, ("<=64", 1): 16, (">64", 0): 128, (">64", 1): 70}[(ncls, mod)]
    return SR(16384 + 5 if capped else 37, n, n + 8 if pitched else 0)


for _what, _rows, _of in (("la_context", AC_ROWS, _ac_row_of), ("la_dcontext", AD_ROWS, _ad_row_of), ("la_bwd_kv", AB_ROWS, _ab_row_of), ("la_kvctx", AK_ROWS, _ak_row_of),
                          ("la_finalize", AF_ROWS, _af_row_of), ("la_dctx_finish", AX_ROWS, _ax_row_of), ("softmax_rows", SR_ROWS, _sr_row_of)):
    for _f in sorted(REACHED[_what] | SMALL_NETWORKS[_what], key=repr):
        if _f not in forms_of_rows(_what):
            _rows.append(_of(_f))
            assert _f in forms_of_rows(_what), (_what, _f, _rows[-1])


def test_form_tables():
    """The tables keep what they were built for, and the forms flagged as reached are tested forms."""
    for what in CLASSIFIERS:
        t = forms_of_rows(what)
        assert REACHED[what] | SMALL_NETWORKS[what] <= t, (what, sorted((REACHED[what] | SMALL_NETWORKS[what]) - t, key=repr))
        assert t - REACHED[what], what
    for rows in (AC_ROWS, AD_ROWS, AB_ROWS):
        assert {r.n for r in rows} >= {16, 144, 256, 300, 576}
    ac = forms_of_rows("la_context")
    assert {f[0] for f in ac} == {"qkv", "kv"} and {f[2:4] for f in ac} == {(0, 0), (0, 1), (1, 0), (1, 1)} and {f[4:] for f in ac} >= {("1", 0), ("1", 1), ("several", 1), (">32", 1)}
    ab = forms_of_rows("la_bwd_kv")
    assert {f[:2] for f in ab} == {(o, l) for o in ("f32", "hl", "h") for l in ("kv", "qkv")} and {f[3] for f in ab} >= {"", "io", "o"} and {f[4] for f in ab} == {0, 1}
    assert {f[2] for f in ab} == {1, 2, 3, 4} and {f[5:] for f in ab} >= {("1", 0, 0), ("1", 1, 1), ("several", 1, 0), ("several", 1, 1), (">32", 1, 1)}
    ak = forms_of_rows("la_kvctx")
    assert {f[:3] for f in ak} == {(l, 64, c) for l in (0, 1) for c in ("1", "several")} | {(0, 32, "several"), (1, 32, "several")}
    assert {f[4:6] for f in ak} == {("1", "several"), ("several", "1"), ("several", "several"), (">32", "1")} and any(f[6] for f in ak) and any(f[3] == "xwk" for f in ak)
    assert {r.dim for r in AK_ROWS} >= {64, 96, 128}
    af = forms_of_rows("la_finalize")
    assert {f[1] for f in af} == {"1", "several", ">32"} and {r.nparts for r in AF_ROWS} >= {1, 8, 33}
    sr = forms_of_rows("softmax_rows")
    assert {f[:2] for f in sr} == {(d, c) for d in ("fwd", "bwd") for c in ("<=64", ">64")} and {f[3] for f in sr} == {0, 1} and {f[4] for f in sr} == {0, 1}


def test_recorded_attn_forms_dry(monkeypatch):
    """test_side_kernel_forms.py::test_recorded_side_forms_dry for the attention entry points."""
    import sys
    from test_side_kernel_forms import dry_recordings, hold_recordings
    hold_recordings(sys.modules[__name__], *dry_recordings(monkeypatch, ALL_NAMES))


# ---------------------------------------------------------------------------------------------------------------------------------
# the tests over the case tables (both backends)
# ---------------------------------------------------------------------------------------------------------------------------------
_ids = lambda r: "-".join(map(str, r))


@pytest.mark.parametrize("r", AC_ROWS, ids=_ids)
def test_linattn_context_forms(be, r):
    _ac_case(be, r)


@pytest.mark.parametrize("r", AD_ROWS, ids=_ids)
def test_linattn_dcontext_forms(be, r):
    _ad_case(be, r)


@pytest.mark.parametrize("r", AB_ROWS, ids=_ids)
def test_linattn_bwd_kv_forms(be, r):
    _ab_case(be, r)


@pytest.mark.parametrize("r", AK_ROWS, ids=_ids)
def test_linattn_kvctx_forms(be, r):
    _ak_case(be, r)


@pytest.mark.parametrize("r", AF_ROWS, ids=_ids)
def test_linattn_finalize_forms(be, r):
    _af_case(be, r)


@pytest.mark.parametrize("r", AX_ROWS, ids=_ids)
def test_linattn_dctx_finish_forms(be, r):
    _ax_case(be, r)


@pytest.mark.parametrize("r", AS_ROWS, ids=_ids)
def test_linattn_softk_dk_forms(be, r):
    _as_case(be, r)


@pytest.mark.parametrize("r", SR_ROWS, ids=_ids)
def test_softmax_rows_forms(be, r):
    _sr_case(be, r)
