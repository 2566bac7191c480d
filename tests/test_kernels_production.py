"""Kernel-level tests at the shapes production launches -- where the chunk / split / block clamps take effect and the kernels switch
to grid-stride or multi-row-chunk walks that the small-shape tests in test_kernels.py never reach.  Each test:
  * computes its reference in float64 on the CPU from the same inputs;
  * poisons every output and workspace with NaN before each launch (tests/poison.py);
  * launches twice and asserts the two results are bit-identical;
  * bounds the error by a model stated with it and prints the worst error / bound.

Error model of an fp32 sum of n terms t_i (any fixed summation order, zero-mean data): the rounding errors of the partial sums walk
randomly, each at most 2^-24 of a partial sum of typical size ||t||_2, so |err| <~ 2^-24 sqrt(n) ||t||_2.  Bounds below are
K_SUM = 4 times that (the existing small-shape tests of the same kernels correspond to K >= 4.8: e.g. test_colsum's 2e-4 over 700
randn rows), and never looser than the existing test's tolerance where that is absolute.
Per-image references that would take > ~20 s at B = 64 compare a fixed sample of images (first, middle, last); reductions over the
batch are compared in full.  Shapes an emulator run can afford run on both backends; the rest are gpu-only.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from poison import nan_empty, poison_, poisoned_allocations
from test_kernels import P, _split, nhwc, r4

U = 2.0 ** -24
K_SUM = 4.0


def sum_bound(terms, dim):
    """K_SUM * 2^-24 * sqrt(n) * max over outputs of ||t||_2 for sums of `terms` (float64) over `dim`."""
    n = 1
    for d in (dim if isinstance(dim, tuple) else (dim,)):
        n *= terms.shape[d]
    return K_SUM * U * math.sqrt(n) * terms.pow(2).sum(dim).sqrt().max().item()


def check(name, got, ref, bound):
    e = (got.detach().cpu().double() - ref.double()).abs().max().item()
    print(f"{name}: worst error {e:.3e} / bound {bound:.3e} = {e / bound:.3f}")
    assert math.isfinite(e) and e <= bound, (name, e, bound)


def twice(launch, outs):
    """Poison outs, launch, keep; poison again, launch: both results bit for bit the same.  Returns the results (on the host)."""
    res = []
    for _ in range(2):
        for o in outs:
            poison_(o)
        launch()
        if torch.cuda.is_available() and outs[0].is_cuda:
            torch.cuda.synchronize()
        res.append([o.detach().cpu().clone() for o in outs])
    for i, (a, b) in enumerate(zip(*res)):
        assert bits_equal(a, b), ("second launch differs", i)
    return res[0]


def bits_equal(a, b):
    """torch.equal on the bit patterns (a NaN the kernel left in a pad column equals itself)."""
    if a.dtype.is_floating_point:
        as_int = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
        a, b = a.view(as_int), b.view(as_int)
    return torch.equal(a, b)


def skip_emu(be, big):
    if big and be.kind == "emu":
        pytest.skip("production shape: too slow for the simulator (runs on the MI355X)")


def sample(B):
    return sorted({0, B // 2, B - 1})


# ---------------------------------------------------------------------------------------------------------------------------------
# column sums: chunk count capped at 1024
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nseg,rows,C,big", [(2, 512 * 1024 + 37, 4, False),       # just past the cap: 1024 chunks of cdiv(rows, 1024) = 513
                                              #   rows -- 1022 full ones, one of 39 rows and an EMPTY last chunk, whose partial sums
                                              #   must still be written (zeros: the poisoned workspace shows NaN otherwise)
                                              (64, 16384, 64, True),               # per-image time-bias gradients, 128 x 128, B = 64
                                              (1, 1048576, 64, True)])             # the whole 64-image batch as one segment
def test_colsum_past_chunk_cap(be, nseg, rows, C, big):
    skip_emu(be, big)
    torch.manual_seed(rows % 1000)
    assert be.L.cdf_colsum_nchunk(rows) == min(1024, max(1, rows // 512))
    ld = C + 4                                                   # a pitched input: the pad columns hold garbage the sums must skip
    x = torch.randn(nseg, rows, ld)
    x[..., C:] = float("nan")
    ref = x[..., :C].double().sum(1)
    bound = sum_bound(x[..., :C].double(), 1)
    nch = be.L.cdf_colsum_nchunk(rows)
    xd = be.to(x)
    ws, out = nan_empty(be, nseg * nch * C), nan_empty(be, nseg, C + 4)
    got = twice(lambda: be.L.cdf_colsum(P(xd), P(out), P(ws), nseg, rows, C, ld, C + 4, 0, be.stream()), [out, ws])[0]
    check(f"cdf_colsum {nseg}x{rows}x{C}", got[:, :C], ref, bound)
    xb = x.bfloat16()
    xbd = be.to(xb.view(torch.int16))
    got = twice(lambda: be.L.cdf_colsum_io(P(xbd), P(out), P(ws), nseg, rows, C, ld, C + 4, 0, 1, be.stream()), [out, ws])[0]
    check(f"cdf_colsum_io {nseg}x{rows}x{C}", got[:, :C], xb[..., :C].double().sum(1), bound)


# ---------------------------------------------------------------------------------------------------------------------------------
# channel LayerNorm: the 1024-block cap, C = 64 / 128 at M = 1,048,576, C = 512 / 1024 at 16 x 16, B = 64
# ---------------------------------------------------------------------------------------------------------------------------------
def _ln_ref(x, g, b, dy, eps=1e-5):
    x, g, b, dy = x.double(), g.double(), b.double(), dy.double()
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    rstd = (var + eps).rsqrt()
    xh = (x - mean) * rstd
    y = xh * g + b
    dxh = dy * g
    dx = rstd * (dxh - dxh.mean(1, keepdim=True) - xh * (dxh * xh).mean(1, keepdim=True))
    return y, mean[:, 0], rstd[:, 0], dx, dy * xh, dy


def _ln_rows_at_cap(be, C):
    """The smallest M with cdf_layernorm_blocks(M, C) == 1024."""
    lo, hi = 1, 1 << 22
    while lo < hi:
        mid = (lo + hi) // 2
        if be.L.cdf_layernorm_blocks(mid, C) >= 1024:
            hi = mid
        else:
            lo = mid + 1
    return lo


@pytest.mark.parametrize("C,M,big", [(8, "cap-1", False), (8, "cap+37", False), (64, 1048576, True), (128, 1048576, True),
                                     (512, 16384, True), (1024, 16384, True), (64, "4cap+37", True)])
def test_layernorm_production(be, C, M, big):
    skip_emu(be, big)
    if isinstance(M, str):
        cap = _ln_rows_at_cap(be, C)
        M = {"cap-1": cap - 1, "cap+37": cap + 37, "4cap+37": 4 * cap + 37}[M]
    torch.manual_seed(C)
    x, g, b, dy = torch.randn(M, C), torch.randn(C), torch.randn(C), torch.randn(M, C)
    y_r, mean_r, rstd_r, dx_r, dg_terms, db_terms = _ln_ref(x, g, b, dy)
    xd, gd, bd, dyd = be.to(x), be.to(g), be.to(b), be.to(dy)
    # forward: elementwise after two sums over C -> a few ulps of |y|, bounded by the existing test's 5e-6 where that is tighter
    y, mo, ro = nan_empty(be, M, C), nan_empty(be, M), nan_empty(be, M)
    yo, mo_, ro_ = twice(lambda: be.L.cdf_layernorm_c_fwd(P(xd), C, P(y), C, P(gd), P(bd), P(mo), P(ro), M, C, 1e-5, 0, 0, 0, be.stream()),
                         [y, mo, ro])
    yscale = y_r.abs().max().item()
    check(f"layernorm fwd M={M} C={C}", yo, y_r, min(5e-6, K_SUM * U * math.sqrt(C) * yscale * 4))
    nb = be.L.cdf_layernorm_blocks(M, C)
    part, dx, dg, db = nan_empty(be, nb * 2 * C), nan_empty(be, M, C), nan_empty(be, C), nan_empty(be, C)
    dxo, dgo, dbo = twice(lambda: be.L.cdf_layernorm_c_bwd(P(dyd), C, P(xd), C, P(gd), P(mo), P(ro), P(dx), C, 0, 0, P(dg), P(db), P(part), M, C,
                                                           0, 0, be.stream()), [dx, dg, db, part])[:3]
    check(f"layernorm bwd dx M={M} C={C}", dxo, dx_r, 1e-5)
    # dg / db: sums over M rows (the existing 2e-5 over 37 rows is K ~ 9 of the same model)
    check(f"layernorm bwd dg M={M} C={C}", dgo, dg_terms.sum(0), sum_bound(dg_terms, 0))
    check(f"layernorm bwd db M={M} C={C}", dbo, db_terms.sum(0), sum_bound(db_terms, 0))
    if C % 8 == 0:
        # the planes form: the same dx, planes = cdf_split_bf16 of it, bit for bit
        ph, pl = nan_empty(be, M, C, dtype=torch.int16), nan_empty(be, M, C, dtype=torch.int16)
        dx2 = nan_empty(be, M, C)
        r = twice(lambda: be.L.cdf_layernorm_c_bwd_planes(P(dyd), C, P(xd), C, P(gd), P(mo), P(ro), P(dx2), C, 0, 0, P(dg), P(db), P(part), M, C,
                                                          0, 0, P(ph), P(pl), C, be.stream()), [dx2, ph, pl, dg, db, part])
        assert torch.equal(r[0], dxo) and torch.equal(r[3], dgo) and torch.equal(r[4], dbo)
        rh, rl = _split(be, be.to(r[0]))
        assert torch.equal(r[1], rh.cpu()) and torch.equal(r[2], rl.cpu())
        _layernorm_io(be, x, g, b, dy, M, C)


def _layernorm_io(be, x, g, b, dy, M, C):
    """The bf16 activation-storage forms (cdf_layernorm_c_fwd_io / _bwd_io) at the same shape: exactly the fp32 kernel on the widened
    values, the bf16 outputs rounded once (test_bf16_storage's contract), and the fp32 outputs within the fp64 bounds above."""
    xb, dyb = x.bfloat16(), dy.bfloat16()
    xbd, xfd, gd, bd = be.to(xb.view(torch.int16)), be.to(xb.float()), be.to(g), be.to(b)
    dybd, dyfd, dyd = be.to(dyb.view(torch.int16)), be.to(dyb.float()), be.to(dy)
    y_r, _, _, dx_r, _, _ = _ln_ref(xb.float(), g, b, dyb.float())
    y, mo, ro, yf, mf, rf = (nan_empty(be, *s) for s in ((M, C), (M,), (M,), (M, C), (M,), (M,)))
    yo, moo, roo = twice(lambda: be.L.cdf_layernorm_c_fwd_io(P(xbd), C, P(y), C, P(gd), P(bd), P(mo), P(ro), M, C, 1e-5, 0, 0, 0, 1, be.stream()),
                         [y, mo, ro])
    ref = twice(lambda: be.L.cdf_layernorm_c_fwd(P(xfd), C, P(yf), C, P(gd), P(bd), P(mf), P(rf), M, C, 1e-5, 0, 0, 0, be.stream()), [yf, mf, rf])
    assert bits_equal(yo, ref[0]) and bits_equal(moo, ref[1]) and bits_equal(roo, ref[2])
    check(f"layernorm fwd_io M={M} C={C}", yo, y_r, 5e-6)
    nb = be.L.cdf_layernorm_blocks(M, C)
    part, dxf, dgf, dbf = nan_empty(be, nb * 2 * C), nan_empty(be, M, C), nan_empty(be, C), nan_empty(be, C)
    dg, db = nan_empty(be, C), nan_empty(be, C)
    dx = nan_empty(be, M, C, dtype=torch.int16)
    mo.copy_(be.to(moo)), ro.copy_(be.to(roo))
    # ConvNeXt block form (io 7): dy, x, dx bf16
    dxfo, dgfo, dbfo = twice(lambda: be.L.cdf_layernorm_c_bwd(P(dyfd), C, P(xfd), C, P(gd), P(mo), P(ro), P(dxf), C, 0, 0, P(dgf), P(dbf), P(part),
                                                              M, C, 0, 0, be.stream()), [dxf, dgf, dbf, part])[:3]
    dxo, dgo, dbo = twice(lambda: be.L.cdf_layernorm_c_bwd_io(P(dybd), C, P(xbd), C, P(gd), P(mo), P(ro), P(dx), C, 0, 0, P(dg), P(db), P(part),
                                                              M, C, 0, 0, 7, be.stream()), [dx, dg, db, part])[:3]
    assert torch.equal(dxo.view(torch.bfloat16), dxfo.bfloat16()) and bits_equal(dgo, dgfo) and bits_equal(dbo, dbfo)
    check(f"layernorm bwd_io dx (fp32, before its rounding) M={M} C={C}", dxfo, dx_r, 1e-5)
    # attention block form (io 14): fp32 dy, bf16 x / dx / add
    add = torch.randn(M, C).bfloat16()
    addd, addf = be.to(add.view(torch.int16)), be.to(add.float())
    dxf2 = nan_empty(be, M, C)
    dxf2o = twice(lambda: be.L.cdf_layernorm_c_bwd(P(dyd), C, P(xfd), C, P(gd), P(mo), P(ro), P(dxf2), C, P(addf), C, P(dgf), P(dbf), P(part),
                                                   M, C, 0, 0, be.stream()), [dxf2, dgf, dbf, part])[0]
    dx2o = twice(lambda: be.L.cdf_layernorm_c_bwd_io(P(dyd), C, P(xbd), C, P(gd), P(mo), P(ro), P(dx), C, P(addd), C, P(dg), P(db), P(part),
                                                     M, C, 0, 0, 14, be.stream()), [dx, dg, db, part])[0]
    assert torch.equal(dx2o.view(torch.bfloat16), dxf2o.bfloat16())


# ---------------------------------------------------------------------------------------------------------------------------------
# GroupNorm (+ SiLU): config 2 shapes and the 64-chunk cap
# ---------------------------------------------------------------------------------------------------------------------------------
def _gn_ref(x, ga, bt, dy, groups, silu, eps=1e-6):
    B, HW, C = x.shape
    xx = x.double().requires_grad_(True)
    z = F.group_norm(xx.permute(0, 2, 1).reshape(B, C, HW, 1), groups, ga.double(), bt.double(), eps=eps)
    y = (z * torch.sigmoid(z) if silu else z).reshape(B, C, HW).permute(0, 2, 1)
    gad, btd = ga.double().requires_grad_(True), bt.double().requires_grad_(True)
    z = F.group_norm(xx.permute(0, 2, 1).reshape(B, C, HW, 1), groups, gad, btd, eps=eps)
    y = (z * torch.sigmoid(z) if silu else z).reshape(B, C, HW).permute(0, 2, 1)
    y.backward(dy.double())
    return y.detach(), xx.grad, gad.grad, btd.grad


@pytest.mark.parametrize("B,HW,C,big", [(2, 16384 + 37, 32, False),        # past the 64-chunk cap, ragged
                                         (128, 1024, 128, True), (128, 1024, 256, True),     # config 2 at 32 x 32
                                         (4, 16384, 128, True)])
def test_groupnorm_production(be, B, HW, C, big):
    skip_emu(be, big)
    torch.manual_seed(HW + C)
    groups, silu = 32, 1
    x, ga, bt, dy = torch.randn(B, HW, C), torch.randn(C), torch.randn(C), torch.randn(B, HW, C)
    y_r, dx_r, dga_r, dbt_r = _gn_ref(x, ga, bt, dy, groups, silu)
    nch = be.L.cdf_groupnorm_nchunk(HW)
    assert nch == min(64, max(1, HW // 256))
    xd, gd, bd, dyd = be.to(x), be.to(ga), be.to(bt), be.to(dy)
    ws = nan_empty(be, B * nch * 2 * C + B * 2 * C + B * groups * 2)
    y, mean, rstd = nan_empty(be, B, HW, C), nan_empty(be, B * groups), nan_empty(be, B * groups)
    yo, mo, ro = twice(lambda: be.L.cdf_groupnorm_fwd_ex(P(xd), C, P(y), C, P(gd), P(bd), P(mean), P(rstd), P(ws), B, HW, C, groups, 1e-6, silu,
                                                         0.0, 0, 0, 0, 0, be.stream()), [y, mean, rstd, ws])[:3]
    # A deliberate exception to the module's K_SUM rule: GroupNorm keeps the existing test's absolute bounds (y 1e-5, dx 2e-5 over groups
    # of <= 900 values; dgamma / dbeta 1e-4 over <= 600 rows) and grows them with the number of terms summed by sqrt(n / n_existing),
    # the random-walk growth of the same model.  At config 2 that is 14.8x for dgamma / dbeta, still well inside K_SUM * 2^-24 sqrt(n) ||t||.
    n_grp = HW * C // groups
    grow_g, grow_r = math.sqrt(max(1.0, n_grp / 900)), math.sqrt(max(1.0, B * HW / 600))
    check(f"groupnorm fwd B={B} HW={HW} C={C}", yo, y_r, 1e-5 * grow_g)
    dx, dga, dbe = nan_empty(be, B, HW, C), nan_empty(be, C), nan_empty(be, C)
    mean.copy_(be.to(mo)), rstd.copy_(be.to(ro))

    def bwd():
        be.L.cdf_groupnorm_bwd_ex(P(dyd), C, P(xd), C, P(gd), P(bd), P(mean), P(rstd), P(dx), C, P(dga), P(dbe), P(ws), B, HW, C, groups, silu,
                                  0, 0, 0.0, 0, be.stream())
    dxo, dgo, dbo = twice(bwd, [dx, dga, dbe, ws])[:3]
    # dx: each element carries two group sums of HW * C / groups terms (existing bound 2e-5)
    check(f"groupnorm bwd dx B={B} HW={HW} C={C}", dxo, dx_r, 2e-5 * grow_g)
    check(f"groupnorm bwd dgamma B={B} HW={HW} C={C}", dgo, dga_r, 1e-4 * grow_r)
    check(f"groupnorm bwd dbeta B={B} HW={HW} C={C}", dbo, dbt_r, 1e-4 * grow_r)


# ---------------------------------------------------------------------------------------------------------------------------------
# depthwise 7 x 7: 128 x 128 at C = 4 (3 padded) and 64, 16 x 16 at C = 512 / 1024, B = 64; the 32-bit offset guard
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C,H,big", [(2, 3, 128, False), (64, 3, 128, True), (64, 64, 128, True), (64, 512, 16, True), (64, 1024, 16, True),
                                       (3, 36, 37, False)])
def test_dwconv7_production(be, B, C, H, big):
    skip_emu(be, big)
    torch.manual_seed(C + H)
    Cp = r4(C)
    x, w = torch.randn(B, C, H, H), torch.randn(C, 1, 7, 7) / 7
    bias, sb = torch.randn(Cp), torch.randn(B, Cp)
    bias[C:], sb[:, C:] = 0, 0                                    # padded channel vectors (the product's layout)
    dy, rs = torch.randn(B, C, H, H), torch.randn(B, H, H, Cp)
    xn, dyn = be.to(nhwc(x)), be.to(nhwc(dy))                     # pad columns zero: new_feat(zero=True) when C % 4
    wp = nan_empty(be, 49, Cp)
    be.L.cdf_pack_weight(P(be.to(w)), P(wp), 49, 1, C, Cp, 1, 0, 49, be.stream())
    bd, sbd, rsd = be.to(bias), be.to(sb), be.to(rs)
    y, dx = nan_empty(be, B, H, H, Cp), nan_empty(be, B, H, H, Cp)
    yo = twice(lambda: be.L.cdf_dwconv7(P(xn), Cp, P(wp), Cp, P(bd), P(sbd), Cp, P(y), Cp, B, H, H, Cp, 0, 0, 0, 0, be.stream()), [y])[0]
    planes = Cp % 8 == 0
    ph, pl = nan_empty(be, B, H, H, Cp, dtype=torch.int16), nan_empty(be, B, H, H, Cp, dtype=torch.int16)
    if planes:
        dxo, pho, plo = twice(lambda: be.L.cdf_dwconv7_planes(P(dyn), Cp, P(wp), Cp, 0, 0, 0, P(dx), Cp, B, H, H, Cp, 1, 0, P(rsd), Cp, P(ph), P(pl), Cp,
                                                              be.stream()), [dx, ph, pl])
        rh, rl = _split(be, be.to(dxo).view(-1, Cp))
        assert torch.equal(pho.view(-1, Cp), rh.cpu()) and torch.equal(plo.view(-1, Cp), rl.cpu())
    else:
        dxo = twice(lambda: be.L.cdf_dwconv7(P(dyn), Cp, P(wp), Cp, 0, 0, 0, P(dx), Cp, B, H, H, Cp, 1, 0, P(rsd), Cp, be.stream()), [dx])[0]
    assert (yo[..., C:] == 0).all() and (dxo[..., C:] == rs[..., C:]).all()   # pad columns: zero weights and biases (+ the residual)
    # 49 products per output: bound K_SUM 2^-24 sqrt(49) ||terms||_2 (<= the existing 1e-5)
    s = sample(B)
    xs, dys, wd = x[s].double(), dy[s].double(), w.double()
    y_r = F.conv2d(xs, wd, bias[:C].double(), padding=3, groups=C) + sb[s, :C].double()[:, :, None, None]
    tb = min(1e-5, K_SUM * U * 7 * (xs.abs().max().item() * wd.abs().max().item() * 7 + bias.abs().max().item() + sb.abs().max().item()))
    check(f"dwconv7 fwd B={B} C={C} H={H}", yo[s][..., :C].permute(0, 3, 1, 2), y_r, tb)
    dx_r = F.conv_transpose2d(dys, wd, padding=3, groups=C) + rs[s][..., :C].permute(0, 3, 1, 2).double()
    check(f"dwconv7 dgrad B={B} C={C} H={H}", dxo[s][..., :C].permute(0, 3, 1, 2), dx_r, min(1e-5, 2 * tb))
    # weight / bias / time-bias gradients: sums over the whole batch (compared in full)
    nch = be.L.cdf_dwconv7_wgrad_nchunk(H)
    assert nch == min(32, max(1, H // 4))
    ws, dw, dbias, dsb = nan_empty(be, B * nch * 50 * C), nan_empty(be, C, 1, 7, 7), nan_empty(be, C), nan_empty(be, B, Cp)
    dwo, dbo, dsbo = twice(lambda: be.L.cdf_dwconv7_wgrad(P(xn), Cp, P(dyn), Cp, P(dw), P(dbias), P(dsb), Cp, P(ws), B, H, H, C, 0, be.stream()),
                           [dw, dbias, dsb, ws])[:3]
    xx, dd = x.double(), dy.double()
    dw_r = torch.nn.grad.conv2d_weight(xx, w.shape, dd, padding=3, groups=C)
    n = B * H * H
    # ||x dy||_2 over a tap's n terms is at most ||x||_inf ||dy||_2; the existing test allows 5e-5 * max(1, |ref|max)
    gb = K_SUM * U * math.sqrt(n) * xx.abs().max().item() * dd.pow(2).sum((0, 2, 3)).sqrt().max().item()
    check(f"dwconv7 wgrad dw B={B} C={C} H={H}", dwo, dw_r, min(gb, 5e-5 * max(1.0, dw_r.abs().max().item())))
    check(f"dwconv7 wgrad dbias B={B} C={C} H={H}", dbo, dd.sum((0, 2, 3)), min(sum_bound(dd.permute(1, 0, 2, 3).reshape(C, -1), 1),
                                                                               5e-5 * max(1.0, dd.sum((0, 2, 3)).abs().max().item())))
    dsb_r = dd.sum((2, 3))
    check(f"dwconv7 wgrad dsb B={B} C={C} H={H}", dsbo[:, :C], dsb_r, min(sum_bound(dd.reshape(B, C, -1), 2), 5e-5 * max(1.0, dsb_r.abs().max().item())))
    _dwconv7_io(be, x, dy, rs, wp, bd, sbd, B, C, H)


def _dwconv7_io(be, x, dy, rs, wp, bd, sbd, B, C, H):
    """The bf16 activation-storage forms at the same shape (the bf16 mode's bench step): cdf_dwconv7_io (io 1: bf16 x -> bf16 y; io 2:
    bf16 dy / res -> fp32 dx) and cdf_dwconv7_wgrad_io must compute exactly what the fp32 kernels compute on the widened values, the bf16
    output rounded once (test_bf16_storage's contract) -- so the fp64 bounds above carry over."""
    Cp = r4(C)
    xb, dyb, rsb = (t.bfloat16() for t in (nhwc(x), nhwc(dy), rs))
    xbd, dybd, rsbd = (be.to(t.view(torch.int16)) for t in (xb, dyb, rsb))
    xfd, dyfd, rsfd = (be.to(t.float()) for t in (xb, dyb, rsb))
    yf, yb = nan_empty(be, B, H, H, Cp), nan_empty(be, B, H, H, Cp, dtype=torch.int16)
    yfo = twice(lambda: be.L.cdf_dwconv7(P(xfd), Cp, P(wp), Cp, P(bd), P(sbd), Cp, P(yf), Cp, B, H, H, Cp, 0, 0, 0, 0, be.stream()), [yf])[0]
    ybo = twice(lambda: be.L.cdf_dwconv7_io(P(xbd), Cp, P(wp), Cp, P(bd), P(sbd), Cp, P(yb), Cp, B, H, H, Cp, 0, 0, 0, 0, 1, be.stream()), [yb])[0]
    assert torch.equal(ybo.view(torch.bfloat16), yfo.bfloat16())
    dxf, dx2 = nan_empty(be, B, H, H, Cp), nan_empty(be, B, H, H, Cp)
    dxfo = twice(lambda: be.L.cdf_dwconv7(P(dyfd), Cp, P(wp), Cp, 0, 0, 0, P(dxf), Cp, B, H, H, Cp, 1, 0, P(rsfd), Cp, be.stream()), [dxf])[0]
    dx2o = twice(lambda: be.L.cdf_dwconv7_io(P(dybd), Cp, P(wp), Cp, 0, 0, 0, P(dx2), Cp, B, H, H, Cp, 1, 0, P(rsbd), Cp, 2, be.stream()), [dx2])[0]
    assert bits_equal(dx2o, dxfo)
    nch = be.L.cdf_dwconv7_wgrad_nchunk(H)
    out = []
    for io in (0, 1):
        ws, dw, dbias, dsb = nan_empty(be, B * nch * 50 * C), nan_empty(be, C, 1, 7, 7), nan_empty(be, C), nan_empty(be, B, Cp)
        if io:
            launch = lambda: be.L.cdf_dwconv7_wgrad_io(P(xbd), Cp, P(dybd), Cp, P(dw), P(dbias), P(dsb), Cp, P(ws), B, H, H, C, 0, 1, be.stream())
        else:
            launch = lambda: be.L.cdf_dwconv7_wgrad(P(xfd), Cp, P(dyfd), Cp, P(dw), P(dbias), P(dsb), Cp, P(ws), B, H, H, C, 0, be.stream())
        out.append(twice(launch, [dw, dbias, dsb, ws])[:3])
    assert all(bits_equal(a, b) for a, b in zip(*out))


def test_dwconv7_planes_pitch_overflow_is_rejected(be):
    """The kernel's per-image element offsets are 32-bit (24 x 24-bit products): the host check must count the bf16 planes' pitch
    ld_ys too, and refuse before any launch.  H W ld_ys = 2^30 here while x / y have pitch 4.  Simulator only: without the check this
    is an out-of-bounds access."""
    if be.kind != "emu":
        pytest.skip("rejection of arguments that would be out of bounds: checked on the simulator only")
    from colddiff._lib import CdfError
    H = W = 1024
    t = be.zeros(64)
    hi, lo = torch.zeros(64, dtype=torch.int16), torch.zeros(64, dtype=torch.int16)
    with pytest.raises(CdfError, match="32-bit per-image offsets"):
        be.L.cdf_dwconv7_planes(P(t), 4, P(t), 4, 0, 0, 0, P(t), 4, 1, H, W, 4, 1, 0, 0, 0, P(hi), P(lo), 1024, be.stream())
    assert b"32-bit" in be.L.cdf_last_error()


# ---------------------------------------------------------------------------------------------------------------------------------
# the image-side block's direct convolutions at 128 x 128, B = 64 (M = 1,048,576: the chunk count is clamped to 1024)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,Cin,Cout,k,act,big", [(64, 128, 3, 128, 3, 1, True), (64, 128, 3, 64, 1, 0, True),
                                                    (1, 725, 3, 128, 3, 1, True),       # M = 512 * 1024 + 1337: past the cap, ragged chunks
                                                    (2, 50, 3, 16, 3, 1, False), (1, 37, 1, 8, 1, 0, False)])
def test_conv_cin4_first_block(be, B, H, Cin, Cout, k, act, big):
    skip_emu(be, big)
    torch.manual_seed(Cout + k)
    M = B * H * H
    x = torch.randn(B, Cin, H, H)
    conv = torch.nn.Conv2d(Cin, Cout, k, padding=k // 2)
    wt, bs = conv.weight.detach(), conv.bias.detach()
    g = torch.randn(B, Cout, H, H)
    KK = k * k
    xd, gd = be.to(nhwc(x)), be.to(g.permute(0, 2, 3, 1).contiguous())     # x: 3 channels padded to 4 with zeros (the product's layout)
    wp = nan_empty(be, KK, 4, Cout)
    be.L.cdf_pack_cin4(P(be.to(wt)), P(wp), Cout, Cout, Cin, k, be.stream())
    bd = be.to(bs)
    y, pre = nan_empty(be, B, H, H, Cout), nan_empty(be, B, H, H, Cout)
    yh, yl = nan_empty(be, B, H, H, Cout, dtype=torch.int16), nan_empty(be, B, H, H, Cout, dtype=torch.int16)
    yo, preo, yho, ylo = twice(lambda: be.L.cdf_conv_cin4_fwd(P(xd), P(wp), Cout, P(bd), P(y), Cout, P(pre), Cout, P(yh), P(yl), Cout, B, H, H, Cout,
                                                              k, act, be.stream()), [y, pre, yh, yl])
    rh, rl = _split(be, be.to(yo))
    assert torch.equal(yho, rh.cpu()) and torch.equal(ylo, rl.cpu())
    s = sample(B)
    xs, wd = x[s].double(), wt.double()
    pre_r = F.conv2d(xs, wd, bs.double(), padding=k // 2)
    y_r = F.gelu(pre_r) if act == 1 else pre_r
    tb = min(2e-5, K_SUM * U * math.sqrt(KK * Cin) * 2 * (xs.abs().max().item() * wd.abs().max().item() * math.sqrt(KK * Cin) + bs.abs().max().item()))
    check(f"conv_cin4 fwd pre {Cin}->{Cout} k{k} B={B} H={H}", preo[s].permute(0, 3, 1, 2), pre_r, tb)
    check(f"conv_cin4 fwd y {Cin}->{Cout} k{k} B={B} H={H}", yo[s].permute(0, 3, 1, 2), y_r, tb)
    # data gradient: Cout * k * k products per input element (existing bound 5e-5 * max(1, |ref|max))
    dx = nan_empty(be, B, H, H, 4)
    dxo = twice(lambda: be.L.cdf_conv_cin4_dgrad(P(gd), Cout, P(wp), Cout, P(dx), B, H, H, Cout, k, 0, be.stream()), [dx])[0]
    gs = g[s].double()
    dx_r = F.conv_transpose2d(gs, wd, padding=k // 2)
    db_ = K_SUM * U * math.sqrt(Cout * KK) * gs.abs().max().item() * wd.abs().max().item() * math.sqrt(Cout * KK)
    check(f"conv_cin4 dgrad {Cin}->{Cout} k{k} B={B} H={H}", dxo[s][..., :Cin].permute(0, 3, 1, 2), dx_r, min(db_, 5e-5 * max(1.0, dx_r.abs().max().item())))
    assert (dxo[..., Cin:] == 0).all()
    if k == 3:
        ldz = (9 * Cin + 3) // 4 * 4
        z = torch.zeros(B, H, H, ldz)
        z[..., :9 * Cin] = g.permute(0, 2, 3, 1).reshape(-1, Cout).matmul(wt.reshape(Cout, 9 * Cin)).reshape(B, H, H, 9 * Cin)
        zd, dx2 = be.to(z), nan_empty(be, B, H, H, 4)
        dx2o = twice(lambda: be.L.cdf_conv_cin4_tapsum3(P(zd), ldz, P(dx2), B, H, H, Cin, 0, be.stream()), [dx2])[0]
        zs = z[s][..., :9 * Cin].double().reshape(len(s), H, H, Cin, 3, 3)
        ts_r = torch.zeros(len(s), H + 2, H + 2, Cin, dtype=torch.float64)
        for i in range(3):
            for j in range(3):                                   # dx[q] = sum over taps (i, j) of z[q - (i - 1, j - 1)][tap]
                ts_r[:, i:i + H, j:j + H] += zs[..., i, j]
        ts_r = ts_r[:, 1:H + 1, 1:H + 1]
        check(f"conv_cin4 tapsum3 B={B} H={H}", dx2o[s][..., :Cin], ts_r, K_SUM * U * 3 * 2 * zs.abs().max().item())
        assert (dx2o[..., Cin:] == 0).all()
    # weight / bias gradients: per-chunk partials over the whole batch, then the fixed-order slab reduction
    nch = be.L.cdf_conv_cin4_nchunk(M)
    assert nch == min(1024, max(1, M // 512))
    part, bsum = nan_empty(be, nch, KK * Cin, Cout), nan_empty(be, nch, Cout)
    dw, dbv = nan_empty(be, Cout, Cin, k, k), nan_empty(be, Cout)

    def wgrad():
        be.L.cdf_conv_cin4_wgrad(P(xd), P(gd), Cout, P(part), P(bsum), B, H, H, Cin, Cout, k, be.stream())
        be.L.cdf_unpack_reduce(P(part), P(dw), nch, KK, Cin, Cout, Cout, 1, KK, Cin * KK, 0, 1, be.stream())
        be.L.cdf_unpack_reduce(P(bsum), P(dbv), nch, 1, 1, Cout, Cout, 0, 0, 1, 0, 1, be.stream())
    dwo, dbo = twice(wgrad, [dw, dbv, part, bsum])[:2]
    gg, xx = g.double(), x.double()
    dw_r = torch.nn.grad.conv2d_weight(xx, wt.shape, gg, padding=k // 2)
    gb = K_SUM * U * math.sqrt(M) * xx.abs().max().item() * gg.pow(2).sum((0, 2, 3)).sqrt().max().item()
    check(f"conv_cin4 wgrad dw {Cin}->{Cout} k{k} B={B} H={H}", dwo, dw_r, min(gb, 5e-5 * max(1.0, dw_r.abs().max().item())))
    db_r = gg.sum((0, 2, 3))
    check(f"conv_cin4 wgrad db {Cin}->{Cout} k{k} B={B} H={H}", dbo, db_r,
          min(sum_bound(gg.permute(1, 0, 2, 3).reshape(Cout, -1), 1), 5e-5 * max(1.0, db_r.abs().max().item())))


# ---------------------------------------------------------------------------------------------------------------------------------
# slab reduction at the slab counts the bench step launches
# ---------------------------------------------------------------------------------------------------------------------------------
# (nsplit, T, R, C) of cdf_unpack_reduce[_bias] calls of one bench step, recorded with test_gpu_invariance.Recorder (43 distinct calls,
# 4 .. 1024 slabs): the most slabs (the image-side block's 1024 clamped chunks), the widest reductions and each tap count
BENCH_UNPACK = [(1024, 9, 3, 128), (1024, 1, 3, 64), (995, 1, 64, 128), (498, 1, 256, 64), (249, 1, 128, 256), (125, 1, 128, 512),
                (42, 9, 128, 256), (21, 9, 256, 512), (16, 9, 256, 1024), (8, 9, 1024, 512), (8, 16, 256, 256), (32, 16, 128, 128),
                (4, 64, 128, 128)]


@pytest.mark.parametrize("ns,T,R,C", BENCH_UNPACK)
def test_unpack_reduce_bench_slab_counts(be, ns, T, R, C):
    skip_emu(be, ns * T * R * C > 4 << 20)
    torch.manual_seed(ns + T + R)
    ldc = r4(C)
    ws = torch.randn(ns, T, R, ldc)
    ws[..., C:] = float("nan")                                   # slab pad columns are not summed
    bws = torch.randn(ns, ldc)
    wsd, bwsd = be.to(ws), be.to(bws)
    ref = ws[..., :C].double().sum(0).permute(2, 1, 0)           # weight layout [C][R][T]
    bound = sum_bound(ws[..., :C].double(), 0)
    for tiled in (1, 0):
        g, gb = nan_empty(be, C, R, T), nan_empty(be, C)
        go, gbo = twice(lambda: be.L.cdf_unpack_reduce_bias(P(wsd), P(g), ns, T, R, C, ldc, 1, T, R * T, P(bwsd), P(gb), ldc, 0, tiled, be.stream()),
                        [g, gb])
        check(f"unpack_reduce_bias ns={ns} T={T} R={R} C={C} tiled={tiled}", go, ref, bound)
        check(f"unpack_reduce_bias bias ns={ns} C={C}", gbo, bws[:, :C].double().sum(0), sum_bound(bws[:, :C].double(), 0))


# ---------------------------------------------------------------------------------------------------------------------------------
# linear attention at n = 16384 (128 x 128), 4 heads: 64 splits; the fused and the unfused backward
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,n,big", [(2, 300, False), (64, 16384, True)])
@pytest.mark.parametrize("fused", [True, False])
def test_linattn_production(be, B, n, big, fused, monkeypatch):
    """ops.linattn_fwd / linattn_bwd (cdf_linattn_context, the K = 32 head GEMMs, cdf_linattn_dcontext, then cdf_linattn_bwd_kv or the
    unfused cdf_linattn_softk + cdf_linattn_dk) with every allocation of the op poisoned, twice."""
    skip_emu(be, big)
    from colddiff import ops, runtime
    monkeypatch.setattr(ops, "_ATTN_KV_FUSED", fused)
    torch.manual_seed(n)
    heads, HD, scale = 4, 128, 32 ** -0.5
    assert be.L.cdf_linattn_nsplit(n) == (n + 255) // 256
    qkv, do = torch.randn(B, n, 3 * HD), torch.randn(B, n, HD)
    saved = runtime._lib_override
    if be.kind == "emu":
        runtime._lib_override = be.L
    try:
        qd, dod = be.to(qkv).view(B, 1, n, 3 * HD), be.to(do).view(B, 1, n, HD)
        res = []
        for _ in range(2):
            with poisoned_allocations():
                out, ctx, ctxs, kmax, ksum = ops.linattn_fwd(qd, heads, scale)
                dqkv = ops.linattn_bwd(qd, dod, ctx, ctxs, kmax, ksum, heads, scale)
            res.append([t.detach().cpu().clone() for t in (out, ctx, dqkv)])
    finally:
        runtime._lib_override = saved
    for a, b in zip(*res):
        assert bits_equal(a, b)
    out, ctx, dqkv = (t.view(B, n, -1) if t.dim() == 4 and t.shape[1] == 1 else t for t in res[0])
    s = sample(B)
    q_, k_, v_ = (t.double().view(len(s), n, heads, 32) for t in qkv[s].chunk(3, dim=2))
    qq, kk, vv = (t.clone().requires_grad_(True) for t in (q_, k_, v_))
    P_ = kk.softmax(dim=1)
    ctx_r = torch.einsum("bnhd,bnhe->bhde", P_, vv)
    out_r = torch.einsum("bhde,bnhd->bnhe", ctx_r, qq * scale).reshape(len(s), n, HD)
    out_r.backward(do[s].double())
    dqkv_r = torch.cat([qq.grad.reshape(len(s), n, HD), kk.grad.reshape(len(s), n, HD), vv.grad.reshape(len(s), n, HD)], 2)
    # ctx is a softmax-weighted mean over n (the weights sum to 1), so its error does not grow with n the way a plain sum's does: the
    # existing test's absolute bounds (ctx / out 2e-6, dqkv 5e-6, at n <= 600) hold as they are
    check(f"linattn ctx B={B} n={n}", ctx[s], ctx_r.detach(), 2e-6)
    check(f"linattn out B={B} n={n}", out.view(B, n, HD)[s], out_r.detach(), 2e-6)
    check(f"linattn dqkv B={B} n={n} fused={fused}", dqkv.view(B, n, 3 * HD)[s], dqkv_r, 5e-6)


# ---------------------------------------------------------------------------------------------------------------------------------
# the folded attention block's kernels (the path the bench step takes): fused k | v projection + context, the k / v backward as bf16
# planes, and the dctx / rvec finish, at n = 16384 (128 x 128), B = 64
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,n,dim,split,big", [(64, 16384, 64, 3, True), (64, 16384, 64, 1, True),     # 128 x 128 level, bf16x3 / bf16
                                               (64, 4096, 128, 3, True), (16, 16384, 64, 3, True),     # 64 x 64 level; the sampler's B
                                               (2, 384, 64, 3, False)])
def test_linattn_kvctx_production(be, B, n, dim, split, big):
    """cdf_linattn_kvctx (k | v = xn . Wkv^T with the softmax context accumulated per part) + cdf_linattn_finalize (the reduction over
    cdf_linattn_kvctx_parts parts, library-default slots as the package passes) with poisoned kv / workspace / outputs, twice.  Bounds:
    those of test_kernels.py::test_linattn_kvctx_fused (kv: the split-precision GEMM's 3e-5, or 2e-2 for hi-only operands, of |kv|max;
    ksum 1e-5 of its max; ctx 2e-5 of max(1, |ctx|max); kmax exact for the kv written), which are already scale-relative."""
    skip_emu(be, big)
    torch.manual_seed(n + dim)
    heads, HD, scale = 4, 128, 32 ** -0.5
    xn = torch.randn(B, n, dim)
    w = torch.randn(3 * HD, dim) / math.sqrt(dim)
    w[HD:2 * HD] *= 3.0
    xn[..., 0] += torch.linspace(-6, 6, n)
    ldk = (dim + 31) // 32 * 32
    whi = torch.zeros(1, 2 * HD, ldk, dtype=torch.int16, device=be.device)
    wlo = torch.zeros_like(whi) if split == 3 else None
    wd = be.to(w)
    be.L.cdf_pack_weight_bf16(P(wd) + 4 * HD * dim, P(whi), P(wlo), 1, 2 * HD, dim, ldk, 1, dim, 1, be.stream())
    be._keep += [whi, wlo]
    parts = be.L.cdf_linattn_kvctx_parts(B, n, 0)
    xd = be.to(xn)
    kv, ws = nan_empty(be, B, n, 2 * HD), nan_empty(be, B * parts * (2 * HD + heads * 1024))
    ctx, ctxs, kmax, ksum = nan_empty(be, B, heads, 32, 32), nan_empty(be, B, heads, 32, 32), nan_empty(be, B, HD), nan_empty(be, B, HD)

    def launch():
        be.L.cdf_linattn_kvctx(P(xd), dim, P(whi), P(wlo), ldk, P(kv), 2 * HD, P(ws), B, n, dim, heads, 0, be.stream())
        be.L.cdf_linattn_finalize(P(ws), parts, P(ctx), P(ctxs), P(kmax), P(ksum), B, heads, scale, be.stream())
    kvo, ctxo, ctxso, kmaxo, ksumo = twice(launch, [kv, ctx, ctxs, kmax, ksum, ws])[:5]
    s = sample(B)
    kv_ref = xn[s].double() @ w[HD:].double().t()
    check(f"linattn_kvctx kv B={B} n={n} dim={dim} split={split} parts={parts}", kvo[s], kv_ref,
          (3e-5 if split == 3 else 2e-2) * kv_ref.abs().max().item())
    kvc = kvo[s].double()
    k, v = kvc[..., :HD], kvc[..., HD:]
    kmax_ref = k.max(1).values
    e = torch.exp(k - kmax_ref[:, None])
    ksum_ref = e.sum(1)
    ctx_ref = torch.einsum("bnhd,bnhe->bhde", (e / ksum_ref[:, None]).view(len(s), n, heads, 32), v.view(len(s), n, heads, 32))
    assert torch.equal(kmaxo[s], kmax_ref.float())
    check(f"linattn_finalize ksum B={B} n={n}", ksumo[s], ksum_ref, 1e-5 * ksum_ref.max().item())
    check(f"linattn_finalize ctx B={B} n={n}", ctxo[s], ctx_ref, 2e-5 * max(1.0, ctx_ref.abs().max().item()))
    check(f"linattn_finalize ctxs B={B} n={n}", ctxso[s], ctx_ref * scale, 2e-5 * max(1.0, ctx_ref.abs().max().item()))


@pytest.mark.parametrize("B,n,heads,big", [(64, 16384, 4, True), (16, 16384, 4, True), (64, 4096, 4, True), (2, 300, 4, False)])
def test_linattn_bwd_kv_planes_production(be, B, n, heads, big):
    """cdf_linattn_bwd_kv (fp32) and cdf_linattn_bwd_kv_planes (dk | dv as bf16 hi / lo planes, and hi only) on a (k | v) tensor with
    poisoned outputs, twice: the fp32 result against fp64 (bound of test_kernels.py::test_linattn_bwd_kv_fused: 2e-5 of max(1, |ref|max)
    -- dk / dv are 32-term products of a softmax column, so the error does not grow with n), the planes bit-equal to cdf_split_bf16 of it."""
    skip_emu(be, big)
    torch.manual_seed(n + B)
    HD = heads * 32
    kv = torch.randn(B, n, 2 * HD)
    k, v = kv[..., :HD], kv[..., HD:]
    kmax = k.max(1).values
    ksum = torch.exp(k - kmax[:, None]).sum(1)
    dctx, ctx = torch.randn(B, heads, 32, 32) * 0.3, torch.randn(B, heads, 32, 32)
    rvec = (dctx * ctx).sum(-1).reshape(B, HD)
    kvd, dctxd, rvecd, kmd, ksd = be.to(kv), be.to(dctx), be.to(rvec), be.to(kmax), be.to(ksum)
    out = nan_empty(be, B, n, 2 * HD)
    outo = twice(lambda: be.L.cdf_linattn_bwd_kv(P(kvd), 2 * HD, 0, P(dctxd), P(rvecd), P(kmd), P(ksd), P(out), 2 * HD, 0, B, n, heads,
                                                 be.stream()), [out])[0]
    hi, lo, hi1 = (nan_empty(be, B, n, 2 * HD, dtype=torch.int16) for _ in range(3))
    hio, loo = twice(lambda: be.L.cdf_linattn_bwd_kv_planes(P(kvd), 2 * HD, 0, P(dctxd), P(rvecd), P(kmd), P(ksd), P(hi), P(lo), 2 * HD, 0, B, n,
                                                            heads, be.stream()), [hi, lo])
    hi1o = twice(lambda: be.L.cdf_linattn_bwd_kv_planes(P(kvd), 2 * HD, 0, P(dctxd), P(rvecd), P(kmd), P(ksd), P(hi1), 0, 2 * HD, 0, B, n,
                                                        heads, be.stream()), [hi1])[0]
    rh, rl = _split(be, be.to(outo))
    assert torch.equal(hio, rh.cpu()) and torch.equal(loo, rl.cpu()) and torch.equal(hi1o, rh.cpu())
    s = sample(B)
    kd, vd = k[s].double(), v[s].double()
    Pn = torch.exp(kd - kmax[s].double()[:, None]) / ksum[s].double()[:, None]
    Ph, vh, dc = Pn.view(len(s), n, heads, 32), vd.view(len(s), n, heads, 32), dctx[s].double()
    dP = torch.einsum("bnhe,bhde->bnhd", vh, dc)
    dk_ref = (Ph * (dP - rvec[s].double().view(len(s), 1, heads, 32))).reshape(len(s), n, HD)
    dv_ref = torch.einsum("bnhd,bhde->bnhe", Ph, dc).reshape(len(s), n, HD)
    check(f"linattn_bwd_kv dk B={B} n={n}", outo[s][..., :HD], dk_ref, 2e-5 * max(1.0, dk_ref.abs().max().item()))
    check(f"linattn_bwd_kv dv B={B} n={n}", outo[s][..., HD:], dv_ref, 2e-5 * max(1.0, dv_ref.abs().max().item()))


@pytest.mark.parametrize("B,heads,extra", [(64, 4, 0), (16, 4, 0), (2, 4, 5)])
def test_linattn_dctx_finish_production(be, B, heads, extra):
    """cdf_linattn_dctx_finish: dctx = scale * raw (one rounding: <= 2^-24 |dctx|), rvec[row] = sum over 32 entries of dctx * ctx
    (K_SUM model, plus dctx's own rounding carried through |ctx|).  rows = B * heads * 32 (+ extra: a ragged last block)."""
    torch.manual_seed(B + extra)
    scale = 32 ** -0.5
    rows = B * heads * 32 + extra
    raw, ctx = torch.randn(rows, 32) * 3, torch.randn(rows, 32)
    rawd, ctxd = be.to(raw), be.to(ctx)
    dctx, rvec = nan_empty(be, rows, 32), nan_empty(be, rows)
    dctxo, rveco = twice(lambda: be.L.cdf_linattn_dctx_finish(P(rawd), P(ctxd), P(dctx), P(rvec), rows, scale, be.stream()), [dctx, rvec])
    sc = torch.tensor(scale, dtype=torch.float32).double()
    dctx_r = raw.double() * sc
    check(f"linattn_dctx_finish dctx rows={rows}", dctxo, dctx_r, U * dctx_r.abs().max().item())
    terms = dctx_r * ctx.double()
    check(f"linattn_dctx_finish rvec rows={rows}", rveco, terms.sum(1),
          sum_bound(terms, 1) + U * math.sqrt(32) * (dctx_r.abs() * ctx.double().abs()).pow(2).sum(1).sqrt().max().item())
