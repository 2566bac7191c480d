"""The small kernels (csrc/k_misc.hip, csrc/k_pool.hip), the row softmax (k_attn.hip) and cdf_norm_param_reduce (k_norm.hip) past
their grid caps -- to the contract of test_kernels_production.py: float64 CPU references from the same inputs, every output, workspace
and pad column NaN-poisoned before each launch, every launch made twice and compared bit for bit, every comparison printed as
worst error / bound.

Every kernel of k_misc.hip / k_pool.hip is a grid-stride loop under a grid cap, and the softmax rows walk under a row cap; a case "past
a cap" is the smallest shape with cap + 261 work items (a ragged second pass that ends inside a block).  Bounds count fp32 roundings
(u = 2^-24 each, of the magnitude stated with the count); sums use the sum model of test_kernels_production.py.  Kernels that update
their output in place (Adam, EMA, scale, axpby with alpha != 0, the accumulate forms) are run twice from the same restored state."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from poison import nan_empty, poison_
from test_kernels import P
from test_kernels_production import K_SUM, U, bits_equal, check, skip_emu, sum_bound, twice

CAP = 8192 * 256          # threads of a k_misc.hip launch: ew_grid's `if (g > 8192) g = 8192` blocks of 256 (csrc/k_misc.hip, ew_grid)
PCAP = 16384 * 256        # k_pool.hip: `blocks = ... < 256 * 64 ? ... : 256 * 64` blocks of 256 (cdf_pool2d, cdf_resize_bilinear_nhwc)
RCAP = 4096 * 4           # rows of a softmax launch: `if (g > 4096) g = 4096` blocks of 4 waves, one row per wave (csrc/k_attn.hip)
PAST = 261
TINY = 2.0 ** -126        # smallest normal fp32: a result below it may be rounded as a subnormal or flushed to zero


def f32(v):
    """v rounded to fp32, as a Python float (how a C `(float)` cast of a host double reaches the kernel)."""
    return float(np.float32(v))


def rows_past(cap, C):
    """The fewest rows with rows * C >= cap + 261; the last block of the second pass must be ragged."""
    rows = -(-(cap + PAST) // C)
    assert rows * C > cap and (rows * C) % 256 != 0
    return rows


def check_elem(name, got, ref, bound):
    """Element-wise bound (float64 tensors): prints the worst error / its bound; where the bound is 0 the result must be exact."""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape == bound.shape, (name, got.shape, ref.shape, bound.shape)
    assert torch.isfinite(got).all(), (name, "non-finite output")
    e = (got - ref).abs()
    ratio = torch.where(e == 0, torch.zeros_like(e), e / bound).reshape(-1)
    i = int(ratio.argmax())
    print(f"{name}: worst error {e.reshape(-1)[i].item():.3e} / bound {bound.reshape(-1)[i].item():.3e} = {ratio[i].item():.3f}")
    assert ratio[i].item() <= 1.0, (name, i, e.reshape(-1)[i].item(), bound.reshape(-1)[i].item())


def twice_inplace(be, launch, state, init):
    """For kernels that update `state` (device tensors) in place: restore it from `init` (host tensors, pads poisoned), launch, keep;
    restore, launch again: bit for bit the same.  Returns the results on the host."""
    res = []
    for _ in range(2):
        for s, i in zip(state, init):
            s.copy_(i)
        launch()
        if be.kind == "hip":
            torch.cuda.synchronize()
        res.append([s.detach().cpu().clone() for s in state])
    for k, (a, b) in enumerate(zip(*res)):
        assert bits_equal(a, b), ("second launch differs", k)
    return res[0]


def pitched(t, ld):
    """[rows, C] -> [rows, ld] with NaN pad columns."""
    out = torch.full((t.shape[0], ld), float("nan"))
    out[:, :t.shape[1]] = t
    return out


def pads_untouched(t, C):
    """Every pad column of a poisoned output still holds its poison."""
    return bool(torch.isnan(t[..., C:]).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the optimizer tail over a flat arena
# ---------------------------------------------------------------------------------------------------------------------------------
def test_adam_ema_scale_past_grid_cap(be):
    """cdf_adam_step at n = CAP + 261, steps 1, 2, 100000, 100001 on one evolving state, against one float64 step of the recurrence in
    the comment above adam_kernel, started from the kernel's own (p, m, v) before that step (so errors do not compound) with the host
    scalars rounded to fp32 as cdf_adam_step rounds them.  torch.optim.Adam is NOT the reference here: its lerp rounds exp_avg
    differently from the documented expression (the share of elements that differ after one step is printed, not asserted)."""
    torch.manual_seed(1)
    n = CAP + PAST
    lr, b1, b2, eps = 2e-5, 0.9, 0.999, 1e-8
    p0 = torch.randn(n)
    p0[:1000] *= 1e-5
    pd, md, vd, gd = be.to(p0), be.zeros(n), be.zeros(n), be.zeros(n)
    omb1, b2f, omb2, epsf = f32(1.0 - b1), f32(b2), f32(1.0 - b2), f32(eps)
    for step in (1, 2, 100000, 100001):
        g = torch.randn(n) * (10.0 ** torch.randint(-6, 2, (n,)).double()).float()
        g[::7] = 0.0
        gd.copy_(g)
        pre = [t.detach().cpu().clone() for t in (pd, md, vd)]
        po, mo, vo = twice_inplace(be, lambda: be.L.cdf_adam_step(P(pd), P(gd), P(md), P(vd), n, lr, b1, b2, eps, step, be.stream()),
                                   [pd, md, vd], pre)
        bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
        nss, bc2s = f32(-(lr / bc1)), f32(math.sqrt(bc2))
        Pd, Md, Vd, G = pre[0].double(), pre[1].double(), pre[2].double(), g.double()
        # m' = m + (g - m) * (1 - b1): 3 roundings (difference, product, sum), each of a quantity <= |g| + |m|
        check_elem(f"adam step {step} m", mo, Md + (G - Md) * omb1, 3 * U * (G.abs() + Md.abs()))
        # v' = v * b2 + ((1 - b2) * g) * g: 4 roundings (three products, one sum), each of a quantity <= |v| + g^2
        check_elem(f"adam step {step} v", vo, Vd * b2f + (omb2 * G) * G, 4 * U * (Vd.abs() + G * G))
        # p' = p + (-step_size * m') / (sqrt(v') / bc2_sqrt + eps) from the kernel's own m', v': the last sum rounds to u |p'|; before it
        # sqrt, quotient, + eps, product, quotient -- 5 roundings, each relative to the update p' - p; K counts all 6 of the expression
        p_ref = Pd + (nss * mo.double()) / (vo.double().sqrt() / bc2s + epsf)
        check_elem(f"adam step {step} p", po, p_ref, U * p_ref.abs() + 6 * U * (p_ref - Pd).abs())
        still = (g == 0) & (pre[1] == 0) & (pre[2] == 0)
        assert int(still.sum()) >= n // 7                        # g == 0 on zero moments: p must not move at all (no bound covers this)
        assert bits_equal(po[still], pre[0][still]) and not mo[still].any() and not vo[still].any()
        if step == 1:
            pt = p0.clone().requires_grad_()
            opt = torch.optim.Adam([pt], lr=lr, betas=(b1, b2), eps=eps)
            pt.grad = g.clone()
            opt.step()
            print("not bit-equal to torch.optim.Adam after step 1 from zero state: p %.4f%%, exp_avg %.4f%%, exp_avg_sq %.4f%%" % (
                100 * (pt.detach() != po).float().mean().item(), 100 * (opt.state[pt]["exp_avg"] != mo).float().mean().item(),
                100 * (opt.state[pt]["exp_avg_sq"] != vo).float().mean().item()))
    # EMA: ma' = ma * beta + (1 - beta) * p: two products and a sum, |error| <= 2 u (|ma beta| + |(1 - beta) p|)
    ma = torch.randn(n)
    mad = be.to(ma)
    mao = twice_inplace(be, lambda: be.L.cdf_ema_update(P(mad), P(pd), n, 0.995, be.stream()), [mad], [ma])[0]
    a, b = ma.double() * f32(0.995), f32(1.0 - 0.995) * pd.detach().cpu().double()
    check_elem("ema", mao, a + b, 2 * U * (a.abs() + b.abs()))
    # scale: one product, one rounding; also at the last size of a single pass
    for m in (CAP - 1, CAP + PAST):
        x = torch.randn(m)
        xd = be.to(x)
        xo = twice_inplace(be, lambda: be.L.cdf_scale(P(xd), m, 0.37, be.stream()), [xd], [x])[0]
        ref = x.double() * f32(0.37)
        check_elem(f"scale n={m}", xo, ref, U * ref.abs())


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. axpby: copies (alpha == 0), skip-connection sums
# ---------------------------------------------------------------------------------------------------------------------------------
def test_axpby_past_grid_cap(be):
    torch.manual_seed(2)
    C, ldd, lds = 37, 40, 43
    rows = rows_past(CAP, C)
    d0, s = torch.randn(rows, C), torch.randn(rows, C)
    sd = be.to(pitched(s, lds))
    dst = nan_empty(be, rows, ldd)
    # the copy form: the destination is never read (it is NaN, pad columns and all)
    out = twice(lambda: be.L.cdf_axpby(P(dst), ldd, P(sd), lds, rows, C, 0.0, 1.0, be.stream()), [dst])[0]
    assert bits_equal(out[:, :C], s) and pads_untouched(out, C)
    init = pitched(d0, ldd)
    for beta, want in ((1.0, d0 + s), (-1.0, d0 - s)):
        out = twice_inplace(be, lambda: be.L.cdf_axpby(P(dst), ldd, P(sd), lds, rows, C, 1.0, beta, be.stream()), [dst], [init])[0]
        assert bits_equal(out[:, :C], want) and pads_untouched(out, C), beta
    alpha, beta = 0.7, -1.3
    out = twice_inplace(be, lambda: be.L.cdf_axpby(P(dst), ldd, P(sd), lds, rows, C, alpha, beta, be.stream()), [dst], [init])[0]
    a, b = f32(alpha) * d0.double(), f32(beta) * s.double()
    check_elem("axpby alpha=0.7 beta=-1.3", out[:, :C], a + b, 3 * U * (a.abs() + b.abs()))      # two products and a sum
    assert pads_untouched(out, C)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. GELU / SiLU / ReLU on vectors, and their derivatives
# ---------------------------------------------------------------------------------------------------------------------------------
SQRT1_2, INV_SQRT_2PI = 0.70710678118654752440, 0.39894228040143267794
ERF_ERR = 1.5e-7          # cdf_common.h: Abramowitz & Stegun 7.1.26, |error| <= 1.5e-7 absolute
# fp32 roundings, counted in cdf_common.h:
#   cdf_gelu: x / sqrt 2, the fma under the reciprocal, the reciprocal, z^2, expf, four polynomial fmas, p t, the fma that ends erf,
#             1 + erf, the product with 0.5 x                                                                            -> 13
#   cdf_silu: expf, 1 + e, the quotient, the product with x                                                             -> 4
#   cdf_gelu_grad: the 11 of erf, 1 + erf, 0.3989 e, its product with x, the sum                                        -> 15
#   cdf_silu_grad: the 3 of the sigmoid, 1 - s, its product with x, 1 + that, the product with s                        -> 7
R_GELU, R_SILU, R_DGELU, R_DSILU = 13, 4, 15, 7


def _act_ref(x, act):
    """(y, dy/dx, bound of y, bound of dy/dx) in float64: the erf formula's documented error (halved by the 0.5, times |x| in GELU) plus
    R roundings of quantities <= max(1, |x|)."""
    x = x.double()
    big = x.abs().clamp_min(1.0)
    if act == 1:
        cdf = 0.5 * (1.0 + torch.special.erf(x * SQRT1_2))
        return x * cdf, cdf + x * INV_SQRT_2PI * torch.exp(-0.5 * x * x), 0.5 * ERF_ERR * x.abs() + R_GELU * U * big, 0.5 * ERF_ERR + R_DGELU * U * big
    if act == 2:
        s = torch.sigmoid(x)
        return x * s, s * (1.0 + x * (1.0 - s)), R_SILU * U * big, R_DSILU * U * big
    return x.clamp_min(0.0), None, torch.zeros_like(x), None


def _act_points():
    return torch.cat([torch.linspace(-12.0, 12.0, 1 << 21), torch.tensor([0.0, -0.0, 1e-30, -1e-30, 40.0, -40.0, 1e4, -1e4])])


@pytest.mark.parametrize("C,ldx,ldy,lddy", [(1, 1, 1, 1), (5, 8, 7, 6)])           # one column; a pitched block with NaN pad columns
@pytest.mark.parametrize("act", [1, 2, 3])
def test_act_past_grid_cap(be, act, C, ldx, ldy, lddy):
    torch.manual_seed(3)
    pts = _act_points()
    n = pts.numel()
    assert n > CAP and n % C == 0 and n % 256 != 0
    rows = n // C
    x = pts.view(rows, C)
    y_r, d_r, y_b, d_b = _act_ref(x, act)
    xd = be.to(pitched(x, ldx))
    y = nan_empty(be, rows, ldy)
    yo = twice(lambda: be.L.cdf_act_fwd(P(xd), ldx, P(y), ldy, rows, C, act, be.stream()), [y])[0]
    assert not torch.isnan(yo[:, :C]).any() and pads_untouched(yo, C)
    check_elem(f"act_fwd act={act} C={C}", yo[:, :C], y_r, y_b)
    if act == 3:
        return
    dy, prior = torch.randn(rows, C), torch.randn(rows, C)
    dyd = be.to(pitched(dy, lddy))
    dx = nan_empty(be, rows, ldy)
    g_r = dy.double() * d_r
    g_b = dy.double().abs() * d_b + U * g_r.abs()                # the derivative's error, and the product's rounding
    dxo = twice(lambda: be.L.cdf_act_bwd(P(xd), ldx, P(dyd), lddy, P(dx), ldy, rows, C, act, 0, be.stream()), [dx])[0]
    assert not torch.isnan(dxo[:, :C]).any() and pads_untouched(dxo, C)
    check_elem(f"act_bwd act={act} C={C}", dxo[:, :C], g_r, g_b)
    # accumulate: prior + g, one more rounding (from the kernel's own g, which the launch above left bit for bit)
    dxa = twice_inplace(be, lambda: be.L.cdf_act_bwd(P(xd), ldx, P(dyd), lddy, P(dx), ldy, rows, C, act, 1, be.stream()), [dx], [pitched(prior, ldy)])[0]
    assert pads_untouched(dxa, C)
    assert bits_equal(dxa[:, :C], prior + dxo[:, :C])
    a_r = prior.double() + g_r
    check_elem(f"act_bwd accumulate act={act} C={C}", dxa[:, :C], a_r, g_b + U * a_r.abs())


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. sinusoidal time embedding
# ---------------------------------------------------------------------------------------------------------------------------------
def test_sinusoidal_past_grid_cap(be):
    """sin / cos of the fp32 product (float)t * freq -- the kernel's documented phase (the table is data): the float64 reference takes the
    same fp32 phase.  Bound: the existing 5e-6."""
    dim, ldo = 64, 68
    half = dim // 2
    B = rows_past(CAP, half)
    t = torch.tensor([0, 5, 199, 999]).repeat(-(-B // 4))[:B]
    freq = torch.exp(torch.arange(half) * -(math.log(10000) / (half - 1)))
    out = nan_empty(be, B, ldo)
    td, fd = be.to(t), be.to(freq)
    o = twice(lambda: be.L.cdf_sinusoidal(P(td), P(fd), P(out), ldo, B, dim, be.stream()), [out])[0]
    phase = (t.float()[:, None] * freq[None, :]).double()
    check(f"sinusoidal B={B} dim={dim}", o[:, :dim], torch.cat((phase.sin(), phase.cos()), 1), 5e-6)
    assert pads_untouched(o, dim)


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. nearest x2 upsample and its adjoint (float4 lanes)
# ---------------------------------------------------------------------------------------------------------------------------------
def _up_batch(H, W, C4, per_pixel):
    B = -(-(CAP + PAST) // (per_pixel * H * W * C4))
    assert (B * per_pixel * H * W * C4) % 256 != 0
    return B


def test_upsample2_past_grid_cap(be):
    torch.manual_seed(5)
    H, W, C, ldx, ldy = 37, 41, 12, 16, 20
    B = _up_batch(H, W, C // 4, 4)
    x = torch.full((B, H, W, ldx), float("nan"))
    x[..., :C] = torch.randn(B, H, W, C)
    xd, y = be.to(x), nan_empty(be, B, 2 * H, 2 * W, ldy)
    yo = twice(lambda: be.L.cdf_upsample2(P(xd), ldx, P(y), ldy, B, H, W, C, be.stream()), [y])[0]
    assert bits_equal(yo[..., :C], x[..., :C].repeat_interleave(2, 1).repeat_interleave(2, 2)) and pads_untouched(yo, C)


def test_upsample2_bwd_past_grid_cap(be):
    torch.manual_seed(6)
    H, W, C, lddy, lddx = 37, 41, 12, 16, 20
    B = _up_batch(H, W, C // 4, 1)
    dy = torch.full((B, 2 * H, 2 * W, lddy), float("nan"))
    dy[..., :C] = torch.randn(B, 2 * H, 2 * W, C)
    v = dy[..., :C]
    want = (v[:, 0::2, 0::2] + v[:, 0::2, 1::2]) + (v[:, 1::2, 0::2] + v[:, 1::2, 1::2])        # the kernel's order, in fp32
    dyd, dx = be.to(dy), nan_empty(be, B, H, W, lddx)
    dxo = twice(lambda: be.L.cdf_upsample2_bwd(P(dyd), lddy, P(dx), lddx, B, H, W, C, 0, be.stream()), [dx])[0]
    assert bits_equal(dxo[..., :C], want) and pads_untouched(dxo, C)
    prior = torch.full((B, H, W, lddx), float("nan"))
    prior[..., :C] = torch.randn(B, H, W, C)
    dxa = twice_inplace(be, lambda: be.L.cdf_upsample2_bwd(P(dyd), lddy, P(dx), lddx, B, H, W, C, 1, be.stream()), [dx], [prior])[0]
    assert bits_equal(dxa[..., :C], want + prior[..., :C]) and pads_untouched(dxa, C)


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. dropout: the mask against an independent statement of cdf_hash32
# ---------------------------------------------------------------------------------------------------------------------------------
def _hash32(seed, idx):
    """cdf_hash32 (csrc/cdf_common.h) on numpy uint64 (wrapping arithmetic)."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + idx.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(32)).astype(np.uint32)


def test_dropout_past_grid_cap(be):
    torch.manual_seed(7)
    C, ldx, ldy, p = 10, 12, 11, 0.1
    rows = rows_past(CAP, C)
    seed = (1 << 40) + 12345
    x = torch.randn(rows, C)
    xd, y = be.to(pitched(x, ldx)), nan_empty(be, rows, ldy)
    yo = twice(lambda: be.L.cdf_dropout(P(xd), ldx, P(y), ldy, rows, C, p, seed, be.stream()), [y])[0]
    pf = np.float32(p)
    thr = np.uint32(int(float(pf) * 4294967296.0))
    keep = torch.from_numpy(_hash32(seed, np.arange(rows * C)) >= thr).view(rows, C)          # idx = row * C + c
    inv = torch.tensor(np.float32(1.0) / (np.float32(1.0) - pf))
    assert bits_equal(yo[:, :C], torch.where(keep, x * inv, torch.zeros(())))                 # mask and kept values, exactly
    assert pads_untouched(yo, C)
    share, sigma = keep.float().mean().item(), math.sqrt(p * (1 - p) / (rows * C))
    print(f"dropout kept share {share:.6f}, expected {1 - p:.6f}: {abs(share - (1 - p)) / sigma:.2f} sigma")
    assert abs(share - (1 - float(pf))) <= 5 * sigma
    yo = twice(lambda: be.L.cdf_dropout(P(xd), ldx, P(y), ldy, rows, C, 0.0, seed, be.stream()), [y])[0]
    assert bits_equal(yo[:, :C], x) and pads_untouched(yo, C)


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. row softmax and its backward: one wave per row, lanes stride the row by 64
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,n", [(203, 64), (203, 65), (203, 256), (203, 1000), (RCAP + 37, 200)])
def test_softmax_rows_production(be, rows, n):
    """Forward bound, per probability p_j = e_j / S with e_j = exp(a_j), a_j = z_j - m, z = scale * s:
      * the argument a_j is an fp32 quantity: the product's and the difference's roundings move it by <= u (|z_j| + |a_j|) =: u A_j, which
        is a RELATIVE error of e_j (the rounding of m itself shifts every argument alike and cancels); the same in S, weighted by p;
      * 5 roundings relative: expf to 1 ulp (2) in e_j and in the terms of S (2), the quotient (1);
      * S by the file's sum model, relative to S;
      * results below the smallest normal number may be subnormal or flushed: + 2^-126 absolute.
    Backward ds = scale p (dp - dot), dot = sum p dp by the sum model, then a difference and two products: 3 roundings of |ds|."""
    torch.manual_seed(n + rows)
    ld, scale = n + 4, 0.125
    s = torch.randn(rows, n) * 3
    for r in range(1, rows, 5):                                  # rows whose scale * s spans +-80
        s[r] = (torch.linspace(-80.0, 80.0, n) / scale)[torch.randperm(n)]
    s[3] = 1.7                                                   # a constant row
    dp = torch.randn(rows, n)
    sd, dpd = be.to(pitched(s, ld)), be.to(pitched(dp, ld))
    p, ds = nan_empty(be, rows, ld), nan_empty(be, rows, ld)
    po = twice(lambda: be.L.cdf_softmax_rows_fwd(P(sd), P(p), rows, n, ld, scale, be.stream()), [p])[0]
    assert pads_untouched(po, n)
    z = s.double() * f32(scale)
    a = z - z.max(1, keepdim=True).values
    e = a.exp()
    S = e.sum(1, keepdim=True)
    p_r = e / S
    A = z.abs() + a.abs()
    rel = U * (A + (p_r * A).sum(1, keepdim=True)) + 5 * U + K_SUM * U * math.sqrt(n) * e.pow(2).sum(1, keepdim=True).sqrt() / S
    check_elem(f"softmax_rows_fwd {rows}x{n}", po[:, :n], p_r, rel * p_r + TINY)
    assert bits_equal(po[3, :n], po[3, :1].expand(n))            # the constant row: one value
    # backward from the kernel's own p (its pad columns are still NaN)
    p.copy_(po)
    dso = twice(lambda: be.L.cdf_softmax_rows_bwd(P(p), P(dpd), P(ds), rows, n, ld, scale, be.stream()), [ds])[0]
    assert pads_untouched(dso, n)                                # ops.softmax_rows_bwd zero-fills them itself and relies on that
    pk = po[:, :n].double()
    terms = pk * dp.double()
    dot = terms.sum(1, keepdim=True)
    ds_r = f32(scale) * pk * (dp.double() - dot)
    e_dot = K_SUM * U * math.sqrt(n) * terms.pow(2).sum(1, keepdim=True).sqrt()
    check_elem(f"softmax_rows_bwd {rows}x{n}", dso[:, :n], ds_r, f32(scale) * pk * e_dot + 3 * U * ds_r.abs() + TINY)


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. skinny linear layers: the 32-row form, several contraction chunks with a ragged last one
# ---------------------------------------------------------------------------------------------------------------------------------
def dot_bound(a, b, extra=None):
    """sum_bound of the products a[m, i] * b[i, j] over i (plus one more term `extra`[m, j] or [j]) without building the [m, i, j] tensor:
    ||terms||_2^2 of output (m, j) is (a^2 @ b^2)[m, j]."""
    sq = a.double().pow(2) @ b.double().pow(2)
    n = a.shape[1]
    if extra is not None:
        sq, n = sq + extra.double().pow(2), n + 1
    return K_SUM * U * math.sqrt(n) * math.sqrt(sq.max().item())


@pytest.mark.parametrize("M,K,N,rows32", [(64, 200, 4100, True), (130, 300, 1700, True), (33, 129, 4036, True), (256, 128, 1000, True),
                                          (64, 200, 4036 - 64, False)])          # (last: just on the 8-row side of the threshold)
def test_linear_small_production(be, M, K, N, rows32):
    torch.manual_seed(M + K + N)
    cdiv = lambda a, b: -(-a // b)
    x, w, bias, g = torch.randn(M, K), torch.randn(N, K) / math.sqrt(K), torch.randn(N), torch.randn(M, N)
    ldi, ldw, ldo = K + 4, N + 8, N + 4
    # which kernel form cdf_linear_small takes is restated here: a change of the threshold in the source must fail, not lose the coverage
    assert (cdiv(ldo, 64) * cdiv(M, 32) >= 128) == rows32
    wp = torch.full((K, ldw), float("nan"))                      # the packed [K][N] weight; its pad columns are never read
    wp[:, :N] = w.t()
    xd, wd, bd = be.to(pitched(x, ldi)), be.to(wp), be.to(bias)
    y = nan_empty(be, M, ldo)
    yo = twice(lambda: be.L.cdf_linear_small(P(xd), ldi, P(wd), ldw, P(bd), P(y), ldo, M, K, N, be.stream()), [y])[0]
    bound = dot_bound(x, w.t(), bias)
    t0 = x[0].double()[:, None] * w.t().double()
    assert sum_bound(t0, 0) <= bound                             # (dot_bound is sum_bound: here on the first output row)
    check(f"linear_small fwd M={M} K={K} N={N} rows32={rows32}", yo[:, :N], x.double() @ w.double().t() + bias.double(), bound)
    assert not yo[:, N:].any()                                   # columns J .. ldo - 1: exactly zero
    # data gradient: contraction over I = N (many 128-wide chunks, a ragged last one), the PyTorch [N][K] weight, no bias
    ldg, ldwk, ldk = N + 4, K + 4, K + 4
    gd, wkd = be.to(pitched(g, ldg)), be.to(pitched(w, ldwk))
    dx = nan_empty(be, M, ldk)
    dxo = twice(lambda: be.L.cdf_linear_small(P(gd), ldg, P(wkd), ldwk, 0, P(dx), ldk, M, N, K, be.stream()), [dx])[0]
    form = "32" if cdiv(ldk, 64) * cdiv(M, 32) >= 128 else "8"
    check(f"linear_small dgrad M={M} I={N} J={K} ({form}-row form, {cdiv(N, 128)} chunks, last {N % 128 or 128})", dxo[:, :K],
          g.double() @ w.double(), dot_bound(g, w))
    assert not dxo[:, K:].any()
    # weight / bias gradients onto non-zero dW, db: the prior value is one more term of each sum
    dW0, db0 = torch.randn(N, K), torch.randn(N)
    dW, db = be.to(dW0), be.to(db0)
    dWo, dbo = twice_inplace(be, lambda: be.L.cdf_linear_small_wgrad(P(gd), ldg, P(xd), ldi, P(dW), P(db), M, N, K, be.stream()),
                             [dW, db], [dW0, db0])
    check(f"linear_small_wgrad dW M={M} N={N} K={K}", dWo, dW0.double() + g.double().t() @ x.double(), dot_bound(g.t(), x, dW0))
    check(f"linear_small_wgrad db M={M} N={N}", dbo, db0.double() + g.double().sum(0), dot_bound(g.t(), torch.ones(M, 1), db0[:, None]))


# ---------------------------------------------------------------------------------------------------------------------------------
# 9. the FID extractor's pooling and resize
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,k,s,p,H,W", [(0, 3, 2, 0, 67, 65), (1, 3, 1, 1, 33, 31)])
def test_pool2d_past_grid_cap(be, mode, k, s, p, H, W):
    """Max pooling is bit-equal to ATen; the average (count_include_pad=False) is within the existing 1e-6 of float64.  Each is written as a
    channel slice of a wider poisoned buffer."""
    torch.manual_seed(9 + mode)
    C = 8
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    B = -(-(PCAP + PAST) // (OH * OW * (C // 4)))
    assert B * OH * OW * (C // 4) > PCAP and (B * OH * OW * (C // 4)) % 256 != 0
    x = torch.randn(B, H, W, C)
    xd, wide = be.to(x), nan_empty(be, B, OH, OW, C + 4)
    got = twice(lambda: be.L.cdf_pool2d(P(xd), C, P(wide) + 16, C + 4, B, H, W, C, k, s, p, mode, be.stream()), [wide])[0]
    assert torch.isnan(got[..., :4]).all()
    xn = x.permute(0, 3, 1, 2)
    if mode == 0:
        assert bits_equal(got[..., 4:].contiguous(), F.max_pool2d(xn, k, s, p).permute(0, 2, 3, 1).contiguous())
    else:
        ref = F.avg_pool2d(xn.double(), k, s, p, count_include_pad=False).permute(0, 2, 3, 1)
        check(f"pool2d avg B={B} {H}x{W}", got[..., 4:], ref, 1e-6)


def test_resize_bilinear_fid_shape(be):
    """(16, 3, 128 x 128) -> 299 x 299, the launch of the FID path: 4,290,768 outputs, past PCAP.  The reference is ATen's own fp32
    F.interpolate, as in test_inception.py: the source index is DEFINED in fp32 (scale = in / out, src = scale (dst + 0.5) - 0.5), so a
    float64 interpolate is another function (indices up to 1e-5 apart).  Bound: the existing 2e-6.  It separates the two ways of rounding
    that index: ATen contracts it into one fused multiply-add; with the product rounded on its own the index near 127 is half an ulp
    (3.8e-6) off, which was 4.6e-6 here before the kernel took the fused form (1e-7 from a float64 lerp on either index; the small test's
    indices stay below 16, where the same slip is under 1e-6)."""
    torch.manual_seed(10)
    B, C, H, W, OH, OW = 16, 3, 128, 128, 299, 299
    assert B * C * OH * OW > PCAP
    img = torch.rand(B, C, H, W)
    imd, out = be.to(img), nan_empty(be, B, OH, OW, 4)
    o = twice(lambda: be.L.cdf_resize_bilinear_nhwc(P(imd), P(out), 4, B, C, H, W, OH, OW, 2.0, -1.0, be.stream()), [out])[0]
    ref = 2 * F.interpolate(img, size=(OH, OW), mode="bilinear", align_corners=False) - 1
    check("resize_bilinear_nhwc 16x3x128x128 -> 299x299", o[..., :C].permute(0, 3, 1, 2), ref, 2e-6)
    assert pads_untouched(o, C)


@pytest.mark.parametrize("HW", [63, 64])
def test_global_avgpool_ragged_channels(be, HW):
    """Four 64-channel groups, the last ragged (C = 200), pitched input with NaN pads: the sum model over HW, the division's rounding."""
    torch.manual_seed(HW)
    B, C, ldx, ldy = 3, 200, 208, 204
    x = torch.full((B, HW, ldx), float("nan"))
    x[..., :C] = torch.randn(B, HW, C)
    xd, y = be.to(x), nan_empty(be, B, ldy)
    yo = twice(lambda: be.L.cdf_global_avgpool(P(xd), ldx, P(y), ldy, B, HW, C, be.stream()), [y])[0]
    ref = x[..., :C].double().mean(1)
    check(f"global_avgpool HW={HW}", yo[:, :C], ref, sum_bound(x[..., :C].double(), 1) / HW + U * ref.abs().max().item())
    assert pads_untouched(yo, C)


# ---------------------------------------------------------------------------------------------------------------------------------
# 10. the norm layers' parameter-gradient reduction, called directly
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("C", [8, 64, 200])                     # C = 200: the dg / db split falls inside a 64-column block
def test_norm_param_reduce_block_counts(be, C, accumulate):
    """part[block][2][C] -> dg, db (+= with accumulate): every tail of the 128- / 32- / 16-block strides, the sum model over nblocks (the prior
    value one more term)."""
    torch.manual_seed(C + accumulate)
    for nb in (1, 15, 16, 17, 33, 127, 128, 129, 1024, 8197):
        part = torch.randn(nb, 2, C)
        prior = torch.randn(2, C)
        pd = be.to(part)
        dg, db = nan_empty(be, C), nan_empty(be, C)
        launch = lambda: be.L.cdf_norm_param_reduce(P(pd), nb, C, P(dg), P(db), accumulate, be.stream())
        if accumulate:
            dgo, dbo = twice_inplace(be, launch, [dg, db], [prior[0], prior[1]])
            terms = torch.cat((part, prior[None]), 0).double()
        else:
            dgo, dbo = twice(launch, [dg, db])
            terms = part.double()
        check(f"norm_param_reduce nblocks={nb} C={C} accumulate={accumulate}", torch.stack((dgo, dbo)), terms.sum(0), sum_bound(terms, 0))
