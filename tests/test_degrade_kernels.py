"""csrc/k_degrade.hip at the arguments and plane sizes the samplers use: step_lo > 0, identity rows, the single-step form, rectangular
planes, MNIST's 28 x 28 (4-wide strips), 128 x 128 planes (130-150 KB of dynamic LDS), planes at the 160 KB cap and just past it, the
global fallback path, and the elementwise kernels past their grid cap (more than 4096 x 256 elements).  Runs on both backends.

Reference: a float64 CPU restatement of the reference op chain (depthwise F.conv2d on an explicitly padded plane, F.interpolate,
sequential mask products).  The same chain restated in fp32 measures how far fp32 arithmetic itself is from float64 on the case's
inputs; the bound of every compared tensor is BOUND_K = 4 times that distance (the factor covers the different summation order of the
dense, separable and library kernels) -- it comes from the reference alone (one addition for results that are a single reduced
value: see check()).  Results whose association is fixed (identity rows, mask
products, noise / blend, the combine) are asserted with torch.equal.  An input whose fp32 restatement is further than 1e-5 from float64
is a bad input.

Every output is carved from one poisoned buffer between guard bands; every launch runs twice on freshly poisoned outputs and must be
bit-identical; after each launch the outputs are finite, the guard bands still NaN and the inputs unchanged.

Batch layout of the chains: B = 4, C = 2 or 3, T = 6 tap sets / masks, per-sample t = [T-1, lo, lo-1, max(lo, 3)] with lo = step_lo:
a full row, a single-step row, an identity row and a middle row in one launch.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from colddiff import degrade as D
from emu_util import P
from poison import Guarded, nan_empty
from test_kernels_production import bits_equal

BOUND_K = 4.0
BAD_INPUT = 1e-5
CDF_E_INVALID = -1
T = 6
RATIOS = {}           # kernel family -> largest (kernel error / fp32-restatement error) seen in this process


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    if RATIOS:
        print("\nlargest kernel error / fp32-restatement error per kernel family (bound: %.0f)" % BOUND_K)
        for fam in sorted(RATIOS):
            print("  %-28s %.3f" % (fam, RATIOS[fam]))


def _sync(be):
    if be.kind == "hip":
        torch.cuda.synchronize()


def check(family, name, got, r64, r32, few_values=False):
    """|got - float64| <= BOUND_K * max|fp32 restatement - float64|, both maxima over the compared tensor.

    few_values: the compared tensor is ONE reduction result (the loss) or one per plane (cdf_plane_mean), so that maximum is a handful of
    roundings and says little: torch's fp32 mean follows the host's thread count and vector width, and may land on the correctly rounded
    value (the l1 loss below sits 6.1e-8 from float64 with 16 threads and 1.8e-9 with 2, on the same inputs; the kernel's 5.8e-8 is 0.97 ulp).
    No fp32 output can be asked to be nearer than the format rounds, so there -- and only there -- the distance is taken as at least half
    an fp32 ulp of the reference value.  With thousands of compared values the largest restatement error is well above that anyway."""
    base = (r32.double() - r64).abs().max().item()
    assert base <= BAD_INPUT, ("bad input: the fp32 restatement itself is off", name, base)
    if few_values:
        mag = r64.float().abs()
        half_ulp = ((torch.nextafter(mag, torch.full_like(mag, math.inf)) - mag) / 2).max().item()
        print(f"{family}: {name}: fp32 restatement {base:.3e}, half an ulp of the value {half_ulp:.3e}")
        base = max(base, half_ulp)
    e = (got.double() - r64).abs().max().item()
    ratio = e / base if base > 0 else (0.0 if e == 0 else math.inf)
    RATIOS[family] = max(RATIOS.get(family, 0.0), ratio)
    print(f"{family}: {name}: error {e:.3e}, fp32 restatement {base:.3e}, ratio {ratio:.3f}")
    assert math.isfinite(e) and e <= BOUND_K * base, (family, name, e, base)


def run_twice(be, shape, n, launch, inputs):
    """launch(*outs) twice on n freshly poisoned outputs between guard bands -> the outputs (host copies)."""
    g = Guarded(be.device, shape, n)
    keep = [d.clone() for d in inputs]
    res = []
    for _ in range(2):
        g.poison()
        launch(*g.outs)
        _sync(be)
        assert g.guards_intact(), "a guard band was written"
        res.append([o.cpu().clone() for o in g.outs])
        for o in res[-1]:
            assert torch.isfinite(o).all(), "an output element was left unwritten"
        for d, k in zip(inputs, keep):
            assert torch.equal(d, k), "an input was written"
    for a, b in zip(*res):
        assert bits_equal(a, b), "second launch differs"
    return res[0]


def images(seed, *shape):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g) * 2 - 1


def row_steps(lo, last=T - 1):
    return [last, lo, lo - 1, min(max(lo, 3), last)]


def pick(states, x, lo, his):
    """states[s] = batch state after step s (s >= lo): per-row (state after step his[b], state before it); identity where his[b] < lo."""
    y = torch.stack([states[h][b] if h >= lo else x[b] for b, h in enumerate(his)])
    prev = torch.stack([(states[h - 1][b] if h - 1 >= lo else x[b]) for b, h in enumerate(his)])
    return y, prev


def quantise8(v):
    return ((v + 1) * 0.5 * 255).int().float() / 255 * 2 - 1


def same_or_one_level(got, ref):
    """8-bit truncation may flip one level (2/255) where the value differs in the last ulp."""
    d = (got - ref).abs()
    return bool((d <= 1e-6).logical_or((d - 2 / 255).abs() <= 1e-6).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. blur chains
# ---------------------------------------------------------------------------------------------------------------------------------
def pad_index(n, h, mode):
    i = torch.arange(-h, n + h)
    if mode == "circular":
        return i % n
    period = 2 * (n - 1)
    i = i % period
    return torch.where(i < n, i, period - i)


def blur_step_ref(z, taps_s, mode):
    """One depthwise conv of the reference (DEBLUR:351-361) on an explicitly padded plane, in z's dtype."""
    C, k = taps_s.shape[0], taps_s.shape[-1]
    zp = z[:, :, pad_index(z.shape[2], k // 2, mode)][:, :, :, pad_index(z.shape[3], k // 2, mode)]
    return F.conv2d(zp, taps_s.to(z.dtype).unsqueeze(1), groups=C)


def rank_one_taps(seed, C, k):
    """T x C kernels gy (x) gx with unrelated, asymmetric factors (a transposed or mirrored tap order shows), each summing to 1."""
    g = torch.Generator().manual_seed(seed)
    gy, gx = (torch.rand((T, C, k), generator=g, dtype=torch.float64) + 0.05 for _ in range(2))
    gy, gx = gy / gy.sum(-1, keepdim=True), gx / gx.sum(-1, keepdim=True)
    return (gy.unsqueeze(-1) * gx.unsqueeze(-2)).float()


_blur_cache = {}


def blur_case(H, W, k, mode, C):
    """Inputs of one case and its references (computed once, shared by the dense and the separable test, never modified)."""
    key = (H, W, k, mode, C)
    if key not in _blur_cache:
        seed = H * 1000 + W * 10 + k
        case = {"x": images(seed, 4, C, H, W), "img": images(seed + 1, 4, C, H, W), "taps": rank_one_taps(seed + 2, C, k), "ref": {}}
        case["taps1d"] = D.separable_taps(case["taps"])
        assert case["taps1d"] is not None and case["taps1d"].shape == (T, C, 2, k)
        _blur_cache[key] = case
    return _blur_cache[key]


def blur_states(case, mode, lo, collapse, dtype):
    """{s: state after step s} for s = lo..T-1 in dtype, the plane replaced by its mean after step `collapse`."""
    key = (lo, collapse, dtype)
    if key not in case["ref"]:
        z, states = case["x"].to(dtype), {}
        for s in range(lo, T):
            z = blur_step_ref(z, case["taps"][s], mode)
            if s == collapse:
                z = z.mean((2, 3), keepdim=True).expand_as(z).contiguous()
            states[s] = z
        case["ref"][key] = states
    return case["ref"][key]


BLUR_CASES = [  # H, W, k, pad, C, step_lo
    (28, 28, 11, "circular", 3, 0),          # MNIST: W % 8 != 0, the 4-wide strip form
    (32, 32, 3, "reflect", 2, 1),
    (16, 24, 11, "reflect", 3, 2),
    (24, 16, 15, "reflect", 2, 3),
    (8, 32, 15, "circular", 3, 0),
    (12, 20, 5, "circular", 2, 1),           # k = 5: the run-time-k instantiation
    (16, 16, 27, "circular", 3, 2),
    (128, 128, 15, "reflect", 2, 3),         # 147,456 B (dense) / 132,224 B (separable) of dynamic LDS
    (128, 128, 11, "circular", 2, 2),        # 142,944 B
    (128, 124, 5, "reflect", 2, 1),
    (8, 16, 27, "circular", 3, 3),           # dense only: the halo wraps more than once
    # H % 4 == 2: the separable kernel's one-row strip form at a compile-time k, inner and border strips in one row
    (10, 12, 3, "reflect", 2, 1),            # reach 4: the strip at x0 = 4 is inner, the others are border
    (18, 24, 11, "circular", 3, 0),          # reach 8: strips at x0 = 8, 12 are inner
    (14, 24, 15, "reflect", 2, 2),           # reach 8, k / 2 = 7 < 14
]


def blur_fn(be, kind):
    return be.L.cdf_blur_chain if kind == "dense" else be.L.cdf_blur_chain_sep


@pytest.mark.parametrize("kind,H,W,k,mode,C,lo", [(kind,) + c for kind in ("dense", "separable") for c in BLUR_CASES
                                                  if kind == "dense" or c[2] // 2 < min(c[0], c[1])])
def test_blur_chain_arguments(be, kind, H, W, k, mode, C, lo):
    case = blur_case(H, W, k, mode, C)
    B, pm, fam = 4, D.PAD_MODES[mode], "blur " + kind
    x, img = case["x"], case["img"]
    his = row_steps(lo)
    xd, imgd, td = be.to(x), be.to(img), be.to(torch.tensor(his, dtype=torch.int64))
    tapsd = be.to(case["taps"] if kind == "dense" else case["taps1d"])
    fn, S, shape = blur_fn(be, kind), be.stream(), (B, C, H, W)
    tag = f"{H}x{W} k={k} {mode} lo={lo}"

    def call(y, snap, im, t, hi, collapse, quant, src=xd):
        fn(P(src), P(y), P(snap), P(im), P(tapsd), P(t), B, C, H, W, k, lo, hi, pm, collapse, quant, S)

    ref64, ref32 = (pick(blur_states(case, mode, lo, -1, dt), x.to(dt), lo, his) for dt in (torch.float64, torch.float32))
    # y and snap
    y, snap = run_twice(be, shape, 2, lambda y, s: call(y, s, None, td, 0, -1, 0), [xd, tapsd, td])
    check(fam, tag + " y", y, ref64[0], ref32[0])
    check(fam, tag + " snap", snap, ref64[1], ref32[1])
    assert torch.equal(y[2], x[2]) and torch.equal(snap[2], x[2]), "identity row"
    assert torch.equal(snap[1], x[1]), "single-step row: the state before its step is the input"
    # Algorithm 2, without and with snap
    alg64, alg32 = ((img.to(r[0].dtype) - r[0]) + r[1] for r in (ref64, ref32))
    (y2,) = run_twice(be, shape, 1, lambda y: call(y, None, imgd, td, 0, -1, 0), [xd, imgd, tapsd, td])
    check(fam, tag + " Alg. 2", y2, alg64, alg32)
    y3, snap3 = run_twice(be, shape, 2, lambda y, s: call(y, s, imgd, td, 0, -1, 0), [xd, imgd, tapsd, td])
    assert torch.equal(y3, y2) and torch.equal(snap3, snap), "Alg. 2 with snap"
    assert torch.equal(y2, (img - y) + snap), "the combine is (img - D_t) + D_{t-1} in this association"
    # collapse after step lo + 1 under per-sample t: rows below, at and above it over the cases
    c64, c32 = (pick(blur_states(case, mode, lo, lo + 1, dt), x.to(dt), lo, his) for dt in (torch.float64, torch.float32))
    yc, sc = run_twice(be, shape, 2, lambda y, s: call(y, s, None, td, 0, lo + 1, 0), [xd, tapsd, td])
    check(fam, tag + " collapse y", yc, c64[0], c32[0])
    check(fam, tag + " collapse snap", sc, c64[1], c32[1])
    # quantise on the collapsed result: same or one 8-bit level
    (yq,) = run_twice(be, shape, 1, lambda y: call(y, None, None, td, 0, lo + 1, 1), [xd, tapsd, td])
    assert same_or_one_level(yq, quantise8(c64[0].float()))
    assert torch.equal(yq[2], quantise8(x[2])), "identity row, quantised"
    # collapse at a row's last step (row 0), with snap
    l64, l32 = (pick(blur_states(case, mode, lo, T - 1, dt), x.to(dt), lo, his) for dt in (torch.float64, torch.float32))
    yl, sl = run_twice(be, shape, 2, lambda y, s: call(y, s, None, td, 0, T - 1, 0), [xd, tapsd, td])
    check(fam, tag + " collapse at the last step y", yl, l64[0], l32[0])
    assert bool((yl[0] == yl[0][:, :1, :1]).all()), "the collapsed row is constant per plane"
    assert torch.equal(sl, snap) and torch.equal(yl[1:], y[1:]), "rows and snapshots before the collapse are untouched by it"
    # scalar step_hi = step_lo - 1, no t: the input, bit for bit
    yi, si = run_twice(be, shape, 2, lambda y, s: call(y, s, None, None, lo - 1, -1, 0), [xd, tapsd])
    assert torch.equal(yi, x) and torch.equal(si, x), "step_hi < step_lo is the identity"
    # y aliasing x (not the Alg. 2 form)
    xa, snap_a = be.to(x), nan_empty(be, *shape)
    call(xa, snap_a, None, td, 0, -1, 0, src=xa)
    _sync(be)
    assert torch.equal(xa.cpu(), y) and torch.equal(snap_a.cpu(), snap), "y aliasing x"


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the LDS cap: the largest planes that fit launch and are right; the next ones are refused and nothing is written
# ---------------------------------------------------------------------------------------------------------------------------------
CAP = 160 * 1024


def pixelate_lds_bytes(H):
    return (2 * H * H + 9 * H) * 4            # cdf_pixelate_chain: U, D, three per-axis tables


@pytest.mark.parametrize("kind,H,W,k,mode,nbytes", [("dense", 136, 144, 3, "reflect", 160160), ("separable", 140, 144, 15, "reflect", 162432)])
def test_blur_chain_at_the_lds_cap(be, kind, H, W, k, mode, nbytes):
    got = be.L.cdf_blur_lds_bytes(H, W, k) if kind == "dense" else be.L.cdf_blur_sep_lds_bytes(H, W)
    assert got == nbytes and 155 * 1024 < nbytes <= CAP
    C, lo, B = 2, 1, 4
    case = blur_case(H, W, k, mode, C)
    x, his = case["x"], row_steps(lo)
    xd, td = be.to(x), be.to(torch.tensor(his, dtype=torch.int64))
    tapsd = be.to(case["taps"] if kind == "dense" else case["taps1d"])
    ref64, ref32 = (pick(blur_states(case, mode, lo, -1, dt), x.to(dt), lo, his) for dt in (torch.float64, torch.float32))
    y, snap = run_twice(be, (B, C, H, W), 2, lambda y, s: blur_fn(be, kind)(P(xd), P(y), P(s), 0, P(tapsd), P(td), B, C, H, W, k, lo, 0,
                                                                            D.PAD_MODES[mode], -1, 0, be.stream()), [xd, tapsd, td])
    check("blur " + kind, f"{H}x{W} k={k} ({nbytes} B of LDS) y", y, ref64[0], ref32[0])
    check("blur " + kind, f"{H}x{W} k={k} ({nbytes} B of LDS) snap", snap, ref64[1], ref32[1])
    assert torch.equal(y[2], x[2])


def refused(be, name, args, outs, plane):
    """The raw entry point returns CDF_E_INVALID, the error text names the plane, the poisoned outputs stay untouched."""
    rc = getattr(be.L._dll, name)(*args)
    _sync(be)
    assert rc == CDF_E_INVALID, (name, rc)
    assert plane.encode() in be.L.cdf_last_error(), be.L.cdf_last_error()
    for o in outs:
        assert bool(torch.isnan(o).all()), "a refused call wrote an output"


def test_planes_past_the_lds_cap_are_refused(be):
    B, C, S = 2, 2, be.stream()
    assert be.L.cdf_blur_lds_bytes(140, 144, 11) > CAP and be.L.cdf_blur_sep_lds_bytes(144, 144) > CAP and pixelate_lds_bytes(142) > CAP
    x = be.to(images(5, B, C, 144, 144))
    t = be.to(torch.tensor([1, 0], dtype=torch.int64))
    taps, taps1d = be.to(rank_one_taps(6, C, 11)), be.to(D.separable_taps(rank_one_taps(6, C, 11)))
    sizes = be.to(torch.tensor([71, 35, 17, 8, 4, 2], dtype=torch.int32))
    y, snap = nan_empty(be, B, C, 144, 144), nan_empty(be, B, C, 144, 144)
    refused(be, "cdf_blur_chain", (P(x), P(y), P(snap), 0, P(taps), P(t), B, C, 140, 144, 11, 0, 0, 1, -1, 0, S), (y, snap), "140x144")
    refused(be, "cdf_blur_chain_sep", (P(x), P(y), P(snap), 0, P(taps1d), P(t), B, C, 144, 144, 11, 0, 0, 1, -1, 0, S), (y, snap), "144x144")
    refused(be, "cdf_pixelate_chain", (P(x), P(y), P(snap), 0, P(sizes), P(t), B, C, 142, 0, 0, 0, S), (y, snap), "142x142")


@pytest.mark.parametrize("H,W,k", [(136, 144, 3), (140, 144, 3), (140, 144, 11), (128, 128, 15), (128, 128, 27), (16, 18, 3)])
def test_python_predicate_agrees_with_the_library(be, H, W, k):
    """degrade.blur_fits_lds (the dispatch of diffusion.py between the LDS-resident chain and the per-step fallback) against the
    return code of cdf_blur_chain on both sides of the cap (the calls that fit run zero steps: step_hi < step_lo)."""
    from colddiff import runtime
    saved, runtime._lib_override = runtime._lib_override, (be.L if be.kind == "emu" else None)
    try:
        fits = D.blur_fits_lds(H, W, k)
    finally:
        runtime._lib_override = saved
    assert fits == (W % 4 == 0 and be.L.cdf_blur_lds_bytes(H, W, k) <= CAP)
    B, C = 1, 2
    x, taps = be.to(images(7, B, C, H, W)), be.to(rank_one_taps(8, C, k)[:1])
    y = nan_empty(be, B, C, H, W)
    rc = be.L._dll.cdf_blur_chain(P(x), P(y), 0, 0, P(taps), 0, B, C, H, W, k, 0, -1, 1, -1, 0, be.stream())
    _sync(be)
    assert (rc == 0) == fits and rc in (0, CDF_E_INVALID), (rc, fits)
    assert torch.equal(y, x) if fits else bool(torch.isnan(y).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the fallback path (cdf_blur_step per step, cdf_x0_step_down) equals the dense chain; cdf_plane_mean
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,k,mode,C", [(28, 28, 11, "circular", 3), (16, 24, 11, "reflect", 3), (128, 124, 5, "reflect", 2),
                                          (128, 128, 15, "reflect", 2)])
def test_fallback_path_equals_the_chain(be, H, W, k, mode, C):
    """Both sum fmaf(w[ky][kx], src, acc) over ky, kx ascending from zero: the same rounding, so the same bits."""
    case = blur_case(H, W, k, mode, C)
    B, lo, hi, pm, S, shape = 4, 2, 4, D.PAD_MODES[mode], be.stream(), (4, C, H, W)
    x, img = case["x"], case["img"]
    xd, imgd, tapsd = be.to(x), be.to(img), be.to(case["taps"])
    n = x.numel()

    def fallback(a, b, c, out):
        cur = xd
        for nxt, s in zip((a, b, c), range(lo, hi + 1)):
            be.L.cdf_blur_step(P(cur), P(nxt), P(tapsd[s]), B, C, H, W, k, pm, S)
            cur = nxt
        be.L.cdf_x0_step_down(P(imgd), P(c), P(b), P(out), n, S)

    _, d_tm1, d_t, comb = run_twice(be, shape, 4, fallback, [xd, imgd, tapsd])
    assert torch.equal(comb, (img - d_t) + d_tm1), "cdf_x0_step_down is (img - D_t) + D_{t-1} in this association"
    states64, states32 = (blur_states(case, mode, lo, -1, dt) for dt in (torch.float64, torch.float32))
    tag = f"{H}x{W} k={k} {mode}"
    check("blur step (fallback)", tag + " D_t", d_t, states64[hi], states32[hi])
    check("blur step (fallback)", tag + " D_t-1", d_tm1, states64[hi - 1], states32[hi - 1])
    y, snap = run_twice(be, shape, 2, lambda y, s: be.L.cdf_blur_chain(P(xd), P(y), P(s), 0, P(tapsd), 0, B, C, H, W, k, lo, hi, pm, -1, 0, S),
                        [xd, tapsd])
    assert torch.equal(y, d_t) and torch.equal(snap, d_tm1), "the chain and the per-step fallback differ"
    (y2,) = run_twice(be, shape, 1, lambda y: be.L.cdf_blur_chain(P(xd), P(y), 0, P(imgd), P(tapsd), 0, B, C, H, W, k, lo, hi, pm, -1, 0, S),
                      [xd, imgd, tapsd])
    assert torch.equal(y2, comb)


@pytest.mark.parametrize("planes,H,W", [(12, 28, 28), (9, 343, 341)])
def test_plane_mean(be, planes, H, W):
    x = images(H, planes, H * W)
    g = Guarded(be.device, (planes, H * W), 1)
    res = []
    for _ in range(2):
        g.poison()
        g.outs[0].copy_(x)
        be.L.cdf_plane_mean(P(g.outs[0]), planes, H * W, be.stream())
        _sync(be)
        assert g.guards_intact(), "a guard band was written"
        res.append(g.outs[0].cpu().clone())
    assert bits_equal(res[0], res[1]), "second launch differs"
    got = res[0]
    assert bool((got == got[:, :1]).all()), "every element of a plane equals its first"
    check("plane mean", f"{planes} x {H}x{W}", got[:, 0], x.double().mean(1), x.mean(1), few_values=True)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. mask chain: 10 x 14 planes inside a 25 x 31 mask table
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offsets", [True, False])
@pytest.mark.parametrize("lo", [0, 2])
def test_mask_chain_arguments(be, lo, offsets):
    B, C, H, W, MH, MW, S = 4, 3, 10, 14, 25, 31, be.stream()
    x, img = images(40 + lo, B, C, H, W), images(41 + lo, B, C, H, W)
    masks = torch.rand((T, MH, MW), generator=torch.Generator().manual_seed(42))
    his = row_steps(lo)
    oy, ox = ([0, 15, 7, 3], [17, 0, 9, 4]) if offsets else ([0] * B, [0] * B)
    xd, imgd, md, td = be.to(x), be.to(img), be.to(masks), be.to(torch.tensor(his, dtype=torch.int64))
    oyd, oxd = (be.to(torch.tensor(o, dtype=torch.int64)) if offsets else None for o in (oy, ox))
    inputs = [xd, imgd, md, td] + ([oyd, oxd] if offsets else [])
    states, z = {}, x
    for s in range(lo, T):                   # sequential products in fp32, as DEFADE:518 forms them
        z = torch.stack([masks[s, oy[b]:oy[b] + H, ox[b]:ox[b] + W] * z[b] for b in range(B)])
        states[s] = z
    ref, refp = pick(states, x, lo, his)

    def call(y, snap, im, t, hi, quant):
        be.L.cdf_mask_chain(P(xd), P(y), P(snap), P(im), P(md), P(t), P(oyd), P(oxd), B, C, H, W, MH, MW, lo, hi, quant, S)

    shape = (B, C, H, W)
    y, snap = run_twice(be, shape, 2, lambda y, s: call(y, s, None, td, 0, 0), inputs)
    assert torch.equal(y, ref) and torch.equal(snap, refp)
    (y1,) = run_twice(be, shape, 1, lambda y: call(y, None, None, td, 0, 0), inputs)
    assert torch.equal(y1, ref)
    y2, snap2 = run_twice(be, shape, 2, lambda y, s: call(y, s, imgd, td, 0, 0), inputs)
    assert torch.equal(y2, (img - ref) + refp) and torch.equal(snap2, refp), "Algorithm 2: (img - v) + prev"
    (yq,) = run_twice(be, shape, 1, lambda y: call(y, None, None, td, 0, 1), inputs)
    assert torch.equal(yq, quantise8(ref))
    # the scalar forms of the samplers: step_hi = times - 1 for every row, and times - 2 < step_lo meaning identity
    ys, ss = run_twice(be, shape, 2, lambda y, s: call(y, s, None, None, lo + 1, 0), inputs)
    assert torch.equal(ys, states[lo + 1]) and torch.equal(ss, states[lo])
    yi, si = run_twice(be, shape, 2, lambda y, s: call(y, s, None, None, lo - 1, 0), inputs)
    assert torch.equal(yi, x) and torch.equal(si, x)


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. pixelate chain
# ---------------------------------------------------------------------------------------------------------------------------------
def pixelate_states(x, sizes, mode, lo, dtype):
    z, H, states = x.to(dtype), x.shape[-1], {}
    for s in range(lo, len(sizes)):
        z = F.interpolate(F.interpolate(z, size=sizes[s], mode=mode, antialias=False), size=H, mode="nearest-exact")
        states[s] = z
    return states


def pixelate_checks(be, x, img, sizes, mode, C, los):
    B, H, S, nsteps = 4, x.shape[-1], be.stream(), len(sizes)
    shape, mi = (B, C, H, H), D.PIX_MODES[mode]
    xd, imgd, szd = be.to(x), be.to(img), be.to(torch.tensor(sizes, dtype=torch.int32))

    def call(y, snap, im, t, lo, hi):
        be.L.cdf_pixelate_chain(P(xd), P(y), P(snap), P(im), P(szd), P(t), B, C, H, lo, hi, mi, S)

    for lo in los:
        his = row_steps(lo, nsteps - 1)
        td = be.to(torch.tensor(his, dtype=torch.int64))
        ref64, ref32 = (pick(pixelate_states(x, sizes, mode, lo, dt), x.to(dt), lo, his) for dt in (torch.float64, torch.float32))
        tag = f"{H} -> {sizes} {mode} lo={lo}"
        y, snap = run_twice(be, shape, 2, lambda y, s: call(y, s, None, td, lo, 0), [xd, szd, td])
        check("pixelate", tag + " y", y, ref64[0], ref32[0])
        check("pixelate", tag + " snap", snap, ref64[1], ref32[1])
        assert torch.equal(y[2], x[2]) and torch.equal(snap[2], x[2]) and torch.equal(snap[1], x[1]), "identity row / first-step snapshot"
        (y1,) = run_twice(be, shape, 1, lambda y: call(y, None, None, td, lo, 0), [xd, szd, td])
        assert torch.equal(y1, y)
        y2, snap2 = run_twice(be, shape, 2, lambda y, s: call(y, s, imgd, td, lo, 0), [xd, imgd, szd, td])
        alg64, alg32 = ((img.to(r[0].dtype) - r[0]) + r[1] for r in (ref64, ref32))
        check("pixelate", tag + " Alg. 2", y2, alg64, alg32)
        assert torch.equal(snap2, snap) and torch.equal(y2, (img - y) + snap)
        yi, si = run_twice(be, shape, 2, lambda y, s: call(y, s, None, None, lo, lo - 1), [xd, szd])
        assert torch.equal(yi, x) and torch.equal(si, x), "step_hi < step_lo is the identity"
    for i in range(nsteps):                  # the single-step form of the sampler: step_lo = step_hi = i
        one64, one32 = (pixelate_states(x, sizes[:i + 1], mode, i, dt)[i] for dt in (torch.float64, torch.float32))
        y, snap = run_twice(be, shape, 2, lambda y, s: call(y, s, None, None, i, i), [xd, szd])
        check("pixelate", f"{H} -> {sizes[i]} {mode} single step", y, one64, one32)
        assert torch.equal(snap, x)


@pytest.mark.parametrize("mode", ["area", "bilinear", "bicubic"])
@pytest.mark.parametrize("H,sizes,C", [(16, [8, 4, 2, 1], 3), (20, [20, 19, 13, 7, 3], 2), (12, [11, 5, 1], 3),
                                       (128, [64, 32, 16, 8], 2)])          # 128: the AFHQ factor-2 routine, about 136 KB of LDS
def test_pixelate_chain_arguments(be, H, sizes, C, mode):
    pixelate_checks(be, images(50 + H, 4, C, H, H), images(51 + H, 4, C, H, H), sizes, mode, C, (0, 1))


@pytest.mark.parametrize("mode", ["area", "bilinear", "bicubic"])
def test_pixelate_chain_at_the_lds_cap(be, mode):
    H = 140
    assert pixelate_lds_bytes(H) == 161840 and 155 * 1024 < pixelate_lds_bytes(H) <= CAP
    # sizes that divide 140: the fp32 scale factor H / S of the bilinear / bicubic source index is exact, so no case is a bad input
    # (140 -> 17 moves the fp32 restatement itself 1.2e-5 away from float64)
    pixelate_checks(be, images(60, 4, 2, H, H), images(61, 4, 2, H, H), [70, 35, 28, 20, 14, 7], mode, 2, (1,))


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. elementwise kernels past the grid cap: 1,052,667 elements -- more than 4096 x 256 (a second loop iteration for some threads
#    only), not a multiple of 256
# ---------------------------------------------------------------------------------------------------------------------------------
EW = (3, 3, 343, 341)


@pytest.fixture(scope="module")
def ew():
    B, C, H, W = EW
    assert B * C * H * W == 1052667 > 4096 * 256 and (B * C * H * W) % 256
    g = torch.Generator().manual_seed(70)
    d = {name: images(71 + i, *EW) for i, name in enumerate(("img", "x1", "x2", "eps"))}
    d["ca"], d["cb"] = (torch.rand(10, generator=g) * 0.7 + 0.3 for _ in range(2))
    d["al"] = torch.rand((T, H * W), generator=g)
    d["om"] = 1 - d["al"]
    return d


def test_noise_kernels_past_the_grid_cap(be, ew):
    B, C, H, W = EW
    S, n = be.stream(), B * C * H * W
    img, x1, eps, ca, cb = (ew[k] for k in ("img", "x1", "eps", "ca", "cb"))
    t = torch.tensor([9, 0, 4])
    imgd, x1d, epsd, cad, cbd, td = (be.to(v) for v in (img, x1, eps, ca, cb, t))
    (q,) = run_twice(be, EW, 1, lambda o: be.L.cdf_noise_qsample(P(x1d), P(epsd), P(cad), P(cbd), P(td), P(o), B, C * H * W, S),
                     [x1d, epsd, cad, cbd, td])
    assert torch.equal(q, ca[t].view(-1, 1, 1, 1) * x1 + cb[t].view(-1, 1, 1, 1) * eps)

    def step_ref(tt, est, dt):
        im, xa, no, a, b = (v.to(dt) for v in (img, x1, eps, ca, cb))
        x2 = (im - a[tt - 1] * xa) / b[tt - 1] if est else no
        xt = a[tt - 1] * xa + b[tt - 1] * x2
        xs = a[tt - 2] * xa + b[tt - 2] * x2 if tt - 1 != 0 else xa
        return (im - xt) + xs

    for tt in (1, 5):
        for est in (0, 1):
            (o,) = run_twice(be, EW, 1, lambda o: be.L.cdf_noise_step(P(imgd), P(x1d), P(epsd), P(cad), P(cbd), tt, est, P(o), n, S),
                             [imgd, x1d, epsd, cad, cbd])
            if est:
                check("noise step, estimated noise", f"t={tt}", o, step_ref(tt, est, torch.float64), step_ref(tt, est, torch.float32))
            else:
                assert torch.equal(o, step_ref(tt, est, torch.float32)), tt


def test_blend_and_combine_past_the_grid_cap(be, ew):
    B, C, H, W = EW
    S, n = be.stream(), B * C * H * W
    img, x1, x2, al, om = (ew[k] for k in ("img", "x1", "x2", "al", "om"))
    t = torch.tensor([T - 1, 0, 3])
    imgd, x1d, x2d, ald, omd, td = (be.to(v) for v in (img, x1, x2, al, om, t))
    (q,) = run_twice(be, EW, 1, lambda o: be.L.cdf_blend_qsample(P(x1d), P(x2d), P(ald), P(omd), P(td), P(o), B, C, H * W, S),
                     [x1d, x2d, ald, omd, td])
    assert torch.equal(q, al[t].view(B, 1, H, W) * x1 + om[t].view(B, 1, H, W) * x2)
    for tt in (1, 5):
        (o,) = run_twice(be, EW, 1, lambda o: be.L.cdf_blend_step(P(imgd), P(x1d), P(x2d), P(ald), P(omd), tt, P(o), H * W, n, S),
                         [imgd, x1d, x2d, ald, omd])
        a1, o1 = al[tt - 1].view(1, 1, H, W), om[tt - 1].view(1, 1, H, W)
        xs = al[tt - 2].view(1, 1, H, W) * x1 + om[tt - 2].view(1, 1, H, W) * x2 if tt - 1 != 0 else x1
        assert torch.equal(o, (img - (a1 * x1 + o1 * x2)) + xs), tt
    (o,) = run_twice(be, EW, 1, lambda o: be.L.cdf_x0_step_down(P(imgd), P(x1d), P(x2d), P(o), n, S), [imgd, x1d, x2d])
    assert torch.equal(o, (img - x1) + x2)


def test_mask_chain_past_the_grid_cap(be, ew):
    B, C, H, W = EW
    MH, MW, lo, S = H + 12, W + 9, 1, be.stream()
    x = ew["img"]
    masks = torch.rand((T, MH, MW), generator=torch.Generator().manual_seed(80))
    his, oy, ox = [T - 1, lo, lo - 1], [12, 0, 5], [0, 9, 4]
    xd, md = be.to(x), be.to(masks)
    td, oyd, oxd = (be.to(torch.tensor(v, dtype=torch.int64)) for v in (his, oy, ox))
    states, z = {}, x
    for s in range(lo, T):
        z = torch.stack([masks[s, oy[b]:oy[b] + H, ox[b]:ox[b] + W] * z[b] for b in range(B)])
        states[s] = z
    ref, refp = pick(states, x, lo, his)
    y, snap = run_twice(be, EW, 2, lambda y, s: be.L.cdf_mask_chain(P(xd), P(y), P(s), 0, P(md), P(td), P(oyd), P(oxd), B, C, H, W, MH, MW,
                                                                     lo, 0, 0, S), [xd, md, td, oyd, oxd])
    assert torch.equal(y, ref) and torch.equal(snap, refp)


@pytest.mark.parametrize("l2", [0, 1])
def test_loss_past_the_grid_cap(be, ew, l2):
    S, n = be.stream(), ew["img"].numel()
    a, b, gout = ew["img"], ew["x1"], torch.tensor([0.5])
    ad, bd, gd = be.to(a), be.to(b), be.to(gout)
    res = []
    for _ in range(2):
        out, part = nan_empty(be, 1), nan_empty(be, 1024)
        be.L.cdf_loss_fwd(P(ad), P(bd), P(out), P(part), n, l2, S)
        _sync(be)
        res.append((out.cpu().clone(), part.cpu().clone()))
        assert torch.isfinite(res[-1][0]).all() and torch.isfinite(res[-1][1]).all(), "all 1024 partial sums are written at this size"
    assert bits_equal(res[0][0], res[1][0]) and bits_equal(res[0][1], res[1][1]), "second launch differs"
    (gy,) = run_twice(be, EW, 1, lambda o: be.L.cdf_loss_bwd(P(ad), P(bd), P(gd), P(o), n, l2, S), [ad, bd, gd])

    def ref(dt):
        bb = b.to(dt).clone().requires_grad_()
        val = F.mse_loss(a.to(dt), bb) if l2 else (a.to(dt) - bb).abs().mean()
        (val * gout.to(dt)[0]).backward()
        return val.detach().reshape(1), bb.grad

    (v64, g64), (v32, g32) = ref(torch.float64), ref(torch.float32)
    name = "l2" if l2 else "l1"
    check("loss value", name, res[0][0], v64, v32, few_values=True)
    check("loss gradient", name, gy, g64, g32)
