"""The side kernels between the GEMMs, first half -- csrc/k_conv_cin4.hip (the image-side direct convolutions: forward, data gradient, the
second stage of the two-stage data gradient, weight gradient) and csrc/k_reduce.hip (slab reductions, column sums) -- in every argument
form the product launches; test_side_kernel_forms_attn.py holds linear attention and the row softmax the same way.  Conventions of
test_norm_dw_forms.py / test_gemm_sp_forms.py: a form is a pure function of a call's argument tuple (no pointer values, only which
pointers are null); every row of a case table builds its tuple through one helper and the case asserts that the launch has the form the
table claims; every output and workspace is NaN-poisoned before each of two launches that must agree bit for bit; float64 CPU references;
every worst error / bound is printed.  test_gpu_invariance.py::test_coverage_guard holds the recorded calls of the bench step (both
modes), the sampler step and config 2's pass against the tables; test_recorded_side_forms_dry makes the same recordings, and those of two
small networks in bf16x3 / bf16 / f32, without a GPU.

What the older tests of these kernels (test_kernels.py, test_kernels_production.py) never pass and the product does: a forward launch
without y (planes only, with or without lo), without planes, without pre; a dy pitch above Cout; `accumulate` onto non-zero contents; a
rectangular image; the k = 1, W % 4 == 0 weight-gradient kernel on the simulator; an empty trailing chunk (B = 2, 129 x 260: 131 chunks of
516 pixels, the 131st empty -- and 728 x 728, where the 1024th of the capped chunks is empty: the bench's 64 images of 128 x 128 divide
evenly, most other sizes past the cap do not); the slab reduction on the attention path's strides ((CA ldw, ldw, 1) with T = B,
(32, 1, HD) with T = heads, (0, dim, 1), (0, 0, 1) on nsplit = B ns bias rows), accumulating onto live gradients, and with R = 3 below
RJ = 4 in the tiled <9, 4> kernel.

Inputs: pad columns of every pitched input (dy, the packed weights, the z rows, the slabs and bias partials) are NaN; x is [B,H,W,4] with
the channels >= Cin zero (the product's layout).  Pad columns of pitched outputs, elements of a parameter the strides do not address and
the stand-in buffers of null outputs must still hold the poison (accumulate: their earlier contents, bit for bit) afterwards.

References (float64, CPU): F.conv2d / F.conv_transpose2d / torch.nn.grad.conv2d_weight, the nine shifted sums of test_conv_cin4_first_block,
plain sums.  Planes, bit for bit: a launch with any subset of (y, pre, hi, lo) writes what the launch with all four wrote (so: a launch
without y writes the planes of the launch with y, hi-only is the hi plane of the two-plane launch), and the planes are cdf_split_bf16 of
the fp32 y.

Bounds, no new constant (test_kernels_production.py::test_conv_cin4_first_block's and sum_bound):
  cin4 fwd    pre, y: min(2e-5, K_SUM 2^-24 sqrt(k^2 Cin) 2 (|x|max |w|max sqrt(k^2 Cin) + |bias|max))
  cin4 dgrad  dx: min(K_SUM 2^-24 Cout k^2 |dy|max |w|max, 5e-5 max(1, |ref|max)); channels >= Cin exact zeros (accumulate: unchanged)
  tapsum3     dx: K_SUM 2^-24 3 2 |z|max
  cin4 wgrad  dw: min(K_SUM 2^-24 sqrt(M) |x|max max||dy||_2, 5e-5 max(1, |ref|max)); db: min(sum_bound, 5e-5 max(1, |ref|max)); an empty
              chunk's slab and bsum row exact zeros
  unpack, colsum: sum_bound
  accumulate  the expected value is old + grad, the bound grows by one rounding 2^-24 |old + grad|max
Rejection (host-side check, nothing launches, both backends): cdf_conv_cin4_tapsum3 with ldz = 52 -- 67,392 B of dynamic LDS through a plain
launch, past the 64 KB such a launch gets; the check said <= 64 before this module and says <= 48 (62,208 B) now.

Cases: cin4 fwd 67, dgrad 29, tapsum3 17 (+ the rejection), wgrad 31, unpack_reduce 111, colsum 21; with the table and dry tests 279 on the
simulator (42 s in one process) and 277 on the MI355X (5 s); with test_side_kernel_forms_attn.py 444 / 440 (87 s / 7 s).
GPU-only: 1 row, the (CA ldw, ldw, 1) reduction at the recorded (16, 64, 128, 128) -- 16 slabs of 1M floats, about 6 s on the simulator; the
same strides run there at (16, 64, 64, 64) and (4, 64, 128, 128).  The rows past the grid cap (130 x 127 x 256 channels, 182 x 182 x 128,
257 x 257 x 64) and the capped weight-gradient rows (768 x 768, 728 x 728, Cout = 8) take 3 to 5 s each on the simulator.
Worst error / bound per output, simulator | MI355X:
    (equal to two digits on both backends: these kernels are plain fp32 loops without matrix cores, the simulator follows them operation
    for operation)
    cin4 fwd      pre 0.20   y 0.20            cin4 dgrad   dx 0.12           tapsum3   dx 0.22
    cin4 wgrad    dw 0.12    db 0.14           unpack       g 0.29  bias 0.32         colsum    out 0.12
Reached forms: REACHED / SMALL_NETWORKS below (cin4 fwd 3 + 2, dgrad 0 + 1, tapsum3 1, wgrad 2 + 2, unpack 17 + 13, colsum 6 + 3).
Seeded faults (simulator only, on a scratch copy; each changes values, never an address outside a buffer), all caught by these two modules;
of the older tests (test_kernels.py, test_kernels_production.py, test_modules.py) the ones that failed too are named:
    a cin4 forward stores pre only when y is non-null               11 forward rows (planes-only with pre); older: 1 module-level test
                                                                    (test_gradient_planes_ride_on_the_gradient_tensors), no kernel-level test
    b cin4 forward writes hi's values into lo when y is null        10 forward rows; older: not run against this fault
    c (m / W) % H written as (m / H) % W in the weight gradient     22 weight-gradient rows (H != W, k = 3); older: none (231 passed)
    d unpack_reduce_kernel<4> ignores `accumulate`                  25 unpack rows + 15 weight-gradient rows (their reduction); older:
                                                                    test_unpack_reduce (4), test_unpack_reduce_tiled (15: its SL4 comparisons),
                                                                    6 module-level tests
    e unpack_tile_body uses s_r for s_t (where that stays inside)   34 unpack rows + 7 weight-gradient rows; older: 67 tests, among them
                                                                    test_unpack_reduce_tiled (12), test_unpack_reduce_bench_slab_counts (1) and
                                                                    every GEMM test that reduces slabs
    f linattn_ctx1p_kernel reads v one HD further when koff = 0     13 context rows (every one-pass (k|v) row); older: test_linattn_context_one_pass
                                                                    (2) and 19 module-level tests
    g the finalize kernel's maximum loop starts at sl + 32          25 context + 8 finalize + 17 kvctx rows; older: not run against this fault
"""
import math
from typing import NamedTuple

import pytest
import torch
import torch.nn.functional as F

from poison import BF16_NAN_BITS, nan_empty
from test_kernels import P, _split, r4
from test_kernels_production import K_SUM, U, bits_equal, check, skip_emu, sum_bound, twice

NAN32 = torch.tensor(float("nan")).view(torch.int32).item()  # the poison bit pattern of tests/poison.py
NAN = float("nan")
cdiv = lambda a, b: -(-a // b)


def _null(v):
    return not int(getattr(v, "value", v) or 0)


def _letters(names, flags):
    return "".join(c for c, f in zip(names, flags) if f)


# ---------------------------------------------------------------------------------------------------------------------------------
# forms: pure functions of (entry point, argument tuple)
# ---------------------------------------------------------------------------------------------------------------------------------
def _grid_capped(M, Cout):
    """The forward / data-gradient grid ceil(M / (256 / LP)) is past its cap of 4096 blocks: the blocks walk a second round of pixels."""
    return int(cdiv(M, 256 // (Cout // 4)) > 4096)


def cin4_fwd_form(name, a):
    """cdf_conv_cin4_fwd: (k; act; present outputs of y p(re) h(i) l(o); bias present; operands of y p s (planes) w whose pitch exceeds Cout;
    LP = Cout / 4 lanes per pixel; grid capped at 4096 blocks; H != W)."""
    ldw, bias, y, ldy, pre, ldp, hi, lo, lds, B, H, W, Cout, k, act = a[2:17]
    on = (not _null(y), not _null(pre), not _null(hi), True)
    return (k, act, _letters("yphl", on[:3] + (not _null(hi) and not _null(lo),)), int(not _null(bias)),
            _letters("ypsw", (o and ld > Cout for o, ld in zip(on, (ldy, ldp, lds, ldw)))), Cout // 4, _grid_capped(B * H * W, Cout), int(H != W))


def cin4_dgrad_form(name, a):
    """cdf_conv_cin4_dgrad: (k; accumulate; dy pitched; LP; grid capped at 4096 blocks; H != W)."""
    ldd, B, H, W, Cout, k, acc = a[1], a[5], a[6], a[7], a[8], a[9], a[10]
    return (k, int(acc), int(ldd > Cout), Cout // 4, _grid_capped(B * H * W, Cout), int(H != W))


def cin4_tapsum3_form(name, a):
    """cdf_conv_cin4_tapsum3: (Cin; accumulate; ldz 'r4' (9 Cin rounded up to 4) or 'wide'; a ragged last 16 x 16 tile along x; along y;
    H != W)."""
    ldz, H, W, Cin, acc = a[1], a[4], a[5], a[6], a[7]
    return (Cin, int(acc), "r4" if ldz == r4(9 * Cin) else "wide", int(W % 16 != 0), int(H % 16 != 0), int(H != W))


def cin4_chunks(M, W):
    """(chunk count, pixels per chunk) of cdf_conv_cin4_wgrad: cdf_conv_cin4_nchunk and the launcher's rounding to groups of PX pixels."""
    nch = min(1024, max(1, M // 512))
    px = 4 if W % 4 == 0 else 1
    return nch, cdiv(cdiv(M, nch), px) * px


def cin4_wgrad_form(name, a):
    """cdf_conv_cin4_wgrad: (k; PX pixels per group, 4 when W % 4 == 0; Cin; bsum present; dy pitched; chunk count '1' / 'many' / 'capped'
    (1024); an empty trailing chunk; H != W)."""
    ldd, bsum, B, H, W, Cin, Cout, k = a[2], a[4], a[5], a[6], a[7], a[8], a[9], a[10]
    M = B * H * W
    nch, mpc = cin4_chunks(M, W)
    return (k, 4 if W % 4 == 0 else 1, Cin, int(not _null(bsum)), int(ldd > Cout), "1" if nch == 1 else ("capped" if M // 512 >= 1024 else "many"),
            int((nch - 1) * mpc >= M), int(H != W))


def unpack_form(name, a):
    """cdf_unpack_reduce / _bias, launch_unpack_reduce's choice restated: (kernel 'tiled<9,4>' / 'tiled<16,2>' / 'tiled<1,32>' / 'SL16' /
    'SL4'; bias reduction fused; accumulate; strides 'c1' (s_c == 1) / 'conv' ((1, T, R T)) / 'other'; C % 32 != 0; R % RJ != 0 (tiled
    kernels only); slab count '<8' / '8-31' / '>=32' -- the tiled kernels have 8 slab lanes, the others 16 from 32 slabs and 4 below)."""
    ns, T, R, C, ldc, s_t, s_r, s_c = a[2:10]
    bias = name == "cdf_unpack_reduce_bias"
    acc, tiled = (a[13], a[14]) if bias else (a[10], a[11])
    rj = 0
    if s_c != 1 and C >= 32 and T in (1, 9, 16) and tiled:
        rj = {9: 4, 16: 2, 1: 32}[T]
        kernel = "tiled<%d,%d>" % (T, rj)
        assert cdiv(C, 32) * cdiv(R, rj) < 1 << 30
    else:
        kernel = "SL16" if ns >= 32 else "SL4"
    strides = "c1" if s_c == 1 else ("conv" if (s_t, s_r, s_c) == (1, T, R * T) else "other")
    return (kernel, int(bias), int(acc), strides, int(C % 32 != 0), int(bool(rj) and R % rj != 0), "<8" if ns < 8 else ("8-31" if ns < 32 else ">=32"))


def colsum_chunks(rows):
    """(chunk count, rows per chunk) of cdf_colsum / _io."""
    nch = min(1024, max(1, rows // 512))
    return nch, cdiv(rows, nch)


def colsum_form(name, a):
    """cdf_colsum / _io: (x is bf16; accumulate; pitched i(nput) o(utput); chunk count '1' / 'many' / 'capped' (1024); an empty chunk;
    C % 64 != 0)."""
    rows, C, ld, ldo, acc = a[4:9]
    io = int(bool(a[9])) if name == "cdf_colsum_io" else 0
    nch, rpc = colsum_chunks(rows)
    return (io, int(acc), _letters("io", (ld > C, ldo > C)), "1" if nch == 1 else ("capped" if rows // 512 >= 1024 else "many"), int((nch - 1) * rpc >= rows),
            int(C % 64 != 0))


CIN4_FWD_NAMES = ("cdf_conv_cin4_fwd",)
CIN4_DGRAD_NAMES = ("cdf_conv_cin4_dgrad",)
CIN4_TAPSUM_NAMES = ("cdf_conv_cin4_tapsum3",)
CIN4_WGRAD_NAMES = ("cdf_conv_cin4_wgrad",)
UNPACK_NAMES = ("cdf_unpack_reduce", "cdf_unpack_reduce_bias")
COLSUM_NAMES = ("cdf_colsum", "cdf_colsum_io")


# ---------------------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------------------
def _pitched(t, ld):
    """t [..., C] in the first columns of a [..., ld] tensor of its dtype, NaN in the pad columns."""
    buf = torch.full(t.shape[:-1] + (ld,), NAN, dtype=t.dtype)
    buf[..., :t.shape[-1]] = t
    return buf


def _poisoned(t):
    """Every element of host tensor t (fp32, or int16 bf16 bits) still holds the poison bit pattern."""
    if t.dtype == torch.int16:
        return bool((t == BF16_NAN_BITS).all())
    return bool((t.view(torch.int32) == NAN32).all())


def _at(ad, key, on=True):
    return (ad[key] if ad else 1) if on else 0


def _chk(group, name, got, ref, bound):
    check(f"[{group}] {name}", got, ref, bound)


def _amax(t):
    return t.abs().max().item() if t.numel() else 0.0


# ---------------------------------------------------------------------------------------------------------------------------------
# cin4 forward
# ---------------------------------------------------------------------------------------------------------------------------------
class CF(NamedTuple):
    """outs: present outputs of y, p(re), h (hi plane), l (lo plane); ld*: pitches of y, pre, the planes, w (0: Cout)."""
    B: int
    H: int
    W: int
    Cin: int
    Cout: int
    k: int
    act: int = 1
    outs: str = "yphl"
    bias: int = 1
    ldy: int = 0
    ldp: int = 0
    lds: int = 0
    ldw: int = 0
    big: bool = False


def cf_call(r, ad=None, stream=0, outs=None):
    """(entry point, argument tuple) of a CF row the way ops.conv_cin4_fwd writes the call (the pitch of an absent pre / planes is 0)."""
    outs = r.outs if outs is None else outs
    C = r.Cout
    has = lambda c: c in outs
    return "cdf_conv_cin4_fwd", (_at(ad, "x"), _at(ad, "w"), r.ldw or C, _at(ad, "bias", r.bias), _at(ad, "y", has("y")), r.ldy or C, _at(ad, "pre", has("p")),
                                 (r.ldp or C) if has("p") else 0, _at(ad, "hi", has("h")), _at(ad, "lo", has("l")), (r.lds or C) if has("h") else 0,
                                 r.B, r.H, r.W, C, r.k, r.act, stream)


def _cin4_inputs(be, r, seed):
    """x [B,H,W,4] (channels >= Cin zero: the product's layout), the weight [Cout,Cin,k,k], bias, the weight packed [taps][4][ldw] with NaN
    pad columns, a generator for what else the case draws."""
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros(r.B, r.H, r.W, 4)
    x[..., :r.Cin] = torch.randn(r.B, r.H, r.W, r.Cin, generator=g)
    wt, bs = torch.randn(r.Cout, r.Cin, r.k, r.k, generator=g) / 2, torch.randn(r.Cout, generator=g)
    wp = nan_empty(be, r.k * r.k, 4, r.Cout)
    be.L.cdf_pack_cin4(P(be.to(wt)), P(wp), r.Cout, r.Cout, r.Cin, r.k, be.stream())
    if be.kind == "hip":
        torch.cuda.synchronize()
    ldw = getattr(r, "ldw", 0) or r.Cout
    return x, wt, bs, be.to(_pitched(wp.cpu(), ldw)), g


def _cf_case(be, r):
    skip_emu(be, r.big)
    B, H, W, Cin, Cout, k = r[:6]
    KK = k * k
    ldy, ldp, lds = r.ldy or Cout, r.ldp or Cout, r.lds or Cout
    tag = "cin4 fwd " + "-".join(map(str, r))
    x, wt, bs, wd, _ = _cin4_inputs(be, r, Cout * 31 + H * 7 + W + Cin)
    xd, bd = be.to(x), be.to(bs)

    def go(outs):
        y, pre = nan_empty(be, B, H, W, ldy), nan_empty(be, B, H, W, ldp)
        hi, lo = nan_empty(be, B, H, W, lds, dtype=torch.int16), nan_empty(be, B, H, W, lds, dtype=torch.int16)
        name, args = cf_call(r, dict(x=P(xd), w=P(wd), bias=P(bd), y=P(y), pre=P(pre), hi=P(hi), lo=P(lo)), be.stream(), outs)
        assert cin4_fwd_form(name, args) == cin4_fwd_form(*cf_call(r, outs=outs)), tag
        return twice(lambda: getattr(be.L, name)(*args), [y, pre, hi, lo])
    form = cin4_fwd_form(*cf_call(r))
    print(f"{tag}: form {form}")
    full = go("yphl")
    xs, wd64 = x[..., :Cin].permute(0, 3, 1, 2).double(), wt.double()
    pre_r = F.conv2d(xs, wd64, bs.double() if r.bias else None, padding=k // 2)
    y_r = (pre_r, F.gelu(pre_r), F.silu(pre_r))[r.act]
    tb = min(2e-5, K_SUM * U * math.sqrt(KK * Cin) * 2 * (_amax(xs) * _amax(wd64) * math.sqrt(KK * Cin) + (_amax(bs) if r.bias else 0.0)))
    _chk("cin4 fwd", f"{tag} pre", full[1][..., :Cout].permute(0, 3, 1, 2), pre_r, tb)
    _chk("cin4 fwd", f"{tag} y", full[0][..., :Cout].permute(0, 3, 1, 2), y_r, tb)
    rh, rl = _split(be, be.to(full[0][..., :Cout]).view(-1, Cout))
    assert torch.equal(full[2].view(-1, lds)[:, :Cout], rh.cpu()[:, :Cout]) and torch.equal(full[3].view(-1, lds)[:, :Cout], rl.cpu()[:, :Cout]), (tag, "planes are not cdf_split_bf16 of y")
    for t, what in zip(full, ("y", "pre", "hi", "lo")):
        assert _poisoned(t[..., Cout:]), (tag, "a pad column of %s changed" % what)
    if r.outs != "yphl":                                     # the row's own subset: what it writes is what the full launch wrote, bit for bit
        own = go(r.outs)
        for letter, got, want in zip("yphl", own, full):
            if letter in r.outs:
                assert bits_equal(got, want), (tag, letter, "differs from the launch with every output (pad columns included)")
            else:
                assert _poisoned(got), (tag, letter, "a null output's stand-in buffer changed")
    return form


_CF_SHAPES = ((5, 12), (12, 5), (7, 9), (9, 7))
_CF_COUT = (4, 8, 32, 128, 256)
_CF_OUTS = ("y", "yp", "yh", "yhl", "yph", "yphl", "h", "hl", "ph", "phl")     # every subset the argument check admits (y || y_hi; lo needs hi)


def _cf_rows():
    rows, i = [], 0
    for rnd in range(2):
        for outs in _CF_OUTS:
            for bias in (0, 1):
                H, W = _CF_SHAPES[(i + rnd) % 4]
                Cout = _CF_COUT[(i + 2 * rnd) % 5]
                pit = dict(ldy=Cout + 8, ldp=Cout + 8, lds=Cout + 8, ldw=Cout + 8) if (i + rnd) % 2 else {}
                rows.append(CF(2, H, W, 1 + (i + rnd) % 4, Cout, (1, 3)[(i // 2 + rnd) % 2], (1, 0, 2)[i % 3], outs, bias, **pit))
                i += 1
    # W in {9, 12} x k in {1, 3} at every LP, one pitch at a time
    for j, (W, k) in enumerate(((9, 1), (9, 3), (12, 1), (12, 3))):
        for n, Cout in enumerate(_CF_COUT):
            one = ("ldy", "ldp", "lds", "ldw")[(j + n) % 4]
            rows.append(CF(2, 5, W, 3, Cout, k, 1, "yphl", 1, **{one: Cout + 8}))
    # past the grid cap of 4096 blocks: B = 1, 130 x 127, Cout = 256 (16,510 pixels, 4 per block)
    rows += [CF(1, 130, 127, 3, 256, 3, 1, "phl", 1), CF(1, 130, 127, 3, 256, 1, 0, "y", 1, ldy=264)]
    return rows


CF_ROWS = _cf_rows()


# ---------------------------------------------------------------------------------------------------------------------------------
# cin4 data gradient (direct, and the second stage of the two-stage form)
# ---------------------------------------------------------------------------------------------------------------------------------
class CD(NamedTuple):
    B: int
    H: int
    W: int
    Cin: int
    Cout: int
    k: int
    acc: int = 0
    ldd: int = 0
    ldw: int = 0
    big: bool = False


def cd_call(r, ad=None, stream=0):
    return "cdf_conv_cin4_dgrad", (_at(ad, "dy"), r.ldd or r.Cout, _at(ad, "w"), r.ldw or r.Cout, _at(ad, "dx"), r.B, r.H, r.W, r.Cout, r.k, r.acc, stream)


def _cd_case(be, r):
    skip_emu(be, r.big)
    B, H, W, Cin, Cout, k = r[:6]
    KK = k * k
    tag = "cin4 dgrad " + "-".join(map(str, r))
    _, wt, _, wd, g = _cin4_inputs(be, r, Cout * 13 + H * 5 + W + Cin)
    dy, dx0 = torch.randn(B, H, W, Cout, generator=g), torch.randn(B, H, W, 4, generator=g)
    dyd, dx0d = be.to(_pitched(dy, r.ldd or Cout)), be.to(dx0)          # dy inside a wider NaN buffer
    dx = nan_empty(be, B, H, W, 4)
    name, args = cd_call(r, dict(dy=P(dyd), w=P(wd), dx=P(dx)), be.stream())
    form = cin4_dgrad_form(*cd_call(r))
    assert cin4_dgrad_form(name, args) == form, tag
    print(f"{tag}: form {form}")

    def launch():
        if r.acc:
            dx.copy_(dx0d)
        getattr(be.L, name)(*args)
    dxo = twice(launch, [dx])[0]
    gs, wd64 = dy.permute(0, 3, 1, 2).double(), wt.double()
    dx_r = F.conv_transpose2d(gs, wd64, padding=k // 2).permute(0, 2, 3, 1)
    db_ = K_SUM * U * math.sqrt(Cout * KK) * _amax(gs) * _amax(wd64) * math.sqrt(Cout * KK)
    bound = min(db_, 5e-5 * max(1.0, _amax(dx_r)))
    ref = torch.zeros(B, H, W, 4, dtype=torch.float64)
    ref[..., :Cin] = dx_r
    if r.acc:
        ref = ref + dx0.double()
        bound += U * _amax(ref)
    _chk("cin4 dgrad", f"{tag} dx", dxo[..., :Cin], ref[..., :Cin], bound)
    assert torch.equal(dxo[..., Cin:], dx0[..., Cin:] if r.acc else torch.zeros(B, H, W, 4 - Cin)), (tag, "channels >= Cin: exact zeros (accumulate: unchanged)")
    return form


def _cd_rows():
    rows, i = [], 0
    for k in (1, 3):
        for (H, W) in _CF_SHAPES:
            for acc in (0, 1):
                Cout = _CF_COUT[i % 5]
                rows.append(CD(2, H, W, 1 + i % 4, Cout, k, acc, (Cout + 8) if (i // 2) % 2 else 0, (Cout + 8) if i % 3 == 0 else 0))
                i += 1
    for n, Cout in enumerate(_CF_COUT):                      # every LP with both flags at W in {9, 12}
        rows += [CD(2, 5, 9, 3, Cout, 3, 1, Cout + 8), CD(2, 5, 12, 3, Cout, 1 if n % 2 else 3, 0, Cout + 8)]
    rows += [CD(1, 130, 127, 3, 256, 3, 1, 264), CD(1, 130, 127, 3, 256, 1, 0)]        # past the grid cap of 4096 blocks
    return rows


CD_ROWS = _cd_rows()


class TS(NamedTuple):
    B: int
    H: int
    W: int
    Cin: int
    ldz: int
    acc: int = 0


def ts_call(r, ad=None, stream=0):
    return "cdf_conv_cin4_tapsum3", (_at(ad, "z"), r.ldz, _at(ad, "dx"), r.B, r.H, r.W, r.Cin, r.acc, stream)


def _ts_case(be, r):
    B, H, W, Cin, ldz = r[:5]
    tag = "cin4 tapsum3 " + "-".join(map(str, r))
    g = torch.Generator().manual_seed(ldz * 11 + H + W)
    z, dx0 = torch.randn(B, H, W, 9 * Cin, generator=g), torch.randn(B, H, W, 4, generator=g)
    zd, dx0d = be.to(_pitched(z, ldz)), be.to(dx0)                       # (the columns 9 Cin .. ldz of a z row are never summed)
    dx = nan_empty(be, B, H, W, 4)
    name, args = ts_call(r, dict(z=P(zd), dx=P(dx)), be.stream())
    form = cin4_tapsum3_form(*ts_call(r))
    assert cin4_tapsum3_form(name, args) == form, tag
    print(f"{tag}: form {form}")

    def launch():
        if r.acc:
            dx.copy_(dx0d)
        getattr(be.L, name)(*args)
    dxo = twice(launch, [dx])[0]
    zs = z.double().reshape(B, H, W, Cin, 3, 3)
    ts_r = torch.zeros(B, H + 2, W + 2, Cin, dtype=torch.float64)
    for i in range(3):
        for j in range(3):                                   # dx[q] = sum over taps (i, j) of z[q - (i - 1, j - 1)][tap]
            ts_r[:, i:i + H, j:j + W] += zs[..., i, j]
    ref = torch.zeros(B, H, W, 4, dtype=torch.float64)
    ref[..., :Cin] = ts_r[:, 1:H + 1, 1:W + 1]
    bound = K_SUM * U * 3 * 2 * _amax(zs)
    if r.acc:
        ref = ref + dx0.double()
        bound += U * _amax(ref)
    _chk("cin4 tapsum3", f"{tag} dx", dxo[..., :Cin], ref[..., :Cin], bound)
    assert torch.equal(dxo[..., Cin:], dx0[..., Cin:] if r.acc else torch.zeros(B, H, W, 4 - Cin)), (tag, "channels >= Cin: exact zeros (accumulate: unchanged)")
    return form


TS_ROWS = [TS(2, 17, 33, 1, 12), TS(2, 17, 33, 3, 28), TS(2, 17, 33, 4, 36), TS(2, 17, 33, 4, 48, 1), TS(2, 17, 33, 1, 12, 1), TS(2, 17, 33, 3, 28, 1),
           TS(2, 17, 33, 2, 36, 1), TS(2, 33, 17, 3, 48), TS(2, 33, 17, 2, 20, 1), TS(1, 16, 32, 3, 28), TS(1, 32, 16, 4, 36, 1), TS(2, 16, 16, 3, 28, 1),
           TS(1, 5, 12, 3, 28), TS(1, 12, 5, 1, 48, 1), TS(1, 16, 33, 3, 28), TS(1, 17, 32, 2, 20, 1)]    # (ragged along x only / along y only)


# ---------------------------------------------------------------------------------------------------------------------------------
# cin4 weight gradient: per-chunk partials, then the slab reduction the product runs (accumulating, bias fused when there is a bsum)
# ---------------------------------------------------------------------------------------------------------------------------------
class CW(NamedTuple):
    B: int
    H: int
    W: int
    Cin: int
    Cout: int
    k: int
    bsum: int = 1
    ldd: int = 0
    big: bool = False


def cw_call(r, ad=None, stream=0):
    return "cdf_conv_cin4_wgrad", (_at(ad, "x"), _at(ad, "dy"), r.ldd or r.Cout, _at(ad, "part"), _at(ad, "bsum", r.bsum), r.B, r.H, r.W, r.Cin, r.Cout, r.k, stream)


def cw_unpack_call(r, ad=None, stream=0):
    """The reduction ops.conv_cin4_bwd launches after it."""
    KK, Cin, C = r.k * r.k, r.Cin, r.Cout
    nch = cin4_chunks(r.B * r.H * r.W, r.W)[0]
    head = (_at(ad, "part"), _at(ad, "dw"), nch, KK, Cin, C, C, 1, KK, Cin * KK)
    if r.bsum:
        return "cdf_unpack_reduce_bias", head + (_at(ad, "bsum"), _at(ad, "db"), C, 1, 1, stream)
    return "cdf_unpack_reduce", head + (1, 1, stream)


def _cw_case(be, r):
    skip_emu(be, r.big)
    B, H, W, Cin, Cout, k = r[:6]
    KK, M = k * k, B * H * W
    tag = "cin4 wgrad " + "-".join(map(str, r))
    g = torch.Generator().manual_seed(Cout * 3 + H * 5 + W + Cin + k)
    x = torch.zeros(B, H, W, 4)
    x[..., :Cin] = torch.randn(B, H, W, Cin, generator=g)
    dy = torch.randn(B, H, W, Cout, generator=g)
    dw0, db0 = torch.randn(Cout, Cin, k, k, generator=g), torch.randn(Cout, generator=g)
    xd, dyd, dw0d, db0d = be.to(x), be.to(_pitched(dy, r.ldd or Cout)), be.to(dw0), be.to(db0)
    nch, mpc = cin4_chunks(M, W)
    assert nch == be.L.cdf_conv_cin4_nchunk(M)
    part, bsum, dw, db = nan_empty(be, nch, KK * Cin, Cout), nan_empty(be, nch, Cout), nan_empty(be, Cout, Cin, k, k), nan_empty(be, Cout)
    ad = dict(x=P(xd), dy=P(dyd), part=P(part), bsum=P(bsum), dw=P(dw), db=P(db))
    name, args = cw_call(r, ad, be.stream())
    uname, uargs = cw_unpack_call(r, ad, be.stream())
    form = cin4_wgrad_form(*cw_call(r))
    assert cin4_wgrad_form(name, args) == form and unpack_form(uname, uargs) == unpack_form(*cw_unpack_call(r)), tag
    print(f"{tag}: form {form} ({nch} chunks of {mpc} pixels), reduced as {unpack_form(uname, uargs)}")

    def launch():
        dw.copy_(dw0d), db.copy_(db0d)
        getattr(be.L, name)(*args)
        getattr(be.L, uname)(*uargs)
    dwo, dbo, parto, bsumo = twice(launch, [dw, db, part, bsum])
    xx, gg = x[..., :Cin].permute(0, 3, 1, 2).double(), dy.permute(0, 3, 1, 2).double()
    dw_r = torch.nn.grad.conv2d_weight(xx, (Cout, Cin, k, k), gg, padding=k // 2)
    gb = K_SUM * U * math.sqrt(M) * _amax(xx) * gg.pow(2).sum((0, 2, 3)).sqrt().max().item()
    ref = dw_r + dw0.double()
    _chk("cin4 wgrad", f"{tag} dw", dwo, ref, min(gb, 5e-5 * max(1.0, _amax(dw_r))) + U * _amax(ref))
    if r.bsum:
        db_r = gg.sum((0, 2, 3))
        ref = db_r + db0.double()
        _chk("cin4 wgrad", f"{tag} db", dbo, ref, min(sum_bound(gg.permute(1, 0, 2, 3).reshape(Cout, -1), 1), 5e-5 * max(1.0, _amax(db_r))) + U * _amax(ref))
    else:
        assert _poisoned(bsumo) and bits_equal(dbo, db0), (tag, "bsum is null in this call: its stand-in buffer and db must be untouched")
    if form[6]:                                              # the empty trailing chunk: its slab and bsum row are written, exact zeros
        assert (nch - 1) * mpc >= M and (parto[-1] == 0).all() and (not r.bsum or (bsumo[-1] == 0).all()), (tag, "the empty chunk's partials are not zeros")
    return form


def _cw_rows():
    rows, i = [], 0
    for (H, W) in ((5, 12), (12, 5), (5, 9), (9, 5), (7, 12)):
        for k in (1, 3):
            for bsum in (1, 0):
                Cout = _CF_COUT[i % 5]
                rows.append(CW(2, H, W, 1 + i % 4, Cout, k, bsum, (Cout + 8) if (i // 2) % 2 == 0 else 0))
                i += 1
    rows += [CW(2, 23, 25, 3, 32, 3, 1, 40), CW(2, 24, 28, 3, 32, 1, 1), CW(2, 24, 28, 2, 8, 3, 0, 16), CW(2, 23, 25, 4, 4, 1, 1)]       # several chunks
    rows += [CW(2, 129, 260, 3, 8, 3, 1), CW(2, 129, 260, 3, 8, 1, 0, 16)]     # 131 chunks of 516 pixels, the 131st empty (PX = 4)
    return rows


CW_ROWS = _cw_rows()


# ---------------------------------------------------------------------------------------------------------------------------------
# slab reductions
# ---------------------------------------------------------------------------------------------------------------------------------
class UR(NamedTuple):
    """st: (s_t, s_r, s_c), or 'conv' for (1, T, R T) / 'tconv' for (1, C T, T) (transposed-conv weights [R][C][T]); ldc 0: r4(C)."""
    ns: int
    T: int
    R: int
    C: int
    st: object = "conv"
    acc: int = 1
    bias: int = 0
    tiled: int = 1
    ldc: int = 0
    big: bool = False


def _ur_strides(r):
    return {"conv": (1, r.T, r.R * r.T), "tconv": (1, r.C * r.T, r.T)}.get(r.st, r.st)


def ur_call(r, ad=None, stream=0):
    ldc = r.ldc or r4(r.C)
    head = (_at(ad, "ws"), _at(ad, "g"), r.ns, r.T, r.R, r.C, ldc) + tuple(_ur_strides(r))
    if r.bias:
        return "cdf_unpack_reduce_bias", head + (_at(ad, "bws"), _at(ad, "gb"), ldc, r.acc, r.tiled, stream)
    return "cdf_unpack_reduce", head + (r.acc, r.tiled, stream)


def _ur_case(be, r):
    skip_emu(be, r.big)
    ns, T, R, C = r[:4]
    ldc = r.ldc or r4(C)
    s_t, s_r, s_c = _ur_strides(r)
    tag = "unpack_reduce " + "-".join(map(str, r))
    g_ = torch.Generator().manual_seed(ns * 7 + T + R + C)
    ws, bws = torch.randn(ns, T, R, C, generator=g_), torch.randn(ns, C, generator=g_)
    idx = (torch.arange(T)[:, None, None] * s_t + torch.arange(R)[None, :, None] * s_r + torch.arange(C)[None, None, :] * s_c).reshape(-1)
    assert idx.unique().numel() == idx.numel(), (tag, "the strides must address each element once")
    n = int(idx.max()) + 1 + 8                                # (8 floats past the last element: they must not change)
    g0, gb0 = torch.randn(n, generator=g_), torch.randn(C + 4, generator=g_)
    wsd, bwsd, g0d, gb0d = be.to(_pitched(ws, ldc)), be.to(_pitched(bws, ldc)), be.to(g0), be.to(gb0)       # slab pad columns: NaN
    g, gb = nan_empty(be, n), nan_empty(be, C + 4)
    name, args = ur_call(r, dict(ws=P(wsd), g=P(g), bws=P(bwsd), gb=P(gb)), be.stream())
    form = unpack_form(*ur_call(r))
    assert unpack_form(name, args) == form, tag
    print(f"{tag}: form {form}")

    def launch():
        if r.acc:
            g.copy_(g0d), gb.copy_(gb0d)
        getattr(be.L, name)(*args)
    go, gbo = twice(launch, [g, gb])
    ref, bound = ws.double().sum(0).reshape(-1), sum_bound(ws.double(), 0)
    bref, bbound = bws.double().sum(0), sum_bound(bws.double(), 0)
    if r.acc:
        ref, bref = ref + g0[idx].double(), bref + gb0[:C].double()
        bound, bbound = bound + U * _amax(ref), bbound + U * _amax(bref)
    _chk("unpack", f"{tag} g", go[idx], ref, bound)
    rest = torch.ones(n, dtype=torch.bool)
    rest[idx] = False
    assert bits_equal(go[rest], g0[rest]) if r.acc else _poisoned(go[rest]), (tag, "an element the strides do not address changed")
    if r.bias:
        _chk("unpack", f"{tag} bias", gbo[:C], bref, bbound)
        assert bits_equal(gbo[C:], gb0[C:]) if r.acc else _poisoned(gbo[C:]), (tag, "an element past the bias gradient changed")
    else:
        assert bits_equal(gbo, gb0) if r.acc else _poisoned(gbo), (tag, "no bias reduction in this call: its stand-in buffer must be untouched")
    return form


def _ur_rows():
    rows = []
    # the attention path's stride sets at the recorded (nsplit, T, R, C), onto live contents (ops.py: linattn weight / bias gradients)
    rows += [UR(16, 64, 64, 64, (64 * 64, 64, 1), 0), UR(16, 64, 64, 64, (64 * 64, 64, 1), 1), UR(4, 64, 128, 128, (128 * 128, 128, 1), 0),
             UR(16, 64, 128, 128, (128 * 128, 128, 1), 1, big=True)]                           # (CA ldw, ldw, 1), T = B
    rows += [UR(16, 4, 32, 64, (32, 1, 128)), UR(16, 4, 32, 128, (32, 1, 128)), UR(1, 4, 32, 32, (32, 1, 128)), UR(16, 4, 32, 64, (32, 1, 128), 0)]   # (32, 1, HD), T = heads
    rows += [UR(64, 1, 128, 64, (0, 64, 1)), UR(64, 1, 128, 128, (0, 128, 1)), UR(2, 1, 128, 32, (0, 32, 1)), UR(64, 1, 128, 64, (0, 64, 1), 0)]      # (0, dim, 1)
    rows += [UR(1024, 1, 1, 64, (0, 0, 1)), UR(256, 1, 1, 128, (0, 0, 1)), UR(18, 1, 1, 32, (0, 0, 1)), UR(4, 1, 1, 32, (0, 0, 1)), UR(1024, 1, 1, 64, (0, 0, 1), 0)]
    rows += [UR(16, 4, 32, 64, (32, 1, 128), ldc=72), UR(64, 1, 100, 60, (0, 72, 1), ldc=64), UR(33, 2, 5, 28, (5 * 40, 40, 1), ldc=36)]           # ldc > C, an output pitch > C
    # the cin4 path's fused call: R = 3 (below RJ = 4) in the tiled <9, 4> kernel, and its 1 x 1 form
    rows += [UR(131, 9, 3, 128, bias=1), UR(9, 9, 3, 64, bias=1), UR(2, 9, 3, 32, bias=1), UR(131, 1, 3, 64, bias=1), UR(9, 1, 3, 32, bias=1), UR(7, 9, 3, 8, bias=1)]
    # every kernel x C in {28, 32, 72} x nsplit in {1, 7, 8, 31, 32, 131}, ldc > C on every other row
    i = 0
    for T, R, st in ((9, 6, "conv"), (9, 5, "conv"), (16, 4, "conv"), (16, 3, "tconv"), (1, 64, "conv"), (1, 37, "conv"), (2, 5, "conv"), (3, 4, (20 * 80, 80, 1))):
        for C in (28, 32, 72):
            for ns in ((1, 8, 32), (7, 31, 131))[i % 2]:
                rows.append(UR(ns, T, R, C, (st[0], st[1], st[2]) if isinstance(st, tuple) else st, (i // 2) % 2 if i % 5 else 1, bias=(i // 3) % 2, ldc=(r4(C) + 8) if i % 2 else 0))
                i += 1
    rows += [UR(13, 9, 8, 64, tiled=0, bias=1), UR(40, 1, 32, 40, tiled=0)]                  # the tiled flag off: the SL kernels on conv strides
    return rows


UR_ROWS = _ur_rows()


# ---------------------------------------------------------------------------------------------------------------------------------
# column sums
# ---------------------------------------------------------------------------------------------------------------------------------
class CS(NamedTuple):
    io: int
    nseg: int
    rows: int
    C: int
    acc: int = 1
    ld: int = 0
    ldo: int = 0
    big: bool = False


def cs_call(r, ad=None, stream=0):
    base = (_at(ad, "x"), _at(ad, "out"), _at(ad, "ws"), r.nseg, r.rows, r.C, r.ld or r.C, r.ldo or r.C, r.acc)
    return ("cdf_colsum_io", base + (1, stream)) if r.io else ("cdf_colsum", base + (stream,))


def _cs_case(be, r):
    skip_emu(be, r.big)
    io, nseg, rows, C = r[:4]
    ld, ldo = r.ld or C, r.ldo or C
    tag = "colsum " + "-".join(map(str, r))
    g_ = torch.Generator().manual_seed(rows % 1000 + C)
    x, o0 = torch.randn(nseg, rows, C, generator=g_), torch.randn(nseg, ldo, generator=g_)
    if io:
        x = x.bfloat16().float()
    nch, rpc = colsum_chunks(rows)
    assert nch == be.L.cdf_colsum_nchunk(rows)
    xp = _pitched(x, ld)
    xd, o0d = be.to(xp.bfloat16().view(torch.int16) if io else xp), be.to(o0)
    ws, out = nan_empty(be, nseg * nch * C), nan_empty(be, nseg, ldo)
    name, args = cs_call(r, dict(x=P(xd), out=P(out), ws=P(ws)), be.stream())
    form = colsum_form(*cs_call(r))
    assert colsum_form(name, args) == form, tag
    print(f"{tag}: form {form} ({nch} chunks of {rpc} rows)")

    def launch():
        if r.acc:
            out.copy_(o0d)
        getattr(be.L, name)(*args)
    oo, wso = twice(launch, [out, ws])
    ref, bound = x.double().sum(1), sum_bound(x.double(), 1)
    if r.acc:
        ref = ref + o0[:, :C].double()
        bound += U * _amax(ref)
    _chk("colsum", f"{tag} out", oo[:, :C], ref, bound)
    assert bits_equal(oo[:, C:], o0[:, C:]) if r.acc else _poisoned(oo[:, C:]), (tag, "a pad column of the output changed")
    if form[4]:
        assert (wso.view(nseg, nch, C)[:, -1] == 0).all(), (tag, "the empty chunk's partial sums are not zeros")
    return form


CS_ROWS = [CS(0, 2, 300, 64, 1, 72, 68), CS(1, 2, 300, 40, 0, 48, 44), CS(0, 3, 37, 130, 0), CS(1, 1, 1023, 64, 1, 0, 72),
           CS(0, 2, 1100, 68, 1, 72, 72), CS(1, 2, 1100, 64, 0, 128), CS(0, 1, 4608, 32, 0, 0, 36), CS(1, 1, 1152, 64, 1, 128),
           CS(0, 1, 512 * 600 + 80, 4, 1, 8, 8), CS(1, 1, 512 * 600 + 80, 4, 0),                      # 600 chunks of 513 rows, the last one empty
           CS(0, 1, 1025 * 512, 4, 1, 8), CS(1, 1, 1025 * 512, 4, 0, 0, 8),                           # capped, no empty chunk (the last one holds one row)
           CS(1, 1, 512 * 1024 + 37, 4, 1, 8, 8)]                                                     # capped, an empty chunk, accumulating, bf16


# ---------------------------------------------------------------------------------------------------------------------------------
# the tested forms; the forms the recordings reach
# ---------------------------------------------------------------------------------------------------------------------------------
CLASSIFIERS = {            # what -> (entry points, form function, rows, the row's (name, stand-in arguments))
    "cin4_fwd": (CIN4_FWD_NAMES, cin4_fwd_form, lambda: CF_ROWS, cf_call),
    "cin4_dgrad": (CIN4_DGRAD_NAMES, cin4_dgrad_form, lambda: CD_ROWS, cd_call),
    "cin4_tapsum3": (CIN4_TAPSUM_NAMES, cin4_tapsum3_form, lambda: TS_ROWS, ts_call),
    "cin4_wgrad": (CIN4_WGRAD_NAMES, cin4_wgrad_form, lambda: CW_ROWS, cw_call),
    "unpack": (UNPACK_NAMES, unpack_form, lambda: UR_ROWS, ur_call),
    "colsum": (COLSUM_NAMES, colsum_form, lambda: CS_ROWS, cs_call),
}
ALL_NAMES = tuple(n for names, *_ in CLASSIFIERS.values() for n in names)


def forms_of_rows(what):
    _, form, rows, call = CLASSIFIERS[what]
    out = {form(*call(r)) for r in rows()}
    if what == "unpack":                                     # a weight-gradient row runs the product's reduction of its partials as well
        out |= {unpack_form(*cw_unpack_call(r)) for r in CW_ROWS}
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
    "cin4_fwd": {
        (1, 0, 'y', 1, '', 16, 1, 0),
        (3, 1, 'ph', 1, '', 32, 1, 0),
        (3, 1, 'phl', 1, '', 32, 1, 0),
    },
    "cin4_dgrad": set(),                                     # (the image-side convs are first layers: no recording asks for their dx)
    "cin4_tapsum3": {
        (3, 0, 'r4', 0, 0, 0),
    },
    "cin4_wgrad": {
        (1, 4, 3, 1, 0, 'capped', 0, 0),
        (3, 4, 3, 1, 0, 'capped', 0, 0),
    },
    "unpack": {
        ('SL16', 0, 1, 'c1', 0, 0, '>=32'),
        ('SL16', 1, 1, 'conv', 1, 0, '>=32'),
        ('SL4', 0, 0, 'c1', 0, 0, '8-31'),
        ('SL4', 0, 0, 'c1', 0, 0, '<8'),
        ('SL4', 0, 1, 'other', 0, 0, '8-31'),
        ('tiled<1,32>', 0, 1, 'conv', 0, 0, '>=32'),
        ('tiled<1,32>', 1, 1, 'conv', 0, 0, '8-31'),
        ('tiled<1,32>', 1, 1, 'conv', 0, 0, '>=32'),
        ('tiled<1,32>', 1, 1, 'conv', 0, 1, '>=32'),
        ('tiled<16,2>', 0, 1, 'other', 0, 0, '8-31'),
        ('tiled<16,2>', 0, 1, 'other', 0, 0, '>=32'),
        ('tiled<16,2>', 1, 1, 'conv', 0, 0, '8-31'),
        ('tiled<16,2>', 1, 1, 'conv', 0, 0, '>=32'),
        ('tiled<9,4>', 1, 1, 'conv', 0, 0, '8-31'),
        ('tiled<9,4>', 1, 1, 'conv', 0, 0, '<8'),
        ('tiled<9,4>', 1, 1, 'conv', 0, 0, '>=32'),
        ('tiled<9,4>', 1, 1, 'conv', 0, 1, '>=32'),
    },
    "colsum": {
        (0, 1, '', '1', 0, 0),
        (0, 1, '', 'capped', 0, 0),
        (0, 1, '', 'many', 0, 0),
        (0, 1, 'i', 'many', 0, 0),
        (1, 1, '', 'capped', 0, 0),
        (1, 1, 'i', 'many', 0, 0),
    },
}
# ... and the forms that one forward + backward pass of two small networks (test_recorded_side_forms_dry; bf16x3, bf16 and f32) reaches besides
SMALL_NETWORKS = {
    "cin4_fwd": {
        (1, 0, 'y', 1, '', 8, 0, 0),
        (3, 1, 'yp', 1, '', 16, 0, 0),
    },
    "cin4_dgrad": {
        (1, 0, 0, 8, 0, 0),
    },
    "cin4_tapsum3": set(),
    "cin4_wgrad": {
        (1, 4, 3, 1, 0, 'many', 0, 0),
        (3, 4, 3, 1, 0, 'many', 0, 0),
    },
    "unpack": {
        ('SL4', 0, 1, 'c1', 0, 0, '8-31'),
        ('SL4', 0, 1, 'c1', 0, 0, '<8'),
        ('SL4', 0, 1, 'other', 0, 0, '<8'),
        ('SL4', 1, 1, 'conv', 1, 0, '8-31'),
        ('SL4', 1, 1, 'conv', 1, 0, '<8'),
        ('tiled<1,32>', 0, 1, 'conv', 0, 0, '8-31'),
        ('tiled<1,32>', 0, 1, 'conv', 0, 0, '<8'),
        ('tiled<1,32>', 1, 1, 'conv', 0, 0, '<8'),
        ('tiled<1,32>', 1, 1, 'conv', 0, 1, '8-31'),
        ('tiled<16,2>', 0, 1, 'other', 0, 0, '<8'),
        ('tiled<16,2>', 1, 1, 'conv', 0, 0, '<8'),
        ('tiled<9,4>', 1, 1, 'conv', 0, 1, '8-31'),
        ('tiled<9,4>', 1, 1, 'conv', 0, 1, '<8'),
    },
    "colsum": {
        (0, 1, '', '1', 0, 1),
        (0, 1, '', 'many', 0, 1),
        (1, 1, '', 'many', 0, 1),
    },
}


# ... with a row for each of them: the smallest shape of the form, built from the form itself (each builder is the inverse of its
# classifier; the assertion below holds it to that)
def _pit(letters, c, C):
    return C + 8 if c in letters else 0


def _cin4_shape(LP, capped, hw):
    """(B, H, W): 2 x 5 x 12 / 2 x 7 x 7, or one image one row or so past 4096 blocks of 256 / LP pixels."""
    if not capped:
        return (2, 5, 12) if hw else (2, 7, 7)
    need = 4096 * (256 // LP) + 1
    if hw:
        return 1, cdiv(need, 127), 127
    side = math.isqrt(need - 1) + 1
    return 1, side, side


def _cf_row_of(f):
    k, act, outs, bias, pit, LP, capped, hw = f
    C = 4 * LP
    return CF(*_cin4_shape(LP, capped, hw), 3, C, k, act, outs, bias, _pit(pit, "y", C), _pit(pit, "p", C), _pit(pit, "s", C), _pit(pit, "w", C))


def _cd_row_of(f):
    k, acc, pitched, LP, capped, hw = f
    return CD(*_cin4_shape(LP, capped, hw), 3, 4 * LP, k, acc, 4 * LP + 8 if pitched else 0)


def _ts_row_of(f):
    Cin, acc, cls, rx, ry, hw = f
    H = 17 if ry else 16
    W = (33 if hw or not ry else 17) if rx else (32 if hw else 16)
    return TS(2, H, W, Cin, r4(9 * Cin) + (8 if cls == "wide" else 0), acc)


def _cw_row_of(f):
    k, px, Cin, bsum, pitched, cls, empty, hw = f
    shape = {("1", 0): {(4, 0): (2, 12, 12), (4, 1): (2, 5, 12), (1, 0): (2, 9, 9), (1, 1): (2, 5, 9)},
             ("many", 0): {(4, 0): (2, 48, 48), (4, 1): (2, 24, 28), (1, 0): (2, 23, 23), (1, 1): (2, 23, 25)},
             ("many", 1): {(4, 1): (2, 129, 260)},
             ("capped", 0): {(4, 0): (1, 768, 768), (4, 1): (1, 731, 728), (1, 0): (1, 729, 729), (1, 1): (1, 727, 729)},
             ("capped", 1): {(4, 0): (1, 728, 728)}}[(cls, empty)][(px, hw)]          # (728 x 728: 1024 chunks of 520 pixels, the last one empty)
    return CW(*shape, Cin, 8, k, bsum, 16 if pitched else 0)


def _ur_row_of(f):
    kernel, bias, acc, strides, c32, rrj, nsc = f
    ns = {"<8": 3, "8-31": 13, ">=32": 37}[nsc]
    if kernel.startswith("tiled"):
        T, rj = {"tiled<9,4>": (9, 4), "tiled<16,2>": (16, 2), "tiled<1,32>": (1, 32)}[kernel]
        R, C = 3 if rrj else 2 * rj, 40 if c32 else 64
        return UR(ns, T, R, C, {"conv": "conv", "other": "tconv"}[strides], acc, bias)
    if strides == "conv":                                    # the SL kernels on conv strides: fewer than 32 output channels
        return UR(ns, 9, 5, 3 if c32 else 16, "conv", acc, bias) if c32 else UR(ns, 2, 5, 64, "conv", acc, bias)
    C = 28 if c32 else 64
    return UR(ns, 4, 32, C, (32, 1, 128), acc, bias) if strides == "other" else UR(ns, 2, 5, C, (5 * (C + 8), C + 8, 1), acc, bias)


def _cs_row_of(f):
    io, acc, pit, cls, empty, c64 = f
    rows = {("1", 0): 300, ("many", 0): 1100, ("many", 1): 512 * 600 + 80, ("capped", 0): 1025 * 512, ("capped", 1): 512 * 1024 + 37}[(cls, empty)]
    C = 40 if c64 else 64
    return CS(io, 1 if cls == "capped" else 2, rows, C, acc, _pit(pit, "i", C), _pit(pit, "o", C))


for _what, _rows, _of in (("cin4_fwd", CF_ROWS, _cf_row_of), ("cin4_dgrad", CD_ROWS, _cd_row_of), ("cin4_tapsum3", TS_ROWS, _ts_row_of),
                          ("cin4_wgrad", CW_ROWS, _cw_row_of), ("unpack", UR_ROWS, _ur_row_of), ("colsum", CS_ROWS, _cs_row_of)):
    for _f in sorted(REACHED[_what] | SMALL_NETWORKS[_what], key=repr):
        if _f not in forms_of_rows(_what):
            _rows.append(_of(_f))
            assert CLASSIFIERS[_what][1](*CLASSIFIERS[_what][3](_rows[-1])) == _f, (_what, _f, _rows[-1])
# the capped weight-gradient shape whose LAST chunk is empty (the bench's 128 x 128 x 64 images divide evenly; most other sizes do not)
CW_ROWS.append(_cw_row_of((3, 4, 3, 1, 0, "capped", 1, 0)))


def test_form_tables():
    """The tables keep what they were built for, and the forms flagged as reached are tested forms."""
    for what in CLASSIFIERS:
        t = forms_of_rows(what)
        assert REACHED[what] | SMALL_NETWORKS[what] <= t, (what, sorted((REACHED[what] | SMALL_NETWORKS[what]) - t, key=repr))
        assert t - REACHED[what], what
    cf = forms_of_rows("cin4_fwd")
    assert {(f[2], f[3]) for f in cf} >= {(o, b) for o in _CF_OUTS for b in (0, 1)} and {f[5] for f in cf} == {1, 2, 8, 16, 32, 64}
    assert {f[0] for f in cf} == {1, 3} and {f[1] for f in cf} == {0, 1, 2} and set("ypsw") <= set("".join(f[4] for f in cf)) and any(f[4] == "ypsw" for f in cf)
    assert {f[6:] for f in cf} >= {(0, 0), (0, 1), (1, 0), (1, 1)} and any(f[2] in ("ph", "phl", "h", "hl") and f[6] for f in cf)
    assert {(r.H, r.W) for r in CF_ROWS} >= {(5, 12), (12, 5), (5, 9), (130, 127)} and {r.Cin for r in CF_ROWS} == {1, 2, 3, 4}
    cd = forms_of_rows("cin4_dgrad")
    assert {f[:3] for f in cd} == {(k, a, p) for k in (1, 3) for a in (0, 1) for p in (0, 1)} and {f[3] for f in cd} >= {1, 2, 8, 32, 64}
    assert {f[4:] for f in cd} >= {(0, 0), (0, 1), (1, 1)} and any(f[1] and f[2] and f[4] for f in cd)
    ts = forms_of_rows("cin4_tapsum3")
    assert {f[0] for f in ts} == {1, 2, 3, 4} and {f[1:3] for f in ts} == {(0, "r4"), (1, "r4"), (0, "wide"), (1, "wide")} and {f[3:5] for f in ts} == {(0, 0), (1, 1), (0, 1), (1, 0)}
    assert {r.ldz for r in TS_ROWS} >= {12, 28, 36, 48} and {(r.H, r.W) for r in TS_ROWS} >= {(17, 33), (33, 17)}
    cw = forms_of_rows("cin4_wgrad")
    assert {f[:2] for f in cw} == {(1, 1), (1, 4), (3, 1), (3, 4)} and {f[2] for f in cw} == {1, 2, 3, 4} and {f[3:5] for f in cw} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {f[5:7] for f in cw} == {("1", 0), ("many", 0), ("many", 1), ("capped", 0), ("capped", 1)} and {f[7] for f in cw} == {0, 1}
    assert (2, 129, 260, 3, 8, 3) in {r[:6] for r in CW_ROWS} and cin4_chunks(2 * 129 * 260, 260) == (131, 516)
    ur = forms_of_rows("unpack")
    assert {f[0] for f in ur} == {"tiled<9,4>", "tiled<16,2>", "tiled<1,32>", "SL16", "SL4"} and {f[3] for f in ur} == {"c1", "conv", "other"}
    for kern in ("tiled<9,4>", "tiled<16,2>", "tiled<1,32>", "SL16", "SL4"):
        fs = {f for f in ur if f[0] == kern}
        assert {f[1] for f in fs} == {0, 1} and {f[2] for f in fs} == {0, 1} and {f[4] for f in fs} == {0, 1}, kern
        assert not kern.startswith("tiled") or ({f[5] for f in fs} == {0, 1} and {f[6] for f in fs} == {"<8", "8-31", ">=32"}), kern
    assert {r.ns for r in UR_ROWS} >= {1, 7, 8, 31, 32, 131} and {r.C for r in UR_ROWS} >= {28, 32, 72} and any(r.ldc > r4(r.C) for r in UR_ROWS)
    for st, acc in (((64 * 64, 64, 1), 1), ((32, 1, 128), 1), ((0, 64, 1), 1), ((0, 0, 1), 1)):
        assert any(r.st == st and r.acc == acc for r in UR_ROWS), st
    cs = forms_of_rows("colsum")
    assert {f[:2] for f in cs} == {(0, 0), (0, 1), (1, 0), (1, 1)} and {f[2] for f in cs} == {"", "i", "o", "io"} and {f[5] for f in cs} == {0, 1}
    assert {f[3:5] for f in cs} == {("1", 0), ("many", 0), ("many", 1), ("capped", 0), ("capped", 1)}


def dry_recordings(monkeypatch, names):
    """(recorded, small): the recordings of test_gpu_invariance.py::test_coverage_guard without a GPU (the technique of
    test_norm_dw_forms.py::test_recorded_norm_dw_forms_dry: real shapes, CPU tensors, every launching entry point a stub that returns 0 --
    the argument tuples are decided by the Python layer from shapes and modes alone) and those of one forward + backward pass of two
    small networks in the three arithmetic modes, as (recording, name, arguments) of the calls to `names`."""
    import ctypes
    import types
    from colddiff import _lib, runtime as rt
    from emu_util import emu_lib
    import test_gpu_invariance as gi
    import test_gpu_parity2 as p2
    from test_norm_dw_forms import _small_networks
    real, stub = emu_lib(), types.SimpleNamespace()
    for name, (restype, _) in real.protos.items():
        launches = restype is ctypes.c_int and not _lib._QUERY.search(name) and name != "cdf_gemm_tuning_default"
        setattr(stub, name, (lambda *a: 0) if launches else getattr(real, name))
    monkeypatch.setattr(rt, "_lib_override", stub)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    monkeypatch.setattr(gi, "DEV", "cpu")
    monkeypatch.setattr(p2, "DEV", "cpu")
    monkeypatch.setattr(gi, "_GEMM_FAMILY", names)
    _, _, calls = gi._guard_calls(p2.bench_step_inputs())
    small = []
    for mode in ("bf16x3", "bf16", "f32"):
        with rt.precision_scope(mode), gi.Recorder(stub) as rec:
            _small_networks()
        small += [("small " + mode, n, a) for n, a in rec.calls if n in names]
    return [c for c in calls if c[1] in names], small


def hold_recordings(mod, calls, small):
    """The guard's two assertions on a form module (this one, test_side_kernel_forms_attn): every recorded form is a tested form, every
    form of its REACHED sets is recorded; and the small networks' forms are tested forms and its SMALL_NETWORKS sets exactly."""
    reached, small = mod.reached_forms(calls), mod.reached_forms(small)
    for what in mod.CLASSIFIERS:
        print(f"{what} forms reached:", *sorted(reached[what], key=repr), sep="\n    ")
        print(f"{what} forms the small networks reach besides:", *sorted(set(small[what]) - set(reached[what]), key=repr), sep="\n    ")
    for what in mod.CLASSIFIERS:
        tested = mod.forms_of_rows(what)
        for src, r_ in (("the recordings", reached[what]), ("the small networks", small[what])):
            assert set(r_) <= tested, (what, src, sorted(set(r_) - tested, key=repr))
        assert mod.REACHED[what] == set(reached[what]), (what, sorted(mod.REACHED[what] ^ set(reached[what]), key=repr))
        besides = set(small[what]) - set(reached[what])
        assert mod.SMALL_NETWORKS[what] == besides, (what, sorted(mod.SMALL_NETWORKS[what] ^ besides, key=repr))


def test_recorded_side_forms_dry(monkeypatch):
    """The recordings of test_gpu_invariance.py::test_coverage_guard (the bench step in both modes, the sampler step, config 2) and of two
    small networks in bf16x3 / bf16 / f32, made without a GPU (dry_recordings), held to the guard's two assertions (hold_recordings)."""
    import sys
    hold_recordings(sys.modules[__name__], *dry_recordings(monkeypatch, ALL_NAMES))


# ---------------------------------------------------------------------------------------------------------------------------------
# the tests over the case tables (both backends)
# ---------------------------------------------------------------------------------------------------------------------------------
_ids = lambda r: "-".join(map(str, r)).replace(" ", "")


@pytest.mark.parametrize("r", CF_ROWS, ids=_ids)
def test_cin4_fwd_forms(be, r):
    _cf_case(be, r)


@pytest.mark.parametrize("r", CD_ROWS, ids=_ids)
def test_cin4_dgrad_forms(be, r):
    _cd_case(be, r)


@pytest.mark.parametrize("r", TS_ROWS, ids=_ids)
def test_cin4_tapsum3_forms(be, r):
    _ts_case(be, r)


@pytest.mark.parametrize("r", CW_ROWS, ids=_ids)
def test_cin4_wgrad_forms(be, r):
    _cw_case(be, r)


@pytest.mark.parametrize("r", UR_ROWS, ids=_ids)
def test_unpack_reduce_forms(be, r):
    _ur_case(be, r)


@pytest.mark.parametrize("r", CS_ROWS, ids=_ids)
def test_colsum_forms(be, r):
    _cs_case(be, r)


def test_cin4_tapsum3_refuses_ldz_52(be):
    """The kernel holds an 18 x 18 halo of z rows in dynamic LDS through a plain launch: 48 floats per row are 62,208 B, 52 would be 67,392 B,
    past the 64 KB such a launch gets (the simulator has no limit).  The argument check refuses it with a status, on both backends; it is
    a host-side check: nothing launches, dx keeps its poison."""
    from colddiff._lib import CdfError
    B, H, W = 1, 4, 4
    zd, dx = be.to(torch.zeros(B, H, W, 52)), nan_empty(be, B, H, W, 4)
    with pytest.raises(CdfError, match="<= 48"):
        be.L.cdf_conv_cin4_tapsum3(P(zd), 52, P(dx), B, H, W, 4, 0, be.stream())
    assert b"67,392" in be.L.cdf_last_error()
    if be.kind == "hip":
        torch.cuda.synchronize()
    assert _poisoned(dx.cpu())
    be.L.cdf_conv_cin4_tapsum3(P(zd), 48, P(dx), B, H, W, 4, 0, be.stream())        # the widest pitch the check admits launches
    if be.kind == "hip":
        torch.cuda.synchronize()
    assert (dx.cpu() == 0).all()
