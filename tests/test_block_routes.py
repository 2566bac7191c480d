"""Every autograd block of colddiff/functions.py and colddiff/bf16store.py, in every arithmetic mode and on both sides of the routes
the Python layer chooses by shape and mode, against an fp64 reference (tests/block_routes_ref.py over oracle/cold_oracle.py).

Per (case, mode) the test
  * runs the block through the module's own `forward` twice from the same state -- the second time on NaN-poisoned allocations -- and
    requires torch.equal on the output, every input gradient and every parameter gradient;
  * records the cdf_* calls and asserts the ROUTE the case must take.  The expectations in CASES are literals, read off
    colddiff/functions.py / ops.py by hand: a moved threshold (ops.WGRAD_SP_MIN_M, functions._SP_KMIN, a predicate) makes this file
    fail instead of silently moving a case onto another route;
  * compares with the fp64 reference:
      "f32", "bf16x3":  output / input gradients / time-embedding gradient  max-abs error <= 1e-4 * |ref|max,
                        each parameter gradient                              <= 1e-4 * max(|ref|max, 1e-3)
                        (the project's parity bound as tests/test_modules.py applies it to blocks; it holds for the attention
                        blocks' gradients too, so the wider 1e-3 * max(1, |ref|max) of test_linear_attention_block_all_forms is
                        not used here);
      "bf16":           runtime.BF16_TOLERANCE["grad_rel_of_tensor_max"] * |ref|max for every tensor (fp32 tensors and the bf16
                        stream alike; stream inputs are rounded to bf16 before the reference sees them).
    The worst error / bound ratio is printed per case.

Route flags (ROUTE_FLAGS: how each is seen in the recorded calls):
  presplit  a conv GEMM on operand planes split up front        lean      an fp32 copy of a planes-only tensor is not written
  cin4/res4 the image-side direct kernels (c1 / res_conv)        lnbwd     LayerNorm backward inside the data-gradient GEMM
  has_norm, tbias, has_res_conv   the block's own structure      dx_planes the block's data gradient leaves as planes too
  fused / qfold / kv_planes / kvctx / unfused_kv                 the forms of the linear-attention block
  n = {...}: exact call counts (cdf_split_bf16: planes that were NOT taken from the producer; the three weight-gradient kernels).

Worst error / bound per family (max over its cases), simulator | MI355X:
  family            f32              bf16x3           bf16             worst case (bf16x3)
  ConvNextBlockFn   0.030 | 0.028    0.247 | 0.247    0.191 | 0.191    cnx_narrow (in-kernel split GEMMs)
  LinAttnBlockFn    0.009 | 0.008    0.444 | 0.443    0.113 | 0.113    la160_512_kvsplit
  ConvFn / Join     0.012 | 0.012    0.147 | 0.148    0.049 | 0.049    join
  Model family      0.013 | 0.014    0.665 | 0.638    0.146 | 0.146    attn64_8 (grad of norm.weight)
  bf16 stream       -                -                0.128 | 0.138    bf_enter
In "f32" every case sits at <= 0.03 of the bound and never closer to it than in "bf16x3" (equal only where no bf16 kernel is involved:
down16, up16, final_1x1, la16_288 and the nodes without a GEMM).
"""
import contextlib
import inspect
import time

import pytest
import torch

import block_routes_ref as R
from poison import poisoned_allocations
from test_gpu_invariance import Recorder
from test_gpu_parity2 import _precision
from test_modules import mbe  # noqa: F401  (fixture: emu = simulator on CPU tensors, hip = MI355X, gpu-marked)

MODES = ("f32", "bf16x3", "bf16")
WX, WB, WF, SPLIT = "cdf_conv_wgrad_bf16x", "cdf_conv_wgrad_bf16", "cdf_conv_wgrad", "cdf_split_bf16"
GX, GXIO, GB, GF = "cdf_conv_gemm_bf16x", "cdf_conv_gemm_bf16x_io", "cdf_conv_gemm_bf16", "cdf_conv_gemm"


# ---------------------------------------------------------------------------------------------------------------------------------------
# how a route shows in the recorded calls
# ---------------------------------------------------------------------------------------------------------------------------------------
def _args(calls, *names):
    return [a for n, a in calls if n in names]


def _has(calls, *names):
    return any(n in names for n, _ in calls)


_DW = ("cdf_dwconv7", "cdf_dwconv7_planes", "cdf_dwconv7_io")           # (x, ldx, w, ldw, bias, sbias, sb_stride, y, ldy, B, H, W, C, flip, accumulate, ...)
ROUTE_FLAGS = {
    "presplit": lambda c: _has(c, GX, GXIO),
    # a producer handed a null fp32 output: cdf_layernorm_c_fwd / cdf_groupnorm_fwd_ex (y = argument 2), cdf_conv_cin4_fwd (4), the pre-split GEMM (7)
    "lean": lambda c: any(a[2] == 0 for a in _args(c, "cdf_layernorm_c_fwd", "cdf_groupnorm_fwd_ex")) or
    any(a[4] == 0 for a in _args(c, "cdf_conv_cin4_fwd")) or any(a[7] == 0 for a in _args(c, GX)),
    "cin4": lambda c: _has(c, "cdf_conv_cin4_tapsum3"),
    "res4": lambda c: _has(c, "cdf_conv_cin4_dgrad"),
    "lnbwd": lambda c: _has(c, "cdf_conv_gemm_bf16x_lnbwd"),
    "has_norm": lambda c: _has(c, "cdf_layernorm_c_fwd", "cdf_layernorm_c_fwd_io"),
    "tbias": lambda c: _has(c, "cdf_linear_small"),
    "has_res_conv": lambda c: any(a[13] == 1 and a[14] == 1 for a in _args(c, *_DW)),     # the depthwise data gradient ADDS to res_conv's
    "dx_planes": lambda c: _has(c, "cdf_dwconv7_planes"),
    "qfold": lambda c: _has(c, "cdf_linattn_kvctx") or any(a[2] == 0 for a in _args(c, "cdf_linattn_context")),       # (k | v tensor: koff = 0)
    "fused": lambda c: not _has(c, "cdf_linattn_dcontext"),
    "kv_planes": lambda c: _has(c, "cdf_linattn_bwd_kv_planes"),
    "kvctx": lambda c: _has(c, "cdf_linattn_kvctx"),
    "unfused_kv": lambda c: _has(c, "cdf_linattn_softk", "cdf_linattn_dk"),
}
# what the completeness guard wants on both sides somewhere in the table, in a mode other than "f32"
GUARDED_FLAGS = ("presplit", "lean", "cin4", "res4", "lnbwd", "has_res_conv", "has_norm", "tbias", "fused", "qfold", "kv_planes", "kvctx",
                 "dx_planes", "unfused_kv")


class E:
    """Expected route of one (case, mode): flags = "name" (on) / "!name" (off) words, n = exact call counts, has / no = entry points
    that must / must not appear."""

    def __init__(self, flags="", n=None, has=(), no=()):
        self.flags = {w.lstrip("!"): not w.startswith("!") for w in flags.split()}
        assert set(self.flags) <= set(ROUTE_FLAGS), set(self.flags) - set(ROUTE_FLAGS)
        self.n, self.has, self.no = dict(n or {}), tuple(has), tuple(no)

    def check(self, calls, tag):
        names = [n for n, _ in calls]
        for f, want in self.flags.items():
            assert ROUTE_FLAGS[f](calls) == want, (tag, "route flag", f, "expected", want, sorted(set(names)))
        for k, want in self.n.items():
            assert names.count(k) == want, (tag, "calls of", k, names.count(k), "expected", want)
        for k in self.has:
            assert k in names, (tag, "missing", k, sorted(set(names)))
        for k in self.no:
            assert k not in names, (tag, "unexpected", k)


def W(split, wx, wb, wf, **more):
    """Call counts: cdf_split_bf16 and the three weight-gradient kernels (planes / in-kernel split / exact fp32)."""
    return dict({SPLIT: split, WX: wx, WB: wb, WF: wf}, **more)


class Case:
    def __init__(self, name, classes, build, routes, family):
        self.name, self.classes, self.build, self.routes, self.family = name, tuple(classes.split()), build, routes, family

    def __repr__(self):
        return self.name


# ---------------------------------------------------------------------------------------------------------------------------------------
# the case table.  Thresholds behind the literals (functions.py / ops.py): _sp_suffix K >= 64 and N >= 64; want_presplit: channels % 8,
# forward AND data-gradient GEMM on the split kernels; lean / plane weight gradient from 512 pixels, CA, CB >= 64 (in-kernel split:
# >= 128); cdf_conv_gemm_bf16x_lnbwd_ok: LayerNorm width 64 or 128, M % 256 == 0, lo planes (bf16x3 only); kv_planes: dim >= 64,
# 512 pixels; kvctx: H*W % 128 == 0, dim % 32 == 0, 64 <= dim <= 512; to_out folded: dim <= 128.
# ---------------------------------------------------------------------------------------------------------------------------------------
_CNX = "ConvNextBlockFn ToNHWC ToNCHW Act Linear"
_CNX_OFF = "!cin4 !res4"
CASES = [
    # -- image-side block: cin4 + res4 + conv_cin_dgrad2, conv2 on planes out of the cin4 kernel; 512 pixels lean, 256 not
    Case("cnx_img_512", _CNX, lambda: R.convnext(3, 64, 2, 16, norm=False), {
        "f32": E("!presplit !lean cin4 res4 !lnbwd !has_norm tbias has_res_conv !dx_planes", W(0, 0, 0, 1), has=["cdf_conv_cin4_fwd"]),
        "bf16x3": E("presplit lean cin4 res4 !lnbwd !has_norm tbias has_res_conv !dx_planes", W(1, 1, 0, 0, **{GX: 2})),
        "bf16": E("presplit lean cin4 res4 !lnbwd !has_norm tbias has_res_conv !dx_planes", W(1, 1, 0, 0, **{GX: 2}))}, "ConvNextBlockFn"),
    Case("cnx_img_256", _CNX, lambda: R.convnext(3, 64, 1, 16, norm=False), {
        "f32": E("!presplit !lean cin4 res4 !lnbwd !has_norm tbias has_res_conv !dx_planes", W(0, 0, 0, 1)),
        "bf16x3": E("presplit !lean cin4 res4 !lnbwd !has_norm tbias has_res_conv !dx_planes", W(1, 0, 0, 1, **{GX: 2})),
        "bf16": E("presplit !lean cin4 res4 !lnbwd !has_norm tbias has_res_conv !dx_planes", W(1, 0, 0, 1, **{GX: 2}))}, "ConvNextBlockFn"),
    # -- narrow block: conv1 forward and conv2's data gradient on the in-kernel-split kernel (K >= 64, N = 64), the rest exact fp32; no planes
    Case("cnx_narrow", _CNX, lambda: R.convnext(16, 32, 2, 12), {
        "f32": E("!presplit !lean %s !lnbwd has_norm tbias has_res_conv !dx_planes" % _CNX_OFF, W(0, 0, 0, 3, **{GB: 0})),
        "bf16x3": E("!presplit !lean %s !lnbwd has_norm tbias has_res_conv !dx_planes" % _CNX_OFF, W(0, 0, 0, 3, **{GB: 2})),
        "bf16": E("!presplit !lean %s !lnbwd has_norm tbias has_res_conv !dx_planes" % _CNX_OFF, W(0, 0, 0, 3, **{GB: 2}))}, "ConvNextBlockFn"),
    # -- wide block with res_conv and norm: planes on both convs; weight gradients on planes at 512 pixels, exact fp32 at 256;
    #    LayerNorm backward inside the data-gradient GEMM (width 64, M % 256 == 0) where the planes have a lo half
    Case("cnx_wide_512", _CNX, lambda: R.convnext(64, 128, 2, 16), {
        "f32": E("!presplit !lean %s !lnbwd has_norm tbias has_res_conv !dx_planes" % _CNX_OFF, W(0, 0, 0, 3, **{GB: 0}), has=["cdf_layernorm_c_bwd"]),
        "bf16x3": E("presplit lean %s lnbwd has_norm tbias has_res_conv dx_planes" % _CNX_OFF, W(1, 2, 0, 1, **{GX: 3, GB: 2}),
                    no=["cdf_layernorm_c_bwd", "cdf_layernorm_c_bwd_planes"]),
        "bf16": E("presplit lean %s !lnbwd has_norm tbias has_res_conv !dx_planes" % _CNX_OFF, W(1, 2, 0, 1, **{GX: 4, GB: 2}), has=["cdf_layernorm_c_bwd"])},
         "ConvNextBlockFn"),
    Case("cnx_wide_256", _CNX, lambda: R.convnext(64, 128, 1, 16), {
        "f32": E("!presplit !lean %s !lnbwd has_norm tbias has_res_conv !dx_planes" % _CNX_OFF, W(0, 0, 0, 3)),
        "bf16x3": E("presplit !lean %s lnbwd has_norm tbias has_res_conv dx_planes" % _CNX_OFF, W(1, 0, 0, 3, **{GX: 3, GB: 2})),
        "bf16": E("presplit !lean %s !lnbwd has_norm tbias has_res_conv !dx_planes" % _CNX_OFF, W(1, 0, 0, 3, **{GX: 4, GB: 2}))}, "ConvNextBlockFn"),
    # -- dim == dim_out: no res_conv, the depthwise data gradient takes res = do
    Case("cnx_same_512", _CNX, lambda: R.convnext(64, 64, 2, 16), {
        "f32": E("!presplit !lean %s !lnbwd has_norm tbias !has_res_conv !dx_planes" % _CNX_OFF, W(0, 0, 0, 2)),
        "bf16x3": E("presplit lean %s lnbwd has_norm tbias !has_res_conv dx_planes" % _CNX_OFF, W(1, 2, 0, 0, **{GX: 3, GB: 0})),
        "bf16": E("presplit lean %s !lnbwd has_norm tbias !has_res_conv !dx_planes" % _CNX_OFF, W(1, 2, 0, 0, **{GX: 4, GB: 0}))}, "ConvNextBlockFn"),
    # -- the other side of conv_dgrad_lnbwd_ok: 4 x 12 x 12 = 576 pixels (lean, planes) is no multiple of 256
    Case("cnx_same_576", _CNX, lambda: R.convnext(64, 64, 4, 12), {
        "f32": E("!presplit !lean %s !lnbwd has_norm tbias !has_res_conv !dx_planes" % _CNX_OFF, W(0, 0, 0, 2)),
        "bf16x3": E("presplit lean %s !lnbwd has_norm tbias !has_res_conv dx_planes" % _CNX_OFF, W(1, 2, 0, 0, **{GX: 4}), has=["cdf_layernorm_c_bwd"]),
        "bf16": E("presplit lean %s !lnbwd has_norm tbias !has_res_conv !dx_planes" % _CNX_OFF, W(1, 2, 0, 0, **{GX: 4}), has=["cdf_layernorm_c_bwd"])},
         "ConvNextBlockFn"),
    # -- ... and a LayerNorm width that is neither 64 nor 128 (96 -> 96 at 512 pixels)
    Case("cnx_96_512", _CNX, lambda: R.convnext(96, 96, 2, 16, mult=1), {
        "f32": E("!presplit !lean %s !lnbwd has_norm tbias !has_res_conv !dx_planes" % _CNX_OFF, W(0, 0, 0, 2)),
        "bf16x3": E("presplit lean %s !lnbwd has_norm tbias !has_res_conv dx_planes" % _CNX_OFF, W(1, 2, 0, 0, **{GX: 4}), has=["cdf_layernorm_c_bwd"]),
        "bf16": E("presplit lean %s !lnbwd has_norm tbias !has_res_conv !dx_planes" % _CNX_OFF, W(1, 2, 0, 0, **{GX: 4}))}, "ConvNextBlockFn"),
    # -- no time embedding (final_conv.0)
    Case("cnx_notime", "ConvNextBlockFn ToNHWC ToNCHW", lambda: R.convnext(64, 64, 1, 16, tdim=None), {
        "f32": E("!presplit !lean %s !lnbwd has_norm !tbias !has_res_conv !dx_planes" % _CNX_OFF, W(0, 0, 0, 2)),
        "bf16x3": E("presplit !lean %s lnbwd has_norm !tbias !has_res_conv dx_planes" % _CNX_OFF, W(1, 0, 0, 2, **{GX: 3})),
        "bf16": E("presplit !lean %s !lnbwd has_norm !tbias !has_res_conv !dx_planes" % _CNX_OFF, W(1, 0, 0, 2, **{GX: 4}))}, "ConvNextBlockFn"),
    # -- output through dest: the first half of a CatBuf (same route as cnx_wide_512)
    Case("cnx_wide_dest", _CNX, lambda: R.convnext(64, 128, 2, 16, dest=True), {
        "f32": E("!presplit !lean %s !lnbwd has_norm tbias has_res_conv !dx_planes" % _CNX_OFF, W(0, 0, 0, 3)),
        "bf16x3": E("presplit lean %s lnbwd has_norm tbias has_res_conv dx_planes" % _CNX_OFF, W(1, 2, 0, 1, **{GX: 3, GB: 2})),
        "bf16": E("presplit lean %s !lnbwd has_norm tbias has_res_conv !dx_planes" % _CNX_OFF, W(1, 2, 0, 1, **{GX: 4, GB: 2}))}, "ConvNextBlockFn"),
    # -- two blocks in a row: the second one's data gradient arrives with its planes (one cdf_split_bf16 for the two blocks) unless the
    #    tensor between them is marked _cdf_grad_f32 (two)
    Case("cnx_chain", _CNX, lambda: R.convnext_chain(2, 16), {
        "f32": E("!presplit !dx_planes", W(0, 0, 0, 4)),
        "bf16x3": E("presplit lean lnbwd dx_planes", W(1, 4, 0, 0, cdf_dwconv7_planes=2)),
        "bf16": E("presplit lean !lnbwd !dx_planes", W(2, 4, 0, 0))}, "ConvNextBlockFn"),
    Case("cnx_chain_marked", _CNX, lambda: R.convnext_chain(2, 16, mark=True), {
        "bf16x3": E("presplit lean lnbwd dx_planes", W(2, 4, 0, 0, cdf_dwconv7_planes=1))}, "ConvNextBlockFn"),

    # -- linear attention, default seams (_ATTN_FUSED = 1, _ATTN_QFOLD = True)
    Case("la64_512", "LinAttnBlockFn", lambda: R.linattn(64, 2, 16), {
        "f32": E("fused qfold !kv_planes !kvctx !unfused_kv", {SPLIT: 0, WX: 0, WB: 0}, has=["cdf_linattn_context", "cdf_linattn_bwd_kv"]),
        "bf16x3": E("fused qfold kv_planes kvctx !unfused_kv", {SPLIT: 0, WX: 1, WB: 0, GX: 1}, has=["cdf_layernorm_c_bwd_planes"],
                    no=["cdf_linattn_context", "cdf_linattn_bwd_kv"]),
        "bf16": E("fused qfold kv_planes kvctx !unfused_kv", {SPLIT: 0, WX: 1, WB: 0, GX: 1}, has=["cdf_layernorm_c_bwd"],
                  no=["cdf_linattn_context", "cdf_linattn_bwd_kv", "cdf_layernorm_c_bwd_planes"])}, "LinAttnBlockFn"),
    Case("la64_256", "LinAttnBlockFn", lambda: R.linattn(64, 1, 16), {
        "f32": E("fused qfold !kv_planes !kvctx !unfused_kv", {SPLIT: 0, WX: 0, WB: 0, GB: 0}),
        "bf16x3": E("fused qfold !kv_planes kvctx !unfused_kv", {SPLIT: 0, WX: 0, WB: 0, GX: 0, GB: 1}, has=["cdf_linattn_bwd_kv"], no=["cdf_linattn_context"]),
        "bf16": E("fused qfold !kv_planes kvctx !unfused_kv", {SPLIT: 0, WX: 0, WB: 0, GX: 0, GB: 1}, has=["cdf_linattn_bwd_kv"], no=["cdf_linattn_context"])},
         "LinAttnBlockFn"),
    # (n = 144 is no multiple of 128: the k | v projection is a GEMM of its own + linattn_context(koff = 0), with the planes on)
    Case("la64_576", "LinAttnBlockFn", lambda: R.linattn(64, 4, 12), {
        "f32": E("fused qfold !kv_planes !kvctx !unfused_kv", {SPLIT: 0, WX: 0, WB: 0, GB: 0}),
        "bf16x3": E("fused qfold kv_planes !kvctx !unfused_kv", {SPLIT: 0, WX: 1, WB: 0, GX: 1, GB: 1}, has=["cdf_linattn_context"], no=["cdf_linattn_bwd_kv"]),
        "bf16": E("fused qfold kv_planes !kvctx !unfused_kv", {SPLIT: 0, WX: 1, WB: 0, GX: 1, GB: 1}, has=["cdf_linattn_context"], no=["cdf_linattn_bwd_kv"])},
         "LinAttnBlockFn"),
    Case("la96_512", "LinAttnBlockFn", lambda: R.linattn(96, 2, 16), {
        "f32": E("fused qfold !kv_planes !kvctx !unfused_kv", {WX: 0, WB: 0}),
        "bf16x3": E("fused qfold kv_planes kvctx !unfused_kv", {SPLIT: 0, WX: 1, WB: 0, GX: 1}),
        "bf16": E("fused qfold kv_planes kvctx !unfused_kv", {SPLIT: 0, WX: 1, WB: 0, GX: 1})}, "LinAttnBlockFn"),
    Case("la128_512", "LinAttnBlockFn", lambda: R.linattn(128, 2, 16), {                    # dim == heads * 32: still folded
        "f32": E("fused qfold !kv_planes !kvctx !unfused_kv", {WX: 0, WB: 0}),
        "bf16x3": E("fused qfold kv_planes kvctx !unfused_kv", {SPLIT: 0, WX: 1, WB: 0, GX: 1}),
        "bf16": E("fused qfold kv_planes kvctx !unfused_kv", {SPLIT: 0, WX: 1, WB: 0, GX: 1})}, "LinAttnBlockFn"),
    Case("la160_128", "LinAttnBlockFn", lambda: R.linattn(160, 2, 8), {                     # above: plain form, dense to_out
        "f32": E("!fused !qfold !kv_planes !kvctx !unfused_kv", {WX: 0, WB: 0, GB: 0}, has=["cdf_linattn_bwd_kv"]),
        "bf16x3": E("!fused !qfold !kv_planes !kvctx !unfused_kv", {SPLIT: 0, WX: 0, WB: 0, GX: 0, GB: 4}, has=["cdf_linattn_bwd_kv", "cdf_layernorm_c_bwd_planes"]),
        "bf16": E("!fused !qfold !kv_planes !kvctx !unfused_kv", {SPLIT: 0, WX: 0, WB: 0, GX: 0, GB: 4}, has=["cdf_linattn_bwd_kv", "cdf_layernorm_c_bwd"])},
         "LinAttnBlockFn"),
    Case("la16_288", "LinAttnBlockFn", lambda: R.linattn(16, 2, 12), {                      # folded, no planes, exact-fp32 k | v GEMM
        m: E("fused qfold !kv_planes !kvctx !unfused_kv", {SPLIT: 0, WX: 0, WB: 0, GX: 0, GB: 0}, has=["cdf_linattn_context", "cdf_linattn_bwd_kv"])
        for m in MODES}, "LinAttnBlockFn"),
    # (ops._ATTN_KV_FUSED off on the plain form: the unfused softk / dk backward; at 512 pixels the 160- and 128-wide weight gradients
    #  are the in-kernel-split kernel's)
    Case("la160_512_kvsplit", "LinAttnBlockFn", lambda: R.linattn(160, 2, 16, seams=[("ops", "_ATTN_KV_FUSED", False)]), {
        "f32": E("!fused !qfold !kv_planes !kvctx unfused_kv", {WX: 0, WB: 0}, no=["cdf_linattn_bwd_kv"]),
        "bf16x3": E("!fused !qfold !kv_planes !kvctx unfused_kv", {SPLIT: 0, WX: 0, WB: 2, GB: 4}, no=["cdf_linattn_bwd_kv"]),
        "bf16": E("!fused !qfold !kv_planes !kvctx unfused_kv", {SPLIT: 0, WX: 0, WB: 2, GB: 4}, no=["cdf_linattn_bwd_kv"])}, "LinAttnBlockFn"),
    Case("la64_dest", "LinAttnBlockFn", lambda: R.linattn(64, 2, 16, dest=True), {          # dest.second()
        "f32": E("fused qfold !kv_planes !kvctx !unfused_kv", {WX: 0, WB: 0}),
        "bf16x3": E("fused qfold kv_planes kvctx !unfused_kv", {SPLIT: 0, WX: 1, WB: 0, GX: 1}),
        "bf16": E("fused qfold kv_planes kvctx !unfused_kv", {SPLIT: 0, WX: 1, WB: 0, GX: 1})}, "LinAttnBlockFn"),

    # -- single dense convs
    Case("down64", "ConvFn", lambda: R.conv("down", 64, 2, 32), {                           # 4 x 4 stride 2 on planes; 2 x 16 x 16 output pixels
        "f32": E("!presplit", W(0, 0, 0, 1)), "bf16x3": E("presplit", W(2, 1, 0, 0, **{GX: 2})), "bf16": E("presplit", W(2, 1, 0, 0, **{GX: 2}))}, "ConvFn"),
    Case("up64", "ConvFn", lambda: R.conv("up", 64, 2, 16), {
        "f32": E("!presplit", W(0, 0, 0, 1)), "bf16x3": E("presplit", W(2, 1, 0, 0, **{GX: 2})), "bf16": E("presplit", W(2, 1, 0, 0, **{GX: 2}))}, "ConvFn"),
    Case("down16", "ConvFn", lambda: R.conv("down", 16, 2, 12), {m: E("!presplit", W(0, 0, 0, 1, **{GB: 0, GF: 2})) for m in MODES}, "ConvFn"),
    Case("up16", "ConvFn", lambda: R.conv("up", 16, 2, 6), {m: E("!presplit", W(0, 0, 0, 1, **{GB: 0, GF: 2})) for m in MODES}, "ConvFn"),
    Case("final_1x1", "ConvFn", lambda: R.conv("final", 64, 2, 12), {m: E("!presplit", W(0, 0, 0, 1, **{GB: 0, GF: 2})) for m in MODES}, "ConvFn"),
    Case("join", "Join ConvFn LinAttnBlockFn", lambda: R.join(2), {
        "f32": E("!presplit fused qfold !kv_planes !kvctx", {WX: 0, WB: 0}),
        "bf16x3": E("presplit fused qfold kv_planes kvctx", {WX: 1, WB: 0}),               # (the attention block's; the up conv has 128 input pixels)
        "bf16": E("presplit fused qfold kv_planes kvctx", {WX: 1, WB: 0})}, "ConvFn"),

    # -- the DDPM `Model` family
    Case("res_64_128_512", "ResnetBlockFn Act Linear", lambda: R.resnet(64, 128, 2, 16), {
        "f32": E("!presplit !lean", W(0, 0, 0, 3, **{GB: 0})),
        "bf16x3": E("presplit lean", W(2, 2, 0, 1, **{GX: 4, GB: 2})), "bf16": E("presplit lean", W(2, 2, 0, 1, **{GX: 4, GB: 2}))}, "Model"),
    Case("res_64_128_256", "ResnetBlockFn Act Linear", lambda: R.resnet(64, 128, 1, 16), {
        "f32": E("!presplit !lean", W(0, 0, 0, 3)),
        "bf16x3": E("presplit !lean", W(2, 0, 0, 3, **{GX: 4, GB: 2})), "bf16": E("presplit !lean", W(2, 0, 0, 3, **{GX: 4, GB: 2}))}, "Model"),
    Case("res_64_64_512", "ResnetBlockFn Act Linear", lambda: R.resnet(64, 64, 2, 16), {
        "f32": E("!presplit !lean", W(0, 0, 0, 2), has=["cdf_axpby"]),
        "bf16x3": E("presplit lean", W(2, 2, 0, 0, **{GX: 4, GB: 0}), has=["cdf_axpby"]),
        "bf16": E("presplit lean", W(2, 2, 0, 0, **{GX: 4, GB: 0}), has=["cdf_axpby"])}, "Model"),
    # (q / k / v / proj_out are 64 -> 64 1 x 1 convs: in-kernel split forward and data gradient, exact-fp32 weight gradients --
    #  four of them plus the two batched transposed products)
    Case("attn64_8", "AttnBlockFn", lambda: R.attn(64, 2, 8), {
        "f32": E("!presplit", W(0, 0, 0, 6, **{GB: 0})), "bf16x3": E("!presplit", W(0, 0, 0, 6, **{GB: 8})), "bf16": E("!presplit", W(0, 0, 0, 6, **{GB: 8}))}, "Model"),
    Case("attn64_16", "AttnBlockFn", lambda: R.attn(64, 2, 16), {
        "f32": E("!presplit", W(0, 0, 0, 6, **{GB: 0})), "bf16x3": E("!presplit", W(0, 0, 0, 6, **{GB: 8})), "bf16": E("!presplit", W(0, 0, 0, 6, **{GB: 8}))}, "Model"),
    Case("upconv64", "UpsampleConvFn", lambda: R.upsample_conv(64, 2, 8), {                  # nearest x 2 -> 3 x 3 at 512 pixels
        "f32": E("!presplit", W(0, 0, 0, 1), has=["cdf_upsample2", "cdf_upsample2_bwd"]),
        "bf16x3": E("presplit", W(3, 1, 0, 0, **{GX: 2})), "bf16": E("presplit", W(3, 1, 0, 0, **{GX: 2}))}, "Model"),
    Case("avgpool16", "AvgPool2Fn", lambda: R.resample("pool", 16, 2, 12), {m: E("", has=["cdf_pool2d", "cdf_upsample2", "cdf_scale"]) for m in MODES}, "Model"),
    Case("upsample2_16", "Upsample2Fn", lambda: R.resample("up", 16, 2, 6), {m: E("", has=["cdf_upsample2", "cdf_upsample2_bwd"]) for m in MODES}, "Model"),
    Case("gn64", "GroupNormFn", lambda: R.groupnorm(64, 2, 12, False), {m: E("", has=["cdf_groupnorm_fwd_ex", "cdf_groupnorm_bwd_ex"]) for m in MODES}, "Model"),
    Case("gn64_silu", "GroupNormFn", lambda: R.groupnorm(64, 2, 12, True), {m: E("", has=["cdf_groupnorm_fwd_ex", "cdf_groupnorm_bwd_ex"]) for m in MODES}, "Model"),

    # -- the bf16 stream (mode "bf16", bf16 tensors in and out): every GEMM is the pre-split kernel's _io form on the tensors themselves
    Case("bf_cnx_wide_512", "ConvNextBlockBF Act Linear", lambda: R.convnext_bf(64, 128, 2, 16), {
        "bf16": E("presplit has_norm tbias has_res_conv", W(0, 3, 0, 0, **{GXIO: 6, GX: 0, GB: 0, GF: 0}), has=["cdf_dwconv7_io", "cdf_layernorm_c_bwd_io"])}, "bf16 stream"),
    Case("bf_cnx_same_512", "ConvNextBlockBF Act Linear", lambda: R.convnext_bf(64, 64, 2, 16), {
        "bf16": E("presplit has_norm tbias !has_res_conv", W(0, 2, 0, 0, **{GXIO: 4, GX: 0, GB: 0, GF: 0}))}, "bf16 stream"),
    Case("bf_enter", "ConvNextBlockBF ConvNextBlockFn ToF32 ToNHWC ToNCHW", lambda: R.enter_bf(2, 16), {
        "bf16": E("presplit lean cin4 res4 has_norm tbias", W(3, 3, 0, 0, **{GXIO: 4, GX: 2}), has=["cdf_bf16_to_f32"])}, "bf16 stream"),
    Case("bf_la64_512", "LinAttnBlockBF", lambda: R.linattn(64, 2, 16, bf=True), {           # kv_planes (hi only) + kvctx
        "bf16": E("fused qfold kv_planes kvctx !unfused_kv", {WX: 1, WB: 0, GXIO: 0, GX: 1}, has=["cdf_layernorm_c_fwd_io", "cdf_layernorm_c_bwd_io"],
                  no=["cdf_linattn_context"])}, "bf16 stream"),
    Case("bf_la64_256", "LinAttnBlockBF", lambda: R.linattn(64, 1, 16, bf=True), {
        "bf16": E("fused qfold !kv_planes kvctx !unfused_kv", {WX: 0, WB: 0, GX: 0, GB: 1}, has=["cdf_linattn_bwd_kv"])}, "bf16 stream"),
    Case("bf_la160_128", "LinAttnBlockBF", lambda: R.linattn(160, 2, 8, bf=True), {          # fp32 inside, rounded back into the stream
        "bf16": E("!fused !qfold !kv_planes !kvctx !unfused_kv", {WX: 0, WB: 0, GX: 0, GB: 4}, has=["cdf_bf16_to_f32", SPLIT])}, "bf16 stream"),
    Case("bf_down64", "ConvFnBF", lambda: R.conv("down", 64, 2, 32, bf=True), {
        "bf16": E("presplit", W(0, 1, 0, 0, **{GXIO: 2, GX: 0}))}, "bf16 stream"),
    Case("bf_up64", "ConvFnBF", lambda: R.conv("up", 64, 2, 16, bf=True), {
        "bf16": E("presplit", W(0, 1, 0, 0, **{GXIO: 2, GX: 0}))}, "bf16 stream"),
    Case("bf_join", "JoinBF ToF32 ConvFnBF LinAttnBlockBF ToNCHW", lambda: R.join(2, bf=True), {
        "bf16": E("presplit fused qfold kv_planes kvctx", {WX: 1, WB: 0, GXIO: 2}, has=["cdf_bf16_to_f32"])}, "bf16 stream"),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
PARAMS = [pytest.param(c.name, m, id="%s-%s" % (c.name, m)) for c in CASES for m in MODES if m in c.routes]

# Function classes that no case here runs, and the test that does
COVERED_ELSEWHERE = {
    "Sinusoidal": "tests/test_modules.py::test_unet_golden",          # the time embedding of the whole network, against the reference's vectors
    "TimeBiasAll": "tests/test_modules.py::test_unet_golden",         # every block's time bias in one launch, ditto (and tests/test_bf16_storage.py)
}

# ---------------------------------------------------------------------------------------------------------------------------------------
# running a case
# ---------------------------------------------------------------------------------------------------------------------------------------
_RIGS = {}


def rig_of(name):
    """The case's rig and its fp64 reference: built once per process, shared by every mode and paired test, never modified."""
    if name not in _RIGS:
        rig = BY_NAME[name].build()
        _RIGS[name] = (rig, rig.reference())
    return _RIGS[name]


@contextlib.contextmanager
def seams(pairs):
    """[(module name, attribute, value)] set while a case runs: the test / tool seams of colddiff.functions / colddiff.ops."""
    from colddiff import functions, ops
    mods = {"functions": functions, "ops": ops}
    saved = [(mods[m], a, getattr(mods[m], a)) for m, a, _ in pairs]
    for m, a, v in pairs:
        setattr(mods[m], a, v)
    try:
        yield
    finally:
        for obj, a, v in saved:
            setattr(obj, a, v)


def run_once(rig, mods, dev):
    for p in mods.parameters():
        p.grad = None
    out = rig.run(mods, dev)
    for n, p in mods.named_parameters():
        assert p.grad is not None, ("no gradient", n)
        out["grad/" + n] = p.grad.detach().cpu().clone()
    return out


_PLAIN = {}          # (case, mode, backend) -> (results, calls) of the case as the table states it: the paired tests below take it from here


def run_case(name, mode, mbe, extra_seams=(), twice=False):  # noqa: F811
    """(results of the first pass, recorded calls) of the case in `mode`; twice: once more from the same state on poisoned allocations,
    which must give the same bits."""
    import copy
    from colddiff import runtime as rt
    key = (name, mode, mbe.kind)
    if not extra_seams and not twice and key in _PLAIN:
        return _PLAIN[key]
    rig, _ = rig_of(name)
    mods = copy.deepcopy(rig.mods).to(mbe.device)
    with _precision(mode), seams(list(rig.seams) + list(extra_seams)):
        rt.tuning()
        with Recorder(rt.lib()) as rec:
            first = run_once(rig, mods, mbe.device)
        if twice:
            with poisoned_allocations():
                second = run_once(rig, mods, mbe.device)
            assert first.keys() == second.keys()
            for k in first:
                assert torch.isfinite(first[k]).all(), (name, mode, k, "not finite")
                assert torch.equal(first[k], second[k]), (name, mode, k, "second (poisoned) pass differs", (first[k] - second[k]).abs().max().item())
    if not extra_seams:
        _PLAIN[key] = (first, rec.calls)
    return first, rec.calls


# AttnBlock's k.bias has NO gradient in exact arithmetic: a constant added to every key shifts each row of q k^T by a constant, which the
# softmax removes.  Its fp64 reference is rounding residue (~1e-16), so |ref|max is no scale for it; what the kernels return is the fp32
# rounding of a sum over every pixel of dk rows that cancel.  It is compared on the scale of q.bias's gradient, the same sum over the same
# pixels of dq rows (fp32 torch autograd itself leaves 3e-6 .. 8e-6 there on these cases, against the 1e-4 * 1e-3 = 1e-7 floor).
ZERO_BY_SYMMETRY = {"grad/k.bias": "grad/q.bias"}


def bound_of(key, ref, mode):
    from colddiff import runtime as rt
    rmax = ref[ZERO_BY_SYMMETRY.get(key, key)].abs().max().item()
    if mode == "bf16":
        return rt.BF16_TOLERANCE["grad_rel_of_tensor_max"] * rmax
    return 1e-4 * (max(rmax, 1e-3) if key.startswith("grad/") else rmax)


def worst_ratio(got, ref, mode, tag):
    assert got.keys() == ref.keys(), (tag, sorted(set(got) ^ set(ref)))
    worst, where = 0.0, None
    for k, r in ref.items():
        assert got[k].shape == r.shape, (tag, k, got[k].shape, r.shape)
        ratio = (got[k].double() - r).abs().max().item() / bound_of(k, ref, mode)
        if ratio > worst:
            worst, where = ratio, k
    return worst, where


@pytest.mark.parametrize("name,mode", PARAMS)
def test_block_route_and_reference(mbe, name, mode):  # noqa: F811
    """One case in one arithmetic mode: second (poisoned) pass bit-identical, the expected route taken, output and every gradient within
    the mode's bound of the fp64 reference (module docstring)."""
    case = BY_NAME[name]
    t0 = time.time()
    got, calls = run_case(name, mode, mbe, twice=True)
    case.routes[mode].check(calls, (name, mode))
    worst, where = worst_ratio(got, rig_of(name)[1], mode, (name, mode))
    print("ROUTE-RATIO %-18s %-6s %s  worst error/bound %.3f at %s  (%.1f s)" % (name, mode, mbe.kind, worst, where, time.time() - t0))
    assert worst <= 1.0, (name, mode, where, worst)


# ---------------------------------------------------------------------------------------------------------------------------------------
# paired runs: two forms of the same block must agree bit for bit
# ---------------------------------------------------------------------------------------------------------------------------------------
def _equal(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k, (a[k] - b[k]).abs().max().item())


def _count(calls, name):
    return sum(1 for n, _ in calls if n == name)


@pytest.mark.parametrize("name,mode", [("cnx_wide_512", "bf16x3"), ("cnx_wide_512", "bf16"), ("cnx_img_512", "bf16x3"), ("res_64_128_512", "bf16x3"),
                                       ("res_64_128_512", "bf16")])
def test_lean_only_omits_fp32_copies(mbe, name, mode):  # noqa: F811
    """functions._LEAN on against off at 512 pixels: the lean form skips the fp32 copies of tensors whose every consumer reads the
    bf16 planes and chooses no other kernel, so output and every gradient are bit-identical."""
    lean, calls_on = run_case(name, mode, mbe)
    full, calls_off = run_case(name, mode, mbe, extra_seams=[("functions", "_LEAN", False)])
    assert ROUTE_FLAGS["lean"](calls_on) and not ROUTE_FLAGS["lean"](calls_off)
    assert [n for n, _ in calls_on] == [n for n, _ in calls_off], "the lean form launched other kernels"
    _equal(lean, full, (name, mode, "_LEAN"))


@pytest.mark.parametrize("name", ["cnx_chain", "cnx_wide_512", "la64_512", "join"])
def test_grad_planes_on_and_off(mbe, name):  # noqa: F811
    """ops.GRAD_PLANES off: gradients travel as fp32 only and the consumer splits them itself -- same planes, same bits."""
    on, calls_on = run_case(name, "bf16x3", mbe)
    off, calls_off = run_case(name, "bf16x3", mbe, extra_seams=[("ops", "GRAD_PLANES", False)])
    assert not _has(calls_off, "cdf_dwconv7_planes", "cdf_layernorm_c_bwd_planes")
    assert _has(calls_on, "cdf_dwconv7_planes", "cdf_layernorm_c_bwd_planes")
    if name == "cnx_chain":                                   # the planes were really taken: one split fewer
        assert _count(calls_off, SPLIT) == _count(calls_on, SPLIT) + 1
    _equal(on, off, (name, "GRAD_PLANES"))


def test_marked_input_keeps_the_gradient_fp32(mbe):  # noqa: F811
    """A block whose input carries `_cdf_grad_f32` writes no planes of its data gradient (ctx.dx_planes off); the block before it then
    splits that gradient itself: one more cdf_split_bf16, same bits."""
    plain, calls_p = run_case("cnx_chain", "bf16x3", mbe)
    marked, calls_m = run_case("cnx_chain_marked", "bf16x3", mbe)
    assert _count(calls_p, "cdf_dwconv7_planes") == 2 and _count(calls_m, "cdf_dwconv7_planes") == 1
    assert _count(calls_m, SPLIT) == _count(calls_p, SPLIT) + 1
    _equal(plain, marked, "_cdf_grad_f32")


@pytest.mark.parametrize("name", ["cnx_wide_512", "cnx_wide_256"])
def test_pre_grad_on_and_off(mbe, name):  # noqa: F811
    """functions._PRE_GRAD on the wide fp32 block in "bf16x3": conv1's epilogue stores GELU'(pre) and conv2's data gradient multiplies
    by it (mul_mode 3) instead of evaluating it from the stored pre-activation (mul_mode 1).  Same erf / exp evaluation: bit-identical."""
    off, calls_off = run_case(name, "bf16x3", mbe)
    on, calls_on = run_case(name, "bf16x3", mbe, extra_seams=[("functions", "_PRE_GRAD", True)])
    mul_mode = lambda calls: sorted({a[32] for a in _args(calls, GX) if a[29]})          # (arguments 29 / 32: mul pointer, mul_mode)
    assert mul_mode(calls_off) == [1] and mul_mode(calls_on) == [3], (mul_mode(calls_off), mul_mode(calls_on))
    _equal(on, off, (name, "_PRE_GRAD"))


@pytest.mark.parametrize("name,plain", [("cnx_wide_dest", "cnx_wide_512"), ("la64_dest", "la64_512")])
@pytest.mark.parametrize("mode", MODES)
def test_dest_equals_plain(mbe, name, plain, mode):  # noqa: F811
    """Writing the output in place into its half of a CatBuf changes nothing but the pitch (the rig itself checks that the other half
    of the buffer is untouched)."""
    a, _ = run_case(name, mode, mbe)
    b, _ = run_case(plain, mode, mbe)
    _equal(a, b, (name, mode))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the table itself
# ---------------------------------------------------------------------------------------------------------------------------------------
def _function_classes():
    from colddiff import bf16store, functions
    out = set()
    for mod in (functions, bf16store):
        for n, obj in inspect.getmembers(mod, inspect.isclass):
            if issubclass(obj, torch.autograd.Function) and obj.__module__ == mod.__name__:
                out.add(n)
    return out


def table_gaps(cases):
    """What the literal expectations of `cases` leave uncovered (empty: complete)."""
    gaps = []
    seen = {f: set() for f in GUARDED_FLAGS}
    wgrad = {WX: 0, WB: 0, WF: 0}
    for c in cases:
        for mode, e in c.routes.items():
            if mode == "f32":
                continue
            for f, v in e.flags.items():
                if f in seen:
                    seen[f].add(v)
            for k in wgrad:
                wgrad[k] += e.n.get(k, 0)
    gaps += ["flag %s never %s" % (f, "on" if v else "off") for f in GUARDED_FLAGS for v in (True, False) if v not in seen[f]]
    gaps += ["no case expects %s" % k for k, v in wgrad.items() if v == 0]
    named = {n for c in cases for n in c.classes} | set(COVERED_ELSEWHERE)
    gaps += ["Function class %s is in no case" % n for n in sorted(_function_classes() - named)]
    return gaps


def test_case_table_is_complete():
    """Each guarded route flag is expected on AND off somewhere in the table in a mode other than "f32", each of the three
    weight-gradient kernels is expected somewhere, and every autograd Function class of functions.py / bf16store.py is named by a case
    (or ticked off in COVERED_ELSEWHERE).  Dropping the only holder of a value must show as a gap."""
    assert table_gaps(CASES) == []
    assert {n for c in CASES for n in c.classes} <= _function_classes(), "a case names a class that does not exist"
    for test_id in COVERED_ELSEWHERE.values():                # (the ticked-off tests exist)
        path, fn = test_id.split("::")
        import os
        src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), path)).read()
        assert "def %s(" % fn in src, test_id
    # the guard has teeth: without the only case on the unfused k / v backward, or the only one below the fold boundary on planes ...
    assert "flag unfused_kv never on" in table_gaps([c for c in CASES if c.name != "la160_512_kvsplit"])
    assert any("kvctx never off" in g for g in table_gaps([c for c in CASES if c.name not in ("la64_576", "la160_128", "la16_288", "la160_512_kvsplit", "bf_la160_128")]))
    for m in MODES:                                           # every fp32-tensor case runs in every mode; the stream in "bf16" only
        assert all((m in c.routes) == (m == "bf16") for c in CASES if c.family == "bf16 stream")
    assert all(set(c.routes) == set(MODES) for c in CASES if c.family != "bf16 stream" and c.name != "cnx_chain_marked")
