"""Run-to-run invariance on the MI355X: the library uses no atomics, sums its split-K slabs and partial sums in a fixed order and
promises bit-identical results for identical inputs (data-parallel replicas stay bit-identical).  The simulator runs one
lane at a time, so a missing barrier or an LDS write-after-read hazard can only show here.  Every check compares with torch.equal:
  * the benchmark's fused 64-image step at 128 x 128, twice (bf16x3 and bf16 modes), once more on NaN-poisoned allocations, and once
    with the resident row-halo grid every multi-rank step launches (resident_reserve = 32);
  * the sampler at B = 16, 128 x 128 (5 reverse steps) and BASELINE config 2's network at 32 x 32, B = 128: twice and under poison;
  * a coverage guard: every cdf_* entry point the bench step and a sampler step call must name its production-shape test below.
"""
import contextlib
import io

import pytest
import torch

from poison import poisoned_allocations
from test_gpu_parity2 import _fused_bench_step, bench_step_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


class Recorder:
    """Wraps every cdf_* attribute of the loaded library (the way bench.py's GemmTimer wraps the GEMM entry points) and records
    the name and arguments of each call while active."""

    def __init__(self, lib):
        self.lib, self.calls, self.orig = lib, [], {}

    def __enter__(self):
        for name in list(vars(self.lib)):
            if name.startswith("cdf_"):
                fn = self.orig[name] = getattr(self.lib, name)
                setattr(self.lib, name, (lambda n, f: lambda *a: (self.calls.append((n, a)), f(*a))[1])(name, fn))
        return self

    def __exit__(self, *exc):
        for name, fn in self.orig.items():
            setattr(self.lib, name, fn)

    def names(self):
        return {n for n, _ in self.calls}


@pytest.fixture(scope="module")
def bench_data():
    return bench_step_inputs()


def _step(f):
    """loss + every parameter gradient of one fused bench step, on the host."""
    from colddiff import runtime as rt
    rt.bump_weights_epoch()
    tr, net, loss = _fused_bench_step(f)
    out = [torch.tensor([loss])] + [p.grad.detach().cpu().clone() for p in net.parameters()]
    del tr, net
    return out


def _same(a, b, what):
    assert len(a) == len(b)
    for i, (u, v) in enumerate(zip(a, b)):
        assert torch.isfinite(u).all(), (what, i)
        assert torch.equal(u, v), (what, i, (u - v).abs().max().item())


@contextlib.contextmanager
def _reserve(n):
    from colddiff import runtime as rt
    saved = rt.tuning().get("resident_reserve")
    rt.tuning().set(resident_reserve=n)
    try:
        yield
    finally:
        rt.tuning().set(resident_reserve=saved)


@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
def test_bench_step_twice_poisoned_and_reserved_bit_identical(bench_data, mode):
    """The bench step from the same state: twice, then on poisoned allocations, then on the resident grid of a multi-rank step
    (resident_reserve = 32 CUs left free: fewer resident blocks, each walking more tiles).  Each tile is computed by one block in a
    fixed K order whatever the grid, so all four must agree bit for bit."""
    from colddiff import runtime as rt
    with rt.precision_scope(mode):
        with _reserve(0):
            first = _step(bench_data)
            second = _step(bench_data)
            with poisoned_allocations():
                poisoned = _step(bench_data)
        with _reserve(32):
            reserved = _step(bench_data)
    _same(first, second, "second run")
    _same(first, poisoned, "poisoned run")
    _same(first, reserved, "resident_reserve=32")
    print(mode, "bench step: loss", first[0].item(), "-- second run, poisoned run and resident_reserve=32 bit-identical")


def _sampler_run(sd, noise):
    from denoising_diffusion_pytorch import GaussianDiffusion, Unet
    from colddiff import runtime as rt
    rt.bump_weights_epoch()
    net = quiet(Unet, dim=64, dim_mults=(1, 2, 4, 8), channels=3)
    net.load_state_dict(sd)
    d = GaussianDiffusion(net.to(DEV), image_size=128, channels=3, timesteps=5, sampling_routine="x0_step_down").to(DEV)
    with torch.no_grad():
        out = [v.detach().cpu().clone() for v in quiet(d.gen_sample, batch_size=noise.shape[0], img=noise.to(DEV))]
    torch.cuda.synchronize()
    return out


def test_sampler_twice_and_poisoned_bit_identical(bench_data):
    """gen_sample at B = 16, 128 x 128, 5 reverse steps (the sampler's shapes): twice, and once on poisoned allocations."""
    torch.manual_seed(4)
    noise = torch.randn(16, 3, 128, 128)
    first = _sampler_run(bench_data["sd"], noise)
    second = _sampler_run(bench_data["sd"], noise)
    with poisoned_allocations():
        poisoned = _sampler_run(bench_data["sd"], noise)
    _same(first, second, "second run")
    _same(first, poisoned, "poisoned run")


def _config2_runner():
    """BASELINE config 2: Model(ch=128, (1, 2, 2, 2), 2 res blocks, attention at 16 x 16, dropout 0.1) at 32 x 32, B = 128: a function that
    runs forward + backward from the same state and returns output, input gradient and every parameter gradient."""
    from deblurring_diffusion_pytorch import Model
    from colddiff import runtime as rt
    kw = dict(resolution=32, in_channels=3, out_ch=3, ch=128, ch_mult=(1, 2, 2, 2), num_res_blocks=2, attn_resolutions=(16,), dropout=0.1)
    torch.manual_seed(21)
    sd = quiet(Model, **kw).state_dict()
    x, t, gy = torch.rand(128, 3, 32, 32) * 2 - 1, torch.randint(0, 1000, (128,)), torch.randn(128, 3, 32, 32) / 1000

    def run():
        rt.bump_weights_epoch()
        net = Model(**kw)
        net.load_state_dict(sd)
        net = net.to(DEV)
        xd = x.to(DEV).requires_grad_(True)
        torch.manual_seed(5)
        y = net(xd, t.to(DEV))
        y.backward(gy.to(DEV))
        torch.cuda.synchronize()
        return [y.detach().cpu(), xd.grad.cpu()] + [p.grad.cpu().clone() for p in net.parameters()]
    return run


def test_config2_model_twice_and_poisoned_bit_identical():
    """BASELINE config 2 (see _config2_runner), forward + backward: twice and once on poisoned allocations (the dropout seed is drawn from
    torch's generator, reseeded per run)."""
    run = _config2_runner()
    first = run()
    second = run()
    with poisoned_allocations():
        poisoned = run()
    _same(first, second, "second run")
    _same(first, poisoned, "poisoned run")


# ------------------------------------------------------------------------------------------------------------------------------------
# coverage guard: every entry point on the hot path names the test(s) that run it at a production shape
# ------------------------------------------------------------------------------------------------------------------------------------
_KP = "test_kernels_production.py::"
_GP = "test_gemm_production.py::"
_K = "test_kernels.py::"
_P2 = "test_gpu_parity2.py::"
_BS = "test_gpu_invariance.py::test_bench_step_twice_poisoned_and_reserved_bit_identical"
COVERED_AT_PRODUCTION_SHAPE = {
    # GEMM family: the *_large GPU tests run the shapes the bench / configs launch; the step-level tests above run them in the step
    "cdf_conv_gemm": [_K + "test_conv_gemm_large", _K + "test_conv_presplit_large"],
    # ... and the pre-split family, form by form (test_coverage_guard below), in test_gemm_production.py
    "cdf_conv_gemm_bf16x": [_GP + "test_gemm_bench_forms", _K + "test_conv_presplit_large", _K + "test_specialised_epilogue_equals_generic_large"],
    "cdf_conv_gemm_bf16x_lnbwd": [_GP + "test_gemm_bench_forms", _K + "test_conv_dgrad_with_layernorm_backward_epilogue_large"],
    "cdf_conv_wgrad": [_GP + "test_wgrad_f32_995_slabs_two_empty", _K + "test_conv_gemm_large"],
    "cdf_conv_wgrad_bf16x": [_GP + "test_wgrad_bench_forms_and_split_counts", _K + "test_conv_presplit_large"],
    "cdf_split_bf16": [_K + "test_conv_presplit_large"],
    "cdf_bf16x_ksplit": [_K + "test_conv_presplit_large"],
    "cdf_wgrad_nsplit": [_KP + "test_unpack_reduce_bench_slab_counts"],
    "cdf_unpack_reduce": [_KP + "test_unpack_reduce_bench_slab_counts", _KP + "test_conv_cin4_first_block"],
    "cdf_unpack_reduce_bias": [_KP + "test_unpack_reduce_bench_slab_counts"],
    # image-side block
    "cdf_conv_cin4_fwd": [_KP + "test_conv_cin4_first_block"],
    "cdf_conv_cin4_dgrad": [_KP + "test_conv_cin4_first_block"],
    "cdf_conv_cin4_tapsum3": [_KP + "test_conv_cin4_first_block"],
    "cdf_conv_cin4_wgrad": [_KP + "test_conv_cin4_first_block"],
    "cdf_conv_cin4_nchunk": [_KP + "test_conv_cin4_first_block"],
    "cdf_pack_cin4": [_KP + "test_conv_cin4_first_block"],
    # reductions, norms, depthwise
    "cdf_colsum": [_KP + "test_colsum_past_chunk_cap"],
    "cdf_colsum_io": [_KP + "test_colsum_past_chunk_cap"],
    "cdf_colsum_nchunk": [_KP + "test_colsum_past_chunk_cap"],
    "cdf_layernorm_blocks": [_KP + "test_layernorm_production"],
    "cdf_layernorm_c_fwd": [_KP + "test_layernorm_production"],
    "cdf_layernorm_c_bwd": [_KP + "test_layernorm_production"],
    "cdf_layernorm_c_bwd_planes": [_KP + "test_layernorm_production"],
    "cdf_layernorm_c_fwd_io": [_KP + "test_layernorm_production"],
    "cdf_layernorm_c_bwd_io": [_KP + "test_layernorm_production"],
    "cdf_groupnorm_fwd_ex": [_KP + "test_groupnorm_production"],
    "cdf_groupnorm_bwd_ex": [_KP + "test_groupnorm_production"],
    "cdf_groupnorm_nchunk": [_KP + "test_groupnorm_production"],
    "cdf_dwconv7": [_KP + "test_dwconv7_production"],
    "cdf_dwconv7_planes": [_KP + "test_dwconv7_production"],
    "cdf_dwconv7_wgrad": [_KP + "test_dwconv7_production"],
    "cdf_dwconv7_wgrad_nchunk": [_KP + "test_dwconv7_production"],
    # linear attention
    "cdf_linattn_nsplit": [_KP + "test_linattn_production"],
    "cdf_linattn_ws_floats": [_KP + "test_linattn_production"],
    "cdf_linattn_context": [_KP + "test_linattn_production"],
    "cdf_linattn_dcontext": [_KP + "test_linattn_production"],
    "cdf_linattn_bwd_kv": [_KP + "test_linattn_production", _KP + "test_linattn_bwd_kv_planes_production"],
    "cdf_linattn_softk": [_KP + "test_linattn_production"],
    "cdf_linattn_dk": [_KP + "test_linattn_production"],
    # ... and the folded attention block's path, which the bench step takes
    "cdf_linattn_kvctx": [_KP + "test_linattn_kvctx_production"],
    "cdf_linattn_kvctx_parts": [_KP + "test_linattn_kvctx_production"],
    "cdf_linattn_finalize": [_KP + "test_linattn_kvctx_production"],
    "cdf_linattn_bwd_kv_planes": [_KP + "test_linattn_bwd_kv_planes_production"],
    "cdf_linattn_dctx_finish": [_KP + "test_linattn_dctx_finish_production"],
    "cdf_dwconv7_io": [_KP + "test_dwconv7_production"],
    "cdf_dwconv7_wgrad_io": [_KP + "test_dwconv7_production"],
    # the typed-operand GEMM entry points of the bf16 stream: cdf_conv_gemm / cdf_conv_gemm_bf16x ARE these entry points with io_bf16 = 0
    # (same tile walk and split; the flag changes only how operands are loaded and stored), so the *_large tests run their production
    # shapes; the bf16 step at the bench shape runs the bf16 operands
    "cdf_conv_gemm_io": [_K + "test_conv_gemm_large", _P2 + "test_bf16_mode_bench_shape_fused_step"],
    "cdf_conv_gemm_bf16x_io": [_GP + "test_gemm_bench_forms", _K + "test_conv_presplit_large", _P2 + "test_bf16_mode_bench_shape_fused_step"],
    # elementwise bf16 -> fp32 widening (exactness: test_bf16_storage.py::test_bf16_to_f32_and_back)
    "cdf_bf16_to_f32": [_P2 + "test_bf16_mode_bench_shape_fused_step", "test_bf16_storage.py::test_bf16_to_f32_and_back"],
    # the in-kernel-split GEMM pair (csrc/k_conv_sp.hip): the 1 x 1 projections and their gradients in BOTH arithmetic modes -- split = 3
    # under bf16x3, split = 1 under bf16 (form by form: test_gemm_sp_forms.py, appended below)
    "cdf_conv_gemm_bf16": [_K + "test_conv_gemm_bf16_large"],
    "cdf_conv_wgrad_bf16": [_K + "test_conv_gemm_bf16_large"],
    # elementwise and layout operations: the bench-shape step.  (They have no reduction or tile walk, but they are not free of a clamp that
    # depends on the shape: the k_misc.hip ones are grid-stride loops under a cap of 8192 blocks, and cdf_linear_small picks its 8- or
    # 32-row form by shape -- the tests that cross those are appended below.)
    **{n: [_P2 + "test_bench_shape_fused_step_vs_oracle", _BS] for n in (
        "cdf_act_fwd", "cdf_act_bwd", "cdf_loss_fwd", "cdf_loss_bwd", "cdf_nchw_to_nhwc", "cdf_nhwc_to_nchw", "cdf_noise_qsample",
        "cdf_sinusoidal", "cdf_linear_small", "cdf_linear_small_wgrad", "cdf_pack_weight", "cdf_pack_weight_bf16")},
    "cdf_noise_step": ["test_gpu_fullsize.py::test_sampler_full_T_denoise", "test_gpu_invariance.py::test_sampler_twice_and_poisoned_bit_identical"],
}
# ... and past their grid caps / on the 32-row side of cdf_linear_small's threshold
_SP = "test_small_kernels_production.py::"
for _name, _test in (("cdf_act_fwd", "test_act_past_grid_cap"), ("cdf_act_bwd", "test_act_past_grid_cap"),
                     ("cdf_sinusoidal", "test_sinusoidal_past_grid_cap"), ("cdf_linear_small", "test_linear_small_production"),
                     ("cdf_linear_small_wgrad", "test_linear_small_production")):
    COVERED_AT_PRODUCTION_SHAPE[_name].append(_SP + _test)
# the exact-fp32 GEMM pair: every tile, batched form, epilogue set and slab layout the product launches (test_coverage_guard holds the
# recordings against that module's form tables)
_FF = "test_gemm_f32_forms.py::"
COVERED_AT_PRODUCTION_SHAPE["cdf_conv_gemm"] += [_FF + "test_igemm_single_launch", _FF + "test_igemm_batched_call_sites"]
COVERED_AT_PRODUCTION_SHAPE["cdf_conv_gemm_io"] += [_FF + "test_igemm_single_launch", _FF + "test_igemm_batched_call_sites"]
COVERED_AT_PRODUCTION_SHAPE["cdf_conv_wgrad"] += [_FF + "test_wgrad_tiles_plans_splits", _FF + "test_wgrad_batched_and_head_split"]
# the in-kernel-split pair: every geometry, tile edge, epilogue path, layout and slab walk the product launches (test_coverage_guard holds
# the recordings against that module's form tables)
_SF = "test_gemm_sp_forms.py::"
COVERED_AT_PRODUCTION_SHAPE["cdf_conv_gemm_bf16"] += [_SF + "test_sp_gemm_forms"]
COVERED_AT_PRODUCTION_SHAPE["cdf_conv_wgrad_bf16"] += [_SF + "test_sp_wgrad_plans_and_splits"]
# the depthwise, LayerNorm and GroupNorm entry points: every pitch, null-pointer, accumulate and tile / chunk form the product launches
# (test_coverage_guard holds the recordings against that module's form tables)
_ND = "test_norm_dw_forms.py::"
for _names, _test in ((("cdf_dwconv7", "cdf_dwconv7_io", "cdf_dwconv7_planes"), "test_dwconv7_forms"),
                      (("cdf_dwconv7_wgrad", "cdf_dwconv7_wgrad_io", "cdf_dwconv7_wgrad_nchunk"), "test_dwconv7_wgrad_forms"),
                      (("cdf_layernorm_c_fwd", "cdf_layernorm_c_fwd_io", "cdf_layernorm_blocks"), "test_layernorm_fwd_forms"),
                      (("cdf_layernorm_c_bwd", "cdf_layernorm_c_bwd_io", "cdf_layernorm_c_bwd_planes", "cdf_layernorm_blocks"), "test_layernorm_bwd_forms"),
                      (("cdf_groupnorm_fwd_ex", "cdf_groupnorm_nchunk"), "test_groupnorm_fwd_forms"),
                      (("cdf_groupnorm_bwd_ex", "cdf_groupnorm_nchunk"), "test_groupnorm_bwd_forms")):
    for _name in _names:
        COVERED_AT_PRODUCTION_SHAPE[_name].append(_ND + _test)
# the FID extractor's launches of the two conv GEMM entry points, at the extractor's own shapes (test_coverage_guard holds a recording of
# the extractor against that module's form tables)
_IF = "test_inception_forms.py::"
COVERED_AT_PRODUCTION_SHAPE["cdf_conv_gemm_bf16"] += [_IF + "test_extractor_sp_forms", _IF + "test_extractor_sp_production_shapes"]
COVERED_AT_PRODUCTION_SHAPE["cdf_conv_gemm"] += [_IF + "test_extractor_f32_forms", _IF + "test_extractor_f32_production_shapes"]
# the image-side direct convolutions, the slab reductions and the column sums: every null-output, pitch, accumulate, stride and kernel /
# chunk form the product launches (test_coverage_guard holds the recordings against that module's form tables)
_SK = "test_side_kernel_forms.py::"
for _names, _test in ((("cdf_conv_cin4_fwd",), "test_cin4_fwd_forms"), (("cdf_conv_cin4_dgrad",), "test_cin4_dgrad_forms"),
                      (("cdf_conv_cin4_tapsum3",), "test_cin4_tapsum3_forms"), (("cdf_conv_cin4_wgrad", "cdf_conv_cin4_nchunk"), "test_cin4_wgrad_forms"),
                      (("cdf_unpack_reduce", "cdf_unpack_reduce_bias"), "test_unpack_reduce_forms"),
                      (("cdf_colsum", "cdf_colsum_io", "cdf_colsum_nchunk"), "test_colsum_forms")):
    for _name in _names:
        COVERED_AT_PRODUCTION_SHAPE[_name].append(_SK + _test)
# ... and linear attention and the attention block's row softmax (test_side_kernel_forms_attn.py), the same way
_SA = "test_side_kernel_forms_attn.py::"
for _names, _test in ((("cdf_linattn_context", "cdf_linattn_nsplit", "cdf_linattn_ws_floats"), "test_linattn_context_forms"),
                      (("cdf_linattn_dcontext",), "test_linattn_dcontext_forms"), (("cdf_linattn_bwd_kv", "cdf_linattn_bwd_kv_planes"), "test_linattn_bwd_kv_forms"),
                      (("cdf_linattn_kvctx", "cdf_linattn_kvctx_parts"), "test_linattn_kvctx_forms"),
                      (("cdf_linattn_finalize",), "test_linattn_finalize_forms"), (("cdf_linattn_dctx_finish",), "test_linattn_dctx_finish_forms"),
                      (("cdf_linattn_softk", "cdf_linattn_dk"), "test_linattn_softk_dk_forms")):
    for _name in _names:
        COVERED_AT_PRODUCTION_SHAPE[_name].append(_SA + _test)
for _name in ("cdf_softmax_rows_fwd", "cdf_softmax_rows_bwd"):
    COVERED_AT_PRODUCTION_SHAPE[_name] = [_SA + "test_softmax_rows_forms"]
# entry points with nothing shape-dependent to test at scale, with the reason
EXEMPT = {
    "cdf_last_error": "host-side error string",
    "cdf_zero": "memset-class fill; no reduction, tiling or chunk clamp",
    "cdf_gemm_tuning_default": "host-side defaults of the tuning struct",
    "cdf_abi_version": "host-side query",
    "cdf_is_device_build": "host-side query",
    "cdf_conv_gemm_bf16x_ksplit": "host-side query (split count)",
    "cdf_conv_gemm_bf16x_lnbwd_ok": "host-side query (epilogue eligibility)",
    "cdf_conv_wgrad_bf16x_is_row3": "host-side query (kernel form)",
    "cdf_conv_gemm_bf16x_form": "host-side query (kernel form: the dispatcher, stopped before the launch)",
    "cdf_conv_wgrad_bf16x_form": "host-side query (kernel form: the dispatcher, stopped before the launch)",
}


_SP_GEMM = ("cdf_conv_gemm_bf16", "cdf_conv_wgrad_bf16")     # the in-kernel-split pair: guarded form by form too (test_gemm_sp_forms.py)
_GEMM_FAMILY = ("cdf_conv_gemm_bf16x", "cdf_conv_gemm_bf16x_io", "cdf_conv_gemm_bf16x_lnbwd", "cdf_conv_wgrad_bf16x", "cdf_conv_wgrad") + _SP_GEMM
_F32_GEMM = ("cdf_conv_gemm", "cdf_conv_gemm_io")            # the exact-fp32 pair: guarded form by form too (test_gemm_f32_forms.py)
# the kernels between the GEMMs (csrc/k_dwconv.hip, csrc/k_norm.hip): guarded form by form too (test_norm_dw_forms.py); their calls are
# kept with the GEMM calls
_NORM_DW = ("cdf_dwconv7", "cdf_dwconv7_io", "cdf_dwconv7_planes", "cdf_dwconv7_wgrad", "cdf_dwconv7_wgrad_io", "cdf_layernorm_c_fwd",
            "cdf_layernorm_c_fwd_io", "cdf_layernorm_c_bwd", "cdf_layernorm_c_bwd_io", "cdf_layernorm_c_bwd_planes", "cdf_groupnorm_fwd",
            "cdf_groupnorm_fwd_ex", "cdf_groupnorm_bwd", "cdf_groupnorm_bwd_ex")
_GEMM_FAMILY += _NORM_DW
# the image-side direct convolutions (csrc/k_conv_cin4.hip) and the reductions (csrc/k_reduce.hip): guarded form by form too
# (test_side_kernel_forms.py); their calls are kept with the GEMM calls as well
_SIDE = ("cdf_conv_cin4_fwd", "cdf_conv_cin4_dgrad", "cdf_conv_cin4_tapsum3", "cdf_conv_cin4_wgrad", "cdf_unpack_reduce", "cdf_unpack_reduce_bias",
         "cdf_colsum", "cdf_colsum_io")
# ... and linear attention and the row softmax (csrc/k_attn.hip, csrc/k_attn_kvctx.hip; test_side_kernel_forms_attn.py)
_SIDE_ATTN = ("cdf_linattn_context", "cdf_linattn_dcontext", "cdf_linattn_bwd_kv", "cdf_linattn_bwd_kv_planes", "cdf_linattn_kvctx", "cdf_linattn_finalize",
              "cdf_linattn_dctx_finish", "cdf_linattn_softk", "cdf_linattn_dk", "cdf_softmax_rows_fwd", "cdf_softmax_rows_bwd")
_SIDE += _SIDE_ATTN
_GEMM_FAMILY += _SIDE


def _guard_calls(bench_data):
    """Every cdf_* call of one bench step in each arithmetic mode the bench reports (bf16x3, and bf16 with its bf16 activation
    stream) and of one sampler step: (set of names, the (nsplit, T, R, C) of the bf16x3 step's slab reductions, the (recording, name,
    arguments) of every GEMM / weight-gradient call (pre-split family, exact-fp32 pair, in-kernel-split pair) and of every depthwise,
    LayerNorm and GroupNorm call (_NORM_DW) of those and of one forward + backward pass of config 2's network (dropout 0.1, training mode)
    -- the phase / tap descriptors copied, they are buffers the caller may reuse; and of every image-side direct convolution, slab
    reduction and column sum (_SIDE) of the same four runs)."""
    from colddiff import runtime as rt
    names, unpack, gemm = set(), set(), []

    def keep(src, rec):
        for n, a in rec.calls:
            if n in _GEMM_FAMILY or n in _F32_GEMM:
                gemm.append((src, n, tuple(tuple(v) if hasattr(v, "_length_") else v for v in a)))
    for mode in ("bf16x3", "bf16"):
        with rt.precision_scope(mode), Recorder(rt.lib()) as rec:
            _step(bench_data)
        names |= rec.names()
        keep("bench " + mode, rec)
        if mode == "bf16x3":
            unpack = {tuple(a[2:6]) for n, a in rec.calls if n in ("cdf_unpack_reduce", "cdf_unpack_reduce_bias")}
    torch.manual_seed(4)
    with Recorder(rt.lib()) as rec:
        _sampler_run(bench_data["sd"], torch.randn(16, 3, 128, 128))
    keep("sampler", rec)
    run2 = _config2_runner()
    with Recorder(rt.lib()) as rec2:
        run2()
    keep("config 2", rec2)
    return names | rec.names(), unpack, gemm


def _c_ints(v):
    import ctypes
    return (ctypes.c_int * len(v))(*v)


def _gemm_code(L, name, a):
    """The kernel-form code of a recorded cdf_conv_gemm_bf16x / _io / _lnbwd call: the query on the recorded arguments themselves."""
    ns = 3 if a[1] else 1
    if name.endswith("_lnbwd"):
        B, H, W, Cin, Cout = a[7:12]
        return L.cdf_conv_gemm_bf16x_form(B, H, W, Cin, Cout, H, W, 1, 1, 1, _c_ints(a[12]), ns, 0, 1, a[-2], 0)
    B, H, W, Cin, OH, OW, Cout, QH, QW, os_, is_, nphase = a[9:21]
    ws, ws_floats = a[-4], a[-3]
    return L.cdf_conv_gemm_bf16x_form(B, H, W, Cin, Cout, QH, QW, os_, is_, nphase, _c_ints(a[21]), ns, ws_floats if ws else 0, 0, a[-2], 0)


def _wgrad_code(L, name, a):
    QH, QW, HA, WA, sa, HB, WB, sb, CA, CB, ntaps = a[10:21]
    return L.cdf_conv_wgrad_bf16x_form(QH, QW, HA, WA, sa, HB, WB, sb, CA, CB, ntaps, _c_ints(a[21]), 3 if a[1] else 1, a[22], a[-2], 0)


def test_coverage_guard(bench_data):
    """A new entry point cannot reach the hot path without a test at a production shape: each name one bench step (both modes) and one
    sampler step call must be listed above (or exempt, with a reason), and each listed test must exist.  The slab counts
    test_kernels_production.BENCH_UNPACK tests must still be ones the bench step launches (stale shapes fail here).
    The pre-split GEMM family is guarded kernel form by kernel form, not by entry-point name: every (form code, NS) that the bench step,
    the sampler step and config 2's network reach -- asked of the library's own dispatcher (cdf_conv_gemm_bf16x_form /
    cdf_conv_wgrad_bf16x_form) with the recorded arguments -- must be a form some test_gemm_production.BENCH_GEMM / BENCH_WGRAD row resolves
    to, and every committed row must still be a call the recordings contain.  The exact-fp32 pair (cdf_conv_gemm, cdf_conv_gemm_io,
    cdf_conv_wgrad) likewise: every form (test_gemm_f32_forms.f32_gemm_form / f32_wgrad_form of the recorded arguments) must be one a row
    of that module's case tables has, and the forms it flags as reached must still be reached.  The in-kernel-split pair
    (cdf_conv_gemm_bf16, cdf_conv_wgrad_bf16) the same way against test_gemm_sp_forms (sp_gemm_form / sp_wgrad_form).  The depthwise,
    LayerNorm and GroupNorm entry points (_NORM_DW) the same way against the six classifiers and case tables of test_norm_dw_forms.
    The image-side direct convolutions, the slab reductions, the column sums, linear attention and the row softmax (_SIDE) the same way
    against the classifiers and case tables of test_side_kernel_forms and test_side_kernel_forms_attn.
    The FID extractor is a recording of its own (test_inception_forms.extractor_calls: none of the four runs above launches it): the forms
    of its cdf_conv_gemm_bf16 / cdf_conv_gemm calls the same way against test_inception_forms' tables (check_recording)."""
    import os
    import re
    from test_kernels_production import BENCH_UNPACK
    from colddiff import runtime as rt
    import test_gemm_production as gp
    names, unpack, gemm = _guard_calls(bench_data)
    here = os.path.dirname(os.path.abspath(__file__))
    for name, tests in COVERED_AT_PRODUCTION_SHAPE.items():
        for t in tests:
            mod, fn = t.split("::")
            assert re.search(r"^def %s\(" % fn, open(os.path.join(here, mod)).read(), flags=re.M), (name, t)
    missing = sorted(n for n in names if n not in COVERED_AT_PRODUCTION_SHAPE and n not in EXEMPT)
    print("entry points called by one bench step (bf16x3, bf16) + one sampler step:", sorted(names))
    assert not missing, "hot-path entry points without a production-shape test: %s" % missing
    stale = sorted(set(BENCH_UNPACK) - unpack)
    assert not stale, "BENCH_UNPACK shapes the bench step no longer launches: %s (it launches %s)" % (stale, sorted(unpack))
    # ---- the pre-split GEMM family, form by form
    L = rt.lib()
    reached_g, reached_w, rows_g, rows_w = {}, {}, set(), set()
    for src, name, a in gemm:
        if name == "cdf_conv_wgrad_bf16x":
            reached_w.setdefault((_wgrad_code(L, name, a), 3 if a[1] else 1), (src, a[9:21], a[22]))
            rows_w.add(gp.wgrad_row(name, a))
        elif name != "cdf_conv_wgrad" and name not in _F32_GEMM and name not in _SP_GEMM and name not in _NORM_DW and name not in _SIDE:
            reached_g.setdefault((_gemm_code(L, name, a), 3 if a[1] else 1), (src, name, a[9:21]))
            rows_g.add(gp.gemm_row(name, a))
    assert all(c > 0 for c, _ in list(reached_g) + list(reached_w)), (reached_g, reached_w)
    tested_g = {(gp.gemm_form(L, r, rt.tune_ptr())[0], r[-1]) for r in gp.BENCH_GEMM}
    tested_w = {(gp.wgrad_form(L, r, rt.tune_ptr())[0], r[-1]) for r in gp.BENCH_WGRAD}
    for what, reached, tested, dec in (("GEMM", reached_g, tested_g, gp.decode), ("weight-gradient", reached_w, tested_w, gp.decode)):
        print("pre-split %s kernel forms reached: %s" % (what, sorted((k[1], tuple(dec(k[0]).items())) for k in reached)))
        untested = {k: v for k, v in reached.items() if k not in tested}
        assert not untested, "%s kernel forms (code, NS) the product reaches without a test_gemm_production row: %s" % (
            what, {(ns, tuple(dec(c).items())): v for (c, ns), v in untested.items()})
    stale = sorted(set(gp.BENCH_GEMM) - rows_g) + sorted(set(gp.BENCH_WGRAD) - rows_w)
    assert not stale, "test_gemm_production rows the recordings no longer contain: %s" % stale
    resident = [(r, gp.gemm_form(L, r, rt.tune_ptr())[1:]) for r in gp.BENCH_GEMM if gp.decode(gp.gemm_form(L, r, rt.tune_ptr())[0])["form"] == gp.ROWHALO]
    print("resident row-halo rows (tiles, grid):", resident)
    assert any(t > g for _, (t, g) in resident), "no BENCH_GEMM row walks several tiles per resident block"
    # ---- the exact-fp32 pair (conv_igemm_kernel, conv_wgrad_kernel), form by form: the forms are pure functions of the recorded arguments
    import test_gemm_f32_forms as ff
    reached_fg, reached_fw = {}, {}
    for src, name, a in gemm:
        if name in _F32_GEMM:
            reached_fg.setdefault(ff.f32_gemm_form(name, a), (src, name, a[6:18], a[32:40]))
        elif name == "cdf_conv_wgrad":
            reached_fw.setdefault(ff.f32_wgrad_form(a), (src, a[6:18], a[19:24]))
    assert reached_fg and reached_fw
    for what, reached, tested, flagged in (("GEMM", reached_fg, ff.forms_of_gemm_rows(), ff.REACHED_GEMM),
                                           ("weight-gradient", reached_fw, ff.forms_of_wgrad_rows(), ff.REACHED_WGRAD)):
        print("exact-fp32 %s forms reached:" % what)
        for k in sorted(reached, key=repr):
            print("    %r," % (k,))
        untested = {k: v for k, v in reached.items() if k not in tested}
        assert not untested, "exact-fp32 %s forms the product reaches without a test_gemm_f32_forms row: %s" % (what, untested)
        stale = sorted(flagged - set(reached), key=repr)
        assert not stale, "test_gemm_f32_forms flags %s forms as reached that the recordings no longer contain: %s" % (what, stale)
    # ---- the in-kernel-split pair (conv_igemm_sp_kernel, conv_wgrad_sp_kernel), form by form
    import test_gemm_sp_forms as sf
    reached_sg, reached_sw = {}, {}
    for src, name, a in gemm:
        if name == "cdf_conv_gemm_bf16":
            reached_sg.setdefault(sf.sp_gemm_form(a), (src, a[1], a[6:19], a[24]))
        elif name == "cdf_conv_wgrad_bf16":
            reached_sw.setdefault(sf.sp_wgrad_form(a), (src, a[1], a[3], a[6:18], a[19]))
    assert reached_sg and reached_sw
    for what, reached, tested, flagged in (("GEMM", reached_sg, sf.forms_of_gemm_rows(), sf.REACHED_SP_GEMM),
                                           ("weight-gradient", reached_sw, sf.forms_of_wgrad_rows(), sf.REACHED_SP_WGRAD)):
        print("in-kernel-split %s forms reached:" % what)
        for k in sorted(reached, key=repr):
            print("    %r," % (k,))
        untested = {k: v for k, v in reached.items() if k not in tested}
        assert not untested, "in-kernel-split %s forms the product reaches without a test_gemm_sp_forms row: %s" % (what, untested)
        stale = sorted(flagged - set(reached), key=repr)
        assert not stale, "test_gemm_sp_forms flags %s forms as reached that the recordings no longer contain: %s" % (what, stale)
    # ---- the kernels between the GEMMs (k_dwconv.hip, k_norm.hip), form by form
    import test_norm_dw_forms as nd
    assert set(nd.ALL_NAMES) == set(_NORM_DW)
    reached_nd = nd.reached_forms(gemm)
    for what, reached in reached_nd.items():
        tested, flagged = nd.forms_of_rows(what), nd.REACHED[what]
        print("%s forms reached:" % what)
        for k in sorted(reached, key=repr):
            print("    %r," % (k,))
        assert reached, what
        untested = {k: v for k, v in reached.items() if k not in tested}
        assert not untested, "%s forms the product reaches without a test_norm_dw_forms row: %s" % (what, untested)
        stale = sorted(flagged - set(reached), key=repr)
        assert not stale, "test_norm_dw_forms flags %s forms as reached that the recordings no longer contain: %s" % (what, stale)
    # ---- the image-side direct convolutions, the slab reductions and the column sums (k_conv_cin4.hip, k_reduce.hip), linear attention and the
    # row softmax (k_attn.hip, k_attn_kvctx.hip), form by form
    import test_side_kernel_forms as sk
    import test_side_kernel_forms_attn as sa
    assert set(sk.ALL_NAMES) | set(sa.ALL_NAMES) == set(_SIDE) and set(sa.ALL_NAMES) == set(_SIDE_ATTN)
    for mod, what, reached in [(m, w, r) for m in (sk, sa) for w, r in m.reached_forms(gemm).items()]:
        tested, flagged = mod.forms_of_rows(what), mod.REACHED[what]
        print("%s forms reached:" % what)
        for k in sorted(reached, key=repr):
            print("    %r," % (k,))
        assert reached or not flagged, what
        untested = {k: v for k, v in reached.items() if k not in tested}
        assert not untested, "%s forms the product reaches without a %s row: %s" % (what, mod.__name__, untested)
        stale = sorted(flagged - set(reached), key=repr)
        assert not stale, "%s flags %s forms as reached that the recordings no longer contain: %s" % (mod.__name__, what, stale)
    # ---- the FID extractor's conv GEMM launches (colddiff/inception.py), form by form: one forward on 64 x 64 images at B = 50 and B = 1 in
    # the default mode, in bf16 and in f32 -- every recorded form must have a row in test_inception_forms, every form it flags is recorded
    import test_inception_forms as tif
    tif.check_recording(tif.extractor_calls(DEV))
