"""Process-wide handles: the kernel library, the HIP stream of the current torch context, and the
packed-weight cache.  There is no CPU fallback: tensors must live on a HIP device."""
import torch

from . import _lib

# Set ONLY by the CPU test-suite (tests/emu_util.install_emu) to run the host SIMT-simulator build
# of the very same kernels on CPU tensors.  Never set by the package itself.
_lib_override = None

# Bumped whenever parameters are rewritten behind torch's back (fused Adam / EMA kernels write
# through raw pointers and do not touch Tensor._version); invalidates the packed-weight cache.
weights_epoch = 0


# Arithmetic of the dense-conv GEMMs (forward + data gradient):
#   "bf16x3" (default) split-precision bf16 MFMA: every fp32 operand = bf16 hi + bf16 lo, a*b ~ ah*bh+ah*bl+al*bh,
#            fp32 accumulate; meets the same 1e-4 parity bound as exact fp32 (tests run in this mode)
#   "f32"    exact fp32 MFMA (v_mfma_f32_32x32x2_f32)
#   "bf16"   plain bf16 operands, fp32 accumulate (NOT parity-grade: ~1e-2)
# Weight gradients, norms, attention, degradations, optimizer are fp32 in every mode.
import os as _os

precision = _os.environ.get("COLDDIFF_PRECISION", "bf16x3")


# Stated tolerance of the "bf16" mode against the fp32 oracle -- asserted by tests/test_gpu_parity2.py (module level and the
# B = 32, 128 x 128 bench shape) and quoted verbatim by bench.py's `bf16_mode` line.
BF16_TOLERANCE = {"forward_max_abs": 2e-2,             # UNet output (image scale, |y| <~ 2.5)
                  "grad_rel_of_tensor_max": 6e-2,      # every gradient tensor: max-abs error / max(|g|max of the tensor, 1e-2 x largest |g|max); measured worst 5.0e-2 (64x64 net), < 4e-2 at the bench shape
                  "loss_rel": 2e-3}                    # micro-step loss


def set_precision(p):
    global precision
    assert p in ("f32", "bf16x3", "bf16"), p
    precision = p


import contextlib as _contextlib


@_contextlib.contextmanager
def precision_scope(p):
    """Run a region in another arithmetic mode.  The packed-weight cache keeps ONE layout per (parameter, kind) -- the mode is not part of
    the slot -- and remembers the mode it was packed in: the first use of a weight in the other mode packs it again over that slot, and
    so does the first use after the region ends.  That holds for every kind: the `_sp` kinds change their contents with the mode (the
    lo plane exists in "bf16x3" only), the kinds without `_sp` (conv_fwd, kv_fwd, dw, lin_fwd, cin4 ...) hold the same values in every
    mode, share their slot across the modes all the same and are re-packed, into the same buffer, by their own launch on each toggle
    (pinned by tests/test_weight_caches.py::test_layout_precision_toggle_on_a_shared_slot)."""
    global precision
    assert p in ("f32", "bf16x3", "bf16"), p
    saved, precision = precision, p
    try:
        yield
    finally:
        precision = saved


# BASELINE config 2 names fp32, and `Model` (the DDPM UNet of the CIFAR-10 scripts) amplifies a per-call error along a T = 50 Algorithm-2
# trajectory (a 6e-5 perturbation per call ends 8e-4 away).  Split precision keeps every single call within 1e-4 (training: loss and
# gradients are single calls), but an ITERATED no-grad application -- the samplers -- runs `Model` on the exact-fp32 matrix-core kernels
# so that the whole trajectory stays within the north_star bound (tests/test_gpu_fullsize.py::test_cfg2_cifar_model_sample_vs_oracle).
# COLDDIFF_MODEL_SAMPLE_PRECISION=same keeps the process-wide mode for those calls too.
MODEL_SAMPLE_PRECISION = _os.environ.get("COLDDIFF_MODEL_SAMPLE_PRECISION", "f32")


def lib():
    return _lib_override if _lib_override is not None else _lib.get()


# The tuning argument this process passes to the pre-split GEMM entry points (include/colddiff.h: cdf_gemm_tuning): defaults of the
# library + the COLDDIFF_SPX_* / COLDDIFF_WGRAD_* environment variables.  Python-side state only; tools / tests change fields through
# `tuning().set(field=value)`.
_tuning = {}


def tuning():
    L = lib()
    t = _tuning.get(id(L))
    if t is None:
        t = _tuning[id(L)] = _lib.GemmTuning(L).from_env()
    return t


def tune_ptr():
    return tuning().ptr


KVCTX_SLOTS = int(_os.environ.get("COLDDIFF_KVCTX_SLOTS", "0"))       # cdf_linattn_kvctx: target block count (0 = the library's default)


def stream(t=None):
    if _lib_override is not None:
        return 0
    return torch.cuda.current_stream(t.device if t is not None else None).cuda_stream


def check(t):
    if t is not None and not t.is_cuda and _lib_override is None:
        raise RuntimeError("colddiff: operators run on the MI355X only (tensor is on %s; no CPU fallback)" % t.device)
    return t


def bump_weights_epoch():
    global weights_epoch
    weights_epoch += 1


def P(t):
    return 0 if t is None else t.data_ptr()


def r4(c):
    return (c + 3) // 4 * 4
