"""References and cache handles of test_weight_caches.py.

`layout_ref` restates the layouts `ops.packed` documents (its docstring and `_pack_geom`) with torch permute / reshape on a host copy of
the CURRENT weight values; no cdf_* function lays anything out here.  The bf16 hi / lo planes of the `_sp` kinds come from
test_kernels._split (cdf_split_bf16) and are held, at every call, against torch's own round-to-nearest-even bfloat16 conversion.
Pad columns (and the rows >= Cin of `cin4`) are zero: the stated contract of cdf_pack_weight / cdf_pack_weight_bf16 / cdf_pack_cin4
(k_pack.hip, test_gemm_f32_forms.py), so whole buffers are compared bit for bit.
"""
import contextlib

import torch

r4 = lambda c: (c + 3) // 4 * 4
r32 = lambda c: (c + 31) // 32 * 32

SP_KINDS = ("conv_fwd_sp", "conv_dgrad_sp", "convT_fwd_sp", "convT_dgrad_sp", "kv_fwd_sp", "kv_dgrad_sp")


def _matrix(w, kind):
    """[T][R][C] of the layout, unpadded (w: host fp32 tensor in the PyTorch parameter layout)."""
    if kind.startswith("kv_"):
        HD = w.shape[0] // 3
        kv = w[HD:, :, 0, 0]                                 # [2 HD][Cin]: the k | v rows of to_qkv
        return (kv.t() if kind in ("kv_fwd", "kv_dgrad_sp") else kv).contiguous()[None]
    if kind == "lin_fwd":
        return w.t().contiguous()[None]                      # [1][K][N]
    if kind == "dw":
        C = w.shape[0]
        return w.reshape(C, 49).t().reshape(49, 1, C).contiguous()
    if kind == "cin_z":
        return w.reshape(1, w.shape[0], -1).contiguous()     # [1][Cout][Cin 9]
    A, B, KH, KW = w.shape                                   # conv: [Cout, Cin, ..]   convT: [Cin, Cout, ..]
    taps_ab = w.permute(2, 3, 0, 1).reshape(KH * KW, A, B)   # [KK][dim 0][dim 1]
    taps_ba = w.permute(2, 3, 1, 0).reshape(KH * KW, B, A)   # [KK][dim 1][dim 0]
    # fp32 layouts are [KK][K][N] (N contiguous), the bf16 planes [KK][N][K] (K contiguous)
    return {"conv_fwd": taps_ba, "conv_dgrad": taps_ab, "convT_fwd": taps_ab, "convT_dgrad": taps_ba,
            "conv_fwd_sp": taps_ab, "conv_dgrad_sp": taps_ba, "convT_fwd_sp": taps_ba, "convT_dgrad_sp": taps_ab}[kind].contiguous()


def _pad_last(m, ld):
    out = torch.zeros(m.shape[:-1] + (ld,), dtype=m.dtype)
    out[..., :m.shape[-1]] = m
    return out


class _SplitBackend:
    """What test_kernels._split asks of a backend, on the library the Python layer is routed to."""

    def __init__(self, device):
        from colddiff import runtime as rt
        self.device, self.L, self._keep = device, rt.lib(), []
        self.stream = lambda: rt.stream()


def _planes(m, device, want_lo):
    """(hi, lo | None) int16 host planes of the fp32 host matrix m [.., C], C % 4 == 0."""
    from test_kernels import _split
    C = m.shape[-1]
    assert C % 4 == 0
    be = _SplitBackend(device)
    hi, lo = _split(be, m.to(device).contiguous(), single=not want_lo)
    hi, lo = hi.cpu()[..., :C], (None if lo is None else lo.cpu()[..., :C])
    t_hi = m.to(torch.bfloat16)                              # torch rounds to nearest even as well
    assert torch.equal(hi, t_hi.view(torch.int16))
    if want_lo:
        assert torch.equal(lo, (m - t_hi.float()).to(torch.bfloat16).view(torch.int16))
    return hi, lo


def layout_ref(w, kind, precision, device):
    """The layout `ops.packed(param, kind)` must return for the host values w in arithmetic mode `precision`:
    an fp32 host tensor, or (hi, lo | None) int16 host planes for the `_sp` kinds."""
    w = w.detach().cpu().float()
    if kind == "cin4":
        Co, Ci, KH, KW = w.shape
        out = torch.zeros(KH * KW, 4, r4(Co))
        out[:, :Ci, :Co] = w.permute(2, 3, 1, 0).reshape(KH * KW, Ci, Co)
        return out
    m = _matrix(w, kind)
    if kind in SP_KINDS:
        hi, lo = _planes(m, device, precision == "bf16x3")
        ld = r32(m.shape[-1])
        return _pad_last(hi, ld), (None if lo is None else _pad_last(lo, ld))
    return _pad_last(m, r4(m.shape[-1]))


def same_layout(got, want):
    """Bit for bit, pad columns included; None where the reference has none."""
    if isinstance(want, tuple):
        if not isinstance(got, tuple) or len(got) != 2:
            return False
        return all((g is None) == (w is None) and (w is None or (g.dtype == w.dtype and g.shape == w.shape and torch.equal(g.cpu(), w)))
                   for g, w in zip(got, want))
    return torch.is_tensor(got) and got.dtype == want.dtype and got.shape == want.shape and torch.equal(got.cpu().view(torch.int32), want.view(torch.int32))


# -- the caches that derive from weights ------------------------------------------------------------------------------------------
def _tb_owners(modules):
    return [m for top in modules for m in top.modules() if "_tb_cache" in m.__dict__]


def empty_caches(modules=(), cores=()):
    """A cold start: every weight-derived cache of the product emptied (packed layouts, their device tables, each network's
    concatenated time-bias weights, each diffusion core's blur tap stack)."""
    from colddiff import ops
    ops._pack_cache.clear()
    ops._pack_tables.clear()
    for m in _tb_owners(modules):
        del m.__dict__["_tb_cache"]
    for c in cores:
        if getattr(c, "_taps_cache", None) is not None:
            c._taps_cache = None


@contextlib.contextmanager
def cold_start(modules=(), cores=()):
    """Run a region from empty caches, then put the warm state back exactly as it was (nothing wrote a weight in between, so it
    describes the weights as well as it did before): a sequence keeps its history across the cold comparison."""
    from colddiff import ops
    saved = (dict(ops._pack_cache), dict(ops._pack_tables), [(m, m.__dict__["_tb_cache"]) for m in _tb_owners(modules)],
             [(c, c._taps_cache) for c in cores if hasattr(c, "_taps_cache")])
    empty_caches(modules, cores)
    try:
        yield
    finally:
        empty_caches(modules, cores)
        ops._pack_cache.update(saved[0])
        ops._pack_tables.update(saved[1])
        for m, v in saved[2]:
            m.__dict__["_tb_cache"] = v
        for c, v in saved[3]:
            c._taps_cache = v


class Trace(list):
    """The events of a sequence; the last ~20 are printed when the sequence fails."""

    def __call__(self, *what):
        self.append(" ".join(str(w) for w in what))

    def __enter__(self):
        return self

    def __exit__(self, et, ev, tb):
        if et is not None:
            print("last events of the failing sequence (%d in all):" % len(self))
            for i, line in enumerate(self[-20:], max(0, len(self) - 20)):
                print("  %3d  %s" % (i, line))
        return False
