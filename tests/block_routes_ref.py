"""Rigs for tests/test_block_routes.py: one autograd block (or a short chain of them) with fixed weights and inputs, its fp64
reference out of the restatements in oracle/cold_oracle.py, and the run through the module's own `forward` on a backend.

A rig's `reference()` and `run(mods, dev)` return the same keys: "y" (block output, NCHW), "dx" / "dx2" (input gradients, NCHW) and
"dtemb" (the gradient reaching the time embedding); the test adds "grad/<name>" for every parameter.  `reference()` works on
`.double()` copies of the parameters and inputs (the oracle functions are dtype-generic); bf16-stream rigs round their inputs to bf16
first, so both sides start from the same numbers.

TEST INFRASTRUCTURE ONLY: the product never imports this module.
"""
import torch
import torch.nn.functional as F

from oracle import cold_oracle as O

BF = torch.bfloat16


def prep(mod, seed):
    """Norm gains / biases off 1 / 0, every other parameter doubled (no gradient tensor ends up ~0)."""
    from colddiff import unet as D
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in mod.modules():
            norm = isinstance(m, (D.LayerNorm, torch.nn.GroupNorm))
            for p in m.parameters(recurse=False):
                if norm:
                    p.add_(0.3 * torch.randn(p.shape, generator=g))
                else:
                    p.mul_(2.0)
    return mod


def rbf(t):
    """fp32 -> the nearest bf16 value, kept as fp32."""
    return t.to(BF).float()


def leaf(t, dev):
    return t.to(dev).clone().requires_grad_(True)


def bf_leaf(t, dev):
    """NCHW fp32 (bf16-valued) -> NHWC bf16 leaf on dev."""
    return t.permute(0, 2, 3, 1).contiguous().to(BF).to(dev).requires_grad_(True)


def bf_nhwc(t, dev):
    return t.permute(0, 2, 3, 1).contiguous().to(BF).to(dev)


def from_bf(t):
    """NHWC bf16 on the device -> NCHW fp32 on the host."""
    return t.detach().float().cpu().permute(0, 3, 1, 2).contiguous()


class Rig:
    """mods: nn.Module with every parameter of the case; ref(sd) -> dict (sd: fp64 leaves named as mods.state_dict());
    run(mods, dev) -> dict of host tensors; seams: [(object, attribute, value)] set while the case runs."""

    def __init__(self, mods, ref, run, seams=()):
        self.mods, self._ref, self.run, self.seams = mods, ref, run, list(seams)

    def reference(self):
        sd = {k: v.detach().double().clone().requires_grad_(True) for k, v in self.mods.state_dict().items()}
        out = {k: v.detach() for k, v in self._ref(sd).items()}
        for k, v in sd.items():
            assert v.grad is not None, k
            out["grad/" + k] = v.grad
        return out


def _d(t):
    return None if t is None else t.double().requires_grad_(True)


def _grad(t):
    return None if t is None else t.grad


def _pack(y, **grads):
    out = {"y": y.detach()}
    out.update({k: v for k, v in grads.items() if v is not None})
    return out


def _cpu(y, **grads):
    out = {"y": y.detach().cpu()}
    out.update({k: v.grad.detach().cpu() for k, v in grads.items() if v is not None})
    return out


# -- ConvNextBlockFn ---------------------------------------------------------------------------------------------------------------------
def convnext(dim, dim_out, B, H, mult=2, tdim=16, norm=True, dest=False, seed=1, seams=()):
    from colddiff import functions as F_, unet as D
    torch.manual_seed(seed)
    blk = prep(D.ConvNextBlock(dim, dim_out, time_emb_dim=tdim, mult=mult, norm=norm), seed)
    x, gy = torch.randn(B, dim, H, H), torch.randn(B, dim_out, H, H)
    temb = torch.randn(B, tdim) if tdim else None

    def ref(sd):
        xr, tr = _d(x), _d(temb)
        y = O.convnext_block(sd, xr, tr)
        y.backward(gy.double())
        return _pack(y, dx=xr.grad, dtemb=_grad(tr))

    def run(m, dev):
        xd = leaf(x, dev)
        td = leaf(temb, dev) if tdim else None
        xn = F_.ToNHWC.apply(xd)
        cat = None
        if dest:                                              # the block writes the first half; the other one must stay as it is
            cat = F_.CatBuf(xn, B, H, H, dim_out, 64)
            cat.buf.fill_(7.0)
        o = m(xn, F_.Act.apply(td, F_.ACT_GELU) if tdim else None, dest=cat)
        y = F_.ToNCHW.apply(o, dim_out, None)
        y.backward(gy.to(dev))
        if dest:
            assert o.data_ptr() == cat.buf.data_ptr() and bool((cat.second() == 7.0).all()), "dest: wrong half written"
        return _cpu(y, dx=xd, dtemb=td)
    return Rig(blk, ref, run, seams)


def convnext_chain(B, H, mark=False, seed=2, seams=()):
    """Two (64 -> 64) blocks in a row; mark: the first block's output carries `_cdf_grad_f32` (as an attention block's or a skip
    join's output does), so the second block hands its data gradient on as fp32 only."""
    from colddiff import functions as F_, unet as D
    torch.manual_seed(seed)
    mods = prep(torch.nn.ModuleDict({"a": D.ConvNextBlock(64, 64, time_emb_dim=16), "b": D.ConvNextBlock(64, 64, time_emb_dim=16)}), seed)
    x, gy, temb = torch.randn(B, 64, H, H), torch.randn(B, 64, H, H), torch.randn(B, 16)

    def ref(sd):
        xr, tr = _d(x), _d(temb)
        y = O.convnext_block(O._sub(sd, "b."), O.convnext_block(O._sub(sd, "a."), xr, tr), tr)
        y.backward(gy.double())
        return _pack(y, dx=xr.grad, dtemb=tr.grad)

    def run(m, dev):
        xd, td = leaf(x, dev), leaf(temb, dev)
        gt = F_.Act.apply(td, F_.ACT_GELU)
        ya = m["a"](F_.ToNHWC.apply(xd), gt)
        if mark:
            ya._cdf_grad_f32 = True
        y = F_.ToNCHW.apply(m["b"](ya, gt), 64, None)
        y.backward(gy.to(dev))
        return _cpu(y, dx=xd, dtemb=td)
    return Rig(mods, ref, run, seams)


# -- LinAttnBlockFn / LinAttnBlockBF -----------------------------------------------------------------------------------------------------
def linattn(dim, B, H, dest=False, bf=False, seed=3, seams=()):
    from colddiff import functions as F_, unet as D
    torch.manual_seed(seed + dim)
    blk = prep(D.Residual(D.PreNorm(dim, D.LinearAttention(dim))), seed)
    x, gy = torch.randn(B, dim, H, H), torch.randn(B, dim, H, H)
    if bf:
        x, gy = rbf(x), rbf(gy)

    def ref(sd):
        xr = _d(x)
        y = O.linear_attention_block(sd, xr)
        y.backward(gy.double())
        return _pack(y, dx=xr.grad)

    def run(m, dev):
        if bf:
            xd = bf_leaf(x, dev)
            cat = F_.CatBuf(xd, B, H, H, dim, dim, dtype=BF) if dest else None
            if dest:
                cat.buf.fill_(7.0)
            o = m(xd, cat)
            o.backward(bf_nhwc(gy, dev))
            if dest:
                assert bool((cat.first() == 7.0).all()), "dest: wrong half written"
            return {"y": from_bf(o), "dx": from_bf(xd.grad)}
        xd = leaf(x, dev)
        xn = F_.ToNHWC.apply(xd)
        cat = F_.CatBuf(xn, B, H, H, dim, dim) if dest else None
        if dest:
            cat.buf.fill_(7.0)
        o = m(xn, cat)
        y = F_.ToNCHW.apply(o, dim, None)
        y.backward(gy.to(dev))
        if dest:
            assert o.data_ptr() == cat.buf.data_ptr() + 4 * dim and bool((cat.first() == 7.0).all()), "dest: wrong half written"
        return _cpu(y, dx=xd)
    return Rig(blk, ref, run, seams)


# -- ConvFn / ConvFnBF -------------------------------------------------------------------------------------------------------------------
def conv(kind, dim, B, H, bf=False, seed=4):
    """kind: "down" (Downsample(dim)), "up" (Upsample(dim)) or "final" (the 1 x 1 Conv2d(dim, 3))."""
    from colddiff import bf16store as BFS, functions as F_, unet as D
    torch.manual_seed(seed + dim)
    mod = prep({"down": lambda: D.Downsample(dim), "up": lambda: D.Upsample(dim), "final": lambda: torch.nn.Conv2d(dim, 3, 1)}[kind](), seed)
    cout = 3 if kind == "final" else dim
    x = torch.randn(B, dim, H, H)
    if bf:
        x = rbf(x)
    args = {"down": ("conv", 2, (1, 1, 1, 1)), "up": ("convT", 2, (1, 1, 1, 1)), "final": ("conv", 1, (0, 0, 0, 0))}[kind]

    def torch_fn(sd, xr):
        if kind == "down":
            return F.conv2d(xr, sd["weight"], sd["bias"], stride=2, padding=1)
        if kind == "up":
            return F.conv_transpose2d(xr, sd["weight"], sd["bias"], stride=2, padding=1)
        return F.conv2d(xr, sd["weight"], sd["bias"])
    with torch.no_grad():
        gy = torch.randn(torch_fn(mod.state_dict(), x).shape)
    if bf:
        gy = rbf(gy)

    def ref(sd):
        xr = _d(x)
        y = torch_fn(sd, xr)
        y.backward(gy.double())
        return _pack(y, dx=xr.grad)

    def run(m, dev):
        if bf:
            xd = bf_leaf(x, dev)
            o = BFS.ConvFnBF.apply(D.anchor(xd), xd, m, dim, *args)
            o.backward(bf_nhwc(gy, dev))
            return {"y": from_bf(o), "dx": from_bf(xd.grad)}
        xd = leaf(x, dev)
        xn = F_.ToNHWC.apply(xd)
        y = F_.ToNCHW.apply(F_.ConvFn.apply(D.anchor(xn), xn, m, dim, *args), cout, None)
        y.backward(gy.to(dev))
        return _cpu(y, dx=xd)
    return Rig(mod, ref, run)


def join(B, bf=False, seed=5):
    """A skip concatenation without copies: the attention block writes the second half of a CatBuf at 16 x 16, the transposed
    up-sampling conv (from 8 x 8) the first, Join / JoinBF hands out the whole; the bf16 stream leaves through ToF32."""
    from colddiff import bf16store as BFS, functions as F_, unet as D
    torch.manual_seed(seed)
    mods = prep(torch.nn.ModuleDict({"attn": D.Residual(D.PreNorm(64, D.LinearAttention(64))), "up": D.Upsample(64)}), seed)
    x1, x2, gy = torch.randn(B, 64, 16, 16), torch.randn(B, 64, 8, 8), torch.randn(B, 128, 16, 16)
    if bf:
        x1, x2 = rbf(x1), rbf(x2)

    def ref(sd):
        a, b = _d(x1), _d(x2)
        up = F.conv_transpose2d(b, sd["up.weight"], sd["up.bias"], stride=2, padding=1)
        y = torch.cat((up, O.linear_attention_block(O._sub(sd, "attn."), a)), dim=1)
        y.backward(gy.double())
        return _pack(y, dx=a.grad, dx2=b.grad)

    def run(m, dev):
        if bf:
            a, b = bf_leaf(x1, dev), bf_leaf(x2, dev)
            an, bn = a, b
        else:
            a, b = leaf(x1, dev), leaf(x2, dev)
            an, bn = F_.ToNHWC.apply(a), F_.ToNHWC.apply(b)
        cat = F_.CatBuf(an, B, 16, 16, 64, 64, dtype=an.dtype)
        skip = m["attn"](an, cat)
        up = (BFS.ConvFnBF if bf else F_.ConvFn).apply(D.anchor(bn), bn, m["up"], 64, "convT", 2, (1, 1, 1, 1), cat)
        j = (BFS.JoinBF if bf else F_.Join).apply(up, skip, cat)
        y = F_.ToNCHW.apply(BFS.ToF32.apply(j) if bf else j, 128, None)
        y.backward(gy.to(dev))
        if bf:
            return {"y": y.detach().cpu(), "dx": from_bf(a.grad), "dx2": from_bf(b.grad)}
        return _cpu(y, dx=a, dx2=b)
    return Rig(mods, ref, run)


# -- ConvNextBlockBF ---------------------------------------------------------------------------------------------------------------------
def convnext_bf(dim, dim_out, B, H, seed=6):
    from colddiff import functions as F_, unet as D
    torch.manual_seed(seed)
    blk = prep(D.ConvNextBlock(dim, dim_out, time_emb_dim=16), seed)
    x, gy, temb = rbf(torch.randn(B, dim, H, H)), rbf(torch.randn(B, dim_out, H, H)), torch.randn(B, 16)

    def ref(sd):
        xr, tr = _d(x), _d(temb)
        y = O.convnext_block(sd, xr, tr)
        y.backward(gy.double())
        return _pack(y, dx=xr.grad, dtemb=tr.grad)

    def run(m, dev):
        xd, td = bf_leaf(x, dev), leaf(temb, dev)
        o = m(xd, F_.Act.apply(td, F_.ACT_GELU))
        assert o.dtype == BF
        o.backward(bf_nhwc(gy, dev))
        return {"y": from_bf(o), "dx": from_bf(xd.grad), "dtemb": td.grad.detach().cpu()}
    return Rig(blk, ref, run)


def enter_bf(B, H, seed=7):
    """The image-side block (3 -> 64, fp32 tensors) followed by the block in which its output enters the bf16 stream; out through ToF32."""
    from colddiff import bf16store as BFS, functions as F_, unet as D
    torch.manual_seed(seed)
    mods = prep(torch.nn.ModuleDict({"a": D.ConvNextBlock(3, 64, time_emb_dim=16, norm=False), "b": D.ConvNextBlock(64, 64, time_emb_dim=16)}), seed)
    x, gy, temb = torch.randn(B, 3, H, H), torch.randn(B, 64, H, H), torch.randn(B, 16)

    def ref(sd):
        xr, tr = _d(x), _d(temb)
        y = O.convnext_block(O._sub(sd, "b."), O.convnext_block(O._sub(sd, "a."), xr, tr), tr)
        y.backward(gy.double())
        return _pack(y, dx=xr.grad, dtemb=tr.grad)

    def run(m, dev):
        xd, td = leaf(x, dev), leaf(temb, dev)
        gt = F_.Act.apply(td, F_.ACT_GELU)
        o = m["b"](m["a"](F_.ToNHWC.apply(xd), gt), gt, enter_bf16=True)
        assert o.dtype == BF
        y = F_.ToNCHW.apply(BFS.ToF32.apply(o), 64, None)
        y.backward(gy.to(dev))
        return _cpu(y, dx=xd, dtemb=td)
    return Rig(mods, ref, run)


# -- the DDPM `Model` family -------------------------------------------------------------------------------------------------------------
def resnet(cin, cout, B, H, seed=8, seams=()):
    from colddiff import functions as F_
    from colddiff.model2 import ResnetBlock
    torch.manual_seed(seed)
    blk = prep(ResnetBlock(in_channels=cin, out_channels=cout, dropout=0.0, temb_channels=32), seed)
    x, gy, temb = torch.randn(B, cin, H, H), torch.randn(B, cout, H, H), torch.randn(B, 32)

    def ref(sd):
        xr, tr = _d(x), _d(temb)
        y = O.resnet_block(sd, xr, tr)
        y.backward(gy.double())
        return _pack(y, dx=xr.grad, dtemb=tr.grad)

    def run(m, dev):
        xd, td = leaf(x, dev), leaf(temb, dev)
        y = F_.ToNCHW.apply(m(F_.ToNHWC.apply(xd), F_.Act.apply(td, F_.ACT_SILU)), cout, None)
        y.backward(gy.to(dev))
        return _cpu(y, dx=xd, dtemb=td)
    return Rig(blk, ref, run, seams)


def _simple(mod, x, torch_fn, apply_fn, cout, seed):
    """A one-input node: y = apply_fn(mod, NHWC x) on the device, torch_fn(sd, x) in fp64."""
    from colddiff import functions as F_
    with torch.no_grad():
        gy = torch.randn(torch_fn({k: v for k, v in mod.state_dict().items()}, x).shape, generator=torch.Generator().manual_seed(seed))

    def ref(sd):
        xr = _d(x)
        y = torch_fn(sd, xr)
        y.backward(gy.double())
        return _pack(y, dx=xr.grad)

    def run(m, dev):
        xd = leaf(x, dev)
        y = F_.ToNCHW.apply(apply_fn(m, F_.ToNHWC.apply(xd)), cout, None)
        y.backward(gy.to(dev))
        return _cpu(y, dx=xd)
    return Rig(mod, ref, run)


def attn(C, B, H, seed=9):
    from colddiff.model2 import AttnBlock
    torch.manual_seed(seed + H)
    blk = prep(AttnBlock(C), seed)
    return _simple(blk, torch.randn(B, C, H, H), lambda sd, x: O.attn_block(sd, x), lambda m, xn: m(xn), C, seed)


def upsample_conv(C, B, H, seed=10):
    from colddiff.model2 import Upsample
    torch.manual_seed(seed)
    mod = prep(Upsample(C, True), seed)
    return _simple(mod, torch.randn(B, C, H, H),
                   lambda sd, x: F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), sd["conv.weight"], sd["conv.bias"], padding=1),
                   lambda m, xn: m(xn), C, seed)


def resample(kind, C, B, H, seed=11):
    """The resamp_with_conv=False pair: "pool" (AvgPool2Fn) or "up" (Upsample2Fn).  No parameters."""
    from colddiff.model2 import Downsample, Upsample
    torch.manual_seed(seed)
    mod = Downsample(C, False) if kind == "pool" else Upsample(C, False)
    fn = (lambda sd, x: F.avg_pool2d(x, kernel_size=2, stride=2)) if kind == "pool" else \
        (lambda sd, x: F.interpolate(x, scale_factor=2.0, mode="nearest"))
    return _simple(mod, torch.randn(B, C, H, H), fn, lambda m, xn: m(xn), C, seed)


def groupnorm(C, B, H, silu, seed=12):
    from colddiff import functions as F_, unet as D
    from colddiff.model2 import Normalize
    torch.manual_seed(seed)
    mod = prep(Normalize(C), seed)

    def fn(sd, x):
        y = F.group_norm(x, 32, sd["weight"], sd["bias"], eps=1e-6)
        return y * torch.sigmoid(y) if silu else y
    return _simple(mod, torch.randn(B, C, H, H) * 1.5 + 0.3, fn, lambda m, xn: F_.GroupNormFn.apply(D.anchor(xn), xn, m, silu), C, seed)
