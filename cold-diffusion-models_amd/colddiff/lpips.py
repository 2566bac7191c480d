"""`LPIPS` — the learned perceptual image patch similarity (Zhang et al. 2018), v0.1 with the AlexNet backbone, on the HIP kernels: the
metric restoration work reports next to SSIM.  Mirrors the `lpips` package's `lpips.LPIPS(net='alex')`:

1. inputs in [-1, 1] (`normalize=True`: in [0, 1], mapped 2 x - 1 first);
2. every channel scaled, (x - shift) / scale with shift = (-.030, -.088, -.188), scale = (.458, .448, .450);
3. torchvision's AlexNet `features`, tapped after the ReLUs of conv1 ... conv5 (64, 192, 384, 256, 256 channels);
4. per tap every pixel's channel vector unit-normalised, f / (sqrt(sum_c f_c^2) + 1e-10);
5. the squared difference of the two normalised maps, a learned non-negative weight per channel (`lin{k}`, a bias-free 1 x 1 conv), summed
   over the channels, averaged over the pixels;
6. summed over the five taps -> [B, 1, 1, 1].

Neither `lpips` nor torchvision is a dependency: the architecture is restated from torchvision.models.alexnet, the module tree is
torchvision's (`features.0`, `.3`, `.6`, `.8`, `.10`) so that its `state_dict` loads unchanged.  Inference only.  Every conv is a launch of
the conv GEMM kernels with bias and ReLU in the epilogue (the 11 x 11 and the 5 x 5 layer accumulate tap sets of 16 first, as
`inception.BasicConv2d` does -- its `run` is the one used here); the pools are `inception.pool`; steps 2 and 4-5 are `csrc/k_lpips.hip`.
`distances(orig, cands)` runs the originals through the network once and scores up to four candidate sets against them per launch.

The pretrained weights are two downloads upstream (torchvision's `alexnet-owt-7be5be79.pth`, the lpips package's `weights/v0.1/alex.pth`);
offline they are read from files (`weights=` / $COLDDIFF_LPIPS_WEIGHTS, `lin=` / $COLDDIFF_LPIPS_LIN, or the torch hub cache) and a missing
file is an error, never a silent random network.
"""
import os

import torch
from torch import nn

from . import inception
from . import ops
from . import runtime as rt
from .runtime import P

ALEX_WEIGHTS_FILE = 'alexnet-owt-7be5be79.pth'
LPIPS_LIN_FILE = 'alex.pth'
CHANNELS = (64, 192, 384, 256, 256)


class ConvReLU(nn.Module):
    """nn.Conv2d(bias=True) followed by ReLU, with the parameters where torchvision keeps them (`weight`, `bias` of the Conv2d itself).
    `run` is `inception.BasicConv2d.run`: one GEMM launch, or tap sets of MAX_TAPS accumulated and cdf_act_fwd."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, kernel_size, kernel_size))
        self.bias = nn.Parameter(torch.empty(out_channels))
        self.cin, self.cout = in_channels, out_channels
        self.k, self.stride, self.pad = (kernel_size, kernel_size), stride, (padding, padding)
        nn.init.kaiming_uniform_(self.weight, a=5 ** 0.5)              # nn.Conv2d's own initialisation
        bound = 1.0 / (in_channels * kernel_size * kernel_size) ** 0.5
        nn.init.uniform_(self.bias, -bound, bound)

    def folded(self):
        return self.weight, self.bias

    run = inception.BasicConv2d.run


class AlexNetFeatures(nn.Module):
    """torchvision.models.alexnet(...).features up to the ReLU of conv5 (the last max pool feeds only the classifier), as a parameter
    container: `features.{0,3,6,8,10}.{weight,bias}`.  `run(x)`: NHWC map [B,H,W,4] (3 channels + zero pad) -> the five NHWC taps."""

    CONVS = ((0, 3, 64, 11, 4, 2), (3, 64, 192, 5, 1, 2), (6, 192, 384, 3, 1, 1), (8, 384, 256, 3, 1, 1), (10, 256, 256, 3, 1, 1))
    POOL_BEFORE = (3, 6)                                                # MaxPool2d(3, 2) in front of conv2 and conv3

    def __init__(self):
        super().__init__()
        self.features = nn.ModuleDict({str(i): ConvReLU(ci, co, k, s, p) for i, ci, co, k, s, p in self.CONVS})
        for p in self.parameters():
            p.requires_grad = False
        self.eval()

    def load_tv_state_dict(self, sd):
        """Load a torchvision `alexnet` state_dict (`features.N.weight / bias`; `classifier.*` is not part of this module)."""
        own = self.state_dict()
        missing = [k for k in own if k not in sd]
        assert not missing, f"AlexNet weights: {len(missing)} tensors missing, e.g. {missing[:3]}"
        self.load_state_dict({k: sd[k] for k in own})
        return self

    MIN_SIZE = 31                                                       # conv1 -> 7, pool -> 3, pool -> 1: the smallest input conv3 can see

    def run(self, x):
        taps = []
        # The metric must not depend on the training arithmetic (see InceptionV3.forward): parity-grade always.
        saved = rt.precision
        if saved == "bf16":
            rt.set_precision("bf16x3")
        try:
            for i, *_ in self.CONVS:
                if i in self.POOL_BEFORE:
                    x = inception.pool(x, 3, 2, 0, 'max')
                x = self.features[str(i)].run(x)
                taps.append(x)
        finally:
            if saved != rt.precision:
                rt.set_precision(saved)
        return taps


def _find(arg, env, filename, what):
    cands = [arg, os.environ.get(env), os.path.join(torch.hub.get_dir(), "checkpoints", filename)]
    for c in cands:
        if c and os.path.exists(c):
            return c
    raise FileNotFoundError(
        f"LPIPS: {what} was not found.  LPIPS(net='alex') needs two files: torchvision's AlexNet weights ({ALEX_WEIGHTS_FILE}: weights=<path> "
        f"or COLDDIFF_LPIPS_WEIGHTS) and the lpips package's linear heads (weights/v0.1/{LPIPS_LIN_FILE}: lin=<path> or COLDDIFF_LPIPS_LIN); "
        f"both are also looked for in {os.path.dirname(cands[2])} (weights='random', lin='random' build an untrained metric for tests only)")


def prep(x, normalize=False):
    """[B,3,H,W] (or [B,1,H,W], repeated) in [-1, 1] -> the scaled NHWC map [B,H,W,4] with a zero pad channel (cdf_lpips_prep_nhwc)."""
    x = rt.check(x).float()
    if x.shape[1] == 1:
        x = x.expand(-1, 3, -1, -1)
    x = x.contiguous()
    B, C, H, W = x.shape
    assert C == 3, "LPIPS takes 3-channel (or 1-channel) images"
    y = torch.empty((B, H, W, 4), device=x.device, dtype=torch.float32)
    rt.lib().cdf_lpips_prep_nhwc(P(x), P(y), 4, B, H, W, 1 if normalize else 0, rt.stream(x))
    return y


def layer_distance(a, cands, w, dist):
    """dist [K, B] (fp64, device) += one tap's term for the originals' NHWC map `a` against the candidates' maps (cdf_lpips_layer)."""
    B, H, W, C = a.shape
    L = rt.lib()
    ld = ops.ld_of(a)
    assert all(c.shape == a.shape and ops.ld_of(c) == ld for c in cands)
    partial = torch.empty((len(cands) * B * L.cdf_lpips_layer_blocks(H * W, C),), device=a.device, dtype=torch.float64)
    ptrs = [P(c) for c in cands] + [0] * (4 - len(cands))
    L.cdf_lpips_layer(P(a), *ptrs, len(cands), ld, P(w), B, H * W, C, P(partial), P(dist), rt.stream(a))
    return dist


class LPIPS(nn.Module):
    """lpips.LPIPS(net='alex', version='0.1') for inference.  weights / lin: a path, a state_dict, None (the environment variables or the
    torch hub cache) or 'random' (tests only).  The network part is torchvision's layout, the heads the lpips file's
    `lin{k}.model.1.weight` [1, C, 1, 1]."""

    def __init__(self, net='alex', weights=None, lin=None, spatial=False):
        super().__init__()
        if net != 'alex':
            raise NotImplementedError(f"LPIPS: only net='alex' is built (got {net!r})")
        if spatial:
            raise NotImplementedError("LPIPS: spatial=True (per-pixel maps) is not built")
        self.net = AlexNetFeatures()
        self.lins = nn.ParameterList([nn.Parameter(torch.rand(c) / c, requires_grad=False) for c in CHANNELS])
        if isinstance(weights, dict):
            self.net.load_tv_state_dict(weights)
        elif weights != 'random':
            self.net.load_tv_state_dict(torch.load(_find(weights, "COLDDIFF_LPIPS_WEIGHTS", ALEX_WEIGHTS_FILE, "the AlexNet weight file"), map_location='cpu'))
        if isinstance(lin, dict):
            self.load_lin_state_dict(lin)
        elif lin != 'random':
            self.load_lin_state_dict(torch.load(_find(lin, "COLDDIFF_LPIPS_LIN", LPIPS_LIN_FILE, "the file of the linear heads"), map_location='cpu'))
        self.eval()

    def load_lin_state_dict(self, sd):
        for k, p in enumerate(self.lins):
            key = f'lin{k}.model.1.weight'
            assert key in sd, f"LPIPS heads: {key} missing"
            w = sd[key]
            assert tuple(w.shape) == (1, CHANNELS[k], 1, 1), f"LPIPS heads: {key} has shape {tuple(w.shape)}"
            with torch.no_grad():
                p.copy_(w.reshape(-1))
        return self

    def features(self, x, normalize=False):
        """The five NHWC taps of a batch."""
        return self.net.run(prep(x, normalize))

    def distances(self, orig, cands, normalize=False):
        """The originals against 1...4 candidate batches of the same shape -> [K, B] fp64 on the device; the originals go through the
        network once, nothing is read back."""
        cands = list(cands)
        assert 1 <= len(cands) <= 4, "LPIPS.distances takes one to four candidate batches"
        assert all(c.shape == orig.shape for c in cands), "LPIPS.distances takes batches of one shape"
        if torch.is_grad_enabled() and any(t.requires_grad for t in [orig] + cands):
            raise NotImplementedError("LPIPS is inference-only here: no gradient (not a training loss)")
        assert min(orig.shape[-2:]) >= AlexNetFeatures.MIN_SIZE, f"LPIPS(net='alex') needs images of at least {AlexNetFeatures.MIN_SIZE} pixels a side"
        fa = self.features(orig, normalize)
        fc = [self.features(c.to(orig.device), normalize) for c in cands]
        dist = torch.zeros((len(cands), orig.shape[0]), device=orig.device, dtype=torch.float64)
        for k, a in enumerate(fa):
            layer_distance(a, [f[k] for f in fc], self.lins[k], dist)
        return dist

    def forward(self, in0, in1, normalize=False):
        """lpips.LPIPS.forward -> [B, 1, 1, 1] fp32."""
        return self.distances(in0, [in1], normalize)[0].float().view(-1, 1, 1, 1)
