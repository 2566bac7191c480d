"""A torch restatement of LPIPS v0.1, net = 'alex' (Zhang et al. 2018; the `lpips` package), written from the definition, in fp32 or fp64.
TEST INFRASTRUCTURE ONLY.

    x in [-1, 1] (normalize: in [0, 1], 2 x - 1 first) -> (x - shift) / scale per channel
    -> AlexNet features, tapped after the ReLU of conv1 ... conv5 (conv1 11 x 11 / 4 pad 2; 3 x 3 / 2 max pool before conv2 and conv3;
       conv2 5 x 5 pad 2; conv3 ... conv5 3 x 3 pad 1; 64, 192, 384, 256, 256 channels)
    -> per tap  f_hat = f / (sqrt(sum_c f_c^2) + 1e-10),   mean_p sum_c w_c (a_hat_pc - b_hat_pc)^2
    -> the sum over the five taps, [B, 1, 1, 1].

The rounding bound of `cdf_lpips_layer` (`layer_bound`), derived, not measured.  u = 2^-24; the kernel's per-pixel arithmetic is fp32 in
the definition's order, its sums over channels fp32 in some order, its sums over pixels fp64.  First-order terms, per pixel, C channels:
    S = fl(sum_c a_c^2):  every product within u, a sum of C non-negative terms in ANY order within (C - 1) u:   |dS| <= C u S
    n = fl(sqrt(S)):      the square root halves it and rounds once:                                             |dn| <= (C / 2 + 1) u n
    n + 1e-10:            one rounding, and 1e-10 itself taken as a float (relative 2^-24 of a part of the sum):  <= (C / 2 + 3) u
    a_hat = fl(a / .):    one rounding:                                                  |d a_hat_c| <= (C / 2 + 4) u |a_hat_c| =: delta |a_hat_c|
    d = fl(a_hat - b_hat): |d - D| <= (delta + u) E,   D = a_hat_c - b_hat_c,  E = |a_hat_c| + |b_hat_c| >= |D|
    fl(d^2):              |. - D^2| <= 2 |D| (delta + u) E + u D^2 <= (2 delta + 3 u) E^2
    fl(w fl(d^2)):        <= (2 delta + 4 u) |w| E^2
    the sum over C channels of those terms, any order: (C - 1) u of sum_c |w_c| d_c^2 <= (C - 1) u sum_c |w_c| E_c^2
  together (2 delta + 4 u + (C - 1) u) = (2 C + 11) u per pixel; the mean over the pixels in fp64 adds HW 2^-53, the second-order terms
  ((2 C u)^2 <= 4e-9 at C = 512) and that fit many times into the 5 u left below
    |dist - exact| <= 2 (C + 8) u  mean_p sum_c |w_c| (|a_hat_pc| + |b_hat_pc|)^2            (a_hat, b_hat the exact normalised vectors).
  For unit vectors and weights summing to W the right side is at most 4 W 2 (C + 8) u: 2.5e-4 W at C = 512.
`prep_ulp`: (x - shift) / scale is a subtraction and a division, both correctly rounded in the kernel and in torch: the restatement in fp32
is the same two roundings (2 x - 1 adds one more, 2 x being exact), so the kernel is held to 2 ulp of it.
"""
import torch
import torch.nn.functional as F

SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
CHANNELS = (64, 192, 384, 256, 256)
CONVS = ((0, 3, 64, 11, 4, 2), (3, 64, 192, 5, 1, 2), (6, 192, 384, 3, 1, 1), (8, 384, 256, 3, 1, 1), (10, 256, 256, 3, 1, 1))   # features.N, cin, cout, k, stride, pad
POOL_BEFORE = (3, 6)
EPS = 1e-10
U = 2.0 ** -24


def scale_input(x, normalize=False):
    """[B,3,H,W] -> the scaled input, in x's dtype (the constants are the package's fp32 tensors)."""
    shift = torch.tensor(SHIFT, dtype=torch.float32).to(x.dtype).view(1, 3, 1, 1)
    scale = torch.tensor(SCALE, dtype=torch.float32).to(x.dtype).view(1, 3, 1, 1)
    if normalize:
        x = 2 * x - 1
    return (x - shift) / scale


def taps(sd, x):
    """The five NCHW taps of the scaled input x under the torchvision-layout weights sd, in x's dtype."""
    out = []
    for i, _, _, _, stride, pad in CONVS:
        if i in POOL_BEFORE:
            x = F.max_pool2d(x, 3, 2)
        x = F.relu(F.conv2d(x, sd[f'features.{i}.weight'].to(x.dtype), sd[f'features.{i}.bias'].to(x.dtype), stride=stride, padding=pad))
        out.append(x)
    return out


def unit(f, dim):
    return f / (torch.sqrt((f * f).sum(dim, keepdim=True)) + EPS)


def layer_dist(a, b, w):
    """One tap's term for maps [B, HW, C] (channels last) and weights [C] -> [B], in the operands' dtype."""
    d = unit(a, 2) - unit(b, 2)
    return ((d * d) * w.view(1, 1, -1)).sum(2).mean(1)


def layer_bound(a, b, w):
    """The bound of the docstring for fp32-valued maps [B, HW, C] -> [B] (fp64)."""
    a, b, w = a.double(), b.double(), w.double()
    C = a.shape[2]
    e = unit(a, 2).abs() + unit(b, 2).abs()
    return 2 * (C + 8) * U * ((e * e) * w.abs().view(1, 1, -1)).sum(2).mean(1)


def lpips(sd, lins, x0, x1, normalize=False, dtype=torch.float32):
    """The distance [B, 1, 1, 1] in `dtype` (weights and images converted to it first)."""
    f0 = taps(sd, scale_input(x0.to(dtype), normalize))
    f1 = taps(sd, scale_input(x1.to(dtype), normalize))
    total = 0
    for k, (a, b) in enumerate(zip(f0, f1)):
        w = lins[f'lin{k}.model.1.weight'].to(dtype).view(1, -1, 1, 1)
        d = unit(a, 1) - unit(b, 1)
        total = total + ((d * d) * w).sum(1, keepdim=True).mean((2, 3), keepdim=True)
    return total


def norm_ratio(sd, x):
    """min over the taps of (smallest pixel norm / median pixel norm): how far every feature vector is from zero."""
    worst = float('inf')
    for f in taps(sd, scale_input(x.double())):
        n = torch.sqrt((f * f).sum(1)).reshape(-1)
        worst = min(worst, float(n.min() / n.median()))
    return worst


def random_alexnet(seed):
    """A torchvision-layout AlexNet `features` state_dict (plus a `classifier` entry a loader must ignore): nn.Conv2d's default weight
    initialisation, biases in [0.05, 0.25] so that no pixel's feature vector is near zero after the ReLU."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for i, cin, cout, k, _, _ in CONVS:
        bound = 1.0 / (cin * k * k) ** 0.5                      # kaiming_uniform_(a = sqrt 5): U(-1 / sqrt(fan_in), 1 / sqrt(fan_in))
        sd[f'features.{i}.weight'] = (torch.rand(cout, cin, k, k, generator=g) * 2 - 1) * bound
        sd[f'features.{i}.bias'] = 0.05 + 0.2 * torch.rand(cout, generator=g)
    sd['classifier.1.weight'] = torch.zeros(4, 4)
    return sd


def random_lins(seed):
    """The lpips file's layout: `lin{k}.model.1.weight` [1, C, 1, 1], non-negative."""
    g = torch.Generator().manual_seed(seed)
    return {f'lin{k}.model.1.weight': torch.rand(1, c, 1, 1, generator=g) * (2.0 / c) for k, c in enumerate(CHANNELS)}
