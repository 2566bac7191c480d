"""The metric step after sampling: RMSE, SSIM and FID as the reference's evaluation code computes them
(deblurring_diffusion_pytorch.py:1677-1702 with Fid/fid_score.py:149-343 and pytorch_msssim.ssim).

* rmse / ssim run on the MI355X (cdf_loss_fwd, cdf_ssim_partial); there is no CPU fallback.  eval_pairs / PairStats: the same two metrics
  of up to four candidate sets against the originals in one pass per batch (cdf_eval_pairs_partial).
* FID = Frechet distance between the Gaussians fitted to InceptionV3 activations: the network is colddiff.inception.InceptionV3 (the
  reference's Fid/inception.py on the HIP kernels); its pretrained `pt_inception-2015-12-05` weights are a download upstream and are
  read from a local file here ($COLDDIFF_FID_WEIGHTS / torch hub cache).  Any other feature extractor
  `model(batch [B,3,H,W] in [0,1]) -> [B, dims]` (or a list of maps) can be passed as `model=`.
"""
import ctypes
import math

import numpy as np
import torch

from . import degrade as D
from . import runtime as rt
from .runtime import P


def rmse(a, b):
    """torch.sqrt(torch.mean((a - b) ** 2)) (DEBLUR:1678)."""
    return torch.sqrt(D.loss(rt.check(a).float().contiguous(), b.to(a.device).float().contiguous(), 'l2'))


def _gauss_window(size=11, sigma=1.5):
    """pytorch_msssim._fspecial_gauss_1d: exp(-x^2 / 2 sigma^2) on coords - size//2, normalised, fp32."""
    coords = torch.arange(size, dtype=torch.float32) - size // 2
    g = torch.exp(-(coords ** 2) / (2 * sigma ** 2))
    return g / g.sum()


def ssim(X, Y, data_range=255, size_average=True, win_size=11, win_sigma=1.5, K=(0.01, 0.03)):
    """pytorch_msssim.ssim(X, Y, data_range, size_average) for [B, C, H, W] batches, one fused kernel."""
    assert X.shape == Y.shape and X.dim() == 4, "ssim takes two [B, C, H, W] batches of the same shape"
    assert win_size == 11, "the HIP kernel is specialised for the 11-tap window the reference uses"
    X = rt.check(X).float().contiguous()
    Y = Y.to(X.device).float().contiguous()
    B, C, H, W = X.shape
    L = rt.lib()
    tiles = L.cdf_ssim_tiles(H, W)
    partial = torch.empty((B * C, tiles), device=X.device, dtype=torch.float32)
    win = (ctypes.c_float * 11)(*_gauss_window(win_size, win_sigma).tolist())
    C1, C2 = (K[0] * data_range) ** 2, (K[1] * data_range) ** 2
    L.cdf_ssim_partial(P(X), P(Y), P(partial), B * C, H, W, win, C1, C2, rt.stream(X))
    per_channel = partial.sum(1).view(B, C) / float((H - win_size + 1) * (W - win_size + 1))
    return per_channel.mean() if size_average else per_channel.mean(1)


def eval_pairs(orig, cands, shift=True, data_range=1, win_size=11, win_sigma=1.5, K=(0.01, 0.03)):
    """The originals against 1...4 candidate batches of the same [B, C, H, W] shape in ONE launch (cdf_eval_pairs_partial): the original's
    tile is read once, every candidate runs against it on chip.  `shift`: the batches are stored in [-1, 1] and taken as (v + 1) * 0.5.
    -> (sse [k], ssim_sum [k]): per candidate the fp64 sums of the squared-error and of the SSIM partials (ssim_sum over every plane's valid
    positions), as device tensors; nothing is read back."""
    cands = list(cands)
    assert 1 <= len(cands) <= 4, "eval_pairs takes one to four candidate batches"
    assert orig.dim() == 4 and all(c.shape == orig.shape for c in cands), "eval_pairs takes [B, C, H, W] batches of one shape"
    assert win_size == 11, "the HIP kernel is specialised for the 11-tap window the reference uses"
    X = rt.check(orig).float().contiguous()
    Ys = [c.to(X.device).float().contiguous() for c in cands]
    B, C, H, W = X.shape
    L = rt.lib()
    tiles = L.cdf_ssim_tiles(H, W)
    partial = torch.empty((2, len(Ys), B * C * tiles), device=X.device, dtype=torch.float32)
    win = (ctypes.c_float * 11)(*_gauss_window(win_size, win_sigma).tolist())
    C1, C2 = (K[0] * data_range) ** 2, (K[1] * data_range) ** 2
    ptrs = [P(y) for y in Ys] + [0] * (4 - len(Ys))
    L.cdf_eval_pairs_partial(P(X), *ptrs, len(Ys), 1 if shift else 0, P(partial[0]), P(partial[1]), B * C, H, W, win, C1, C2, rt.stream(X))
    sums = partial.double().sum(2)
    return sums[1], sums[0]


class PairStats:
    """Running RMSE / SSIM of named candidate sets against the originals over the batches of a sweep: `add(orig, cands)` per batch (one
    launch, sums kept on the device in fp64), `result()` at the end (the one host read) ->
    {'rmse_<name>': sqrt(SSE / count), 'ssim_<name>': S / (planes (H - 10) (W - 10))}: the whole-set `rmse` and
    `ssim(data_range=1, size_average=True)` of the concatenated sets up to summation order."""

    def __init__(self, names, shift=True):
        self.names = tuple(names)
        assert 1 <= len(self.names) <= 4
        self.shift = shift
        self.sums = None                 # [2, K] fp64 on the device: SSE, SSIM sums
        self.count = 0                   # values per set
        self.positions = 0               # valid SSIM positions per set

    def add(self, orig, cands):
        assert len(cands) == len(self.names)
        sse, ss = eval_pairs(orig, cands, shift=self.shift)
        cur = torch.stack((sse, ss))
        self.sums = cur if self.sums is None else self.sums + cur
        B, C, H, W = orig.shape
        self.count += B * C * H * W
        self.positions += B * C * (H - 10) * (W - 10)

    def result(self):
        assert self.sums is not None, "PairStats.result(): no batch was added"
        sums = self.sums.cpu()
        out = {}
        for k, name in enumerate(self.names):
            out[f'rmse_{name}'] = math.sqrt(float(sums[0, k]) / self.count)
            out[f'ssim_{name}'] = float(sums[1, k]) / self.positions
        return out


# -- FID (Fid/fid_score.py) ------------------------------------------------------------------------------------------
def calculate_frechet_distance(mu1, sigma1, mu2, sigma2, eps=1e-6):
    """d^2 = |mu1 - mu2|^2 + Tr(C1 + C2 - 2 sqrt(C1 C2)), the numerically careful form of Fid/fid_score.py:149-200
    (singular product -> eps on the diagonals; a small imaginary part from sqrtm is dropped, a large one is an error)."""
    from scipy import linalg
    mu1, mu2 = np.atleast_1d(mu1), np.atleast_1d(mu2)
    sigma1, sigma2 = np.atleast_2d(sigma1), np.atleast_2d(sigma2)
    assert mu1.shape == mu2.shape, 'Training and test mean vectors have different lengths'
    assert sigma1.shape == sigma2.shape, 'Training and test covariances have different dimensions'
    diff = mu1 - mu2
    covmean, _ = linalg.sqrtm(sigma1.dot(sigma2), disp=False)
    if not np.isfinite(covmean).all():
        print('fid calculation produces singular product; adding %s to diagonal of cov estimates' % eps)
        offset = np.eye(sigma1.shape[0]) * eps
        covmean = linalg.sqrtm((sigma1 + offset).dot(sigma2 + offset))
    if np.iscomplexobj(covmean):
        if not np.allclose(np.diagonal(covmean).imag, 0, atol=1e-3):
            raise ValueError('Imaginary component {}'.format(np.max(np.abs(covmean.imag))))
        covmean = covmean.real
    return diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2 * np.trace(covmean)


def get_activations(samples, model, batch_size=50, dims=2048, device='cuda:0'):
    """[N, dims] float64 activations of `model` over `samples` ([N, 3, H, W] in [0, 1]) (Fid/fid_score.py get_activations;
    like the reference, a trailing partial batch IS processed: drop_last=False)."""
    n = samples.shape[0]
    out = np.empty((n, dims))
    for s in range(0, n, batch_size):
        with torch.no_grad():
            pred = model(samples[s:s + batch_size].to(device))
        if isinstance(pred, (list, tuple)):
            pred = pred[0]
        if pred.dim() == 4:                                   # not yet pooled: global spatial average (dims != 2048 in the reference)
            pred = pred.mean((2, 3))
        out[s:s + pred.shape[0]] = pred.reshape(pred.shape[0], -1).double().cpu().numpy()
    return out


def calculate_activation_statistics(samples, model, batch_size=50, dims=2048, device='cuda:0'):
    act = get_activations(samples, model, batch_size, dims, device)
    return np.mean(act, axis=0), np.cov(act, rowvar=False)


def calculate_fid_given_samples(samples, batch_size=50, device='cuda:0', dims=2048, num_workers=1, model=None):
    """FID of two sample collections `samples = [A, B]` (Fid/fid_score.py:331-343).  `model`: a feature extractor to use instead of
    InceptionV3([BLOCK_INDEX_BY_DIM[dims]])."""
    if model is None:
        from .inception import InceptionV3
        model = InceptionV3([InceptionV3.BLOCK_INDEX_BY_DIM[dims]]).to(device)          # raises FileNotFoundError without the weight file
    m1, s1 = calculate_activation_statistics(samples[0], model, batch_size, dims, device)
    m2, s2 = calculate_activation_statistics(samples[1], model, batch_size, dims, device)
    return calculate_frechet_distance(m1, s1, m2, s2)
