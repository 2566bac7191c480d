"""The metric step after sampling: RMSE, SSIM and FID as the reference's evaluation code computes them
(deblurring_diffusion_pytorch.py:1677-1702 with Fid/fid_score.py:149-343 and pytorch_msssim.ssim).

* rmse / ssim run on the MI355X (cdf_loss_fwd, cdf_ssim_partial); there is no CPU fallback.  eval_pairs / PairStats: the same two metrics
  of up to four candidate sets against the originals in one pass per batch (cdf_eval_pairs_partial).
* FidStats / frechet_distance_device / DeviceFid: the same FID without the host -- fp64 statistics accumulated per batch on the device
  (cdf_moments_f64; `merge` / `all_reduce` join the accumulators of several ranks, cdf_moments_merge_f64) and both matrix square
  roots by a Newton-Schulz iteration on the fp64 matrix cores (cdf_gemm_f64).  The functions
  of Fid/fid_score.py below them stay as they are; `calculate_frechet_distance` is the fallback when the iteration does not settle.
* KidStats / kid_distance_device / DeviceFidKid: the Kernel Inception Distance of the same features (the metric torch-fidelity and
  clean-fid pair with FID; upstream has none) -- the rows kept on the device in fp64, the unbiased polynomial-kernel MMD^2 of every random
  subset in one launch pair on the fp64 matrix cores (cdf_kid_poly3_f64), torch-fidelity's draws from a private RandomState.
* knn_sq / ball_counts / prdc_device / DeviceFidKidPrdc: improved precision and recall (torch-fidelity's `prc`) and density and coverage
  of the same rows -- k-th-neighbour radii and ball memberships from fp64 Gram tiles consumed in the epilogue (cdf_knn_sq_f64,
  cdf_ball_counts_f64), no n x n matrix, one host read of four integer sums.
* LpipsStats / DeviceLpips: LPIPS v0.1 (AlexNet) of up to four candidate sets against the originals -- the network is colddiff.lpips.LPIPS
  on the conv GEMM kernels, the distance arithmetic cdf_lpips_layer; per set an fp64 device sum of the per-image distances.
* _SumStats: the `merge` and the `all_reduce` PairStats and LpipsStats share.  SweepStats: the accumulators of one Trainer evaluation
  sweep (a PairStats, the four `new_stats()` of the fid_func, an LpipsStats, the kept sets of a plain callable) behind `add(sets)`, one
  `all_reduce` and per-set `fid` / `kid` / `prdc`; metric_line / prdc_line / fid_gain_line: the sentences the sweeps print.
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


def _group_size(group=None):
    """Ranks of `group` (the default group for None); 1 without an initialised process group."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return 1
    return dist.get_world_size(group)


def _exchange_device():
    """Where a rank that holds no tensor of its own puts its part of an exchange: the GPU when there is one (RCCL carries nothing else)."""
    return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")


def _gather_rows(mine, group=None):
    """`mine` (one flat tensor of the same length on every rank) of every rank of `group` -> [world, len], rows in rank order.  The
    tensors travel as they are -- device tensors through RCCL, or through gloo (which stages them on the host itself), as
    `parallel.GradSync` hands its buckets to the backend in use: one broadcast per rank into that rank's row."""
    import torch.distributed as dist
    world, me = dist.get_world_size(group), dist.get_rank(group)
    rows = torch.empty((world, mine.numel()), device=mine.device, dtype=mine.dtype)
    rows[me].copy_(mine)
    for r in range(world):
        dist.broadcast(rows[r], src=dist.get_global_rank(group, r) if group is not None else r, group=group)
    return rows


class _SumStats:
    """What PairStats and LpipsStats share: `names`, `sums` -- an fp64 device tensor of shape `(*rows, K)`, None until the first batch --
    and the Python-int attributes named in `counts`; the one `merge` and the one `all_reduce` of both."""
    what = rows = counts = None          # set by the subclass: its name in messages, the leading shape of `sums`, the count attributes

    def __init__(self, names):
        self.names = tuple(names)
        assert 1 <= len(self.names) <= 4
        self.sums = None
        for c in self.counts:
            setattr(self, c, 0)

    def _add(self, cur, *counts):
        self.sums = cur if self.sums is None else self.sums + cur
        for c, n in zip(self.counts, counts):
            setattr(self, c, getattr(self, c) + n)

    def merge(self, other):
        """Adds the sums and counts of `other` (the same names; an instance without a batch adds nothing) -> self."""
        assert other.names == self.names, f"{self.what}.merge: the candidate sets differ"
        if other.sums is not None:
            cur = other.sums.to(self.sums.device) if self.sums is not None else other.sums.clone()
            self.sums = cur if self.sums is None else self.sums + cur
        for c in self.counts:
            setattr(self, c, getattr(self, c) + getattr(other, c))
        return self

    def all_reduce(self, group=None, device=None):
        """The sums of every rank of `group`, added in rank order in fp64 on every rank (bit-identical everywhere); a rank without a batch
        contributes zeros (on `device`: where the other ranks keep their sums).  One small exchange per sweep; without a process group,
        or alone in it, nothing happens.  -> self"""
        world = _group_size(group)
        if world == 1:
            return self
        dev = self.sums.device if self.sums is not None else torch.device(device) if device is not None else _exchange_device()
        shape, n = (*self.rows, len(self.names)), len(self.counts)
        mine = torch.zeros(math.prod(shape) + n, device=dev, dtype=torch.float64)      # sums.reshape(-1), then the counts
        if self.sums is not None:
            mine[:-n] = self.sums.reshape(-1)
        mine[-n:] = torch.tensor([getattr(self, c) for c in self.counts], dtype=torch.float64)      # (integers far below 2^53)
        parts = _gather_rows(mine, group)
        total = parts[0].clone()
        for r in range(1, world):
            total = total + parts[r]
        self.sums = total[:-n].reshape(shape).clone()
        for c, v in zip(self.counts, total[-n:].cpu()):
            setattr(self, c, int(v))
        return self


class PairStats(_SumStats):
    """Running RMSE / SSIM of named candidate sets against the originals over the batches of a sweep: `add(orig, cands)` per batch (one
    launch, sums kept on the device in fp64), `result()` at the end (the one host read) ->
    {'rmse_<name>': sqrt(SSE / count), 'ssim_<name>': S / (planes (H - 10) (W - 10))}: the whole-set `rmse` and
    `ssim(data_range=1, size_average=True)` of the concatenated sets up to summation order.
    `sums` [2, K]: SSE, SSIM sums; `count`: values per set; `positions`: valid SSIM positions per set."""
    what, rows, counts = 'PairStats', (2,), ('count', 'positions')

    def __init__(self, names, shift=True):
        super().__init__(names)
        self.shift = shift

    def add(self, orig, cands):
        assert len(cands) == len(self.names)
        sse, ss = eval_pairs(orig, cands, shift=self.shift)
        B, C, H, W = orig.shape
        self._add(torch.stack((sse, ss)), B * C * H * W, B * C * (H - 10) * (W - 10))

    def result(self):
        assert self.sums is not None, "PairStats.result(): no batch was added"
        sums = self.sums.cpu()
        out = {}
        for k, name in enumerate(self.names):
            out[f'rmse_{name}'] = math.sqrt(float(sums[0, k]) / self.count)
            out[f'ssim_{name}'] = float(sums[1, k]) / self.positions
        return out


class LpipsStats(_SumStats):
    """Running LPIPS of named candidate sets against the originals over the batches of a sweep: `add(orig, cands, model)` per batch (the
    originals' features computed once, sums of the per-image distances kept on the device in fp64), `result()` at the end (the one host
    read) -> {'lpips_<name>': the mean distance over the images}.  Batches are in [-1, 1], as PairStats takes them.
    `sums` [K]; `count`: images per set."""
    what, rows, counts = 'LpipsStats', (), ('count',)

    def add(self, orig, cands, model):
        assert len(cands) == len(self.names)
        self._add(model.distances(orig, cands).sum(1), orig.shape[0])

    def result(self):
        assert self.sums is not None, "LpipsStats.result(): no batch was added"
        sums = self.sums.cpu()
        return {f'lpips_{name}': float(sums[k]) / self.count for k, name in enumerate(self.names)}


class DeviceLpips:
    """Holds the LPIPS network for the Trainers' evaluation sweeps (`lpips=`), which feed its `new_stats(names)` per batch.  model: a
    `colddiff.lpips.LPIPS`; None builds one from **kw (`weights=`, `lin=`: raises FileNotFoundError without the two weight files)."""

    def __init__(self, model=None, device='cuda:0', **kw):
        if model is None:
            from .lpips import LPIPS
            model = LPIPS(**kw).to(device)
        self.model = model

    def new_stats(self, names):
        return LpipsStats(names)


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


def calculate_fid_given_samples(samples, batch_size=50, device='cuda:0', dims=2048, num_workers=1, model=None, on_device=False):
    """FID of two sample collections `samples = [A, B]` (Fid/fid_score.py:331-343).  `model`: a feature extractor to use instead of
    InceptionV3([BLOCK_INDEX_BY_DIM[dims]]).  `on_device`: statistics and distance on the device (DeviceFid) instead of numpy / scipy."""
    if on_device:
        return DeviceFid(model=model, dims=dims, batch_size=batch_size, device=device)(samples=samples)
    if model is None:
        from .inception import InceptionV3
        model = InceptionV3([InceptionV3.BLOCK_INDEX_BY_DIM[dims]]).to(device)          # raises FileNotFoundError without the weight file
    m1, s1 = calculate_activation_statistics(samples[0], model, batch_size, dims, device)
    m2, s2 = calculate_activation_statistics(samples[1], model, batch_size, dims, device)
    return calculate_frechet_distance(m1, s1, m2, s2)


# -- FID on the device ---------------------------------------------------------------------------------------------------
def gemm_f64(a, b, out=None, alpha=1.0, diag=0.0):
    """out[m, n] = alpha * a[m, k] @ b[k, n] + diag * I in fp64 on the matrix cores (cdf_gemm_f64); out must not alias a or b."""
    assert a.dtype == b.dtype == torch.float64 and a.dim() == b.dim() == 2 and a.shape[1] == b.shape[0]
    assert a.stride(1) == 1 and b.stride(1) == 1, "gemm_f64 takes row-major operands"
    rt.check(a)
    m, k = a.shape
    n = b.shape[1]
    if out is None:
        out = torch.empty((m, n), device=a.device, dtype=torch.float64)
    assert out.shape == (m, n) and out.dtype == torch.float64 and out.stride(1) == 1
    rt.lib().cdf_gemm_f64(P(a), a.stride(0), P(b), b.stride(0), P(out), out.stride(0), m, n, k, float(alpha), float(diag), rt.stream(a))
    return out


class FidStats:
    """Running mean / covariance of feature rows, on the device in fp64: `add(features)` per batch (one cdf_moments_f64 launch, nothing
    read back), `mean()` / `cov()` device tensors, `result()` the one host read -> (mu, sigma) as `calculate_activation_statistics`
    returns them.  The first batch's column mean is the pivot every row is centred on before it is squared, so the one-pass formula
    cov = (outer - sum sum^T / n) / (n - 1) does not cancel."""

    def __init__(self, dims, device):
        self.dims = int(dims)
        self.device = torch.device(device)
        self.n = 0
        self.pivot = None
        self.sum = torch.zeros(self.dims, device=self.device, dtype=torch.float64)
        self.outer = torch.zeros((self.dims, self.dims), device=self.device, dtype=torch.float64)     # upper block triangle (64 x 64 tiles)
        self._mu = self._sigma = None                                                                 # set by load(): frozen
        self._n_known = True                                                                          # False: loaded from a file without n

    @staticmethod
    def _rows(features):
        if isinstance(features, (list, tuple)):
            features = features[0]
        rt.check(features)
        if features.dim() == 4:                                   # not yet pooled: global spatial average, as get_activations
            features = features.mean((2, 3))
        return features.reshape(features.shape[0], math.prod(features.shape[1:])).float().contiguous()      # (-1 is ambiguous for an empty batch)

    def add(self, features):
        if self._mu is not None:
            raise RuntimeError("FidStats.add: statistics loaded from a file are frozen")
        f = self._rows(features)
        assert f.shape[1] == self.dims, "FidStats(dims=%d).add: got %d features per row" % (self.dims, f.shape[1])
        if f.shape[0] == 0:
            return self
        if self.pivot is None:
            self.pivot = f.double().mean(0)
        rt.lib().cdf_moments_f64(P(f), f.stride(0), f.shape[0], self.dims, P(self.pivot), P(self.sum), P(self.outer), self.outer.stride(0),
                                 rt.stream(f))
        self.n += f.shape[0]
        return self

    def _parts(self):
        """(n, pivot, sum, outer) as `merge` reads them; loaded statistics enter as pivot = mu, sum = 0, outer = (n - 1) sigma."""
        if self._mu is None:
            return self.n, self.pivot, self.sum, self.outer
        if not self._n_known:
            raise ValueError("FidStats.merge: the statistics were loaded from a file saved without n (the row count weighs them)")
        return self.n, self._mu, torch.zeros_like(self._mu), self._sigma * float(self.n - 1)

    def merge(self, other):
        """Adds the rows `other` has seen: one cdf_moments_merge_f64 launch, nothing read back; `self` then holds the statistics of the
        union of rows, on its own pivot.  `other` is left as it is.  An empty `other` is a no-op; an empty `self` adopts a copy.  -> self"""
        if self._mu is not None:
            raise RuntimeError("FidStats.merge: statistics loaded from a file are frozen")
        if other.dims != self.dims:
            raise ValueError("FidStats(dims=%d).merge: the other statistics have dims=%d" % (self.dims, other.dims))
        n, pivot, s, outer = other._parts()
        if n == 0:
            return self
        pivot, s, outer = (z.to(self.device) for z in (pivot, s, outer))
        if self.n == 0:
            self.pivot = pivot.clone()
            self.sum.copy_(s)
            self.outer.copy_(outer)
        else:
            assert outer.stride(1) == 1 and s.is_contiguous() and pivot.is_contiguous()
            rt.check(outer)
            rt.lib().cdf_moments_merge_f64(float(n), P(pivot), P(s), P(outer), outer.stride(0), P(self.pivot), P(self.sum), P(self.outer),
                                           self.outer.stride(0), self.dims, rt.stream(outer))
        self.n += n
        return self

    def all_reduce(self, group=None):
        """The statistics of the rows of EVERY rank of `group`, on every rank: each rank's (n, pivot, sum, outer) is gathered (one
        exchange per sweep) and the parts are merged in rank order, starting from the first rank that saw a row -- so every rank ends
        with bit-identical statistics whatever order the parts arrived in.  Ranks that added nothing take part.  Without a process group,
        or alone in it, `self` is returned untouched."""
        world = _group_size(group)
        if world == 1:
            return self
        if self._mu is not None:
            raise RuntimeError("FidStats.all_reduce: statistics loaded from a file are frozen")
        d = self.dims
        mine = torch.zeros(1 + 2 * d + d * d, device=self.device, dtype=torch.float64)
        mine[0] = self.n
        if self.n:
            mine[1:1 + d], mine[1 + d:1 + 2 * d] = self.pivot, self.sum
            mine[1 + 2 * d:] = self.outer.reshape(-1)
        rows = _gather_rows(mine, group)
        counts = [int(v) for v in rows[:, 0].cpu()]
        total, part = FidStats(d, self.device), FidStats(d, self.device)
        for r in range(world):
            if counts[r]:                                             # (`part`: views of row r; merge copies what it adopts)
                part.n, part.pivot, part.sum, part.outer = counts[r], rows[r, 1:1 + d], rows[r, 1 + d:1 + 2 * d], rows[r, 1 + 2 * d:].view(d, d)
                total.merge(part)
        self.n, self.pivot, self.sum, self.outer = total.n, total.pivot, total.sum, total.outer
        return self

    def add_images(self, samples, model, batch_size=50):
        """The extractor batch by batch over `samples` [N, 3, H, W] in [0, 1] (a trailing partial batch included, as get_activations)."""
        for s in range(0, samples.shape[0], batch_size):
            with torch.no_grad():
                self.add(model(samples[s:s + batch_size].to(self.device)))
        return self

    def mean(self):
        if self._mu is not None:
            return self._mu
        assert self.n >= 1, "FidStats.mean(): no batch was added"
        return self.pivot + self.sum / self.n

    def cov(self):
        if self._sigma is not None:
            return self._sigma
        assert self.n >= 2, "FidStats.cov(): needs at least two rows"
        up = torch.triu(self.outer)
        full = up + torch.triu(self.outer, 1).t()
        return (full - torch.outer(self.sum, self.sum) / self.n) / (self.n - 1)

    def result(self):
        both = torch.cat((self.mean()[None], self.cov())).cpu().numpy()
        return both[0], both[1:]

    def save(self, path):
        mu, sigma = self.result()
        with open(path, "wb") as f:                               # (a file object: np.savez would append .npz to a bare name)
            np.savez(f, mu=mu, sigma=sigma, n=np.int64(self.n))

    @classmethod
    def load(cls, path, device):
        z = np.load(path)
        st = cls(z["mu"].shape[0], device)
        st._mu = torch.from_numpy(np.ascontiguousarray(z["mu"], dtype=np.float64)).to(st.device)
        st._sigma = torch.from_numpy(np.ascontiguousarray(z["sigma"], dtype=np.float64)).to(st.device)
        st.n = int(z["n"]) if "n" in z.files else 0
        st._n_known = "n" in z.files
        return st


NS_CAP = 64            # Newton-Schulz steps per square root
NS_FLOOR = 1e-9        # a rise of delta below this is the noise floor (see _sqrt_newton_schulz)


def _sqrt_newton_schulz(A, max_iter=NS_CAP):
    """sqrt of a symmetric positive semi-definite fp64 device matrix by the coupled Newton-Schulz iteration on cdf_gemm_f64:
    c = |A|_F, Y0 = A / c, Z0 = I;  T = 1.5 I - 0.5 Z Y (one launch);  Y <- Y T, Z <- T Z;  sqrt(A) = sqrt(c) Y.
    A rank-deficient A (every covariance of N < dims rows) makes the unbounded iteration diverge, so it stops by rule on
    tr = Tr Y, the one scalar read per step: delta = |tr - tr_prev| / |tr|; stop with the new iterate at delta <= 1e-13, with the
    previous one once delta_prev < NS_FLOOR = 1e-9 and delta >= delta_prev (the noise floor), fail at the cap or on a non-finite value.
    Why 1e-9 and not 1e-6: an eigenvalue l << c enters Tr Y as ~(l / c) 1.5^k while it still grows, so delta RISES for a few steps
    whenever a cluster of small eigenvalues is on its way up -- at d = 768, N = 64 delta went 5.93e-7, 6.70e-7, 5.44e-7, ... and the
    iteration settled five steps later, 1.5e-6 of Tr sqrt further on.  A rise below 1e-9 at step k >= 14 can only come from eigenvalues
    under ~1e-9 / 1.5^14 = 3e-12 of c; after convergence delta sits at 1e-13 ... 1e-11 and creeps up from there, so the first rise
    below 1e-9 is met within a step or two of it.
    -> (root or None, steps taken)"""
    d = A.shape[0]
    c = float(torch.linalg.norm(A))
    if not math.isfinite(c):
        return None, 0
    if c == 0.0:
        return torch.zeros_like(A), 0
    Y = A / c
    Z = torch.eye(d, device=A.device, dtype=torch.float64)
    T, Yn, Zn = torch.empty_like(Y), torch.empty_like(Y), torch.empty_like(Y)
    tr_prev, d_prev = float(torch.trace(Y)), math.inf
    for it in range(1, max_iter + 1):
        gemm_f64(Z, Y, out=T, alpha=-0.5, diag=1.5)
        gemm_f64(Y, T, out=Yn)
        gemm_f64(T, Z, out=Zn)
        tr = float(torch.trace(Yn))
        if not math.isfinite(tr) or tr == 0.0:
            return None, it
        delta = abs(tr - tr_prev) / abs(tr)
        if delta <= 1e-13:
            return Yn * math.sqrt(c), it
        if d_prev < NS_FLOOR and delta >= d_prev:
            return Y * math.sqrt(c), it
        Y, Yn = Yn, Y
        Z, Zn = Zn, Z
        tr_prev, d_prev = tr, delta
    return None, max_iter


def frechet_distance_device(s1, s2, eps=1e-6, _max_iter=NS_CAP, _info=None):
    """d^2 = |mu1 - mu2|^2 + Tr C1 + Tr C2 - 2 Tr sqrt(C1 C2) of two FidStats, on the device: Tr sqrt(C1 C2) = Tr sqrt(S1 C2 S1) with
    S1 = sqrt(C1), both roots by `_sqrt_newton_schulz`, M = S1 C2 S1 symmetrised in between.  If a root does not settle (cap, non-finite
    value) one line says so and the host `calculate_frechet_distance(..., eps)` of the same statistics is returned.
    `_info` (a dict) receives the step counts and Tr sqrt(C1 C2)."""
    mu1, mu2, C1, C2 = s1.mean(), s2.mean(), s1.cov(), s2.cov()
    assert mu1.shape == mu2.shape, 'Training and test mean vectors have different lengths'
    assert C1.shape == C2.shape, 'Training and test covariances have different dimensions'
    info = {} if _info is None else _info
    info.update(iters=(0, 0), tr_sqrt=None, fallback=False)
    S1, it1 = _sqrt_newton_schulz(C1, _max_iter)
    it2, tr_sqrt = 0, None
    if S1 is not None:
        M = gemm_f64(S1, gemm_f64(C2, S1))
        M = (M + M.t()) * 0.5
        S2, it2 = _sqrt_newton_schulz(M, _max_iter)
        if S2 is not None:
            tr_sqrt = float(torch.trace(S2))
    info["iters"] = (it1, it2)
    diff = mu1 - mu2
    if tr_sqrt is None or not math.isfinite(tr_sqrt):
        print('fid on the device: the square-root iteration did not settle within %d steps; using the host calculate_frechet_distance'
              % _max_iter)
        info["fallback"] = True
        return float(calculate_frechet_distance(mu1.cpu().numpy(), C1.cpu().numpy(), mu2.cpu().numpy(), C2.cpu().numpy(), eps))
    info["tr_sqrt"] = tr_sqrt
    return float(diff.dot(diff) + torch.trace(C1) + torch.trace(C2)) - 2.0 * tr_sqrt


class DeviceFid:
    """FID with the statistics and the distance on the device: a drop-in `fid_func` (`__call__(samples=[A, B]) -> float`) for the
    Trainers' evaluation methods, which feed its `new_stats()` per batch instead of keeping the image sets."""

    def __init__(self, model=None, dims=2048, batch_size=50, device='cuda:0'):
        if model is None:
            from .inception import InceptionV3
            model = InceptionV3([InceptionV3.BLOCK_INDEX_BY_DIM[dims]]).to(device)      # raises FileNotFoundError without the weight file
        self.model, self.dims, self.batch_size, self.device = model, dims, batch_size, torch.device(device)

    def new_stats(self):
        return FidStats(self.dims, self.device)

    def stats(self, samples):
        return self.new_stats().add_images(samples, self.model, self.batch_size)

    def distance(self, s1, s2):
        return frechet_distance_device(s1, s2)

    def __call__(self, samples):
        return self.distance(self.stats(samples[0]), self.stats(samples[1]))


# -- KID on the device ---------------------------------------------------------------------------------------------------
def kid_poly3(x, y, ix, iy, gamma=None, coef0=1.0):
    """out[nsub, 4] = (sxx, syy, sxy, mmd2) per subset of the cubic polynomial kernel k(a, b) = (gamma a.b + coef0)^3 (gamma: 1 / d),
    in fp64 on the matrix cores (cdf_kid_poly3_f64): x [n1, d], y [n2, d] fp64 row-major, ix / iy [nsub, m] int32 row numbers into
    x / y -- every one of them must be a row of its matrix, nothing checks them on the device."""
    assert x.dtype == y.dtype == torch.float64 and x.dim() == y.dim() == 2 and x.shape[1] == y.shape[1]
    assert x.stride(1) == 1 and y.stride(1) == 1, "kid_poly3 takes row-major feature matrices"
    assert ix.dtype == iy.dtype == torch.int32 and ix.dim() == 2 and ix.shape == iy.shape and ix.is_contiguous() and iy.is_contiguous()
    assert x.device == y.device == ix.device == iy.device
    rt.check(x)
    (nsub, m), d = ix.shape, x.shape[1]
    L = rt.lib()
    partial = torch.empty(nsub * 3 * max(1, L.cdf_kid_tiles(m)), device=x.device, dtype=torch.float64)
    out = torch.empty((nsub, 4), device=x.device, dtype=torch.float64)
    L.cdf_kid_poly3_f64(P(x), x.stride(0), P(ix), P(y), y.stride(0), P(iy), nsub, m, d, 1.0 / d if gamma is None else float(gamma),
                        float(coef0), P(partial), P(out), rt.stream(x))
    return out


class KidStats:
    """The feature rows of an image set, kept on the device in fp64 for the Kernel Inception Distance: `add(features)` per batch (the
    inputs of `FidStats.add`; nothing read back), `merge` / `all_reduce` to join the rows of several accumulators or ranks, `rows()` the
    [n, dims] matrix.  KID draws subsets of rows, so unlike FID it has no running summary: 16 KB per image at dims = 2048."""

    def __init__(self, dims, device):
        self.dims = int(dims)
        self.device = torch.device(device)
        self.n = 0
        self._chunks = []

    def add(self, features):
        f = FidStats._rows(features)
        assert f.shape[1] == self.dims, "KidStats(dims=%d).add: got %d features per row" % (self.dims, f.shape[1])
        if f.shape[0]:
            self._chunks.append(f.double())
            self.n += f.shape[0]
        return self

    add_images = FidStats.add_images

    def rows(self):
        if len(self._chunks) != 1:
            self._chunks = [torch.cat(self._chunks) if self._chunks else torch.empty((0, self.dims), device=self.device, dtype=torch.float64)]
        return self._chunks[0]

    def merge(self, other):
        """Appends the rows of `other` (left as it is) below this one's.  -> self"""
        if other.dims != self.dims:
            raise ValueError("KidStats(dims=%d).merge: the other rows have dims=%d" % (self.dims, other.dims))
        if other.n:
            self._chunks.append(other.rows().to(self.device))
            self.n += other.n
        return self

    def all_reduce(self, group=None):
        """The rows of EVERY rank of `group`, concatenated in rank order, on every rank: the counts are exchanged first and each rank's
        rows travel padded to the largest, so every rank ends with the same matrix (and the same subsets of it).  Ranks that added nothing
        take part.  Without a process group, or alone in it, `self` is returned untouched."""
        world = _group_size(group)
        if world == 1:
            return self
        counts = [int(v) for v in _gather_rows(torch.tensor([float(self.n)], device=self.device, dtype=torch.float64), group)[:, 0].cpu()]
        if max(counts):
            mine = torch.zeros(max(counts) * self.dims, device=self.device, dtype=torch.float64)
            mine[:self.n * self.dims] = self.rows().reshape(-1)
            parts = _gather_rows(mine, group)
            self._chunks = [torch.cat([parts[r, :c * self.dims].view(c, self.dims) for r, c in enumerate(counts)])]
            self.n = sum(counts)
        return self


def kid_subset_indices(n1, n2, subsets, m, seed):
    """The draws of torch-fidelity's `kid`: one `RandomState(seed)`; per subset `choice(n1, m, replace=False)`, then
    `choice(n2, m, replace=False)`.  numpy's global stream is not touched.  -> (ix, iy) int32 [subsets, m]"""
    rng = np.random.RandomState(seed)
    ix, iy = np.empty((subsets, m), dtype=np.int32), np.empty((subsets, m), dtype=np.int32)
    for s in range(subsets):
        ix[s] = rng.choice(n1, m, replace=False)
        iy[s] = rng.choice(n2, m, replace=False)
    return ix, iy


def kid_distance_device(s1, s2, subsets=100, subset_size=1000, seed=2020):
    """Kernel Inception Distance of two KidStats -> (mean, std) over `subsets` random subsets of `subset_size` rows each (None: the
    smaller row count) of the unbiased MMD^2 with k(a, b) = (a.b / dims + 1)^3 -- torch-fidelity's estimator, defaults and draw order
    (`kid_subset_indices`), so the value is comparable with that tool's on the same features.  Every subset in one launch pair
    (`kid_poly3`), one host read of the `subsets` values."""
    lo = min(s1.n, s2.n)
    m = lo if subset_size is None else int(subset_size)
    if m > lo or m < 2:
        raise ValueError("kid: subset_size = %d must be at least 2 and at most the smaller row count, min(%d, %d) = %d"
                         % (m, s1.n, s2.n, lo))
    assert s1.dims == s2.dims, 'Training and test feature rows have different lengths'
    assert subsets >= 1
    x, y = s1.rows(), s2.rows()
    ix, iy = (torch.from_numpy(z).to(x.device) for z in kid_subset_indices(s1.n, s2.n, subsets, m, seed))
    vals = kid_poly3(x, y.to(x.device), ix, iy)[:, 3].cpu().numpy()
    return float(np.mean(vals)), float(np.std(vals))


class FidKidStats(FidStats):
    """A FidStats that also keeps the rows (`kid_stats`, a KidStats): one extractor pass feeds both metrics."""

    def __init__(self, dims, device):
        super().__init__(dims, device)
        self.kid_stats = KidStats(dims, device)

    def add(self, features):
        f = self._rows(features)
        super().add(f)
        self.kid_stats.add(f)
        return self

    def merge(self, other):
        super().merge(other)
        self.kid_stats.merge(other.kid_stats)
        return self

    def all_reduce(self, group=None):
        super().all_reduce(group)
        self.kid_stats.all_reduce(group)
        return self


class DeviceFidKid(DeviceFid):
    """DeviceFid whose `new_stats()` also keep the feature rows: `distance` is the FID as before, `kid(s1, s2) -> (mean, std)` the Kernel
    Inception Distance of the same two sets (`kid_distance_device` with this object's `kid_subsets`, `kid_subset_size`, `kid_seed`).  The
    Trainers' sweeps add `kid_<name>` / `kid_std_<name>` beside every `fid_<name>` when their fid_func has `kid`."""

    def __init__(self, model=None, dims=2048, batch_size=50, device='cuda:0', kid_subsets=100, kid_subset_size=1000, kid_seed=2020):
        super().__init__(model=model, dims=dims, batch_size=batch_size, device=device)
        self.kid_subsets, self.kid_subset_size, self.kid_seed = kid_subsets, kid_subset_size, kid_seed

    def new_stats(self):
        return FidKidStats(self.dims, self.device)

    def kid(self, s1, s2):
        return kid_distance_device(s1.kid_stats, s2.kid_stats, self.kid_subsets, self.kid_subset_size, self.kid_seed)


# -- precision / recall / density / coverage on the device -------------------------------------------------------------------------------
def _f64_rows(t, what):
    assert t.dtype == torch.float64 and t.dim() == 2 and t.stride(1) == 1, "%s takes a row-major fp64 matrix" % what
    return rt.check(t)


def row_norms_sq(x):
    """|x_j|^2 per row of a row-major fp64 matrix, one fixed-order tree per row (cdf_rowsumsq_f64): the norm vector `knn_sq` and
    `ball_counts` take, computed once per set and shared by every pass."""
    _f64_rows(x, "row_norms_sq")
    out = torch.empty(x.shape[0], device=x.device, dtype=torch.float64)
    rt.lib().cdf_rowsumsq_f64(P(x), x.stride(0), x.shape[0], x.shape[1], P(out), rt.stream(x))
    return out


def knn_sq(x, k, norms=None):
    """knn[n, k], ascending: the k smallest squared distances D(x_j, x_l) = max(0, |x_j|^2 + |x_l|^2 - 2 x_j.x_l), l != j, of every row
    of x [n, d] (fp64, row-major, any row pitch) to the other rows of the set, on the fp64 matrix cores (cdf_knn_sq_f64).  Self is left out
    by position: a second row with the same values is a neighbour at distance 0.  1 <= k <= 8 and n >= k + 1, else CdfError.
    `norms`: `row_norms_sq(x)` when the caller has it already."""
    _f64_rows(x, "knn_sq")
    n, d = x.shape
    norms = row_norms_sq(x) if norms is None else norms
    assert norms.dtype == torch.float64 and norms.shape == (n,) and norms.is_contiguous() and norms.device == x.device
    L = rt.lib()
    partial = torch.empty(max(1, L.cdf_knn_splits(n)) * n * max(int(k), 1), device=x.device, dtype=torch.float64)
    out = torch.empty((n, max(int(k), 0)), device=x.device, dtype=torch.float64)
    L.cdf_knn_sq_f64(P(x), x.stride(0), n, d, int(k), P(norms), P(partial), P(out), rt.stream(x))
    return out


def ball_counts(a, b, rcol=None, rrow=None, anorm=None, bnorm=None):
    """(cnt_col, cnt_row), int32 [na] each, for the rows of a [na, d] against the rows of b [nb, d] (fp64, row-major, any row pitch):
    cnt_col[i] = #{ j : D(a_i, b_j) <= rcol[j] } (rcol [nb]: a radius per row of b), cnt_row[i] = #{ j : D(a_i, b_j) <= rrow[i] } (rrow
    [na]: a radius per row of a); both from one walk of the Gram tiles (cdf_ball_counts_f64), `None` for the side not asked for.  D is the
    squared distance of `knn_sq`, `<=` includes ties, no row is left out (a and b are different sets)."""
    _f64_rows(a, "ball_counts")
    _f64_rows(b, "ball_counts")
    assert a.shape[1] == b.shape[1] and a.device == b.device
    (na, d), nb = a.shape, b.shape[0]
    anorm = row_norms_sq(a) if anorm is None else anorm
    bnorm = row_norms_sq(b) if bnorm is None else bnorm
    for v, rows in ((anorm, na), (bnorm, nb), (rcol, nb), (rrow, na)):
        assert v is None or (v.dtype == torch.float64 and v.shape == (rows,) and v.is_contiguous() and v.device == a.device)
    L = rt.lib()
    partial = torch.empty(max(1, L.cdf_ball_splits(na, nb)) * na * 2, device=a.device, dtype=torch.int32)
    cnt_col = None if rcol is None else torch.empty(na, device=a.device, dtype=torch.int32)
    cnt_row = None if rrow is None else torch.empty(na, device=a.device, dtype=torch.int32)
    L.cdf_ball_counts_f64(P(a), a.stride(0), na, P(anorm), P(b), b.stride(0), nb, P(bnorm), d, P(rcol), P(rrow), P(partial), P(cnt_col),
                          P(cnt_row), rt.stream(a))
    return cnt_col, cnt_row


def prdc_device(s1, s2, k=3):
    """Improved precision and recall (Kynkaanniemi et al. 2019; torch-fidelity's `prc`) and density and coverage (Naeem et al. 2020) of
    two KidStats -- s1 the originals X (n rows), s2 the candidates Y (m rows) -- as dict(precision, recall, density, coverage, f_score).
    With D the squared Euclidean distance in fp64 and rho_S(j) the k-th smallest D of row j of S to the OTHER rows of S (self left out by
    position, a duplicate row is a neighbour at 0):
        precision = #{ i : exists j, D(y_i, x_j) <= rho_X(j) } / m        recall   = #{ j : exists i, D(x_j, y_i) <= rho_Y(i) } / n
        density   = sum_i #{ j : D(y_i, x_j) <= rho_X(j) } / (k m)        coverage = #{ j : exists i, D(x_j, y_i) <= rho_X(j) } / n
        f_score   = 2 precision recall / max(precision + recall, 1e-5)
    `<=` throughout, which is torch-fidelity's choice for precision and recall; Naeem's reference code compares with `<`.  The two differ
    only where a distance equals a radius exactly.  The counts are integers, so the numbers do not depend on any summation order nor on
    the order of the rows within either set.  Features must be finite (not checked).
    Two norm launches, two `knn_sq`, two `ball_counts` -- (Y rows, X columns, rcol = rho_X) for precision and density, (X rows, Y
    columns, rcol = rho_Y, rrow = rho_X) for recall and coverage -- and ONE host read, of the four integer sums."""
    k = int(k)
    if not 1 <= k <= 8 or min(s1.n, s2.n) < k + 1:
        raise ValueError("prdc: k = %d must be in 1...8 and both sets need at least k + 1 rows (got %d and %d)" % (k, s1.n, s2.n))
    assert s1.dims == s2.dims, 'Training and test feature rows have different lengths'
    x = s1.rows()
    y = s2.rows().to(x.device)
    nx, ny = row_norms_sq(x), row_norms_sq(y)
    rho_x = knn_sq(x, k, nx)[:, k - 1].contiguous()
    rho_y = knn_sq(y, k, ny)[:, k - 1].contiguous()
    in_x, _ = ball_counts(y, x, rcol=rho_x, anorm=ny, bnorm=nx)                           # per y_i: the X balls it lies in
    in_y, own = ball_counts(x, y, rcol=rho_y, rrow=rho_x, anorm=nx, bnorm=ny)             # per x_j: the Y balls it lies in; the y in its own
    sums = torch.stack(((in_x > 0).sum(), in_x.sum(dtype=torch.int64), (in_y > 0).sum(), (own > 0).sum())).cpu().tolist()
    n, m = s1.n, s2.n
    precision, density, recall, coverage = sums[0] / m, sums[1] / (k * m), sums[2] / n, sums[3] / n
    return dict(precision=precision, recall=recall, density=density, coverage=coverage,
                f_score=2.0 * precision * recall / max(precision + recall, 1e-5))


class DeviceFidKidPrdc(DeviceFidKid):
    """DeviceFidKid with `prdc(s1, s2)`: the dict of `prdc_device` (neighbourhood size `prdc_k`) of the same two sets' rows.  The
    Trainers' sweeps add `precision_<name>`, `recall_<name>`, `density_<name>`, `coverage_<name>` and `f_score_<name>` after
    `kid_std_<name>` when their fid_func has `prdc`."""

    def __init__(self, model=None, dims=2048, batch_size=50, device='cuda:0', kid_subsets=100, kid_subset_size=1000, kid_seed=2020, prdc_k=3):
        super().__init__(model=model, dims=dims, batch_size=batch_size, device=device, kid_subsets=kid_subsets,
                         kid_subset_size=kid_subset_size, kid_seed=kid_seed)
        self.prdc_k = prdc_k

    def prdc(self, s1, s2):
        return prdc_device(s1.kid_stats, s2.kid_stats, self.prdc_k)


# -- the accumulators and the printed lines of an evaluation sweep -----------------------------------------------------------------------
class SweepStats:
    """The accumulators of one `fid_distance_decrease_from_manifold` sweep over the originals and the candidate sets `names`: `pairs` (a
    PairStats; None with pairs=False), `fstats` (one `fid.new_stats()` per set, the originals' first, when `fid` has `new_stats`), `lstats`
    (`lpips.new_stats(names)` when `lpips` is given) and, with keep=True, the [0, 1] sets a plain callable `fid` and the whole-set metrics
    need.  `fid(k)`, `kid(k)`, `prdc(k)` of candidate set k compute when asked: launches, host reads and lines fall where the sweep asks."""

    def __init__(self, names, fid=None, lpips=None, keep=False, pairs=True):
        self.names, self.fid_func, self.lpips = tuple(names), fid, lpips
        self.pairs = PairStats(names) if pairs else None
        self.fstats = [fid.new_stats() for _ in range(1 + len(self.names))] if hasattr(fid, 'new_stats') else []
        self.lstats = lpips.new_stats(names) if lpips is not None else None
        self.sets = [[] for _ in range(1 + len(self.names))] if keep else None
        self.has_kid, self.has_prdc = hasattr(fid, 'kid'), hasattr(fid, 'prdc')

    def add(self, sets):
        """sets = [orig, *cands]: 3-channel batches in [-1, 1]."""
        if self.pairs is not None:
            self.pairs.add(sets[0], sets[1:])
        if self.lstats is not None:
            self.lstats.add(sets[0], sets[1:], self.lpips.model)
        if self.sets is not None:
            for dst, z in zip(self.sets, sets):
                dst.append((z + 1) * 0.5)
        for st, z in zip(self.fstats, sets):
            st.add_images((z + 1) * 0.5, self.fid_func.model, self.fid_func.batch_size)

    def all_reduce(self, device):
        for st in (self.pairs, self.lstats):
            if st is not None:
                st.all_reduce(device=device)
        for st in self.fstats:
            st.all_reduce()

    def kept(self):
        """[orig, *cands] in [0, 1], each concatenated over the batches (keep=True): the one place a sweep concatenates image sets."""
        if isinstance(self.sets[0], list):
            self.sets = [torch.cat(z, dim=0) for z in self.sets]
        return self.sets

    def fid(self, k):
        if self.fstats:
            return self.fid_func.distance(self.fstats[0], self.fstats[k + 1])
        return self.fid_func(samples=[self.kept()[0], self.kept()[k + 1]])

    def kid(self, k):
        return self.fid_func.kid(self.fstats[0], self.fstats[k + 1])

    def prdc(self, k):
        return self.fid_func.prdc(self.fstats[0], self.fstats[k + 1])


PRDC_KEYS = ('precision', 'recall', 'density', 'coverage', 'f_score')


def metric_line(metric, word, value, std=None):
    """The sentence both sweeps print per metric and set; with `std` the KID form "value +- std"."""
    return f"The {metric} of {word} images with original image is {value}" + ("" if std is None else f" +- {std}")


def prdc_line(word, prdc):
    return metric_line('precision / recall / density / coverage / F-score', word, ' / '.join(str(prdc[key]) for key in PRDC_KEYS))


def put_prdc(out, name, prdc):
    out.update({f'{key}_{name}': prdc[key] for key in PRDC_KEYS})


def fid_gain_line(out, name):
    return f"Hence the improvement in FID using {'sampling' if name == 'deblur' else 'direct sampling'} is {out['fid_blur'] - out[f'fid_{name}']}"
