"""Gaussian mixture on the device: the `torch_gmm` the reference's generation scripts fit on the GPU (`pycave.bayes.GaussianMixture`,
deblurring_diffusion_pytorch.py:1391-1564 and the `*_test.py` drivers), with pycave's interface as those scripts call it and
scikit-learn's EM arithmetic -- upstream's own library for the vector samplers -- in fp64 on the HIP kernels of csrc/k_gmm.hip and on
`cdf_gemm_f64`:

    M-step   nk, resp                 cdf_gmm_resp_f64 (of the E-step before it)
             means = resp X / nk      cdf_gemm_f64
             Z_k = sqrt(r_k / nk) (X - mu_k), Z_k^T          cdf_gmm_center_scale_f64
             cov_k = Z_k^T Z_k + reg I                       cdf_gemm_f64 (its `diag` argument)
             L_k = chol(cov_k), P_k^T = L_k^-T               cdf_potrf_f64, cdf_trtri_lower_f64   (`_compute_precision_cholesky`)
    E-step   Y_k = (X - mu_k) P_k^T, maha_k = rowsum Y_k^2   cdf_gmm_center_scale_f64, cdf_gemm_f64, cdf_rowsumsq_f64
             log det, responsibilities, sum of log-likelihoods   cdf_logdet_diag_f64, cdf_gmm_resp_f64

The fit is full-batch with one host read per iteration (the lower bound and the Cholesky `info` words, one buffer).  It is opt-in: no
Trainer method uses it unless it is passed as `torch_gmm` or asked for with `device_gmm=True`.  Sizes: a fit at D = 3 is a few dozen tiny
launches per iteration and gains nothing over the host library; the class is for the vector samplers' D = siz * siz * ch features
(profiles/gmm_device.md).

Initialisation without `*_init` is k-means (k-means++ seeding from a CPU `torch.Generator(random_state)`, Lloyd iterations on the device):
deterministic, the same wherever the kernels run, and NEITHER scikit-learn's nor pycave's random stream.  The same holds for `sample`.
"""
import math

import torch

from . import runtime as rt
from .metrics import gemm_f64
from .runtime import P

_ILL_DEFINED = ("Fitting the mixture model failed because some components have ill-defined empirical covariance (for instance caused by "
                "singleton or collapsed samples). Try to decrease the number of components, increase reg_covar, or scale the input data.")


def _own(v, **f):
    """a contiguous device copy of an array-like or tensor (the *_init arguments stay the caller's)"""
    return (v.detach() if torch.is_tensor(v) else torch.tensor(v)).to(**f).contiguous().clone()


# ---- kernel calls ------------------------------------------------------------------------------------------------------------------
def potrf_(a, info):
    """a [K, d, d] fp64 (rows may be pitched): lower Cholesky factors in place, lower triangle only; info [K] int32 on the device."""
    K, d, _ = a.shape
    rt.lib().cdf_potrf_f64(P(a), a.stride(1), a.stride(0), d, K, P(info), rt.stream(a))
    return a


def trtri_lower(l, out=None):
    """-> (l^-1)^T per matrix, upper triangular with a zeroed lower triangle."""
    K, d, _ = l.shape
    if out is None:
        out = torch.empty((K, d, d), device=l.device, dtype=torch.float64)
    rt.lib().cdf_trtri_lower_f64(P(l), l.stride(1), l.stride(0), P(out), out.stride(1), out.stride(0), d, K, rt.stream(l))
    return out


def tril_copy(a, transpose=False, out=None):
    K, d, _ = a.shape
    if out is None:
        out = torch.empty((K, d, d), device=a.device, dtype=torch.float64)
    rt.lib().cdf_tril_copy_f64(P(a), a.stride(1), a.stride(0), P(out), out.stride(1), out.stride(0), d, K, int(transpose), rt.stream(a))
    return out


def logdet_diag(m, out=None):
    K, d, _ = m.shape
    if out is None:
        out = torch.empty(K, device=m.device, dtype=torch.float64)
    rt.lib().cdf_logdet_diag_f64(P(m), m.stride(1), m.stride(0), d, K, P(out), rt.stream(m))
    return out


def center_scale(x, mean, z, zt=None, resp=None, nk=None):
    """z = s (x - mean) with s_i = sqrt(resp_i / nk) (nk a one-element device tensor) or 1; zt (optional) receives z^T.  x fp32 or fp64."""
    n, d = x.shape
    assert x.dtype in (torch.float32, torch.float64) and x.stride(1) == 1
    rt.lib().cdf_gmm_center_scale_f64(P(x), int(x.dtype == torch.float64), x.stride(0), n, d, P(mean), P(resp), P(nk), P(z), z.stride(0),
                                      P(zt), 0 if zt is None else zt.stride(0), rt.stream(x))
    return z


def rowsumsq(y, out):
    n, d = y.shape
    rt.lib().cdf_rowsumsq_f64(P(y), y.stride(0), n, d, P(out), rt.stream(y))
    return out


def resp_partial(n, K, device):
    return torch.empty(max(1, rt.lib().cdf_gmm_resp_blocks(n)) * (K + 1), device=device, dtype=torch.float64)


def responsibilities(maha, logdet, logw, d, resp, nk, lse_sum, partial, hard=False):
    K, n = maha.shape
    rt.lib().cdf_gmm_resp_f64(P(maha), maha.stride(0), P(logdet), P(logw), n, d, K, int(hard), P(resp), resp.stride(0), P(nk), P(lse_sum),
                              P(partial), rt.stream(maha))


class _Work:
    """The buffers one fit reuses: nothing of size n d or K d^2 is allocated inside an iteration (the M-step overwrites the covariances,
    factors and precisions in place once the E-step has read them; the fitted model keeps them)."""

    def __init__(self, n, d, K, device):
        f = dict(device=device, dtype=torch.float64)
        self.z, self.zt, self.y = torch.empty(n, d, **f), torch.empty(d, n, **f), torch.empty(n, d, **f)
        self.maha, self.resp = torch.empty(K, n, **f), torch.empty(K, n, **f)
        self.nk, self.logdet = torch.empty(K, **f), torch.empty(K, **f)
        self.partial = resp_partial(n, K, device)
        self.n = torch.full((), float(n), **f)
        self.cov, self.chol, self.pt = (torch.empty(K, d, d, **f) for _ in range(3))          # covariances, their factors, (factor^-1)^T
        # the iteration's one host read: [sum of the log-likelihoods (8 bytes) | K info words]
        self.host = torch.zeros(8 + 4 * K, device=device, dtype=torch.uint8)
        self.lse_sum, self.info = self.host[:8].view(torch.float64), self.host[8:].view(torch.int32)


class GaussianMixture:
    """pycave's `GaussianMixture` as the reference constructs and calls it (`num_components`, `trainer_params`, `covariance_type`,
    `convergence_tolerance`, `batch_size`, `covariance_regularization`; `.fit(tensor)`, `.sample(num_datapoints)`).  `trainer_params` and
    `batch_size` are accepted and unused: the fit is full-batch on the device the data is on.  Only covariance_type='full' is built."""

    def __init__(self, num_components=10, trainer_params=None, covariance_type='full', convergence_tolerance=0.001, batch_size=None,
                 covariance_regularization=1e-6, *, max_iter=100, random_state=0, weights_init=None, means_init=None, precisions_init=None):
        if covariance_type != 'full':
            raise ValueError(f"colddiff.gmm.GaussianMixture: covariance_type={covariance_type!r} is not built (only 'full', the value "
                             "the reference passes)")
        given = [v is not None for v in (weights_init, means_init, precisions_init)]
        if any(given) and not all(given):
            raise ValueError("colddiff.gmm.GaussianMixture: weights_init, means_init and precisions_init come together (all or none)")
        self.num_components, self.trainer_params, self.covariance_type = int(num_components), trainer_params, covariance_type
        self.convergence_tolerance, self.batch_size = float(convergence_tolerance), batch_size
        self.covariance_regularization, self.max_iter, self.random_state = float(covariance_regularization), int(max_iter), int(random_state)
        self.weights_init, self.means_init, self.precisions_init = weights_init, means_init, precisions_init
        self.converged_, self.n_iter_, self.lower_bound_ = False, 0, -math.inf
        self.weights_ = self.means_ = self.covariances_ = self.precisions_cholesky_ = self.cholesky_ = None
        self._sample_gen = torch.Generator().manual_seed(self.random_state)

    # -- the two steps --------------------------------------------------------------------------------------------------------------
    def _maha(self, x, means, prec_chol, w):
        """w.maha[k][i] = |(x_i - mu_k) prec_chol_k|^2"""
        for k in range(means.shape[0]):
            center_scale(x, means[k], w.z)
            gemm_f64(w.z, prec_chol[k], out=w.y)
            rowsumsq(w.y, w.maha[k])

    def _e_step(self, x, weights, means, prec_chol, w):
        self._maha(x, means, prec_chol, w)
        logdet_diag(prec_chol, w.logdet)
        responsibilities(w.maha, w.logdet, torch.log(weights), x.shape[1], w.resp, w.nk, w.lse_sum, w.partial)

    def _m_step(self, x, xd, w, reg):
        """weights, means, covariances, their factors and precisions_cholesky from w.resp / w.nk; w.info holds the factorisation's status."""
        n, d = x.shape
        K = w.nk.shape[0]
        means = gemm_f64(w.resp, xd) / w.nk[:, None]
        for k in range(K):
            center_scale(x, means[k], w.z, zt=w.zt, resp=w.resp[k], nk=w.nk[k:k + 1])
            gemm_f64(w.zt, w.z, out=w.cov[k], diag=reg)
        potrf_(w.chol.copy_(w.cov), w.info)                          # (the strict upper triangle of chol keeps the covariance's: never read)
        weights = w.nk / w.n                                         # (tensor / tensor: torch turns a division by a host scalar into a
                                                                     # multiplication by its reciprocal on the GPU, one rounding more than the CPU's)
        return weights / weights.sum(), means, w.cov, w.chol, trtri_lower(w.chol, out=w.pt)

    def _raise_if_ill_defined(self, info):
        if any(int(v) != 0 for v in info):
            raise ValueError(_ILL_DEFINED)

    # -- initialisation --------------------------------------------------------------------------------------------------------------
    def _kmeans(self, x, xd, w):
        """Hard responsibilities in w.resp / w.nk: k-means++ seeding on the host generator, Lloyd iterations on the device."""
        n, d = x.shape
        K = self.num_components
        g = torch.Generator().manual_seed(self.random_state)
        dist = torch.empty(n, device=x.device, dtype=torch.float64)
        first = int(torch.randint(n, (1,), generator=g))
        centres = [xd[first]]
        closest = None
        for _ in range(1, K):
            center_scale(x, centres[-1], w.z)
            rowsumsq(w.z, dist)
            closest = dist.clone() if closest is None else torch.minimum(closest, dist)
            p = closest.cpu()
            pick = int(torch.multinomial(p / p.sum(), 1, generator=g)) if float(p.sum()) > 0 else int(torch.randint(n, (1,), generator=g))
            centres.append(xd[pick])
        centres = torch.stack(centres).contiguous()
        prev = None
        for _ in range(100):
            for k in range(K):
                center_scale(x, centres[k], w.z)
                rowsumsq(w.z, w.maha[k])
            responsibilities(w.maha, None, None, d, w.resp, w.nk, w.lse_sum, w.partial, hard=True)
            labels = w.resp.argmax(0)
            if prev is not None and torch.equal(labels, prev):
                break
            prev = labels
            centres = (gemm_f64(w.resp, xd) / w.nk[:, None]).contiguous()
        return labels

    # -- fit --------------------------------------------------------------------------------------------------------------------------
    def fit(self, data):
        x = rt.check(torch.as_tensor(data).detach())
        if x.dtype not in (torch.float32, torch.float64):
            x = x.float()
        assert x.dim() == 2, "GaussianMixture.fit takes [rows, features]"
        x = x.contiguous()
        n, d = x.shape
        K, reg = self.num_components, self.covariance_regularization
        if n < K:
            raise ValueError(f"GaussianMixture.fit: {n} rows for {K} components")
        xd = x if x.dtype == torch.float64 else x.double()        # the fp64 operand of the mean GEMM
        w = _Work(n, d, K, x.device)
        self.converged_, self.n_iter_, self.lower_bound_ = False, 0, -math.inf
        f = dict(device=x.device, dtype=torch.float64)
        if self.weights_init is not None:
            weights, means, prec = (_own(v, **f) for v in (self.weights_init, self.means_init, self.precisions_init))
            assert weights.shape == (K,) and means.shape == (K, d) and prec.shape == (K, d, d)
            potrf_(prec, w.info)                                   # scikit-learn: precisions_cholesky_ = cholesky(precisions_init, lower=True)
            prec_chol = tril_copy(prec)
            self._raise_if_ill_defined(w.info.cpu())
            cov = chol = None
        else:
            self._kmeans(x, xd, w)
            weights, means, cov, chol, prec_chol = self._m_step(x, xd, w, reg)
            self._raise_if_ill_defined(w.info.cpu())
        lower_bound = -math.inf
        for it in range(1, self.max_iter + 1):
            prev = lower_bound
            self._e_step(x, weights, means, prec_chol, w)
            weights, means, cov, chol, prec_chol = self._m_step(x, xd, w, reg)
            host = w.host.cpu()                                     # the iteration's one host read
            self._raise_if_ill_defined(host[8:].view(torch.int32))
            lower_bound = float(host[:8].view(torch.float64)) / n
            self.n_iter_ = it
            if abs(lower_bound - prev) < self.convergence_tolerance:
                self.converged_ = True
                break
        if cov is None:                                             # max_iter = 0 with given parameters: no covariances to report
            raise ValueError("GaussianMixture.fit: max_iter = 0 is the k-means initialisation alone; with *_init it must be at least 1")
        self.weights_, self.means_, self.covariances_, self.cholesky_, self.precisions_cholesky_ = weights, means, cov, chol, prec_chol
        self.lower_bound_ = lower_bound
        return self

    # -- sampling ---------------------------------------------------------------------------------------------------------------------
    def sample(self, num_datapoints, return_labels=False):
        """x = mu_k + z L_k^T with z ~ N(0, I) in fp64 on the device; rows grouped by component in ascending order (as scikit-learn returns
        them); the counts per component are one multinomial draw on the CPU generator seeded with `random_state`.  -> float32 [n, D] on the
        device (and the int64 labels with return_labels)."""
        if self.means_ is None:
            raise RuntimeError("GaussianMixture.sample: fit first")
        n = int(num_datapoints)
        K, d = self.means_.shape
        dev = self.means_.device
        draws = torch.multinomial(self.weights_.cpu(), n, replacement=True, generator=self._sample_gen)
        counts = torch.bincount(draws, minlength=K)
        zgen = torch.Generator(device=dev).manual_seed(int(torch.randint(2 ** 31, (1,), generator=self._sample_gen)))
        z = torch.randn(n, d, device=dev, dtype=torch.float64, generator=zgen)
        out = torch.empty(n, d, device=dev, dtype=torch.float64)
        lt = torch.empty(1, d, d, device=dev, dtype=torch.float64)
        lo = 0
        for k in range(K):
            c = int(counts[k])
            if c:
                tril_copy(self.cholesky_[k:k + 1], transpose=True, out=lt)
                gemm_f64(z[lo:lo + c], lt[0], out=out[lo:lo + c])
                out[lo:lo + c] += self.means_[k]
            lo += c
        self.last_sample_counts_ = counts
        x = out.float()
        if return_labels:
            return x, torch.repeat_interleave(torch.arange(K), counts).to(dev)
        return x

    def get_params(self):
        """The keys of `colddiff.evaluate.GMM.get_params`, as host numpy arrays."""
        return {"weights": self.weights_.cpu().numpy(), "means": self.means_.cpu().numpy(), "covariances": self.covariances_.cpu().numpy()}


class SklearnStyle:
    """A fitted device mixture behind the two calls the scikit-learn-only Trainer methods make: `.sample(n_samples) -> (X, labels)`."""

    def __init__(self, model):
        self.model = model

    def sample(self, n_samples=1):
        return self.model.sample(n_samples, return_labels=True)
