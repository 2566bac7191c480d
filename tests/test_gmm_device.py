"""`colddiff.gmm.GaussianMixture`: the device-side EM fit and sampler against scikit-learn 1.7 on the same inputs and the same
`weights_init / means_init / precisions_init`, and through the Trainer methods that take a mixture.  Simulator and MI355X (`routed`).

Every case also runs against `np_em`, a numpy restatement of the three scikit-learn functions the class restates
(`_estimate_gaussian_parameters`, `_compute_precision_cholesky`, `_estimate_log_gaussian_prob`) and of its fit loop, so that the
comparison still runs where scikit-learn is absent; where it is there, the restatement itself is checked against it.

Inputs (`make_case`), all from numpy.random.RandomState(seed) in this order: centres randn(K, D) sep; per label a mixing matrix
(0.3 randn(D, D) + I, or randn(D, r) for the rank-r case); randn(N, D) (or (N, r)) latent rows; row n = centre + mixing[label] latent_n
with label = n % K; rows rounded through float32.  Initial means: the mean of the first five rows of each label; initial precisions:
identity; initial weights: label frequencies.

Tolerances are 8 x the larger of (a) the device-vs-scikit-learn difference measured on the simulator and on an MI355X and (b) scikit-learn's
own difference between a fit and the same fit on permuted rows -- one order of magnitude for the summation order of two correct fp64 EMs.
MEASURED holds those figures per case: (device vs scikit-learn on the simulator, on the MI355X, scikit-learn permuted rows) for the means
(absolute), the covariances (relative to their largest entry), the weights and the lower bound; profiles/gmm_device.md has the same table.
A measured 0 would make the tolerance 0; the floor is 8 ulp of the quantity's magnitude (one ulp being the least two different fp64
results can differ by).
"""
import functools
import os

import numpy as np
import pytest
import torch

from colddiff import gmm as G

#        name: (seed, N, D, K, sep, reg, rank or None)
CASES = {"a": (1, 600, 3, 3, 6.0, 1e-6, None),
         "b": (2, 500, 48, 4, 3.0, 1e-4, None),
         "c": (3, 40, 130, 2, 3.0, 1e-6, 5),
         "d": (4, 300, 65, 3, 3.0, 1e-6, None),
         "overlap": (11, 600, 3, 3, 1.0, 1e-6, None)}
# scikit-learn's iteration counts on these inputs (all converge; no component under weight 0.25); the device class must take the same
# number.  'overlap' (sep 1.0, seed picked on the CPU) is the case that needs at least 10.
SK_ITERS = {"a": 4, "b": 3, "c": 3, "d": 3, "overlap": 11}

# quantity -> case -> (simulator vs scikit-learn, MI355X vs scikit-learn, scikit-learn on permuted rows)
MEASURED = {
    "means": {"a": (1.78e-15, 1.78e-15, 7.11e-15), "b": (0.0, 0.0, 0.0), "c": (0.0, 0.0, 0.0), "d": (0.0, 0.0, 0.0),
              "overlap": (3.55e-15, 2.66e-15, 2.22e-15)},
    "covariances": {"a": (5.56e-16, 5.56e-16, 4.44e-16), "b": (6.95e-16, 6.95e-16, 3.97e-16), "c": (4.27e-16, 4.27e-16, 3.21e-16),
                    "d": (5.87e-16, 5.87e-16, 5.87e-16), "overlap": (1.02e-15, 1.02e-15, 1.52e-15)},
    "weights": {"a": (5.55e-17, 5.55e-17, 1.11e-16), "b": (0.0, 0.0, 0.0), "c": (0.0, 0.0, 0.0), "d": (0.0, 5.55e-17, 0.0),
                "overlap": (4.44e-16, 4.44e-16, 4.44e-16)},
    "lower_bound": {"a": (0.0, 0.0, 0.0), "b": (1.56e-13, 1.56e-13, 6.54e-13), "c": (1.58e-8, 1.58e-8, 6.55e-9), "d": (0.0, 0.0, 0.0),
                    "overlap": (0.0, 0.0, 8.88e-16)},
}
EPS = float(np.finfo(np.float64).eps)


@pytest.fixture
def routed(be):
    """The Python layer (colddiff.gmm) on the backend of `be`: the simulator build for 'emu'."""
    from colddiff import runtime
    from emu_util import install_emu
    if be.kind == "emu":
        install_emu()
    else:
        runtime._lib_override = None
    yield be
    runtime._lib_override = None


@functools.lru_cache(maxsize=None)
def make_case(name):
    seed, N, D, K, sep, reg, rank = CASES[name]
    r = np.random.RandomState(seed)
    centres = r.randn(K, D) * sep
    labels = np.arange(N) % K
    if rank is None:
        mix = [0.3 * r.randn(D, D) + np.eye(D) for _ in range(K)]
        lat = r.randn(N, D)
    else:
        mix = [r.randn(D, rank) for _ in range(K)]
        lat = r.randn(N, rank)
    X = np.stack([centres[labels[n]] + mix[labels[n]] @ lat[n] for n in range(N)]).astype(np.float32)
    Xd = X.astype(np.float64)
    means0 = np.stack([Xd[labels == k][:5].mean(0) for k in range(K)])
    prec0 = np.stack([np.eye(D) for _ in range(K)])
    w0 = np.bincount(labels, minlength=K) / N
    for a in (X, means0, prec0, w0, labels):
        a.setflags(write=False)
    return dict(X=X, w0=w0, means0=means0, prec0=prec0, reg=reg, K=K, labels=labels)


# ---- the numpy restatement -----------------------------------------------------------------------------------------------------------
def np_parameters(X, resp, reg):
    """_estimate_gaussian_parameters, 'full'"""
    nk = resp.sum(0) + 10 * EPS
    means = resp.T @ X / nk[:, None]
    K, D = means.shape
    cov = np.empty((K, D, D))
    for k in range(K):
        diff = X - means[k]
        cov[k] = (resp[:, k] * diff.T) @ diff / nk[k]
        cov[k].flat[::D + 1] += reg
    return nk, means, cov


def np_precision_cholesky(cov):
    """_compute_precision_cholesky, 'full': (L^-1)^T per component; a failing factorisation is scikit-learn's ValueError"""
    out = np.empty_like(cov)
    for k, c in enumerate(cov):
        try:
            L = np.linalg.cholesky(c)
        except np.linalg.LinAlgError:
            raise ValueError("ill-defined empirical covariance")
        out[k] = np.linalg.solve(L, np.eye(c.shape[0])).T          # (scikit-learn: solve_triangular(L, I, lower=True).T)
    return out


def np_log_prob(X, means, prec_chol):
    """_estimate_log_gaussian_prob, 'full'"""
    N, D = X.shape
    K = means.shape[0]
    log_det = np.array([np.log(np.diag(p)).sum() for p in prec_chol])
    lp = np.empty((N, K))
    for k in range(K):
        y = X @ prec_chol[k] - means[k] @ prec_chol[k]
        lp[:, k] = (y * y).sum(1)
    return -0.5 * (D * np.log(2 * np.pi) + lp) + log_det


def np_em(X, w0, means0, prec0, reg, tol=1e-3, max_iter=100):
    X = X.astype(np.float64)
    weights, means = w0.copy(), means0.copy()
    prec_chol = np.stack([np.linalg.cholesky(p) for p in prec0])
    lb, converged, n_iter = -np.inf, False, 0
    for n_iter in range(1, max_iter + 1):
        prev = lb
        wlp = np_log_prob(X, means, prec_chol) + np.log(weights)
        mx = wlp.max(1)
        lse = mx + np.log(np.exp(wlp - mx[:, None]).sum(1))
        lb = lse.mean()
        nk, means, cov = np_parameters(X, np.exp(wlp - lse[:, None]), reg)
        weights = nk / X.shape[0]
        weights = weights / weights.sum()
        prec_chol = np_precision_cholesky(cov)
        if abs(lb - prev) < tol:
            converged = True
            break
    return dict(weights=weights, means=means, covariances=cov, lower_bound=lb, n_iter=n_iter, converged=converged)


def sk_em(X, w0, means0, prec0, reg, tol=1e-3):
    from sklearn.mixture import GaussianMixture
    m = GaussianMixture(n_components=len(w0), tol=tol, reg_covar=reg, weights_init=w0, means_init=means0, precisions_init=prec0,
                        random_state=0).fit(X.astype(np.float64))
    return dict(weights=m.weights_, means=m.means_, covariances=m.covariances_, lower_bound=m.lower_bound_, n_iter=m.n_iter_,
                converged=m.converged_)


@functools.lru_cache(maxsize=None)
def reference(name, which):
    c = make_case(name)
    return (sk_em if which == "sklearn" else np_em)(c["X"], c["w0"], c["means0"], c["prec0"], c["reg"])


def device_fit(be, name, **kw):
    c = make_case(name)
    m = G.GaussianMixture(num_components=c["K"], covariance_regularization=c["reg"], weights_init=c["w0"], means_init=c["means0"],
                          precisions_init=c["prec0"], **kw)
    return m.fit(be.to(torch.from_numpy(c["X"].copy())))


def as_dict(m):
    return dict(weights=m.weights_.cpu().numpy(), means=m.means_.cpu().numpy(), covariances=m.covariances_.cpu().numpy(),
                lower_bound=m.lower_bound_, n_iter=m.n_iter_, converged=m.converged_)


def differences(got, ref):
    """-> {quantity: (difference, magnitude of the quantity)}: means / weights / lower bound absolute, covariances relative to the largest entry"""
    cmax = np.abs(ref["covariances"]).max()
    return {"means": (np.abs(got["means"] - ref["means"]).max(), np.abs(ref["means"]).max()),
            "covariances": (np.abs(got["covariances"] - ref["covariances"]).max() / cmax, 1.0),
            "weights": (np.abs(got["weights"] - ref["weights"]).max(), 1.0),
            "lower_bound": (abs(got["lower_bound"] - ref["lower_bound"]), abs(ref["lower_bound"]))}


def check_against(be, name, ref, tag):
    got = as_dict(device_fit(be, name))
    assert ref["converged"] and ref["n_iter"] == SK_ITERS[name], (ref["converged"], ref["n_iter"])
    assert got["converged"] and got["n_iter"] == ref["n_iter"], (got["converged"], got["n_iter"], ref["n_iter"])
    for q, (diff, mag) in differences(got, ref).items():
        tol = max(8 * max(MEASURED[q][name]), 8 * EPS * mag)
        print(f"gmm [{be.kind}] case {name} vs {tag}: {q} differ by {diff:.3g} (tolerance {tol:.3g})")
        assert diff <= tol, (q, diff, tol)


@pytest.mark.parametrize("name", list(CASES))
def test_fit_agrees_with_scikit_learn(routed, name):
    pytest.importorskip("sklearn")
    check_against(routed, name, reference(name, "sklearn"), "scikit-learn")


@pytest.mark.parametrize("name", list(CASES))
def test_fit_agrees_with_the_numpy_restatement(routed, name):
    check_against(routed, name, reference(name, "numpy"), "numpy restatement")


@pytest.mark.parametrize("name", list(CASES))
def test_the_numpy_restatement_is_scikit_learns_arithmetic(name):
    pytest.importorskip("sklearn")
    sk, mine = reference(name, "sklearn"), reference(name, "numpy")
    assert sk["n_iter"] == mine["n_iter"] and sk["converged"] and mine["converged"]
    assert min(sk["weights"]) >= (0.25 if name in "abcd" else 0.05)
    for q, (diff, mag) in differences(mine, sk).items():
        assert diff <= max(8 * MEASURED[q][name][2], 64 * EPS * mag), (q, diff)


def test_singular_covariance_raises_and_the_object_stays_usable(routed):
    c = make_case("c")
    m = G.GaussianMixture(num_components=c["K"], covariance_regularization=0.0, weights_init=c["w0"], means_init=c["means0"],
                          precisions_init=c["prec0"])
    x = routed.to(torch.from_numpy(c["X"].copy()))
    with pytest.raises(ValueError, match="ill-defined empirical covariance.*reg_covar"):
        m.fit(x)
    m.covariance_regularization = c["reg"]
    assert m.fit(x) is m and m.converged_ and m.n_iter_ == SK_ITERS["c"]


def test_constructor_is_pycaves_and_refuses_what_is_not_built():
    import inspect
    names = list(inspect.signature(G.GaussianMixture.__init__).parameters)
    assert names[1:7] == ["num_components", "trainer_params", "covariance_type", "convergence_tolerance", "batch_size", "covariance_regularization"]
    p = inspect.signature(G.GaussianMixture.__init__).parameters
    assert [p[n].default for n in names[1:7]] == [10, None, "full", 0.001, None, 1e-6]
    assert all(p[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("max_iter", "random_state", "weights_init", "means_init", "precisions_init"))
    assert (p["max_iter"].default, p["random_state"].default) == (100, 0)
    for ct in ("diag", "spherical", "tied"):
        with pytest.raises(ValueError, match=ct):
            G.GaussianMixture(covariance_type=ct)
    m = G.GaussianMixture(num_components=2, trainer_params=dict(gpus=1), covariance_type="full", convergence_tolerance=0.001, batch_size=100)
    assert m.num_components == 2


# ---- k-means initialisation -----------------------------------------------------------------------------------------------------------
def kmeans_fit(be, name="a"):
    c = make_case(name)
    return G.GaussianMixture(num_components=c["K"], covariance_regularization=c["reg"], random_state=3).fit(be.to(torch.from_numpy(c["X"].copy())))


def test_kmeans_initialisation_is_deterministic_and_recovers_separated_clusters(routed):
    c = make_case("a")
    m1, m2 = kmeans_fit(routed), kmeans_fit(routed)
    for a, b in ((m1.weights_, m2.weights_), (m1.means_, m2.means_), (m1.covariances_, m2.covariances_), (m1.precisions_cholesky_, m2.precisions_cholesky_)):
        assert torch.equal(a, b)
    assert m1.converged_ and m1.lower_bound_ == m2.lower_bound_
    # the label partition: every fitted component's mean is the mean of one label's rows (to the EM's own accuracy), each label once
    X = c["X"].astype(np.float64)
    label_means = np.stack([X[c["labels"] == k].mean(0) for k in range(c["K"])])
    dist = np.abs(m1.means_.cpu().numpy()[:, None, :] - label_means[None]).max(2)
    assert sorted(dist.argmin(1).tolist()) == list(range(c["K"])) and dist.min(1).max() < 0.05
    assert np.abs(np.sort(m1.weights_.cpu().numpy()) - 1 / 3).max() < 1e-3
    assert set(m1.get_params()) == {"weights", "means", "covariances"}


@pytest.mark.gpu
def test_kmeans_initialisation_is_bit_identical_on_simulator_and_hardware():
    """The same build, the same random_state: the seeding is a CPU generator and the Lloyd steps and the parameters taken from the hard
    assignment involve only IEEE operations (products and sums in the kernels' fixed order, division, square root) -- no exp / log, where
    the host's and the device's libm may differ in the last place -- so the initial parameters (max_iter=0) must be `==`."""
    from colddiff import runtime
    from conftest import Backend
    from emu_util import install_emu, uninstall_emu
    c = make_case("a")
    fits = []
    for kind in ("hip", "emu"):
        if kind == "emu":
            install_emu()
        else:
            runtime._lib_override = None
        try:
            be = Backend(kind)
            fits.append(G.GaussianMixture(num_components=3, random_state=3, max_iter=0).fit(be.to(torch.from_numpy(c["X"].copy()))))
        finally:
            uninstall_emu()
    a, b = fits
    assert a.n_iter_ == 0 and a.means_.is_cuda and not b.means_.is_cuda
    for u, v in ((a.weights_, b.weights_), (a.means_, b.means_), (a.covariances_, b.covariances_), (a.precisions_cholesky_, b.precisions_cholesky_)):
        assert torch.equal(u.cpu(), v)


# ---- sampling -----------------------------------------------------------------------------------------------------------------------
def test_sample_counts_moments_dtype_and_grouping(routed):
    m = device_fit(routed, "a", random_state=5)
    n, K = 20000, 3
    x, labels = m.sample(n, return_labels=True)
    assert x.dtype == torch.float32 and x.device == routed.device and x.shape == (n, 3)
    want = torch.bincount(torch.multinomial(m.weights_.cpu(), n, replacement=True, generator=torch.Generator().manual_seed(5)), minlength=K)
    counts = torch.bincount(labels.cpu(), minlength=K)
    assert torch.equal(counts, want) and torch.equal(labels.cpu(), torch.sort(labels.cpu()).values)      # grouped by component, ascending
    x, lo = x.double().cpu().numpy(), 0
    means, cov = m.means_.cpu().numpy(), m.covariances_.cpu().numpy()
    for k in range(K):
        nk = int(counts[k])
        xs = x[lo:lo + nk]
        lo += nk
        # 5 standard errors: the sample mean of nk draws has variance cov_jj / nk; an entry of the sample covariance of Gaussian rows has
        # variance (cov_ii cov_jj + cov_ij^2) / (nk - 1).  (The float32 rounding of the output, 6e-8 relative, is far below both.)
        se_mean = np.sqrt(np.diag(cov[k]) / nk)
        assert (np.abs(xs.mean(0) - means[k]) <= 5 * se_mean).all()
        se_cov = np.sqrt((np.outer(np.diag(cov[k]), np.diag(cov[k])) + cov[k] ** 2) / (nk - 1))
        assert (np.abs(np.cov(xs, rowvar=False) - cov[k]) <= 5 * se_cov).all()
    y = m.sample(num_datapoints=7)
    assert y.shape == (7, 3) and y.dtype == torch.float32


# ---- wiring -------------------------------------------------------------------------------------------------------------------------
def quiet(fn, *a, **k):
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def image_folder(tmp_path, S, count):
    from PIL import Image
    folder = tmp_path / "imgs"
    folder.mkdir()
    g = torch.Generator().manual_seed(5)
    for i in range(count):
        Image.fromarray((torch.rand(S, S, 3, generator=g) * 255).to(torch.uint8).numpy()).save(folder / f"{i}.png")
    return folder


def test_trainer_methods_take_the_device_mixture(routed, tmp_path, monkeypatch):
    """The tiny Trainers of tests/test_modules.py's CaptureGMM tests: `torch_gmm=colddiff.gmm.GaussianMixture` in a method that takes
    `torch_gmm`, `device_gmm=True` in a scikit-learn-only one; the files are the scikit-learn route's, the sampler is fed device tensors,
    and `device_gmm=False` still goes to scikit-learn."""
    import deblurring_diffusion_pytorch as DB
    import denoising_diffusion_pytorch as DN
    from colddiff import evaluate
    S = 16
    folder = image_folder(tmp_path, S, 8)
    torch.manual_seed(0)
    fits = []
    real_fit = G.GaussianMixture.fit
    monkeypatch.setattr(G.GaussianMixture, "fit", lambda self, data: (fits.append((data.device, tuple(data.shape))), real_fit(self, data))[1])

    # -- a torch_gmm method (deblurring Trainer): D = 3 channel means
    net = quiet(DB.Unet, dim=8, dim_mults=(1, 2), channels=3).to(routed.device)
    d = DB.GaussianDiffusion(net, image_size=S, device_of_kernel='cuda' if routed.kind == 'hip' else 'cpu', channels=3, timesteps=3,
                             kernel_std=0.5, kernel_size=3, blur_routine='Incremental', sampling_routine='x0_step_down').to(routed.device)
    tr = quiet(DB.Trainer, d, str(folder), image_size=S, train_batch_size=2, results_folder=str(tmp_path / "deb"), device_data=False, num_workers=0)
    saved, seeds = [], []
    tr._save = lambda img, name, nrow=6: saved.append(os.path.relpath(name, tmp_path))
    gen = tr.ema_core.gen_sample
    tr.ema_core.gen_sample = lambda **kw: (seeds.append(kw["img"]), gen(**kw))[1]
    assert quiet(tr.sample_as_a_mean_blur_torch_gmm_ablation, G.GaussianMixture, clusters=2, num_samples=4, bs=2) == 4
    assert fits and fits[-1] == (routed.device, (8, 3))
    assert all(s.device == routed.device and s.dtype == torch.float32 and s.shape == (2, 3, S, S) and torch.isfinite(s).all() for s in seeds)
    assert sorted(saved) == sorted(f"deb_{f}/sample-x0-{i}.png" for f in ("out", "xt", "dir_recons") for i in range(4))

    # -- a scikit-learn-only method (denoising Trainer): D = 4 * 4 * 3 resampled vectors
    net = quiet(DN.Unet, dim=8, dim_mults=(1, 2), channels=3).to(routed.device)
    d = DN.GaussianDiffusion(net, image_size=S, channels=3, timesteps=3).to(routed.device)
    tr = quiet(DN.Trainer, d, str(folder), image_size=S, train_batch_size=2, results_folder=str(tmp_path / "den"), device_data=False, num_workers=0)
    names, fed = {}, []
    all_sample = tr.ema_core.all_sample
    tr.ema_core.all_sample = lambda **kw: (fed.append(kw["img"]), all_sample(**kw))[1]
    for flag in (False, True):
        del saved[:]
        tr._save = lambda img, name, nrow=6: saved.append(os.path.relpath(name, tmp_path))
        nfit = len(fits)
        X0, Xt = quiet(tr.sample_as_a_vector_gmm, start=-1, end=7, siz=4, clusters=2, num_samples=2, device_gmm=flag)
        assert X0[-1].shape == (2, 3, S, S) and torch.isfinite(X0[-1]).all()
        assert fed[-1].device == routed.device and fed[-1].dtype == torch.float32 and fed[-1].shape == (2, 3, S, S)
        assert (len(fits) - nfit) == int(flag) and (not flag or fits[-1] == (routed.device, (8, 48)))
        names[flag] = list(saved)
    assert names[True] == names[False] and names[True][0] == "den/og--1-7-4-2-vec.png"
    del saved[:]
    assert quiet(tr.sample_as_a_vector_gmm_and_save, start=-1, end=7, siz=4, clusters=2, n_sample=4, num_samples=2, device_gmm=True) == 4
    assert saved == [f"den_4_2/sample-x0-{i}.png" for i in range(4)]

    # -- device_gmm=False (the default) calls scikit-learn: its import target is replaced and must be the one that is used
    import sklearn.mixture
    calls = []

    class Spy(sklearn.mixture.GaussianMixture):
        def fit(self, X, y=None):
            calls.append(X.shape)
            return super().fit(X, y)

    monkeypatch.setattr(sklearn.mixture, "GaussianMixture", Spy)
    nfit = len(fits)
    quiet(tr.sample_as_a_vector_gmm, start=-1, end=7, siz=4, clusters=2, num_samples=2)
    assert calls == [(8, 48)] and len(fits) == nfit
    quiet(tr.sample_as_a_vector_gmm, start=-1, end=7, siz=4, clusters=2, num_samples=2, device_gmm=True)
    assert calls == [(8, 48)] and len(fits) == nfit + 1
    assert evaluate.GMM is not G.GaussianMixture                      # the default of every torch_gmm=None stays the host class
