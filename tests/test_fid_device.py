"""FID on the device: `metrics.FidStats`, `frechet_distance_device`, `DeviceFid` and the two `fid_distance_decrease_from_manifold` sweeps
fed by it.  Simulator and MI355X.

References.  Primary: the eigenvalue route in fp64 on the host -- Tr sqrt(C1 C2) = sum sqrt(max(eig(S1 C2 S1), 0)), S1 = sqrt(C1) through
`eigh` (the closed form of tests/test_eval.py::test_frechet_distance_and_fid_plumbing).  Secondary: `calculate_frechet_distance` (scipy
sqrtm), which must itself be finite, real and within the tolerance of the eigenvalue route on the same statistics (checked up to
d = 768; at d = 2048 one sqrtm is ~10 s of host time and it is not used as a reference there).
Tolerances, as the issue sets them: |Tr sqrt_device - Tr sqrt_eig| <= 1e-6 Tr sqrt_eig, |fid_device - fid_eig| <= 2e-6 Tr sqrt_eig,
|fid(A, A)| <= 2e-6 Tr C.  (The numpy prototype's worst error was 4.6e-8; the margin is for the MFMA's summation order and the iterate at
which the stop rule fires.)  Every case prints its measured errors and step counts; profiles/fid_device.md records them.
Finding kept there: with the noise-floor threshold at 1e-6 the d = 768 case measured 1.5e-6 / 3.0e-6 on the MI355X -- the rule fired on a
plateau of slowly growing eigenvalues, five steps early; the threshold is 1e-9 now (metrics.NS_FLOOR) and the tolerances are as they were.
"""
import contextlib
import io
import os
import tempfile

import numpy as np
import pytest
import torch

from test_decolor_trainer import MBE, mbe, quiet  # noqa: F401  (mbe: the fixture)

EMU_CASES = [(40, 100, 90), (64, 48, 48)]                         # (d, N1, N2)
GPU_CASES = [(192, 48, 48), (768, 64, 64), (2048, 300, 260)]
SCIPY_MAX_D = 768


def features(d, n, seed, shift):
    """max(G W + b, 0) in fp32 with a decaying column scale: W = randn(d, d) * arange(1, d + 1)^-0.8."""
    rng = np.random.RandomState(seed)
    W = rng.randn(d, d) * np.arange(1, d + 1) ** -0.8
    b = rng.randn(d) * 0.3 + shift
    return torch.from_numpy(np.maximum(rng.randn(n, d) @ W + b, 0).astype(np.float32))


def eig_route(mu1, C1, mu2, C2):
    w, v = np.linalg.eigh(C1)
    r1 = (v * np.sqrt(np.clip(w, 0, None))) @ v.T
    M = r1 @ C2 @ r1
    tr = np.sqrt(np.clip(np.linalg.eigvalsh((M + M.T) * 0.5), 0, None)).sum()
    return ((mu1 - mu2) ** 2).sum() + np.trace(C1) + np.trace(C2) - 2 * tr, tr


_cases = {}


def case(mbe, d, n1, n2):
    """The two FidStats of a case (fed in batches of 50) and the host references of THEIR statistics; made once per backend and case."""
    from colddiff import metrics
    key = (mbe.kind, d, n1, n2)
    if key not in _cases:
        stats = []
        for n, seed, shift in ((n1, 10 * d + 1, 0.1), (n2, 10 * d + 2, 0.25)):
            f = mbe.to(features(d, n, seed, shift))
            st = metrics.FidStats(d, mbe.device)
            for s in range(0, n, 50):
                st.add(f[s:s + 50])
            stats.append(st)
        (m1, c1), (m2, c2) = stats[0].result(), stats[1].result()
        fid_eig, tr_eig = eig_route(m1, c1, m2, c2)
        _cases[key] = (stats, (m1, c1, m2, c2), fid_eig, tr_eig)
    return _cases[key]


def check_distance(mbe, d, n1, n2):
    from colddiff import metrics
    stats, (m1, c1, m2, c2), fid_eig, tr_eig = case(mbe, d, n1, n2)
    info = {}
    fid = metrics.frechet_distance_device(stats[0], stats[1], _info=info)
    assert isinstance(fid, float) and not info["fallback"], info
    e_tr, e_fid = abs(info["tr_sqrt"] - tr_eig) / tr_eig, abs(fid - fid_eig) / tr_eig
    print(f"frechet_distance_device [{mbe.kind}] d={d} N=({n1}, {n2}): steps {info['iters']}, Tr sqrt {tr_eig:.6g}, fid {fid_eig:.6g}, "
          f"|dTr| / Tr {e_tr:.3g}, |dfid| / Tr {e_fid:.3g}")
    if d <= SCIPY_MAX_D:
        host = quiet(metrics.calculate_frechet_distance, m1, c1, m2, c2)
        e_host = abs(host - fid_eig) / tr_eig
        print(f"    calculate_frechet_distance on the same statistics: |dfid| / Tr {e_host:.3g}")
        assert np.isrealobj(host) and np.isfinite(host) and e_host <= 2e-6, "the secondary reference is itself off: fix the input"
        assert abs(fid - host) <= 4e-6 * tr_eig
    assert e_tr <= 1e-6, (info, tr_eig)
    assert e_fid <= 2e-6, (fid, fid_eig)
    # identical statistics
    same = metrics.frechet_distance_device(stats[0], stats[0], _info=info)
    print(f"    fid(A, A) = {same:.3g} ({abs(same) / np.trace(c1):.3g} of Tr C, steps {info['iters']})")
    assert not info["fallback"] and abs(same) <= 2e-6 * np.trace(c1)


@pytest.mark.parametrize("d,n1,n2", EMU_CASES)
def test_distance_against_the_eigenvalue_route(mbe, d, n1, n2):
    check_distance(mbe, d, n1, n2)


@pytest.mark.gpu
@pytest.mark.parametrize("d,n1,n2", GPU_CASES)
def test_distance_against_the_eigenvalue_route_on_the_gpu(d, n1, n2):
    from colddiff import runtime
    runtime._lib_override = None
    check_distance(MBE("hip"), d, n1, n2)


def test_a_forced_cap_returns_the_host_value_and_says_so(mbe, capsys):
    from colddiff import metrics
    stats, (m1, c1, m2, c2), fid_eig, tr_eig = case(mbe, *EMU_CASES[0])
    info = {}
    fid = metrics.frechet_distance_device(stats[0], stats[1], _max_iter=2, _info=info)
    out = capsys.readouterr().out
    assert info["fallback"] and out.count("did not settle within 2 steps") == 1 and "calculate_frechet_distance" in out
    assert fid == float(metrics.calculate_frechet_distance(m1, c1, m2, c2))


def test_stats_accept_the_extractor_output_forms_and_round_trip_through_a_file(mbe, tmp_path):
    from colddiff import metrics
    f = features(40, 30, 5, 0.2)
    a = metrics.FidStats(40, mbe.device).add(mbe.to(f))
    b = metrics.FidStats(40, mbe.device).add(mbe.to(f[:, :, None, None]))
    assert torch.equal(a.mean(), b.mean()) and torch.equal(a.cov(), b.cov())
    maps = mbe.to(torch.rand(30, 40, 2, 3))                                                # an unpooled map, in the list an extractor returns
    c, e = metrics.FidStats(40, mbe.device).add([maps]), metrics.FidStats(40, mbe.device).add(maps.mean((2, 3)))
    assert torch.equal(c.mean(), e.mean()) and torch.equal(c.cov(), e.cov())
    assert a.mean().dtype == a.cov().dtype == torch.float64 and a.cov().device.type == mbe.device.type and a.n == 30
    mu, sigma = a.result()
    assert mu.shape == (40,) and sigma.shape == (40, 40) and mu.dtype == sigma.dtype == np.float64
    path = str(tmp_path / "stats.npz")
    a.save(path)
    z = np.load(path)
    assert sorted(z.files) == ["mu", "n", "sigma"]                                         # pytorch-fid's keys + n
    back = metrics.FidStats.load(path, mbe.device)
    assert back.n == 30 and np.array_equal(back.result()[0], mu) and np.array_equal(back.result()[1], sigma)
    assert torch.equal(back.mean(), a.mean()) and torch.equal(back.cov(), a.cov())
    with pytest.raises(RuntimeError, match="frozen"):
        back.add(mbe.to(f))
    assert metrics.frechet_distance_device(back, a) == metrics.frechet_distance_device(a, a)
    with pytest.raises(AssertionError):
        metrics.FidStats(41, mbe.device).add(mbe.to(f))


# ---- DeviceFid against the host route, with a stand-in extractor ----------------------------------------------------------------------
def feat12(x):
    """12 features of a batch [B, 3, H, W] in [0, 1] (tests/test_eval.py's stand-in, widened): channel means and deviations, the
    quadrant means of channel 0, the mean of every other row, the mean horizontal step.  Image by image, so that a row does not depend on
    the batch it came in (a device reduction may split its work by the batch size): the two routes under comparison batch differently."""
    return torch.cat([_feat12(x[i:i + 1]) for i in range(x.shape[0])])


def _feat12(x):
    h, w = x.shape[2] // 2, x.shape[3] // 2
    quad = [x[:, 0, :h, :w], x[:, 0, :h, w:], x[:, 0, h:, :w], x[:, 0, h:, w:]]
    cols = [x.mean((2, 3)), x.std((2, 3)), torch.stack([q.mean((1, 2)) for q in quad], 1), x[:, :, ::2].mean((1, 2, 3))[:, None],
            (x[:, :, :, 1:] - x[:, :, :, :-1]).abs().mean((1, 2, 3))[:, None]]
    return torch.cat(cols, 1)


class Counting:
    def __init__(self, fn):
        self.fn, self.images = fn, 0

    def __call__(self, x):
        self.images += x.shape[0]
        return self.fn(x)


def fid_tolerance(fid, a, b):
    """2e-6 Tr sqrt(C1 C2), the trace by the eigenvalue route on the statistics `fid` (a DeviceFid) accumulates for the two sets."""
    (m1, c1), (m2, c2) = fid.stats(a).result(), fid.stats(b).result()
    return 2e-6 * eig_route(m1, c1, m2, c2)[1]


def test_device_fid_equals_the_host_route_with_a_stand_in_extractor(mbe):
    from colddiff import metrics
    g = torch.Generator().manual_seed(9)
    A = mbe.to(torch.rand(40, 3, 8, 8, generator=g))
    B = mbe.to(torch.rand(40, 3, 8, 8, generator=g) * 0.5 + 0.1 * torch.rand(40, 3, 1, 1, generator=g))
    fid = metrics.DeviceFid(model=feat12, dims=12, batch_size=16, device=str(mbe.device))
    got = fid(samples=[A, B])
    want = quiet(metrics.calculate_fid_given_samples, [A, B], batch_size=16, device=str(mbe.device), dims=12, model=feat12)
    tol = fid_tolerance(fid, A, B)
    print(f"DeviceFid [{mbe.kind}] stand-in extractor: device {got:.9g}, host {want:.9g}, difference {abs(got - want):.3g} (tolerance {tol:.3g})")
    assert isinstance(got, float) and abs(got - want) <= tol
    assert metrics.calculate_fid_given_samples([A, B], batch_size=16, device=str(mbe.device), dims=12, model=feat12, on_device=True) == got
    assert fid.stats(A).n == 40 and fid.new_stats().n == 0                                 # 16 + 16 + 8: the partial batch is included
    assert fid.distance(fid.stats(A), fid.stats(B)) == got
    if mbe.kind == "emu":
        with pytest.raises(FileNotFoundError, match="pt_inception-2015-12-05"):            # no weight file: an error, as the host route
            metrics.DeviceFid(device="cpu")


# ---- the two Trainer sweeps -----------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def watch_cat():
    """Records the shape of every 4-D [N, 3, H, W] concatenation along dim 0 (what keeping the image sets ends in)."""
    seen, real = [], torch.cat

    def cat(tensors, *a, **k):
        out = real(tensors, *a, **k)
        if out.dim() == 4 and out.shape[1] == 3 and (a[0] if a else k.get("dim", 0)) == 0:
            seen.append(tuple(out.shape))
        return out

    torch.cat = cat
    try:
        yield seen
    finally:
        torch.cat = real


def compare_sweeps(mbe, run, n, rmse_ssim_rel):
    """`run(fid_func)` -> result dict; the plain callable against DeviceFid on the same extractor."""
    from colddiff import metrics
    plain_model, dev_model = Counting(feat12), Counting(feat12)
    sets = []

    def plain(samples):
        sets.append([z.detach().clone() for z in samples])
        return metrics.calculate_fid_given_samples(samples, batch_size=50, device=str(mbe.device), dims=12, model=plain_model)

    with watch_cat() as cats_plain:
        want = run(plain)
    fid = metrics.DeviceFid(model=dev_model, dims=12, batch_size=50, device=str(mbe.device))
    text = io.StringIO()
    with watch_cat() as cats_dev, contextlib.redirect_stdout(text):
        got = run(fid)
    assert list(got) == list(want)
    assert plain_model.images == 6 * n and dev_model.images == 4 * n, (plain_model.images, dev_model.images)
    assert (n, 3, 16, 16) in cats_plain and not cats_dev, (cats_plain, cats_dev)
    for k in want:
        if k.startswith("fid_"):
            tol = fid_tolerance(metrics.DeviceFid(model=feat12, dims=12, device=str(mbe.device)), *sets[("blur", "deblur", "direct_deblur").index(k[4:])])
            print(f"sweep [{mbe.kind}] {k}: device {got[k]:.9g}, host {want[k]:.9g}, difference {abs(got[k] - want[k]):.3g} (tolerance {tol:.3g})")
            assert isinstance(got[k], float) and abs(got[k] - want[k]) <= tol, k
        else:
            assert abs(got[k] - want[k]) <= rmse_ssim_rel * abs(want[k]), (k, got[k], want[k])
    return text.getvalue()


def test_decolor_sweep_fed_per_batch(mbe, tmp_path):
    """DecolorTrainer.fid_distance_decrease_from_manifold (the snow Trainer inherits it) on the 20 images of the evaluation fixture, in
    batches of 16 + 4: RMSE / SSIM equal (the same PairStats either way), the three FIDs within tolerance, the extractor on 4 N instead
    of 6 N images, no [N, 3, H, W] set concatenated, the printed lines those of the plain path."""
    from test_decolor_snow_eval import numpy_seed, trainer_of
    tr, imgs, M = trainer_of(mbe, "decolor", "rgb", tmp_path)

    def run(fid_func):
        with numpy_seed(M.NP_SEED):
            if hasattr(fid_func, "new_stats"):
                return tr.fid_distance_decrease_from_manifold(fid_func, start=M.START, end=M.END)
            return quiet(tr.fid_distance_decrease_from_manifold, fid_func, start=M.START, end=M.END)

    text = compare_sweeps(mbe, run, M.END - M.START, 0.0)
    for word in ("blurry", "deblurred", "direct deblurred"):
        for m in ("FID", "RMSE", "SSIM"):
            assert f"The {m} of {word} images with original image is " in text
    assert text.count(f"torch.Size([{M.END - M.START}, 3, {M.S}, {M.S}])") == 4
    assert "Hence the improvement in FID using sampling is " in text and "Hence the improvement in FID using direct sampling is " in text


def test_eval_mixin_sweep_fed_per_batch(mbe, tmp_path):
    """EvalMixin.fid_distance_decrease_from_manifold (deblurring Trainer) on the 8-image folder of tests/test_eval.py, in batches of 4.
    The plain path computes RMSE / SSIM of the concatenated sets with fp32 reductions (cdf_loss_fwd, the fp32 sum of the SSIM tile
    partials), the fed path with PairStats' fp64 sums of the same per-tile partials: the two differ by summation order only.  Bound
    1e-5 relative: either side rounds at most once per partial it adds (8 x 3 planes x 1 tile SSIM partials, <= 24 x 42 squared-error
    partial sums of a few hundred terms), each rounding <= 2^-24 of the running sum of same-sign terms; 1e-5 = 168 x 2^-24.
    The covariances are rank 7 of 12: the rank-deficient path of the distance."""
    from deblurring_diffusion_pytorch import GaussianDiffusion, Trainer, Unet
    from test_data import _write_images
    folder = str(tmp_path / "imgs")
    _write_images(folder, 8)
    torch.manual_seed(0)
    dev = mbe.device
    with contextlib.redirect_stdout(io.StringIO()):
        net = Unet(dim=8, dim_mults=(1, 2), channels=3).to(dev)
        d = GaussianDiffusion(net, image_size=16, device_of_kernel=str(dev), channels=3, timesteps=3, kernel_size=3, kernel_std=0.5,
                              sampling_routine="x0_step_down").to(dev)
        tr = Trainer(d, folder, image_size=16, train_batch_size=4, train_num_steps=1, dataset="train", results_folder=str(tmp_path / "res"),
                     num_workers=0, device_data=True)

    def run(fid_func):
        if hasattr(fid_func, "new_stats"):
            return tr.fid_distance_decrease_from_manifold(fid_func=fid_func, start=-1, end=7, batch=4)
        return quiet(tr.fid_distance_decrease_from_manifold, fid_func=fid_func, start=-1, end=7, batch=4)

    text = compare_sweeps(mbe, run, 8, 1e-5)
    for name in ("blur", "deblur", "direct_deblur"):
        for m in ("FID", "RMSE", "SSIM"):
            assert f"The {m} of {name} images with original image is " in text
    assert "Hence the improvement in FID using sampling is " in text and "Hence the improvement in FID using direct sampling is " in text


@pytest.mark.gpu
def test_device_fid_end_to_end_with_inception_on_the_gpu():
    """DeviceFid builds the extractor itself (weights from $COLDDIFF_FID_WEIGHTS: oracle.inception_ref's randomised network) at
    dims = 192 on 48 images of 32 x 32, as tests/test_inception.py::test_fid_end_to_end_on_the_gpu; the value equals the Frechet distance
    of the restatement's features within that test's tolerance (the network's bf16x3 arithmetic dominates)."""
    from colddiff import metrics, runtime
    from oracle import inception_ref as R
    runtime._lib_override = None
    ref = R.randomise(R.FidInception3(), seed=11)
    torch.manual_seed(4)
    a, b = torch.rand(48, 3, 32, 32), (torch.rand(48, 3, 32, 32) * 0.8 + 0.1)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "pt_inception.pth")
        torch.save(ref.state_dict(), path)
        os.environ["COLDDIFF_FID_WEIGHTS"] = path
        try:
            fid = metrics.DeviceFid(dims=192, batch_size=16, device="cuda:0")(samples=[a, b])
        finally:
            del os.environ["COLDDIFF_FID_WEIGHTS"]
    with torch.no_grad():
        fa = R.features(ref, a, output_blocks=(1,))[0].mean((2, 3)).double().numpy()
        fb = R.features(ref, b, output_blocks=(1,))[0].mean((2, 3)).double().numpy()
    want = metrics.calculate_frechet_distance(fa.mean(0), np.cov(fa, rowvar=False), fb.mean(0), np.cov(fb, rowvar=False))
    print("DeviceFid", fid, "restatement", want)
    assert abs(fid - want) <= 2e-2 * abs(want) + 1e-3
