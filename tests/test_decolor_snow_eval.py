"""The evaluation path of the decolorization and snowification Trainers (the reference's `test.py` calls): `metrics.PairStats` against the
whole-set `metrics.rmse` / `metrics.ssim`, the sampler's ends-only mode against the full `all_sample`, and `test_from_data`,
`test_with_mixup`, `test_from_random`, `paper_invert_section_images` and `fid_distance_decrease_from_manifold` against what the
UNMODIFIED reference methods computed (tests/golden/decolor/decolor_eval.pt, tests/golden/snow/snow_eval.pt; the generators beside them
say how).  Simulator (CPU tensors) and MI355X.  Bounds: the sets 2e-4, RMSE 2e-5, SSIM 1e-4 -- those tests/test_eval.py holds the same
sweep of the older packages to; the originals 1e-6.
"""
import contextlib
import io
import itertools
import os
import sys

import numpy as np
import pytest
import torch

import decolor_ref
import snow_ref
from test_decolor_trainer import MBE, mbe, quiet  # noqa: F401  (mbe: the fixture)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ("blur", "deblur", "direct_deblur")
CASES = [("decolor", "rgb"), ("decolor", "lab"), ("snow", "plain"), ("snow", "fix")]

try:
    import scipy.ndimage  # noqa: F401
    HAVE_SCIPY = True
except ImportError:
    HAVE_SCIPY = False


def _generator(pkg):
    folder = os.path.join(GOLDEN, pkg)
    sys.path.insert(0, folder)
    try:
        return __import__(f"make_golden_{pkg}_eval")
    finally:
        sys.path.remove(folder)


_fixtures = {}


def fixture(pkg):
    if pkg not in _fixtures:
        _fixtures[pkg] = torch.load(os.path.join(GOLDEN, pkg, f"{pkg}_eval.pt"), weights_only=False)
    return _fixtures[pkg]


def err(a, b):
    return (a.detach().cpu() - b).abs().max().item()


def diffusion_of(mbe, pkg, key):
    """This repository's diffusion object of a fixture case: the generator's network, sizes and seed."""
    if pkg == "snow" and not HAVE_SCIPY:
        pytest.skip("the host part of Snow needs scipy")
    M = _generator("decolor")
    D = decolor_ref.mine() if pkg == "decolor" else snow_ref.mine()
    sd = torch.load(os.path.join(GOLDEN, "decolor", "decolor_net.pt"), weights_only=False)["state_dict"]
    net = quiet(D.UnetConvNextBlock, dim=8, dim_mults=(1, 2))
    net.load_state_dict(sd, strict=True)
    net = net.to(mbe.device).eval()
    kw = dict(to_lab=key == "lab") if pkg == "decolor" else dict(forward_process_type='Snow', snow_level=1, fix_brightness=key == "fix",
                                                                 results_folder=None)
    torch.manual_seed(M.SEED)                                  # (Snow: the planes the reference's constructor drew after this seed)
    gd = quiet(D.GaussianDiffusion, net, image_size=(M.S, M.S), device_of_kernel='cuda', channels=3, timesteps=M.T,
               sampling_routine=M.SAMPLING, **kw).to(mbe.device)
    return D, gd, M


def trainer_of(mbe, pkg, key, tmp_path):
    D, gd, M = diffusion_of(mbe, pkg, key)
    imgs = M.eval_images()
    tr = quiet(D.Trainer, gd, None, image_size=(M.S, M.S), train_batch_size=M.TFD_BATCH, train_num_steps=1, dataset='synthetic',
               results_folder=str(tmp_path / "res"), to_lab=key == "lab", num_workers=0)

    class ListDS(torch.utils.data.Dataset):
        def __len__(self):
            return imgs.shape[0]

        def __getitem__(self, i):
            return imgs[i]

    tr.ds = ListDS()
    return tr, imgs, M


def feed(tr, mbe, imgs, batch):
    """The loader yields imgs[:batch] for ever (the Trainer's own post-processing -- rgb2lab with to_lab -- still applies)."""
    tr.batch_size = batch
    tr.dl = itertools.cycle([mbe.to(imgs[:batch].clone())])


def capture(tr):
    got = {}
    write = tr._write_image

    def spy(tensor, path, nrow=8):
        got[os.path.basename(str(path))] = tensor.detach().cpu().clone()
        return write(tensor, path, nrow=nrow)

    tr._write_image = spy
    return got


@contextlib.contextmanager
def numpy_seed(seed):
    state = np.random.get_state()
    np.random.seed(seed)
    try:
        yield
    finally:
        np.random.set_state(state)


# ---------------------------------------------------------------------------------------------------------------------------------------
# metrics.eval_pairs / PairStats
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_pair_stats_equal_the_whole_set_metrics(mbe):
    """Two batches of different size (5 and 3 images of 3 x 43 x 45: two tiles along each axis, the second a strip) through `PairStats`
    against `metrics.rmse` / `metrics.ssim(data_range=1, size_average=True)` of the concatenated, shifted sets.  Bounds: 2e-5 (RMSE) and
    1e-4 (SSIM), absolute, as tests/test_eval.py:188-189 holds the same quantities.
    Measured on the simulator: |RMSE difference| <= 5.1e-9, |SSIM difference| <= 1.8e-8 (summation order only)."""
    from colddiff import metrics
    g = torch.Generator().manual_seed(77)
    x = torch.randint(0, 256, (8, 3, 43, 45), generator=g).float() / 255 * 2 - 1
    cands = [(x + s * torch.randn(x.shape, generator=g)).clamp(-1, 1) for s in (0.6, 0.05, 0.2)]
    dx, dc = mbe.to(x), [mbe.to(c) for c in cands]
    sse, ss = metrics.eval_pairs(dx[:5], [c[:5] for c in dc])
    assert sse.dtype == ss.dtype == torch.float64 and sse.shape == ss.shape == (3,) and sse.device.type == mbe.device.type
    stats = metrics.PairStats(NAMES)
    stats.add(dx[:5], [c[:5] for c in dc])
    stats.add(dx[5:], [c[5:] for c in dc])
    res = stats.result()
    assert sorted(res) == sorted(f"{m}_{k}" for m in ("rmse", "ssim") for k in NAMES)
    sx = (dx + 1) * 0.5
    for k, c in zip(NAMES, dc):
        sc = (c + 1) * 0.5
        d_rmse = abs(res[f"rmse_{k}"] - float(metrics.rmse(sx, sc)))
        d_ssim = abs(res[f"ssim_{k}"] - float(metrics.ssim(sx, sc, data_range=1, size_average=True)))
        print(f"PairStats [{mbe.kind}] {k}: |rmse difference| {d_rmse:.3g}, |ssim difference| {d_ssim:.3g}")
        assert d_rmse <= 2e-5 and d_ssim <= 1e-4, (k, d_rmse, d_ssim)
    # shift=False on sets already in [0, 1] is the same computation
    plain = metrics.PairStats(NAMES, shift=False)
    plain.add(sx, [(c + 1) * 0.5 for c in dc])
    assert all(abs(plain.result()[k] - res[k]) <= 1e-6 for k in res)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the sampler's ends-only mode
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pkg,key", [("decolor", "rgb"), ("decolor", "lab"), ("snow", "plain")])
def test_ends_only_is_bit_equal_to_the_full_all_sample(mbe, pkg, key, monkeypatch):
    from colddiff import decolor as CD
    D, gd, M = diffusion_of(mbe, pkg, key)
    x = mbe.to(M.eval_images()[:3].clone())
    calls = []
    real = CD.lab2rgb
    monkeypatch.setattr(CD, "lab2rgb", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    for times in (None, 1):
        n = M.T if times is None else times
        calls.clear()
        X_0s, X_ts, init, fwd = gd.all_sample(batch_size=3, img=x.clone(), times=times)
        full_calls = len(calls)
        assert len(X_0s) == len(X_ts) == n and init is None and fwd == [] and all(not v.is_cuda for v in X_0s + X_ts)
        calls.clear()
        ends = gd.all_sample(batch_size=3, img=x.clone(), times=times, ends_only=True)
        assert len(ends) == 3 and all(e.device.type == mbe.device.type for e in ends)
        assert torch.equal(ends[0].cpu(), X_ts[0]) and torch.equal(ends[1].cpu(), X_0s[0]) and torch.equal(ends[2].cpu(), X_0s[-1])
        if key == "lab":
            assert full_calls == 2 * n and len(calls) == min(3, 2 * n) and (len(calls) < full_calls or n == 1)
        else:
            assert full_calls == len(calls) == 0
    with pytest.raises(ValueError):
        gd.all_sample(batch_size=3, img=x.clone(), times=0, ends_only=True)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the Trainer methods against the reference's
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pkg,key", CASES)
def test_metric_sweep_against_the_reference(mbe, pkg, key, tmp_path):
    tr, imgs, M = trainer_of(mbe, pkg, key, tmp_path)
    sw = fixture(pkg)[key]["sweep"]
    calls = []

    def fid_func(samples):
        assert all(z.device.type == mbe.device.type for z in samples)             # the sets stay on the device
        calls.append([z.detach().cpu().clone() for z in samples])
        return float(len(calls))

    with numpy_seed(sw["np_seed"]):
        res = quiet(tr.fid_distance_decrease_from_manifold, fid_func, start=sw["start"], end=sw["end"])
    assert len(calls) == 3 and calls[0][0].shape == sw["sets"]["orig"].shape == (sw["end"] - sw["start"], 3, M.S, M.S)
    for i, k in enumerate(NAMES):
        e_orig, e_set = err(calls[i][0], sw["sets"]["orig"]), err(calls[i][1], sw["sets"][k])
        d_rmse, d_ssim = abs(res[f"rmse_{k}"] - float(sw["rmse"][k])), abs(res[f"ssim_{k}"] - float(sw["ssim"][k]))
        print(f"sweep {pkg}/{key} [{mbe.kind}] {k}: originals {e_orig:.3g}, set {e_set:.3g}, rmse {d_rmse:.3g}, ssim {d_ssim:.3g}")
        assert e_orig <= 1e-6, k                                                   # ... so the walk follows np.random.seed
        assert e_set <= 2e-4, k
        assert d_rmse <= 2e-5, (k, res[f"rmse_{k}"], float(sw["rmse"][k]))
        assert d_ssim <= 1e-4, (k, res[f"ssim_{k}"], float(sw["ssim"][k]))
        assert res[f"fid_{k}"] == float(i + 1)
    assert sorted(res) == sorted(f"{m}_{k}" for m in ("rmse", "ssim", "fid") for k in NAMES)
    if (pkg, key) == ("decolor", "rgb"):                       # without a fid_func: the accumulator alone, no FID, the same numbers
        with numpy_seed(sw["np_seed"]):
            res2 = quiet(tr.fid_distance_decrease_from_manifold, None, start=sw["start"], end=sw["end"])
        assert res2 == {k: v for k, v in res.items() if not k.startswith("fid_")}


def test_metric_sweep_prints_the_reference_lines(mbe, tmp_path):
    tr, imgs, M = trainer_of(mbe, "decolor", "rgb", tmp_path)
    out = io.StringIO()
    with numpy_seed(3), contextlib.redirect_stdout(out):
        res = tr.fid_distance_decrease_from_manifold(lambda samples: 2.0 if len(samples[0]) else 0.0, start=0, end=2, eval_batch_size=1)
    text = out.getvalue()
    for word in ("blurry", "deblurred", "direct deblurred"):
        for m in ("FID", "RMSE", "SSIM"):
            assert f"The {m} of {word} images with original image is " in text
    assert "Hence the improvement in FID using sampling is 0.0" in text and "Hence the improvement in FID using direct sampling is 0.0" in text
    assert res["fid_blur"] == 2.0 and text.index("The FID of blurry") < text.index("The RMSE of blurry") < text.index("The SSIM of blurry")


@pytest.mark.parametrize("pkg,key", CASES)
def test_from_data_against_the_reference(mbe, pkg, key, tmp_path):
    tr, imgs, M = trainer_of(mbe, pkg, key, tmp_path)
    c = fixture(pkg)[key]["test_from_data"]
    feed(tr, mbe, imgs, c["batch"])
    got = capture(tr)
    assert quiet(tr.test_from_data, 't', s_times=c["s_times"]) is None
    want_names = ["og-t.png"] + [f"sample-{i}-t-{tag}.png" for i in range(c["s_times"]) for tag in ("x0", "xt")]
    assert sorted(got) == sorted(c["saved"]) == sorted(want_names)
    res = tmp_path / "res"
    for name in want_names + ["Gif-t-x0.gif", "Gif-t-xt.gif"]:
        assert os.path.exists(res / name), name
    worst = 0.0
    for name, want in c["saved"].items():
        assert got[name].shape == want.shape, name
        worst = max(worst, err(got[name], want))
        assert err(got[name], want) <= 2e-4, (name, err(got[name], want))
    print(f"test_from_data {pkg}/{key} [{mbe.kind}]: grids within {worst:.3g} of the reference's")
    from PIL import Image
    gif = Image.open(res / "Gif-t-x0.gif")
    assert gif.n_frames == c["s_times"] and gif.size == (got["sample-0-t-x0.png"].shape[2], got["sample-0-t-x0.png"].shape[1])
    assert tr.gif_len == c["s_times"] and torch.equal(tr.shift_data_range(torch.tensor([-1.0, 0.0, 1.0])), torch.tensor([0.0, 0.5, 1.0]))


@pytest.mark.parametrize("pkg", ["decolor", "snow"])
def test_with_mixup_and_from_random_write_their_files(mbe, pkg, tmp_path):
    tr, imgs, M = trainer_of(mbe, pkg, "rgb" if pkg == "decolor" else "plain", tmp_path)
    tr.batch_size = 2
    tr.dl = itertools.cycle([mbe.to(imgs[:2].clone()), mbe.to(imgs[2:4].clone())])
    got = capture(tr)
    quiet(tr.test_with_mixup, 'mix')
    res = tmp_path / "res"
    names = ["og1-mix.png", "og2-mix.png", "og-mix.png", "Gif-mix-x0.gif", "Gif-mix-xt.gif"] + \
            [f"sample-{i}-mix-{tag}.png" for i in range(M.T) for tag in ("x0", "xt")]
    assert all(os.path.exists(res / n) for n in names)
    assert err(got["og-mix.png"], (got["og1-mix.png"] + got["og2-mix.png"]) / 2) <= 1e-6
    quiet(tr.test_from_random, 'rnd')
    names = ["og-rnd.png", "Gif-rnd-x0.gif", "Gif-rnd-xt.gif"] + [f"sample-{i}-rnd-{tag}.png" for i in range(M.T) for tag in ("x0", "xt")]
    assert all(os.path.exists(res / n) for n in names)
    assert got["sample-0-rnd-x0.png"].dim() == 3 and torch.isfinite(got["sample-0-rnd-x0.png"]).all()
    assert err(got["og-rnd.png"][:, 2:18, 2:18], (imgs[0] * 0.9 + 1) * 0.5) <= 1e-6       # the batch scaled by 0.9, first cell of the grid


@pytest.mark.parametrize("pkg,key", [("decolor", "rgb"), ("snow", "plain")])
def test_paper_invert_section_images_against_the_reference(mbe, pkg, key, tmp_path):
    from PIL import Image
    tr, imgs, M = trainer_of(mbe, pkg, key, tmp_path)
    c = fixture(pkg)[key]["paper"]
    feed(tr, mbe, imgs, c["batch"])
    got = capture(tr)
    quiet(tr.paper_invert_section_images, rounds=1)
    parts = ("blurry_image", "direct_recons", "sampling_recons", "original")      # the montage's order, left to right
    assert sorted(got) == sorted(f"{p}_{j}.png" for p in parts for j in range(c["windows"]))
    res = tmp_path / "res"
    worst = 0.0
    for j in range(c["windows"]):
        for p in parts:
            e = err(got[f"{p}_{j}.png"], c["rows"][p][j: j + 9])                   # (window j is rows j ... j + 8)
            worst = max(worst, e)
            assert e <= 2e-4, (p, j, e)
        tiles = [np.asarray(Image.open(res / f"{p}_{j}.png").convert("RGB")) for p in parts]
        h, w = tiles[0].shape[:2]
        assert (h, w) == (3 * 18 + 2, 3 * 18 + 2)                                  # a 3-column grid of nine 16 x 16 images
        montage = np.asarray(Image.open(res / f"all_{j}.png").convert("RGB"))
        assert montage.shape == (h + 20, 4 * (w + 20), 3)
        inner = np.zeros(montage.shape[:2], dtype=bool)
        for k, tile in enumerate(tiles):
            x0 = k * (w + 20) + 10
            assert np.array_equal(montage[10: 10 + h, x0: x0 + w], tile), (j, parts[k])
            inner[10: 10 + h, x0: x0 + w] = True
        assert (montage[~inner] == 0).all()
    print(f"paper_invert_section_images {pkg}/{key} [{mbe.kind}]: windows within {worst:.3g} of the reference's")
    assert not os.path.exists(res / f"all_{c['windows']}.png")


# ---------------------------------------------------------------------------------------------------------------------------------------
# live reference (where its tree exists; never on the GPU machine)
# ---------------------------------------------------------------------------------------------------------------------------------------
def _same(path, got, want):
    if isinstance(want, dict):
        assert isinstance(got, dict) and sorted(got) == sorted(want), path
        for k in want:
            _same(path + "/" + str(k), got[k], want[k])
    elif isinstance(want, torch.Tensor):
        assert got.dtype == want.dtype and torch.equal(got, want), path
    else:
        assert got == want, path


@pytest.mark.skipif(not decolor_ref.available(), reason="needs the reference tree")
@pytest.mark.parametrize("pkg", ["decolor", "snow"])
def test_generators_reproduce_the_committed_fixtures(pkg):
    if pkg == "snow" and not HAVE_SCIPY:
        pytest.skip("the host part of Snow needs scipy")
    _same(pkg, quiet(_generator(pkg).generate), fixture(pkg))
    assert os.path.getsize(os.path.join(GOLDEN, pkg, f"{pkg}_eval.pt")) < 1000000


@pytest.mark.skipif(not decolor_ref.available(), reason="needs the reference tree")
@pytest.mark.parametrize("pkg", ["decolor", "snow"])
def test_built_methods_follow_the_prefix_rule(pkg):
    from test_boundary import _accepts_every_reference_call, _shown
    sys.path.insert(0, os.path.join(GOLDEN, "decolor"))
    try:
        from make_golden_decolor import signature_params
    finally:
        sys.path.remove(os.path.join(GOLDEN, "decolor"))
    R = decolor_ref if pkg == "decolor" else snow_ref
    theirs = R.load()._cdf_ref_modules["diffusion.diffusion"].Trainer
    ours = R.mine().Trainer
    built = ("save_gif", "save_og_test", "shift_data_range", "test_from_data", "test_with_mixup", "test_from_random",
             "paper_invert_section_images", "fid_distance_decrease_from_manifold")
    assert not set(built) & set(ours.NOT_BUILT)
    for name in built:
        rp, mp = signature_params(getattr(theirs, name)), signature_params(getattr(ours, name))
        assert _accepts_every_reference_call(rp, mp), (name, _shown(rp), _shown(mp))
    for name in ours.NOT_BUILT:
        assert hasattr(theirs, name), name                                          # what stays closed is the reference's figure / dead code
    assert signature_params(R.mine().GaussianDiffusion.all_sample)[:len(signature_params(R.load()._cdf_ref_modules["diffusion.diffusion"].GaussianDiffusion.all_sample))] \
        == signature_params(R.load()._cdf_ref_modules["diffusion.diffusion"].GaussianDiffusion.all_sample)
