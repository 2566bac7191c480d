"""The transcript of the two `fid_distance_decrease_from_manifold` sweeps: which keys they return in which order, which lines they print
in which order, and which `cdf_*` entry points they call in which order.  Simulator and MI355X.

Every metric is on in the `full` cases (`metrics.DeviceFidKidPrdc` on the 12-feature stand-in of tests/test_fid_device.py, `metrics.DeviceLpips`
on the random AlexNet of tests/lpips_ref.py); `plain` hands the sweep a plain callable (the whole-set path), `none` no fid_func at all.
Four images in batches of 3 and 1.  The numbers themselves are held by the tests of each metric; what is held here is the shape of the
sweep around them: a printed line is cut after its " is ", a bare `print` (sizes, indices) is kept whole.  The call list of a second
identical run must equal the first one's (which also packs the fresh network's weights, once: `cdf_pack_*`), and its length is a
literal: the sweep's time on the GPU is its launches.  One thing in that list is not the sweep's to decide: the square-root iteration of
a FID (`frechet_distance_device`) launches `cdf_gemm_f64` until it settles, and on the rank-3 covariances of four images the step count
hangs on the last bits of the features -- it differs between the simulator and the matrix cores, and between two processes on the matrix
cores.  Each unbroken run of `cdf_gemm_f64` therefore counts as one entry, `cdf_gemm_f64 ...`; everything else is held call by call.
"""
import contextlib
import io
import itertools

import pytest
import torch

from test_decolor_trainer import MBE, Recorder, mbe, quiet  # noqa: F401  (mbe: the fixture)

NAMES = ("blur", "deblur", "direct_deblur")
PRDC = ("precision", "recall", "density", "coverage", "f_score")
SEED = 11


def the(metric, word):
    return f"The {metric} of {word} images with original image is"


PRDC_WORD = "precision / recall / density / coverage / F-score"
HENCE = ["Hence the improvement in FID using sampling is", "Hence the improvement in FID using direct sampling is"]

# ---- the deblurring package, per name: keys rmse, ssim, fid, lpips, kid, kid_std, the five; lines RMSE, SSIM, LPIPS, FID, KID, the five;
# both "Hence" lines after the loop
DEBLUR_KEYS = {
    "full": [f"{m}_{n}" for n in NAMES for m in ("rmse", "ssim", "fid", "lpips", "kid", "kid_std") + PRDC],
    "plain": [f"{m}_{n}" for n in NAMES for m in ("rmse", "ssim", "fid")],
    "none": [f"{m}_{n}" for n in NAMES for m in ("rmse", "ssim")],
}
DEBLUR_LINES = {
    "full": [the(m, n) for n in NAMES for m in ("RMSE", "SSIM", "LPIPS", "FID", "KID", PRDC_WORD)] + HENCE,
    "plain": [the(m, n) for n in NAMES for m in ("RMSE", "SSIM", "FID")] + HENCE,
    "none": [the(m, n) for n in NAMES for m in ("RMSE", "SSIM")],
}
DEBLUR_CALLS = {"full": 705, "plain": 499, "none": 499}

# ---- decolor / snow: rmse and ssim interleaved per name, all lpips, then per name fid, kid, kid_std, the five --------------------------
WORDS = ("blurry", "deblurred", "direct deblurred")
DECOLOR_KEYS = {
    "full": ([f"{m}_{n}" for n in NAMES for m in ("rmse", "ssim")] + [f"lpips_{n}" for n in NAMES]
             + [f"{m}_{n}" for n in NAMES for m in ("fid", "kid", "kid_std") + PRDC]),
    "plain": [f"{m}_{n}" for n in NAMES for m in ("rmse", "ssim")] + [f"fid_{n}" for n in NAMES],
}
WALK = ["8", "0", "4", "torch.Size([3, 3, 32, 32])", "torch.Size([1, 3, 32, 32])"] + ["torch.Size([4, 3, 32, 32])"] * 4
DECOLOR_LINES = {
    "full": WALK + [ln for w, hence in zip(WORDS, ([], HENCE[:1], HENCE[1:]))
                    for ln in [the(m, w) for m in ("FID", "KID", PRDC_WORD, "RMSE", "SSIM", "LPIPS")] + hence],
    "plain": WALK + [ln for w, hence in zip(WORDS, ([], HENCE[:1], HENCE[1:])) for ln in [the(m, w) for m in ("FID", "RMSE", "SSIM")] + hence],
}
DECOLOR_CALLS = {"full": 685, "plain": 474}


def fid_and_lpips(mbe, how):
    from colddiff import metrics
    from test_fid_device import feat12
    from test_lpips_device import model_of
    if how == "full":
        return (metrics.DeviceFidKidPrdc(model=feat12, dims=12, batch_size=50, device=str(mbe.device), kid_subsets=3, kid_subset_size=2,
                                         kid_seed=7, prdc_k=1), metrics.DeviceLpips(model_of(mbe, SEED)))
    plain = lambda samples: float((samples[0].mean() - samples[1].mean()).abs()) + float(len(samples[0]))
    return (plain if how == "plain" else None), None


def deblur_sweep(mbe, tmp_path, how):
    """The deblurring Trainer of tests/test_lpips_device.py (32-pixel images, 8 in the folder); -> run() of images 0 ... 3."""
    from deblurring_diffusion_pytorch import GaussianDiffusion, Trainer, Unet
    from test_data import _write_images
    folder = str(tmp_path / "imgs")
    _write_images(folder, 8)
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        net = Unet(dim=8, dim_mults=(1, 2), channels=3).to(mbe.device)
        d = GaussianDiffusion(net, image_size=32, device_of_kernel=str(mbe.device), channels=3, timesteps=3, kernel_size=3, kernel_std=0.5,
                              sampling_routine="x0_step_down").to(mbe.device)
        tr = Trainer(d, folder, image_size=32, train_batch_size=4, train_num_steps=1, dataset="train", results_folder=str(tmp_path / "res"),
                     num_workers=0, device_data=True)
    fid, lpips = fid_and_lpips(mbe, how)

    def run():
        torch.manual_seed(9)
        return tr.fid_distance_decrease_from_manifold(fid_func=fid, start=-1, end=3, batch=3, **({"lpips": lpips} if lpips else {}))

    return run


def decolor_sweep(mbe, tmp_path, how):
    """The decolorization Trainer of tests/test_lpips_device.py on its 8-item ListDS; -> run() of items 1 ... 4 of the permutation walk."""
    import decolor_ref
    from test_decolor_snow_eval import numpy_seed
    from test_lpips_device import B, case
    D = decolor_ref.mine()
    torch.manual_seed(5)
    net = quiet(D.UnetConvNextBlock, dim=8, dim_mults=(1, 2)).to(mbe.device).eval()
    gd = quiet(D.GaussianDiffusion, net, image_size=(32, 32), device_of_kernel='cuda', channels=3, timesteps=3,
               sampling_routine='x0_step_down').to(mbe.device)
    tr = quiet(D.Trainer, gd, None, image_size=(32, 32), train_batch_size=2, train_num_steps=1, dataset='synthetic',
               results_folder=str(tmp_path / "res"), num_workers=0)
    imgs = case(32, 12)["x"]

    class ListDS(torch.utils.data.Dataset):
        def __len__(self):
            return 8

        def __getitem__(self, i):
            return imgs[i % B].roll(i, 2)

    tr.ds = ListDS()
    fid, lpips = fid_and_lpips(mbe, how)

    def run():
        torch.manual_seed(9)
        with numpy_seed(77):
            return tr.fid_distance_decrease_from_manifold(fid, start=0, end=4, eval_batch_size=3, **({"lpips": lpips} if lpips else {}))

    return run


def transcript(run):
    """-> (keys of the result, printed lines cut after " is ", cdf_* calls in order with each run of `cdf_gemm_f64` as one) of one run."""
    from colddiff import runtime as rt
    text = io.StringIO()
    with contextlib.redirect_stdout(text), Recorder(rt.lib()) as rec:
        out = run()
    lines = [ln.split(" is ")[0] + " is" if " is " in ln else ln for ln in text.getvalue().splitlines()]
    calls = []
    for name, run_of in itertools.groupby(rec.calls):
        calls += ["cdf_gemm_f64 ..."] if name == "cdf_gemm_f64" else list(run_of)
    return list(out), lines, calls


def check(run, keys, lines, ncalls):
    """The first run also packs the fresh network's weights (`cdf_pack_*`, once per weight); apart from those calls the second run must
    repeat it call for call, and the second run's length is the literal."""
    got_keys, got_lines, first = transcript(run)
    again_keys, again_lines, calls = transcript(run)
    print(f"{len(first)} calls, then {len(calls)}")
    assert got_keys == keys and again_keys == keys
    assert got_lines == lines and again_lines == lines
    assert not [c for c in calls if c.startswith("cdf_pack_")], "the second run packs weights again"
    assert [c for c in first if not c.startswith("cdf_pack_")] == calls, "a second identical run calls something else"
    assert len(calls) == ncalls


@pytest.mark.parametrize("how", ["full", "plain", "none"])
def test_deblurring_sweep_keys_lines_and_calls(mbe, tmp_path, how):
    check(deblur_sweep(mbe, tmp_path, how), DEBLUR_KEYS[how], DEBLUR_LINES[how], DEBLUR_CALLS[how])


@pytest.mark.parametrize("how", ["full", "plain"])
def test_decolor_sweep_keys_lines_and_calls(mbe, tmp_path, how):
    check(decolor_sweep(mbe, tmp_path, how), DECOLOR_KEYS[how], DECOLOR_LINES[how], DECOLOR_CALLS[how])
