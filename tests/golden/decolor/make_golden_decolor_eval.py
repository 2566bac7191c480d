"""Generator of tests/golden/decolor/decolor_eval.pt: what the UNMODIFIED evaluation methods of the reference Trainer
(decolor-diffusion/diffusion/diffusion.py:764-959, 1000-1145) computed on a reference Trainer object whose dataset is a fixed in-memory
list -- the pattern of `evaluation_cases()` in tests/golden/make_golden.py.  Needs the reference tree; the tests read only the .pt file.

    python tests/golden/decolor/make_golden_decolor_eval.py

Cases: RGB and `to_lab=True` (the latter through the kornia functions RESTATED in decolor_ref.py, like every Lab fixture), both with
`sampling_routine='x0_step_down'`, 16 x 16 images, T = 3, the dim-8 (1, 2) network of decolor_net.pt.  Per case
  * fid_distance_decrease_from_manifold(fid_func, start=0, end=20) on 24 images after `np.random.seed(NP_SEED)`: the four sets handed to
    fid_func, the three RMSE values, the three SSIM values (pytorch_msssim is not installed: `ssim_msssim` of make_golden.py stands in);
  * test_from_data('t', s_times=2) on one batch of 2: every tensor `utils.save_image` received, by file name;
  * (first case only, for size) paper_invert_section_images() with batches of 18, i.e. two windows: the four sets of its first round --
    stored once as rows 0...9, of which window j is rows j...j+8 (upstream's windows start at j, not 9 j).
The images are not stored: `eval_images()` redraws them from a seed.

Harness notes (none of it touches the methods under record): `utils.save_image` captures; `utils.make_grid` is torchvision's grid
algorithm restated (torchvision is not installed); `add_title` (cv2 text) is a no-op on the object; cv2's imread / copyMakeBorder /
hconcat / imwrite and imageio's imread / mimsave are no-ops (the montage and the GIFs are not recorded); `torch.cuda.FloatTensor` is
torch.FloatTensor; `.cuda()` is the identity (ref_shim).  Only data goes into the file.
"""
import contextlib
import io
import itertools
import math
import os
import pathlib
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.dirname(HERE)
TESTS = os.path.dirname(GOLDEN)
REPO = os.path.dirname(TESTS)
for p in (TESTS, REPO, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import decolor_ref as R  # noqa: E402
from make_golden_decolor import images  # noqa: E402

SEED, NP_SEED = 123457, 20261
THREADS = 1
S, T, N_IMAGES, START, END = 16, 3, 24, 0, 20
TFD_BATCH, TFD_TIMES, PAPER_BATCH = 2, 2, 18
SAMPLING = 'x0_step_down'
NAMES = ("blur", "deblur", "direct_deblur")


def eval_images():
    return images(N_IMAGES, 31, size=S)


def make_grid_tv(tensor, nrow=8, padding=2, pad_value=0.0):
    """torchvision.utils.make_grid for [B,C,H,W] / [C,H,W] float tensors (normalize=False), restated from its documentation."""
    if tensor.dim() == 3:
        tensor = tensor.unsqueeze(0)
    if tensor.size(0) == 1:
        return tensor.squeeze(0)
    nmaps = tensor.size(0)
    xmaps = min(nrow, nmaps)
    ymaps = int(math.ceil(float(nmaps) / xmaps))
    height, width = int(tensor.size(2) + padding), int(tensor.size(3) + padding)
    grid = tensor.new_full((tensor.size(1), height * ymaps + padding, width * xmaps + padding), pad_value)
    k = 0
    for y in range(ymaps):
        for x in range(xmaps):
            if k >= nmaps:
                break
            grid.narrow(1, y * height + padding, height - padding).narrow(2, x * width + padding, width - padding).copy_(tensor[k])
            k = k + 1
    return grid


def _ssim_restated():
    sys.path.insert(0, GOLDEN)
    try:
        from make_golden import ssim_msssim
    finally:
        sys.path.remove(GOLDEN)
    return ssim_msssim


def run_case(ref_mods, gd, to_lab, with_paper, shared):
    """The three methods on a reference Trainer object around the reference diffusion `gd`.  `shared`: tensors already stored by an
    earlier case of the file (an equal tensor is stored once)."""
    mod = ref_mods["diffusion.diffusion"]
    imgs = eval_images()

    class ListDS(torch.utils.data.Dataset):
        def __len__(self):
            return imgs.shape[0]

        def __getitem__(self, i):
            return imgs[i]

    post = mod.rgb2lab if to_lab else (lambda x: x)
    tr = object.__new__(mod.Trainer)
    tr.ds, tr.image_size, tr.to_lab, tr.post_process_func = ListDS(), (S, S), to_lab, post
    tr.ema_model, tr.num_timesteps = gd, T
    tr.results_folder = pathlib.Path(tempfile.mkdtemp())
    tr.add_title = lambda *a, **k: None
    saved, ssim_calls, fid_calls = [], [], []
    ssim_msssim = _ssim_restated()

    def ssim_capture(X, Y, **kw):
        v = ssim_msssim(X, Y, **kw)
        ssim_calls.append(v.clone())
        return v

    def fid_func(samples):
        fid_calls.append([z.clone() for z in samples])
        return float(len(fid_calls))

    nothing = lambda *a, **k: None
    cv2, imageio, msssim = sys.modules["cv2"], mod.imageio, sys.modules["pytorch_msssim"]
    undo = []

    def patch(obj, name, value):
        undo.append((obj, name, getattr(obj, name, patch)))
        setattr(obj, name, value)

    patch(mod.utils, "save_image", lambda t, path, **kw: saved.append((os.path.basename(str(path)), t.detach().clone())))
    patch(mod.utils, "make_grid", make_grid_tv)
    patch(mod.transforms, "ToPILImage", lambda: None)
    patch(torch.cuda, "FloatTensor", torch.FloatTensor)
    patch(msssim, "ssim", ssim_capture)
    for name in ("imread", "mimsave"):
        patch(imageio, name, nothing)
    for name in ("imread", "copyMakeBorder", "hconcat", "imwrite", "BORDER_CONSTANT"):
        patch(cv2, name, nothing)
    np_state = np.random.get_state()
    out = {"to_lab": to_lab}
    keep = lambda t: shared.setdefault((tuple(t.shape), t.double().sum().item(), t.double().abs().sum().item()), t)
    try:
        with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
            np.random.seed(NP_SEED)
            tr.fid_distance_decrease_from_manifold(fid_func, start=START, end=END)
            orig = fid_calls[0][0]
            assert len(fid_calls) == 3 and all(torch.equal(c[0], orig) for c in fid_calls) and orig.shape == (END - START, 3, S, S)
            sets = dict(orig=keep(orig), blur=fid_calls[0][1], deblur=fid_calls[1][1], direct_deblur=fid_calls[2][1])
            out["sweep"] = dict(start=START, end=END, np_seed=NP_SEED, sets=sets,
                                rmse={k: torch.sqrt(torch.mean((orig - sets[k]) ** 2)) for k in NAMES}, ssim=dict(zip(NAMES, ssim_calls)))
            # -- test_from_data: the first batch of the loader ---------------------------------------------------------------------
            saved.clear()
            tr.batch_size = TFD_BATCH
            tr.data_loader = [imgs[:TFD_BATCH].clone()]
            tr.test_from_data('t', s_times=TFD_TIMES)
            assert len(saved) == 1 + 2 * TFD_TIMES
            out["test_from_data"] = dict(batch=TFD_BATCH, s_times=TFD_TIMES, saved={name: t for name, t in saved})
            # -- paper_invert_section_images: 20 rounds on the same batch; the first round's two windows ------------------------------
            if with_paper:
                saved.clear()
                tr.batch_size = PAPER_BATCH
                tr.dl = itertools.cycle([post(imgs[:PAPER_BATCH].clone())])
                tr.paper_invert_section_images()
                assert len(saved) == 20 * 2 * 4
                win = {name: t for name, t in saved[:8]}
                rows = {}
                for part in ("original", "direct_recons", "sampling_recons", "blurry_image"):
                    w0, w1 = win[f"{part}_0.png"], win[f"{part}_1.png"]
                    assert torch.equal(w0[1:], w1[:8])                   # (windows j and j + 1 overlap in eight rows)
                    rows[part] = torch.cat((w0, w1[8:]), dim=0)
                out["paper"] = dict(batch=PAPER_BATCH, windows=2, rows=rows)
    finally:
        np.random.set_state(np_state)
        for obj, name, old in reversed(undo):
            if old is patch:
                delattr(obj, name)
            else:
                setattr(obj, name, old)
    return out


def _gd(ref, sd, **kw):
    m = ref._cdf_ref_modules
    torch.manual_seed(SEED)
    with contextlib.redirect_stdout(io.StringIO()):
        net = m["diffusion.model.unet_convnext"].UnetConvNextBlock(dim=8, dim_mults=(1, 2))
        net.load_state_dict(sd, strict=True)
        return m["diffusion.diffusion"].GaussianDiffusion(net.eval(), image_size=(S, S), device_of_kernel='cuda', channels=3, timesteps=T,
                                                          sampling_routine=SAMPLING, **kw)


def generate():
    ref = R.load()
    sd = torch.load(os.path.join(HERE, "decolor_net.pt"), weights_only=False)["state_dict"]
    threads, state = torch.get_num_threads(), torch.get_rng_state()
    torch.set_num_threads(THREADS)
    try:
        shared = {}
        return {"restated_kornia": True,
                "rgb": run_case(ref._cdf_ref_modules, _gd(ref, sd), False, True, shared),
                "lab": run_case(ref._cdf_ref_modules, _gd(ref, sd, to_lab=True), True, False, shared)}
    finally:
        torch.set_num_threads(threads)
        torch.set_rng_state(state)


def main():
    assert R.available(), "needs the reference tree"
    path = os.path.join(HERE, "decolor_eval.pt")
    torch.save(generate(), path)
    print(os.path.basename(path), os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
