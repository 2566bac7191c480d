"""TEST INFRASTRUCTURE for the snowification package: the live reference loader and the plain-torch restatements the tests compare with.

* `load()` imports the UNMODIFIED reference package `snowification/diffusion` (usable where the reference tree exists) under the stubs
  of oracle/ref_shim.py and tests/decolor_ref.py (kornia's grayscale restated there), and adds the 1-D
  `torchgeometry.image.get_gaussian_kernel` to the torchgeometry stub: `ref_shim.gaussian_1d`, the same restatement of torchgeometry
  0.1.2 the 2-D stub is built from.  The reference pins no torchgeometry version, so the motion-blur taps are an UNPINNED boundary of the
  same kind as the 2-D Gaussian.  scipy (`scipy.ndimage.zoom`) is the real library.
* `mine()` imports this repository's drop-in `diffusion` package of `cold-diffusion-models_amd/snowification` and leaves sys.modules as
  it found it: the decolorization drop-in has the same name, and a test that runs afterwards must get its own.
* `degrade_t` / `layers_t` / `state_t`: sequential fp32 restatements on CPU tensors, for the machines without the reference tree.
"""
import contextlib
import importlib
import os
import sys

import torch

import decolor_ref
from decolor_ref import q_sample_counts                # noqa: F401  (the q_sample index arithmetic is the decolorization package's)
from oracle import ref_shim

REF_FOLDER = os.path.join(ref_shim.REFERENCE_ROOT, "snowification")
PKG = "diffusion"
MINE_ROOT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cold-diffusion-models_amd")
MINE_FOLDER = os.path.join(MINE_ROOT, "snowification")


def available():
    return os.path.isdir(os.path.join(REF_FOLDER, PKG))


def get_gaussian_kernel(ksize, sigma):
    """torchgeometry.image.get_gaussian_kernel (0.1.2), restated: UNPINNED boundary."""
    return ref_shim.gaussian_1d(ksize, sigma)


def _is_pkg(name):
    return name == PKG or name.startswith(PKG + ".")


@contextlib.contextmanager
def _fresh_package(folder, keep=None):
    """sys.modules without any `diffusion*` entry and `folder` first on sys.path; afterwards both are as found.  `keep`: receives the
    modules imported inside."""
    saved = {n: m for n, m in sys.modules.items() if _is_pkg(n)}
    for n in saved:
        del sys.modules[n]
    sys.path.insert(0, folder)
    try:
        yield
    finally:
        sys.path.remove(folder)
        made = {n: m for n, m in sys.modules.items() if _is_pkg(n)}
        for n in made:
            del sys.modules[n]
        sys.modules.update(saved)
        if keep is not None:
            keep.update(made)


def load():
    """The reference `diffusion` package of snowification/, sys.modules left as found."""
    assert available(), "reference tree not present"
    ref_shim.install_stubs()
    decolor_ref.install_kornia_stubs()
    sys.modules["torchgeometry.image"].get_gaussian_kernel = get_gaussian_kernel
    tv = sys.modules["torchvision.transforms"]
    for n in ("ColorJitter", "RandomResizedCrop", "RandomApply"):
        if not hasattr(tv, n):
            setattr(tv, n, ref_shim._Anything)
    for n in ("CIFAR10", "CelebA", "Flowers102"):
        if not hasattr(sys.modules["torchvision.datasets"], n):
            setattr(sys.modules["torchvision.datasets"], n, ref_shim._Anything)
    mods = {}
    with _fresh_package(REF_FOLDER, mods):
        mod = importlib.import_module(PKG)
        importlib.import_module(PKG + ".model.unet_convnext")
        importlib.import_module(PKG + ".forward_process_impl")
    mod._cdf_ref_modules = mods
    return mod


_mine = None


def mine():
    """This repository's drop-in `diffusion` package of the snowification folder (its modules in `._cdf_modules`)."""
    global _mine
    if _mine is None:
        if MINE_ROOT not in sys.path:
            sys.path.insert(0, MINE_ROOT)
        mods = {}
        with _fresh_package(MINE_FOLDER, mods):
            mod = importlib.import_module(PKG)
            importlib.import_module(PKG + ".model.get_model")
        assert "snowification" in mod.__file__, mod.__file__
        mod._cdf_modules = mods
        _mine = mod
    return _mine


@contextlib.contextmanager
def mine_importable():
    """`import diffusion` resolves to the snowification drop-in inside the block (for the reference's own import lines)."""
    mod = mine()
    saved = {n: m for n, m in sys.modules.items() if _is_pkg(n)}
    for n in saved:
        del sys.modules[n]
    sys.modules.update(mod._cdf_modules)
    try:
        yield mod
    finally:
        for n in [n for n in sys.modules if _is_pkg(n)]:
            del sys.modules[n]
        sys.modules.update(saved)


# ---- plain-torch restatements (CPU) ----------------------------------------------------------------------------------------------------
def degrade_t(og, plane, br, i, fix=False):
    """D(og, i): `plane` is step i's snow plane, [1|B,1,H,W] (one channel, broadcast over the three); br the list of python doubles.
    float32(br) and float32(1.0 - br) multiply the fp32 images, as the reference's tensor arithmetic rounds them."""
    og_r = (og + 1.) / 2.
    r, g, b = og_r[:, 0:1], og_r[:, 1:2], og_r[:, 2:3]
    gray = (0.299 * r + 0.587 * g + 0.114 * b) * 1.5 + 0.5
    gray = torch.maximum(og_r, gray)
    if fix:
        scaled = og_r
    else:
        scaled = torch.tensor(br[i], dtype=torch.float32) * og_r + torch.tensor(1.0 - br[i], dtype=torch.float32) * gray
    rot = torch.flip(plane, dims=[-2, -1])
    return torch.clip(scaled + plane + rot, 0.0, 1.0) * 2. - 1.


def layers_t(base, thres, taps, vertical):
    """base [L,H,W], thres [T], taps [T,k] (fp32 tensors), vertical [T,L] -> [T,L,H,W]: threshold (fp32 compare), clip, one-row blur with
    zero padding, the k taps accumulated one after the other in ascending order of the source pixel."""
    L, H, W = base.shape
    T, k = taps.shape
    half = k // 2
    out = torch.zeros((T, L, H, W), dtype=torch.float32)
    for t in range(T):
        v = torch.where(base < thres[t], torch.zeros_like(base), base).clamp(0.0, 1.0)
        pad = torch.zeros((L, H + 2 * half, W + 2 * half), dtype=torch.float32)
        pad[:, half:half + H, half:half + W] = v
        for l in range(L):
            acc = torch.zeros((H, W), dtype=torch.float32)
            for j in range(k):
                if bool(vertical[t, l]):
                    acc = acc + taps[t, k - 1 - j] * pad[l, j:j + H, half:half + W]
                else:
                    acc = acc + taps[t, j] * pad[l, half:half + H, j:j + W]
            out[t, l] = acc
    return out


def state_t(og, start, n, planes, br, layers=None, fix=False):
    """Row b after n[b] (tensor / list) or n (int) steps: D(og_b, n - 1) for n >= 1, start_b (None: og_b) for n == 0, og_b for a negative
    count.  planes [T,L,H,W]; row b reads layer layers[b] if given, else b when L > 1, else 0."""
    B, L = og.shape[0], planes.shape[1]
    counts = [int(n)] * B if isinstance(n, int) else [int(v) for v in n]
    out = og.clone()
    for b, nb in enumerate(counts):
        if nb == 0 and start is not None:
            out[b] = start[b]
        elif nb >= 1:
            lay = int(layers[b]) if layers is not None else (b if L > 1 else 0)
            out[b] = degrade_t(og[b:b + 1], planes[nb - 1, lay][None, None], br, nb - 1, fix)[0]
    return out
