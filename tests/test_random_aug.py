"""The `random_aug=True` chain of the decolorization / snowification packages on the device (`cdf_augment_jitter_batch`, one launch per batch):
RandomResizedCrop -> RandomHorizontalFlip -> RandomApply([ColorJitter(0.8, 0.8, 0.8, 0.2)], p=0.8) -> ToTensor -> t * 2 - 1.

The oracle is written here with PIL calls only (torchvision is not installed; this is what its PIL path runs): `crop`,
`resize(..., Image.BILINEAR)`, `transpose`, `ImageEnhance.Brightness / Contrast / Color`, `convert('HSV')` plus the uint8 add, and
ToTensor's arithmetic -- independent of the package's helpers.  Every stage is integer arithmetic or a few correctly rounded float
operations on 8-bit values, so every comparison is `torch.equal`.  The parameter table is packed here from its documented layout
(include/colddiff.h), not with the package's own packer."""
import contextlib
import io
import itertools
import math
import os
import sys

import numpy as np
import pytest
import torch

from emu_util import P

STRIDE = 16                                                            # CDF_JITTER_STRIDE
NONE = (-1, -1, -1, -1)


# -- the oracle ---------------------------------------------------------------------------------------------------------------------
def _oracle(arr, top, left, h, w, H, W, flip=0, order=NONE, factors=(1.0, 1.0, 1.0), shift=0):
    """arr: uint8 [SH, SW, 3] -> float32 [3, H, W] as torchvision's chain yields it on the PIL image, with the decisions given."""
    from PIL import Image, ImageEnhance
    im = Image.fromarray(np.ascontiguousarray(arr), 'RGB').crop((left, top, left + w, top + h)).resize((W, H), Image.BILINEAR)   # F.resized_crop
    if flip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    for op in order:
        if op == 0:
            im = ImageEnhance.Brightness(im).enhance(float(np.float32(factors[0])))
        elif op == 1:
            im = ImageEnhance.Contrast(im).enhance(float(np.float32(factors[1])))
        elif op == 2:
            im = ImageEnhance.Color(im).enhance(float(np.float32(factors[2])))
        elif op == 3:                                                  # F.adjust_hue: the 8-bit H channel plus uint8(hue_factor * 255), wrapping
            hh, ss, vv = im.convert('HSV').split()
            np_h = (np.array(hh, dtype=np.uint8).astype(np.int32) + int(shift)) & 255
            im = Image.merge('HSV', (Image.fromarray(np_h.astype(np.uint8), 'L'), ss, vv)).convert('RGB')
    t = torch.from_numpy(np.asarray(im).copy()).permute(2, 0, 1).float().div(255)     # ToTensor
    return t * 2 - 1


def _row(top, left, h, w, flip=0, order=NONE, factors=(1.0, 1.0, 1.0), shift=0):
    return dict(top=top, left=left, h=h, w=w, flip=flip, order=tuple(order), factors=tuple(factors), shift=shift)


def _pack(rows):
    t = torch.zeros((len(rows), STRIDE), dtype=torch.int32)
    for i, r in enumerate(rows):
        t[i, 0:5] = torch.tensor([r['top'], r['left'], r['h'], r['w'], r['flip']], dtype=torch.int32)
        t[i, 5:9] = torch.tensor(r['order'], dtype=torch.int32)
        t[i, 9:12] = torch.from_numpy(np.asarray(r['factors'], dtype=np.float32).view(np.int32).copy())
        t[i, 12] = int(r['shift']) & 255
    return t


def _unpack(params):
    rows = []
    for p in params.tolist():
        fac = np.asarray(p[9:12], dtype=np.int32).view(np.float32)
        rows.append(_row(p[0], p[1], p[2], p[3], p[4], tuple(p[5:9]), tuple(float(f) for f in fac), p[12]))
    return rows


def _launch(be, cache, idx, rows, H, W):
    """One launch over the uint8 cache [N, SH, SW, 3] -> CPU float32 [B, 3, H, W]."""
    N, SH, SW, C = cache.shape
    B = len(rows)
    params = _pack(rows)
    out = be.empty(B, 3, H, W)
    be.L.cdf_augment_jitter_batch(P(be.to(cache)), N, SH, SW, C, P(be.to(torch.as_tensor(idx, dtype=torch.int64))), P(be.to(params)), P(params),
                                  P(out), B, H, W, be.stream())
    return out.cpu()


def _check(be, cache, idx, rows, H, W):
    out = _launch(be, cache, idx, rows, H, W)
    arrs = cache.numpy()
    for b, r in enumerate(rows):
        ref = _oracle(arrs[idx[b]], r['top'], r['left'], r['h'], r['w'], H, W, r['flip'], r['order'], r['factors'], r['shift'])
        assert torch.equal(out[b], ref), (b, r, float((out[b] - ref).abs().max()) * 127.5)
    return out


def _images(n, h, w, seed):
    """smooth + noisy content, so that neither the resize nor the colour ops are trivial"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for i in range(n):
        img = np.stack([(xx * 255 // w), (yy * 255 // h), ((xx + yy) * 255 // (w + h))], -1).astype(np.int32) + rng.randint(-60, 60, (h, w, 3))
        out.append(np.clip(np.roll(img, i, axis=2), 0, 255).astype(np.uint8))
    return torch.from_numpy(np.stack(out))


# -- 1. resize geometry ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [16, 32])
def test_resize_geometry(be, size):
    """The filter window is clamped to the CROP: whole image (down both axes), 5 x 7 (up both), 16 x 16 at the four corners (identity at
    size 16), 1 x 1 and 1 x 52 (degenerate windows), 40 x 3 (down one axis, up the other); each with and without the mirror.  No jitter."""
    SH, SW = 40, 52
    cache = _images(3, SH, SW, seed=1)
    boxes = [(0, 0, SH, SW), (11, 20, 5, 7), (0, 0, 16, 16), (0, SW - 16, 16, 16), (SH - 16, 0, 16, 16), (SH - 16, SW - 16, 16, 16),
             (7, 9, 1, 1), (13, 0, 1, SW), (0, 25, SH, 3)]
    rows = [_row(*bx, flip=f) for f in (0, 1) for bx in boxes]
    idx = [i % 3 for i in range(len(rows))]
    _check(be, cache, idx, rows, size, size)


def test_resize_to_a_rectangle_that_is_no_multiple_of_four(be):
    """H != W and H * W odd: the last 4-pixel group of the working image is partial and the stores take the scalar form."""
    cache = _images(2, 40, 52, seed=2)
    rows = [_row(3, 5, 30, 41, flip=1, order=(1, 3, 0, 2), factors=(1.3, 0.6, 1.7), shift=222), _row(0, 0, 40, 52), _row(1, 1, 13, 9, order=(2, 1, -1, -1), factors=(1, 1.8, 0.2))]
    _check(be, cache, [0, 1, 1], rows, 13, 9)


# -- 2. each op alone -------------------------------------------------------------------------------------------------------------------
def _op_images():
    rng = np.random.RandomState(7)
    rnd = rng.randint(0, 256, (16, 16, 3)).astype(np.uint8)
    black, white = np.zeros((16, 16, 3), np.uint8), np.full((16, 16, 3), 255, np.uint8)
    grey = np.repeat(rng.randint(0, 256, (16, 16, 1)), 3, axis=2).astype(np.uint8)
    # r = g = b = v has L = v, so the grey mean is sum(v) / 256: 100 + 128 / 256 is exactly the half-integer 100.5 (rounds up to 101),
    # 100 + 127 / 256 is the nearest mean below it (rounds to 100)
    half = np.full(256, 100, np.uint8)
    half[:128] = 101
    below = np.full(256, 100, np.uint8)
    below[:127] = 101
    half = np.repeat(rng.permutation(half).reshape(16, 16, 1), 3, axis=2)
    below = np.repeat(rng.permutation(below).reshape(16, 16, 1), 3, axis=2)
    return torch.from_numpy(np.stack([rnd, black, white, grey, half, below]))


def test_each_op_alone(be):
    """Brightness / contrast / saturation at 0.2 and 0.63 (interpolating branch of Image.blend: truncation), 1.0, 1.37 and 1.8
    (extrapolating branch: clipped at 0 and 255); hue shifts 0, +51, 205 (= -51), 255; on a random, a black, a white and a grey image and
    on two images whose grey mean is at / just below a half-integer."""
    cache = _op_images()
    rows, idx = [], []
    for n in range(cache.shape[0]):
        for op in (0, 1, 2):
            for f in (0.2, 0.63, 1.0, 1.37, 1.8):
                fac = [1.0, 1.0, 1.0]
                fac[op] = f
                rows.append(_row(0, 0, 16, 16, order=(op, -1, -1, -1), factors=fac))
                idx.append(n)
        for sh in (0, 51, 205, 255):
            rows.append(_row(0, 0, 16, 16, order=(-1, 3, -1, -1), shift=sh))
            idx.append(n)
    out = _check(be, cache, idx, rows, 16, 16)
    assert out.min() == -1.0 and out.max() == 1.0                        # both clamps were reached


# -- 3. op order ----------------------------------------------------------------------------------------------------------------------------
def test_all_orders_in_one_launch(be):
    """The 24 permutations and the declined RandomApply, 25 rows of one launch with per-row parameters: each op sees the uint8 result of
    the one before, and contrast the grey mean of the image as it is when it runs."""
    cache = _images(1, 16, 16, seed=3)
    rows = [_row(0, 0, 16, 16, order=perm, factors=(0.6, 1.5, 1.4), shift=30) for perm in itertools.permutations(range(4))]
    rows.append(_row(0, 0, 16, 16, order=NONE, factors=(0.6, 1.5, 1.4), shift=30))
    out = _check(be, cache, [0] * 25, rows, 16, 16)
    assert len({out[b].numpy().tobytes() for b in range(25)}) > 12      # the order matters


# -- 4. hue over the whole domain ----------------------------------------------------------------------------------------------------------------
def test_hue_over_the_rgb_cube(be):
    """Hue op only, shifts 0 and 37, identity crops of 64 x 64 images that enumerate RGB triples: all 2^24 colours (4096 images) on the
    MI355X, 64 of the images (262 144 colours, fixed seed) on the simulator."""
    from PIL import Image
    if be.kind == "hip":
        pick = np.arange(4096)
    else:
        pick = np.sort(np.random.RandomState(11).choice(4096, 64, replace=False))
    c = (pick[:, None].astype(np.int64) * 4096 + np.arange(4096)[None, :])
    arr = np.stack([c >> 16, (c >> 8) & 255, c & 255], -1).astype(np.uint8).reshape(len(pick), 64, 64, 3)
    cache = torch.from_numpy(arr)
    N = len(pick)
    dcache = be.to(cache)
    idx = be.to(torch.arange(N, dtype=torch.int64))
    hsv = np.asarray(Image.fromarray(arr.reshape(-1, 64, 3), 'RGB').convert('HSV')).copy()
    for shift in (0, 37):
        params = _pack([_row(0, 0, 64, 64, order=(3, -1, -1, -1), shift=shift)] * N)
        out = be.empty(N, 3, 64, 64)
        be.L.cdf_augment_jitter_batch(P(dcache), N, 64, 64, 3, P(idx), P(be.to(params)), P(params), P(out), N, 64, 64, be.stream())
        moved = hsv.copy()
        moved[:, :, 0] = ((moved[:, :, 0].astype(np.int32) + shift) & 255).astype(np.uint8)
        rgb = np.asarray(Image.fromarray(moved, 'HSV').convert('RGB')).reshape(N, 64, 64, 3)
        ref = torch.from_numpy(rgb.copy()).permute(0, 3, 1, 2).float().div(255) * 2 - 1
        got = out.cpu()
        bad = int((got != ref).any(dim=1).sum())
        assert bad == 0, f"shift {shift}: {bad} of {N * 4096} colours differ"
        del out, got, ref


# -- 5. production geometry -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_production_geometry_with_drawn_parameters():
    """One 8-image batch from a 218 x 178 cache (CelebA's aligned size) to 128 x 128 -- the largest LDS footprint the Trainer produces --
    with the parameters the loader draws under a fixed seed, image by image against the PIL oracle."""
    from colddiff import _lib
    from colddiff.trainer import draw_random_aug, jitter_lds_bytes
    L = _lib.get()
    dev = torch.device("cuda:0")
    SH, SW, S = 218, 178, 128
    assert 48 * 1024 < jitter_lds_bytes(SH, SW, S, S) <= 64 * 1024
    cache = _images(8, SH, SW, seed=5)
    params = draw_random_aug(torch.Generator().manual_seed(2024), 8, SH, SW)
    rows = _unpack(params)
    assert any(r['order'] != NONE for r in rows) and len({(r['h'], r['w']) for r in rows}) > 4
    idx = torch.tensor([3, 0, 7, 1, 6, 2, 5, 4])
    dcache, didx, dparams = cache.to(dev), idx.to(dev), params.to(dev)
    out = torch.empty((8, 3, S, S), device=dev)
    L.cdf_augment_jitter_batch(P(dcache), 8, SH, SW, 3, P(didx), P(dparams), P(params), P(out), 8, S, S, torch.cuda.current_stream().cuda_stream)
    again = torch.empty_like(out)
    L.cdf_augment_jitter_batch(P(dcache), 8, SH, SW, 3, P(didx), P(dparams), P(params), P(again), 8, S, S, torch.cuda.current_stream().cuda_stream)
    got = out.cpu()
    assert torch.equal(got, again.cpu())                                  # integer reductions: run-to-run identical
    arrs = cache.numpy()
    for b, r in enumerate(rows):
        ref = _oracle(arrs[idx[b]], r['top'], r['left'], r['h'], r['w'], S, S, r['flip'], r['order'], r['factors'], r['shift'])
        assert torch.equal(got[b], ref), (b, r)


# -- 6. argument checks -----------------------------------------------------------------------------------------------------------------------
def test_argument_checks_return_status_without_a_device():
    """A bad argument is a status + message, never an abort, never a launch: the checks are host-side (on the parameter table's host copy),
    so they run on the device build without a GPU."""
    from colddiff import _lib
    from colddiff.trainer import jitter_lds_bytes
    lib = _lib.Lib(_lib.LIB_PATH)
    cache = torch.zeros((2, 20, 24, 3), dtype=torch.uint8)
    idx = torch.zeros(2, dtype=torch.int64)
    out = torch.zeros((2, 3, 8, 8))
    good = _row(0, 0, 20, 24, order=(0, 1, 2, 3))

    def expect(text, rows=(good, good), C=3, H=8, W=8, SH=20, SW=24, null=None):
        params = _pack(list(rows))
        args = [P(cache), 2, SH, SW, C, P(idx), P(params), P(params), P(out), 2, H, W, 0]
        if null is not None:
            args[null] = 0
        with pytest.raises(_lib.CdfError) as e:
            lib.cdf_augment_jitter_batch(*args)
        assert text in str(e.value), str(e.value)

    for pos in (0, 5, 6, 7, 8):
        expect("null pointer", null=pos)
    expect("1 channels", C=1)
    expect("4 channels", C=4)
    for bad in (_row(0, 0, 21, 24), _row(0, 1, 20, 24), _row(-1, 0, 5, 5), _row(0, -2, 5, 5), _row(19, 0, 2, 5), _row(3, 3, 0, 5), _row(3, 3, 5, 0),
                _row(3, 3, -4, 5), _row(0, 0, 2 ** 31 - 1, 5)):
        expect("crop box of row 1", rows=(good, bad))
    expect("op code 4 in row 0", rows=(_row(0, 0, 5, 5, order=(0, 4, 1, 2)), good))
    expect("op code -2 in row 1", rows=(good, _row(0, 0, 5, 5, order=(-1, -1, -1, -2))))
    # the 160 KB cap: image_size 256 (a 192 KB working image), and tables whose pitch a huge source inflates
    expect("bytes of LDS", H=256, W=256)
    need = jitter_lds_bytes(20, 40000, 128, 128)
    assert need > 160 * 1024 >= jitter_lds_bytes(218, 178, 128, 128)
    expect(f"needs {need} bytes of LDS", H=128, W=128, SW=40000)
    assert lib._dll.cdf_augment_jitter_batch(0, 2, 20, 24, 3, 0, 0, 0, 0, 2, 8, 8, 0) == -1            # CDF_E_INVALID


def test_kernel_compiles_to_zero_scratch():
    """hipcc's resource report for gfx950 (cross-compiles without a GPU), as test_abi does for the hot kernels."""
    import re
    import shutil
    import subprocess
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    if not shutil.which(hipcc):
        pytest.skip("hipcc not available")
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(repo, "cold-diffusion-models_amd", "csrc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I", csrc, "-I", os.path.join(repo, "include"), "-c",
                        os.path.join(csrc, "k_data.hip"), "-o", os.devnull, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    cur, seen = None, {}
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and cur:
            seen[cur] = int(m.group(1))
    mine = {k: v for k, v in seen.items() if "augment_jitter_kernel" in k}
    assert mine and all(v == 0 for v in mine.values()), seen


# -- 7. draws -----------------------------------------------------------------------------------------------------------------------------------
def test_draws_follow_the_documented_distributions():
    from colddiff.trainer import draw_random_aug
    SH, SW, n = 40, 52, 4096
    p = draw_random_aug(torch.Generator().manual_seed(99), n, SH, SW)
    assert p.shape == (n, STRIDE) and p.dtype == torch.int32
    assert torch.equal(p, draw_random_aug(torch.Generator().manual_seed(99), n, SH, SW))          # one seed, one table
    top, left, h, w, flip = (p[:, i].double() for i in range(5))
    assert bool(((h >= 1) & (w >= 1) & (top >= 0) & (left >= 0) & (top + h <= SH) & (left + w <= SW)).all())
    drawn = p[:, 13] >= 0                                                                          # accepted attempt (else the fallback box)
    assert int(drawn.sum()) > n * 0.99 and int(p[:, 13].max()) <= 9 and int(p[:, 13].min()) >= -1
    # w = round(sqrt(a r)), h = round(sqrt(a / r)) are each within 1/2 of the real value, so (w -+ 1/2)(h -+ 1/2) brackets the drawn
    # area a in [0.08, 1] * SH * SW, and (w -+ 1/2) / (h +- 1/2) the drawn ratio r in [3/4, 4/3]: nothing beyond the integer rounding
    area = float(SH * SW)
    hd, wd = h[drawn], w[drawn]
    assert bool(((wd + 0.5) * (hd + 0.5) >= 0.08 * area).all()) and bool(((wd - 0.5) * (hd - 0.5) <= area).all())
    assert bool(((wd - 0.5) / (hd + 0.5) <= 4.0 / 3.0).all()) and bool(((wd + 0.5) / (hd - 0.5) >= 3.0 / 4.0).all())
    assert float((wd * hd).min()) < 0.15 * area and float((wd * hd).max()) > 0.9 * area             # the range is used
    assert int(top.max()) > 0 and int(left.max()) > 0
    fb = p[~drawn]
    assert bool(((fb[:, 2] == SH) & (fb[:, 3] == SW) & (fb[:, 0] == 0) & (fb[:, 1] == 0)).all())   # 52 / 40 is an allowed ratio: the whole image
    # ops: a permutation of 0..3 or all -1; factors in [0.2, 1.8]; shift = trunc(hue_factor * 255) mod 256 with |hue_factor| <= 0.2
    ops = p[:, 5:9]
    applied = ops[:, 0] >= 0
    assert bool((ops[~applied] == -1).all()) and bool((ops[applied].sort(dim=1).values == torch.arange(4, dtype=torch.int32)).all())
    assert len({tuple(r) for r in ops[applied].tolist()}) == 24
    fac = torch.from_numpy(p[:, 9:12].contiguous().numpy().view(np.float32).copy()).double()[applied]
    assert float(fac.min()) >= 0.2 and float(fac.max()) <= 1.8 and float(fac.min()) < 0.21 and float(fac.max()) > 1.79
    allowed = {v % 256 for v in range(-math.trunc(0.2 * 255), math.trunc(0.2 * 255) + 1)}
    shifts = set(p[applied, 12].tolist())
    assert shifts <= allowed and len(shifts) > 90
    # frequencies: a Bernoulli(q) count over n draws has sigma = sqrt(n q (1 - q)); 5 sigma is a 6e-7 two-sided tail
    for count, q in ((int(flip.sum()), 0.5), (int(applied.sum()), 0.8)):
        assert abs(count - n * q) <= 5 * math.sqrt(n * q * (1 - q)), (count, q)
    # a 4 x 200 image: every attempt has h = round(sqrt(a / r)) >= sqrt(0.08 * 800 / (4/3)) = 6.9 > 4, so all ten fail and the
    # box is the centred 4/3 one: h = 4, w = round(4 * 4/3) = 5
    q = draw_random_aug(torch.Generator().manual_seed(5), 256, 4, 200)
    assert bool((q[:, 13] == -1).all()) and bool((q[:, 0:4] == torch.tensor([0, 97, 4, 5], dtype=torch.int32)).all())
    # ... and a 200 x 4 one: w = 4, h = round(4 / (3/4)) = 5
    q = draw_random_aug(torch.Generator().manual_seed(5), 64, 200, 4)
    assert bool((q[:, 13] == -1).all()) and bool((q[:, 0:4] == torch.tensor([97, 0, 5, 4], dtype=torch.int32)).all())


def test_recipes_keep_their_repr():
    """The new Recipe fields are defaulted: the existing recipes and their repr are unchanged."""
    from colddiff import trainer as T
    assert repr(T.AUG1) == "Recipe(Dataset_Aug1: resize=sq112 pad=0 crop=random flip=True rgb=False)"
    assert T.AUG1.jitter is None and T.RANDOM_AUG.crop == 'rrc' and T.RANDOM_AUG.jitter == (0.8, 0.8, 0.8, 0.2) and T.RANDOM_AUG.jitter_p == 0.8
    assert T.RANDOM_AUG.with_rgb().jitter == T.RANDOM_AUG.jitter


# -- 8. end to end ------------------------------------------------------------------------------------------------------------------------------
class _Where:
    def __init__(self, kind):
        self.kind = kind
        self.device = torch.device("cuda:0" if kind == "hip" else "cpu")


@pytest.fixture(params=[pytest.param("emu"), pytest.param("hip", marks=pytest.mark.gpu)])
def where(request):
    from colddiff import runtime
    if request.param == "emu":
        from emu_util import install_emu
        install_emu()
    else:
        runtime._lib_override = None
    yield _Where(request.param)
    runtime._lib_override = None


def _write_folder(folder, n, h, w, seed=0, mode='RGB'):
    from PIL import Image
    os.makedirs(folder, exist_ok=True)
    imgs = _images(n, h, w, seed).numpy()
    for i in range(n):
        a = imgs[i] if mode == 'RGB' else imgs[i][:, :, 0]
        Image.fromarray(a, mode).save(os.path.join(folder, f"im{i:02d}.png"))
    return imgs


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()) as buf:
        return fn(*a, **k), buf.getvalue()


def test_loader_and_trainer_on_a_folder(where, tmp_path, monkeypatch):
    from PIL import Image
    from colddiff import decolor as D
    from colddiff import trainer as T
    folder = str(tmp_path / "imgs")
    _write_folder(folder, 7, 40, 52)
    S = 16
    cache = T.DeviceImageCache(folder, S, where.device, decode_threads=2, recipe=T.RANDOM_AUG)
    assert cache.data.shape == (7, 40, 52, 3) and cache.data.device.type == where.device.type
    files = [np.asarray(Image.open(p)) for p in cache.paths]
    dl = T.DeviceLoader(cache, batch_size=3, shuffle=True, seed=21)
    tables = []
    for _ in range(2):
        x = next(dl).cpu()
        assert x.shape == (3, 3, S, S) and dl.last_params.shape == (3, STRIDE) and dl.last_idx.shape == (3,)
        tables.append(dl.last_params.clone())
        for b, r in enumerate(_unpack(dl.last_params)):
            ref = _oracle(files[int(dl.last_idx[b])], r['top'], r['left'], r['h'], r['w'], S, S, r['flip'], r['order'], r['factors'], r['shift'])
            assert torch.equal(x[b], ref), (b, r)
    assert not torch.equal(tables[0], tables[1])
    # the draws come from a CPU generator: the same seed gives the same tables wherever the kernel runs
    g = torch.Generator().manual_seed(21)
    assert torch.equal(tables[0], T.draw_random_aug(g, 3, 40, 52)) and torch.equal(tables[1], T.draw_random_aug(g, 3, 40, 52))
    other = T.DeviceLoader(cache, batch_size=3, shuffle=True, seed=21, rank=1, world=2)
    next(other)
    assert not torch.equal(other.last_params, tables[0])                  # seed + 7919 * rank

    # -- the Trainer, with torchvision absent ---------------------------------------------------------------------------------------
    monkeypatch.setitem(sys.modules, "torchvision", None)                 # `import torchvision` raises ImportError (other tests may have left a stub)
    torch.manual_seed(0)
    net = _quiet(D.UnetConvNextBlock, dim=8, dim_mults=(1, 2))[0].to(where.device)
    diff = D.DecolorDiffusion(net, image_size=(S, S), device_of_kernel='cuda', channels=3, timesteps=4, loss_type='l1').to(where.device)
    kw = dict(image_size=(S, S), train_batch_size=2, gradient_accumulate_every=2, results_folder=str(tmp_path / "res"), num_workers=0)
    tr, _ = _quiet(D.DecolorTrainer, diff, folder, random_aug=True, device_data=True, **kw)
    assert tr.device_data and type(tr.dl).__name__ == "DeviceLoader" and tr.recipe is T.RANDOM_AUG and len(tr.ds) == 7
    b = tr._next_batch()
    assert b.shape == (2, 3, S, S) and b.dtype == torch.float32 and b.device.type == where.device.type
    assert -1 <= float(b.min()) and float(b.max()) <= 1
    r = _unpack(tr.dl.last_params)[1]
    ref = _oracle(files[int(tr.dl.last_idx[1])], r['top'], r['left'], r['h'], r['w'], S, S, r['flip'], r['order'], r['factors'], r['shift'])
    assert torch.equal(b[1].cpu(), ref)
    if where.kind == "hip":                                               # automatic: on for a HIP device
        tr2, _ = _quiet(D.DecolorTrainer, diff, folder, random_aug=True, **kw)
        assert tr2.device_data and type(tr2.dl).__name__ == "DeviceLoader"
    # the host path is unchanged: it needs torchvision and says which option asked for it
    with pytest.raises(ImportError, match="random_aug=True"):
        _quiet(D.DecolorTrainer, diff, folder, random_aug=True, device_data=False, **kw)
    with pytest.raises(ImportError, match="torchvision_dataset=True"):
        _quiet(D.DecolorTrainer, diff, folder, random_aug=True, torchvision_dataset=True, device_data=True, dataset='cifar10', **kw)
    # a folder the cache cannot hold (ragged sizes; greyscale files) falls back to the host path with the printed reason
    ragged = str(tmp_path / "ragged")
    _write_folder(ragged, 3, 40, 52)
    Image.fromarray(np.zeros((30, 30, 3), np.uint8)).save(os.path.join(ragged, "zz.png"))
    grey = str(tmp_path / "grey")
    _write_folder(grey, 3, 40, 52, mode='L')
    for bad, why in ((ragged, "ragged sizes"), (grey, "RGB folder")):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf), pytest.raises(ImportError, match="random_aug=True"):
            D.DecolorTrainer(diff, bad, random_aug=True, device_data=True, **kw)
        assert "device image cache not used" in buf.getvalue() and why in buf.getvalue(), buf.getvalue()
    with pytest.raises(T.CacheUnfit, match="bytes of LDS"):
        big = str(tmp_path / "big")
        _write_folder(big, 1, 4, 16000)
        T.DeviceImageCache(big, 128, where.device, recipe=T.RANDOM_AUG)
