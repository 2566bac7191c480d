"""The Trainers' input pipeline and image-grid writers: dataset recipes as data, PIL datasets, the device image cache and its loader (SURVEY
8(f) item 2).  Imports neither `trainer` nor `evaluate` (both import from here); `colddiff.trainer` re-exports every public name."""
import os
from pathlib import Path

import torch
from torch.utils import data

from . import runtime as rt


def cycle(dl, sampler=None):
    """Endless iterator over a DataLoader (DEBLUR:52-55); a DistributedSampler is re-seeded on every wrap-around so that the
    ranks' shards are re-shuffled each epoch."""
    epoch = 0
    while True:
        if sampler is not None and hasattr(sampler, 'set_epoch'):
            sampler.set_epoch(epoch)
        for d in dl:
            yield d
        epoch += 1


# -- image folder datasets with PIL only (torchvision is not a dependency) -------------------------------------------
class Recipe:
    """One of the reference's `transforms.Compose` chains, as data.  Every chain is
    [deterministic resize] -> crop (random / centre, optionally after a zero border) -> [mirror] -> ToTensor -> t * 2 - 1.

    resize: 'sq112'  transforms.Resize((int(1.12 s), int(1.12 s)))                    (DEBLUR:990, 1011)
            'short'  transforms.Resize(s): shorter edge to s, aspect kept             (RESOL:824, DEFADE:564)
            'none'   the file's own size                                              (DEFADE:588: RandomCrop first; the Resize(s)
                                                                                       after an s x s crop returns its input)
    pad:    RandomCrop(s, padding=pad), constant fill 0                               (RESOL:825, DEFADE:588)
    crop:   'random' (RandomCrop) | 'center' (CenterCrop)
    rgb:    img.convert('RGB') before the chain                                       (DENOISE:565, 588)

    The one chain of another shape is crop 'rrc': RandomResizedCrop(s) -> mirror -> RandomApply([ColorJitter(*jitter)], p=jitter_p)
    (decolorization / snowification `random_aug=True`, diffusion.py:516-526); its crop is resized PER SAMPLE, on the device."""

    def __init__(self, name, resize, crop, flip, pad=0, rgb=False, jitter=None, jitter_p=0.0):
        self.name, self.resize, self.crop, self.flip, self.pad, self.rgb = name, resize, crop, flip, pad, rgb
        self.jitter, self.jitter_p = jitter, jitter_p

    def with_rgb(self):
        return Recipe(self.name, self.resize, self.crop, self.flip, self.pad, True, self.jitter, self.jitter_p)

    def __repr__(self):
        return f"Recipe({self.name}: resize={self.resize} pad={self.pad} crop={self.crop} flip={self.flip} rgb={self.rgb})"


AUG1 = Recipe('Dataset_Aug1', 'sq112', 'random', True)                  # DEBLUR:983-1004
CENTER112 = Recipe('Dataset', 'sq112', 'center', False)                 # DEBLUR:1006-1026
AUG2 = Recipe('Dataset_Aug2', 'short', 'random', True, pad=4)           # RESOL:817-831
CIFAR_PAD = Recipe('DatasetCifar10', 'none', 'random', True, pad=4)     # DEFADE:579-599
CENTER_SHORT = Recipe('Dataset', 'short', 'center', False)              # DEFADE:557-576
RANDOM_AUG = Recipe('Dataset(random_aug)', 'none', 'rrc', True, jitter=(0.8, 0.8, 0.8, 0.2), jitter_p=0.8)   # DECOLOR diffusion.py:516-526


def center_offset(full, size):
    """torchvision's CenterCrop: int(round((full - size) / 2.0)) with Python's round-half-to-even -- NOT (full - size) // 2:
    143 -> 128 starts at 8, 71 -> 64 at 4, 35 -> 32 and 31 -> 28 at 2."""
    return int(round((full - size) / 2.0))


def resized(img, size, recipe):
    """The deterministic head of the chain on a PIL image (convert, Resize)."""
    from PIL import Image
    if recipe.rgb:
        img = img.convert('RGB')
    if recipe.resize == 'sq112':
        big = int(size * 1.12)
        return img.resize((big, big), Image.BILINEAR)
    if recipe.resize == 'short':
        w, h = img.size
        short, long = (w, h) if w <= h else (h, w)
        if short == size:
            return img                                   # torchvision returns the image itself
        new_long = int(size * long / short)
        return img.resize((size, new_long) if w <= h else (new_long, size), Image.BILINEAR)
    return img


def _load_image(path, size, recipe):
    from PIL import Image
    import numpy as np
    img = resized(Image.open(path), size, recipe)
    arr = np.asarray(img)
    if arr.ndim == 2:
        arr = arr[:, :, None]
    if recipe.pad:
        arr = np.pad(arr, ((recipe.pad, recipe.pad), (recipe.pad, recipe.pad), (0, 0)))
    H, W = arr.shape[:2]
    assert H >= size and W >= size, f"{path}: {W}x{H} after the resize is smaller than the {size}x{size} crop"
    if recipe.crop == 'random':
        if H == size and W == size:
            oy = ox = 0                                  # RandomCrop.get_params draws nothing in this case
        else:
            oy = int(torch.randint(0, H - size + 1, (1,)))          # i (top) first, then j (left)
            ox = int(torch.randint(0, W - size + 1, (1,)))
    else:
        oy, ox = center_offset(H, size), center_offset(W, size)
    arr = arr[oy:oy + size, ox:ox + size]
    if recipe.flip and torch.rand(1).item() < 0.5:
        arr = arr[:, ::-1]
    t = torch.from_numpy(np.array(arr)).permute(2, 0, 1).float().div(255)   # ToTensor
    return t * 2 - 1


class Dataset(data.Dataset):
    recipe = CENTER112

    def __init__(self, folder, image_size, exts=('jpg', 'jpeg', 'png'), recipe=None):
        super().__init__()
        self.folder, self.image_size = folder, image_size
        self.paths = [p for ext in exts for p in Path(f'{folder}').glob(f'**/*.{ext}')]
        if recipe is not None:
            self.recipe = recipe

    def __len__(self):
        return len(self.paths)

    def __getitem__(self, index):
        return _load_image(self.paths[index], self.image_size, self.recipe)


class Dataset_Aug1(Dataset):
    recipe = AUG1


class Dataset_Aug2(Dataset):
    recipe = AUG2


class DatasetCifar10(Dataset):
    recipe = CIFAR_PAD


class SyntheticImages:
    """Endless 8-bit-quantised uniform images generated on the device (benchmarks, smoke tests)."""

    def __init__(self, batch_size, channels, image_size, device, seed=123457):
        self.shape = (batch_size, channels, image_size, image_size)
        self.device = device
        self.gen = torch.Generator(device=device)
        self.gen.manual_seed(seed)

    def __iter__(self):
        return self

    def __next__(self):
        return torch.randint(0, 256, self.shape, generator=self.gen, device=self.device).float() / 255 * 2 - 1


def make_grid(tensor, nrow=8, single_as_is=True):
    """Minimal torchvision.utils.make_grid (padding 2, pad value 0): [B,C,H,W] (or one [C,H,W] image) -> [C, rows, cols] on the host, unscaled.
    `single_as_is`: a batch of ONE image is returned as it is, without the frame, as torchvision does."""
    t = tensor.detach().float().cpu()
    if t.dim() == 3:
        t = t[None]
    B, C, H, W = t.shape
    if B == 1 and single_as_is:
        return t[0]
    ncol = min(nrow, B)
    nr = (B + ncol - 1) // ncol
    pad = 2
    grid = torch.zeros(C, nr * (H + pad) + pad, ncol * (W + pad) + pad)
    for i in range(B):
        r, c = divmod(i, ncol)
        grid[:, pad + r * (H + pad): pad + r * (H + pad) + H, pad + c * (W + pad): pad + c * (W + pad) + W] = t[i]
    return grid


def write_grid(grid, path):
    """[C, rows, cols] in [0,1] -> PNG (torchvision's rounding: x * 255 + 0.5, clamped, truncated)."""
    from PIL import Image
    C = grid.shape[0]
    arr = (grid * 255 + 0.5).clamp(0, 255).to(torch.uint8).permute(1, 2, 0).numpy()
    Image.fromarray(arr[:, :, 0] if C == 1 else arr).save(str(path))


def save_image(tensor, path, nrow=6):
    """Minimal torchvision.utils.save_image: [B,C,H,W] in [0,1] -> PNG grid."""
    write_grid(make_grid(tensor.detach().float().clamp(0, 1), nrow, single_as_is=False), path)


# -- device-side input pipeline -----------------------------------------------------------------------
class CacheUnfit(Exception):
    """The folder cannot live in the device cache (ragged image sizes after the recipe's resize, or larger than the memory
    budget): the Trainer falls back to the host Dataset + DataLoader."""


JITTER_STRIDE = 16           # CDF_JITTER_STRIDE of include/colddiff.h: int32 words per image in the packed parameter table
JITTER_LDS_CAP = 160 * 1024


def jitter_lds_bytes(SH, SW, H, W):
    """LDS need of cdf_augment_jitter_batch (csrc/k_data.hip, jitter_lds_bytes): the uint8 working image + the two coefficient tables,
    whose pitch is Pillow's tap count for a crop as large as the cached image."""
    ksize = lambda n_in, n_out: 3 if n_in <= n_out else 2 * ((n_in + n_out - 1) // n_out) + 1
    return 3 * ((H * W + 3) // 4 * 4) + 4 * (W * ksize(SW, W) + H * ksize(SH, H) + 2 * (W + H) + 16)


def draw_random_aug(gen, B, SH, SW, jitter=(0.8, 0.8, 0.8, 0.2), p=0.8, flip=True, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0)):
    """The decisions of RandomResizedCrop -> RandomHorizontalFlip -> RandomApply([ColorJitter]) for B images of SH x SW, drawn from the CPU
    generator `gen` and packed as cdf_augment_jitter_batch takes them: int32 [B, JITTER_STRIDE] =
    top, left, h, w, flip, the four op codes in application order (0 brightness, 1 contrast, 2 saturation, 3 hue; all -1 when RandomApply
    declined), the three factors as float32 bit patterns, the hue shift, and in word 13 (which the kernel ignores) the index of the
    accepted crop attempt, -1 for the fallback box.

    Like the rest of the device loader this reproduces torchvision's DISTRIBUTIONS, not its random stream, and all of a batch's draws are
    vectorised (the ten crop attempts of every image at once).  torchvision is not a dependency and is not installed where this was
    written: the rules below are restated from its documented behaviour and could not be compared against it live.
      crop   : up to 10 attempts of area * U(scale), aspect exp(U(ln ratio)); w = round(sqrt(a r)), h = round(sqrt(a / r)); the first with
               0 < w <= SW and 0 < h <= SH wins, top ~ randint[0, SH - h], left ~ randint[0, SW - w]; otherwise the centred box of the
               nearest allowed aspect ratio (the whole image when its own ratio is allowed)
      flip   : U < 0.5            apply : U <= p            order : randperm(4)
      factors: U(max(0, 1 - x), 1 + x) as float32 for brightness, contrast, saturation; hue_factor ~ U(-hue, hue), and the shift added to
               the 8-bit H channel is trunc(hue_factor * 255) mod 256 (the uint8 cast torchvision applies)"""
    import math
    f64 = torch.float64
    area = float(SH * SW)
    target = area * (scale[0] + (scale[1] - scale[0]) * torch.rand((B, 10), generator=gen, dtype=f64))
    lo, hi = math.log(ratio[0]), math.log(ratio[1])
    aspect = torch.exp(lo + (hi - lo) * torch.rand((B, 10), generator=gen, dtype=f64))
    w = torch.round(torch.sqrt(target * aspect)).to(torch.int64)
    h = torch.round(torch.sqrt(target / aspect)).to(torch.int64)
    ok = (w > 0) & (w <= SW) & (h > 0) & (h <= SH)
    any_ok = ok.any(dim=1)
    first = torch.argmax(ok.to(torch.int8), dim=1)                          # the first accepted attempt (0 where none is: replaced below)
    w, h = w.gather(1, first[:, None])[:, 0], h.gather(1, first[:, None])[:, 0]
    u_top, u_left = torch.rand((B,), generator=gen, dtype=f64), torch.rand((B,), generator=gen, dtype=f64)
    in_ratio = SW / SH
    if in_ratio < ratio[0]:
        fw, fh = SW, int(round(SW / ratio[0]))
    elif in_ratio > ratio[1]:
        fh, fw = SH, int(round(SH * ratio[1]))
    else:
        fw, fh = SW, SH
    w, h = torch.where(any_ok, w, torch.tensor(fw)), torch.where(any_ok, h, torch.tensor(fh))
    top = torch.minimum(torch.floor(u_top * (SH - h + 1)).to(torch.int64), SH - h)
    left = torch.minimum(torch.floor(u_left * (SW - w + 1)).to(torch.int64), SW - w)
    top, left = torch.where(any_ok, top, (SH - h) // 2), torch.where(any_ok, left, (SW - w) // 2)
    u_flip = torch.rand((B,), generator=gen, dtype=f64)
    u_apply = torch.rand((B,), generator=gen, dtype=f64)
    order = torch.argsort(torch.rand((B, 4), generator=gen, dtype=f64), dim=1)
    u_fac = torch.rand((B, 3), generator=gen, dtype=torch.float32)
    u_hue = torch.rand((B,), generator=gen, dtype=f64)
    out = torch.zeros((B, JITTER_STRIDE), dtype=torch.int32)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = top, left, h, w
    out[:, 4] = (u_flip < 0.5) if flip else 0
    out[:, 5:9] = -1
    out[:, 13] = torch.where(any_ok, first, torch.tensor(-1))
    if jitter is not None:
        apply = u_apply <= p
        out[:, 5:9] = torch.where(apply[:, None], order, torch.tensor(-1)).to(torch.int32)
        # the float32 values nearest the interval's ends from INSIDE: float32(0.2) + float32(1.6) rounds to a value above 1.8
        inf = torch.tensor(float('inf'), dtype=torch.float32)
        f_lo = torch.tensor([max(0.0, 1.0 - x) for x in jitter[:3]], dtype=torch.float32)
        f_hi = torch.tensor([1.0 + x for x in jitter[:3]], dtype=torch.float32)
        f_lo = torch.where(f_lo.double() < torch.tensor([max(0.0, 1.0 - x) for x in jitter[:3]], dtype=f64), torch.nextafter(f_lo, inf), f_lo)
        f_hi = torch.where(f_hi.double() > torch.tensor([1.0 + x for x in jitter[:3]], dtype=f64), torch.nextafter(f_hi, -inf), f_hi)
        fac = torch.maximum(torch.minimum(f_lo + (f_hi - f_lo) * u_fac, f_hi), f_lo)
        out[:, 9:12] = fac.contiguous().view(torch.int32)
        hue_factor = jitter[3] * (2.0 * u_hue - 1.0)
        out[:, 12] = (torch.trunc(hue_factor * 255.0).to(torch.int64) % 256).to(torch.int32)
    return out


class DeviceImageCache:
    """An image folder decoded ONCE and kept in HBM as uint8 NHWC, already past the DETERMINISTIC head of the reference's
    transform chain (`convert('RGB')`, `transforms.Resize(...)` -- done with the same PIL call on the host at cache-build time by a
    thread pool).  What is random per sample (crop offset, mirror) or pure arithmetic (border, ToTensor, t*2-1) runs per batch in
    ONE kernel (cdf_augment_batch_pad): the training loop never waits for host image workers (the reference spawns 8-16 PIL
    processes, DEBLUR:1095, 1107, 1114).  CelebA (202 599 images) at S = 143: 12.4 GB of the MI355X's 288 GB.
    Raises CacheUnfit when the images are not all of one size after the resize (`Resize(s)` keeps the aspect ratio) or when the
    cache would not fit next to the model (budget: COLDDIFF_CACHE_FRACTION of the free HBM, default 0.5; pinned host staging buffer
    of the same size, at most half of the free host RAM)."""

    def __init__(self, folder, image_size, device, exts=('jpg', 'jpeg', 'png'), decode_threads=None, paths=None, recipe=None):
        import numpy as np
        from concurrent.futures import ThreadPoolExecutor
        from PIL import Image
        self.recipe = recipe = recipe or AUG1
        self.image_size = image_size
        self.paths = list(paths) if paths is not None else [p for ext in exts for p in Path(f'{folder}').glob(f'**/*.{ext}')]
        assert len(self.paths) > 0, f"no images under {folder}"

        def load(p):
            arr = np.asarray(resized(Image.open(p), image_size, recipe))
            return arr[:, :, None] if arr.ndim == 2 else arr

        first = load(self.paths[0])
        self.SH, self.SW, self.channels = first.shape
        self.S = self.SH                                            # (square caches: the 1.12x chains)
        n = len(self.paths)
        dev = torch.device(device)
        need = n * first.size
        if dev.type == 'cuda':
            free_hbm = torch.cuda.mem_get_info(dev)[0]
            frac = float(os.environ.get("COLDDIFF_CACHE_FRACTION", "0.5"))
            if need > frac * free_hbm:
                raise CacheUnfit(f"{n} images of {self.SH}x{self.SW}x{self.channels} = {need / 2**30:.1f} GiB exceed "
                                 f"{frac:.2f} of the free HBM ({free_hbm / 2**30:.1f} GiB)")
            try:
                import psutil
                if need > 0.5 * psutil.virtual_memory().available:
                    raise CacheUnfit(f"{need / 2**30:.1f} GiB of pinned staging exceed half of the free host memory")
            except ImportError:
                pass
        pad = recipe.pad
        if recipe.crop == 'rrc':
            # RandomResizedCrop scales any box to the output size (a file may be smaller than the crop); what bounds the kernel is RGB and LDS
            if self.channels != 3:
                raise CacheUnfit(f"{self.paths[0]}: {self.channels} channel(s); ColorJitter on the device needs an RGB folder")
            lds = jitter_lds_bytes(self.SH, self.SW, image_size, image_size)
            if lds > JITTER_LDS_CAP:
                raise CacheUnfit(f"{image_size}x{image_size} crops of {self.SW}x{self.SH} images need {lds} bytes of LDS (cap {JITTER_LDS_CAP})")
        elif self.SH + 2 * pad < image_size or self.SW + 2 * pad < image_size:
            raise CacheUnfit(f"{self.paths[0]}: {self.SW}x{self.SH} is smaller than the {image_size}x{image_size} crop")
        host = torch.empty((n, self.SH, self.SW, self.channels), dtype=torch.uint8, pin_memory=dev.type == 'cuda')
        hv = host.numpy()
        hv[0] = first

        def fill(i):
            a = load(self.paths[i])
            if a.shape != first.shape:
                raise CacheUnfit(f"{self.paths[i]}: {a.shape} vs {first.shape} (ragged sizes / mixed image modes in one folder)")
            hv[i] = a

        with ThreadPoolExecutor(max_workers=decode_threads or min(32, os.cpu_count() or 1)) as ex:   # PIL releases the GIL while decoding / resizing
            list(ex.map(fill, range(1, n)))
        self.data = host.to(device, non_blocking=True)

    def __len__(self):
        return len(self.paths)

    def span(self):
        """(rows, columns) of valid crop offsets: the padded image minus the crop, plus one."""
        p = self.recipe.pad
        return self.SH + 2 * p - self.image_size + 1, self.SW + 2 * p - self.image_size + 1

    def center(self):
        p = self.recipe.pad
        return center_offset(self.SH + 2 * p, self.image_size), center_offset(self.SW + 2 * p, self.image_size)

    def batch(self, idx, oy, ox, flip):
        """[B, C, H, H] fp32 batch: images idx (int64 [B]) cropped at (oy, ox) of the bordered image, mirrored where flip != 0
        (int32 [B] each, on the device)."""
        rt.check(self.data)
        B, H = idx.numel(), self.image_size
        out = torch.empty((B, self.channels, H, H), device=self.data.device, dtype=torch.float32)
        rt.lib().cdf_augment_batch_pad(rt.P(self.data), len(self.paths), self.SH, self.SW, self.channels, self.recipe.pad, rt.P(idx), rt.P(oy),
                                       rt.P(ox), rt.P(flip), rt.P(out), B, H, H, rt.stream(self.data))
        return out

    def batch_jitter(self, idx, params_host):
        """[B, 3, H, H] fp32 batch of the 'rrc' recipe in ONE launch: images idx (int64 [B], on the device) through crop -> Pillow's
        bilinear resize -> mirror -> ColorJitter -> ToTensor -> t * 2 - 1 with the decisions `params_host` (CPU int32 [B, JITTER_STRIDE] as
        `draw_random_aug` packs them).  The table travels as one pinned, non-blocking copy; the entry point checks the host copy."""
        rt.check(self.data)
        dev = self.data.device
        B, H = idx.numel(), self.image_size
        assert params_host.shape == (B, JITTER_STRIDE) and params_host.dtype == torch.int32 and params_host.device.type == 'cpu'
        if dev.type == 'cuda':
            pinned = torch.empty((B, JITTER_STRIDE), dtype=torch.int32, pin_memory=True)
            pinned.copy_(params_host)
            params_host, params_dev = pinned, pinned.to(dev, non_blocking=True)
        else:
            params_host = params_dev = params_host.contiguous()
        out = torch.empty((B, 3, H, H), device=dev, dtype=torch.float32)
        rt.lib().cdf_augment_jitter_batch(rt.P(self.data), len(self.paths), self.SH, self.SW, self.channels, rt.P(idx), rt.P(params_dev),
                                          rt.P(params_host), rt.P(out), B, H, H, rt.stream(self.data))
        return out

    def item(self, idx):
        """Image idx as the non-random chain yields it ([C, H, H]; centre crop, no mirror)."""
        dev = self.data.device
        i32 = lambda v: torch.tensor([v], dtype=torch.int32, device=dev)
        cy, cx = self.center()
        return self.batch(torch.tensor([idx], device=dev), i32(cy), i32(cx), i32(0))[0]


class DeviceLoader:
    """Endless batch iterator over a DeviceImageCache with the sampling semantics of the reference's loader: `shuffle=True`
    permutes the indices every epoch, `drop_last` as the package's DataLoader has it (DEBLUR:1095-1096 drops, RESOL:887 keeps the
    short batch), batch_size images per step; with several ranks every rank takes the DistributedSampler slice perm[rank::world] of
    the SAME epoch permutation (seed + epoch on a CPU generator).  Crop and mirror follow the cache's recipe: RandomCrop offsets
    (row first, then column; none drawn when the image IS the crop size, like RandomCrop.get_params) and RandomHorizontalFlip(0.5),
    or CenterCrop.  The 'rrc' recipe (RANDOM_AUG) draws its crop boxes, mirrors and ColorJitter decisions with `draw_random_aug` from a CPU
    generator seeded the same way (seed + 7919 * rank), so one seed gives the same batches on the simulator and on the device;
    `last_params` / `last_idx` hold the packed decisions and the image indices of the batch returned last, for replaying it."""

    last_params = None
    last_idx = None

    def __init__(self, cache, batch_size, shuffle=True, seed=123457, rank=0, world=1, drop_last=True, augment=None):
        self.cache, self.batch_size, self.shuffle, self.drop_last = cache, batch_size, shuffle, drop_last
        rec = cache.recipe
        self.rrc = rec.crop == 'rrc'
        if self.rrc:
            self.aug_gen = torch.Generator()
            self.aug_gen.manual_seed(seed + 7919 * rank)
        self.random_crop = rec.crop == 'random' if augment is None else bool(augment)
        self.flip = rec.flip if augment is None else bool(augment)
        self.seed, self.rank, self.world = seed, rank, world
        self.epoch, self.pos, self.order = 0, 0, None
        dev = cache.data.device
        self.gen = torch.Generator(device=dev)
        self.gen.manual_seed(seed + 7919 * rank)
        n = len(cache) // world if world > 1 else len(cache)
        assert n >= batch_size or not drop_last, f"{len(cache)} images over {world} ranks: fewer than one batch of {batch_size}"
        cy, cx = (0, 0) if self.rrc else cache.center()
        self._cy = torch.full((batch_size,), cy, dtype=torch.int32, device=dev)
        self._cx = torch.full((batch_size,), cx, dtype=torch.int32, device=dev)
        self._noflip = torch.zeros((batch_size,), dtype=torch.int32, device=dev)

    def _new_epoch(self):
        n = len(self.cache)
        if self.shuffle:
            g = torch.Generator().manual_seed(self.seed + self.epoch)
            perm = torch.randperm(n, generator=g)
        else:
            perm = torch.arange(n)
        if self.world > 1:
            perm = perm[:n - n % self.world][self.rank::self.world]
        self.order_host = perm
        self.order = perm.to(self.cache.data.device)
        self.pos = 0
        self.epoch += 1

    def __iter__(self):
        return self

    def __next__(self):
        B = self.batch_size
        left = 0 if self.order is None else self.order.numel() - self.pos
        if left <= 0 or (left < B and self.drop_last):
            self._new_epoch()
            left = self.order.numel()
        B = min(B, left)                                                   # (short last batch when drop_last is off)
        idx = self.order[self.pos:self.pos + B].contiguous()
        if self.rrc:
            rec = self.cache.recipe
            self.last_idx = self.order_host[self.pos:self.pos + B].clone()
            self.last_params = draw_random_aug(self.aug_gen, B, self.cache.SH, self.cache.SW, jitter=rec.jitter, p=rec.jitter_p, flip=rec.flip)
            self.pos += B
            return self.cache.batch_jitter(idx, self.last_params)
        self.pos += B
        return self.batch_of(idx)

    def take_indices(self):
        """Graph mode (drop_last loaders, not 'rrc'): move on by one batch exactly as __next__ does -- a new permutation at an epoch's
        end -- and return the batch's image indices on the HOST (int64 [batch_size]); the Trainer uploads them into a static
        device buffer and `batch_of` reads them there."""
        assert self.drop_last and not self.rrc
        B = self.batch_size
        left = 0 if self.order is None else self.order.numel() - self.pos
        if left < B:
            self._new_epoch()
        idx = self.order_host[self.pos:self.pos + B]
        self.pos += B
        return idx

    def batch_of(self, idx):
        """The batch of images idx (int64 on the device): crop offsets and mirrors are device draws from the loader's generator."""
        B = idx.numel()
        dev = self.cache.data.device
        sy, sx = self.cache.span()
        if self.random_crop and (sy > 1 or sx > 1):
            oy = torch.randint(0, sy, (B,), generator=self.gen, device=dev, dtype=torch.int32)     # RandomCrop: i (top), then j (left)
            ox = torch.randint(0, sx, (B,), generator=self.gen, device=dev, dtype=torch.int32)
        elif self.random_crop:
            oy = ox = self._noflip[:B]
        else:
            oy, ox = self._cy[:B], self._cx[:B]
        if self.flip:
            flip = (torch.rand((B,), generator=self.gen, device=dev) < 0.5).to(torch.int32)      # RandomHorizontalFlip(p = 0.5)
        else:
            flip = self._noflip[:B]
        return self.cache.batch(idx, oy, ox, flip)
