"""`Trainer` — the training loop of the cold-diffusion packages on the fused optimizer tail.

Follows deblurring_diffusion_pytorch.py:1057-1235 (and the denoising variant,
denoising_diffusion_pytorch.py:620-789): same constructor, `train() / save() / load() / step_ema()
/ reset_parameters()`, same checkpoint dict (`step`, `model`, `ema` state_dicts with the
DataParallel `module.` prefix when the model was wrapped), gradient accumulation, Adam(lr) defaults,
EMA copy-then-lerp schedule and milestone sampling.  Differences, all performance-only:
  * Adam / EMA / zero_grad are single kernel launches over a flat parameter arena (colddiff.flat)
  * multi-GPU = one process per GPU + RCCL all-reduce (colddiff.parallel) instead of DataParallel
  * the loss is logged without a host sync on every micro-step (the reference calls loss.item() twice)
"""
import copy
import glob
import os
from functools import partial
from pathlib import Path

import torch
from torch.utils import data

from . import flat, parallel
from .evaluate import EvalMixin, GenEvalMixin
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


def unwrap(model):
    """The reference scripts hand the Trainer a torch.nn.DataParallel wrapper; compute on its module."""
    if isinstance(model, (torch.nn.DataParallel, torch.nn.parallel.DistributedDataParallel)):
        return model.module
    return model


class EMA:
    def __init__(self, beta):
        self.beta = beta

    def update_model_average(self, ma_arena, model_arena):
        flat.ema_update(ma_arena, model_arena, self.beta)


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


def _match_module_prefix(sd, target_keys):
    """The authors' checkpoints are state_dicts of DataParallel-wrapped models (`module.` on every key: DEBLUR:1140-1157 with
    celebA_128.py:102); the same file must load whether or not THIS model is wrapped (the reference's test scripts carry
    remove_data_parallel / adjust_data_parallel helpers for that, e.g. DEBLUR:1026-1055)."""
    has = len(sd) > 0 and all(k.startswith('module.') for k in sd)
    want = all(k.startswith('module.') for k in target_keys)
    if has and not want:
        return {k[len('module.'):]: v for k, v in sd.items()}
    if want and not has:
        return {'module.' + k: v for k, v in sd.items()}
    return sd


class Trainer(EvalMixin):
    # which transform chain a `dataset=` name selects (DEBLUR:1094-1114); the other packages override this table
    drop_last = True
    force_shuffle = False
    image_size_from_model = False

    @staticmethod
    def recipe_for(dataset):
        if dataset in ('mnist', 'cifar10', 'flower', 'celebA', 'AFHQ'):
            return AUG1
        if dataset == 'LSUN_train':                      # (upstream reads the LSUN lmdb through torchvision.datasets; a folder of its
            return Recipe('LSUN_train', 'sq112', 'random', False)     # images gets the same chain: no mirror, DEBLUR:1098-1108)
        return CENTER112

    def __init__(self, diffusion_model, folder, *, ema_decay=0.995, image_size=128, train_batch_size=32, train_lr=2e-5,
                 train_num_steps=100000, gradient_accumulate_every=2, fp16=False, step_start_ema=2000, update_ema_every=10,
                 save_and_sample_every=1000, results_folder='./results', load_path=None, dataset=None, shuffle=True,
                 num_workers=8, device_data=None, graph=None):
        super().__init__()
        assert not fp16, "apex fp16 is not supported (every reference script passes fp16=False)"
        # graph: replay the optimizer step as one captured graph where the Trainer is eligible (`_graph_reason`).  None = read
        # COLDDIFF_GRAPH ("1" turns it on).  Off by default; decided at the first train_step / graph_state call.
        if graph is None:
            graph = os.environ.get("COLDDIFF_GRAPH") == "1"
        self._graph_req = bool(graph)
        self._gs = None
        self.model = diffusion_model
        self.ema = EMA(ema_decay)
        self.ema_model = copy.deepcopy(self.model)
        self.update_ema_every = update_ema_every
        self.step_start_ema = step_start_ema
        self.save_and_sample_every = save_and_sample_every
        self.batch_size = train_batch_size
        self.gradient_accumulate_every = gradient_accumulate_every
        self.train_num_steps = train_num_steps
        self.core = unwrap(self.model)
        # RESOL:874 / DEFADE:681 take the sampling size from the model; the dataset still crops to the `image_size` argument
        self.image_size = self.core.image_size if self.image_size_from_model else image_size
        self.data_image_size = image_size
        self.ema_core = unwrap(self.ema_model)
        # the denoising package feeds (image, fresh Gaussian noise) pairs (DENOISE:738-742)
        self.pair_noise = hasattr(self.core, 'sqrt_alphas_cumprod')
        self.device = next(self.core.parameters()).device
        # device_data: keep the (1.12x-resized, uint8) image folder in HBM and crop / mirror / convert per batch in one kernel instead
        # of PIL DataLoader workers.  None = automatic: on for a HIP device unless COLDDIFF_DEVICE_DATA=0.
        if device_data is None:
            device_data = self.device.type == 'cuda' and os.environ.get("COLDDIFF_DEVICE_DATA", "1") != "0"
        self.device_data = bool(device_data)

        self.ds, self.dl = self._make_loader(folder, dataset, shuffle, num_workers, seed=123457)

        # Adam(diffusion_model.parameters(), lr): one flat arena over every parameter of the model
        self.arena = flat.FlatArena(list(self.core.parameters()))
        self.ema_arena = flat.FlatArena(list(self.ema_core.parameters()))
        self.opt = flat.FusedAdam(self.arena, lr=train_lr)
        self.step = 0
        self.results_folder = Path(results_folder)
        self.results_folder.mkdir(exist_ok=True)
        self.fp16 = fp16
        self.quiet = False

        parallel.init_distributed()
        self.sync = None
        if parallel.world_size() > 1:
            self.sync = parallel.GradSync(self.arena)
            parallel.set_engine(self.sync)
            # ranks may arrive here minutes apart (each decoded its image folder into its device cache above): wait on the long-timeout
            # host group first, so that the broadcast's own watchdog only ever covers the broadcast
            parallel.milestone_barrier()
            # every rank starts from rank 0's weights (the reference replicates GPU 0's module)
            torch.distributed.broadcast(self.arena.data, src=0)
            rt.bump_weights_epoch()
            parallel.decorrelate_rng()     # weights are equal now: from here on every rank draws its own t / noise / masks
        self.reset_parameters()
        if load_path is not None:
            self.load(load_path)

    def _make_loader(self, folder, dataset, shuffle, num_workers, seed):
        """(dataset, endless batch iterator): image folder as in the reference (DEBLUR:1094-1096), or synthetic images."""
        if dataset == 'synthetic' or folder is None:
            # (every rank draws its own shard: the seed is offset by the rank)
            return None, SyntheticImages(self.batch_size, self.core.channels, self.data_image_size, self.device, seed=seed + parallel.rank())
        recipe = self.recipe_for(dataset)
        self.recipe = recipe
        print(dataset, "DA used" if recipe.crop == 'random' else "")
        shuffle = True if self.force_shuffle else shuffle
        drop_last = self.drop_last or parallel.world_size() > 1      # (ranks must run the same number of equal micro-batches)
        if self.device_data:
            try:
                cache = DeviceImageCache(folder, self.data_image_size, self.device, recipe=recipe)
                return cache, DeviceLoader(cache, self.batch_size, shuffle=shuffle, seed=seed, rank=parallel.rank(),
                                           world=parallel.world_size(), drop_last=drop_last)
            except CacheUnfit as e:
                print(f"device image cache not used ({e}); falling back to the host DataLoader")
                self.device_data = False
        ds = Dataset(folder, self.data_image_size, recipe=recipe)
        sampler = None
        if parallel.world_size() > 1:
            sampler = data.distributed.DistributedSampler(ds, shuffle=shuffle)
        dl = cycle(data.DataLoader(ds, batch_size=self.batch_size, shuffle=shuffle and sampler is None, sampler=sampler,
                                   pin_memory=self.device.type == 'cuda', num_workers=num_workers, drop_last=drop_last), sampler)
        return ds, dl

    # -- EMA / checkpoint --------------------------------------------------------------------------------
    def reset_parameters(self):
        """ema_model.load_state_dict(model.state_dict()) (DEBLUR:1131-1132; every `update_ema_every`-th step until step_start_ema): the
        parameters live in two flat arenas of one layout, so they are ONE device copy instead of one per tensor (238 for the CelebA net);
        buffers go through load_state_dict's own path."""
        a, e = getattr(self, "arena", None), getattr(self, "ema_arena", None)
        if a is not None and e is not None and a.numel == e.numel and a.offsets == e.offsets and a.intact() and e.intact():
            e.data.copy_(a.data)
            bufs = dict(self.model.named_buffers())
            with torch.no_grad():
                for name, b in self.ema_model.named_buffers():
                    if name in bufs and b.data_ptr() != bufs[name].data_ptr():
                        b.copy_(bufs[name])
        else:
            self.ema_model.load_state_dict(self.model.state_dict())
        rt.bump_weights_epoch()

    def step_ema(self):
        if self.step < self.step_start_ema:
            self.reset_parameters()
            return
        self.ema.update_model_average(self.ema_arena, self.arena)

    def save(self, itrs=None):
        if parallel.rank() != 0:
            return
        ckpt = {'step': self.step, 'model': self.model.state_dict(), 'ema': self.ema_model.state_dict()}
        name = 'model.pt' if itrs is None else f'model_{itrs}.pt'
        torch.save(ckpt, str(self.results_folder / name))

    def load(self, load_path):
        print("Loading : ", load_path)
        ckpt = torch.load(load_path, map_location=self.device)
        self.step = ckpt['step']
        self.model.load_state_dict(_match_module_prefix(ckpt['model'], self.model.state_dict().keys()))
        self.ema_model.load_state_dict(_match_module_prefix(ckpt['ema'], self.ema_model.state_dict().keys()))
        rt.bump_weights_epoch()
        if self._gs is not None:
            self._graph_rewarm()

    # -- the hot loop (DEBLUR:1183-1235) -----------------------------------------------------------------
    def _next_batch(self):
        d = next(self.dl)
        if isinstance(d, (list, tuple)):
            d = d[0]
        return d.to(self.device, non_blocking=True)

    def _second(self, batch):
        """The second argument of forward(x1, x2), None for the one-image packages; fresh Gaussian noise for the
        denoising package (DENOISE:738-742)."""
        return torch.randn_like(batch) if self.pair_noise else None

    def _sample_source(self):
        """The images a milestone samples from: a data batch, or for the two-image packages the second image
        (fresh noise drawn like a batch: DENOISE:759-762)."""
        og_img = self._next_batch()
        x2 = self._second(og_img)
        return og_img if x2 is None else x2

    # -- degradation prefetch (deblurring: q_sample is up to T sequential blur steps on B*C planes, independent of the network) ----
    # The trajectory is bit-identical to the non-prefetching loop BETWEEN milestones; a milestone's sample batch is drawn after the
    # micro-batches in the queue were already prefetched, i.e. one batch later in the data order than without prefetch for the plain
    # loop and `gradient_accumulate_every` batches later with fused accumulation.  ONE queue serves both loops (draw order = launch
    # order), so switching COLDDIFF_FUSE_ACCUM / falling back after an out-of-memory mid-run skips nothing and leaks nothing.
    _side = None
    _pending_q = None            # prefetched micro-batches [(prep, event)], oldest first
    _fuse_off = False            # set by the out-of-memory fallback of _fused_step

    def _can_prefetch(self):
        """Only for the plain loop on a HIP device: not when a test / subclass replaced _loss, not for two-image packages."""
        return (self.device.type == 'cuda' and hasattr(self.core, 'can_prepare_async') and '_loss' not in self.__dict__
                and type(self)._loss is Trainer._loss and not self.pair_noise and rt._lib_override is None
                and getattr(self.core, 'train_routine', None) == 'Final' and os.environ.get("COLDDIFF_PREFETCH", "1") != "0"
                and self.core.can_prepare_async())

    # -- fused gradient accumulation -------------------------------------------------------------------------------------------
    # The reference runs `gradient_accumulate_every` micro-batches one after the other, (loss_i / accumulate).backward() each
    # (DEBLUR:1188-1195) -- a memory measure for 16 GB cards.  With 288 GB of HBM the micro-batches of one optimizer step are
    # degraded one by one (same data order, same t / noise / offset draws in the same order) and then go through the network as ONE
    # batch: the loss of the concatenated batch is the mean of the micro-batch losses, so one backward pass yields the same
    # gradient sum, every GEMM sees twice the rows (the 16 x 16 layers fill the chip, the weight gradients need half the split-K
    # slabs), weights are read once per step instead of per micro-batch and the launch count halves.
    # CelebA-128 step (2 x 32 images): 58.4 -> 53.2 ms, 1096 -> 1202 img/s in one call (profiles/round4_fused_accumulation_ab.txt).
    FUSE_MAX_PIXELS = int(os.environ.get("COLDDIFF_FUSE_MAX_PIXELS", str(1 << 21)))     # 128 images of 128 x 128 (~90 GB of activations)

    def _can_fuse(self):
        """The plain loop only (not when a test / subclass replaced _loss), equal-sized micro-batches (the loaders that may end an
        epoch on a short batch do not fuse), a core whose training routine has the two-phase form."""
        acc = self.gradient_accumulate_every
        return (acc > 1 and not self._fuse_off and '_loss' not in self.__dict__ and type(self)._loss is Trainer._loss and os.environ.get("COLDDIFF_FUSE_ACCUM", "1") != "0"
                and hasattr(self.core, 'prepare') and self.core.fusable() and (self.drop_last or self.ds is None or parallel.world_size() > 1)
                and acc * self.batch_size * self.data_image_size ** 2 <= self.FUSE_MAX_PIXELS)

    def _prepare_micro(self):
        """One micro-batch in the reference's order of draws: the data batch, the second image / fresh noise (DENOISE:738-742), then
        forward()'s t (and whatever the degradation draws)."""
        batch = self._next_batch()
        x2 = self._second(batch)
        return self.core.prepare(batch) if x2 is None else self.core.prepare(batch, x2)

    def _take_prepared(self, keep):
        """The oldest prefetched micro-batch (launched now if the queue is empty), ordered before the compute stream's next kernel;
        afterwards the queue is topped up to `keep` entries."""
        if self._pending_q is None:
            self._pending_q = []
        if not self._pending_q:
            self._pending_q.append(self._launch_prepare())
        prep, ev = self._pending_q.pop(0)
        torch.cuda.current_stream().wait_event(ev)
        while len(self._pending_q) < keep:
            self._pending_q.append(self._launch_prepare())
        return prep

    def _fused_step(self, acc, prefetch):
        if self.sync is not None:
            self.sync.begin()
        if prefetch:
            # all of the NEXT step's micro-batches are degraded on the side stream under this step's forward / backward
            if self._pending_q is None:
                self._pending_q = []
            while len(self._pending_q) < acc:
                self._pending_q.append(self._launch_prepare())
            preps = [self._take_prepared(0) for _ in range(acc)]
            for _ in range(acc):
                self._pending_q.append(self._launch_prepare())
        else:
            preps = [self._prepare_micro() for _ in range(acc)]
        oom = False
        try:
            prep = tuple(torch.cat(parts) for parts in zip(*preps))
            loss = torch.mean(self.core.loss_prepared(prep))          # = the mean of the micro-batch losses (equal sizes)
            if self.sync is not None:
                self.sync.arm()
            (loss * (1.0 / parallel.world_size())).backward()
            return loss.detach()
        except torch.OutOfMemoryError:
            # FUSE_MAX_PIXELS counts pixels, not model width: a wide model / a shared device may not hold `acc` micro-batches of
            # activations where the reference's one-by-one loop fits.  Single rank only (on several ranks the others are already inside
            # their collectives).  Only a flag is set here: while this handler runs, the exception's traceback keeps every frame of the
            # aborted pass alive (Unet.forward's skip list, the nodes' locals, the partial graph with its saved activations), so the retry
            # happens AFTER the handler, when all of that has been released.
            if self.sync is not None:
                raise
            oom = True
        if oom:
            # drop what the aborted pass left, switch fusion off for this Trainer and run the SAME prepared micro-batches one after the
            # other -- the step's data, t and noise draws are unchanged
            import gc
            prep = loss = None
            self._fuse_off = True
            gc.collect()
            torch.cuda.empty_cache()
            self.opt.zero_grad()
            print(f"fused accumulation of {acc} micro-batches does not fit in device memory: running them one by one from here on")
            total = None
            for p_i in preps:
                l_i = torch.mean(self.core.loss_prepared(p_i))
                (l_i * (1.0 / acc)).backward()
                total = l_i.detach() if total is None else total + l_i.detach()
            return total / acc

    def _launch_prepare(self):
        main = torch.cuda.current_stream()
        if self._side is None:
            self._side = torch.cuda.Stream()
        # every launch: whatever the main stream produced that the side stream reads (the epoch permutation a milestone's
        # _next_batch rebuilt, kernel-stack tensors) is ordered before it.  Issued BEFORE forward i is enqueued, so the prefetch
        # still overlaps with the forward / backward of micro-batch i.
        self._side.wait_stream(main)
        with torch.cuda.stream(self._side):
            prep = self.core.prepare(self._next_batch())
            ev = torch.cuda.Event()
            ev.record(self._side)
        for t in prep:
            t.record_stream(main)                            # produced on the side stream, consumed (and freed) on the main stream
        return prep, ev

    def _loss(self, batch):
        x2 = self._second(batch)
        return self.core(batch) if x2 is None else self.core(batch, x2)

    def train_step(self):
        """One optimizer step = gradient_accumulate_every micro-batches (one fused pass when `_can_fuse()`, else one forward /
        backward each: DEBLUR:1188-1195) + Adam (+ EMA); returns the mean micro-batch loss as a 0-dim device tensor (no host sync)."""
        if self._graph_req:
            loss = self._graph_train_step()
            if loss is not None:
                return loss
        acc = self.gradient_accumulate_every
        scale = 1.0 / (acc * parallel.world_size())
        total = None
        prefetch = self._can_prefetch()
        fused = self._can_fuse()
        if fused:
            total = self._fused_step(acc, prefetch) * acc
        for i in range(0 if fused else acc):
            if self.sync is not None:
                self.sync.begin()
            if prefetch:
                prep = self._take_prepared(1)                # micro-batch i+1 is degraded under the forward / backward of micro-batch i
                loss = torch.mean(self.core.loss_prepared(prep))
            else:
                loss = torch.mean(self._loss(self._next_batch()))
            if self.sync is not None and i == acc - 1:
                self.sync.arm()
            (loss * scale).backward()
            total = loss.detach() if total is None else total + loss.detach()
        if self.sync is not None:
            self.sync.finish()
        self.opt.step()
        self.opt.zero_grad()
        if self.step % self.update_ema_every == 0:
            self.step_ema()
        return total / acc

    # -- graph mode: the optimizer step replayed as ONE captured graph (opt-in: Trainer(graph=True) / COLDDIFF_GRAPH=1) -------------
    # The 32 x 32 configurations are host-bound: ~700 launches in ~10 ms of device time.  A replayed graph has no launch cost, but it
    # re-runs its kernels with the arguments of the capture pass, so everything a step takes from the host lives in device memory
    # (flat.StepTable: Adam's scalars, the loader's indices, the dropout seeds) and the host part of a step is one small upload:
    #   upload -> [graph-form step: eagerly for the first GRAPH_WARMUP steps, captured once, replayed from then on] -> count, EMA
    # The graph-form step is the fused / single micro-batch step without the side-stream prefetch (one chain of kernels), with
    # cdf_adam_step_dev and the `_sd` dropout entry points; it advances NO host state, so the capture pass (which launches nothing) is
    # not a step and the first replay is the next real step.  The trajectory is bit-identical to the eager Trainer's.
    GRAPH_WARMUP = 3             # eager graph-form steps before a capture: lazily built caches (packed weights, their table, kernel stacks) settle in two

    def graph_state(self):
        """{'mode': 'off' | 'eager' | 'graph', 'reason', 'captures', 'replays'}: 'eager' = graph mode was requested and this Trainer
        runs the ordinary step, for `reason`.  `captures` counts the graphs this Trainer set out to capture (the first one, and one
        per change of something baked into the graph or load(): each warms up again); `replays` the steps a graph ran."""
        gs = self._graph_decide()
        return {k: gs[k] for k in ('mode', 'reason', 'captures', 'replays')}

    def _graph_reason(self):
        """Why the step cannot be captured (the first failed condition), None when it can: declared properties only."""
        if self.device.type != 'cuda':
            return "no HIP device"
        if self.sync is not None:
            return "more than one rank"
        if rt._lib_override is not None:
            return "library override"
        if '_loss' in self.__dict__ or type(self)._loss is not Trainer._loss:
            return "_loss is replaced"
        if 'train_step' in self.__dict__ or type(self).train_step is not Trainer.train_step:
            return "train_step is replaced"
        if type(self)._second is not Trainer._second or type(self)._next_batch is not Trainer._next_batch:
            return "_second / _next_batch is replaced"
        if not (self._can_fuse() or self.gradient_accumulate_every == 1):
            return "gradient accumulation does not fuse (_can_fuse)"
        core = self.core
        if not (hasattr(core, 'prepare') and hasattr(core, 'loss_prepared')):
            return "the core has no two-phase form (prepare / loss_prepared)"
        if not (hasattr(core, 'graph_safe') and core.graph_safe()):
            return "the core's prepare is not graph_safe(): it may read device values on the host"
        if isinstance(self.dl, DeviceLoader):
            if self.dl.rrc:
                return "the random_aug loader draws its parameters on the host"
            if not self.dl.drop_last:
                return "the loader keeps the short last batch (no drop_last)"
        elif not isinstance(self.dl, SyntheticImages):
            return "host DataLoader"
        return None

    def _graph_sig(self):
        """What a captured step has baked in besides addresses; a change warms up and captures again.  (The learning rate is not
        in it: it travels in the uploaded scalars.)"""
        net = self.core._network() if hasattr(self.core, '_network') else self.core
        return (rt.precision, self.batch_size, self.gradient_accumulate_every, self._fuse_off, self.core.training, net.training,
                self.data_image_size, self.image_size, id(self.dl))

    def _graph_set_mode(self, mode, reason):
        self._gs['mode'], self._gs['reason'] = mode, reason
        print(f"graph mode: {mode} ({reason})")

    def _graph_decide(self):
        if self._gs is None:
            self._gs = {'mode': 'off', 'reason': 'not requested', 'captures': 0, 'replays': 0, 'graph': None, 'loss': None, 'warm': 0,
                        'sig': None, 'table': None, 'keep': None}
            if self._graph_req:
                why = self._graph_reason()
                self._graph_set_mode('eager' if why else 'graph', why or 'the step is captured after %d warm-up steps' % self.GRAPH_WARMUP)
                if why is None:
                    self._gs['captures'], self._gs['sig'] = 1, self._graph_sig()
        return self._gs

    def _graph_rewarm(self):
        """Drop the graph and its static buffers; the next GRAPH_WARMUP steps are eager graph-form steps again."""
        gs = self._gs
        if gs['mode'] == 'graph':
            gs['graph'] = gs['loss'] = gs['table'] = gs['keep'] = None
            gs['warm'] = 0
            gs['captures'] += 1

    def _graph_snapshot(self):
        gen = getattr(self.dl, 'gen', None)
        return {'cpu': torch.get_rng_state(), 'cuda': torch.cuda.get_rng_state(self.device), 'gen': None if gen is None else gen.get_state(),
                'dl': {k: getattr(self.dl, k) for k in ('epoch', 'pos', 'order', 'order_host') if hasattr(self.dl, k)},
                'step_count': self.opt.step_count, 'pending': None if self._pending_q is None else list(self._pending_q)}

    def _graph_restore(self, snap):
        torch.set_rng_state(snap['cpu'])
        torch.cuda.set_rng_state(snap['cuda'], self.device)
        if snap['gen'] is not None:
            self.dl.gen.set_state(snap['gen'])
        for k, v in snap['dl'].items():
            setattr(self.dl, k, v)
        self.opt.step_count, self._pending_q = snap['step_count'], snap['pending']

    def _graph_upload(self, table):
        """The host part of a graph-mode step: the loader moves on and hands over this step's indices, the dropout seeds are drawn,
        Adam's scalars are computed for the coming step -- one non-blocking upload."""
        from . import functions as Fn
        idx = None
        if isinstance(self.dl, DeviceLoader):
            idx = torch.cat([self.dl.take_indices() for _ in range(self.gradient_accumulate_every)])
        table.upload(self.opt.host_params(self.opt.step_count + 1), idx, Fn._seed)

    def _graph_form_step(self, table):
        """forward / backward / Adam / zero_grad of one optimizer step with every per-step value read from `table`; advances no host
        state.  Same kernels on the same values as train_step's fused (or single micro-batch) path without the prefetch."""
        from . import functions as Fn
        acc, B = self.gradient_accumulate_every, self.batch_size
        Fn.seed_table, self.opt.hp_dev = table, table.hp
        try:
            preps = []
            for i in range(acc):
                batch = self.dl.batch_of(table.idx[i * B:(i + 1) * B]) if isinstance(self.dl, DeviceLoader) else self._next_batch()
                x2 = self._second(batch)
                preps.append(self.core.prepare(batch) if x2 is None else self.core.prepare(batch, x2))
            if acc > 1:
                prep = tuple(torch.cat(parts) for parts in zip(*preps))
                loss = torch.mean(self.core.loss_prepared(prep))
                (loss * (1.0 / parallel.world_size())).backward()
                total = loss.detach() * acc
            else:
                loss = torch.mean(self.core.loss_prepared(preps[0]))
                (loss * (1.0 / (acc * parallel.world_size()))).backward()
                total = loss.detach()
            table.end_step()
            self.opt.step()
            self.opt.zero_grad()
            return total / acc
        finally:
            Fn.seed_table, self.opt.hp_dev = None, None

    def _graph_capture(self, table):
        """-> (graph, its static loss).  Launches nothing; the loader's generator is registered with the graph (torch registers the
        default one), so a replay advances their offsets as the eager draws would."""
        g = torch.cuda.CUDAGraph()
        gen = getattr(self.dl, 'gen', None)
        if gen is not None:
            g.register_generator_state(gen)
        table.rewind()
        with torch.cuda.graph(g):
            loss = self._graph_form_step(table)
        # The graph has the addresses of cached buffers baked in that the caches REPLACE, not rewrite, when another model steps or
        # samples in between (ops._repack_all builds a new record table for another set of layouts and drops the old one; a layout
        # packed in another arithmetic mode gets new planes): the graph keeps what it was captured with alive.  It writes the packed
        # layouts itself at every replay before it reads them, so it stays consistent whatever the caches point to by then.
        from . import ops
        self._gs['keep'] = (ops._pack_tables.get(self.device), [e.out for e in ops._pack_cache.values()], getattr(self.core, '_taps_cache', None))
        return g, loss

    def _graph_train_step(self):
        """One optimizer step in graph mode; None when this Trainer runs (or from now on has to run) the ordinary step."""
        gs = self._graph_decide()
        if gs['mode'] != 'graph':
            return None
        sig = self._graph_sig()
        if sig != gs['sig']:
            gs['sig'] = sig
            self._graph_rewarm()
            why = self._graph_reason()
            if why is not None:
                self._graph_set_mode('eager', why)
                return None
        if gs['table'] is None:
            n_idx = self.batch_size * self.gradient_accumulate_every if isinstance(self.dl, DeviceLoader) else 0
            gs['table'] = flat.StepTable(self.device, n_idx)
        table = gs['table']
        if gs['graph'] is None and gs['warm'] < self.GRAPH_WARMUP:
            self._graph_upload(table)
            loss = self._graph_form_step(table)
            gs['warm'] += 1
        else:
            if gs['graph'] is None:
                # the capture pass is not a step: the graph-form step advances nothing on the host (loader position and epoch, Adam's
                # step count, the generators, _pending_q stay where they are).  A pass that raises may have: the state of before is
                # put back and the ordinary step takes over for good, from this very step (a capture is never tried twice).
                snap = self._graph_snapshot()
                try:
                    gs['graph'], gs['loss'] = self._graph_capture(table)
                    err = None
                except Exception as e:
                    err = f"the capture raised {type(e).__name__}: {e}"
                rt.bump_weights_epoch()          # the pass marked packed layouts as current without writing them
                if err is not None:
                    self._graph_restore(snap)
                    gs['graph'] = gs['loss'] = gs['table'] = gs['keep'] = None
                    self._graph_set_mode('eager', err)
                    return None
            self._graph_upload(table)
            gs['graph'].replay()
            gs['replays'] += 1
            loss = gs['loss'].clone()
        self.opt.step_count += 1
        rt.bump_weights_epoch()
        if self.step % self.update_ema_every == 0:
            self.step_ema()
        return loss

    def train(self):
        acc_loss = 0
        while self.step < self.train_num_steps:
            u_loss = self.train_step()
            if self.step % 100 == 0 and parallel.rank() == 0 and not self.quiet:
                print(f'{self.step}: {u_loss.item()}')
            acc_loss = acc_loss + u_loss
            if self.step != 0 and self.step % self.save_and_sample_every == 0:
                self._milestone(acc_loss)
                acc_loss = 0
            self.step += 1
        print('training completed')

    def _milestone(self, acc_loss):
        milestone = self.step // self.save_and_sample_every
        if parallel.rank() == 0:                       # sampling and checkpointing stay on one GPU
            og_img = self._sample_source()
            if hasattr(self.ema_core, 'defade_fn'):
                xt, direct_recons, all_images = self.ema_core.sample(batch_size=self.batch_size, faded_recon_sample=og_img)
            else:
                xt, direct_recons, all_images = self.ema_core.sample(batch_size=self.batch_size, img=og_img)
            for name, im in (('og', og_img), ('recon', all_images), ('direct_recons', direct_recons), ('xt', xt)):
                save_image((im + 1) * 0.5, self.results_folder / f'sample-{name}-{milestone}.png', nrow=6)
            mean = float(acc_loss) / (self.save_and_sample_every + 1)
            print(f'Mean of last {self.step}: {mean}')
            self.save()
            if self.step % (self.save_and_sample_every * 100) == 0:
                self.save(self.step)
        parallel.milestone_barrier()


class DemixTrainer(GenEvalMixin, Trainer):
    """Trainer of demixing_diffusion_pytorch (DEMIX:596-775): two image folders; every micro-step mixes a batch of the
    first into a batch of the second, and sampling starts from images of the second."""

    @property
    def _fid_batch(self):                      # DEMIX:818: bs = self.batch_size, seeds = the next batch of the second folder
        return self.batch_size

    def _seed_images(self, bs):
        return self._second()[:bs]

    def __init__(self, diffusion_model, folder1, folder2, *, dataset=None, shuffle=True, num_workers=8, **kw):
        super().__init__(diffusion_model, folder1, dataset=dataset, shuffle=shuffle, num_workers=num_workers, **kw)
        self.pair_noise = False
        self.ds1, self.dl1 = self.ds, self.dl
        self.ds2, self.dl2 = self._make_loader(folder2, dataset, shuffle, num_workers, seed=7654321)

    @staticmethod
    def recipe_for(dataset):                   # DEMIX:636-643: 'train' augments; both datasets convert to RGB (DEMIX:545, 568)
        return (AUG1 if dataset == 'train' else CENTER112).with_rgb()

    def _second(self, batch=None):
        d = next(self.dl2)
        if isinstance(d, (list, tuple)):
            d = d[0]
        return d.to(self.device, non_blocking=True)

    def _sample_source(self):
        return self._second()          # DEMIX:744 draws from the second loader only


class DefadeGenTrainer(GenEvalMixin, Trainer):
    """Trainer of the defading-generation package (DEFGEN:646-810): the second image is one uniform random colour per
    sample and channel, rand(B, 3) - 0.5 spread over the image (DEFGEN:769-773)."""

    @property
    def _fid_batch(self):                      # DEFGEN:880-887: bs = self.batch_size, seeds = one random colour per image
        return self.batch_size

    def _seed_images(self, bs):
        n = self.image_size
        return (torch.rand((bs, 3)) - 0.5)[:, :, None, None].expand(bs, 3, n, n).to(self.device).contiguous()

    def __init__(self, diffusion_model, folder, **kw):
        super().__init__(diffusion_model, folder, **kw)
        self.pair_noise = False

    @staticmethod
    def recipe_for(dataset):                   # DEFGEN:682-687: 'train' augments; both datasets convert to RGB (DEFGEN:591, 614)
        return (AUG1 if dataset == 'train' else CENTER112).with_rgb()

    def _second(self, batch):
        B, C, H, W = batch.shape
        c = torch.rand((B, C), device=batch.device) - 0.5
        return c[:, :, None, None].expand(B, C, H, W).contiguous()


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


# -- the other packages' Trainers: same loop, their own `dataset=` tables and loader options ---------------------------------
class DenoiseTrainer(GenEvalMixin, Trainer):
    """denoising_diffusion_pytorch.py:620-789: `dataset == 'train'` augments, everything else is the centre crop; both datasets
    convert to RGB first (DENOISE:565, 588)."""
    _fid_batch = 128                           # DENOISE:835-839: bs = 128, seeds = N(0, 1) images (128 x 128 upstream: the model's size here)

    def _seed_images(self, bs):
        n = self.image_size
        return torch.randn(bs, 3, n, n).to(self.device)

    def _gen(self, bs, og_img, noise):         # (DENOISE:843: gen_sample has no noise_level in this package)
        return self.ema_core.gen_sample(batch_size=bs, img=og_img)

    @staticmethod
    def recipe_for(dataset):
        return (AUG1 if dataset == 'train' else CENTER112).with_rgb()


class ResolutionTrainer(Trainer):
    """resolution_diffusion_pytorch.py:837-900: 'cifar10' / 'celebA' -> Dataset_Aug1, 'flower' -> Dataset_Aug2 (Resize(s),
    RandomCrop(s, padding=4), mirror), else the centre crop; the DataLoader keeps the short last batch (no drop_last, RESOL:887);
    image_size comes from the model (RESOL:874)."""
    drop_last = False
    image_size_from_model = True

    @staticmethod
    def recipe_for(dataset):
        if dataset in ('cifar10', 'celebA'):
            return AUG1
        if dataset == 'flower':
            return AUG2
        return CENTER112

    def sample_as_a_mean_blur_torch_gmm_ablation(self, torch_gmm, siz=2, ch=3, clusters=10, sample_at=6, noise=0, num_samples=6400, bs=64):
        """RESOL:1117-1182 (this package's form of the method: the GMM is fitted on the `siz` x `siz` area-resampled degradations
        `opt(img, t=sample_at)` of the dataset, its samples are blown up nearest-exact and handed to `gen_sample`)."""
        import torch.nn.functional as F
        from .evaluate import _create_folder
        feats = [F.interpolate(self.ema_core.opt(img, t=sample_at), size=siz, mode='area').flatten(1) for img in self._dataset_batches(100)]
        model = self._fit_gmm(torch_gmm, torch.cat(feats, dim=0), clusters, 100)
        n = self.image_size
        og_x = F.interpolate(model.sample(num_datapoints=num_samples).to(self.device).reshape(num_samples, 3, siz, siz).float(), size=n,
                             mode='nearest-exact')
        xt_folder, out_folder, dr_folder = f'{self.results_folder}_xt', f'{self.results_folder}_out', f'{self.results_folder}_dir_recons'
        for f in (xt_folder, out_folder, dr_folder):
            _create_folder(f)
        cnt = 0
        for j in range(num_samples // bs):
            og_img = og_x[j * bs: j * bs + bs].expand(bs, ch, n, n).float().contiguous()
            xt, direct_recons, all_images = self.ema_core.gen_sample(batch_size=bs, img=og_img, noise_level=noise)
            for i in range(all_images.shape[0]):
                self._save(all_images[i:i + 1], f'{out_folder}/sample-x0-{cnt}.png', nrow=1)
                self._save(xt[i:i + 1], f'{xt_folder}/sample-x0-{cnt}.png', nrow=1)
                self._save(direct_recons[i:i + 1], f'{dr_folder}/sample-x0-{cnt}.png', nrow=1)
                cnt += 1
        return cnt


class DefadeTrainer(Trainer):
    """defading_diffusion_gaussian.py:651-705: 'cifar10' -> DatasetCifar10 (RandomCrop(s, padding=4) on the file's own size, mirror),
    'celebA' -> DatasetCelebA (= Dataset_Aug1), 'celebA_test' -> DatasetCelebATest (1.12x, centre), else Resize(s) + CenterCrop(s);
    always shuffled (DEFADE:695), no `shuffle=` argument upstream (accepted and ignored here)."""
    force_shuffle = True
    image_size_from_model = True

    def __init__(self, diffusion_model, folder, *, train_num_steps=700000, save_and_sample_every=10000, **kw):
        # this package's own defaults (DEFADE:661, 666); its scripts (cifar10_train.py, celebA_train.py) do not pass
        # save_and_sample_every, so a ported script must checkpoint / run the T-step sampler every 10000 steps, not every 1000
        super().__init__(diffusion_model, folder, train_num_steps=train_num_steps, save_and_sample_every=save_and_sample_every, **kw)

    @staticmethod
    def recipe_for(dataset):
        if dataset == 'cifar10':
            return CIFAR_PAD
        if dataset == 'celebA':
            return Recipe('DatasetCelebA', 'sq112', 'random', True)
        if dataset == 'celebA_test':
            return Recipe('DatasetCelebATest', 'sq112', 'center', False)
        return CENTER_SHORT

    # ---- this package's test methods (DEFADE:814-940, 1146-1244): `all_sample` / `sample` take `faded_recon_sample=` here -------------------
    def _frames(self, og_img, extra_path, x0_list, xt_list):
        """og-<extra>.png, sample-<i>-<extra>-x0 / -xt.png and the two GIFs (titles are figure code)"""
        from PIL import Image
        self._save(og_img, str(self.results_folder / f'og-{extra_path}.png'))
        frames_0, frames_t = [], []
        for i in range(len(x0_list)):
            p0, pt = str(self.results_folder / f'sample-{i}-{extra_path}-x0.png'), str(self.results_folder / f'sample-{i}-{extra_path}-xt.png')
            self._save(x0_list[i], p0)
            frames_0.append(p0)
            if i < len(xt_list):
                self._save(xt_list[i], pt)
                frames_t.append(pt)
        for name, frames in ((f'Gif-{extra_path}-x0.gif', frames_0), (f'Gif-{extra_path}-xt.gif', frames_t)):
            ims = [Image.open(f).convert('RGB') for f in frames if os.path.exists(f)]
            if ims:
                ims[0].save(str(self.results_folder / name), save_all=True, append_images=ims[1:], duration=100, loop=0)
        return x0_list, xt_list

    def test_from_data(self, extra_path, s_times=None):                # DEFADE:814-841
        og_img = self._next_batch()
        x0_list, xt_list = self.ema_core.all_sample(batch_size=self.batch_size, faded_recon_sample=og_img, times=s_times)
        return self._frames(og_img, extra_path, x0_list, xt_list)

    def test_with_mixup(self, extra_path):                             # DEFADE:843-883: the mean of two batches as the start
        og_img_1, og_img_2 = self._next_batch(), self._next_batch()
        og_img = (og_img_1 + og_img_2) / 2
        x0_list, xt_list = self.ema_core.all_sample(batch_size=self.batch_size, faded_recon_sample=og_img)
        self._save(og_img_1, str(self.results_folder / f'og1-{extra_path}.png'))
        self._save(og_img_2, str(self.results_folder / f'og2-{extra_path}.png'))
        return self._frames(og_img, extra_path, x0_list, xt_list)

    def test_from_random(self, extra_path):                            # DEFADE:885-920: a batch scaled by 0.9 as the start
        og_img = self._next_batch() * 0.9
        x0_list, xt_list = self.ema_core.all_sample(batch_size=self.batch_size, faded_recon_sample=og_img)
        return self._frames(og_img, extra_path, x0_list, xt_list)

    def controlled_direct_reconstruct(self, extra_path):               # DEFADE:922-940
        torch.manual_seed(0)
        og_img = self._next_batch()
        xt, direct_recons, all_images = self.ema_core.sample(batch_size=self.batch_size, faded_recon_sample=og_img)
        for name, im in (('og', og_img), ('recon', all_images), ('direct_recons', direct_recons), ('xt', xt)):
            self._save(im, str(self.results_folder / f'sample-{name}-{extra_path}.png'))
        self.save()
        return xt, direct_recons, all_images

    def test_from_data_save_results(self, batch_size=100, chunk=32):  # DEFADE:1146-1244: four folders of per-image PNGs
        from .evaluate import _create_folder
        all_samples = torch.cat(list(self._dataset_batches(batch_size)), dim=0)
        folders = [f'{self.results_folder}_{n}/' for n in ('orig', 'blur', 'deblur', 'd_deblur')]
        for f in folders:
            _create_folder(f)
        cnt = 0
        while cnt < all_samples.shape[0]:
            og_img = all_samples[cnt: cnt + chunk].to(self.device).float().contiguous()
            x0_list, xt_list = self.ema_core.all_sample(batch_size=og_img.shape[0], faded_recon_sample=og_img, times=None)
            sets = (og_img.cpu(), xt_list[0].cpu(), x0_list[-1].cpu(), x0_list[0].cpu())
            for i in range(og_img.shape[0]):
                for f, t in zip(folders, sets):
                    self._save(t[i:i + 1].repeat(1, 3 // t.shape[1], 1, 1), f'{f}{cnt + i}.png', nrow=1)
            cnt += og_img.shape[0]
        return cnt
