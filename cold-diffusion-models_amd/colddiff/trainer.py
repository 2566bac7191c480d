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
import gc
import os
from pathlib import Path

import torch
from torch.utils import data

from . import flat, ops, parallel
from . import functions as Fn
from . import runtime as rt
from .data import (AUG1, AUG2, CENTER112, CENTER_SHORT, CIFAR_PAD, JITTER_LDS_CAP, JITTER_STRIDE, RANDOM_AUG, CacheUnfit, Dataset,   # noqa: F401
                   Dataset_Aug1, Dataset_Aug2, DatasetCifar10, DeviceImageCache, DeviceLoader, Recipe, SyntheticImages, center_offset,
                   cycle, draw_random_aug, jitter_lds_bytes, make_grid, resized, save_image, write_grid)      # (re-exported: the input pipeline)
from .evaluate import EvalMixin, GenEvalMixin, _create_folder
from .graphstep import GraphStep


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
                 num_workers=8, device_data=None, graph=None, sample_graph=None):
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
        # sample_graph: the samplers of the EMA core replay one captured reverse step (colddiff/graphsample.py).  None leaves the core's
        # own switch (COLDDIFF_SAMPLE_GRAPH) as it is.
        if sample_graph is not None and hasattr(self.ema_core, '_sg'):
            self.ema_core.sample_graph = bool(sample_graph)
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
            self._gs.rewarm()

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
    # The reference runs `gradient_accumulate_every` micro-batches one after the other, a backward pass on loss_i / accumulate
    # each (DEBLUR:1188-1195) -- a memory measure for 16 GB cards.  With 288 GB of HBM the micro-batches of one optimizer step are
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

    def _prepare_micro(self, batch=None):
        """One micro-batch in the reference's order of draws: the data batch (drawn here unless given), the second image / fresh noise
        (DENOISE:738-742), then forward()'s t (and whatever the degradation draws)."""
        batch = self._next_batch() if batch is None else batch
        x2 = self._second(batch)
        return self.core.prepare(batch) if x2 is None else self.core.prepare(batch, x2)

    def _accumulate(self, groups, n, weight, prepared=True):
        """Forward / backward over `n` groups, drawn from `groups` one at a time: loss_i = the mean loss of a prepared micro-batch (of a data batch
        through `_loss` with prepared=False), backward pass of loss_i * weight, the exchange armed before the last -> the sum of the detached loss_i."""
        total = None
        for i, group in enumerate(groups):
            loss = torch.mean(self.core.loss_prepared(group) if prepared else self._loss(group))
            if self.sync is not None and i == n - 1:
                self.sync.arm()
            (loss * weight).backward()
            total = loss.detach() if total is None else total + loss.detach()
        return total

    def _micro_batches(self, acc, prefetch):
        """The plain loop's micro-batches, drawn one at a time: prepared when prefetched (i + 1 is degraded under i), else data batches."""
        for _ in range(acc):
            if self.sync is not None:
                self.sync.begin()
            yield self._take_prepared(1) if prefetch else self._next_batch()

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

    # The fused pass and the prefetch queue (_take_prepared, _launch_prepare) keep the text they had before `_accumulate` existed: on the
    # host-bound 32 x 32 configuration the eager step through `_accumulate` and a queue object measured above the previous form's
    # slowest run in two sessions (profiles/trainer_step_ab.txt).
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
            prep = loss = None
            self._fuse_off = True
            gc.collect()
            torch.cuda.empty_cache()
            self.opt.zero_grad()
            print(f"fused accumulation of {acc} micro-batches does not fit in device memory: running them one by one from here on")
            return self._accumulate(preps, acc, 1.0 / acc) / acc

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
        loss = self._graph().step() if self._graph_req else None
        if loss is not None:
            # a graph-form step, replayed or not, advanced no host state, and cdf_adam_step_dev left the bump to its caller
            self.opt.step_count += 1
            rt.bump_weights_epoch()
        else:
            acc = self.gradient_accumulate_every
            prefetch = self._can_prefetch()
            if self._can_fuse():
                total = self._fused_step(acc, prefetch) * acc
            else:
                total = self._accumulate(self._micro_batches(acc, prefetch), acc, 1.0 / (acc * parallel.world_size()), prepared=prefetch)
            if self.sync is not None:
                self.sync.finish()
            self.opt.step()
            self.opt.zero_grad()
            loss = total / acc
        if self.step % self.update_ema_every == 0:
            self.step_ema()
        return loss

    # -- graph mode: the optimizer step replayed as ONE captured graph (opt-in: Trainer(graph=True) / COLDDIFF_GRAPH=1) -------------
    # The 32 x 32 configurations are host-bound: ~700 launches in ~10 ms of device time.  colddiff.graphstep.GraphStep has the capture
    # and replay machinery; what a step takes from the host (flat.StepTable: Adam's scalars, the loader's indices, the dropout seeds)
    # is one small upload:
    #   upload -> [graph-form step: eagerly for the first GRAPH_WARMUP steps, captured once, replayed from then on] -> count, EMA
    # The graph-form step is the fused / single micro-batch step without the side-stream prefetch (one chain of kernels), with
    # cdf_adam_step_dev and the `_sd` dropout entry points; it advances NO host state, so the capture pass (which launches nothing) is
    # not a step and the first replay is the next real step.  The trajectory is bit-identical to the eager Trainer's.
    GRAPH_WARMUP = 3             # eager graph-form steps before a capture: lazily built caches (packed weights, their table, kernel stacks) settle in two

    def _graph(self):
        if self._gs is None:                     # (built, and the mode decided, at the first use)
            self._gs = GraphStep(self.GRAPH_WARMUP, reason=self._graph_reason, signature=self._graph_sig, table=self._graph_table,
                                 upload=self._graph_upload, step=self._graph_form_step, snapshot=self._graph_snapshot, capture=self._graph_capture_pass)
        return self._gs

    def graph_state(self):
        """{'mode': 'off' | 'eager' | 'graph', 'reason', 'captures', 'replays'}: 'eager' = graph mode was requested and this Trainer
        runs the ordinary step, for `reason`.  `captures` counts the graphs this Trainer set out to capture (the first one, and one
        per change of something baked into the graph or load(): each warms up again); `replays` the steps a graph ran."""
        return self._graph().state() if self._graph_req else {'mode': 'off', 'reason': 'not requested', 'captures': 0, 'replays': 0}

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

    def _graph_table(self):
        return flat.StepTable(self.device, self.batch_size * self.gradient_accumulate_every if isinstance(self.dl, DeviceLoader) else 0)

    def _graph_snapshot(self):
        """-> restore() of what a capture pass must leave alone: the loader's generator, position and epoch, Adam's step count, _pending_q."""
        gen = getattr(self.dl, 'gen', None)
        gen_state = None if gen is None else gen.get_state()
        state = [(self.dl, k, getattr(self.dl, k)) for k in ('epoch', 'pos', 'order', 'order_host') if hasattr(self.dl, k)]
        state += [(self.opt, 'step_count', self.opt.step_count), (self, '_pending_q', None if self._pending_q is None else list(self._pending_q))]

        def restore():
            if gen is not None:
                gen.set_state(gen_state)
            for obj, k, v in state:
                setattr(obj, k, v)
        return restore

    def _graph_upload(self, table):
        """The host part of a graph-mode step: the loader moves on and hands over this step's indices, the dropout seeds are drawn,
        Adam's scalars are computed for the coming step -- one non-blocking upload."""
        idx = None
        if isinstance(self.dl, DeviceLoader):
            idx = torch.cat([self.dl.take_indices() for _ in range(self.gradient_accumulate_every)])
        table.upload(self.opt.host_params(self.opt.step_count + 1), idx, Fn._seed)

    def _graph_form_step(self, table):
        """train_step's fused (or single micro-batch) pass, Adam and zero_grad without the prefetch, every per-step value read from `table`:
        the batches' indices, the dropout seeds (Fn.seed_table), Adam's scalars (opt.hp_dev); advances no host state."""
        acc, B = self.gradient_accumulate_every, self.batch_size
        Fn.seed_table, self.opt.hp_dev = table, table.hp
        try:
            if isinstance(self.dl, DeviceLoader):
                preps = [self._prepare_micro(self.dl.batch_of(table.idx[i * B:(i + 1) * B])) for i in range(acc)]
            else:
                preps = [self._prepare_micro() for _ in range(acc)]
            group = preps[0] if acc == 1 else tuple(torch.cat(parts) for parts in zip(*preps))
            loss = self._accumulate([group], 1, 1.0 / parallel.world_size())
            table.end_step()
            self.opt.step()
            self.opt.zero_grad()
            return (loss * acc if acc > 1 else loss) / acc       # (as train_step counts a fused pass: `acc` times)
        finally:
            Fn.seed_table, self.opt.hp_dev = None, None

    def _graph_capture(self, table):
        """-> (graph, its static loss).  The loader's generator is registered with the graph."""
        gen = getattr(self.dl, 'gen', None)
        g, loss = self._gs.capture(table, [] if gen is None else [gen])
        # The graph has the addresses of cached buffers baked in that the caches REPLACE, not rewrite, when another model steps or
        # samples in between (ops._repack_all builds a new record table for another set of layouts and drops the old one; a layout
        # packed in another arithmetic mode gets new planes): the graph keeps what it was captured with alive.  It writes the packed
        # layouts itself at every replay before it reads them, so it stays consistent whatever the caches point to by then.
        self._gs.keep = (ops._pack_tables.get(self.device), [e.out for e in ops._pack_cache.values()], getattr(self.core, '_taps_cache', None))
        return g, loss

    def _graph_capture_pass(self, table):
        try:
            return self._graph_capture(table)
        finally:
            rt.bump_weights_epoch()          # the pass, raising or not, marked packed layouts as current without writing them

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


# -- the other packages' Trainers: same loop, their own `dataset=` tables and loader options ---------------------------------
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
