"""Flat parameter / gradient arenas and the fused optimizer tail.

All parameters of a model are re-homed into ONE contiguous fp32 buffer (and their gradients into a
second one), each tensor starting on a 16-byte boundary.  With 288 GB of HBM per MI355X there is no
reason to keep 238 separate allocations: Adam, EMA, zero_grad and the data-parallel gradient
all-reduce each become a single pass (or a few large buckets) over the arena at HBM / xGMI speed.
Replaces torch.optim.Adam + EMA of deblurring_diffusion_pytorch.py:68-81,1117,1200-1204.
"""
import torch

from . import runtime as rt
from .runtime import P


class FlatArena:
    def __init__(self, params):
        self.params = [p for p in params]
        assert self.params, "no parameters"
        dev = self.params[0].device
        self.offsets, off = [], 0
        for p in self.params:
            assert p.device == dev and p.dtype == torch.float32
            self.offsets.append(off)
            off += (p.numel() + 3) // 4 * 4
        self.numel = off
        self.data = torch.zeros(off, device=dev, dtype=torch.float32)
        self.grad = torch.zeros(off, device=dev, dtype=torch.float32)
        self._ptrs = []
        for p, o in zip(self.params, self.offsets):
            n = p.numel()
            self.data[o:o + n].copy_(p.detach().reshape(-1))
            old_grad = p.grad
            p.data = self.data[o:o + n].view(p.shape)
            g = self.grad[o:o + n].view(p.shape)
            if old_grad is not None:
                g.copy_(old_grad)
            p.grad = g
            self._ptrs.append(p.data_ptr())
        rt.bump_weights_epoch()

    def intact(self):
        """False if someone re-homed the parameters (e.g. module.cuda() after flattening)."""
        return all(p.data_ptr() == q and p.grad is not None and p.grad.data_ptr() == self.grad.data_ptr() + 4 * o
                   for p, q, o in zip(self.params, self._ptrs, self.offsets))

    def zero_grad(self):
        rt.lib().cdf_zero(P(self.grad), self.numel * 4, rt.stream(self.grad))

    def slice_of(self, p):
        i = next(k for k, q in enumerate(self.params) if q is p)
        return self.offsets[i], self.offsets[i] + p.numel()


class FusedAdam:
    """torch.optim.Adam(params, lr) with default betas/eps/no weight decay, as one kernel launch."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        self.arena = params if isinstance(params, FlatArena) else FlatArena(list(params))
        self.lr, self.betas, self.eps = lr, betas, eps
        self.exp_avg = torch.zeros_like(self.arena.data)
        self.exp_avg_sq = torch.zeros_like(self.arena.data)
        self.step_count = 0
        self.param_groups = [{"lr": lr, "betas": betas, "eps": eps, "params": self.arena.params}]
        # graph mode only (Trainer(graph=True)): the step's scalars live in this device buffer (StepTable.hp) and step() neither counts
        # nor bumps the weights epoch -- whoever uploads the scalars does, once per real step (a capture pass is not a step)
        self.hp_dev = None

    def host_params(self, step):
        """The six scalars cdf_adam_step computes for `step` with the group's current lr / betas / eps, as 8 floats on the host."""
        g = self.param_groups[0]
        out = torch.empty(8, dtype=torch.float32)
        rt.lib().cdf_adam_params(g["lr"], g["betas"][0], g["betas"][1], g["eps"], step, out.data_ptr())
        return out

    def step(self):
        a = self.arena
        assert a.intact(), "parameters were moved after the optimizer was built (call .cuda() before creating the Trainer)"
        if self.hp_dev is not None:
            rt.lib().cdf_adam_step_dev(P(a.data), P(a.grad), P(self.exp_avg), P(self.exp_avg_sq), a.numel, P(self.hp_dev), rt.stream(a.data))
            return
        self.step_count += 1
        g = self.param_groups[0]
        rt.lib().cdf_adam_step(P(a.data), P(a.grad), P(self.exp_avg), P(self.exp_avg_sq), a.numel, g["lr"], g["betas"][0], g["betas"][1],
                               g["eps"], self.step_count, rt.stream(a.data))
        rt.bump_weights_epoch()

    def zero_grad(self, set_to_none=False):
        self.arena.zero_grad()

    def state_dict(self):
        return {"step": self.step_count, "exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq, "lr": self.lr}

    def load_state_dict(self, sd):
        self.step_count = sd["step"]
        self.exp_avg.copy_(sd["exp_avg"])
        self.exp_avg_sq.copy_(sd["exp_avg_sq"])


class StepTable:
    """The per-step host values of a graph-mode optimizer step in ONE static device buffer of 64-bit words:
    [Adam's scalars: 4 words = 8 floats | loader indices: n_idx | dropout seeds: up to MAX_SEEDS].  A captured graph has the
    buffer's addresses baked in; `upload` rewrites its contents before every step with one pinned, non-blocking copy (stream order
    puts it behind the previous step's kernels, the caching host allocator keeps the staging block alive until the copy ran).

    Dropout seeds: the blocks `take()` one slot each, in call order (the backward reuses its forward's slot).  How many a step takes is
    not declared anywhere, so the first step after `reset_seeds()` runs in draw mode: take() draws the seed on the host as the eager
    block does and writes it into its slot at once; the count is known from then on and `upload` carries that many seeds, drawn from
    the same generator in the same order and number."""
    MAX_SEEDS = 1024

    def __init__(self, device, n_idx):
        self.n_idx = n_idx
        self.dev = torch.zeros(4 + n_idx + self.MAX_SEEDS, dtype=torch.int64, device=device)
        self.hp = self.dev[:4].view(torch.float32)
        self.idx = self.dev[4:4 + n_idx]
        self.seeds = self.dev[4 + n_idx:]
        assert self.hp.data_ptr() % 16 == 0
        self.n_seeds = None          # None: not counted yet (draw mode)
        self.taken = 0

    def reset_seeds(self):
        self.n_seeds, self.taken = None, 0

    def upload(self, hp, idx, draw_seed):
        n = 4 + self.n_idx + (self.n_seeds or 0)
        host = torch.empty(n, dtype=torch.int64, pin_memory=True)
        host[:4].view(torch.float32).copy_(hp)
        if self.n_idx:
            host[4:4 + self.n_idx].copy_(idx)
        if self.n_seeds:
            host[4 + self.n_idx:].copy_(torch.tensor([draw_seed() for _ in range(self.n_seeds)], dtype=torch.int64))
        self.dev[:n].copy_(host, non_blocking=True)
        self.taken = 0
        self._draw = draw_seed if self.n_seeds is None else None

    def rewind(self):
        """Before a capture pass: the slots are handed out again from the first one, and nothing is drawn or written."""
        assert self.n_seeds is not None
        self.taken, self._draw = 0, None

    def take(self):
        k = self.taken
        assert k < self.MAX_SEEDS, "more dropout layers than StepTable.MAX_SEEDS"
        self.taken = k + 1
        slot = self.seeds[k:k + 1]
        if self._draw is not None:
            slot.copy_(torch.tensor([self._draw()], dtype=torch.int64))
        else:
            assert k < self.n_seeds, "this step takes more dropout seeds than the step that was counted"
        return slot

    def end_step(self):
        """After a step's forward: fix the count (draw mode) or check it."""
        if self.n_seeds is None:
            self.n_seeds = self.taken
        assert self.taken == self.n_seeds, f"{self.taken} dropout seeds taken, {self.n_seeds} uploaded"
        self._draw = None


def ema_update(ema_arena, model_arena, beta):
    """EMA.update_model_average: ma = ma*beta + (1-beta)*p over every parameter (DEBLUR:73-81)."""
    assert ema_arena.numel == model_arena.numel
    rt.lib().cdf_ema_update(P(ema_arena.data), P(model_arena.data), ema_arena.numel, beta, rt.stream(ema_arena.data))
    rt.bump_weights_epoch()
