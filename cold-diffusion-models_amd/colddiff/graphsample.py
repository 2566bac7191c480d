"""Sampler graph mode (opt-in: `core.sample_graph = True`, `graph=True` on a sampler call, COLDDIFF_SAMPLE_GRAPH=1): ONE reverse step
captured as a graph and replayed for the T steps of a sampler call.

A reverse step is `x_t -> (x0 estimate, x_{t-1})`: one call of the network and one degradation launch, the same few hundred launches as
a training forward with a third of the device work behind each.  graphstep.GraphStep has the capture / replay and snapshot / restore
machinery; what is specific to a sampler:

  step table    `StepTable.dev`, static int64 words [step: B | step-1: B | slot: 1], filled ONCE per sampler call on the device.  The
                network and the chain kernels read their rows as the per-image `t` (`chain_hi()` reads t[b]; a row of -1 is the
                identity, as a chain of zero steps is), cdf_noise_step_dev / cdf_blend_step_dev read word 0, cdf_traj_put reads `slot`.
                The LAST node of the step, cdf_steps_advance, moves every word down by one (floor -1): nothing else moves the counter
                between replays, and the host uploads nothing per step.
  static state  `cur` (x_t; the step's result is copied back into it), the call's fixed second images / offsets (`st`), and for
                all_sample two slabs [T, B, C, H, W] written at row `step`.
  a call        with no valid graph: SAMPLE_GRAPH_WARMUP eager graph-form steps (real steps), one capture pass (launches nothing,
                advances nothing), replays for the rest; a later call with the same signature replays every step.  A call of
                t <= warm-up + 1 steps never captures: it runs the ordinary loop.
The trajectory is bit-identical to the eager sampler's: the same kernels on the same values, `t` read from the table instead of
passed by value.  noise_level draws, the forward process, eval() / train() stay outside, in the callers' order.

`SampleGraphMixin._walk` is the reverse loop of every sampler, captured or not: it tries `SampleGraph.reverse` where the caller
describes the call for it, and runs what is left (all of it, by default) as the ordinary loop, with the core's `_update` as the
step rule of both."""
import os
import weakref

import torch

from . import degrade as D
from . import ops, parallel
from . import runtime as rt
from .graphstep import GraphStep

SAMPLE_GRAPH_WARMUP = 2       # eager graph-form steps before the capture: packed weights and the other lazily built caches settle in one
_OFF = {'mode': 'off', 'reason': 'not requested', 'captures': 0, 'replays': 0}


class StepTable:
    """The static buffers of one captured reverse step (see the module docstring).  `rows` > 0 allocates the two trajectory slabs."""

    def __init__(self, img, st, rows):
        dev, B = img.device, img.shape[0]
        self.B = B
        self.dev = torch.zeros(2 * B + 1, dtype=torch.int64, device=dev)
        self.step, self.prev, self.slot = self.dev[:B], self.dev[B:2 * B], self.dev[2 * B:]
        self.zero = torch.zeros(1, dtype=torch.int64, device=dev)          # the slot of `cur`, a slab of one row
        self.cur = torch.empty(img.shape, dtype=torch.float32, device=dev)
        self.st = {k: torch.empty(v.shape, dtype=v.dtype, device=dev) for k, v in st.items()}
        self.slabs = tuple(torch.empty((rows,) + tuple(img.shape), dtype=torch.float32, device=dev) for _ in range(2)) if rows else None
        self.none = torch.empty(0, device=dev)                             # GraphStep's per-step result: the outputs stay in the table

    def load(self, img, st, t):
        """Once per sampler call, all on the device: x_t, the fixed inputs, the counter at step t - 1."""
        self.cur.copy_(img)
        for k, v in st.items():
            self.st[k].copy_(v)
        self.step.fill_(t - 1)
        self.prev.fill_(t - 2)
        self.slot.fill_(t - 1)

    def rewind(self):             # (GraphStep.capture: nothing is handed out per step here)
        pass


class SampleGraph:
    """The sampler graph of one core: at most one captured step, keyed by `signature`."""

    def __init__(self, core):
        # (a weak reference: core -> SampleGraph -> core would be a cycle, and a core nobody refers to any more would keep its graph
        #  and the graph's pool until the cyclic collector runs)
        self._core, self.gs, self.tb, self.why = weakref.ref(core), None, None, None
        self._sig = self._call = self._fn = self._put = None
        self.x0 = None

    @property
    def core(self):
        return self._core()

    def __deepcopy__(self, memo):              # (copy.deepcopy(core), as the Trainer's EMA copy is made: the copy captures its own)
        return SampleGraph(memo.get(id(self.core), self.core))

    # -- what the core reports -------------------------------------------------------------------------------------------
    def state(self):
        gs = self.gs
        n = {'captures': gs.captures if gs else 0, 'replays': gs.replays if gs else 0}
        if self.why is not None:
            return {'mode': 'eager', 'reason': self.why, **n}
        if gs is None:
            return {'mode': 'graph', 'reason': 'captured by the first call of more than %d steps' % (SAMPLE_GRAPH_WARMUP + 1), **n}
        return gs.state()

    def drop(self):
        self.gs = self.tb = self.x0 = self._call = self._fn = None

    # -- eligibility and signature ---------------------------------------------------------------------------------------
    def declared(self, img, batch_size):
        """Why no sampler of this process / this call can be captured (the core's own reasons come from the caller)."""
        if rt._lib_override is not None:
            return "library override"
        if not img.is_cuda:
            return "no HIP device"
        if parallel.world_size() > 1:
            return "more than one rank"
        if batch_size != img.shape[0]:
            return "batch_size differs from the image batch (the step vector is broadcast)"
        net = self.core._network()
        if net.training and any(isinstance(m, torch.nn.Dropout) and m.p > 0 for m in net.modules()):
            # (the resolution and defading samplers do not call eval(), as upstream does not)
            return "the network is in training mode: its dropout layers draw a seed on the host at every step"
        return None

    def signature(self, variant, img, st, rows):
        """What a captured step has baked in besides the addresses of its own static buffers: a change drops the graph."""
        core = self.core
        net = core._network()
        tensors = list(core.parameters()) + list(core.buffers()) + [v for v in (getattr(core, 'fade_kernels', None),) if v is not None]
        return (type(core), variant, tuple(getattr(core, k, None) for k in ('sampling_routine', 'train_routine', 'blur_routine', 'resolution_routine',
                                                                           'fade_routine', 'discrete', 'num_timesteps')),
                id(net), net.training, tuple(img.shape), str(img.device), rt.precision, rt.MODEL_SAMPLE_PRECISION, rows,
                tuple((k, tuple(v.shape), v.dtype) for k, v in st.items()),
                # ... and what ops.packed keys the packed weights on: a step that rewrote the weights has to pack them again, eagerly
                rt.weights_epoch, tuple((p.data_ptr(), p._version) for p in tensors))

    # -- GraphStep's callables -------------------------------------------------------------------------------------------
    def _table(self):
        img, st, t, rows = self._call
        self.tb = StepTable(img, st, rows)
        return self.tb

    def _upload(self, table):
        if self._call is not None:                 # the first step of a call; from then on the counter moves on the device
            img, st, t, rows = self._call
            table.load(img, st, t)
            self._call = None

    def _step(self, table):
        """The graph-form step: cur -> (x0 estimate, next x_t) -> cur, on one stream; advances nothing on the host."""
        x0, nxt = self._fn(table.cur, table)
        if self._put is not None:
            D.traj_put(table.slabs[0], x0, table.slot)
            D.traj_put(table.slabs[1], nxt if self._put == 'next' else table.cur, table.slot)
        D.traj_put(table.cur.unsqueeze(0), nxt, table.zero)
        D.steps_advance(table.dev, -1, -1)
        self.x0 = x0
        return table.none

    def _capture(self, table):
        g, res = self.gs.capture(table)
        core, net = self.core, self.core._network()
        # the addresses the graph has baked in of buffers that their caches REPLACE when something else runs in between
        self.gs.keep = (ops._pack_tables.get(table.dev.device), [e.out for e in ops._pack_cache.values()], getattr(core, '_taps_cache', None),
                        getattr(core, 'fade_kernels', None), dict(getattr(core, '_sizes_cache', None) or {}),
                        [m.__dict__.get('_tb_cache') for m in net.modules()], self.x0)
        return g, res

    # -- a sampler call --------------------------------------------------------------------------------------------------
    def reverse(self, variant, fn, img, t, batch_size, st=None, put=None, why=None):
        """`t` reverse steps from x_t = img, `fn(cur, table) -> (x0, next)` being the core's step with every `t` read from the table.
        -> None: run the ordinary loop (state() says why), or (direct_recons, img, steps left, (x0 rows, x_t rows) | None): `steps
        left` > 0 only after a capture pass that raised -- the ordinary loop finishes the call from there."""
        why = why or self.declared(img, batch_size)
        if why is None and put is not None and t > self.core.num_timesteps:
            why = "more steps than num_timesteps"
        self.why = why
        if why is not None:
            return None
        gs = self.gs
        if gs is not None and gs.mode != 'graph':               # a capture pass raised: never tried twice
            return None
        st = {k: v for k, v in (st or {}).items() if v is not None}
        rows = self.core.num_timesteps if put is not None else 0
        sig = self.signature(variant, img, st, rows)
        if t <= SAMPLE_GRAPH_WARMUP + 1 and (gs is None or gs.graph is None or gs.sig != sig):
            return None
        self._sig, self._call, self._fn, self._put = sig, (img, st, t, rows), fn, put
        if gs is None:
            gs = self.gs = GraphStep(SAMPLE_GRAPH_WARMUP, reason=lambda: None, signature=lambda: self._sig, table=self._table,
                                     upload=self._upload, step=self._step, snapshot=lambda: (lambda: None), capture=self._capture)
        direct_recons, done = None, 0
        while done < t:
            if gs.step() is None:
                break
            done += 1
            if done == 1:
                direct_recons = self.x0.clone() if gs.graph is not None else self.x0
        tb = self.tb
        self._call = self._fn = None               # (the step's closure refers to the core; a replay does not need it)
        lists = None
        if put is not None:
            lists = tuple(list(s[t - done:t].flip(0).unbind(0)) for s in tb.slabs)      # iteration k wrote row t - 1 - k
        return direct_recons, tb.cur.clone(), t - done, lists


class SampleGraphMixin:
    """The switch and the public surface on a core: `sample_graph` (class attribute, default COLDDIFF_SAMPLE_GRAPH == "1"),
    `sample_graph_state()`, `drop_sample_graph()`."""
    sample_graph = os.environ.get("COLDDIFF_SAMPLE_GRAPH") == "1"
    _sample_graph = None

    def _sg(self, graph):
        """The core's SampleGraph when this call asks for graph mode (`graph`; None reads self.sample_graph), else None."""
        if not (self.sample_graph if graph is None else graph):
            return None
        if self._sample_graph is None:
            self.__dict__['_sample_graph'] = SampleGraph(self)
        return self._sample_graph

    def _sg_eager(self, graph, why):
        """A sampler that is not captured: runs as it is, and the state says why."""
        sg = self._sg(graph)
        if sg is not None:
            sg.why = why

    def _walk(self, img, n, batch_size, update, collect=None, graph=None, variant=None, st=None, put=None, why=None):
        """THE reverse walk of every sampler: `n` reverse steps from x_t = img -> (first x0 estimate, x_{t-n}).
        `update(x_t, x0, t, tb) -> x_{t-1}` is the core's step rule in both of its forms: the ordinary loop hands it the host step
        count `t` (tb None), a captured step the StepTable `tb` (t None).  `collect(x0, x_t)` sees every step; `put` = 'next' hands it
        the step's result in place of its input.  `variant` names the call for SampleGraph.reverse (with `st`, `put`, `why`: its
        arguments; `why` may be a callable, asked only in graph mode); a sampler that is never captured passes none and states its
        reason through _sg_eager."""
        net, direct_recons = self._network(), None
        sg = self._sg(graph) if variant is not None else None
        if sg is not None:
            def step(cur, tb):
                x = net(cur, tb.step)
                return x, update(cur, x, None, tb)
            done = sg.reverse(variant, step, img, n, batch_size, st=st, put=put, why=why() if callable(why) else why)
            if done is not None:
                direct_recons, img, n, lists = done
                for x, x_t in zip(*(lists or ((), ()))):
                    collect(x, x_t)
        while n:
            x = net(img, torch.full((batch_size,), n - 1, dtype=torch.long, device=img.device))
            if direct_recons is None:
                direct_recons = x
            nxt = update(img, x, n, None)
            if collect is not None:
                collect(x, nxt if put == 'next' else img)
            img, n = nxt, n - 1
        return direct_recons, img

    def sample_graph_state(self):
        """{'mode': 'off' | 'eager' | 'graph', 'reason', 'captures', 'replays'}: 'eager' = graph mode was requested and the last
        sampler call ran the ordinary loop, for `reason`; `captures` counts the graphs set out to capture, `replays` the steps a graph ran."""
        sg = self._sample_graph
        return dict(_OFF) if sg is None else sg.state()

    def drop_sample_graph(self):
        """Free the captured step, its static buffers and its pool; the next graph-mode call warms up and captures again."""
        if self._sample_graph is not None:
            self._sample_graph.drop()
