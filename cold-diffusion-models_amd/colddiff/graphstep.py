"""`GraphStep` -- a step of device work replayed as ONE captured graph: upload -> [graph-form step: eagerly for the first `warmup` steps,
captured once, replayed from then on].  Everything the step takes from the host lives in a flat.StepTable; the step advances NO host state, so
the capture pass (which launches nothing) is not a step and the first replay is the next real step."""
import gc

import torch


class GraphStep:
    # What is specific to the user (colddiff.trainer.Trainer: the optimizer step) comes in as callables:
    #   reason()        why the step cannot be captured (declared properties only), None when it can
    #   signature()     what a captured step has baked in besides addresses; a change warms up and captures again
    #   table()         a fresh flat.StepTable of the user's size
    #   upload(table)   the host part of a step: advance the host state, hand this step's values to `table`
    #   step(table)     the graph-form step -> its result (a device tensor); every per-step value is read from `table`
    #   snapshot()      -> restore(): puts back the host state a capture pass that raised may have moved (the generators are kept here)
    #   capture(table)  -> (graph, static result); default `GraphStep.capture`
    def __init__(self, warmup, *, reason, signature, table, upload, step, snapshot, capture=None):
        self.warmup, self._reason, self._signature, self._table, self._upload, self._step = warmup, reason, signature, table, upload, step
        self._snapshot, self._capture = snapshot, capture or self.capture
        self.captures = self.replays = self.warm = 0
        self.sig = self.table = self.graph = self.loss = self.mode = None
        self.keep = None             # what the graph has baked the addresses of and its user may replace: set by the user's capture
        why = reason()
        self.set_mode('eager' if why else 'graph', why or 'the step is captured after %d warm-up steps' % warmup)
        if why is None:
            self.captures, self.sig = 1, signature()

    def __getitem__(self, name):                 # gs['table'], gs['graph'], ...: as the dict this class replaced was read
        return getattr(self, name)

    def state(self):
        return {'mode': self.mode, 'reason': self.reason, 'captures': self.captures, 'replays': self.replays}

    def set_mode(self, mode, reason):
        self.mode, self.reason = mode, reason
        print(f"graph mode: {mode} ({reason})")

    def rewarm(self):
        """Drop the graph and its static buffers; the next `warmup` steps are eager graph-form steps again."""
        if self.mode == 'graph':
            self.graph = self.loss = self.table = self.keep = None
            self.warm, self.captures = 0, self.captures + 1

    def snapshot(self):
        return torch.get_rng_state(), torch.cuda.get_rng_state(self.table.dev.device), self._snapshot()

    def restore(self, snap):
        torch.set_rng_state(snap[0])
        torch.cuda.set_rng_state(snap[1], self.table.dev.device)
        snap[2]()

    def capture(self, table, generators=()):
        """-> (graph, its static result).  Launches nothing; a replay advances `generators` (and the default one) as eager draws would."""
        g = torch.cuda.CUDAGraph()
        for gen in generators:
            g.register_generator_state(gen)
        table.rewind()
        # A dead reference cycle that holds another captured graph (a core or Trainer nobody refers to any more) is destroyed when the
        # cyclic collector gets to it.  Inside a capture pass that is a prohibited call and ends the process: collect before the pass,
        # and keep the collector out of it (torch.cuda.graph does neither).
        gc.collect()
        was_enabled = gc.isenabled()
        gc.disable()
        try:
            with torch.cuda.graph(g):
                loss = self._step(table)
        finally:
            if was_enabled:
                gc.enable()
        return g, loss

    def step(self):
        """One step in graph mode -> its result; None when the user runs (or from now on has to run) the ordinary step."""
        if self.mode != 'graph':
            return None
        sig = self._signature()
        if sig != self.sig:
            self.sig = sig
            self.rewarm()
            why = self._reason()
            if why is not None:
                self.set_mode('eager', why)
                return None
        if self.table is None:
            self.table = self._table()
        if self.graph is None and self.warm < self.warmup:
            self._upload(self.table)
            loss = self._step(self.table)
            self.warm += 1
            return loss
        if self.graph is None:
            # the capture pass is not a step: the graph-form step advances nothing on the host.  A pass that raises may have: the state
            # of before is put back and the ordinary step takes over for good, from this very step (a capture is never tried twice).
            snap = self.snapshot()
            try:
                self.graph, self.loss = self._capture(self.table)
            except Exception as e:
                self.restore(snap)
                self.graph = self.loss = self.table = self.keep = None
                self.set_mode('eager', f"the capture raised {type(e).__name__}: {e}")
                return None
        self._upload(self.table)
        self.graph.replay()
        self.replays += 1
        return self.loss.clone()
