"""Every weight-derived cache of the Python layer: the warm state must equal a cold start.

The C API writes weights through raw pointers (cdf_adam_step, cdf_adam_step_dev, cdf_ema_update, a graph replay, a broadcast) and
`Tensor._version` never moves, so a cached copy of the weights is current only if the hand-placed `rt.bump_weights_epoch()` calls and
the conditions of `ops.packed` / `ops._repack_all` are right.  These tests walk that state machine with seeded random event sequences
(`random.Random(seed)`, the seeds are the lists below; a failing sequence prints its last 20 events) on both backends (fixture `mbe`:
the simulator on CPU tensors, and gpu-marked the MI355X).

1. Layout level (`test_layout_*`): seven small ragged parameters reach every kind `_pack_geom` knows plus `cin4` (22 slots).  Events:
   request a subset of the slots | rewrite all or one parameter behind torch's back (NumPy view on the simulator, cdf_axpby or
   cdf_adam_step on the raw pointer on the MI355X) + bump | an in-place torch write | set_precision | a bare bump | re-home
   (`p.data = p.data.clone()`) | drop and recreate.  Every returned buffer is compared bit for bit, pad columns included (zero: the
   stated contract of the pack kernels), with weight_cache_ref.layout_ref: the documented layout restated with permute / reshape on
   the current values, hi / lo planes from test_kernels._split (held against torch's bfloat16 rounding), lo None in "bf16" mode.
   Structure: the cache holds exactly the live slots over 50 epochs and the device table is rebuilt only when its signature changes;
   "rewrite all + bump" refreshes with exactly one cdf_pack_many and no cdf_pack_weight* launch; a single layout is re-packed alone;
   a layout skipped for n epochs is not rewritten after its first idle epoch and is right on its next use; a precision toggle
   re-packs the shared slot of a kind without `_sp` (what runtime.precision_scope documents).
2. Network level (`test_network_*`): Unet(dim 16 | 64, (1, 2)) at 8 x 8 and the small Model of test_graph_train.py at 16 x 16, B = 2,
   each with an EMA twin, both in FlatArenas, FusedAdam at lr 0.05.  Events: train step | forward + backward without a step |
   flat.ema_update(beta 0.5) | Trainer.reset_parameters' arena copy | load_state_dict of scaled weights into either net | a mode
   change | no_grad evaluation of either net | a second, unrelated net stepping on the same device.  After each evaluation
   (a) the output is within the project's forward bound of oracle.cold_oracle at the net's current state_dict (1e-4 max-abs in f32 /
   bf16x3 as in test_unet_golden, runtime.BF16_TOLERANCE["forward_max_abs"] in bf16), and (b) it is bit-equal to the same call from
   a cold start (weight_cache_ref.cold_start empties _pack_cache, _pack_tables, every _tb_cache and _taps_cache, and puts the warm
   state back afterwards so that the sequence keeps its history).
   Those bounds are absolute ones for outputs at image scale, and one Adam step at lr 0.05 multiplies the output by ~60 (|y|max 0.3
   -> 19; the bf16 error is ~0.5 % of |y|max throughout).  So after every event that moved a net its LAST layer is rescaled, by an
   in-place torch write, to |oracle output|max = 1 (Twin.to_image_scale); every other parameter keeps its version counter and depends
   on the weights epoch alone.  Worst forward error / bound over all network tests: f32 / bf16x3 0.37 (3.7e-5), bf16 0.53 on the
   simulator, 0.41 and 0.48 on the MI355X.
   For (a) to mean anything a forward through weights one event old must miss the bound by a wide margin:
   test_network_stale_weights_break_the_bound asserts, on the oracle alone, at least 10 x the widest (bf16) bound for a first move of
   each kind; the sequences print the margin of every move and assert 10 x the f32 / bf16x3 bound (later Adam steps are smaller as the
   momentum settles and an EMA half-step shrinks with the distance: 0.57 x the bf16 bound = 114 x the f32 bound is the smallest seen,
   40 .. 75 x the bf16 bound is typical; the first moves of the premise test give 33 x and more).  So in bf16 mode (a) alone could
   pass on a layout one LATE event stale: there (b), the bit-for-bit cold start, is the guard, and (a) guards the first moves.
   test_network_every_writer_between_two_evaluations puts each writer directly between two evaluations of the net it writes: the
   random sequences reach `evaluate, write, evaluate` inside one epoch only by chance (seeded fault 4 went through all of them).
   TimeBiasAll (two forwards, backwards in reverse order) and the blur taps (after .to(device), load_state_dict and a re-homed
   weight) have a direct case each.
3. Graph mode (`test_graph_mode_*`, gpu only): a graph-mode Trainer (lr 1e-3: its own L1 loss keeps the output at image scale) replays
   three steps, the training and the EMA net are evaluated eagerly in the captured mode and under precision_scope("f32") with (a)
   and (b), two more replays, a second Trainer steps, evaluations, a last replay; every weight and buffer of both models is bit-equal
   to an eager Trainer fed the same events, and so are the arenas whole (parameters, Adam's moments, EMA: alignment gaps included);
   the gradient arena is all zero bits after the last step.  cdf_zero under capture has a bounds case of its own.

Left out: the folded extractor weights of inception.py (keyed on ptr and version, written through torch only; its forms have
test_inception_forms.py) -- cold_start does not empty that cache and no case here reads it.

Not as the plan had it: a layout skipped for n epochs IS rewritten once, in its first idle epoch, because the one-launch refresh
goes by what the previous epoch used; it is left alone from then on.  test_layout_skipped_for_n_epochs pins exactly that.

Seeded faults (simulator, on a scratch copy, each alone; none is committed).  "seq" = test_layout_sequences (6) / test_network_sequences
(7).  Of the older Python-layer modules (test_modules, test_poison, test_block_routes, test_bf16_storage, test_graph_train,
test_decolor_trainer, test_snow_trainer) the tests that failed too are named:
    1 _repack_all skips its last entry, advances its epoch   layout seq 6/6, raw_and_torch, cache_size_and_table, many_refreshed, skipped x 2,
                                                             every_writer x 3, network seq 3/7; older: none (also none in test_kernels*.py)
    2 packed ignores `precision`                             layout seq 2/6, many_refreshed, precision_toggle, network seq 5/7; older: none
    3 packed ignores `_version`                              layout seq 2/6, raw_and_torch, every_writer x 3, network seq 1/7; older: none
    4 flat.ema_update without its bump                       every_writer x 3 (no sequence: see above); older: none
    5 individual path reuses hit.out across a want_lo change layout seq 6/6, many_refreshed, single_layout x 2, precision_toggle, network seq 7/7;
                                                             older: none
    6 TimeBiasAll's key without weights_epoch                every_writer x 3, network seq 5/7 (both Unets);
                                                             older: test_modules test_trainer_matches_oracle, test_fused_accumulation_matches_oracle_micro_steps,
                                                             test_decolor_trainer test_optimizer_steps_match_the_cpu_restatement
    7 a kv_* geometry with off = 0                           layout seq 6/6 and 7 more layout tests, every_writer x 3, network seq 6/7; 
                                                             older: 52 tests of the seven modules (every net with LinearAttention: goldens,
                                                             block routes, bf16 stream, trainers)
"""
import contextlib
import gc
import random
import types

import pytest
import torch

import weight_cache_ref as R
from oracle import cold_oracle as O
from test_modules import mbe, quiet  # noqa: F401  (mbe: the fixture)

LAYOUT_SEEDS = [101, 102, 103, 104, 105, 106]
LAYOUT_EVENTS = 60
MODES = ("bf16x3", "bf16", "f32")

# name -> (shape, kinds): every kind of ops._pack_geom, plus cin4
PARAMS = {
    "conv3": ((40, 24, 3, 3), ("conv_fwd", "conv_dgrad", "conv_fwd_sp", "conv_dgrad_sp")),
    "conv1": ((24, 40, 1, 1), ("conv_fwd", "conv_dgrad", "conv_fwd_sp", "conv_dgrad_sp")),
    "convT": ((24, 40, 4, 4), ("convT_fwd", "convT_dgrad", "convT_fwd_sp", "convT_dgrad_sp")),
    "to_qkv": ((96, 24, 1, 1), ("kv_fwd", "kv_dgrad", "kv_fwd_sp", "kv_dgrad_sp", "conv_fwd")),      # HD = 32: off = 32 * 24
    "dw": ((24, 1, 7, 7), ("dw",)),
    "lin": ((40, 24), ("lin_fwd",)),
    "cin": ((8, 3, 3, 3), ("cin4", "cin_z", "conv_fwd")),
}
SLOTS = [(n, k) for n, (_, kinds) in PARAMS.items() for k in kinds]


@pytest.fixture(autouse=True)
def _own_caches():
    """Each test starts cold, in the default mode, and leaves nothing of its own behind."""
    from colddiff import runtime as rt
    gc.collect()
    saved = rt.precision
    R.empty_caches()
    yield
    rt.set_precision(saved)
    R.empty_caches()


def _sync(mbe):
    if mbe.kind == "hip":
        torch.cuda.synchronize()


class Weights:
    """The parameters of the layout-level tests and the ways to write them."""

    def __init__(self, mbe, seed):
        self.mbe = mbe
        self.gen = torch.Generator().manual_seed(seed)
        self.p = {n: self._new(n) for n in PARAMS}

    def _values(self, name):
        return torch.randn(PARAMS[name][0], generator=self.gen) * 0.5

    def _new(self, name):
        return torch.nn.Parameter(self.mbe.to(self._values(name)).contiguous())

    def recreate(self, name):
        del self.p[name]
        self.p[name] = self._new(name)

    def raw_write(self, name, how="axpby"):
        """New values through the raw pointer: Tensor._version does not move.  Every write stays inside the parameter's own numel()."""
        from colddiff import runtime as rt
        p = self.p[name]
        v0, n = p._version, p.numel()
        assert p.is_contiguous()
        if self.mbe.kind == "emu":
            p.detach().numpy()[...] = self._values(name).numpy()
        elif how == "axpby":
            src = self.mbe.to(self._values(name)).contiguous()
            rt.lib().cdf_axpby(p.data_ptr(), n, src.data_ptr(), n, 1, n, 0.0, 1.0, rt.stream(p))
            torch.cuda.synchronize()
        else:                                                # one Adam step of the parameter as its own arena: moves every element by ~lr
            g, m, v = (self.mbe.to(t).contiguous() for t in (self._values(name), torch.zeros(n), torch.zeros(n)))
            rt.lib().cdf_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, 0.05, 0.9, 0.999, 1e-8, 1, rt.stream(p))
            torch.cuda.synchronize()
        assert p._version == v0                              # (the caller bumps the epoch: that is the rule under test)

    def torch_write(self, name):
        with torch.no_grad():
            self.p[name].mul_(0.75).add_(self.mbe.to(self._values(name)), alpha=0.25)

    def rehome(self, name):
        p = self.p[name]
        old = p.data_ptr()
        p.data = p.data.clone()
        assert p.data_ptr() != old


def _request(mbe, W, slots):
    """ops.packed of each slot, each held against the reference at the parameter's current values."""
    from colddiff import ops, runtime as rt
    for name, kind in slots:
        got = ops.packed(W.p[name], kind)
        _sync(mbe)
        want = R.layout_ref(W.p[name], kind, rt.precision, mbe.device)
        if kind in R.SP_KINDS:
            assert isinstance(got, tuple) and (got[1] is None) == (rt.precision != "bf16x3"), (name, kind, rt.precision)
        assert R.same_layout(got, want), (name, kind, rt.precision, rt.weights_epoch)


def _cache_is_live_slots(W, requested):
    """The cache holds one entry per requested slot of a LIVE parameter and nothing else."""
    from colddiff import ops
    live = {(id(W.p[n]), k) for n, k in requested}
    assert set(ops._pack_cache) == live, (len(ops._pack_cache), len(live))
    assert all(e.ref() is not None for e in ops._pack_cache.values())


@pytest.mark.parametrize("seed", LAYOUT_SEEDS)
def test_layout_sequences(mbe, seed):
    from colddiff import runtime as rt
    rng = random.Random(seed)
    W = Weights(mbe, seed)
    requested = set()
    with R.Trace() as log:
        for _ in range(LAYOUT_EVENTS):
            ev = rng.choice(["request"] * 5 + ["raw_all", "raw_one", "raw_one", "torch", "precision", "precision", "bump", "rehome", "recreate"])
            if ev == "request":
                slots = rng.sample(SLOTS, rng.randint(1, len(SLOTS)))
                log("request", rt.precision, "epoch", rt.weights_epoch, slots)
                _request(mbe, W, slots)
                requested |= set(slots)
                _cache_is_live_slots(W, requested)
            elif ev in ("raw_all", "raw_one"):
                names = list(PARAMS) if ev == "raw_all" else [rng.choice(list(PARAMS))]
                how = rng.choice(["axpby", "adam"])
                log(ev, how, names)
                for n in names:
                    W.raw_write(n, how)
                rt.bump_weights_epoch()
            elif ev == "torch":
                n = rng.choice(list(PARAMS))
                log("torch write", n)
                W.torch_write(n)
            elif ev == "precision":
                p = rng.choice([m for m in MODES if m != rt.precision])
                log("set_precision", p)
                rt.set_precision(p)
            elif ev == "bump":
                log("bump")
                rt.bump_weights_epoch()
            elif ev == "rehome":
                n = rng.choice(list(PARAMS))
                log("re-home", n)
                W.rehome(n)
            else:
                n = rng.choice(list(PARAMS))
                log("drop and recreate", n)
                W.recreate(n)
                requested = {s for s in requested if s[0] != n}
        log("final request of every slot", rt.precision)
        _request(mbe, W, SLOTS)
        _cache_is_live_slots(W, set(SLOTS))


def test_layout_raw_and_torch_write_in_one_epoch(mbe):
    """A parameter rewritten through torch and through a kernel in the same epoch, in either order, with the other layouts refreshed
    in one launch around it."""
    from colddiff import runtime as rt
    W = Weights(mbe, 7)
    _request(mbe, W, SLOTS)
    for order in (("raw", "torch"), ("torch", "raw"), ("raw", "torch", "raw")):
        for n in PARAMS:
            W.raw_write(n)
        for step in order:
            W.raw_write("conv3", "adam") if step == "raw" else W.torch_write("conv3")
        rt.bump_weights_epoch()
        _request(mbe, W, SLOTS)
        W.torch_write("to_qkv")                              # and a torch write after the refresh, inside the epoch
        _request(mbe, W, SLOTS)


def _recorder():
    from colddiff import runtime as rt
    from test_gpu_invariance import Recorder
    return Recorder(rt.lib())


def _count(rec, name):
    return sum(n == name for n, _ in rec.calls)


def _packs(rec):
    """{entry point: launches} of the pack kernels in a recording."""
    names = ("cdf_pack_many", "cdf_pack_weight", "cdf_pack_weight_bf16", "cdf_pack_cin4")
    return {n: _count(rec, n) for n in names if _count(rec, n)}


def test_layout_cache_size_and_table_over_50_epochs(mbe):
    """50 epochs of rewrite-all + bump + use: the cache stays as large as the number of live slots, the device table of cdf_pack_many is
    built once and rebuilt only when its signature (the set of sources and destinations) changes."""
    from colddiff import ops, runtime as rt
    W = Weights(mbe, 3)
    _request(mbe, W, SLOTS)
    _cache_is_live_slots(W, set(SLOTS))
    assert mbe.device not in ops._pack_tables                # the first pack of each layout is its own launch
    tab = None
    for epoch in range(50):
        for n in PARAMS:
            W.raw_write(n)
        rt.bump_weights_epoch()
        check = epoch in (0, 1, 24, 49)                      # (every epoch refreshes; the reference is computed at four of them)
        if check:
            _request(mbe, W, SLOTS)
        else:
            for n, k in SLOTS:
                ops.packed(W.p[n], k)
        _cache_is_live_slots(W, set(SLOTS))
        if tab is None:
            tab = ops._pack_tables[mbe.device]
        assert ops._pack_tables[mbe.device] is tab and len(ops._pack_tables) == 1, epoch
    n_geom = sum(k != "cin4" for _, k in SLOTS)
    assert tab[2] == n_geom
    # a dropped and recreated parameter: its slots leave with it, come back on use, and the table follows the new signature
    W.recreate("conv1")
    live = {s for s in SLOTS if s[0] != "conv1"}
    _cache_is_live_slots(W, live)
    _request(mbe, W, SLOTS)
    for n in PARAMS:
        W.raw_write(n)
    rt.bump_weights_epoch()
    _request(mbe, W, SLOTS)
    _cache_is_live_slots(W, set(SLOTS))
    tab2 = ops._pack_tables[mbe.device]
    assert tab2 is not tab and tab2[0] != tab[0] and tab2[2] == n_geom
    # a re-homed parameter changes the signature too; a bare bump does not
    W.rehome("lin")
    for bare in (False, True, True):
        if not bare:
            for n in PARAMS:
                W.raw_write(n)
        rt.bump_weights_epoch()
        _request(mbe, W, SLOTS)
    tab3 = ops._pack_tables[mbe.device]
    assert tab3 is not tab2 and tab3[0] != tab2[0]
    rt.bump_weights_epoch()
    _request(mbe, W, SLOTS)
    assert ops._pack_tables[mbe.device] is tab3


def test_layout_many_refreshed_in_one_launch(mbe):
    """After "rewrite all + bump" the first request of an epoch refreshes every layout the previous epoch used with exactly one
    cdf_pack_many and no cdf_pack_weight* launch (cin4 has no geometry: cdf_pack_cin4 packs it alone)."""
    from colddiff import ops, runtime as rt
    W = Weights(mbe, 4)
    for mode in MODES:
        rt.set_precision(mode)
        _request(mbe, W, SLOTS)
        for _ in range(2):
            for n in PARAMS:
                W.raw_write(n)
            rt.bump_weights_epoch()
            with _recorder() as rec:
                first = ops.packed(W.p["dw"], "dw")
            assert _count(rec, "cdf_pack_many") == 1 and {n for n in rec.names() if n.startswith("cdf_pack_weight")} == set(), rec.names()
            del first
            with _recorder() as rec:
                _request(mbe, W, SLOTS)
            packs = _packs(rec)
            assert packs == {"cdf_pack_cin4": 1}, (mode, packs)
    # a subset: only what the previous epoch used is refreshed, the rest is packed on demand
    used = [s for s in SLOTS if s[0] in ("conv3", "to_qkv")]
    for n in PARAMS:
        W.raw_write(n)
    rt.bump_weights_epoch()
    _request(mbe, W, used)
    for n in PARAMS:
        W.raw_write(n)
    rt.bump_weights_epoch()
    with _recorder() as rec:
        _request(mbe, W, used)
    assert _packs(rec) == {"cdf_pack_many": 1}
    tab = ops._pack_tables[mbe.device]
    assert tab[2] == len(used)
    rest = [s for s in SLOTS if s not in used]               # refreshed one epoch ago, last used two epochs ago: each on its own
    with _recorder() as rec:
        _request(mbe, W, SLOTS)
    assert _packs(rec) == {
        "cdf_pack_weight": sum(k not in R.SP_KINDS and k != "cin4" for _, k in rest), "cdf_pack_weight_bf16": sum(k in R.SP_KINDS for _, k in rest),
        "cdf_pack_cin4": 1}
    assert ops._pack_tables[mbe.device] is tab


@pytest.mark.parametrize("slot", [("conv3", "conv_fwd"), ("conv3", "conv_dgrad_sp"), ("to_qkv", "kv_dgrad_sp"), ("cin", "cin4")])
def test_layout_single_layout_is_repacked_alone(mbe, slot):
    """Fewer than two refreshable layouts: _repack_all returns 0 and the one layout is re-packed by its own launch, and is right."""
    from colddiff import ops, runtime as rt
    W = Weights(mbe, 5)
    own = {"conv_fwd": "cdf_pack_weight", "conv_dgrad_sp": "cdf_pack_weight_bf16", "kv_dgrad_sp": "cdf_pack_weight_bf16", "cin4": "cdf_pack_cin4"}[slot[1]]
    _request(mbe, W, [slot])
    for mode in ("bf16x3", "bf16", "bf16x3"):
        rt.set_precision(mode)
        for _ in range(2):
            W.raw_write(slot[0])
            rt.bump_weights_epoch()
            with _recorder() as rec:
                _request(mbe, W, [slot])
            assert _packs(rec) == {own: 1}, (mode, rec.names())
    assert len(ops._pack_cache) == 1 and not ops._pack_tables


@pytest.mark.parametrize("n_skip", [1, 3])
def test_layout_skipped_for_n_epochs(mbe, n_skip):
    """A layout nobody asks for during n epochs (the EMA net between milestones, the f32 layouts of a no_grad sampling pass): the first
    idle epoch still refreshes it (the one launch goes by what the PREVIOUS epoch used), from then on it is not rewritten -- its
    buffers keep those bits -- and it is right at its next use."""
    from colddiff import ops, runtime as rt
    W = Weights(mbe, 6)
    idle = [("convT", "convT_dgrad"), ("convT", "convT_fwd_sp"), ("to_qkv", "kv_fwd_sp"), ("lin", "lin_fwd")]
    busy = [s for s in SLOTS if s not in idle]
    _request(mbe, W, SLOTS)
    for n in PARAMS:
        W.raw_write(n)
    rt.bump_weights_epoch()
    _request(mbe, W, SLOTS)                                  # the idle layouts were refreshed by cdf_pack_many once: in place
    held = {s: ops._pack_cache[(id(W.p[s[0]]), s[1])].out for s in idle}
    flat_ = lambda o: [t for t in (o if isinstance(o, tuple) else (o,)) if t is not None]
    for n in PARAMS:
        W.raw_write(n)
    rt.bump_weights_epoch()
    _request(mbe, W, busy)                                   # the first idle epoch
    _sync(mbe)
    for s in idle:                                           # (refreshed with the rest: the bits of THIS epoch's weights)
        assert R.same_layout(held[s], R.layout_ref(W.p[s[0]], s[1], rt.precision, mbe.device)), s
    before = {s: [t.clone() for t in flat_(o)] for s, o in held.items()}
    for _ in range(n_skip):
        for n in PARAMS:
            W.raw_write(n)
        rt.bump_weights_epoch()
        _request(mbe, W, busy)
        _request(mbe, W, busy)
        _sync(mbe)
        for s in idle:
            assert ops._pack_cache[(id(W.p[s[0]]), s[1])].out is held[s]
            assert all(torch.equal(a, b) for a, b in zip(flat_(held[s]), before[s])), s
    with _recorder() as rec:
        _request(mbe, W, idle)
    assert _count(rec, "cdf_pack_many") == 0                 # too old for the one-launch refresh: each on its own
    _request(mbe, W, SLOTS)
    for n in PARAMS:
        W.raw_write(n)
    rt.bump_weights_epoch()
    _request(mbe, W, SLOTS)


def test_layout_precision_toggle_on_a_shared_slot(mbe):
    """What runtime.precision_scope documents: the cache keeps ONE layout per (parameter, kind).  A kind without `_sp` holds the same
    values in every mode, shares its slot across the modes and is packed again on a toggle (its buffer is reused); an `_sp` kind
    changes its contents with the mode (lo plane or None)."""
    from colddiff import ops, runtime as rt
    W = Weights(mbe, 8)
    slots = [("conv3", "conv_fwd"), ("conv3", "conv_fwd_sp"), ("to_qkv", "kv_fwd"), ("to_qkv", "kv_dgrad_sp"), ("cin", "cin4")]
    _request(mbe, W, slots)
    bufs = {s: ops._pack_cache[(id(W.p[s[0]]), s[1])].out for s in slots}
    for mode in ("f32", "bf16x3", "bf16", "f32", "bf16", "bf16x3"):
        with rt.precision_scope(mode), _recorder() as rec:
            _request(mbe, W, slots)
            again = _packs(rec)
            _request(mbe, W, slots)
        toggled = mode != "bf16x3"
        assert again == ({"cdf_pack_weight": 2, "cdf_pack_weight_bf16": 2, "cdf_pack_cin4": 1} if toggled else {}), (mode, again)
        assert len(ops._pack_cache) == len(slots)
        for s in slots:
            e = ops._pack_cache[(id(W.p[s[0]]), s[1])]
            assert e.precision == mode
            if s[1] in ("conv_fwd", "kv_fwd"):
                assert e.out is bufs[s]                      # one slot, one buffer, whatever the mode
        with _recorder() as rec:                             # ... and the first use after the region ends packs again
            _request(mbe, W, slots)
        assert bool(rec.names() & {"cdf_pack_weight", "cdf_pack_weight_bf16"}) == toggled


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. network level: warm equals cold equals the oracle
# ---------------------------------------------------------------------------------------------------------------------------------
NETS = {
    # kind -> (constructor keywords, image size, seeds, events per sequence)
    "unet16": (dict(dim=16, dim_mults=(1, 2), channels=3), 8, [201, 202, 203], 25),
    "unet64": (dict(dim=64, dim_mults=(1, 2), channels=3), 8, [211, 212], 12),             # pre-split _sp / kv_*_sp layouts, gradient planes
    "model": (dict(resolution=16, in_channels=3, out_ch=3, ch=32, ch_mult=(1, 2), num_res_blocks=1, attn_resolutions=(8,), dropout=0.1), 16,
              [221, 222], 12),                                                              # the f32 sampling path under no_grad
}
LR, BETA = 0.05, 0.5


def forward_bound(mode):
    from colddiff import runtime as rt
    return rt.BF16_TOLERANCE["forward_max_abs"] if mode == "bf16" else 1e-4


def _build_net(kind, seed):
    from deblurring_diffusion_pytorch import Model, Unet
    torch.manual_seed(seed)
    return Model(**NETS[kind][0]) if kind == "model" else quiet(Unet, **NETS[kind][0])


def _oracle(kind, sd, x, t):
    sd = {k: v.detach().cpu().clone() for k, v in sd.items()}
    if kind == "model":
        return O.model_forward(sd, x, t, num_res_blocks=1, num_resolutions=2)
    return O.unet_forward(sd, x, t)


class Twin:
    """A net and its EMA twin, each in a FlatArena, with a FusedAdam on the net; and what the oracle needs to judge an evaluation."""

    def __init__(self, mbe, kind, seed):
        import copy
        from colddiff import flat
        self.mbe, self.kind = mbe, kind
        self.net = _build_net(kind, seed).to(mbe.device)
        self.ema = copy.deepcopy(self.net)
        self.arena = flat.FlatArena(list(self.net.parameters()))
        self.ema_arena = flat.FlatArena(list(self.ema.parameters()))
        self.opt = flat.FusedAdam(self.arena, lr=LR)
        size = NETS[kind][1]
        g = torch.Generator().manual_seed(seed + 1)
        self.x = torch.rand(2, 3, size, size, generator=g) * 2 - 1
        self.t = torch.tensor([3, 17])
        self.gy = torch.randn(2, 3, size, size, generator=g)
        # what (a)'s margin needs: the state of each net before its last move, and whether it moved since its last evaluation
        self.before = {"net": None, "ema": None}
        self.moved = {"net": False, "ema": False}
        self.margins = []

    def module(self, which):
        return self.net if which == "net" else self.ema

    def data(self, which):
        return (self.arena if which == "net" else self.ema_arena).data

    @contextlib.contextmanager
    def moving(self, which):
        """Around an event that may rewrite `which`: remember the state of before if it did."""
        sd = {k: v.detach().cpu().clone() for k, v in self.module(which).state_dict().items()}
        old = self.data(which).clone()
        yield
        # (ema_update of an EMA that equals the model only rounds it: a move is one the eye can see, a quarter of an EMA half-step)
        if (old - self.data(which)).abs().max().item() >= LR / 8:
            self.before[which], self.moved[which] = sd, True
            self.to_image_scale(which)

    def to_image_scale(self, which):
        """One Adam step at lr 0.05 moves the output by an order of magnitude, and the project's forward bounds are absolute ones for
        outputs at image scale (runtime.BF16_TOLERANCE: |y| <~ 2.5).  So after every event that moved a net, its LAST layer (the output
        is linear in it) is rescaled by an in-place torch write to |oracle output|max = 1.  Every other parameter keeps its version
        counter: their layouts still depend on the weights epoch alone."""
        m = self.module(which)
        last = m.conv_out if self.kind == "model" else m.final_conv[1]
        s = 1.0 / _oracle(self.kind, m.state_dict(), self.x, self.t).abs().max().item()
        with torch.no_grad():
            last.weight.mul_(s)
            last.bias.mul_(s)

    # -- events ---------------------------------------------------------------------------------------------------------------------
    def fwd_bwd(self, step):
        from colddiff import runtime as rt
        self.net.train()
        y = self.net(self.mbe.to(self.x), self.mbe.to(self.t))
        if self.kind != "model":                             # (Model draws dropout masks in training mode: no oracle for that pass)
            self.check_oracle("net", y.detach(), rt.precision)
        y.backward(self.mbe.to(self.gy))
        if step:
            with self.moving("net"):
                self.opt.step()
        self.opt.zero_grad()

    def ema_update(self):
        from colddiff import flat
        with self.moving("ema"):
            flat.ema_update(self.ema_arena, self.arena, BETA)

    def arena_copy(self):
        from colddiff.trainer import Trainer
        with self.moving("ema"):
            Trainer.reset_parameters(types.SimpleNamespace(arena=self.arena, ema_arena=self.ema_arena, model=self.net, ema_model=self.ema))

    def load_scaled(self, which, scale):
        m = self.module(which)
        sd = {k: (v * scale if v.is_floating_point() else v) for k, v in m.state_dict().items()}
        with self.moving(which):
            m.load_state_dict(sd)
        assert self.arena.intact() and self.ema_arena.intact()

    # -- checks ---------------------------------------------------------------------------------------------------------------------
    def check_oracle(self, which, y, mode):
        ref = _oracle(self.kind, self.module(which).state_dict(), self.x, self.t)
        err, bound = (y.cpu() - ref).abs().max().item(), forward_bound(mode)
        print(f"  {self.kind} {which} {mode}: forward error {err:.3g} (bound {bound:g}, |y|max {ref.abs().max().item():.3g})")
        assert err <= bound, (which, mode, err, bound)
        return ref

    def evaluate(self, which, others=()):
        """no_grad evaluation of one net: (a) against the oracle at its current state_dict, (b) bit-equal to a cold start."""
        from colddiff import runtime as rt
        m = self.module(which)
        m.eval()
        with torch.no_grad():
            y = m(self.mbe.to(self.x), self.mbe.to(self.t))
        # Model samples on the exact-fp32 kernels under no_grad in the default mode (model2.py); the bound is the same 1e-4
        ref = self.check_oracle(which, y, rt.precision)
        if self.moved[which]:
            stale = _oracle(self.kind, self.before[which], self.x, self.t)
            d = (stale - ref).abs().max().item()
            print(f"  {self.kind} {which}: stale margin {d / forward_bound('f32'):.3g} x the f32 / bf16x3 bound, {d / forward_bound('bf16'):.3g} x the bf16 bound")
            self.margins.append(d)
            # (test_network_stale_weights_break_the_bound asserts 10 x the bf16 bound for a first move of each kind; later Adam steps are
            # smaller: the momentum settles.  Here every move must at least be far outside the tight bound.)
            assert d >= 10 * forward_bound("f32"), (which, rt.precision, d)
            self.moved[which] = False
        with R.cold_start([self.net, self.ema] + [o for o in others]):
            with torch.no_grad():
                y2 = m(self.mbe.to(self.x), self.mbe.to(self.t))
        assert torch.equal(y, y2), (which, rt.precision, (y - y2).abs().max().item())


def _network_sequence(mbe, kind, seed, n_events):
    from colddiff import runtime as rt
    rng = random.Random(seed)
    tw = Twin(mbe, kind, seed)
    other = Twin(mbe, "unet16", seed + 50)                   # a second, unrelated net on the same device
    alphabet = (["step"] * 4 + ["fwd_bwd", "ema_update", "ema_update", "arena_copy", "load_net", "load_ema", "mode", "other_step"] +
                ["eval_net"] * 3 + ["eval_ema"] * 3)
    with R.Trace() as log:
        for _ in range(n_events):
            ev = rng.choice(alphabet)
            log(ev, "| mode", rt.precision, "epoch", rt.weights_epoch)
            if ev == "step":
                tw.fwd_bwd(True)
            elif ev == "fwd_bwd":
                tw.fwd_bwd(False)
            elif ev == "ema_update":
                tw.ema_update()
            elif ev == "arena_copy":
                tw.arena_copy()
            elif ev in ("load_net", "load_ema"):
                tw.load_scaled(ev[5:], rng.choice(SCALES))
            elif ev == "mode":
                rt.set_precision(rng.choice(MODES))
                log[-1] += " -> " + rt.precision
            elif ev == "other_step":
                other.fwd_bwd(True)
            else:
                tw.evaluate(ev[5:], others=[other.net, other.ema])
        for mode in MODES:                                   # every sequence ends with both nets in every mode
            rt.set_precision(mode)
            for which in ("net", "ema"):
                log("final eval", which, mode)
                tw.evaluate(which, others=[other.net, other.ema])
    return tw


@pytest.mark.parametrize("kind,seed", [(k, s) for k, v in NETS.items() for s in v[2]])
def test_network_sequences(mbe, kind, seed):
    tw = _network_sequence(mbe, kind, seed, NETS[kind][3])
    assert tw.margins, "the sequence never evaluated a net after moving it"


@pytest.mark.parametrize("mode", MODES)
def test_network_every_writer_between_two_evaluations(mbe, mode):
    """Each writer of weights directly between two evaluations of the net it writes, with no other event (and so no other writer's
    bump) in between: the second evaluation is (a) the oracle's at the new weights and (b) the cold start's.  The random sequences
    reach `evaluate, write, evaluate` within one epoch only by chance; this is the case a writer without its bump fails."""
    from colddiff import runtime as rt
    rt.set_precision(mode)
    tw = Twin(mbe, "unet16", 31)
    with R.Trace() as log:
        for which, name, write in (("net", "Adam step", lambda: tw.fwd_bwd(True)),
                                   ("ema", "ema_update", tw.ema_update),
                                   ("ema", "ema_update again", tw.ema_update),
                                   ("net", "load_state_dict", lambda: tw.load_scaled("net", SCALES[0])),
                                   ("ema", "arena copy", tw.arena_copy),
                                   ("ema", "load_state_dict", lambda: tw.load_scaled("ema", SCALES[1])),
                                   ("net", "Adam step", lambda: tw.fwd_bwd(True)),
                                   ("ema", "ema_update", tw.ema_update)):
            log("evaluate", which, "|", name, "| evaluate", which, "in", mode)
            tw.evaluate(which)
            tw.moved[which] = False
            write()
            assert tw.moved[which], name
            tw.evaluate(which)
    assert len(tw.margins) == 8


def _last_layer(kind):
    return "conv_out" if kind == "model" else "final_conv.1"


def _at_image_scale(kind, sd, x, t):
    """(sd with its last layer rescaled to |oracle output|max = 1, that output): Twin.to_image_scale on a host state_dict."""
    y = _oracle(kind, sd, x, t)
    s = 1.0 / y.abs().max().item()
    last = _last_layer(kind)
    return {k: (v * s if k in (last + ".weight", last + ".bias") else v.clone()) for k, v in sd.items()}, y * s


SCALES = (0.5, 2.0)                  # load_state_dict events: every floating-point entry times one of these


@pytest.mark.parametrize("kind", list(NETS))
def test_network_stale_weights_break_the_bound(kind):
    """The premise of (a), on the oracle alone: a forward through weights one event old differs from the current one by at least 10 x
    the bound, for each kind of event that rewrites weights -- an Adam step at lr 0.05 (the first one: every element moves by lr
    against the sign of its gradient), ema_update at beta 0.5 one step behind, a state_dict scaled by SCALES -- with the outputs at
    image scale as in the sequences, and for the widest bound (bf16 mode; the f32 / bf16x3 bound is 200 times tighter)."""
    net = _build_net(kind, 5)
    size = NETS[kind][1]
    g = torch.Generator().manual_seed(6)
    x, t, gy = torch.rand(2, 3, size, size, generator=g) * 2 - 1, torch.tensor([3, 17]), torch.randn(2, 3, size, size, generator=g)
    sd0, y0 = _at_image_scale(kind, {k: v.detach().clone() for k, v in net.state_dict().items()}, x, t)
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd0.items()}
    y = O.model_forward(leaves, x, t, num_res_blocks=1, num_resolutions=2) if kind == "model" else O.unet_forward(leaves, x, t)
    y.backward(gy)
    assert all(v.grad is not None for v in leaves.values())
    sd1, _ = _at_image_scale(kind, {k: v - LR * torch.sign(leaves[k].grad) for k, v in sd0.items()}, x, t)
    bound = forward_bound("bf16")
    cases = [("adam step", sd1), ("ema_update one step behind", {k: BETA * sd0[k] + (1 - BETA) * sd1[k] for k in sd0})]
    cases += [("scaled %g" % s, {k: v * s for k, v in sd0.items()}) for s in SCALES]
    for name, sd in cases:
        d = (_at_image_scale(kind, sd, x, t)[1] - y0).abs().max().item()
        print(f"  {kind} {name}: the output moves by {d:.3g} = {d / bound:.3g} x the bf16 bound")
        assert d >= 10 * bound, (name, d)


def test_time_bias_all_backwards_in_reverse_order(mbe):
    """TimeBiasAll's backward reads the owner's CURRENT cache: two forwards, then the backwards in reverse order, under unchanged
    weights, give bit for bit the gradients of the straight order."""
    net = _build_net("unet16", 9).to(mbe.device)
    g = torch.Generator().manual_seed(10)
    xs = [mbe.to(torch.rand(2, 3, 8, 8, generator=g) * 2 - 1) for _ in range(2)]
    ts = [mbe.to(torch.tensor([3, 17])), mbe.to(torch.tensor([0, 9]))]
    gys = [mbe.to(torch.randn(2, 3, 8, 8, generator=g)) for _ in range(2)]

    def grads():
        out = [p.grad.detach().cpu().clone() for p in net.parameters()]
        net.zero_grad(set_to_none=True)
        return out
    straight = []
    for i in (0, 1):
        net(xs[i], ts[i]).backward(gys[i])
        straight.append(grads())
    ys = [net(xs[i], ts[i]) for i in (0, 1)]
    assert "_tb_cache" in net.__dict__
    rev = {}
    for i in (1, 0):
        ys[i].backward(gys[i])
        rev[i] = grads()
    for i in (0, 1):
        assert all(torch.equal(a, b) for a, b in zip(straight[i], rev[i])), i
        assert any(a.abs().max() > 0 for a in straight[i])


def test_blur_taps_follow_the_state_dict(mbe):
    """GaussianDiffusion._taps after load_state_dict (a torch write: the version moves) and after .to(device) / a re-homed weight (the
    pointer moves): the stack is the current weights', and q_sample from the warm cache is the cold start's bit for bit."""
    from deblurring_diffusion_pytorch import GaussianDiffusion
    d = GaussianDiffusion(torch.nn.Identity(), image_size=16, device_of_kernel="cuda", channels=3, timesteps=5, kernel_std=0.3, kernel_size=5,
                          blur_routine="Incremental")
    g = torch.Generator().manual_seed(11)
    x, t = torch.rand(3, 3, 16, 16, generator=g) * 2 - 1, torch.tensor([4, 0, 2])
    host = d._taps(torch.device("cpu")).clone()              # (built before the move: the cache holds a host stack now)
    d = d.to(mbe.device)

    def check(what):
        want = torch.stack([m.weight.detach()[:, 0] for m in d.gaussian_kernels])
        taps = d._taps(mbe.device)
        assert taps.device.type == mbe.device.type and torch.equal(taps, want), what
        with torch.no_grad():
            y = d.q_sample(mbe.to(x), mbe.to(t))
            with R.cold_start(cores=[d]):
                y2 = d.q_sample(mbe.to(x), mbe.to(t))
        assert torch.equal(y, y2), what
        return y.cpu()
    y0 = check(".to(device)")
    assert torch.equal(d._taps(mbe.device).cpu(), host)
    sd = {k: (v * 0.5 if "gaussian_kernels" in k else v) for k, v in d.state_dict().items()}
    d.load_state_dict(sd)
    y1 = check("load_state_dict")
    assert not torch.equal(y0, y1)
    for m in d.gaussian_kernels:                             # re-homed with other values, as Module.to() does it
        m.weight.data = m.weight.data * 3.0
    y2 = check("re-homed")
    assert not torch.equal(y1, y2)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. graph mode
# ---------------------------------------------------------------------------------------------------------------------------------
GRAPH_LR = 1e-3              # the Trainer's own L1 loss keeps the output at image scale at this rate; one step still moves it visibly


@pytest.mark.gpu
def test_graph_mode_eager_evaluations_between_replays(monkeypatch, tmp_path):
    """A graph-mode Trainer: 3 warm-up steps and 3 replays, the training and the EMA net evaluated eagerly in the captured mode and
    under precision_scope("f32"), 2 more replays, a second Trainer steps, both nets evaluated again.  Every evaluation satisfies (a)
    and (b); the final weights, moments and EMA -- the arenas whole, alignment gaps included -- are bit for bit those of an eager
    Trainer fed the same events, and the gradient arena is all zero bits after the last step on both sides.  (The evaluations read
    weights back to the host between the replays; with a memset node in the captured step the replayed zero_grad left denormal-size
    values in the gradient arena after such reads and Adam carried them into exp_avg: cdf_zero is a kernel node under capture.)"""
    from colddiff import runtime as rt
    import test_graph_train as G
    rt._lib_override = None
    g = torch.Generator().manual_seed(12)
    x, t = (torch.rand(2, 1, 16, 16, generator=g) * 2 - 1).to(G.DEV), torch.tensor([1, 3], device=G.DEV)

    host = lambda net: {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    before = {}

    def evaluate(tr, other, what):
        for core in (tr.core, tr.ema_core):
            net = core.denoise_fn
            with torch.no_grad():
                y = net(x, t)
            ref = O.unet_forward(host(net), x.cpu(), t.cpu())
            err = (y.cpu() - ref).abs().max().item()
            print(f"  {what} {'ema' if core is tr.ema_core else 'net'} {rt.precision}: forward error {err:.3g}, |y|max {ref.abs().max().item():.3g}")
            assert err <= forward_bound(rt.precision), (what, err)
            if core is tr.core:                              # the weights of one step ago would miss the bound by a wide margin
                d = (O.unet_forward(before[id(tr)], x.cpu(), t.cpu()) - ref).abs().max().item()
                print(f"  {what} net: stale margin {d / forward_bound(rt.precision):.3g} x bound")
                assert d >= 10 * forward_bound(rt.precision), (what, d)
            with R.cold_start([tr.model, tr.ema_model, other.model, other.ema_model], cores=[tr.core, tr.ema_core]), torch.no_grad():
                y2 = net(x, t)
            assert torch.equal(y, y2), what

    def events(graph, folder):
        folder.mkdir()
        other = G.build("unet3", False, folder / "o")
        tr = G.build("unet", graph, folder / "t", train_lr=GRAPH_LR)

        def steps(n):
            for _ in range(n):
                before[id(tr)] = host(tr.core.denoise_fn)
                G._quiet(tr.train_step)
                tr.step += 1
        steps(G.W + 3)
        evaluate(tr, other, "after 3 replays")
        with rt.precision_scope("f32"):
            evaluate(tr, other, "after 3 replays")
        steps(2)
        state = torch.get_rng_state(), torch.cuda.get_rng_state(G.DEV)
        for _ in range(2):
            G._quiet(other.train_step)
        torch.set_rng_state(state[0]), torch.cuda.set_rng_state(state[1], G.DEV)
        evaluate(tr, other, "after the second Trainer")
        steps(1)
        evaluate(tr, other, "at the end")
        torch.cuda.synchronize()
        out = {"net." + k: v.cpu() for k, v in tr.model.state_dict().items()}
        out.update({"ema." + k: v.cpu() for k, v in tr.ema_model.state_dict().items()})
        # the arenas whole, alignment gaps included, as test_graph_train.run compares them; the gradient arena as the step's zero_grad left it
        out.update({"arena": tr.arena.data.cpu(), "exp_avg": tr.opt.exp_avg.cpu(), "exp_avg_sq": tr.opt.exp_avg_sq.cpu(), "ema_arena": tr.ema_arena.data.cpu(),
                    "grad": tr.arena.grad.cpu(), "counts": torch.tensor([tr.opt.step_count, tr.step])})
        return tr, out
    monkeypatch.setenv("COLDDIFF_PREFETCH", "0")
    _, eager = events(False, tmp_path / "e")
    monkeypatch.delenv("COLDDIFF_PREFETCH")
    tg, graph = events(True, tmp_path / "g")
    for side in (eager, graph):
        assert not side["grad"].view(torch.int32).any()      # zero bits everywhere: a replayed zero_grad zeroes what the eager one does
    G.same(eager, graph)
    G.graphed(tg, G.W + 6, captures=1, replays=6)


@pytest.mark.gpu
@pytest.mark.parametrize("skip,nbytes", [(0, 4096), (4, 16), (1, 3), (3, 4096 * 3 + 5), (16, 1 << 20), (7, 9)])
def test_graph_mode_captured_zero_stays_inside_its_range(skip, nbytes):
    """cdf_zero under stream capture is a kernel (16-byte stores from the first aligned address, ragged ends byte by byte): replayed
    twice over a 0xA5-filled buffer it zeroes bytes [skip, skip + nbytes) and nothing else, for aligned and unaligned starts, lengths
    below one 16-byte group and lengths that are no multiple of it.  Outside capture the same call (a memset) does the same."""
    from colddiff import runtime as rt
    rt._lib_override = None
    dev = torch.device("cuda:0")
    buf = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device=dev)
    want = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8)
    want[skip:skip + nbytes] = 0
    rt.lib().cdf_zero(buf.data_ptr() + skip, nbytes, rt.stream(buf))
    assert torch.equal(buf.cpu(), want)
    g = torch.cuda.CUDAGraph()
    buf.fill_(0xA5)
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        rt.lib().cdf_zero(buf.data_ptr() + skip, nbytes, rt.stream(buf))
    torch.cuda.synchronize()
    assert torch.equal(buf.cpu(), torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8))       # a capture pass launches nothing
    for _ in range(2):
        buf.fill_(0xA5)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(buf.cpu(), want)
