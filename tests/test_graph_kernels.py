"""The entry points a graph-mode optimizer step needs (ABI 16): the per-step host scalars read from device memory.

  cdf_adam_params / cdf_adam_step_dev            Adam's six scalars computed on the host once, read by the kernel from `hp`
  cdf_dropout_sd, cdf_groupnorm_{fwd,bwd}_ex_sd  the dropout seed read from `seed_dev`

Each must give, bit for bit, what its by-value original gives for the same values -- and must give the OTHER values' result when
only the contents of hp / seed_dev change between two launches with identical arguments: that is what a graph replay does.
Runs on the simulator and on the MI355X (`be`)."""
import pytest
import torch

from colddiff._lib import CdfError
from poison import GUARD, nan_empty, poison_
from test_kernels import P
from test_kernels_production import bits_equal, twice
from test_norm_dw_forms import GB_ROWS, GF_ROWS, GN_EPS, GROUPS
from test_small_kernels_production import CAP, PAST

SEEDS = (0, 1, (1 << 40) + 12345, (1 << 62) - 1)
PS = (0.1, 0.5)


def expect(fn, args, text):
    try:
        fn(*args)
    except CdfError as e:
        assert text in str(e), str(e)
    else:
        raise AssertionError("expected CdfError containing %r" % text)


def sync(be):
    if be.kind == "hip":
        torch.cuda.synchronize()


def seed_word(be, seed=0):
    return be.to(torch.tensor([seed], dtype=torch.int64))


# ---------------------------------------------------------------------------------------------------------------------------------
# Adam
# ---------------------------------------------------------------------------------------------------------------------------------
def host_params(be, lr, b1, b2, eps, step):
    out = torch.full((8,), float("nan"))
    be.L.cdf_adam_params(lr, b1, b2, eps, step, out.data_ptr())
    return out


def test_adam_params_are_the_scalars_of_adam_step(be):
    """The documented layout, from the double arithmetic of cdf_adam_step (its float roundings via numpy's float32)."""
    import numpy as np
    lr, b1, b2, eps = 2e-5, 0.9, 0.999, 1e-8
    for step in (1, 2, 100000, 100001):
        got = host_params(be, lr, b1, b2, eps, step)
        bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
        want = [np.float32(1.0 - b1), np.float32(b2), np.float32(1.0 - b2), np.float32(-(lr / bc1)), np.float32(np.sqrt(bc2)), np.float32(eps), 0.0, 0.0]
        assert got.tolist() == [float(w) for w in want], (step, got.tolist(), want)
    expect(be.L.cdf_adam_params, [lr, b1, b2, eps, 0, torch.zeros(8).data_ptr()], "bad args")
    expect(be.L.cdf_adam_params, [lr, b1, b2, eps, 1, 0], "bad args")


@pytest.mark.parametrize("n", [1000, CAP + PAST])
def test_adam_step_dev_equals_adam_step(be, n):
    torch.manual_seed(n % 977)
    lr, b1, b2, eps = 2e-5, 0.9, 0.999, 1e-8
    s = be.stream()
    bufs = [nan_empty(be, n + GUARD) for _ in range(3)]                  # p, m, v of the device-scalar launches, a poisoned band behind each
    pd, md, vd = (b[:n] for b in bufs)
    pr, mr, vr, gd = be.zeros(n), be.zeros(n), be.zeros(n), be.zeros(n)    # the by-value reference's state
    hp = be.to(torch.zeros(8))
    assert hp.data_ptr() % 16 == 0
    state = [torch.randn(n), torch.zeros(n), torch.zeros(n)]
    state[0][:500] *= 1e-5

    def by_value(lr_, step_):
        for d, h in zip((pr, mr, vr), state):
            d.copy_(h)
        be.L.cdf_adam_step(P(pr), P(gd), P(mr), P(vr), n, lr_, b1, b2, eps, step_, s)
        sync(be)
        return [t.detach().cpu().clone() for t in (pr, mr, vr)]

    def by_table():
        for d, h in zip((pd, md, vd), state):
            d.copy_(h)
        be.L.cdf_adam_step_dev(P(pd), P(gd), P(md), P(vd), n, P(hp), s)          # the SAME arguments every time: only hp's contents move
        sync(be)
        assert all(bool(torch.isnan(b[n:]).all()) for b in bufs), "a guard band behind p / m / v was written"
        return [t.detach().cpu().clone() for t in (pd, md, vd)]

    for step in (1, 2, 100000, 100001):
        g = torch.randn(n) * (10.0 ** torch.randint(-6, 2, (n,)).double()).float()
        g[::7] = 0.0
        gd.copy_(g)
        want = by_value(lr, step)
        hp.copy_(host_params(be, lr, b1, b2, eps, step))
        got = by_table()
        again = by_table()
        for k, (a, b, c) in enumerate(zip(got, want, again)):
            assert bits_equal(a, b), (step, "pmv"[k], "differs from cdf_adam_step")
            assert bits_equal(a, c), (step, "pmv"[k], "the same launch twice differs")
        # a replay: same launch, other contents of hp (another lr, another step)
        want2 = by_value(lr * 0.5, step + 7)
        hp.copy_(host_params(be, lr * 0.5, b1, b2, eps, step + 7))
        got2 = by_table()
        for k, (a, b) in enumerate(zip(got2, want2)):
            assert bits_equal(a, b), (step, "pmv"[k], "new contents of hp did not give cdf_adam_step's result for them")
        assert not bits_equal(got2[0], got[0])
        state = got                                                                # one evolving state


def test_adam_step_dev_refuses_bad_hp(be):
    n = 64
    p, g, m, v, hp = be.to(torch.randn(n)), be.to(torch.randn(n)), be.zeros(n), be.zeros(n), be.to(torch.zeros(12))
    before = p.detach().cpu().clone()
    expect(be.L.cdf_adam_step_dev, [P(p), P(g), P(m), P(v), n, P(hp) + 4, be.stream()], "16B aligned")
    expect(be.L.cdf_adam_step_dev, [P(p), P(g), P(m), P(v), n, P(hp) + 8, be.stream()], "16B aligned")
    expect(be.L.cdf_adam_step_dev, [P(p), P(g), P(m), P(v), n, 0, be.stream()], "null hp")
    expect(be.L.cdf_adam_step_dev, [0, P(g), P(m), P(v), n, P(hp), be.stream()], "bad args")
    sync(be)
    assert bits_equal(p.detach().cpu(), before) and not m.any() and not v.any()     # a status and a message, no launch


# ---------------------------------------------------------------------------------------------------------------------------------
# dropout
# ---------------------------------------------------------------------------------------------------------------------------------
def test_dropout_sd_equals_dropout(be):
    """A [34, 40] map with a pitch wider than its row (48 in, 44 out)."""
    torch.manual_seed(5)
    rows, C, ldx, ldy = 34, 40, 48, 44
    x = be.to(torch.randn(rows, ldx))
    y, sd = nan_empty(be, rows, ldy), seed_word(be)
    masks = {}
    for p in PS:
        for seed in SEEDS:
            want, = twice(lambda: be.L.cdf_dropout(P(x), ldx, P(y), ldy, rows, C, p, seed, be.stream()), [y])
            sd.fill_(seed)
            got, = twice(lambda: be.L.cdf_dropout_sd(P(x), ldx, P(y), ldy, rows, C, p, P(sd), be.stream()), [y])      # same arguments for every seed
            assert bits_equal(got, want), (p, seed)
            assert bool(torch.isnan(got[:, C:]).all())
            masks[p, seed] = got[:, :C] != 0
        assert len({tuple(m.reshape(-1).tolist()) for (q, _), m in masks.items() if q == p}) == len(SEEDS), "two seeds gave one mask"
    expect(be.L.cdf_dropout_sd, [P(x), ldx, P(y), ldy, rows, C, 1.0, P(sd), be.stream()], "cdf_dropout: bad args")
    expect(be.L.cdf_dropout_sd, [P(x), ldx, 0, ldy, rows, C, 0.1, P(sd), be.stream()], "cdf_dropout: bad args")
    expect(be.L.cdf_dropout_sd, [P(x), ldx, P(y), ldy, rows, C, 0.1, 0, be.stream()], "seed_dev")
    expect(be.L.cdf_dropout_sd, [P(x), ldx, P(y), ldy, rows, C, 0.1, P(sd) + 4, be.stream()], "seed_dev")


# ---------------------------------------------------------------------------------------------------------------------------------
# GroupNorm + SiLU + dropout
# ---------------------------------------------------------------------------------------------------------------------------------
def _smallest(rows, pred):
    return min((r for r in rows if r.p and pred(r)), key=lambda r: r.B * r.HW * r.C)


GF_PLAIN = _smallest(GF_ROWS, lambda r: "h" not in r.out)            # fp32 output only
GF_SPLIT = _smallest(GF_ROWS, lambda r: "h" in r.out)                # with the bf16 output planes
GB_DROP = _smallest(GB_ROWS, lambda r: True)


@pytest.mark.parametrize("r", [GF_PLAIN, GF_SPLIT], ids=lambda r: "-".join(map(str, r)))
def test_groupnorm_fwd_ex_sd_equals_fwd_ex(be, r):
    B, HW, C = r.B, r.HW, r.C
    ldx, ldy, ldp = r.ldx or C, r.ldy or C, r.ldp or C
    g_ = torch.Generator().manual_seed(C + HW)
    x, ga, bt = be.to(torch.randn(B, HW, ldx, generator=g_)), be.to(torch.randn(C, generator=g_)), be.to(torch.randn(C, generator=g_))
    nch = be.L.cdf_groupnorm_nchunk(HW)
    y, mean, rstd, ws = nan_empty(be, B, HW, ldy), nan_empty(be, B * GROUPS), nan_empty(be, B * GROUPS), nan_empty(be, B * nch * 2 * C)
    hi, lo = nan_empty(be, B, HW, ldp, dtype=torch.int16), nan_empty(be, B, HW, ldp, dtype=torch.int16)
    sd = seed_word(be)
    h, l_ = "h" in r.out, "l" in r.out

    def args(p, seed, y_on=("y" in r.out), hi_p=None, lo_p=None):
        return [P(x), ldx, P(y) if y_on else 0, ldy, P(ga), P(bt), P(mean), P(rstd), P(ws), B, HW, C, GROUPS, GN_EPS, r.silu, p, seed,
                (P(hi) if h else 0) if hi_p is None else hi_p, (P(lo) if l_ else 0) if lo_p is None else lo_p, ldp if h else 0, be.stream()]
    outs = [y, mean, rstd, hi, lo]
    seen = {}
    for p in PS:
        for seed in SEEDS:
            want = twice(lambda: be.L.cdf_groupnorm_fwd_ex(*args(p, seed)), outs)
            sd.fill_(seed)
            got = twice(lambda: be.L.cdf_groupnorm_fwd_ex_sd(*args(p, P(sd))), outs)
            for k, (a, b) in enumerate(zip(got, want)):
                assert bits_equal(a, b), (r, p, seed, ("y", "mean", "rstd", "hi", "lo")[k])
            seen[p, seed] = (got[0] if "y" in r.out else got[3]).reshape(-1).tolist()
        assert len({tuple(v) for (q, _), v in seen.items() if q == p}) == len(SEEDS), "two seeds gave one mask"
    expect(be.L.cdf_groupnorm_fwd_ex_sd, args(1.0, P(sd)), "dropout probability")
    expect(be.L.cdf_groupnorm_fwd_ex_sd, args(0.1, P(sd), y_on=True, hi_p=0, lo_p=P(lo)), "lo plane without hi plane")
    expect(be.L.cdf_groupnorm_fwd_ex_sd, args(0.1, 0), "seed_dev")


def test_groupnorm_bwd_ex_sd_equals_bwd_ex(be):
    r = GB_DROP
    B, HW, C = r.B, r.HW, r.C
    ldx, lddy, lddx = r.ldx or C, r.lddy or C, r.lddx or C
    g_ = torch.Generator().manual_seed(C + HW + 1)
    rn = lambda *s: torch.randn(*s, generator=g_)
    x, dy, ga, bt = be.to(rn(B, HW, ldx)), be.to(rn(B, HW, lddy)), be.to(rn(C)), be.to(rn(C))
    mean, rstd = be.to(rn(B * GROUPS) * 0.1), be.to(rn(B * GROUPS).abs() + 0.5)
    old = [be.to(rn(B, HW, lddx)), be.to(rn(C)), be.to(rn(C))]
    nch = be.L.cdf_groupnorm_nchunk(HW)
    dx, dga, dbt, ws = nan_empty(be, B, HW, lddx), nan_empty(be, C), nan_empty(be, C), nan_empty(be, B * nch * 2 * C + B * 2 * C + B * GROUPS * 2)
    sd = seed_word(be)

    def run(fn, p, seed):
        res = []
        for _ in range(2):
            poison_(ws)
            for d, o in zip((dx, dga, dbt), old):                       # (the accumulate forms read what is there)
                d.copy_(o)
            fn(P(dy), lddy, P(x), ldx, P(ga), P(bt), P(mean), P(rstd), P(dx), lddx, P(dga), P(dbt), P(ws), B, HW, C, GROUPS, r.silu, r.accdx, r.accp, p,
               seed, be.stream())
            sync(be)
            res.append([t.detach().cpu().clone() for t in (dx, dga, dbt)])
        assert all(bits_equal(a, b) for a, b in zip(*res)), "second launch differs"
        return res[0]
    seen = {}
    for p in PS:
        for seed in SEEDS:
            want = run(be.L.cdf_groupnorm_bwd_ex, p, seed)
            sd.fill_(seed)
            got = run(be.L.cdf_groupnorm_bwd_ex_sd, p, P(sd))
            for k, (a, b) in enumerate(zip(got, want)):
                assert bits_equal(a, b), (r, p, seed, ("dx", "dgamma", "dbeta")[k])
            seen[p, seed] = got[0].reshape(-1).tolist()
        assert len({tuple(v) for (q, _), v in seen.items() if q == p}) == len(SEEDS), "two seeds gave one mask"
    bad = [P(dy), lddy, P(x), ldx, P(ga), P(bt), P(mean), P(rstd), P(dx), lddx, P(dga), P(dbt), P(ws), B, HW, C, GROUPS, r.silu, r.accdx, r.accp]
    expect(be.L.cdf_groupnorm_bwd_ex_sd, bad + [1.0, P(sd), be.stream()], "dropout probability")
    expect(be.L.cdf_groupnorm_bwd_ex_sd, bad + [0.1, 0, be.stream()], "seed_dev")


def test_ops_take_a_device_seed(be):
    """colddiff.ops routes a one-element int64 tensor seed to the `_sd` entry points and an int to the originals: same result."""
    from colddiff import ops
    from emu_util import install_emu, uninstall_emu
    if be.kind == "emu":
        install_emu()
    try:
        torch.manual_seed(3)
        x = be.to(torch.randn(2, 4, 4, 32))
        ga, bt = be.to(torch.randn(32)), be.to(torch.randn(32))
        seed = (1 << 40) + 12345
        sd = seed_word(be, seed)
        assert bits_equal(ops.dropout(x, 0.25, sd).cpu(), ops.dropout(x, 0.25, seed).cpu())
        a = ops.groupnorm_fwd(x, ga, bt, 32, 1e-6, True, drop=(0.25, seed))
        b = ops.groupnorm_fwd(x, ga, bt, 32, 1e-6, True, drop=(0.25, sd))
        assert all(bits_equal(u.cpu(), v.cpu()) for u, v in zip(a, b))
        with pytest.raises(AssertionError):
            ops.dropout(x, 0.25, torch.zeros(2, dtype=torch.int64, device=x.device))
    finally:
        if be.kind == "emu":
            uninstall_emu()
