"""The snow kernels of csrc/k_snow.hip -- cdf_snow_chain, cdf_snow_layers -- on the simulator (`-m "not gpu"`) and on the MI355X (`-m gpu`)
through `be`, into poisoned buffers.

Chain: `torch.equal` with tests/snow_ref.py's `state_t`.  The kernel evaluates the restatement's expressions in the restatement's order
without contraction, and the restatement is bit-equal to the live reference (tests/test_snow_golden.py).  Every case asserts that the
plane it reads has non-zero pixels and that some but not all output pixels reach the clip at 1: a kernel that dropped the snow term or
the clip would not pass.  The planes are the reference's own (tests/golden/snow/snow_cases.pt).

Layers: max-abs <= 2e-6 against the fixture planes.  The bound is derived, not tuned: the outputs lie in [0, 1]; a k-term fp32 dot product
with weights summing to 1 errs by at most k * 2^-24 <= 6.6e-7 for k = 11; twice that covers the reference's unknown summation order.
Measured (printed by the test): simulator 1.19e-7, MI355X 1.19e-7; the CPU restatement `layers_t` is 1.19e-7 from the live reference.
"""
import os

import pytest
import torch

import snow_ref as R
from emu_util import P
from poison import nan_empty

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "snow")
LAYER_TOL = 2e-6
T = 20
_cases = None


def cases():
    global _cases
    if _cases is None:
        _cases = torch.load(os.path.join(GOLD, "snow_cases.pt"), weights_only=False)
    return _cases


def _rgb(B, H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand((B, 3, H, W), generator=g) * 2 - 1


def taps_of(sigmas, k):
    return torch.stack([R.get_gaussian_kernel(k, s) for s in sigmas])


def planes_for(H, W, L, level=1):
    """([T,L,H,W] planes, br list) made by the restatement from the fixture's 32 x 32 bases (the four `single_snow` layers, then the plain
    one), cut to H x W around the first layer's brightest pixel so that even the first step's plane of a small cut has snow in it."""
    single, plain = cases()["layers"][f"L{level}_32_single"], cases()["layers"][f"L{level}_32_plain"]
    base = torch.cat([single["base"], plain["base"]])[:L]
    vertical = torch.cat([single["vertical"], plain["vertical"]], dim=1)[:, :L]
    at = int(base[0].argmax())
    y0, x0 = min(max(at // 32 - H // 2, 0), 32 - H), min(max(at % 32 - W // 2, 0), 32 - W)
    base = base[:, y0:y0 + H, x0:x0 + W].contiguous()
    k = 5 if level == 1 else 11
    planes = R.layers_t(base, torch.tensor(single["snow_thres_list"]), taps_of(single["mb_sigma_list"], k), vertical)
    return planes, single["br_coef_list"]


def run_chain(be, og, planes, br, n=0, nb=None, nmax=0, start=None, total=False, snap=False, img=None, layers=None, fix=False, twice=False):
    """-> dict of the outputs of one cdf_snow_chain launch on poisoned buffers (CPU tensors); `twice`: launched a second time into the
    same buffers, which must leave the same bits."""
    B, _, H, W = og.shape
    Tn, L = planes.shape[0], planes.shape[1]
    dog, dpl = be.to(og), be.to(planes)
    dbr = be.to(torch.tensor(br, dtype=torch.float32))
    domb = be.to(torch.tensor([1.0 - v for v in br], dtype=torch.float32))
    dn = None if nb is None else be.to(torch.as_tensor(nb, dtype=torch.int64))
    dl = None if layers is None else be.to(torch.as_tensor(layers, dtype=torch.int64))
    ds = None if start is None else be.to(start)
    di = None if img is None else be.to(img)
    y = nan_empty(be, *og.shape)
    tt = nan_empty(be, *og.shape) if total else None
    ss = nan_empty(be, *og.shape) if snap else None

    def launch():
        be.L.cdf_snow_chain(P(dog), P(ds), P(y), P(tt), P(ss), P(di), P(dpl), P(dbr), P(domb), P(dn), P(dl), B, H * W, L, Tn, n, nmax,
                            1 if fix else 0, be.stream())
        return {k: (None if v is None else v.cpu().clone()) for k, v in (("y", y), ("total", tt), ("snap", ss))}
    out = launch()
    if twice:
        again = launch()
        for k, v in out.items():
            assert v is None or torch.equal(v, again[k]), k
    return out


def covered(planes, steps, out):
    """The coverage conditions: the planes read are not empty, and some but not all output pixels sit at the clip."""
    for s in steps:
        assert (planes[s] != 0).any(), f"the plane of step {s} is all zero"
    at_clip = (out == 1.0).float().mean().item()
    assert 0.0 < at_clip < 1.0, at_clip
    return at_clip


COUNTS = [0, T, 8, -1, 1]


@pytest.mark.parametrize("H,W,L", [(5, 7, 1), (8, 8, 1), (32, 32, 1), (32, 32, 5)])
@pytest.mark.parametrize("fix", [False, True])
def test_chain_per_row_counts_and_scalar_count(be, H, W, L, fix):
    planes, br = planes_for(H, W, L)
    og, start = _rgb(5, H, W, seed=1), _rgb(5, H, W, seed=2)
    out = run_chain(be, og, planes, br, nb=COUNTS, start=start, fix=fix, twice=True)["y"]
    want = R.state_t(og, start, COUNTS, planes, br, fix=fix)
    assert torch.equal(out, want)
    assert torch.equal(out[0], start[0]) and torch.equal(out[3], og[3])          # zero steps: start; negative: the row of og
    frac = covered(planes, (T - 1, 7, 0), out[[1, 2, 4]])
    print(f"chain {H}x{W} L={L} fix={fix} [{be.kind}]: bit-equal, {100 * frac:.1f} % of the degraded pixels at the clip")
    out = run_chain(be, og, planes, br, nb=COUNTS, fix=fix)["y"]                  # start == NULL: a zero-step row is og
    assert torch.equal(out, R.state_t(og, None, COUNTS, planes, br, fix=fix))
    for n in (8, T, 0):                                                           # the scalar count (nsteps_b == NULL)
        assert torch.equal(run_chain(be, og, planes, br, n=n, fix=fix)["y"], R.state_t(og, None, n, planes, br, fix=fix)), n


def test_chain_at_the_clip_rate_of_the_reference_planes(be):
    """Level 1, T = 20, step 7, 32 x 32: 9 ... 10 % of the pixels clip (measured on the CPU with the reference)."""
    c = cases()
    planes = torch.zeros(T, 1, 32, 32)
    lay = c["layers"]["L1_32_plain"]
    planes[7] = lay["planes"][lay["steps"].index(7)]
    x = c["forward"]["x32"]
    out = run_chain(be, x, planes, lay["br_coef_list"], n=8)["y"]
    assert torch.equal(out, c["forward"]["L1_32"]["forward_7"])                   # the reference's own output, bit for bit
    frac = covered(planes, (7,), out)
    assert 0.09 <= frac <= 0.10, frac


def test_chain_layer_permutation(be):
    planes, br = planes_for(32, 32, 5)
    og = _rgb(5, 32, 32, seed=3)
    perm = [3, 0, 4, 1, 2]
    nb = [T, 8, 1, 3, 12]
    out = run_chain(be, og, planes, br, nb=nb, layers=perm, twice=True)["y"]
    assert torch.equal(out, R.state_t(og, None, nb, planes, br, layers=perm))
    assert not torch.equal(out, R.state_t(og, None, nb, planes, br))              # (the layers differ: the permutation matters)
    covered(planes, (T - 1, 7, 0, 2, 11), out)
    # more rows than layers needs layer_b
    out = run_chain(be, torch.cat([og, og]), planes, br, n=8, layers=perm + perm)["y"]
    assert torch.equal(out[:5], out[5:])


@pytest.mark.parametrize("H,W", [(5, 7), (8, 8)])
@pytest.mark.parametrize("nmax", [T, 9, 1, 0])
def test_chain_total_snap_and_combine(be, H, W, nmax):
    planes, br = planes_for(H, W, 1)
    og, start, img = _rgb(5, H, W, seed=4), _rgb(5, H, W, seed=5), _rgb(5, H, W, seed=6)
    exp_y = R.state_t(og, start, COUNTS, planes, br)
    exp_t = R.state_t(og, start, [nmax if v >= 0 else -1 for v in COUNTS], planes, br)
    exp_s = R.state_t(og, start, [max(min(v, nmax - 1), 0) if v >= 0 else -1 for v in COUNTS], planes, br)
    covered(planes, (T - 1, 7, 0), exp_y[[1, 2, 4]])
    for total, snap in ((True, False), (False, True), (True, True)):              # each alone and together
        out = run_chain(be, og, planes, br, nb=COUNTS, nmax=nmax, start=start, total=total, snap=snap, twice=True)
        assert torch.equal(out["y"], exp_y)
        assert (out["total"] is None) == (not total) and (out["snap"] is None) == (not snap)
        assert not total or torch.equal(out["total"], exp_t)
        assert not snap or torch.equal(out["snap"], exp_s)
    for snap in (False, True):                                                    # Algorithm 2's combine, in that association
        out = run_chain(be, og, planes, br, nb=COUNTS, nmax=nmax, start=start, img=img, snap=snap, twice=True)
        assert torch.equal(out["y"], (img - exp_y) + exp_s)
        assert not snap or torch.equal(out["snap"], exp_s)


@pytest.mark.parametrize("t", [[3, 5, 0, 5], [0, 0, 0, 0], [2, 2, 2, 2]])
def test_combine_mirrors_the_reference_loop(be, t):
    """`x0_step_down` of sample_one_step (diffusion.py:221-237) restated with its loop: forward() ignores its first argument, so the noise
    added to the prediction survives only in the rows that take zero steps -- which is what `start` carries."""
    planes, br = planes_for(8, 8, 1)
    x, img = _rgb(4, 8, 8, seed=7), _rgb(4, 8, 8, seed=8)
    noisy = x + 0.05 * _rgb(4, 8, 8, seed=9)
    tt = torch.tensor(t)
    x_times = noisy.clone()
    x_sub = x_times.clone()
    cur = torch.zeros_like(tt)
    idx = torch.where(cur < tt)[0]
    for i in range(int(tt.max())):
        x_sub = x_times.clone()
        x_times[idx] = R.degrade_t(x[idx], planes[i][None], br, i)
        cur += 1
        idx = torch.where(cur < tt)[0]
    out = run_chain(be, x, planes, br, nb=t, nmax=int(tt.max()), start=noisy, img=img, snap=True)
    assert torch.equal(out["snap"], x_sub)
    assert torch.equal(out["y"], (img - x_times) + x_sub)


def _layers(be, base, thres, taps, vertical):
    L, H, W = base.shape
    Tn, k = taps.shape
    out = nan_empty(be, Tn, L, H, W)
    be.L.cdf_snow_layers(P(be.to(base)), P(be.to(thres)), P(be.to(taps)), P(be.to(vertical)), P(out), H, W, L, Tn, k, be.stream())
    return out.cpu()


@pytest.mark.parametrize("size", [13, 32])
@pytest.mark.parametrize("level", [1, 2, 3, 4])                                   # k = 5 at level 1, k = 11 (a halo of most of a 13-pixel row) above
def test_layers_against_the_reference_planes(be, size, level):
    worst = 0.0
    for kind in ("plain", "single"):                                              # one direction for every layer / mixed flags, L = 4
        c = cases()["layers"][f"L{level}_{size}_{kind}"]
        k = 5 if level == 1 else 11
        got = _layers(be, c["base"], torch.tensor(c["snow_thres_list"]), taps_of(c["mb_sigma_list"], k), c["vertical"])
        e = (got[list(c["steps"])] - c["planes"]).abs().max().item()
        assert (c["planes"] != 0).any() and got.min().item() >= 0.0 and got.max().item() <= 1.0 + LAYER_TOL
        if kind == "single":
            assert 0 < int(c["vertical"].sum()) < c["vertical"].numel()
        worst = max(worst, e)
        assert e <= LAYER_TOL, (kind, e)
    print(f"snow layers level {level} {size}x{size} [{be.kind}]: max-abs {worst:.3g} (bound {LAYER_TOL:.3g})")


@pytest.mark.parametrize("flag", [0, 1])
def test_layers_direction_flags_and_empty_plane(be, flag):
    """All-horizontal and all-vertical flags on the same 4-layer base against the restatement, a non-square image, and one threshold above
    every base value: that plane is zero exactly."""
    c = cases()["layers"]["L2_13_single"]
    base = c["base"][:, :13, :11].contiguous()
    thres = torch.tensor(c["snow_thres_list"])
    thres[5] = base.max().item() + 1.0
    taps = taps_of(c["mb_sigma_list"], 11)
    vertical = torch.full((T, 4), flag, dtype=torch.uint8)
    got = _layers(be, base, thres, taps, vertical)
    want = R.layers_t(base, thres, taps, vertical)
    e = (got - want).abs().max().item()
    print(f"snow layers all-{'vertical' if flag else 'horizontal'} 13x11 [{be.kind}]: max-abs {e:.3g} against the restatement")
    assert e <= LAYER_TOL and (want != 0).any()
    assert torch.equal(got[5], torch.zeros(4, 13, 11))
    other = _layers(be, base, thres, taps, 1 - vertical)
    assert not torch.equal(other, got)                                            # (the direction is read)


def test_argument_checks_return_a_status(be):
    from colddiff._lib import CdfError
    planes, br = planes_for(8, 8, 2)
    x = be.to(_rgb(2, 8, 8))
    y = be.empty(2, 3, 8, 8)
    dp, dbr = be.to(planes), be.to(torch.tensor(br, dtype=torch.float32))
    st = be.stream()
    chain = lambda *a: be.L.cdf_snow_chain(*a, st)
    bad = [
        (lambda: chain(0, 0, P(y), 0, 0, 0, P(dp), P(dbr), P(dbr), 0, 0, 2, 64, 2, T, 1, 0, 0), "null pointer"),
        (lambda: chain(P(x), 0, 0, 0, 0, 0, P(dp), P(dbr), P(dbr), 0, 0, 2, 64, 2, T, 1, 0, 0), "null pointer"),
        (lambda: chain(P(x), 0, P(y), 0, 0, 0, 0, P(dbr), P(dbr), 0, 0, 2, 64, 2, T, 1, 0, 0), "null pointer"),
        (lambda: chain(P(x), 0, P(y), 0, 0, 0, P(dp), P(dbr), P(dbr), 0, 0, 2, 64, 2, T, T + 1, 0, 0), "exceeds"),
        (lambda: chain(P(x), 0, P(y), 0, 0, 0, P(dp), P(dbr), P(dbr), 0, 0, 2, 64, 2, T, 1, T + 1, 0), "exceeds"),
        (lambda: chain(P(x), 0, P(y), 0, 0, 0, P(dp), P(dbr), P(dbr), 0, 0, 3, 64, 2, T, 1, 0, 0), "no layer_b"),
        (lambda: chain(P(x), 0, P(y), P(y), 0, P(x), P(dp), P(dbr), P(dbr), 0, 0, 2, 64, 2, T, 1, 1, 0), "exclude"),
        (lambda: chain(P(x), 0, P(y), 0, 0, 0, P(dp), P(dbr), P(dbr), 0, 0, 2, 64, 2, 2000, 1, 0, 0), "1..1024"),
        (lambda: be.L.cdf_snow_layers(P(x), P(dbr), P(dbr), 0, P(y), 8, 8, 1, 1, 5, st), "null pointer"),
        (lambda: be.L.cdf_snow_layers(P(x), P(dbr), P(dbr), P(x), P(y), 8, 8, 1, 1, 4, st), "odd tap count"),
        (lambda: be.L.cdf_snow_layers(P(x), P(dbr), P(dbr), P(x), P(y), 8, 8, 700, 100, 5, st), "1..65535"),
    ]
    for call, text in bad:
        with pytest.raises(CdfError, match=text):
            call()
    chain(P(x), 0, P(y), 0, 0, 0, P(dp), P(dbr), P(dbr), 0, 0, 2, 64, 2, T, T, 0, 0)
    assert torch.isfinite(y.cpu()).all()
