"""The four entry points of sampler graph mode (colddiff/graphsample.py), kernel by kernel on both backends:
cdf_noise_step_dev / cdf_blend_step_dev (the reverse step with t = step[0] + 1 read on the device), cdf_steps_advance (the device-side
step counter) and cdf_traj_put (the device-indexed trajectory store).

The `_dev` forms are compared with the host-`t` forms by torch.equal (they share one __device__ body): for every t in 1 .. T, the
t == 1 branch included, with the SAME arguments on every launch -- only the word is rewritten, as a replayed graph does.  Outputs are
carved from poison.Guarded buffers and every launch runs twice (test_degrade_kernels.run_twice).  The coefficient tables sit between
NaN guard bands, so a table read with an out-of-range word shows up as a NaN in `out`."""
import pytest
import torch

from colddiff._lib import CdfError
from emu_util import P
from poison import GUARD, Guarded, nan_empty
from test_degrade_kernels import _sync, images, run_twice

T = 6
HW = 16 * 16
SIZES = [3 * 16 * 16 * 4, 4099, 4096 * 256 + 257]        # the sampler test shape, an odd size, just past the element-wise grid cap (4096 blocks of 256)


def guarded_table(be, values):
    """`values` on the backend between two NaN bands of GUARD floats -> (the table view, the whole buffer kept alive by `be`)."""
    n = values.numel()
    buf = torch.full((2 * GUARD + n,), float("nan"))
    buf[GUARD:GUARD + n] = values.reshape(-1)
    d = be.to(buf)
    return d[GUARD:GUARD + n].view(values.shape)


def schedule(seed, *shape):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g) * 0.9 + 0.05            # (0.05, 0.95): cb is a divisor in the estimated-noise form


def word(be, v):
    return be.to(torch.tensor([v], dtype=torch.int64))


def noise_inputs(be, n):
    return (be.to(images(1, n)), be.to(images(2, n)), be.to(images(3, n)), guarded_table(be, schedule(4, T)), guarded_table(be, schedule(5, T)))


def blend_inputs(be, n):
    return (be.to(images(1, n)), be.to(images(2, n)), be.to(images(3, n)), guarded_table(be, schedule(4, T, HW)), guarded_table(be, schedule(5, T, HW)))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("est", [1, 0])
def test_noise_step_dev_equals_the_host_form(be, n, est):
    S = be.stream()
    img, x1, eps, ca, cb = noise_inputs(be, n)
    w = word(be, 0)
    for t in range(1, T + 1):
        ref = nan_empty(be, n)
        be.L.cdf_noise_step(P(img), P(x1), P(eps), P(ca), P(cb), t, est, P(ref), n, S)
        w.fill_(t - 1)
        (o,) = run_twice(be, (n,), 1, lambda o: be.L.cdf_noise_step_dev(P(img), P(x1), P(eps), P(ca), P(cb), P(w), T, est, P(o), n, S),
                         [img, x1, eps, ca, cb, w])
        assert torch.equal(o, ref.cpu()), (n, est, t)
    if est:                                                          # the estimated-noise form takes no noise tensor
        w.fill_(2)
        ref = nan_empty(be, n)
        be.L.cdf_noise_step(P(img), P(x1), 0, P(ca), P(cb), 3, 1, P(ref), n, S)
        (o,) = run_twice(be, (n,), 1, lambda o: be.L.cdf_noise_step_dev(P(img), P(x1), 0, P(ca), P(cb), P(w), T, 1, P(o), n, S), [img, x1, w])
        assert torch.equal(o, ref.cpu())


@pytest.mark.parametrize("n", SIZES)
def test_blend_step_dev_equals_the_host_form(be, n):
    S = be.stream()
    img, x1, x2, al, om = blend_inputs(be, n)
    w = word(be, 0)
    for t in range(1, T + 1):
        ref = nan_empty(be, n)
        be.L.cdf_blend_step(P(img), P(x1), P(x2), P(al), P(om), t, P(ref), HW, n, S)
        w.fill_(t - 1)
        (o,) = run_twice(be, (n,), 1, lambda o: be.L.cdf_blend_step_dev(P(img), P(x1), P(x2), P(al), P(om), P(w), T, P(o), HW, n, S),
                         [img, x1, x2, al, om, w])
        assert torch.equal(o, ref.cpu()), (n, t)


@pytest.mark.parametrize("bad", [-1, T])
def test_a_word_out_of_range_reads_no_table(be, bad):
    """out = img; a read of ca[-1] / ca[T] (or of the mask rows there) would be a NaN of the guard bands."""
    S, n = be.stream(), SIZES[1]
    img, x1, eps, ca, cb = noise_inputs(be, n)
    w = word(be, bad)
    for est in (1, 0):
        (o,) = run_twice(be, (n,), 1, lambda o: be.L.cdf_noise_step_dev(P(img), P(x1), P(eps), P(ca), P(cb), P(w), T, est, P(o), n, S),
                         [img, x1, eps, ca, cb, w])
        assert torch.equal(o, img.cpu())
    img, x1, x2, al, om = blend_inputs(be, n)
    (o,) = run_twice(be, (n,), 1, lambda o: be.L.cdf_blend_step_dev(P(img), P(x1), P(x2), P(al), P(om), P(w), T, P(o), HW, n, S),
                     [img, x1, x2, al, om, w])
    assert torch.equal(o, img.cpu())


@pytest.mark.parametrize("n", [1, 5, 1000])
def test_steps_advance(be, n):
    """words = max(words + delta, floor): the floor holds over repeated calls, nothing outside the n words is written."""
    S = be.stream()
    g = Guarded(be.device, (2 * n,), 1)                              # n int64 words = 2 n floats between the bands
    words = g.outs[0].view(torch.int64)
    start = torch.arange(n, dtype=torch.int64) % 7 - 1             # -1 .. 5
    runs = []
    for _ in range(2):
        g.poison()
        words.copy_(start)
        seen = []
        for k in range(1, 9):
            be.L.cdf_steps_advance(P(words), n, -1, -1, S)
            _sync(be)
            seen.append(words.cpu().clone())
            assert torch.equal(seen[-1], (start - k).clamp(min=-1)), k
        be.L.cdf_steps_advance(P(words), n, 3, 1, S)                # upwards, and a floor above the sum
        _sync(be)
        seen.append(words.cpu().clone())
        assert torch.equal(seen[-1], torch.full((n,), 2, dtype=torch.int64))
        assert g.guards_intact(), "a guard band was written"
        runs.append(torch.stack(seen))
    assert torch.equal(runs[0], runs[1])


def test_traj_put(be):
    S, slots, per = be.stream(), 5, 3 * 16 * 16 * 4 + 3
    src = be.to(images(7, per))
    g = Guarded(be.device, (slots, per), 1)
    slab = g.outs[0]
    w = word(be, 0)
    for slot in range(-1, slots + 1):
        w.fill_(slot)
        got = []
        for _ in range(2):
            g.poison()
            be.L.cdf_traj_put(P(slab), P(src), per, P(w), slots, S)
            _sync(be)
            assert g.guards_intact(), "a guard band was written"
            got.append(slab.cpu().clone())
        a, b = got
        for r in range(slots):
            if r == slot:
                assert torch.equal(a[r], src.cpu()) and torch.equal(b[r], src.cpu()), slot
            else:
                assert bool(torch.isnan(a[r]).all()) and bool(torch.isnan(b[r]).all()), (slot, r)   # the other rows / every row: untouched
        assert torch.equal(src.cpu(), images(7, per)) and int(w.item()) == slot


def test_bad_arguments_are_a_status_not_a_launch(be):
    S, n = be.stream(), 64
    buf = nan_empty(be, 4 * n)
    p, w = P(buf), P(word(be, 0))
    L = be.L
    cases = [(L.cdf_noise_step_dev, [0, p, p, p, p, w, T, 1, p, n, S]), (L.cdf_noise_step_dev, [p, p, p, p, p, 0, T, 1, p, n, S]),
             (L.cdf_noise_step_dev, [p, p, p, p, p, w, 0, 1, p, n, S]), (L.cdf_noise_step_dev, [p, p, p, p, p, w, T, 1, p, 0, S]),
             (L.cdf_noise_step_dev, [p, p, 0, p, p, w, T, 0, p, n, S]),          # the fixed-noise form without its noise tensor
             (L.cdf_noise_step_dev, [p, p, p, p, p, w, T, 1, 0, n, S]),
             (L.cdf_blend_step_dev, [p, p, 0, p, p, w, T, p, 16, n, S]), (L.cdf_blend_step_dev, [p, p, p, p, p, 0, T, p, 16, n, S]),
             (L.cdf_blend_step_dev, [p, p, p, p, p, w, 0, p, 16, n, S]), (L.cdf_blend_step_dev, [p, p, p, p, p, w, T, p, 16, -1, S]),
             (L.cdf_blend_step_dev, [p, p, p, p, p, w, T, p, 0, n, S]),
             (L.cdf_steps_advance, [0, 4, -1, -1, S]), (L.cdf_steps_advance, [w, 0, -1, -1, S]),
             (L.cdf_traj_put, [0, p, n, w, 2, S]), (L.cdf_traj_put, [p, 0, n, w, 2, S]), (L.cdf_traj_put, [p, p, n, 0, 2, S]),
             (L.cdf_traj_put, [p, p, 0, w, 2, S]), (L.cdf_traj_put, [p, p, n, w, 0, S])]
    for fn, args in cases:
        with pytest.raises(CdfError, match="bad args|needs the noise tensor"):
            fn(*args)
    _sync(be)
    assert bool(torch.isnan(buf).all()), "a refused call wrote"


@pytest.mark.parametrize("be", [pytest.param("hip", marks=pytest.mark.gpu)], indirect=True)
def test_production_shape(be):
    """16 x 3 x 128 x 128, the sampler shape of the bench configuration: T = 200 tables, first, middle and last step."""
    S, n, T2, hw = be.stream(), 16 * 3 * 128 * 128, 200, 128 * 128
    img, x1, x2 = be.to(images(1, n)), be.to(images(2, n)), be.to(images(3, n))
    ca, cb = guarded_table(be, schedule(4, T2)), guarded_table(be, schedule(5, T2))
    al, om = guarded_table(be, schedule(6, T2, hw)), guarded_table(be, schedule(7, T2, hw))
    w = word(be, 0)
    for t in (1, 2, 117, T2):
        w.fill_(t - 1)
        for est in (1, 0):
            ref = nan_empty(be, n)
            be.L.cdf_noise_step(P(img), P(x1), P(x2), P(ca), P(cb), t, est, P(ref), n, S)
            (o,) = run_twice(be, (n,), 1, lambda o: be.L.cdf_noise_step_dev(P(img), P(x1), P(x2), P(ca), P(cb), P(w), T2, est, P(o), n, S),
                             [img, x1, x2, w])
            assert torch.equal(o, ref.cpu()), (t, est)
        ref = nan_empty(be, n)
        be.L.cdf_blend_step(P(img), P(x1), P(x2), P(al), P(om), t, P(ref), hw, n, S)
        (o,) = run_twice(be, (n,), 1, lambda o: be.L.cdf_blend_step_dev(P(img), P(x1), P(x2), P(al), P(om), P(w), T2, P(o), hw, n, S),
                         [img, x1, x2, w])
        assert torch.equal(o, ref.cpu()), t
