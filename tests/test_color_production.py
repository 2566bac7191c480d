"""cdf_color_chain at the shapes the decolorization package launches on the MI355X: the training `q_sample` (64 x 3 x 128 x 128, T = 50,
random t, total requested) and the sampler's Algorithm-2 combine at 16 images, RGB and Lab.  Every output sits inside ONE poisoned
allocation between guard bands; each launch runs twice and must be bit-identical; the guard bands and the inputs must come back untouched
(nothing outside the outputs is written).  References: the sequential CPU restatement of tests/decolor_ref.py on a sample of images.
"""
import pytest
import torch

import decolor_ref as R
from emu_util import P
from poison import GUARD, Guarded  # noqa: F401  (GUARD: the module kept the name)
from test_color_kernels import LAB_CHAIN_TOL, LAB_SCALE, RGB_CHAIN_TOL
from test_kernels_production import bits_equal, sample

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    """The hardware backend only (these shapes are out of the simulator's reach; the simulator runs the same code paths at small
    shapes in test_color_kernels.py)."""
    from conftest import Backend
    return Backend("hip")


def _run_twice(g, launch):
    res = []
    for _ in range(2):
        g.poison()
        launch()
        torch.cuda.synchronize()
        assert g.guards_intact(), "a guard band was written"
        res.append([o.cpu().clone() for o in g.outs])
    for a, b in zip(*res):
        assert bits_equal(a, b), "second launch differs"
        assert torch.isfinite(a).all(), "an output element was left unwritten"
    return res[0]


@pytest.mark.parametrize("lab", [False, True])
def test_training_q_sample_shape(be, lab):
    B, H, W, T = 64, 128, 128, 50
    g0 = torch.Generator().manual_seed(21)
    x = torch.rand((B, 3, H, W), generator=g0) * 2 - 1
    if lab:
        x = R.rgb2lab_t(x)
    t = torch.randint(0, T, (B,), generator=g0)
    t[0], t[1] = T - 1, 0
    nb = (t + 1).tolist()
    nmax = int(t.max()) + 1
    table = R.table_of("Constant", T)
    dx, dw, dn = be.to(x), be.to(table), be.to(torch.tensor(nb, dtype=torch.int64))
    keep = dx.clone()
    g = Guarded(be.device, x.shape, 2)
    y, total = g.outs
    got_y, got_t = _run_twice(g, lambda: be.L.cdf_color_chain(P(dx), P(y), P(total), 0, 0, P(dw), P(dn), B, 3, H * W, T, 0, nmax,
                                                              1 if lab else 0, be.stream()))
    assert torch.equal(dx, keep), "the input was written"
    rows = sample(B) + [1]
    err = (lambda a, b: ((a - b).abs() / LAB_SCALE).max().item()) if lab else (lambda a, b: (a - b).abs().max().item())
    tol = LAB_CHAIN_TOL if lab else RGB_CHAIN_TOL
    e_y = err(got_y[rows], R.chain_t(x[rows], table, [nb[r] for r in rows], lab))
    e_t = err(got_t[rows], R.chain_t(x[rows], table, nmax, lab))
    print(f"q_sample 64x3x128x128 lab={lab}: y {e_y:.3g}, total {e_t:.3g} (tolerance {tol:.3g})")
    assert e_y <= tol and e_t <= tol
    if not lab:                      # row 0 ran the total-removal step: grey, bit for bit
        assert torch.equal(got_y[0, 0], got_y[0, 1]) and torch.equal(got_y[0, 0], got_y[0, 2])


@pytest.mark.parametrize("lab", [False, True])
def test_sampler_combine_shape(be, lab):
    B, H, W, T = 16, 128, 128, 50
    g0 = torch.Generator().manual_seed(22)
    x, img = torch.rand((B, 3, H, W), generator=g0) * 2 - 1, torch.rand((B, 3, H, W), generator=g0) * 2 - 1
    if lab:
        x, img = R.rgb2lab_t(x), R.rgb2lab_t(img)
    table = R.table_of("Linear", T)
    step = 37
    dx, di, dw = be.to(x), be.to(img), be.to(table)
    keep_x, keep_i = dx.clone(), di.clone()
    g = Guarded(be.device, x.shape, 2)
    y, snap = g.outs
    got_y, got_s = _run_twice(g, lambda: be.L.cdf_color_chain(P(dx), P(y), 0, P(snap), P(di), P(dw), 0, B, 3, H * W, T, step, step,
                                                              1 if lab else 0, be.stream()))
    assert torch.equal(dx, keep_x) and torch.equal(di, keep_i), "an input was written"
    rows = sample(B)
    xn, xs = R.chain_t(x[rows], table, step, lab), R.chain_t(x[rows], table, step - 1, lab)
    err = (lambda a, b: ((a - b).abs() / LAB_SCALE).max().item()) if lab else (lambda a, b: (a - b).abs().max().item())
    tol = LAB_CHAIN_TOL if lab else RGB_CHAIN_TOL
    e_s, e_y = err(got_s[rows], xs), err(got_y[rows], (img[rows] - xn) + xs)
    print(f"combine 16x3x128x128 lab={lab}: snap {e_s:.3g}, y {e_y:.3g} (tolerance {tol:.3g}, y: three terms)")
    assert e_s <= tol and e_y <= 3 * tol
