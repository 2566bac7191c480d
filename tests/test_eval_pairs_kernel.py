"""`cdf_eval_pairs_partial` (csrc/k_metrics.hip): the originals against up to four candidate sets in one pass -- per candidate the SSIM
partial sums of `cdf_ssim_partial`, bit for bit, and the squared error with every pixel owned by exactly one tile.  Simulator and MI355X.

Shapes (planes = 6): 11 x 11 one output position; 16 x 16 the golden size; 42 x 42 one tile that owns through the edge; 43 x 43 a second
tile with one valid output and an 11-wide owned strip; 32 x 75 non-square; 128 x 128 the production size, 4 x 4 tiles.

Squared-error bound: a tile's fp32 sum of at most 42^2 = 1764 non-negative terms, in any order, is within 1764 * 2^-24 of the exact sum,
relatively; so is the fp64 sum of the tiles.  A pixel counted twice or not at all at 42 / 43 wide moves the sum by >= 2 %.
"""
import ctypes

import pytest
import torch

from colddiff import metrics
from colddiff._lib import CdfError
from emu_util import P
from poison import nan_empty

PLANES = 6
SHAPES = [(11, 11), (16, 16), (42, 42), (43, 43), (32, 75), (128, 128)]
SSE_REL = 1764 * 2.0 ** -24
C1, C2 = 0.01 ** 2, 0.03 ** 2


def _win():
    return (ctypes.c_float * 11)(*metrics._gauss_window(11, 1.5).tolist())


_inputs = {}


def inputs(H, W):
    """x and four candidates in [-1, 1], [PLANES, H, W] (8-bit levels, as images are); made once per shape and left unchanged."""
    if (H, W) not in _inputs:
        g = torch.Generator().manual_seed(1000 * H + W)
        x = torch.randint(0, 256, (PLANES, H, W), generator=g).float() / 255 * 2 - 1
        cands = [(x + s * torch.randn(PLANES, H, W, generator=g)).clamp(-1, 1) for s in (0.5, 0.1, 0.02, 1.0)]
        _inputs[(H, W)] = (x, cands)
    return _inputs[(H, W)]


def run(be, x, cands, shift, H, W):
    K = len(cands)
    tiles = be.L.cdf_ssim_tiles(H, W)
    ss, se = nan_empty(be, K, PLANES, tiles), nan_empty(be, K, PLANES, tiles)
    dx, dc = be.to(x), [be.to(c) for c in cands]
    be.L.cdf_eval_pairs_partial(P(dx), *([P(c) for c in dc] + [0] * (4 - K)), K, shift, P(ss), P(se), PLANES, H, W, _win(), C1, C2, be.stream())
    return ss.cpu(), se.cpu()


def ssim_partial(be, a, b, H, W):
    out = nan_empty(be, PLANES, be.L.cdf_ssim_tiles(H, W))
    be.L.cdf_ssim_partial(P(be.to(a)), P(be.to(b)), P(out), PLANES, H, W, _win(), C1, C2, be.stream())
    return out.cpu()


@pytest.mark.parametrize("K", [1, 3, 4])
@pytest.mark.parametrize("H,W", SHAPES)
def test_against_ssim_partial_and_the_exact_squared_error(be, H, W, K):
    x, cands = inputs(H, W)
    cands = cands[:K]
    sx, sc = (x + 1) * 0.5, [(c + 1) * 0.5 for c in cands]                      # one rounding, as the kernel's load
    ss, se = run(be, x, cands, 1, H, W)
    ss0, se0 = run(be, sx, sc, 0, H, W)
    assert torch.isfinite(ss).all() and torch.isfinite(se).all(), "poison left in the outputs"
    assert torch.equal(ss, ss0) and torch.equal(se, se0), "shift=1 on the stored form differs from shift=0 on the shifted tensors"
    for k in range(K):
        assert torch.equal(ss[k], ssim_partial(be, sx, sc[k], H, W)), (k, "SSIM partials are not those of cdf_ssim_partial")
        want = ((sx - sc[k]) ** 2).double().sum().item()
        got = se[k].double().sum().item()
        rel = abs(got - want) / want
        print(f"eval_pairs sse [{be.kind}] {H}x{W} K={K} k={k}: relative difference {rel:.3g} (bound {SSE_REL:.3g})")
        assert rel <= SSE_REL, (k, got, want)
        # per plane too: a pixel moved from one plane's count to another's would cancel in the total
        wp = ((sx - sc[k]) ** 2).double().sum((1, 2))
        assert ((se[k].double().sum(1) - wp).abs() / wp).max().item() <= SSE_REL


@pytest.mark.parametrize("H,W", SHAPES)
def test_a_candidate_equal_to_the_original(be, H, W):
    x, cands = inputs(H, W)
    ss, se = run(be, x, [cands[0], x, cands[1]], 1, H, W)
    assert torch.equal(se[1], torch.zeros_like(se[1]))
    sx = (x + 1) * 0.5
    assert torch.equal(ss[1], ssim_partial(be, sx, sx, H, W))
    assert (se[0] > 0).all() and (se[2] > 0).all()                                # every tile owns pixels, the neighbours are untouched


def test_bad_arguments_are_a_status_with_the_message(be):
    x = be.to(torch.zeros(PLANES, 16, 16))
    out = be.empty(4, PLANES, 1)
    L, w, st = be.L, _win(), be.stream()
    with pytest.raises(CdfError, match="K must be 1...4"):
        L.cdf_eval_pairs_partial(P(x), P(x), 0, 0, 0, 0, 1, P(out), P(out), PLANES, 16, 16, w, C1, C2, st)
    with pytest.raises(CdfError, match="K must be 1...4"):
        L.cdf_eval_pairs_partial(P(x), P(x), P(x), P(x), P(x), 5, 1, P(out), P(out), PLANES, 16, 16, w, C1, C2, st)
    with pytest.raises(CdfError, match=r"null pointer \(candidate 1 of 2\)"):
        L.cdf_eval_pairs_partial(P(x), P(x), 0, 0, 0, 2, 1, P(out), P(out), PLANES, 16, 16, w, C1, C2, st)
    with pytest.raises(CdfError, match="null pointer"):
        L.cdf_eval_pairs_partial(0, P(x), 0, 0, 0, 1, 1, P(out), P(out), PLANES, 16, 16, w, C1, C2, st)
    with pytest.raises(CdfError, match="null pointer"):
        L.cdf_eval_pairs_partial(P(x), P(x), 0, 0, 0, 1, 1, P(out), 0, PLANES, 16, 16, w, C1, C2, st)
    with pytest.raises(CdfError, match="at least 11 x 11 \\(got 10 x 16\\)"):
        L.cdf_eval_pairs_partial(P(x), P(x), 0, 0, 0, 1, 1, P(out), P(out), PLANES, 10, 16, w, C1, C2, st)
    with pytest.raises(CdfError, match="at least 11 x 11"):
        L.cdf_eval_pairs_partial(P(x), P(x), 0, 0, 0, 1, 1, P(out), P(out), PLANES, 16, 10, w, C1, C2, st)
