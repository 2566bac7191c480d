"""`cdf_moments_merge_f64` (csrc/k_fid.hip): accumulator b of `cdf_moments_f64`, re-centred on a's pivot, added to accumulator a.
Simulator and MI355X.

Exact tests: the rows are integers in [-8, 8] and both pivots are means of a power-of-two number of rows (<= 8), so every centred value,
every delta = pivot_b - pivot_a and every product is a dyadic rational with a denominator <= 64 and a magnitude far below 2^53 / 64: fp64
is exact in any order, and the merge of moments(A, pivot_a) and moments(B, pivot_b) must `==` ONE cdf_moments_f64 pass over cat(A, B) on
pivot_a -- in sum and in every owned element of outer (the 64 x 64 tiles of the upper block triangle, a diagonal tile whole).
Random data, bound derived (not measured), R = max |x - pivot| over all rows and both pivots, n = n_a + n_b:
    |dcov| <= 16 n 2^-53 R^2,   |dmean| <= 8 n 2^-53 R
twice the bound tests/test_fid_kernels.py derives for one accumulator: the re-centring adds four products of two roundings each, every
one at most n_b R^2 (|delta| <= 2 R is covered by the factor), to the two gamma_n sums.
"""
import numpy as np
import pytest
import torch

from colddiff._lib import CdfError
from emu_util import P
from poison import poison_
from test_fid_kernels import U, _hip, int_features, moments, new_outer, owned_mask

# (d, n_a, n_b, ldo_a, ldo_b)
EXACT_SHAPES = [(40, 24, 13, 40, 48),            # one tile, d off the tile, pitches differ
                (72, 7, 50, 80, 72),             # two tiles: the off-diagonal tile (0, 1)
                (130, 16, 16, 136, 130),         # three tiles: tile (0, 2)
                (72, 16, 1, 72, 72)]             # n_b = 1


def merge(be, nb, pb, sb, ob, ldo_b, pa, sa, oa, ldo_a, d):
    be.L.cdf_moments_merge_f64(float(nb), P(pb), P(sb), P(ob), ldo_b, P(pa), P(sa), P(oa), ldo_a, d, be.stream())


def dyadic_pivot(x, d):
    """The mean of the first 2^k <= min(n, 8) rows: what FidStats takes as its pivot, with a power-of-two first batch."""
    k = 1
    while 2 * k <= min(x.shape[0], 8):
        k *= 2
    return x[:k, :d].double().mean(0)


def accumulate(be, x, d, pivot, ldo, pad=5):
    """moments(x, pivot) in poisoned accumulators: sum [d + pad] (zero up to d), outer [d + 3, ldo] (zero in the owned tiles)."""
    s = poison_(torch.empty(d + pad, device=be.device, dtype=torch.float64))
    s[:d] = 0
    o = new_outer(be, d, ldo)
    moments(be, be.to(x), x.shape[0], d, x.shape[1], pivot, s, o, ldo)
    return s, o


def same_owned(d, s, o, s_want, o_want, what):
    """sum[:d] and the owned elements of outer `==`; everything else of both accumulators still poison."""
    s, o, s_want, o_want = s.cpu(), o.cpu(), s_want.cpu(), o_want.cpu()
    assert torch.equal(s[:d], s_want[:d]), what + ": sum"
    assert torch.isnan(s[d:]).all(), what + ": sum written past d"
    own = owned_mask(d, o.shape[0], o.shape[1])
    assert torch.isnan(o[~own]).all(), what + ": written outside [d, d] or below the block triangle's tiles"
    assert not torch.isnan(o[own]).any() and torch.equal(o[own], o_want[owned_mask(d, o_want.shape[0], o_want.shape[1])]), what + ": outer"


def check_exact(be, d, n_a, n_b, ldo_a, ldo_b, same_pivot=False):
    A, B = int_features(n_a, d, d + 3, 7 * d + n_a), int_features(n_b, d, d, 7 * d + n_b + 1)
    pa = be.to(dyadic_pivot(A, d))
    pb = pa.clone() if same_pivot else be.to(dyadic_pivot(B, d))
    sa, oa = accumulate(be, A, d, pa, ldo_a)
    sb, ob = accumulate(be, B, d, pb, ldo_b, pad=2)
    keep = [t.clone() for t in (sb, ob, pa, pb)]
    merge(be, n_b, pb, sb, ob, ldo_b, pa, sa, oa, ldo_a, d)
    cat = torch.cat((A[:, :d], B[:, :d]))
    s1, o1 = accumulate(be, cat, d, pa, ldo_a)
    same_owned(d, sa, oa, s1, o1, f"d={d} n=({n_a}, {n_b})")
    for t, k, name in zip((sb, ob, pa, pb), keep, ("sum_b", "outer_b", "pivot_a", "pivot_b")):
        assert torch.equal(t.cpu().nan_to_num(nan=-7.0), k.cpu().nan_to_num(nan=-7.0)), name + " was written"
    if same_pivot:                                                      # delta = 0: a plain sum of the two accumulators
        s2, o2 = accumulate(be, A, d, pa, ldo_a)
        own = owned_mask(d, o2.shape[0], ldo_a)
        own_b = owned_mask(d, ob.shape[0], ldo_b)
        assert torch.equal(sa.cpu()[:d], s2.cpu()[:d] + sb.cpu()[:d]) and torch.equal(oa.cpu()[own], o2.cpu()[own] + ob.cpu()[own_b])


@pytest.mark.parametrize("d,n_a,n_b,ldo_a,ldo_b", EXACT_SHAPES)
def test_merge_equals_one_pass_over_the_concatenation(be, d, n_a, n_b, ldo_a, ldo_b):
    check_exact(be, d, n_a, n_b, ldo_a, ldo_b)


def test_merge_on_one_pivot_is_a_plain_sum(be):
    check_exact(be, 72, 8, 8, 72, 80, same_pivot=True)


@pytest.mark.gpu
def test_merge_at_pool3_width_on_the_gpu():
    """d = 2048, n = (50, 30): the product's own size (528 tiles)."""
    check_exact(_hip(), 2048, 50, 30, 2048, 2048)


def test_merge_chains_in_either_association(be):
    """(A u B) u C and A u (B u C) -- the latter merged into A -- both equal the single pass over cat(A, B, C) on pivot_a."""
    d, ldo = 72, 72
    parts = [int_features(n, d, d, 300 + i) for i, n in enumerate((16, 9, 34))]
    pivots = [be.to(dyadic_pivot(p, d)) for p in parts]
    s1, o1 = accumulate(be, torch.cat(parts), d, pivots[0], ldo)
    (sa, oa), (sb, ob), (sc, oc) = (accumulate(be, p, d, pv, ldo) for p, pv in zip(parts, pivots))
    merge(be, 9, pivots[1], sb, ob, ldo, pivots[0], sa, oa, ldo, d)
    merge(be, 34, pivots[2], sc, oc, ldo, pivots[0], sa, oa, ldo, d)
    same_owned(d, sa, oa, s1, o1, "(A u B) u C")
    (sa, oa), (sb, ob), (sc, oc) = (accumulate(be, p, d, pv, ldo) for p, pv in zip(parts, pivots))
    merge(be, 34, pivots[2], sc, oc, ldo, pivots[1], sb, ob, ldo, d)
    merge(be, 9 + 34, pivots[1], sb, ob, ldo, pivots[0], sa, oa, ldo, d)
    same_owned(d, sa, oa, s1, o1, "A u (B u C)")


def test_merge_of_random_features_within_the_derived_bound_and_run_to_run_identical(be):
    from colddiff import metrics
    from test_fid_device import features
    d, n_a, n_b = 72, 50, 37
    fa, fb = features(d, n_a, 31, 0.1), features(d, n_b, 32, 0.25)
    pa, pb = be.to(fa.double().mean(0)), be.to(fb.double().mean(0))
    base_a, base_b = accumulate(be, fa, d, pa, d, pad=0), accumulate(be, fb, d, pb, d, pad=0)
    outs = []
    for _ in range(2):
        (sa, oa), (sb, ob) = (tuple(t.clone() for t in base) for base in (base_a, base_b))
        merge(be, n_b, pb, sb, ob, d, pa, sa, oa, d, d)
        outs.append((sa.cpu(), oa.cpu()))
    own = owned_mask(d, d + 3, d)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1][own], outs[1][1][own]), "two launches on fresh copies differ"
    st = metrics.FidStats(d, be.device)
    st.n, st.pivot, st.sum, st.outer = n_a + n_b, pa, sa, oa[:d].nan_to_num(nan=0.0)          # (cov reads the upper triangle: owned)
    allf = torch.cat((fa, fb)).numpy().astype(np.longdouble)
    n = n_a + n_b
    mean = allf.mean(0)
    xc = allf - mean
    cov = (xc.T @ xc) / (n - 1)
    R = max(np.abs(allf - p.cpu().numpy().astype(np.longdouble)).max() for p in (pa, pb))
    dm = float(np.abs(st.mean().cpu().numpy() - mean).max())
    dc = float(np.abs(st.cov().cpu().numpy() - cov).max())
    print(f"merge [{be.kind}] (50 + 37, 72): |dmean| {dm:.3g} (bound {8 * n * U * R:.3g}), |dcov| {dc:.3g} (bound {16 * n * U * R * R:.3g})")
    assert dm <= 8 * n * U * R
    assert dc <= 16 * n * U * R * R


def test_merge_bad_arguments_are_a_status_and_write_nothing(be):
    d = 16
    x = int_features(4, d, d, 1)
    pv = be.to(torch.zeros(d, dtype=torch.float64))
    (sa, oa), (sb, ob) = accumulate(be, x, d, pv, d), accumulate(be, x, d, pv, d)
    keep = [t.clone() for t in (sa, oa)]
    L, st = be.L, be.stream()
    for args, text in (((4.0, P(pv), P(sb), P(ob), d, P(pv), P(sa), P(oa), d, 0, st), "at least 1"),
                       ((4.0, P(pv), P(sb), 0, d, P(pv), P(sa), P(oa), d, d, st), "null pointer"),
                       ((4.0, P(pv), P(sb), P(ob), d, P(pv), 0, P(oa), d, d, st), "null pointer"),
                       ((4.0, P(pv), P(sb), P(ob), d, P(pv), P(sa), P(oa), d - 1, d, st), "ldo_a"),
                       ((4.0, P(pv), P(sb), P(ob), d - 1, P(pv), P(sa), P(oa), d, d, st), "ldo_b"),
                       ((0.0, P(pv), P(sb), P(ob), d, P(pv), P(sa), P(oa), d, d, st), "n_b"),
                       ((4.0, P(pv), P(sb), P(oa), d, P(pv), P(sa), P(oa), d, d, st), "must not be"),
                       ((4.0, P(pv), P(sa), P(ob), d, P(pv), P(sa), P(oa), d, d, st), "must not be")):
        with pytest.raises(CdfError, match=text):
            L.cdf_moments_merge_f64(*args)
    assert L._dll.cdf_moments_merge_f64(4.0, P(pv), P(sb), P(ob), d, P(pv), P(sa), P(oa), d, -3, st) == -1
    for t, k in zip((sa, oa), keep):
        assert torch.equal(t.cpu().nan_to_num(nan=-7.0), k.cpu().nan_to_num(nan=-7.0)), "a refused call wrote"
