"""`cdf_knn_sq_f64` and `cdf_ball_counts_f64` (csrc/k_prdc.hip): k-th-neighbour radii and ball memberships of fp64 feature rows on the
matrix cores, the two passes behind precision / recall / density / coverage.  Simulator and MI355X.

Exact tests: integer features in [-3, 3] make every |a|^2, a.b and hence every D an exact integer (d <= 72: |a|^2 <= 648) in any summation
order, and full of ties: `knn` and both counts must equal numpy's by `==`.  `<=` against `<`, a masked column counted at distance |a|^2,
a self-distance left in and a K tail read from the pitch padding (NaN here) all show at once.

Random data: the bound is derived in tests/prdc_ref.py (its docstring), not measured:
    |dD(a, b)| <= B(a, b) = 2 u [(d + 2)(|a|^2 + |b|^2) + 2 (d + 1) sum_k |a_k b_k|] / (1 - (d + 2) u),   |d knn[j][q]| <= max_l B(x_j, x_l);
a count is exact when no pair lies within B + B_rho of its radius, which the test asserts of its data first, on the reference alone.

Every launch here runs on poisoned, guarded buffers: nothing outside partial, knn, cnt_col, cnt_row may change, and every element inside
must be written; the pitch padding of the operands is NaN.
"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import prdc_ref as R
from colddiff import _lib
from colddiff._lib import CdfError
from emu_util import P
from poison import poison_

GUARD = 64
INT_POISON = 0x5A5A5A5A


def int_features(n, d, ld, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.full((n, ld), float("nan"), dtype=torch.float64)                # pitch padding is poison: it must not be read into a sum
    x[:, :d] = torch.randint(-3, 4, (n, d), generator=g).double()
    return x


def padded(rows, extra):
    x = torch.full((rows.shape[0], rows.shape[1] + extra), float("nan"), dtype=torch.float64)
    x[:, :rows.shape[1]] = rows
    return x


def same(a, b):
    return torch.equal(torch.nan_to_num(a, nan=-1.25), torch.nan_to_num(b, nan=-1.25))


def norms_of(be, dx, d):
    out = poison_(torch.empty(dx.shape[0], device=be.device, dtype=torch.float64))
    be.L.cdf_rowsumsq_f64(P(dx), dx.stride(0), dx.shape[0], d, P(out), be.stream())
    return out


def launch_knn(be, x, d, k, partial=None):
    """One cdf_knn_sq_f64 on guarded buffers -> (knn [n, k] on the host, the partial buffer).  Asserts the ownership contract."""
    n = x.shape[0]
    S = be.L.cdf_knn_splits(n)
    assert 1 <= S <= (n + 63) // 64
    own_p, own_o = S * n * k, n * k
    if partial is None:
        partial = poison_(torch.empty(own_p + 2 * GUARD, device=be.device, dtype=torch.float64))
    before = partial.cpu().clone()
    out = poison_(torch.empty(own_o + 2 * GUARD, device=be.device, dtype=torch.float64))
    dx = be.to(x)
    nrm = norms_of(be, dx, d)
    be.L.cdf_knn_sq_f64(P(dx), dx.stride(0), n, d, k, P(nrm), P(partial) + 8 * GUARD, P(out) + 8 * GUARD, be.stream())
    p, o = partial.cpu(), out.cpu()
    assert torch.isnan(o[:GUARD]).all() and torch.isnan(o[GUARD + own_o:]).all(), "knn written outside [n][k]"
    assert same(p[:GUARD], before[:GUARD]) and same(p[GUARD + own_p:], before[GUARD + own_p:]), "partial written outside [S][n][k]"
    assert not torch.isnan(o[GUARD:GUARD + own_o]).any(), "an element of knn was not written"
    assert not torch.isnan(p[GUARD:GUARD + own_p]).any(), "a partial of this call was not written"
    assert same(dx.cpu(), x), "the operand was written"
    return o[GUARD:GUARD + own_o].view(n, k).numpy(), partial


def launch_ball(be, a, b, d, rcol=None, rrow=None, partial=None):
    """One cdf_ball_counts_f64 on guarded buffers -> (cnt_col, cnt_row, the partial buffer); the output of a side whose radius is None is
    handed in all the same and must stay poisoned."""
    na, nb = a.shape[0], b.shape[0]
    S = be.L.cdf_ball_splits(na, nb)
    assert 1 <= S <= (nb + 63) // 64
    own_p = S * na * 2
    if partial is None:
        partial = poison_(torch.empty(own_p + 2 * GUARD, device=be.device, dtype=torch.int32))
    before = partial.cpu().clone()
    outs = [poison_(torch.empty(na + 2 * GUARD, device=be.device, dtype=torch.int32)) for _ in range(2)]
    da, db = be.to(a), be.to(b)
    an, bn = norms_of(be, da, d), norms_of(be, db, d)
    rc = None if rcol is None else be.to(torch.from_numpy(np.ascontiguousarray(rcol)))
    rr = None if rrow is None else be.to(torch.from_numpy(np.ascontiguousarray(rrow)))
    be.L.cdf_ball_counts_f64(P(da), da.stride(0), na, P(an), P(db), db.stride(0), nb, P(bn), d, P(rc), P(rr), P(partial) + 4 * GUARD,
                             P(outs[0]) + 4 * GUARD, P(outs[1]) + 4 * GUARD, be.stream())
    p = partial.cpu()
    assert torch.equal(p[:GUARD], before[:GUARD]) and torch.equal(p[GUARD + own_p:], before[GUARD + own_p:]), "partial written outside [S][na][2]"
    assert not (p[GUARD:GUARD + own_p] == INT_POISON).any(), "a partial of this call was not written"
    got = []
    for o, radius, name in zip((t.cpu() for t in outs), (rcol, rrow), ("cnt_col", "cnt_row")):
        assert (o[:GUARD] == INT_POISON).all() and (o[GUARD + na:] == INT_POISON).all(), name + " written outside [na]"
        if radius is None:
            assert (o == INT_POISON).all(), name + " was touched though its radius is null"
            got.append(None)
        else:
            assert not (o[GUARD:GUARD + na] == INT_POISON).any(), "an element of " + name + " was not written"
            got.append(o[GUARD:GUARD + na].numpy())
    return got[0], got[1], partial


# ---- exact on integers --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [16, 40, 72])                                   # one K chunk; off the chunk; off the tile
@pytest.mark.parametrize("n,k", [(n, k) for n in (5, 64, 65, 70, 130) for k in (1, 3, 8) if n >= k + 1])     # tile tail, one tile, one row past, 2 x 2,
def test_knn_exact_on_integer_features(be, n, k, d):                          # 3 x 3 tiles; n < k + 1 is refused (test_bad_arguments_are_a_status)
    x = int_features(n, d, d + 3, 1000 * n + 10 * d + k)
    got, _ = launch_knn(be, x, d, k)
    want = R.knn(x[:, :d].numpy(), k)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert n < 64 or k == 1 or (want[:, :-1] == want[:, 1:]).any(), "the case has no ties"


@pytest.mark.parametrize("d", [16, 40, 72])
@pytest.mark.parametrize("na,nb", [(5, 70), (64, 64), (65, 130), (130, 65)])
def test_ball_counts_exact_on_integer_features_with_radii_from_knn(be, na, nb, d):
    a, b = int_features(na, d, d + 3, 100 * na + d), int_features(nb, d, d + 5, 100 * nb + d + 1)
    a[:na // 2, :d] = b[:na // 2, :d]                                         # shared rows: a neighbour AT the radius is among the rows of a
    ha, hb = a[:, :d].numpy(), b[:, :d].numpy()
    rcol, rrow = R.knn(hb, 3)[:, 2], R.knn(ha, 2)[:, 1]
    col, row, _ = launch_ball(be, a, b, d, rcol, rrow)
    wcol, wrow = R.ball_counts(ha, hb, rcol, rrow)
    assert np.array_equal(col, wcol) and np.array_equal(row, wrow)
    D = R.dist_sq(ha, hb)
    assert (D == rcol[None, :]).any() and (D == rrow[:, None]).any(), "no distance equals a radius: <= against < is not exercised"
    assert wcol.max() > 0 and wrow.max() > 0


def test_a_row_that_appears_twice_is_a_neighbour_at_zero_and_self_is_never_one(be):
    d, k = 16, 3
    x = int_features(70, d, d + 1, 5)
    x[66] = x[2]                                                              # two tiles apart
    got, _ = launch_knn(be, x, d, k)
    assert got[2, 0] == 0.0 and got[66, 0] == 0.0
    assert np.array_equal(got, R.knn(x[:, :d].numpy(), k))
    assert (np.delete(got[:, 0], [2, 66]) > 0).all(), "a row without a twin reports distance 0: its own position was left in"
    # n = k + 1: every other row is a neighbour, the row itself is not (no +inf, no 0)
    for n, kk in ((2, 1), (4, 3), (9, 8)):
        y = int_features(n, d, d, 40 + n)
        g, _ = launch_knn(be, y, d, kk)
        assert np.array_equal(g, R.knn(y[:, :d].numpy(), kk)) and np.isfinite(g).all() and (g > 0).all()


def test_null_sides_leave_their_outputs_untouched(be):
    d = 40
    a, b = int_features(65, d, d + 3, 61), int_features(70, d, d + 1, 62)
    ha, hb = a[:, :d].numpy(), b[:, :d].numpy()
    rcol, rrow = R.knn(hb, 3)[:, 2], R.knn(ha, 3)[:, 2]
    wcol, wrow = R.ball_counts(ha, hb, rcol, rrow)
    col, row, _ = launch_ball(be, a, b, d, rcol, None)                       # (launch_ball asserts the other output stayed poisoned)
    assert row is None and np.array_equal(col, wcol)
    col, row, _ = launch_ball(be, a, b, d, None, rrow)
    assert col is None and np.array_equal(row, wrow)
    col, row, _ = launch_ball(be, a, b, d, rcol, rrow)
    assert np.array_equal(col, wcol) and np.array_equal(row, wrow)
    # a null OUTPUT pointer on the side not asked for
    da, db = be.to(a), be.to(b)
    an, bn = norms_of(be, da, d), norms_of(be, db, d)
    rc = be.to(torch.from_numpy(rcol.copy()))
    part = poison_(torch.empty(be.L.cdf_ball_splits(65, 70) * 65 * 2, device=be.device, dtype=torch.int32))
    out = poison_(torch.empty(65, device=be.device, dtype=torch.int32))
    be.L.cdf_ball_counts_f64(P(da), da.stride(0), 65, P(an), P(db), db.stride(0), 70, P(bn), d, P(rc), 0, P(part), P(out), 0, be.stream())
    assert np.array_equal(out.cpu().numpy(), wcol)


def test_a_stale_partial_does_not_survive_a_smaller_call(be):
    d = 16
    x = int_features(130, d, d, 21)
    _, partial = launch_knn(be, x, d, 3)                                      # 3 splits of 130 rows
    small = x[:65].contiguous()                                               # 2 splits of 65 rows, the same scratch
    got, _ = launch_knn(be, small, d, 3, partial=partial)
    assert np.array_equal(got, R.knn(small[:, :d].numpy(), 3))
    b = int_features(130, d, d, 22)
    rcol, rrow = R.knn(b[:, :d].numpy(), 3)[:, 2], R.knn(x[:, :d].numpy(), 3)[:, 2]
    _, _, bpart = launch_ball(be, x, b, d, rcol, rrow)
    col, row, _ = launch_ball(be, small, b[:65].contiguous(), d, rcol[:65], rrow[:65], partial=bpart)
    wcol, wrow = R.ball_counts(small[:, :d].numpy(), b[:65, :d].numpy(), rcol[:65], rrow[:65])
    assert np.array_equal(col, wcol) and np.array_equal(row, wrow)


# ---- random Gaussian features -------------------------------------------------------------------------------------------------------------
RN, RM, RD, RK = 130, 70, 72, 3
_random = {}


def random_case():
    """Features and the numpy fp64 reference of the random case; made once."""
    if not _random:
        g = torch.Generator().manual_seed(31)
        x = torch.randn(RN, RD, generator=g).double()                         # fp32 values, as the extractor's
        y = (torch.randn(RM, RD, generator=g) * 1.1 + 0.1).double()
        hx, hy = x.numpy(), y.numpy()
        _random.update(x=x, y=y, hx=hx, hy=hy, knn_x=R.knn(hx, RK), knn_y=R.knn(hy, RK), bx=R.knn_bound(hx), by=R.knn_bound(hy))
    return _random


def check_knn_bound(got, want, bnd, tag):
    err = np.abs(got - want).max(1)
    print(f"knn_sq [{tag}]: largest error {err.max():.3g}, its bound {bnd[err.argmax()]:.3g}, smallest radius {want[:, -1].min():.6g}")
    assert (err <= bnd).all(), (err.argmax(), err.max(), bnd[err.argmax()])


def test_random_features_knn_within_the_bound_counts_exact_and_run_to_run_identical(be):
    c = random_case()
    rho_x, rho_y = c["knn_x"][:, RK - 1], c["knn_y"][:, RK - 1]
    # the condition of the data, on the reference alone: no pair within B + B_rho of its radius, in either pass of the four metrics
    assert R.ambiguous_counts(c["hy"], c["hx"], rcol=rho_x, bcol=c["bx"]) == 0
    assert R.ambiguous_counts(c["hx"], c["hy"], rcol=rho_y, rrow=rho_x, bcol=c["by"], brow=c["bx"]) == 0
    x, y = padded(c["x"], 3), padded(c["y"], 1)
    runs = [(launch_knn(be, x, RD, RK)[0], launch_knn(be, y, RD, RK)[0]) for _ in range(2)]
    check_knn_bound(runs[0][0], c["knn_x"], c["bx"], be.kind + ", X")
    check_knn_bound(runs[0][1], c["knn_y"], c["by"], be.kind + ", Y")
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1]), "two runs differ"
    # the counts with the KERNEL's radii (what prdc_device feeds them) equal the reference's with its own
    kx, ky = runs[0][0][:, RK - 1], runs[0][1][:, RK - 1]
    for _ in range(2):
        col, _, _ = launch_ball(be, y, x, RD, kx, None)
        assert np.array_equal(col, R.ball_counts(c["hy"], c["hx"], rcol=rho_x)[0])
        col, row, _ = launch_ball(be, x, y, RD, ky, kx)
        wcol, wrow = R.ball_counts(c["hx"], c["hy"], rcol=rho_y, rrow=rho_x)
        assert np.array_equal(col, wcol) and np.array_equal(row, wrow)
    assert 0 < wrow.astype(bool).sum() < RN, "the case does not separate covered from uncovered rows"


def test_the_bound_is_not_vacuous():
    """numpy with the features summed in reversed order (another summation order of the same terms) stays inside the bound; a relative
    perturbation of 1e-9 does not."""
    c = random_case()
    rev = R.knn(np.ascontiguousarray(c["hx"][:, ::-1]), RK)
    check_knn_bound(rev, c["knn_x"], c["bx"], "numpy, features reversed")
    assert (np.abs(c["knn_x"] * (1 + 1e-9) - c["knn_x"]).max(1) > c["bx"]).all()
    assert (c["bx"] < 1e-10 * c["knn_x"][:, 0]).all()


# ---- argument checks --------------------------------------------------------------------------------------------------------------------
def check_argument_errors(L, p, st):
    """Every host-side check of include/colddiff.h: a status and a text, no launch (the pointers are not device memory on the device build)."""
    knn_names = ("x", "ldx", "n", "d", "k", "norms", "partial", "knn", "stream")
    knn_good = [p, 16, 9, 16, 3, p, p, p, st]
    ball_names = ("a", "lda", "na", "anorm", "b", "ldb", "nb", "bnorm", "d", "rcol", "rrow", "partial", "cnt_col", "cnt_row", "stream")
    ball_good = [p, 16, 4, p, p, 16, 5, p, 16, p, p, p, p, p, st]

    def bad(names, good, **kw):
        a = list(good)
        for k, v in kw.items():
            a[names.index(k)] = v
        return a

    for kw, text in ((dict(x=0), "null pointer"), (dict(norms=0), "null pointer"), (dict(partial=0), "null pointer"), (dict(knn=0), "null pointer"),
                     (dict(k=0), r"k must be in \[1, 8\] \(got 0\)"), (dict(k=9, n=20), r"k must be in \[1, 8\] \(got 9\)"),
                     (dict(n=3), r"at least k \+ 1 \(got n = 3, k = 3\)"), (dict(n=(1 << 30) + 1), "2\\^30 rows"),
                     (dict(d=0, ldx=0), "d must be at least 1"), (dict(ldx=15), "ldx")):
        with pytest.raises(CdfError, match=text):
            L.cdf_knn_sq_f64(*bad(knn_names, knn_good, **kw))
    assert L._dll.cdf_knn_sq_f64(*bad(knn_names, knn_good, n=-3)) == -1
    for kw, text in ((dict(a=0), "null pointer"), (dict(anorm=0), "null pointer"), (dict(b=0), "null pointer"), (dict(bnorm=0), "null pointer"),
                     (dict(partial=0), "null pointer"), (dict(cnt_col=0), "rcol without cnt_col"), (dict(cnt_row=0), "rrow without cnt_row"),
                     (dict(na=0), "at least 1"), (dict(nb=0), "at least 1"), (dict(d=0, lda=0, ldb=0), "at least 1"),
                     (dict(nb=(1 << 30) + 1), "2\\^30 rows"), (dict(lda=15), "lda"), (dict(ldb=15), "ldb")):
        with pytest.raises(CdfError, match=text):
            L.cdf_ball_counts_f64(*bad(ball_names, ball_good, **kw))
    assert L._dll.cdf_ball_counts_f64(*bad(ball_names, ball_good, na=-3)) == -1
    # the split counts: pure functions of the row counts, 0 for what the entry points refuse, never more than the column tiles
    assert [L.cdf_knn_splits(n) for n in (0, 1, 2, 64, 65, 130, 1000, (1 << 30) + 1)] == [0, 0, 1, 1, 2, 3, 16, 0]
    assert L.cdf_knn_splits(10000) == 6 and L.cdf_knn_splits(1 << 20) == 1
    assert [L.cdf_ball_splits(*q) for q in ((0, 5), (5, 0), (5, 70), (130, 65), (10000, 10000), (5, (1 << 30) + 1))] == [0, 0, 2, 2, 6, 0]


def test_bad_arguments_are_a_status(be):
    buf = torch.zeros(64, device=be.device, dtype=torch.float64)
    check_argument_errors(be.L, P(buf), be.stream())


def test_bad_arguments_are_a_status_on_the_device_build_without_a_gpu():
    buf = torch.zeros(64, dtype=torch.float64)
    check_argument_errors(_lib.Lib(_lib.LIB_PATH), buf.data_ptr(), 0)


def test_prdc_kernels_use_no_scratch_and_the_f64_mfma():
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    if not shutil.which(hipcc):
        pytest.skip("hipcc not available")
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(repo, "cold-diffusion-models_amd", "csrc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I", csrc, "-I", os.path.join(repo, "include"),
                        "-S", os.path.join(csrc, "k_prdc.hip"), "-o", "-", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    sizes = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    # the k-NN kernel with a list of 4 and of 8 (a spill of the list to scratch is how it would go quietly wrong), the ball kernel, two folds
    assert len(names) == 5 and sum("knn_sq_kernel" in n for n in names) == 2 and sum("ball_counts_kernel" in n for n in names) == 1
    assert sizes == [0] * 5, r.stderr[-3000:]
    bodies = re.split(r"^\s*\.globl\s+", r.stdout, flags=re.M)[1:]
    main = [b for b in bodies if "knn_sq_kernel" in b.split(None, 1)[0] or "ball_counts_kernel" in b.split(None, 1)[0]]
    assert len(main) == 3 and all(b.count("v_mfma_f64_16x16x4_f64") >= 16 for b in main)      # 16 per K chunk
