"""The Gaussian-mixture kernels of csrc/k_gmm.hip: Cholesky, triangular inverse, centre-and-scale, row sums of squares, responsibilities.
Simulator and MI355X (fixture `be`).

Exact tests.  A = L L^T for an integer lower-triangular L with entries in [-3, 3] and a diagonal in {1, 2, 4}: every Schur complement is an
integer matrix far below 2^53, every pivot a perfect square (1, 4, 16) and every division is by 1, 2 or 4, so a correct Cholesky returns L
itself whatever its blocking.  For the inverse, L = (I + N1)(I + N2)(I + N3) with N_i integer and non-zero only in a bottom-left block
(N_i^2 = 0): L^-1 = (I - N3)(I - N2)(I - N1) is an integer matrix and all partial sums stay integers far below 2^53.

Derived bounds (u = 2^-53):
  potrf   |L L^T - A|_max <= 4 d u max|A|.   The computed factor satisfies |A - L L^T| <= gamma_{d+1} |L||L^T| (Higham, Accuracy and
          Stability, Thm 10.3; each entry is a sum of at most d products, a subtraction and a division or square root, in any order), and
          (|L||L^T|)_ij <= |l_i||l_j| = sqrt(a_ii a_jj) <= max|A|.  The factor 4 covers (d + 1) / d, gamma / (d u), and the gamma_d of the
          test's own numpy product L L^T.
  trtri   The kernel solves L P = I by (blocked) forward substitution, so R = L P - I obeys |R| <= gamma_d |L||P| (Higham Thm 8.5 per
          column); P L - I = L^-1 R L, hence |P L - I| <= 4 d u (|P| (|L||P|) |L|) entrywise, with |P| standing for |L^-1| (first order) and
          the factor 4 as above (plus the test's own product).
  resp    log and exp of the two libms are taken as accurate to 2 ulp (glibc < 1, ROCm's device library documents 1).  lp is formed the
          same way as the restatement (four roundings); a perturbation e of lp - lse perturbs resp = exp(.) by a relative e, and
          |lp|, |lse| <= M = the largest |lp| of the case, so e <= 8 u M covers the roundings of lp, of lse (a K-term sum of exps, log, add)
          and of the difference: |dresp| <= (8 M + 4 + K) u resp + tiny, |dlse| <= (8 + K) u M.  nk and the lse sum add an n-term sum:
          + n u times the sum of magnitudes.
"""
import numpy as np
import pytest
import torch

from colddiff._lib import CdfError
from emu_util import P
from poison import poison_

U = 2.0 ** -53
DS = [1, 3, 48, 64, 65, 130, 200]
KS = [1, 3]


def f64(be, *shape):
    return poison_(torch.empty(*shape, device=be.device, dtype=torch.float64))


def int_lower(d, seed):
    r = np.random.RandomState(seed)
    L = np.tril(r.randint(-3, 4, (d, d)).astype(np.float64), -1)
    L[np.arange(d), np.arange(d)] = r.choice([1.0, 2.0, 4.0], d)
    return L


def unit_lower_with_integer_inverse(d, seed):
    r = np.random.RandomState(seed)
    L, Linv = np.eye(d), np.eye(d)
    for h in sorted({max(1, d // 4), max(1, d // 2), max(1, 3 * d // 4)}):
        N = np.zeros((d, d))
        N[h:, :h] = r.randint(-2, 3, (d - h, h))
        L, Linv = L @ (np.eye(d) + N), (np.eye(d) - N) @ Linv
    assert np.array_equal(L @ Linv, np.eye(d)) and np.abs(L).max() < 2 ** 30 and np.abs(Linv).max() < 2 ** 30
    return L, Linv


def batch(be, mats, lower_only=True):
    """K matrices in a poisoned [K, d + 1, d + 3] buffer (pitch and stride wider than the matrix); with lower_only the strict upper
    triangle stays poison too.  -> (device buffer, mask of the elements that were filled)."""
    K, d = len(mats), mats[0].shape[0]
    host = torch.full((K, d + 1, d + 3), float("nan"), dtype=torch.float64)
    mask = torch.zeros(K, d + 1, d + 3, dtype=torch.bool)
    tri = torch.ones(d, d).tril().bool() if lower_only else torch.ones(d, d, dtype=torch.bool)
    for k, m in enumerate(mats):
        host[k, :d, :d] = torch.where(tri, torch.from_numpy(np.ascontiguousarray(m)), torch.full((d, d), float("nan"), dtype=torch.float64))
        mask[k, :d, :d] = tri
    return be.to(host), mask


def potrf(be, buf, d, K):
    info = poison_(torch.empty(K + 2, device=be.device, dtype=torch.int32))
    be.L.cdf_potrf_f64(P(buf), buf.stride(1), buf.stride(0), d, K, P(info), be.stream())
    info = info.cpu()
    assert (info[K:] == 0x5A5A5A5A).all(), "info written past the batch"
    return info[:K]


def trtri(be, lbuf, d, K):
    out = f64(be, K, d + 2, d + 5)
    be.L.cdf_trtri_lower_f64(P(lbuf), lbuf.stride(1), lbuf.stride(0), P(out), out.stride(1), out.stride(0), d, K, be.stream())
    out = out.cpu()
    assert torch.isnan(out[:, d:]).all() and torch.isnan(out[:, :, d:]).all(), "written outside [d, d]"
    return out[:, :d, :d].numpy()


# ---- cdf_potrf_f64 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("d", DS)
def test_potrf_returns_the_integer_factor_exactly(be, d, K):
    Ls = [int_lower(d, 100 * d + k) for k in range(K)]
    runs = []
    for _ in range(2):
        buf, mask = batch(be, [L @ L.T for L in Ls])
        info = potrf(be, buf, d, K)
        assert (info == 0).all()
        runs.append(buf.cpu())
    got = runs[0]
    assert torch.isnan(got[~mask]).all(), "the strict upper triangle or the pitch padding was written"
    for k, L in enumerate(Ls):
        g = got[k, :d, :d].numpy()
        il = np.tril_indices(d)
        assert np.array_equal(g[il], L[il])
    assert torch.equal(runs[0][mask], runs[1][mask]), "two runs differ"


@pytest.mark.parametrize("d", [3, 65, 130, 200])
def test_potrf_random_spd_within_the_bound(be, d):
    r = np.random.RandomState(d)
    mats = []
    for k in range(2):
        g = r.randn(d, d + 5)
        mats.append(g @ g.T / d + 0.1 * np.eye(d))
    runs = []
    for _ in range(2):
        buf, mask = batch(be, mats)
        assert (potrf(be, buf, d, 2) == 0).all()
        runs.append(buf.cpu())
    assert torch.equal(runs[0][mask], runs[1][mask]), "two runs differ"
    assert torch.isnan(runs[0][~mask]).all()
    for k, A in enumerate(mats):
        L = np.tril(np.nan_to_num(runs[0][k, :d, :d].numpy()))
        err, bound = np.abs(L @ L.T - A).max(), 4 * d * U * np.abs(A).max()
        print(f"potrf [{be.kind}] d {d}: |L L^T - A| {err:.3g} (bound {bound:.3g})")
        assert err <= bound


def test_potrf_negative_pivot_is_a_status_and_leaves_the_others_alone(be):
    d = 130
    good = [int_lower(d, 7), int_lower(d, 8)]
    L = int_lower(d, 9)
    bad = L @ L.T
    # the leading 70 x 70 minor is untouched (it only involves rows / columns < 70); pivot 70 becomes l_70,70^2 - 100 < 0
    bad[70, 70] -= 100.0
    buf, mask = batch(be, [good[0] @ good[0].T, bad, good[1] @ good[1].T])
    info = potrf(be, buf, d, 3)                                   # (a checked call: no error status)
    assert info.tolist() == [0, 71, 0]
    got = buf.cpu()
    assert torch.isnan(got[~mask]).all(), "out of bounds or upper-triangle write"
    il = np.tril_indices(d)
    for k, Lk in ((0, good[0]), (2, good[1])):
        assert np.array_equal(got[k, :d, :d].numpy()[il], Lk[il])
    g = np.nan_to_num(got[1, :d, :d].numpy())
    assert np.array_equal(np.tril(g)[:, :64], np.tril(L)[:, :64]), "the panel before the bad pivot's is complete"
    # a later call on a good batch clears the status words
    buf2, _ = batch(be, [good[0] @ good[0].T])
    assert potrf(be, buf2, d, 1).tolist() == [0]


# ---- cdf_trtri_lower_f64 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("d", DS)
def test_trtri_integer_inverse_exact_with_zeroed_triangle(be, d, K):
    pairs = [unit_lower_with_integer_inverse(d, 10 * d + k) for k in range(K)]
    runs = []
    for _ in range(2):
        buf, _ = batch(be, [p[0] for p in pairs])                  # (strict upper triangle of L is poison: it must not be read)
        runs.append(trtri(be, buf, d, K))
    assert np.array_equal(runs[0], runs[1]), "two runs differ"
    for k, (_, Linv) in enumerate(pairs):
        assert np.array_equal(runs[0][k], Linv.T)                  # (== treats -0.0 as 0.0: the zeroed triangle included)


@pytest.mark.parametrize("d", [3, 65, 130, 200])
def test_trtri_random_within_the_bound(be, d):
    r = np.random.RandomState(d + 1)
    Ls = [np.tril(r.randn(d, d), -1) / np.sqrt(d) + np.diag(1.0 + r.rand(d)) for _ in range(2)]
    buf, _ = batch(be, Ls)
    PT = trtri(be, buf, d, 2)
    for k, L in enumerate(Ls):
        Pm = PT[k].T
        assert np.array_equal(np.triu(Pm, 1), np.zeros((d, d)))
        err = np.abs(Pm @ L - np.eye(d)).max()
        bound = 4 * d * U * (np.abs(Pm) @ (np.abs(L) @ np.abs(Pm)) @ np.abs(L)).max()
        print(f"trtri [{be.kind}] d {d}: |P L - I| {err:.3g} (bound {bound:.3g})")
        assert err <= bound


def test_tril_copy_and_logdet(be):
    d, K = 70, 2
    r = np.random.RandomState(3)
    mats = [r.randint(-5, 6, (d, d)).astype(np.float64) for _ in range(K)]
    buf, _ = batch(be, mats)                                        # upper triangle poison: only the lower one may be read
    for tr in (0, 1):
        out = f64(be, K, d + 1, d + 2)
        be.L.cdf_tril_copy_f64(P(buf), buf.stride(1), buf.stride(0), P(out), out.stride(1), out.stride(0), d, K, tr, be.stream())
        out = out.cpu()
        assert torch.isnan(out[:, d:]).all() and torch.isnan(out[:, :, d:]).all()
        for k in range(K):
            assert np.array_equal(out[k, :d, :d].numpy(), np.tril(mats[k]).T if tr else np.tril(mats[k]))
    diag = [2.0 ** r.randint(-3, 4, d) for _ in range(K)]
    buf, _ = batch(be, [np.diag(v) for v in diag])
    outs = []
    for _ in range(2):
        ld = f64(be, K + 1)
        be.L.cdf_logdet_diag_f64(P(buf), buf.stride(1), buf.stride(0), d, K, P(ld), be.stream())
        outs.append(ld.cpu())
    assert torch.isnan(outs[0][K:]).all() and torch.equal(outs[0][:K], outs[1][:K])
    for k in range(K):                                                # log 2^e = e log 2: a d-term sum of multiples of log 2, each 1 ulp
        assert abs(outs[0][k].item() - np.log(diag[k]).sum()) <= 4 * d * U * np.abs(np.log(diag[k])).sum()


# ---- cdf_gmm_center_scale_f64 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("n", [1, 7, 257])
@pytest.mark.parametrize("d", [3, 65, 130])
def test_center_scale_exact_on_dyadic_data(be, n, d, dtype):
    r = np.random.RandomState(n * 1000 + d)
    x = torch.full((n, d + 2), float("nan"), dtype=dtype)
    x[:, :d] = torch.from_numpy(r.randint(-64, 65, (n, d)) / 8.0).to(dtype)
    mean = torch.from_numpy(r.randint(-16, 17, d) / 4.0)
    scale = r.choice([0.0, 0.25, 1.0, 4.0, 16.0], n)                # = resp / nk with nk = 4: perfect squares, sqrt exact
    resp, nk = torch.from_numpy(scale * 4.0), torch.tensor([4.0], dtype=torch.float64)
    dx, dm, dr, dn = be.to(x), be.to(mean), be.to(resp), be.to(nk)
    want_plain = x[:, :d].double().numpy() - mean.numpy()
    want = np.sqrt(scale)[:, None] * want_plain
    runs = []
    for _ in range(2):
        z, zt = f64(be, n + 1, d + 3), f64(be, d + 1, n + 2)
        be.L.cdf_gmm_center_scale_f64(P(dx), int(dtype == torch.float64), d + 2, n, d, P(dm), P(dr), P(dn), P(z), d + 3, P(zt), n + 2, be.stream())
        z, zt = z.cpu(), zt.cpu()
        assert torch.isnan(z[n:]).all() and torch.isnan(z[:, d:]).all() and torch.isnan(zt[d:]).all() and torch.isnan(zt[:, n:]).all()
        assert np.array_equal(z[:n, :d].numpy(), want) and np.array_equal(zt[:d, :n].numpy(), want.T)
        runs.append((z, zt))
    assert torch.equal(runs[0][0][:n, :d], runs[1][0][:n, :d]) and torch.equal(runs[0][1][:d, :n], runs[1][1][:d, :n])
    z = f64(be, n, d)
    be.L.cdf_gmm_center_scale_f64(P(dx), int(dtype == torch.float64), d + 2, n, d, P(dm), 0, 0, P(z), d, 0, 0, be.stream())
    assert np.array_equal(z.cpu().numpy(), want_plain)               # null scale: the plain centred matrix, no transposed copy


# ---- cdf_rowsumsq_f64 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 300])
@pytest.mark.parametrize("d", [1, 3, 130, 4099])
def test_rowsumsq_exact_on_integer_data(be, n, d):
    r = np.random.RandomState(n + d)
    y = torch.full((n, d + 3), float("nan"), dtype=torch.float64)
    y[:, :d] = torch.from_numpy(r.randint(-9, 10, (n, d)).astype(np.float64))
    dy = be.to(y)
    outs = []
    for _ in range(2):
        out = f64(be, n + 2)
        be.L.cdf_rowsumsq_f64(P(dy), d + 3, n, d, P(out), be.stream())
        outs.append(out.cpu())
    assert torch.isnan(outs[0][n:]).all()
    assert np.array_equal(outs[0][:n].numpy(), (y[:, :d].numpy() ** 2).sum(1)) and torch.equal(outs[0][:n], outs[1][:n])


# ---- cdf_gmm_resp_f64 ----------------------------------------------------------------------------------------------------------------
def run_resp(be, maha, logdet, logw, d, hard):
    K, n = maha.shape
    dm = be.to(torch.from_numpy(np.pad(maha, ((0, 0), (0, 3)), constant_values=np.nan)))
    dl = be.to(torch.from_numpy(logdet)) if logdet is not None else None
    dw = be.to(torch.from_numpy(logw)) if logw is not None else None
    nblk = be.L.cdf_gmm_resp_blocks(n)
    assert nblk == (n + 255) // 256
    resp, nk, lse, part = f64(be, K + 1, n + 5), f64(be, K + 1), f64(be, 2), f64(be, nblk * (K + 1) + 1)
    be.L.cdf_gmm_resp_f64(P(dm), n + 3, P(dl), P(dw), n, d, K, hard, P(resp), n + 5, P(nk), P(lse), P(part), be.stream())
    resp, nk, lse, part = resp.cpu(), nk.cpu(), lse.cpu(), part.cpu()
    assert torch.isnan(resp[K:]).all() and torch.isnan(resp[:, n:]).all() and torch.isnan(nk[K:]).all() and torch.isnan(lse[1:]).all()
    assert torch.isnan(part[-1:]).all()
    return resp[:K, :n].numpy(), nk[:K].numpy(), lse[0].item()


@pytest.mark.parametrize("K", [1, 3, 10])
@pytest.mark.parametrize("n", [5, 700])
def test_resp_against_the_numpy_restatement(be, K, n):
    d = 7
    r = np.random.RandomState(K * 31 + n)
    maha = r.rand(K, n) * 40.0
    maha[:, 0] = 5.0                                                  # a full tie
    maha[0, 1], maha[1:, 1] = 1.0, 4000.0                             # one dominant component: exp underflows to an exact 0
    logdet, w = r.randn(K), r.rand(K) + 0.1
    logw = np.log(w / w.sum())
    lp = -0.5 * (d * np.log(2 * np.pi) + maha) + logdet[:, None] + logw[:, None]
    mx = lp.max(0)
    lse = mx + np.log(np.exp(lp - mx).sum(0))
    want = np.exp(lp - lse)
    a = run_resp(be, maha, logdet, logw, d, 0)
    b = run_resp(be, maha, logdet, logw, d, 0)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2], "two runs differ"
    resp, nk, lse_sum = a
    M = np.abs(lp).max()
    tol = (8 * M + 4 + K) * U * want + 1e-300
    print(f"resp [{be.kind}] K {K} n {n}: max |dresp| / tol {np.max(np.abs(resp - want) / tol):.3g}")
    assert (np.abs(resp - want) <= tol).all()
    assert resp[0, 1] == 1.0 and (resp[1:, 1] == 0.0).all()
    assert np.abs(nk - (want.sum(1) + 10 * np.finfo(float).eps)).max() <= (8 * M + 4 + K + n) * U * want.sum(1).max()
    assert abs(lse_sum - lse.sum()) <= (8 + K + n) * U * np.abs(lse).sum()


def test_resp_hard_assignment_takes_the_lowest_index_on_ties(be):
    K, n = 3, 300
    r = np.random.RandomState(4)
    maha = r.randint(0, 6, (K, n)).astype(np.float64)                 # many ties
    maha[:, :3] = [[2, 1, 1], [2, 1, 0], [2, 3, 0]]
    resp, nk, lse_sum = run_resp(be, maha, None, None, 5, 1)
    arg = maha.argmin(0)                                               # numpy: first occurrence
    assert arg[:3].tolist() == [0, 0, 1]
    assert np.array_equal(resp, np.eye(K)[arg].T)
    assert np.array_equal(nk, np.bincount(arg, minlength=K) + 10 * np.finfo(float).eps) and lse_sum == 0.0
    again = run_resp(be, maha, None, None, 5, 1)
    assert np.array_equal(resp, again[0]) and np.array_equal(nk, again[1])


# ---- argument checks ---------------------------------------------------------------------------------------------------------------
def test_gmm_entry_points_refuse_bad_arguments_with_a_status(be):
    L, st = be.L, be.stream()
    a, b = be.to(torch.zeros(2, 8, 8, dtype=torch.float64)), be.to(torch.zeros(2, 8, 8, dtype=torch.float64))
    info = be.to(torch.zeros(2, dtype=torch.int32))
    x, v = be.to(torch.zeros(4, 8)), be.to(torch.zeros(64, dtype=torch.float64))
    pa, pb, pi, px, pv = P(a), P(b), P(info), P(x), P(v)
    for fn, args, text in (
            (L.cdf_potrf_f64, (0, 8, 64, 8, 2, pi, st), "null pointer"),
            (L.cdf_potrf_f64, (pa, 8, 64, 8, 2, 0, st), "null pointer"),
            (L.cdf_potrf_f64, (pa, 8, 64, 0, 2, pi, st), "at least 1"),
            (L.cdf_potrf_f64, (pa, 7, 64, 8, 2, pi, st), "lda"),
            (L.cdf_potrf_f64, (pa, 8, 60, 8, 2, pi, st), "stride"),
            (L.cdf_trtri_lower_f64, (pa, 8, 64, 0, 8, 64, 8, 2, st), "null pointer"),
            (L.cdf_trtri_lower_f64, (pa, 8, 64, pb, 8, 64, 8, 0, st), "at least 1"),
            (L.cdf_trtri_lower_f64, (pa, 8, 64, pb, 7, 64, 8, 2, st), "row pitch"),
            (L.cdf_trtri_lower_f64, (pa, 8, 64, pb, 8, 10, 8, 2, st), "stride"),
            (L.cdf_trtri_lower_f64, (pa, 8, 64, pa + 8 * 8, 8, 64, 8, 1, st), "alias"),
            (L.cdf_tril_copy_f64, (pa, 8, 64, pa, 8, 64, 8, 2, 0, st), "alias"),
            (L.cdf_tril_copy_f64, (pa, 8, 64, pb, 7, 64, 8, 2, 0, st), "row pitch"),
            (L.cdf_logdet_diag_f64, (pa, 7, 64, 8, 2, pv, st), "ld"),
            (L.cdf_logdet_diag_f64, (pa, 8, 64, 8, 2, 0, st), "null pointer"),
            (L.cdf_gmm_center_scale_f64, (px, 0, 8, 4, 8, pv, pv, 0, pa, 8, 0, 0, st), "come together"),
            (L.cdf_gmm_center_scale_f64, (px, 0, 7, 4, 8, pv, 0, 0, pa, 8, 0, 0, st), "row pitch"),
            (L.cdf_gmm_center_scale_f64, (px, 0, 8, 4, 8, pv, 0, 0, pa, 8, pb, 3, st), "ldzt"),
            (L.cdf_gmm_center_scale_f64, (px, 2, 8, 4, 8, pv, 0, 0, pa, 8, 0, 0, st), "x_is_f64"),
            (L.cdf_gmm_center_scale_f64, (px, 0, 8, 0, 8, pv, 0, 0, pa, 8, 0, 0, st), "at least 1"),
            (L.cdf_gmm_center_scale_f64, (px, 0, 8, 4, 8, 0, 0, 0, pa, 8, 0, 0, st), "null pointer"),
            (L.cdf_rowsumsq_f64, (pa, 7, 4, 8, pv, st), "ldy"),
            (L.cdf_rowsumsq_f64, (pa, 8, 4, 8, 0, st), "null pointer"),
            (L.cdf_gmm_resp_f64, (pa, 8, pv, pv, 8, 3, 2, 0, pb, 8, pv, pv, 0, st), "null pointer"),
            (L.cdf_gmm_resp_f64, (pa, 7, pv, pv, 8, 3, 2, 0, pb, 8, pv, pv, pv, st), "row pitch"),
            (L.cdf_gmm_resp_f64, (pa, 8, pv, pv, 8, 3, 2, 2, pb, 8, pv, pv, pv, st), "hard"),
            (L.cdf_gmm_resp_f64, (pa, 8, 0, 0, 8, 3, 2, 0, pb, 8, pv, pv, pv, st), "only with hard"),
            (L.cdf_gmm_resp_f64, (pa, 8, pv, pv, 8, 3, 0, 0, pb, 8, pv, pv, pv, st), "at least 1")):
        with pytest.raises(CdfError, match=text):
            fn(*args)
    assert L._dll.cdf_potrf_f64(pa, 8, 64, -1, 2, pi, st) == -1
    assert L.cdf_gmm_resp_blocks(0) == 0 and L.cdf_gmm_resp_blocks(257) == 2
