"""Host statement of improved precision / recall, density / coverage and of the rounding-error bound of their squared distances, shared by
tests/test_prdc_kernel.py and tests/test_prdc_device.py.  TEST INFRASTRUCTURE ONLY.

Definitions (include/colddiff.h, cdf_knn_sq_f64 / cdf_ball_counts_f64), by brute force in numpy fp64.  X: n rows, Y: m rows.
    D(a, b) = max(0, (|a|^2 + |b|^2) - 2 a.b)                                     squared distances throughout, no square root
    knn_X[j][0..k) ascending: the k smallest of { D(x_j, x_l) : l != j }          self left out by position;  rho_X(j) = knn_X[j][k - 1]
    precision = #{ i : exists j, D(y_i, x_j) <= rho_X(j) } / m       recall   = #{ j : exists i, D(x_j, y_i) <= rho_Y(i) } / n
    density   = sum_i #{ j : D(y_i, x_j) <= rho_X(j) } / (k m)       coverage = #{ j : exists i, D(x_j, y_i) <= rho_X(j) } / n
    f_score   = 2 precision recall / max(precision + recall, 1e-5)

The bound (u = 2^-53).  One fp64 evaluation of D(a, b), in any summation order, against the exact value, to first order in u:
  * |a|^2 as a d-term sum of rounded squares: d roundings on every term at most, |d |a|^2| <= d u |a|^2; |b|^2 likewise;
  * a.b as a d-term sum of rounded products in any order (a fused multiply-add does no worse): |d a.b| <= d u sum_k |a_k b_k|;
  * the sum |a|^2 + |b|^2 rounds once: u (|a|^2 + |b|^2);  the doubling of a.b is exact;
  * the difference rounds once: u |(|a|^2 + |b|^2) - 2 a.b| <= u (|a|^2 + |b|^2 + 2 sum_k |a_k b_k|);
  * max(0, .) is 1-Lipschitz and the exact D is >= 0: it adds nothing.
Together E(a, b) = u [(d + 2)(|a|^2 + |b|^2) + 2 (d + 1) sum_k |a_k b_k|].  The terms of second order are at most (d + 2) u times that
(every factor (1 + u)^p - 1 with p <= d + 2 is at most p u / (1 - p u)), which the division below covers.  Two evaluations -- the
kernel's and numpy's -- are each within E of the exact value, hence within
    B(a, b) = 2 u [(d + 2)(|a|^2 + |b|^2) + 2 (d + 1) sum_k |a_k b_k|] / (1 - (d + 2) u)
of each other.
An order statistic is 1-Lipschitz in the sup norm: moving every D(x_j, .) by at most max_l B(x_j, x_l) moves the q-th smallest by at most
that, so |d knn[j][q]| <= Bknn(j) = max_l B(x_j, x_l).
A comparison D(a, b) <= rho comes out the same in both evaluations wherever |D - rho| > B(a, b) + B_rho (B_rho: the bound of that radius,
0 when both sides are handed the same numbers); a pair inside that margin is AMBIGUOUS.  A count is exact wherever none of its pairs is,
and so are the four metrics when no pair of either pass is: `ambiguous_*` count them on the reference alone.
"""
import numpy as np

U = 2.0 ** -53


def dist_sq(a, b):
    """[na, nb]: D of every row of a [na, d] against every row of b [nb, d]."""
    na, nb = (a * a).sum(1), (b * b).sum(1)
    return np.maximum(0.0, (na[:, None] + nb[None, :]) - 2.0 * (a @ b.T))


def knn(x, k):
    """[n, k] ascending, self left out by position."""
    D = dist_sq(x, x)
    np.fill_diagonal(D, np.inf)
    return np.sort(D, axis=1)[:, :k]


def ball_counts(a, b, rcol=None, rrow=None):
    """(cnt_col [na] or None, cnt_row [na] or None) of cdf_ball_counts_f64."""
    D = dist_sq(a, b)
    return (None if rcol is None else (D <= rcol[None, :]).sum(1).astype(np.int32),
            None if rrow is None else (D <= rrow[:, None]).sum(1).astype(np.int32))


def prdc(x, y, k):
    n, m = len(x), len(y)
    rho_x, rho_y = knn(x, k)[:, k - 1], knn(y, k)[:, k - 1]
    in_x, _ = ball_counts(y, x, rcol=rho_x)
    in_y, own = ball_counts(x, y, rcol=rho_y, rrow=rho_x)
    precision, recall = int((in_x > 0).sum()) / m, int((in_y > 0).sum()) / n
    return dict(precision=precision, recall=recall, density=int(in_x.sum()) / (k * m), coverage=int((own > 0).sum()) / n,
                f_score=2.0 * precision * recall / max(precision + recall, 1e-5))


def bound(a, b):
    """B(a, b) [na, nb]."""
    d = a.shape[1]
    na, nb = (a * a).sum(1), (b * b).sum(1)
    return 2 * U * ((d + 2) * (na[:, None] + nb[None, :]) + 2 * (d + 1) * (np.abs(a) @ np.abs(b).T)) / (1 - (d + 2) * U)


def knn_bound(x):
    """Bknn [n]: the bound of every knn[j][q]."""
    return bound(x, x).max(1)


def ambiguous_counts(a, b, rcol=None, rrow=None, bcol=None, brow=None):
    """The number of pairs (i, j) whose comparison against rcol[j] / rrow[i] lies within B(a_i, b_j) + the radius's own bound (bcol [nb] /
    brow [na]; None: the radius is handed to both sides as it is)."""
    D, B = dist_sq(a, b), bound(a, b)
    cnt = 0
    if rcol is not None:
        cnt += int((np.abs(D - rcol[None, :]) <= B + (0.0 if bcol is None else bcol[None, :])).sum())
    if rrow is not None:
        cnt += int((np.abs(D - rrow[:, None]) <= B + (0.0 if brow is None else brow[:, None])).sum())
    return cnt


def ambiguous_prdc(x, y, k):
    """The ambiguous pairs of both passes of `prdc`, every radius taken with its own bound: 0 means all five numbers are exact."""
    rho_x, rho_y = knn(x, k)[:, k - 1], knn(y, k)[:, k - 1]
    bx, by = knn_bound(x), knn_bound(y)
    return ambiguous_counts(y, x, rcol=rho_x, bcol=bx) + ambiguous_counts(x, y, rcol=rho_y, rrow=rho_x, bcol=by, brow=bx)
