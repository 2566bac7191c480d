"""Host statement of the Kernel Inception Distance and its rounding-error bound, shared by tests/test_kid_kernel.py and
tests/test_kid_device.py.  TEST INFRASTRUCTURE ONLY.

Definitions (include/colddiff.h, cdf_kid_poly3_f64): k(a, b) = (gamma a.b + coef0)^3; sxx / syy sum k over positions i != j of one subset,
sxy over all i, j of the two; mmd2 = (sxx + syy) / (m (m - 1)) - 2 sxy / (m m).

The bound (u = 2^-53, first order, times 2 for the higher-order terms and nothing more).  For one pair of rows let
Z = |gamma| sum_k |a_k b_k| + |coef0|.  A d-term dot product in any order is off by at most d u sum|a_k b_k|; the multiplication by gamma
and the addition of coef0 round once each:  |dz| <= (d + 2) u Z.  Cubing:  |d(z^3)| <= 3 Z^2 |dz| + 3 u Z^3 = 3 (d + 3) u Z^3.  A P-term
sum in any order adds gamma_P sum|k| <= P u sum Z^3.  So for a sum S over a set of P pairs
    |dS| <= B(S) = 2 u (3 (d + 3) + P) sum Z^3
and
    |d mmd2| <= (B(sxx) + B(syy)) / (m (m - 1)) + 2 B(sxy) / (m m) + 4 ulp of the larger of the two terms.
B bounds the distance of ANY fp64 evaluation from the exact value -- the kernel's and numpy's alike; `P` is the worst case over summation
orders (a tree of depth log P does far better), which is what keeps the comparison of two such evaluations inside one B.
"""
import numpy as np

U = 2.0 ** -53


def kernel_matrix(a, b, gamma, coef0):
    z = gamma * (a @ b.T) + coef0
    return z * z * z


def sums(xs, ys, gamma, coef0):
    """(sxx, syy, sxy) of two [m, d] float64 subsets, by position."""
    off = ~np.eye(xs.shape[0], dtype=bool)
    return (kernel_matrix(xs, xs, gamma, coef0)[off].sum(), kernel_matrix(ys, ys, gamma, coef0)[off].sum(),
            kernel_matrix(xs, ys, gamma, coef0).sum())


def mmd2_terms(sxx, syy, sxy, m):
    return (sxx + syy) / (float(m) * (m - 1.0)), 2.0 * sxy / (float(m) * m)


def mmd2(sxx, syy, sxy, m):
    a, b = mmd2_terms(sxx, syy, sxy, m)
    return a - b


def bounds(xs, ys, gamma, coef0):
    """(B(sxx), B(syy), B(sxy), bound of mmd2) for two [m, d] float64 subsets."""
    m, d = xs.shape
    off = ~np.eye(m, dtype=bool)

    def B(a, b, mask):
        z3 = (abs(gamma) * (np.abs(a) @ np.abs(b).T) + abs(coef0)) ** 3
        return 2 * U * (3 * (d + 3) + int(mask.sum())) * z3[mask].sum()

    bxx, byy, bxy = B(xs, xs, off), B(ys, ys, off), B(xs, ys, np.ones((m, m), dtype=bool))
    t = mmd2_terms(*sums(xs, ys, gamma, coef0), m)
    return bxx, byy, bxy, (bxx + byy) / (m * (m - 1.0)) + 2 * bxy / (m * m) + 4 * np.spacing(max(abs(t[0]), abs(t[1])))


def kid(x, y, subsets, m, seed, gamma=None, coef0=1.0):
    """The whole procedure on two [n, d] float64 matrices: torch-fidelity's draws (one RandomState(seed); per subset choice(n1, m), then
    choice(n2, m), both without replacement) -> (values [subsets], their mmd2 bounds [subsets])."""
    rng = np.random.RandomState(seed)
    gamma = 1.0 / x.shape[1] if gamma is None else gamma
    vals, bnds = [], []
    for _ in range(subsets):
        xs = x[rng.choice(len(x), m, replace=False)]
        ys = y[rng.choice(len(y), m, replace=False)]
        vals.append(mmd2(*sums(xs, ys, gamma, coef0), m))
        bnds.append(bounds(xs, ys, gamma, coef0)[3])
    return np.array(vals), np.array(bnds)
