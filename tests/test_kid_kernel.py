"""`cdf_kid_poly3_f64` (csrc/k_kid.hip): the unbiased polynomial-kernel MMD^2 of index-selected subsets on the fp64 matrix cores.
Simulator and MI355X.

Exact tests: integer features in [-3, 3] with gamma a power of two make every gamma g + coef0 dyadic, its cube exact and every partial sum
far below 2^53 (d = 64, gamma = 1/64: |z| <= 10 in steps of 2^-6, z^3 < 2^10 in steps of 2^-18, 130^2 terms < 2^15: 43 bits; d = 72,
gamma = 1/8: z^3 < 2^20 in steps of 2^-9, 70^2 terms < 2^13: 42 bits), so sxx, syy, sxy must equal numpy's by `==` in any summation order.
A padded tile row counted as coef0^3 = 1, a diagonal entry left in, an off-diagonal tile counted once or a K tail read from the pitch padding
(NaN here) all show at once.  mmd2 is held to the formula evaluated from those sums within 4 ulp of its larger term (three roundings).

Random data: the bound is derived in tests/kid_ref.py (its docstring), not measured:
    |dS| <= 2 u (3 (d + 3) + P) sum Z^3,  Z = |gamma| sum_k |a_k b_k| + |coef0|,  P the number of pairs summed,
    |d mmd2| <= (B(sxx) + B(syy)) / (m (m - 1)) + 2 B(sxy) / m^2 + 4 ulp of the larger term.

Every launch here runs on poisoned, guarded buffers: nothing outside partial[nsub][3][tiles] and out[nsub][4] may change, and every element
inside must be written.
"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import kid_ref as R
from colddiff import _lib
from colddiff._lib import CdfError
from emu_util import P
from poison import poison_

GUARD = 64
EXACT_CASES = [(5, 1), (64, 2), (65, 3), (70, 2), (130, 1)]                   # (m, nsub): tile tail both ways, one tile, one row past, 3 x 3 tiles


def int_features(n, d, ld, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.full((n, ld), float("nan"), dtype=torch.float64)                # pitch padding is poison: it must not be read into a sum
    x[:, :d] = torch.randint(-3, 4, (n, d), generator=g).double()
    return x


def gapped_indices(n, m, nsub, seed):
    """[nsub, m] int32: each row the first m of a permutation of n > m rows."""
    rng = np.random.RandomState(seed)
    return torch.from_numpy(np.stack([rng.permutation(n)[:m] for _ in range(nsub)]).astype(np.int32))


def launch(be, x, y, ix, iy, d, gamma, coef0, partial=None):
    """One call on guarded buffers -> (out [nsub, 4] on the host, the partial buffer).  Asserts the ownership contract."""
    nsub, m = ix.shape
    tiles = be.L.cdf_kid_tiles(m)
    assert tiles == ((m + 63) // 64) ** 2
    own_p, own_o = nsub * 3 * tiles, nsub * 4
    if partial is None:
        partial = poison_(torch.empty(own_p + 2 * GUARD, device=be.device, dtype=torch.float64))
    before = partial.cpu().clone()
    out = poison_(torch.empty(own_o + 2 * GUARD, device=be.device, dtype=torch.float64))
    dx, dy, dix, diy = be.to(x), be.to(y), be.to(ix), be.to(iy)
    be.L.cdf_kid_poly3_f64(P(dx), dx.stride(0), P(dix), P(dy), dy.stride(0), P(diy), nsub, m, d, gamma, coef0, P(partial) + 8 * GUARD,
                           P(out) + 8 * GUARD, be.stream())
    p, o = partial.cpu(), out.cpu()
    assert torch.isnan(o[:GUARD]).all() and torch.isnan(o[GUARD + own_o:]).all(), "out written outside [nsub][4]"
    same = lambda a, b: torch.equal(torch.nan_to_num(a, nan=-1.25), torch.nan_to_num(b, nan=-1.25))
    assert same(p[:GUARD], before[:GUARD]) and same(p[GUARD + own_p:], before[GUARD + own_p:]), "partial written outside [nsub][3][tiles]"
    assert not torch.isnan(o[GUARD:GUARD + own_o]).any(), "an element of out was not written"
    assert not torch.isnan(p[GUARD:GUARD + own_p]).any(), "a partial of this call was not written"
    return o[GUARD:GUARD + own_o].view(nsub, 4).numpy(), partial


def check_exact(got, x, y, ix, iy, d, gamma, coef0):
    m = ix.shape[1]
    for s in range(ix.shape[0]):
        xs, ys = x[ix[s].long(), :d].numpy(), y[iy[s].long(), :d].numpy()
        sxx, syy, sxy = R.sums(xs, ys, gamma, coef0)
        assert (got[s, 0], got[s, 1], got[s, 2]) == (sxx, syy, sxy), (s, got[s], (sxx, syy, sxy))
        terms = R.mmd2_terms(sxx, syy, sxy, m)
        assert abs(got[s, 3] - (terms[0] - terms[1])) <= 4 * np.spacing(max(abs(terms[0]), abs(terms[1]))), (s, got[s, 3], terms)


@pytest.mark.parametrize("d", [16, 64])
@pytest.mark.parametrize("m,nsub", EXACT_CASES)
def test_exact_on_integer_features_through_gapped_indices(be, m, nsub, d):
    n1, n2 = m + 7, m + 3
    x, y = int_features(n1, d, d + 3, 100 * m + d), int_features(n2, d, d + 5, 100 * m + d + 1)
    ix, iy = gapped_indices(n1, m, nsub, m), gapped_indices(n2, m, nsub, m + 1)
    got, _ = launch(be, x, y, ix, iy, d, 1.0 / d, 1.0)
    check_exact(got, x, y, ix, iy, d, 1.0 / d, 1.0)


@pytest.mark.parametrize("d", [40, 72])
def test_exact_with_d_off_the_k_chunk_and_off_the_tile(be, d):
    """The K tail (d = 40: half a chunk; d = 72: a tile plus half a chunk) contributes zeros, not the NaN of the pitch padding."""
    m, nsub = 70, 2
    x, y = int_features(m + 7, d, d + 3, d), int_features(m + 3, d, d + 1, d + 1)
    ix, iy = gapped_indices(m + 7, m, nsub, d), gapped_indices(m + 3, m, nsub, d + 1)
    got, _ = launch(be, x, y, ix, iy, d, 0.125, 1.0)
    check_exact(got, x, y, ix, iy, d, 0.125, 1.0)


def test_a_source_row_named_twice_counts_off_the_diagonal(be):
    """Positions decide, not row numbers: ix names row 4 at positions 1 and 66 (two different tiles), iy row 2 at positions 0 and 1."""
    m, d = 70, 16
    x, y = int_features(m, d, d, 7), int_features(m, d, d, 8)
    ix, iy = gapped_indices(m, m, 1, 3), gapped_indices(m, m, 1, 4)
    ix[0, 1] = ix[0, 66] = 4
    iy[0, 0] = iy[0, 1] = 2
    got, _ = launch(be, x, y, ix, iy, d, 1.0 / d, 1.0)
    check_exact(got, x, y, ix, iy, d, 1.0 / d, 1.0)                           # (kid_ref.sums masks by position)
    assert (float(x[4] @ x[4]) / d + 1.0) ** 3 > 0                            # the (1, 66) and (66, 1) entries a row-number mask would drop


def test_a_stale_partial_does_not_survive_a_call_with_fewer_tiles(be):
    m, d = 130, 16
    x, y = int_features(m, d, d, 21), int_features(m, d, d, 22)
    ix, iy = gapped_indices(m, m, 1, 5), gapped_indices(m, m, 1, 6)
    _, partial = launch(be, x, y, ix, iy, d, 1.0 / d, 1.0)                    # 9 tiles per pair
    ix2, iy2 = ix[:, :65].contiguous(), iy[:, :65].contiguous()               # 4 tiles per pair, the same scratch
    got, _ = launch(be, x, y, ix2, iy2, d, 1.0 / d, 1.0, partial=partial)
    check_exact(got, x, y, ix2, iy2, d, 1.0 / d, 1.0)


# ---- random fp32-valued features ------------------------------------------------------------------------------------------------------
RM, RD, RNSUB = 70, 72, 2
_random = {}


def random_case():
    """Features, indices and the numpy fp64 reference of the random case; made once."""
    if not _random:
        g = torch.Generator().manual_seed(31)
        x = torch.randn(RM + 9, RD, generator=g).double()                     # fp32 values, as the extractor's
        y = (torch.randn(RM + 4, RD, generator=g) * 1.5 + 0.2).double()
        ix, iy = gapped_indices(RM + 9, RM, RNSUB, 11), gapped_indices(RM + 4, RM, RNSUB, 12)
        subs = [(x[ix[s].long()].numpy(), y[iy[s].long()].numpy()) for s in range(RNSUB)]
        want = [R.sums(xs, ys, 1.0 / RD, 1.0) for xs, ys in subs]
        _random.update(x=x, y=y, ix=ix, iy=iy, subs=subs, want=want, bounds=[R.bounds(xs, ys, 1.0 / RD, 1.0) for xs, ys in subs])
    return _random


def check_random(got, tag):
    c = random_case()
    for s in range(RNSUB):
        sxx, syy, sxy = c["want"][s]
        ref = (sxx, syy, sxy, R.mmd2(sxx, syy, sxy, RM))
        for q, name in enumerate(("sxx", "syy", "sxy", "mmd2")):
            err = abs(got[s][q] - ref[q])
            print(f"kid_poly3 [{tag}] subset {s} {name}: {ref[q]:.12g}, error {err:.3g} (bound {c['bounds'][s][q]:.3g})")
            assert err <= c["bounds"][s][q], (s, name, got[s][q], ref[q])


def test_random_features_within_the_derived_bound_and_run_to_run_identical(be):
    c = random_case()
    runs = [launch(be, c["x"], c["y"], c["ix"], c["iy"], RD, 1.0 / RD, 1.0)[0] for _ in range(2)]
    check_random(runs[0], be.kind)
    assert np.array_equal(runs[0], runs[1]), "two runs differ"
    assert all(abs(runs[0][s, 3]) > 1e3 * c["bounds"][s][3] for s in range(RNSUB)), "the case does not resolve its own mmd2"


def test_the_bound_is_not_vacuous_for_numpy_itself():
    """numpy's own sums with the rows taken in reversed order (another summation order of the same terms) and a long-double evaluation
    (u = 2^-64 on x86: the exact value to 11 more bits) are inside the same bound."""
    c = random_case()
    rev = [[*R.sums(xs[::-1].copy(), ys[::-1].copy(), 1.0 / RD, 1.0)] for xs, ys in c["subs"]]
    check_random([r + [R.mmd2(*r, RM)] for r in rev], "numpy, rows reversed")
    ld = [[float(v) for v in R.sums(xs.astype(np.longdouble), ys.astype(np.longdouble), np.longdouble(1) / RD, np.longdouble(1))]
          for xs, ys in c["subs"]]
    check_random([r + [R.mmd2(*r, RM)] for r in ld], "numpy long double")


def test_the_definition_is_sklearns_polynomial_kernel(be):
    pw = pytest.importorskip("sklearn.metrics.pairwise")
    c = random_case()
    got = launch(be, c["x"], c["y"], c["ix"], c["iy"], RD, 1.0 / RD, 1.0)[0]
    off = ~np.eye(RM, dtype=bool)
    for s, (xs, ys) in enumerate(c["subs"]):
        kxx, kyy, kxy = (pw.polynomial_kernel(a, b, degree=3, gamma=None, coef0=1) for a, b in ((xs, xs), (ys, ys), (xs, ys)))
        sk = (kxx[off].sum(), kyy[off].sum(), kxy.sum())
        for q in range(3):
            assert abs(got[s, q] - sk[q]) <= c["bounds"][s][q], (s, q, got[s, q], sk[q])
        assert abs(got[s, 3] - R.mmd2(*sk, RM)) <= c["bounds"][s][3]


# ---- argument checks --------------------------------------------------------------------------------------------------------------------
def check_argument_errors(L, p, st):
    """Every host-side check of include/colddiff.h: a status and a text, no launch (the pointers are not device memory on the device build)."""
    good = [p, 16, p, p, 16, p, 1, 4, 16, 1.0 / 16, 1.0, p, p, st]

    def bad(**kw):
        names = ("x", "ldx", "ix", "y", "ldy", "iy", "nsub", "m", "d", "gamma", "coef0", "partial", "out", "stream")
        a = list(good)
        for k, v in kw.items():
            a[names.index(k)] = v
        return a

    for args, text in ((bad(x=0), "null pointer"), (bad(ix=0), "null pointer"), (bad(y=0), "null pointer"), (bad(iy=0), "null pointer"),
                       (bad(partial=0), "null pointer"), (bad(out=0), "null pointer"),
                       (bad(m=1), "m must be at least 2"), (bad(nsub=0), "at least 1"), (bad(d=0, ldx=0, ldy=0), "at least 1"),
                       (bad(ldx=15), "ldx"), (bad(ldy=15), "ldy"),
                       (bad(nsub=65536), "65535 subsets"), (bad(m=64 * 46340 + 1), "tiles of 64")):
        with pytest.raises(CdfError, match=text):
            L.cdf_kid_poly3_f64(*args)
    assert L._dll.cdf_kid_poly3_f64(*bad(m=-3)) == -1
    assert L.cdf_kid_tiles(1) == 0 and L.cdf_kid_tiles(2) == 1 and L.cdf_kid_tiles(65) == 4 and L.cdf_kid_tiles(64 * 46340 + 1) == 0


def test_bad_arguments_are_a_status(be):
    buf = torch.zeros(64, device=be.device, dtype=torch.float64)
    check_argument_errors(be.L, P(buf), be.stream())


def test_bad_arguments_are_a_status_on_the_device_build_without_a_gpu():
    buf = torch.zeros(64, dtype=torch.float64)
    check_argument_errors(_lib.Lib(_lib.LIB_PATH), buf.data_ptr(), 0)


def test_kid_kernels_use_no_scratch_and_the_f64_mfma():
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    if not shutil.which(hipcc):
        pytest.skip("hipcc not available")
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(repo, "cold-diffusion-models_amd", "csrc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I", csrc, "-I", os.path.join(repo, "include"),
                        "-S", os.path.join(csrc, "k_kid.hip"), "-o", "-", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    sizes = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) == 2 and sizes == [0, 0], r.stderr[-2000:]
    vgprs = [int(v) for v in re.findall(r" VGPRs: (\d+)", r.stderr)]
    assert max(vgprs) <= 128, r.stderr[-2000:]
    assert r.stdout.count("v_mfma_f64_16x16x4_f64") >= 16                          # 16 per K chunk
