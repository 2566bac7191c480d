"""`cdf_moments_f64` and `cdf_gemm_f64` (csrc/k_fid.hip): the fp64 matrix-core kernels behind the device-side FID.  Simulator and MI355X.

Exact tests: integer-valued inputs make every product and every partial sum an integer far below 2^53, so the kernels must agree with
numpy by `==` whatever their summation order -- a wrong fragment row map (the fp64 MFMA's differs from the fp32 forms') moves whole rows.
Random-data bounds are derived, not measured:
  gemm     |dC|    <= 4 k 2^-53 max|a| max|b|   a k-term fp64 sum of products bounded by max|a| max|b| has error <= gamma_k of the bound in
                                               any order; alpha and diag add two roundings; the factor 4 covers gamma_k / (k u) and those.
  moments  |dcov|  <= 8 n 2^-53 R^2, |dmean| <= 4 n 2^-53 R,  R = max|x - pivot|: the same gamma_n bound on the n-term sums, the correction
                                               term sum sum^T / n and the division by n - 1 folded into the factor.
"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from colddiff._lib import CdfError
from emu_util import P
from poison import poison_

U = 2.0 ** -53
EXACT_SHAPES = [(7, 40, 40, 40), (50, 72, 80, 96), (4, 16, 16, 16)]          # (n, d, ldx, ldo): n tail, d off the tile, pitches wider than d
GEMM_SHAPES = [(40, 72, 50), (64, 64, 4), (17, 16, 33)]


def _hip():
    from colddiff import runtime
    from conftest import Backend
    runtime._lib_override = None
    return Backend("hip")


@pytest.fixture
def routed(be):
    """The Python layer (colddiff.metrics) on the backend of `be`: the simulator build for 'emu'."""
    from colddiff import runtime
    from emu_util import install_emu
    if be.kind == "emu":
        install_emu()
    else:
        runtime._lib_override = None
    yield be
    runtime._lib_override = None


def f64(be, *shape):
    return torch.zeros(*shape, device=be.device, dtype=torch.float64)


def int_features(n, d, ldx, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.full((n, ldx), float("nan"))                                    # pitch padding is poison: it must not be read into a sum
    x[:, :d] = torch.randint(-8, 9, (n, d), generator=g).float()
    return x


def moments(be, x, n, d, ldx, pivot, sum_, outer, ldo):
    be.L.cdf_moments_f64(P(x), ldx, n, d, P(pivot), P(sum_), P(outer), ldo, be.stream())


def new_outer(be, d, ldo, rows=None):
    """A poisoned [rows, ldo] accumulator whose upper-block-triangle tiles (inside [d, d]) start at zero."""
    rows = d + 3 if rows is None else rows
    o = poison_(torch.empty(rows, ldo, device=be.device, dtype=torch.float64))
    for bi in range(0, d, 64):
        o[bi:min(bi + 64, d), bi:d] = 0
    return o


def owned_mask(d, rows, ldo):
    m = torch.zeros(rows, ldo, dtype=torch.bool)
    for bi in range(0, d, 64):
        m[bi:min(bi + 64, d), bi:d] = True
    return m


@pytest.mark.parametrize("n,d,ldx,ldo", EXACT_SHAPES)
def test_moments_exact_on_integer_data_and_poisoned_padding(be, n, d, ldx, ldo):
    x = int_features(n, d, ldx, 11 * n + d)
    pivot = torch.randint(-3, 4, (d,), generator=torch.Generator().manual_seed(d)).double()
    s = poison_(torch.empty(d + 5, device=be.device, dtype=torch.float64))
    s[:d] = 0
    o = new_outer(be, d, ldo)
    moments(be, be.to(x), n, d, ldx, be.to(pivot), s, o, ldo)
    xc = x[:, :d].double().numpy() - pivot.numpy()
    s, o = s.cpu(), o.cpu()
    assert np.array_equal(s[:d].numpy(), xc.sum(0))
    assert torch.isnan(s[d:]).all(), "sum written past d"
    want = xc.T @ xc
    own = owned_mask(d, o.shape[0], ldo)
    assert torch.isnan(o[~own]).all(), "written outside [d, d] or below the block triangle's tiles"
    got = o[:d, :d].numpy()
    iu = np.triu_indices(d)
    assert np.array_equal(got[iu], want[iu])
    assert np.array_equal(got[own[:d, :d].numpy()], want[own[:d, :d].numpy()])      # a diagonal tile is written whole


def test_moments_two_tiles_exact_with_asymmetric_columns(be):
    """d = 72 spans two tiles: the off-diagonal tile (0, 1) has different A and B stripes -- a transposed or row-permuted store shows."""
    n, d = 9, 72
    x = torch.zeros(n, d)
    x[:, :] = torch.arange(d).float()[None, :] % 7 + torch.arange(n).float()[:, None] * (torch.arange(d).float()[None, :] % 3)
    pivot = torch.zeros(d, dtype=torch.float64)
    s, o = f64(be, d), f64(be, d, d)
    moments(be, be.to(x), n, d, d, be.to(pivot), s, o, d)
    want = x.double().numpy().T @ x.double().numpy()
    iu = np.triu_indices(d)
    assert np.array_equal(o.cpu().numpy()[iu], want[iu])
    assert torch.equal(o.cpu()[64:, :64], torch.zeros(8, 64, dtype=torch.float64)), "the tile below the block triangle was written"


def test_moments_accumulate_and_are_deterministic(be):
    n, d = 50, 72
    parts = [int_features(m, d, d, 100 + i) for i, m in enumerate((n, 7, 16))]
    pivot = be.to(torch.full((d,), 2.0, dtype=torch.float64))
    s3, o3 = f64(be, d), f64(be, d, d)
    for p in parts:
        moments(be, be.to(p), p.shape[0], d, d, pivot, s3, o3, d)
    cat = torch.cat(parts)
    s1, o1 = f64(be, d), f64(be, d, d)
    moments(be, be.to(cat), cat.shape[0], d, d, pivot, s1, o1, d)
    assert torch.equal(s3, s1) and torch.equal(o3, o1), "three accumulating launches differ from one launch on the concatenation"
    # random data, twice: bit-identical
    g = torch.Generator().manual_seed(5)
    xr = be.to(torch.randn(n, d, generator=g))
    outs = []
    for _ in range(2):
        s, o = f64(be, d), f64(be, d, d)
        moments(be, xr, n, d, d, pivot, s, o, d)
        moments(be, xr, n, d, d, pivot, s, o, d)
        outs.append((s.cpu(), o.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def check_stats_against_numpy(be, n, d, batches, seed, tag):
    from colddiff import metrics
    g = torch.Generator().manual_seed(seed)
    feats = [torch.relu(torch.randn(n, d, generator=g) + 0.3) for _ in range(batches)]
    st = metrics.FidStats(d, be.device)
    for f in feats:
        st.add(be.to(f))
    allf = torch.cat(feats).double().numpy()
    R = np.abs(allf - st.pivot.cpu().numpy()).max()
    N = allf.shape[0]
    assert st.n == N
    dm = np.abs(st.mean().cpu().numpy() - allf.mean(0)).max()
    cov = st.cov().cpu().numpy()
    dc = np.abs(cov - np.cov(allf, rowvar=False)).max()
    print(f"FidStats [{be.kind}] {tag}: |dmean| {dm:.3g} (bound {4 * N * U * R:.3g}), |dcov| {dc:.3g} (bound {8 * N * U * R * R:.3g})")
    assert dm <= 4 * N * U * R
    assert dc <= 8 * N * U * R * R
    assert np.array_equal(cov, cov.T)


def test_stats_of_random_features_against_numpy(routed):
    check_stats_against_numpy(routed, 23, 72, 3, 1, "3 x (23, 72)")


@pytest.mark.gpu
def test_stats_at_pool3_and_at_many_rows_on_the_gpu():
    be_hip = _hip()
    check_stats_against_numpy(be_hip, 50, 2048, 6, 2, "6 x (50, 2048)")
    check_stats_against_numpy(be_hip, 1000, 192, 1, 3, "(1000, 192)")


def test_moments_bad_arguments_are_a_status(be):
    x, pv, s, o = be.to(torch.zeros(4, 16)), f64(be, 16), f64(be, 16), f64(be, 16, 16)
    L, st = be.L, be.stream()
    for args, text in (((P(x), 16, 0, 16, P(pv), P(s), P(o), 16, st), "at least 1"),
                       ((P(x), 16, 4, 0, P(pv), P(s), P(o), 16, st), "at least 1"),
                       ((P(x), 15, 4, 16, P(pv), P(s), P(o), 16, st), "ldx"),
                       ((P(x), 16, 4, 16, P(pv), P(s), P(o), 15, st), "ldo"),
                       ((0, 16, 4, 16, P(pv), P(s), P(o), 16, st), "null pointer"),
                       ((P(x), 16, 4, 16, P(pv), P(s), 0, 16, st), "null pointer")):
        with pytest.raises(CdfError, match=text):
            L.cdf_moments_f64(*args)
    assert L._dll.cdf_moments_f64(P(x), 16, -1, 16, P(pv), P(s), P(o), 16, st) == -1


# ---- cdf_gemm_f64 ---------------------------------------------------------------------------------------------------------------
def gemm(be, a, b, alpha, diag, ldc_pad=0):
    m, k = a.shape
    n = b.shape[1]
    c = poison_(torch.empty(m + 2, n + ldc_pad, device=be.device, dtype=torch.float64))
    da, db = be.to(a), be.to(b)
    be.L.cdf_gemm_f64(P(da), da.stride(0), P(db), db.stride(0), P(c), c.stride(0), m, n, k, alpha, diag, be.stream())
    c = c.cpu()
    assert torch.isnan(c[m:]).all() and torch.isnan(c[:, n:]).all(), "written outside [m, n]"
    return c[:m, :n].numpy()


@pytest.mark.parametrize("alpha,diag", [(-0.5, 1.5), (1.0, 0.0)])
@pytest.mark.parametrize("m,n,k", GEMM_SHAPES)
def test_gemm_exact_on_integers_and_within_the_bound_on_random_data(be, m, n, k, alpha, diag):
    g = torch.Generator().manual_seed(m * 1000 + n * 10 + k)
    a = torch.randint(-8, 9, (m, k), generator=g).double()
    b = torch.randint(-8, 9, (k, n), generator=g).double()
    want = alpha * (a.numpy() @ b.numpy()) + diag * np.eye(m, n)
    assert np.array_equal(gemm(be, a, b, alpha, diag, ldc_pad=5), want)
    a = torch.randn(m, k, generator=g, dtype=torch.float64)
    b = torch.randn(k, n, generator=g, dtype=torch.float64)
    want = alpha * (a.numpy() @ b.numpy()) + diag * np.eye(m, n)
    err = np.abs(gemm(be, a, b, alpha, diag) - want).max()
    bound = 4 * k * U * a.abs().max().item() * b.abs().max().item()
    print(f"gemm_f64 [{be.kind}] {m}x{n}x{k} alpha {alpha}: max error {err:.3g} (bound {bound:.3g})")
    assert err <= bound


def test_gemm_takes_pitched_operands(be):
    g = torch.Generator().manual_seed(3)
    big_a = torch.randint(-8, 9, (40, 61), generator=g).double()
    big_b = torch.randint(-8, 9, (50, 77), generator=g).double()
    da, db = be.to(big_a), be.to(big_b)
    c = f64(be, 40, 72)
    be.L.cdf_gemm_f64(P(da), 61, P(db), 77, P(c), 72, 40, 72, 50, 1.0, 0.0, be.stream())
    assert np.array_equal(c.cpu().numpy(), big_a[:, :50].numpy() @ big_b[:, :72].numpy())


def test_gemm_aliasing_and_bad_arguments_are_a_status(be):
    a, c = f64(be, 16, 16), f64(be, 16, 16)
    L, st = be.L, be.stream()
    for args, text in (((P(a), 16, P(c), 16, P(a), 16, 16, 16, 16, 1.0, 0.0, st), "alias"),
                       ((P(c), 16, P(a), 16, P(a), 16, 16, 16, 16, 1.0, 0.0, st), "alias"),
                       ((P(a), 16, P(a), 16, P(a) + 8 * 100, 16, 16, 16, 16, 1.0, 0.0, st), "alias"),
                       ((P(a), 16, P(a), 16, P(c), 16, 0, 16, 16, 1.0, 0.0, st), "at least 1"),
                       ((P(a), 16, P(a), 16, P(c), 16, 16, 16, 0, 1.0, 0.0, st), "at least 1"),
                       ((P(a), 15, P(a), 16, P(c), 16, 16, 16, 16, 1.0, 0.0, st), "row pitch"),
                       ((P(a), 16, P(a), 16, P(c), 15, 16, 16, 16, 1.0, 0.0, st), "row pitch"),
                       ((0, 16, P(a), 16, P(c), 16, 16, 16, 16, 1.0, 0.0, st), "null pointer")):
        with pytest.raises(CdfError, match=text):
            L.cdf_gemm_f64(*args)
    L.cdf_gemm_f64(P(a), 16, P(a), 16, P(c), 16, 16, 16, 16, 1.0, 0.0, st)          # a == b is no alias of c


@pytest.mark.gpu
def test_gemm_2048_cubed_on_the_gpu():
    be_hip = _hip()
    g = torch.Generator().manual_seed(7)
    a = torch.randn(2048, 2048, generator=g, dtype=torch.float64)
    b = torch.randn(2048, 2048, generator=g, dtype=torch.float64)
    da, db = a.cuda(), b.cuda()
    c = poison_(torch.empty(2048, 2048, device="cuda", dtype=torch.float64))
    be_hip.L.cdf_gemm_f64(P(da), 2048, P(db), 2048, P(c), 2048, 2048, 2048, 2048, -0.5, 1.5, be_hip.stream())
    want = -0.5 * torch.matmul(a, b) + 1.5 * torch.eye(2048, dtype=torch.float64)
    err = (c.cpu() - want).abs().max().item()
    bound = 4 * 2048 * U * a.abs().max().item() * b.abs().max().item()
    print(f"gemm_f64 [hip] 2048^3: max error {err:.3g} (bound {bound:.3g})")
    assert err <= bound


def test_fid_kernels_use_no_scratch_and_the_f64_mfma():
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    if not shutil.which(hipcc):
        pytest.skip("hipcc not available")
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(repo, "cold-diffusion-models_amd", "csrc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I", csrc, "-I", os.path.join(repo, "include"),
                        "-S", os.path.join(csrc, "k_fid.hip"), "-o", "-", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    sizes = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    # the two matrix-core kernels and the merge of two accumulators, which has no MFMA
    assert len(names) == 3 and all(sum(k in n for n in names) == 1 for k in ("gemm_f64_kernel", "moments_f64_kernel", "moments_merge_f64_kernel"))
    assert sizes == [0] * 3, r.stderr[-2000:]
    bodies = re.split(r"^\s*\.globl\s+", r.stdout, flags=re.M)[1:]
    main = [b for b in bodies if "gemm_f64_kernel" in b.split(None, 1)[0] or "moments_f64_kernel" in b.split(None, 1)[0]]
    assert len(main) == 2 and all(b.count("v_mfma_f64_16x16x4_f64") >= 16 for b in main)      # 16 per K chunk, in each of the two
