"""`cdf_lpips_layer` and `cdf_lpips_prep_nhwc` (csrc/k_lpips.hip): the LPIPS arithmetic on the feature maps and the input scaling.
Simulator and MI355X.

Exact tests: one nonzero channel per pixel, its value +- a power of two in [2^-6, 2^3], dyadic weights and HW a power of two make every fp32
step exact -- the norm is the power of two itself, 1e-10 is absorbed by it (half an ulp of 2^-6 is 9.3e-10), the normalised value is +-1,
differences are in {0, +-1, +-2}, every sum is a short dyadic number -- so the result does not depend on any summation order and must
equal the restatement's by `==`.  The restatement is tests/lpips_ref.py's with the per-pixel steps in fp32 (exact here) and the mean over
the pixels in fp64: in fp64 all the way 1e-10 is NOT absorbed by 2^-6 (a relative 6.4e-9 per normalised value), so that evaluation is held
to the derived bound instead, here as everywhere.

Random data: |dist - fp64 restatement on the same fp32 inputs| <= 2 (C + 8) u mean_p sum_c |w_c| (|a_hat| + |b_hat|)^2, u = 2^-24, derived
in tests/lpips_ref.py (its docstring), not measured.

Every launch runs on poisoned, guarded buffers: nothing outside dist[K][B] and partial[K][B][blocks] may change, every element inside is
written, the operands stay as they were and their pitch padding is NaN.
"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import lpips_ref as R
from colddiff import _lib
from colddiff._lib import CdfError
from emu_util import P
from poison import poison_

GUARD = 64


def same(a, b):
    return torch.equal(torch.nan_to_num(a, nan=-1.25), torch.nan_to_num(b, nan=-1.25))


def padded(m, ld):
    """[B, HW, C] -> [B, HW, ld] with NaN in the pitch padding."""
    out = torch.full((m.shape[0], m.shape[1], ld), float("nan"))
    out[:, :, :m.shape[2]] = m
    return out


def launch(be, maps, w, C, dist=None, partial=None):
    """One cdf_lpips_layer of maps[0] (the originals) against maps[1:] on guarded buffers; `dist` / `partial`: the guarded buffers of an
    earlier launch (dist is accumulated into; a fresh one starts at zero).  -> (dist [K, B] on the host, dist buffer, partial buffer).
    Asserts the ownership contract."""
    K, (B, HW, ld) = len(maps) - 1, maps[0].shape
    nb = be.L.cdf_lpips_layer_blocks(HW, C)
    assert 1 <= nb <= 32
    own_d, own_p = K * B, K * B * nb
    if dist is None:
        dist = poison_(torch.empty(own_d + 2 * GUARD, device=be.device, dtype=torch.float64))
        dist[GUARD:GUARD + own_d] = 0.0
    if partial is None:
        partial = poison_(torch.empty(own_p + 2 * GUARD, device=be.device, dtype=torch.float64))
    before_p, before_d = partial.cpu().clone(), dist.cpu().clone()
    dev = [be.to(m) for m in maps]
    dw = be.to(w)
    ptrs = [P(m) for m in dev[1:]] + [0] * (4 - K)
    be.L.cdf_lpips_layer(P(dev[0]), *ptrs, K, ld, P(dw), B, HW, C, P(partial) + 8 * GUARD, P(dist) + 8 * GUARD, be.stream())
    d, p = dist.cpu(), partial.cpu()
    assert same(d[:GUARD], before_d[:GUARD]) and same(d[GUARD + own_d:], before_d[GUARD + own_d:]), "dist written outside [K][B]"
    assert same(p[:GUARD], before_p[:GUARD]) and same(p[GUARD + own_p:], before_p[GUARD + own_p:]), "partial written outside [K][B][blocks]"
    assert not torch.isnan(p[GUARD:GUARD + own_p]).any(), "a partial of this call was not written"
    assert not torch.isnan(d[GUARD:GUARD + own_d]).any(), "an element of dist is NaN: unwritten, or the pitch padding was read"
    assert all(same(t.cpu(), m) for t, m in zip(dev, maps)) and torch.equal(dw.cpu(), w), "an operand was written"
    return d[GUARD:GUARD + own_d].view(K, B).clone(), dist, partial


# ---- exact on one-hot power-of-two pixels ---------------------------------------------------------------------------------------------
def one_hot_map(B, HW, C, g, zero_rate=0.2):
    """One nonzero channel per pixel, +- 2^e with e in [-6, 3]; a fifth of the pixels all zero."""
    m = torch.zeros(B, HW, C)
    ch = torch.randint(0, C, (B, HW), generator=g)
    val = torch.pow(2.0, torch.randint(-6, 4, (B, HW), generator=g).float()) * (torch.randint(0, 2, (B, HW), generator=g) * 2 - 1).float()
    val = val * (torch.rand(B, HW, generator=g) >= zero_rate).float()
    m.scatter_(2, ch[:, :, None], val[:, :, None])
    return m


def exact_reference(a, b, w):
    """lpips_ref.layer_dist with the per-pixel steps in fp32 (exact for these data in any order) and the mean over the pixels in fp64."""
    d = R.unit(a, 2) - R.unit(b, 2)
    return ((d * d) * w.view(1, 1, -1)).sum(2).double().mean(1)


EXACT = [(4, 1, 1, 1), (20, 16, 3, 2), (64, 64, 1, 3), (68, 16, 3, 4), (192, 64, 3, 2), (256, 16, 1, 4), (384, 64, 3, 3), (512, 16, 3, 4),
         (64, 1024, 1, 2)]                                                    # the last: two passes of a block's pixel loop


@pytest.mark.parametrize("C,HW,B,K", EXACT)
def test_exact_on_one_hot_power_of_two_pixels(be, C, HW, B, K):
    g = torch.Generator().manual_seed(1000 * C + HW + K)
    a = one_hot_map(B, HW, C, g)
    cands = [one_hot_map(B, HW, C, g) for _ in range(K)]
    cands[-1][:, ::2] = a[:, ::2]                                              # every other pixel equal to the original's: adds 0
    w = torch.randint(0, 9, (C,), generator=g).float() / 64
    got, _, _ = launch(be, [padded(m, C + 4) for m in [a] + cands], w, C)
    for k in range(K):
        want = exact_reference(a, cands[k], w)
        assert torch.equal(got[k], want), (k, got[k], want)
        assert (R.layer_dist(a.double(), cands[k].double(), w.double()) - got[k]).abs().le(R.layer_bound(a, cands[k], w)).all()
    assert HW == 1 or (got > 0).any(), "the case has no nonzero distance"


def test_equal_maps_give_exactly_zero_also_on_random_data(be):
    g = torch.Generator().manual_seed(3)
    a = torch.randn(3, 49, 68, generator=g)
    got, _, _ = launch(be, [padded(a, 72)] * 4, torch.rand(68, generator=g), 68)
    assert torch.equal(got, torch.zeros(3, 3, dtype=torch.float64))


def test_zero_pixels_by_hand(be):
    """HW = 4, C = 8.  Pixel 0: zero on both sides, adds 0.  Pixel 1: the original zero, the candidate 2^-3 at channel 3: adds w_3 b_hat_3^2 =
    w_3.  Pixel 2: the candidate zero, the original -4 at channel 5: adds w_5.  Pixel 3: +2 against -2^-6 at channel 6: adds 4 w_6."""
    a, b = torch.zeros(1, 4, 8), torch.zeros(1, 4, 8)
    b[0, 1, 3] = 0.125
    a[0, 2, 5] = -4.0
    a[0, 3, 6], b[0, 3, 6] = 2.0, -2.0 ** -6
    w = torch.tensor([0.5, 0.5, 0.5, 0.25, 0.5, 0.75, 0.125, 0.5])
    got, _, _ = launch(be, [padded(a, 12), padded(b, 12)], w, 8)
    assert got.item() == (0.25 + 0.75 + 4 * 0.125) / 4


# ---- shapes, random data, the derived bound -------------------------------------------------------------------------------------------
CS = (4, 20, 64, 68, 192, 256, 384, 512)
HWS = (1, 9, 49, 225, 961)
_cases = {}


def random_case(C, HW, B):
    """Four candidate maps, the fp64 restatement and the bound of each against the originals; made once per shape."""
    key = (C, HW, B)
    if key not in _cases:
        g = torch.Generator().manual_seed(7 * C + HW + B)
        maps = [torch.relu(torch.randn(B, HW, C, generator=g) + 0.3) * (0.5 + k) for k in range(5)]     # post-ReLU: non-negative, a third zeros
        w = torch.rand(C, generator=g) * (2.0 / C)
        ref = [R.layer_dist(maps[0].double(), m.double(), w.double()) for m in maps[1:]]
        bnd = [R.layer_bound(maps[0], m, w) for m in maps[1:]]
        _cases[key] = (maps, w, ref, bnd)
    return _cases[key]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("HW", HWS)
@pytest.mark.parametrize("C", CS)
def test_every_shape_within_the_derived_bound_and_accumulated_over_two_launches(be, C, HW, B):
    K = 1 + (CS.index(C) + HWS.index(HW) + B) % 4                              # one to four candidates, every count at every C
    ld = C + (4 if (HWS.index(HW) + B) % 2 else 8)
    maps, w, ref, bnd = random_case(C, HW, B)
    ops = [padded(m, ld) for m in maps[:K + 1]]
    one, dist, partial = launch(be, ops, w, C)
    two, _, _ = launch(be, ops, w, C, dist=dist, partial=partial)
    worst = 0.0
    for k in range(K):
        err = (one[k] - ref[k]).abs()
        worst = max(worst, float((err / bnd[k]).max()))
        assert (err <= bnd[k]).all(), (k, err, bnd[k])
        assert torch.equal(two[k], one[k] + one[k]), "the second launch did not add to dist"
        assert (ref[k] > 1e3 * bnd[k]).all(), "the case does not resolve its own distance"
    print(f"lpips_layer [{be.kind}] C={C} HW={HW} B={B} K={K} ld={ld}: largest error / bound {worst:.3g}")


def test_the_bound_is_not_vacuous():
    """torch's own fp32 evaluation, and the same with the channels reversed (another summation order), stay inside the bound; a relative
    perturbation of 1e-3 does not."""
    maps, w, ref, bnd = random_case(384, 49, 3)
    for flip in (False, True):
        ms = [m.flip(2) if flip else m for m in maps]
        ww = w.flip(0) if flip else w
        for k in range(4):
            assert ((R.layer_dist(ms[0], ms[k + 1], ww).double() - ref[k]).abs() <= bnd[k]).all()
    assert all((1e-3 * ref[k] > bnd[k]).all() for k in range(4))


# ---- contract ------------------------------------------------------------------------------------------------------------------------------
def test_two_runs_are_bit_identical_and_a_stale_scratch_is_harmless(be):
    maps, w, ref, bnd = random_case(192, 225, 3)
    ops = [padded(m, 196) for m in maps]
    first, _, partial = launch(be, ops, w, 192)
    second, _, _ = launch(be, ops, w, 192)
    assert torch.equal(first, second), "two runs differ"
    # the scratch of the larger call, still full of its partials, under a smaller one: fewer images, fewer candidates
    small = [m[:1, :49].contiguous() for m in ops[:3]]
    got, _, _ = launch(be, small, w, 192, partial=partial)
    fresh, _, _ = launch(be, small, w, 192)
    assert torch.equal(got, fresh)


def check_argument_errors(L, p, st):
    """Every host-side check: a status and a text, no launch (the pointers are not device memory on the device build)."""
    names = ("a", "c0", "c1", "c2", "c3", "K", "ld", "w", "B", "HW", "C", "partial", "dist", "stream")
    good = [p, p, p, p, p, 4, 64, p, 2, 9, 64, p, p, st]

    def bad(**kw):
        args = list(good)
        for k, v in kw.items():
            args[names.index(k)] = v
        return args

    for kw, text in ((dict(C=6, ld=8), r"C must be a multiple of 4 in \[4, 512\] \(got 6\)"), (dict(C=516, ld=516), r"\(got 516\)"),
                     (dict(C=0), r"\(got 0\)"), (dict(ld=66), r"ld must be a multiple of 4, at least C \(got ld = 66, C = 64\)"),
                     (dict(ld=60), "at least C"), (dict(K=0), r"K must be 1\.\.\.4"), (dict(K=5), r"K must be 1\.\.\.4"),
                     (dict(c3=0), r"candidate 3 of 4"), (dict(c1=p + 4), r"candidate 1 of 4"), (dict(a=0), "null pointer"),
                     (dict(w=0), "null pointer"), (dict(partial=0), "null pointer"), (dict(dist=0), "null pointer"),
                     (dict(a=p + 4), "16B aligned"), (dict(B=0), "B must be in"), (dict(B=65536), "B must be in"), (dict(HW=0), "HW at least 1")):
        with pytest.raises(CdfError, match=text):
            L.cdf_lpips_layer(*bad(**kw))
    assert L._dll.cdf_lpips_layer(*bad(C=6, ld=8)) == -1
    for kw, text in ((dict(x=0), "null pointer"), (dict(y=0), "null pointer"), (dict(ldy=6), "ldy"), (dict(ldy=0), "ldy"), (dict(B=0), "at least 1"),
                     (dict(H=0), "at least 1"), (dict(y=p + 4), "16B aligned")):
        args = dict(x=p, y=p, ldy=4, B=1, H=2, W=2, from01=0, stream=st)
        args.update(kw)
        with pytest.raises(CdfError, match=text):
            L.cdf_lpips_prep_nhwc(*args.values())
    # the block count: a pure function of the shape, 0 for what the entry point refuses, the pixel groups of a block otherwise, at most 32
    q = L.cdf_lpips_layer_blocks
    assert [q(9, 6), q(9, 516), q(0, 64), q(9, 0)] == [0, 0, 0, 0]
    assert [q(1, 4), q(257, 4), q(961, 64), q(49, 384), q(49, 512), q(9, 20), q(10 ** 6, 256)] == [1, 2, 32, 13, 13, 1, 32]


def test_bad_arguments_are_a_status(be):
    buf = torch.zeros(64, device=be.device, dtype=torch.float64)
    check_argument_errors(be.L, P(buf), be.stream())


def test_bad_arguments_are_a_status_on_the_device_build_without_a_gpu():
    buf = torch.zeros(64, dtype=torch.float64)
    check_argument_errors(_lib.Lib(_lib.LIB_PATH), buf.data_ptr(), 0)


def test_lpips_kernels_use_no_scratch():
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    if not shutil.which(hipcc):
        pytest.skip("hipcc not available")
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(repo, "cold-diffusion-models_amd", "csrc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I", csrc, "-I", os.path.join(repo, "include"),
                        "-S", os.path.join(csrc, "k_lpips.hip"), "-o", "-", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    sizes = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    vgprs = [int(v) for v in re.findall(r" VGPRs: (\d+)", r.stderr)]
    # the layer kernel with one and two float4 per lane for one to four candidates (a pixel's vectors spilled to scratch is how it would
    # go quietly wrong), the fold, the input scaling
    assert len(names) == 10 and sum("lpips_layer_kernel" in n for n in names) == 8
    assert sizes == [0] * 10 and max(vgprs) <= 128, r.stderr[-3000:]
    bodies = re.split(r"^\s*\.globl\s+", r.stdout, flags=re.M)[1:]
    layer = [b for b in bodies if "lpips_layer_kernel" in b.split(None, 1)[0]]
    # 16-byte loads only: NV (1 + K) of the maps and NV of the weights per kernel; no dword load (a load split behind per-lane branches)
    assert len(layer) == 8 and all(len(re.findall(r"global_load_dword\s", b)) == 0 for b in layer)
    assert sorted(len(re.findall(r"global_load_dwordx4\s", b)) for b in layer) == sorted(nv * (2 + k) for nv in (1, 2) for k in (1, 2, 3, 4))


# ---- cdf_lpips_prep_nhwc ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("from01", [0, 1])
@pytest.mark.parametrize("B,H,W,ld", [(1, 5, 7, 4), (3, 33, 31, 8), (2, 64, 64, 4)])
def test_prep_scales_every_channel_and_zeroes_the_pad_channel(be, B, H, W, ld, from01):
    g = torch.Generator().manual_seed(B * H + W + from01)
    x = torch.rand(B, 3, H, W, generator=g) if from01 else torch.rand(B, 3, H, W, generator=g) * 2 - 1
    n = B * H * W * ld
    out = poison_(torch.empty(n + 2 * GUARD, device=be.device, dtype=torch.float32))
    dx = be.to(x)
    be.L.cdf_lpips_prep_nhwc(P(dx), P(out) + 4 * GUARD, ld, B, H, W, from01, be.stream())
    o = out.cpu()
    assert torch.isnan(o[:GUARD]).all() and torch.isnan(o[GUARD + n:]).all(), "written outside the map"
    assert torch.equal(dx.cpu(), x), "the operand was written"
    y = o[GUARD:GUARD + n].view(B, H, W, ld)
    assert torch.equal(y[..., 3], torch.zeros(B, H, W)), "the pad channel is not zero"
    assert torch.isnan(y[..., 4:]).all(), "channels past the pad channel were written"
    want = R.scale_input(x, bool(from01)).permute(0, 2, 3, 1)
    ulp = torch.from_numpy(np.spacing(np.abs(want.numpy())))
    assert ((y[..., :3] - want).abs() <= 2 * ulp).all()
    exact = R.scale_input(x.double(), bool(from01)).permute(0, 2, 3, 1)
    assert (y[..., :3].double() - exact).abs().max() < 1e-6
