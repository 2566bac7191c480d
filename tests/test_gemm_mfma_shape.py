"""The 16 x 16 x 32 bf16 MFMA form of the pre-split GEMM K loops (csrc/cdf_conv_sp.h: CDF_MFMA16_BF16, cdf_mma_tile on f32x4q_t accumulators,
cdf_swz<16>, the MF = 16 fragment readers; csrc/cdf_common.h: the f32x4q_t staging) -- the LDS-resident-input (halo) kernel runs on it in
every W / BN / BM / NS instance (csrc/k_conv_halo.hip: cdf_halo_mfma).  Both backends, small shapes.

The product itself: cdf_mfma_bf16_16x16x32 issues one product through the lane maps the K loops use (A lane l: row l & 15, k = 8 (l >> 4) + j;
B likewise with column l & 15; C register r: row 4 (l >> 4) + r, column l & 15) against a float64 matmul of the same bf16 values.  A wrong
map of either operand or of the result moves whole rows / K blocks and shows as an O(1) error.  Bound: bf16 products are exact in fp32, so
only the 33 fp32 additions per output round -- 33 2^-24 sum |terms|, whatever their order.

The halo kernel: through cdf_conv_gemm_bf16x_io after cdf_conv_gemm_bf16x_form has said that the halo form, tile height and N tile are the
ones the case is about; reference, bounds and conventions are test_gemm_production._gemm_case's (float64 convolution of the split planes,
K_SUM model, poisoned outputs, two launches bit for bit).  Shapes, the smallest that reach each hazard:
    tile height and batch   W = 16, H = 16, B = 2: TH = 8 (BM 128) or 16 (BM 256), an image boundary between tiles
    chunk count             Cin = 64 (two 32-channel chunks: both halo buffers) and 96 (three: the double buffer and the weight stages wrap).
                            Cin = 32 is not a case: the dispatcher hands the halo kernel layers of Cin >= 64 only (k_conv_spx.hip)
    output width, epilogue  Cout = 64 and 128 (BN 64 / 128; 128 at this size needs small_n64 = 0), Cout = 72 (ragged N, generic epilogue)
    wider images            W = 32, 64 and 128 with H so that M = 256: a wave's fragment rows cross image rows of the halo
    NS = 3 and 1;  epilogues: plain | bias + pre-activation + GELU with bf16 planes out | bias + residual
"""
import math

import pytest
import torch

from poison import nan_empty
from test_gemm_production import HALO, _gemm_case, decode
from test_kernels import P
from test_kernels_production import U, twice


def test_mfma_16x16x32_product_and_lane_maps(be):
    g = torch.Generator().manual_seed(1632)
    a, bt, c0 = torch.randn(16, 32, generator=g).bfloat16(), torch.randn(16, 32, generator=g).bfloat16(), torch.randn(16, 16, generator=g)
    ad, bd = be.to(a.view(torch.int16)), be.to(bt.view(torch.int16))
    c0d, c = be.to(c0), nan_empty(be, 16, 16)

    def launch():
        c.copy_(c0d)                                         # (the accumulator is an input)
        be.L.cdf_mfma_bf16_16x16x32(P(ad), P(bd), P(c), be.stream())
    got = twice(launch, [c])[0]
    ref = c0.double() + a.double() @ bt.double().t()
    bound = 33 * U * (c0.double().abs() + a.double().abs() @ bt.double().abs().t()).max().item()
    err = (got.double() - ref).abs().max().item()
    print(f"cdf_mfma_bf16_16x16x32 [{be.kind}]: worst error {err:.3e} / bound {bound:.3e} = {err / bound:.3f}")
    assert math.isfinite(err) and err <= bound
    # every operand element reaches exactly its output row / column: a unit at A[i][k] and at Bt[n][k] gives C[i][n] = 1 and nothing else
    for (i, n, k) in ((0, 0, 0), (5, 9, 7), (15, 3, 8), (9, 15, 17), (12, 4, 31)):
        ua, ub = torch.zeros(16, 32), torch.zeros(16, 32)
        ua[i, k], ub[n, k] = 1.0, 1.0
        uad, ubd = be.to(ua.bfloat16().view(torch.int16)), be.to(ub.bfloat16().view(torch.int16))
        cz = be.zeros(16, 16)
        be.L.cdf_mfma_bf16_16x16x32(P(uad), P(ubd), P(cz), be.stream())
        want = torch.zeros(16, 16)
        want[i, n] = 1.0
        assert torch.equal(cz.cpu(), want), (i, n, k)


PLAIN, BIAS_PRE_GELU_PLANES, BIAS_RES = "plain", "bp-gelu-planes", "br"


def _row(B, H, W, Cin, Cout, epi, ns):
    # (entry, kind, B, H, W, Cin, Cout, k, s, pad, nphase, operands, act, mul_mode, accumulate, io_bf16, planes, y, ws, NS)
    ops, act, planes = {PLAIN: ("", 0, 0), BIAS_PRE_GELU_PLANES: ("bp", 1, 2 if ns == 3 else 1), BIAS_RES: ("br", 0, 0)}[epi]
    return ("gemm", "conv_fwd", B, H, W, Cin, Cout, 3, 1, 1, 1, ops, act, 0, 0, 0, planes, 1, 0, ns)


# (B, H, W, Cin, Cout, BM, BN, epilogue)
HALO_CASES = [
    (2, 16, 16, 64, 64, 128, 64, PLAIN),
    (2, 16, 16, 64, 64, 256, 64, BIAS_RES),
    (2, 16, 16, 64, 128, 256, 128, BIAS_PRE_GELU_PLANES),
    (2, 16, 16, 96, 128, 128, 128, PLAIN),
    (2, 16, 16, 96, 72, 128, 128, BIAS_RES),
    (2, 16, 16, 64, 72, 256, 128, BIAS_PRE_GELU_PLANES),
    (1, 8, 32, 64, 128, 256, 128, BIAS_PRE_GELU_PLANES),
    (1, 8, 32, 96, 64, 128, 64, BIAS_RES),
    (1, 4, 64, 64, 128, 256, 128, PLAIN),
    (1, 4, 64, 96, 72, 128, 128, BIAS_PRE_GELU_PLANES),
    (1, 4, 64, 64, 64, 256, 64, BIAS_RES),
    (1, 4, 64, 96, 64, 128, 64, PLAIN),
    (1, 2, 128, 64, 64, 256, 64, PLAIN),
    (1, 2, 128, 64, 128, 128, 128, BIAS_RES),
]
# NS = 1 at W = 64 with the 128-wide N tile stays on the 32 x 32 x 16 product (cdf_halo_mfma): no case here
HALO_PARAMS = [(c, ns) for c in HALO_CASES for ns in (3, 1) if not (ns == 1 and c[2] == 64 and c[6] == 128)]


@pytest.mark.parametrize("case,ns", HALO_PARAMS, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else f"ns{v}")
def test_halo_kernel_on_the_16x16x32_product(be, case, ns):
    B, H, W, Cin, Cout, bm, bn, epi = case
    # halo bit 16: the 128-wide N tile at 128-pixel width; small_n64 = 0: Cout = 128 keeps its 128-wide tile on a grid this small
    tune = dict(halo=63, halo_bm=bm, small_n64=0)
    d = decode(_gemm_case(be, _row(B, H, W, Cin, Cout, epi, ns), tune=tune))     # (_gemm_case asks cdf_conv_gemm_bf16x_form before it launches)
    assert (d["form"], d["bm"], d["bn"], d["w"]) == (HALO, bm, bn, W), d
