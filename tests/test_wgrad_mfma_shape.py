"""The pre-split weight-gradient kernels on the 16 x 16 x 32 bf16 MFMA (csrc/k_conv_wgrad_spx.hip: cdf_wgrad_spx_mfma / cdf_wgrad_row3_mfma choose
the shape per kernel form; csrc/cdf_conv_sp.h: cdf_px_off, the swizzled pixel-major LDS image, and the fragment geometry of the transposing
read).  Both backends, small shapes; every case runs whichever shape its form is built with, so the same cases hold for a form that stays on
32 x 32 x 16.

Dense cases: test_gemm_production._wgrad_case -- float64 reference of the split planes, the K_SUM bound, poisoned outputs, two launches bit
for bit -- after cdf_conv_wgrad_bf16x_form has said that the case reaches the form it is about.

Row-of-taps forms (conv_wgrad_row3_kernel), B = 2 so that a chunk sequence crosses an image boundary:
    W = 16, H = 4   a 32-pixel chunk is two image rows: lane groups 2 and 3 read two halo rows further on (M = 128, 4 chunks)
    W = 16, H = 6   the same with 6 chunks, for the chunk counts 3 and 6
    W = 32, H = 3   a chunk is one image row, both halo columns outside the image (6 chunks)
    W = 64, H = 2   two chunks per row: one halo column inside the image (8 chunks)
    W = 128, H = 2  four chunks per row (16 chunks)
    chunks per split 1 (the prologue alone), 2, 3 (odd tail), 4, 5 / 6 / 8 (both staged register sets wrap), and a split without pixels
    channel pairs (64, 128), (128, 64), (128, 128) and ragged (72, 128), (128, 72): masked rows and the zeroed pad columns
Per-tap forms (wgrad_row3 = 0): tiles <64, 64>, <64, 128>, <128, 64>, <128, 128>, the stacked two-tap tile at 9 taps (the tenth is the all-zero
one), a 4 x 4 stride-2 convolution and a transposed one (16 taps, strided operand).

Unit impulses: one 1 in X and one in dY give exactly one weight-gradient element, equal to 1, everything else exactly 0 -- a swapped pair of
16-byte chunks, 16-channel halves or pixel blocks that a dense case could hide inside its bound's slack moves the 1 or loses it.  Positions
sit on both sides of every bit the lane map and the swizzle use: pixel of the chunk in 0-3, 4-7, 8-15, 16-31 (bits 2, 3, 4), channel in
either 16-channel half and either 8-channel chunk of a 32-channel block (bits 3, 4) and in different 32-channel blocks, all three dx taps."""
import pytest
import torch
import torch.nn.functional as F

from poison import nan_empty
from test_gemm_production import _wgrad_case, decode, wgrad_form, wgrad_plan
from test_kernels import P, _split, r4
from test_kernels_production import twice

ROW3, PER_TAP, STACK2 = 1, 2, 3

# (H, W, split counts): B = 2 throughout; chunks per split in the module docstring's order
ROW3_GEOMS = [
    (4, 16, (4, 5, 2, 1)),        # 1 | 1 + an empty split | 2 | 4
    (6, 16, (2, 1)),              # 3 | 6
    (3, 32, (6, 7, 2, 1)),        # 1 | 1 + an empty split | 3 | 6
    (2, 64, (8, 3, 1)),           # 1 | 3, 3, 2 | 8
    (2, 128, (16, 6, 5, 3)),      # 1 | 3 ... 1 | 4 + an empty split | 6, 6, 4
]
PAIRS = [(64, 128), (128, 64), (128, 128), (72, 128), (128, 72)]


def _row3_cases():
    cases = []
    for gi, (H, W, splits) in enumerate(ROW3_GEOMS):
        for si, nsplit in enumerate(splits):                 # the 128 x 128 tile in split precision at every chunk count
            cases.append((H, W, 128, 128, nsplit, (gi + si) & 1, 3))
        for pi, (CA, CB) in enumerate(PAIRS):                # every pair at every geometry, chunk counts / bsum / NS in rotation
            nsplit = splits[(gi + pi) % len(splits)]
            ns = 1 if (gi + pi) & 1 else 3
            if (CA, CB) != (128, 128) or ns == 1:
                cases.append((H, W, CA, CB, nsplit, (gi + pi + 1) & 1, ns))
        cases.append((H, W, 72, 128, splits[-1], 1, 1 if gi & 1 else 3))
    return list(dict.fromkeys(cases))


@pytest.mark.parametrize("case", _row3_cases(), ids=lambda c: "-".join(map(str, c)))
def test_row_of_taps_forms(be, case):
    H, W, CA, CB, nsplit, bsum, ns = case
    d = decode(_wgrad_case(be, ("conv_wgrad", 2, H, W, CA, CB, 3, 1, 1, nsplit, bsum, ns)))
    assert (d["form"], d["bm"], d["bn"]) == (ROW3, 64 if CA <= 64 else 128, 64 if CB <= 64 else 128), d


# (row, tuning beside wgrad_row3 = 0, (form, TA, TB))
PER_TAP_CASES = [
    (("conv_wgrad", 2, 8, 12, 64, 40, 3, 1, 1, 2, 1, 3), {}, (PER_TAP, 64, 64)),
    (("conv_wgrad", 2, 8, 12, 40, 64, 3, 1, 1, 6, 0, 1), {}, (PER_TAP, 64, 64)),
    (("conv_wgrad", 2, 8, 12, 64, 128, 3, 1, 1, 2, 1, 3), dict(wgrad_stack=0), (PER_TAP, 64, 128)),
    (("conv_wgrad", 2, 8, 12, 40, 72, 3, 1, 1, 7, 0, 1), dict(wgrad_stack=0), (PER_TAP, 64, 128)),
    (("conv_wgrad", 2, 8, 12, 128, 64, 3, 1, 1, 2, 0, 3), {}, (PER_TAP, 128, 64)),
    (("conv_wgrad", 2, 8, 12, 72, 40, 3, 1, 1, 6, 1, 1), {}, (PER_TAP, 128, 64)),
    (("conv_wgrad", 2, 8, 12, 128, 128, 3, 1, 1, 2, 1, 3), {}, (PER_TAP, 128, 128)),
    (("conv_wgrad", 2, 8, 12, 72, 136, 3, 1, 1, 1, 0, 3), {}, (PER_TAP, 128, 128)),
    (("conv_wgrad", 2, 8, 12, 136, 72, 3, 1, 1, 7, 1, 1), {}, (PER_TAP, 128, 128)),
    (("conv_wgrad", 2, 8, 12, 64, 128, 3, 1, 1, 2, 1, 3), {}, (STACK2, 128, 128)),     # 9 taps in 5 stacked pairs: the last one's second tap is zero
    (("conv_wgrad", 2, 8, 12, 40, 72, 3, 1, 1, 6, 0, 1), {}, (STACK2, 128, 128)),
    (("conv_wgrad", 2, 16, 16, 72, 128, 4, 2, 1, 2, 1, 3), {}, (PER_TAP, 128, 128)),
    (("convT_wgrad", 2, 8, 8, 128, 72, 4, 2, 1, 3, 0, 3), {}, (PER_TAP, 128, 128)),
    (("convT_wgrad", 2, 8, 8, 64, 64, 4, 2, 1, 1, 0, 1), {}, (PER_TAP, 64, 64)),
]


@pytest.mark.parametrize("row,tune,form", PER_TAP_CASES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_per_tap_forms(be, row, tune, form):
    d = decode(_wgrad_case(be, row, tune=dict(tune, wgrad_row3=0)))
    assert (d["form"], d["bm"], d["bn"]) == form, d


# ---------------------------------------------------------------------------------------------------------------------------------
# unit impulses
# ---------------------------------------------------------------------------------------------------------------------------------
def _impulse_case(be, H, W, CA, CB, ns, form, impulses, tune):
    """3 x 3 same-size weight gradient of B = 1: for each (pixel of dY, ca, cb, dy, dx) one launch with X = 1 at (pixel shifted by the tap, ca)
    and dY = 1 at (pixel, cb); dW must be 1 at [cb][ca][dy + 1][dx + 1] and exactly 0 elsewhere."""
    L = be.L
    row = ("conv_wgrad", 1, H, W, CA, CB, 3, 1, 1, 1, 0, ns)
    old = {f: be.tune.get(f) for f in tune}
    be.tune.set(**tune)
    try:
        d = decode(wgrad_form(L, row, be.tune.ptr)[0])
        assert d["form"] == form, d
        wp = wgrad_plan("conv_wgrad", H, W, 3, 1, 1)
        ldo, zero = r4(CB), be.zeros(16)
        for (pix, ca, cb, dy, dx) in impulses:
            y, x = divmod(pix, W)
            assert 0 <= y + dy < H and 0 <= x + dx < W, "the impulse's tap must stay inside the image"
            a, b = torch.zeros(1, H, W, CA), torch.zeros(1, H, W, CB)
            a[0, y + dy, x + dx, ca], b[0, y, x, cb] = 1.0, 1.0
            as_, bs_ = _split(be, be.to(a), ns == 1), _split(be, be.to(b), ns == 1)
            ws, gw = nan_empty(be, 1, 9, CA, ldo), nan_empty(be, CB, CA, 3, 3)

            def launch():
                L.cdf_conv_wgrad_bf16x(P(as_[0]), P(as_[1]), as_[0].shape[-1], P(bs_[0]), P(bs_[1]), bs_[0].shape[-1], P(zero), P(ws), ldo, 1, wp.QH,
                                       wp.QW, wp.HA, wp.WA, wp.sa, wp.HB, wp.WB, wp.sb, CA, CB, wp.ntaps, wp.desc, 1, P(None), be.tune.ptr, be.stream())
                L.cdf_unpack_reduce(P(ws), P(gw), 1, 9, CA, CB, ldo, 1, 9, CA * 9, 0, 1, be.stream())
            got = twice(launch, [gw])[0]
            want = torch.zeros(CB, CA, 3, 3)
            want[cb, ca, dy + 1, dx + 1] = 1.0
            nz = got.nonzero().tolist()
            assert torch.equal(got, want), ((pix, ca, cb, dy, dx), "nonzeros at", nz[:8], [got[tuple(i)].item() for i in nz[:8]])
    finally:
        be.tune.set(**old)


# (pixel of the chunk [+ 32: the second chunk], ca, cb, dy, dx): pixels 1 | 6 | 11 | 21, 30 and channels 3 | 12 | 19 | 28 (+ 32-channel blocks) cross
# bits 2, 3, 4 of either index; every dx with pixels and channels on both sides of bit 3 and bit 4
# (dy = -1 only from the second chunk on: the tap has to stay inside the image)
IMPULSES = [
    (1, 3, 28, 0, -1), (1, 28, 3, 1, 0), (2, 19, 12, 0, 1),
    (6, 12, 19, 0, -1), (6, 3, 3, 1, 1), (5, 28, 28, 1, 0),
    (11, 19, 3, 0, 1), (11, 44, 60, 1, -1), (13, 35, 83, 1, 0),
    (21, 12, 28, 0, -1), (21, 99, 12, 1, 1), (30, 3, 19, 0, 0), (26, 124, 115, 0, 1),
    (32 + 6, 51, 76, -1, -1), (32 + 27, 92, 44, -1, 1),
]


@pytest.mark.parametrize("W,H", [(16, 6), (32, 3)], ids=lambda v: str(v))
@pytest.mark.parametrize("ns", [3, 1], ids=lambda v: f"ns{v}")
def test_row_of_taps_unit_impulses(be, W, H, ns):
    _impulse_case(be, H, W, 128, 128, ns, ROW3, IMPULSES, {})


@pytest.mark.parametrize("CA,CB,pairs", [(64, 128, [(3, 28), (28, 3), (19, 12), (12, 19), (44, 83), (60, 124)]),
                                         (128, 64, [(28, 3), (3, 28), (12, 19), (19, 12), (83, 44), (124, 60)])], ids=lambda v: str(v))
def test_row_of_taps_unit_impulses_thin_tiles(be, CA, CB, pairs):
    imp = [(pix, ca, cb, dy, dx) for (pix, _, _, dy, dx), (ca, cb) in zip(IMPULSES[1::2], pairs)]
    _impulse_case(be, 6, 16, CA, CB, 3, ROW3, imp, {})


@pytest.mark.parametrize("ns", [3, 1], ids=lambda v: f"ns{v}")
def test_per_tap_unit_impulses(be, ns):
    _impulse_case(be, 6, 16, 128, 128, ns, PER_TAP, IMPULSES[::2], dict(wgrad_row3=0))
    imp = [(pix, ca & 63, cb, dy, dx) for (pix, ca, cb, dy, dx) in IMPULSES[1::3]]
    _impulse_case(be, 6, 16, 64, 128, ns, STACK2, imp, dict(wgrad_row3=0))
